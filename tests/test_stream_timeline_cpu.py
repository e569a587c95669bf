"""The streaming anomaly timeline on the CPU (include/krca.h: krca_stream_timeline):

* tests/stream_timeline_ref.py, the restatement the GPU tests compare the kernel with, against the
  batch restatement tests/timeline_ref.py (a horizon larger than the stream: equal after every
  window) and against itself over other partitions of the same steps;
* the fixtures really carry episodes across window ends and really expire episodes, so a GPU pass
  cannot be one that never crossed a boundary or never expired anything;
* StreamingRCA(timeline=True) -- windows, snapshots, first_movers' refusals -- over a NumPy shard.
"""
import numpy as np
import pytest

import stream_timeline_ref as SR
import timeline_ref as R
from numpy_shard import NumpyShard

CASE_IDS = ["P37-M8-W10-H33", "P33-M1-W7-H5", "P9-M64-W10-H1000", "P70-M4-W60-H40"]
_batch = {}


def batch_prefixes(case):
    """timeline_ref.timeline over the prefix at every window end of the case (computed once)."""
    if case[:5] not in _batch:
        P, M, W, H, seed, wins = case
        x, _ = SR.case_data(case)
        _batch[case[:5]] = [R.timeline(x[:t], W, SR.THR, SR.GAP, SR.MINC) for t in np.cumsum(wins)]
    return _batch[case[:5]]


@pytest.mark.parametrize("case", SR.CASES, ids=CASE_IDS)
def test_large_horizon_equals_batch_timeline(case):
    """H = 10**9: nothing expires, so after every window the six outputs are the batch timeline's
    over the series so far."""
    P, M, W, H, seed, wins = case
    x, _ = SR.case_data(case)
    got = SR.stream_timeline(x, W, SR.THR, SR.GAP, SR.MINC, 10**9, wins)
    for i, (g, b) in enumerate(zip(got, batch_prefixes(case))):
        assert SR.differing(g, b) == [], (i, SR.differing(g, b))


@pytest.mark.parametrize("case", SR.CASES, ids=CASE_IDS)
def test_partition_independence(case):
    """At the case's H: the case's list, [1] * T and [T] agree (outputs and series state) at every
    common window end."""
    P, M, W, H, seed, wins = case
    x, _ = SR.case_data(case)
    T = sum(wins)
    run = lambda w: SR.stream_timeline(x, W, SR.THR, SR.GAP, SR.MINC, H, w, with_state=True)  # noqa: E731
    a, ones, whole = run(wins), run([1] * T), run([T])
    keys = SR.KEYS + SR.SeriesState.FIELDS
    for i, t in enumerate(np.cumsum(wins)):
        assert SR.differing(a[i], ones[t - 1], keys) == [], (i, t)
    assert SR.differing(a[-1], whole[0], keys) == []


def continuations(x, W, wins):
    """Pairs of consecutive exceedances of a series at most GAP apart with a window end between them."""
    T, P, M = x.shape
    ex, _ = R.rolling_exceed(x.reshape(T, P * M), W, SR.THR)
    ends = np.cumsum(wins)[:-1]  # a call ends after step e - 1
    n = 0
    for s in range(P * M):
        steps = np.flatnonzero(ex[:, s])
        for t1, t2 in zip(steps[:-1], steps[1:]):
            if t2 - t1 <= SR.GAP and ((ends > t1) & (ends <= t2)).any():
                n += 1
    return n


@pytest.mark.parametrize("case", SR.CASES, ids=CASE_IDS)
def test_fixture_conditions(case):
    """Episodes continue across a window end in every case; with a small H some (pod, window end)
    differs from the batch timeline of the prefix, and in cases 1 and 4 some differing pod still
    reports an episode (the kept one expired and a weaker one took its place)."""
    P, M, W, H, seed, wins = case
    x, ref = SR.case_data(case)
    cont = continuations(x, W, wins)
    differ = still = 0
    for g, b in zip(ref, batch_prefixes(case)):
        d = np.zeros(P, bool)
        for k in SR.KEYS:
            d |= g[k] != b[k]
        differ += int(d.sum())
        still += int((d & (g["onset"] >= 0)).sum())
    print(f"case {case[:5]}: continuations {cont}, pod-windows differing {differ}, still reporting {still}")
    assert cont >= 1
    if H < sum(wins):
        assert differ >= 1
    else:
        assert differ == 0
    if case in (SR.CASES[0], SR.CASES[3]):
        assert still >= 1


# ---- StreamingRCA(timeline=True) over a NumPy shard ------------------------------------------
class TimelineShard(NumpyShard):
    """NumpyShard + stream_timeline: the reference over the kept history (the outputs at a step do
    not depend on the partition, so one call over the whole history states them)."""

    def stream_timeline(self, x_new, t0, horizon, gap, min_count):
        out = dict(self.stream_score(x_new, t0, horizon))
        tl = SR.stream_timeline(self._hist, self.cfg.window, self.cfg.z_threshold, gap, min_count, horizon,
                                [len(self._hist)], with_state=True)[0]
        out.update({k: tl[k] for k in SR.KEYS})
        self._episodes = np.stack([tl[f].astype(np.float32).view(np.int32) if f.endswith("peak")
                                   else tl[f].astype(np.int32) for f in SR.SeriesState.FIELDS])
        self.score_out = out
        return out

    def state_dict(self, M, horizon):
        st = super().state_dict(M, horizon)
        if getattr(self, "_episodes", None) is not None:
            st["episode_state"] = self._episodes
        return st

    def load_state_dict(self, st, M, horizon):
        super().load_state_dict(st, M, horizon)
        if "episode_state" in st:  # the history restates it; kept to check the round trip
            self._episodes = np.asarray(st["episode_state"], np.int32)


NP, NM, NW, NH = 256, 4, 10, 25
WINDOWS = [NW + 15, 5, 1, 20, 9, 30]


def _mesh():
    import timeline_cases as C
    from krca import synth
    m = synth.make_graph(NP, avg_degree=8, seed=5)
    return m, C.dyadic_metrics(NP, NM, sum(WINDOWS), NW, seed=6)


def _stream(m, world=1, cls=TimelineShard, **kw):
    from krca.rca import Comm, Config, shard_graph, shard_range
    from krca.stream import StreamingRCA
    cfg = Config(window=NW)
    lo, hi, n_max = shard_range(NP, world, 0)
    rp, col, od = shard_graph(m.row_ptr, m.col, m.outdeg, lo, hi)
    sh = cls(np.zeros((0, hi - lo, NM), np.float32), rp, col, od, NP, n_max, world, cfg)
    return StreamingRCA(None, m.row_ptr, m.col, m.outdeg, NM, cfg, horizon=NH, tol=1e-9, max_iter=60,
                        comm=Comm(world, 0), shard=sh, **kw)


def _row(out, s):
    sc = out["scores"]
    return {k: np.array(sc[k]) for k in sc}, [int(i) for i in out["top"][0]], out["iters"]


def test_streaming_rca_timeline_snapshot_round_trip(tmp_path):
    """A timeline stream snapshotted after window 3 and restored into a fresh object continues
    identically: scores, the six timeline tensors, top-k, iteration counts."""
    m, x = _mesh()
    ends = np.cumsum(WINDOWS)

    def run(snap_at):
        s = _stream(m, timeline=True, gap=SR.GAP, min_count=SR.MINC)
        rows, t = [], 0
        for i, d in enumerate(WINDOWS):
            out = s.window(x[t:t + d])
            t += d
            assert set(SR.KEYS) <= set(out["scores"]) and "score" in out["scores"]
            rows.append(_row(out, s))
            if i == snap_at:
                path = str(tmp_path / "tl.npz")
                s.snapshot(path)
                with np.load(path) as z:
                    assert "episode_state" in z.files
                s = _stream(m, timeline=True, gap=SR.GAP, min_count=SR.MINC)
                s.restore(path)
                assert s.t == t
        return rows
    a, b = run(None), run(2)
    ref = SR.stream_timeline(x, NW, 3.0, SR.GAP, SR.MINC, NH, WINDOWS)
    for i in range(len(WINDOWS)):
        assert SR.differing(a[i][0], b[i][0], tuple(a[i][0])) == [], i
        assert a[i][1:] == b[i][1:], i
        assert SR.differing(a[i][0], ref[i]) == [], (i, ends[i])
    assert any((r["onset"] >= 0).any() for r in ref)


def test_restore_across_timeline_on_and_off_raises(tmp_path):
    m, x = _mesh()
    on = _stream(m, timeline=True, gap=SR.GAP, min_count=SR.MINC)
    off = _stream(m)
    on.window(x[:NW + 15])
    off.window(x[:NW + 15])
    p_on, p_off = str(tmp_path / "on.npz"), str(tmp_path / "off.npz")
    on.snapshot(p_on)
    off.snapshot(p_off)
    with pytest.raises(ValueError, match="timeline"):
        _stream(m).restore(p_on)
    with pytest.raises(ValueError, match="timeline"):
        _stream(m, timeline=True, gap=SR.GAP, min_count=SR.MINC).restore(p_off)
    with pytest.raises(ValueError, match="gap"):
        _stream(m, timeline=True, gap=SR.GAP + 1, min_count=SR.MINC).restore(p_on)
    with pytest.raises(ValueError, match="min_count"):
        _stream(m, timeline=True, gap=SR.GAP, min_count=SR.MINC + 1).restore(p_on)
    _stream(m, timeline=True, gap=SR.GAP, min_count=SR.MINC).restore(p_on)
    _stream(m).restore(p_off)


def test_default_stream_writes_todays_snapshot_keys(tmp_path):
    """A stream without the timeline: the arrays and the meta keys a snapshot held before the
    timeline existed, nothing more; its scores hold the four scoring outputs only."""
    import json
    m, x = _mesh()
    s = _stream(m, cls=NumpyShard)
    out = s.window(x[:NW + 15])
    assert set(out["scores"]) == {"z_last", "score", "n_exceed", "flags"}
    path = str(tmp_path / "plain.npz")
    s.snapshot(path)
    with np.load(path) as z:
        assert set(z.files) == {"meta", "hist", "r"}
        meta = json.loads(bytes(z["meta"]).decode())
    assert set(meta) == {"version", "shard", "N", "M", "H", "lo", "hi", "n_max", "world", "rank", "cfg", "tol", "t",
                         "solved", "last_iters"}
    from krca.rca import DeviceShard
    assert hasattr(DeviceShard, "stream_timeline")


def test_first_movers_refusals():
    m, x = _mesh()
    with pytest.raises(ValueError, match="world"):
        _stream(m, world=2, timeline=True).first_movers()
    with pytest.raises(ValueError, match="no window"):
        _stream(m, timeline=True).first_movers()
    with pytest.raises(ValueError, match="timeline"):
        _stream(m).first_movers()


def test_timeline_window_bytes_model():
    from krca.stream import timeline_window_bytes, window_bytes
    for P, M, d in ((1_000_000, 8, 1), (37, 8, 5), (9, 64, 1)):
        assert timeline_window_bytes(P, M, d) == window_bytes(P, M, d) + 32 * P * M + 18 * P


def test_abi_exports_and_argument_checks():
    """The two exports exist; the argument checks run before any device work (no GPU here)."""
    from krca import native
    lib = native.load_library()
    assert lib.krca_stream_episode_state_size(10, 8) >= 10 * 8 * 32
    assert lib.krca_stream_episode_state_size(0, 8) == 0
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(gap=3, minc=3, t0=0, delta=1, ep=p, P=1):
        return lib.krca_stream_timeline(p, P, 8, delta, t0, 10, 33, 3.0, gap, minc, p, ep, p, p, p, p, p, p, p, p,
                                        p, p, None)
    assert call(gap=-1) < 0 and b"gap" in lib.krca_last_error()
    assert call(minc=0) < 0 and b"min_count" in lib.krca_last_error()
    assert call(t0=2**31 - 1, delta=1) < 0 and b"INT32_MAX" in lib.krca_last_error()
    assert call(ep=None) < 0 and b"null" in lib.krca_last_error()
    assert call(P=0, ep=None) == 0
