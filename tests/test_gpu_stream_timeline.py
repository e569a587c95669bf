"""krca_stream_timeline on the device against tests/stream_timeline_ref.py (bit-exact: the fixtures
are dyadic, see tests/timeline_ref.py): the six timeline outputs after every window, the scoring
outputs and the rolling state against a parallel krca_stream_score stream, the batch timeline at a
large horizon, other partitions of the same steps, poisoned states, argument errors, and
StreamingRCA(timeline=True) end to end with first movers and a snapshot."""
import numpy as np
import pytest
import torch

import stream_timeline_ref as SR
import timeline_ref as R
from guarded import GuardedEngine, run_poisons, same_bytes
from krca import native, synth
from krca.rca import Config
from krca.stream import StreamingRCA

pytestmark = pytest.mark.gpu

SIX = SR.KEYS
FOUR = ("z_last", "score", "n_exceed", "flags")
CASE_IDS = ["P37-M8-W10-H33", "P33-M1-W7-H5", "P9-M64-W10-H1000", "P70-M4-W60-H40"]


@pytest.fixture(scope="module")
def eng():
    return GuardedEngine()


def host(t):
    return t.cpu().numpy().copy()


def new_outputs(e, P, M, six):
    t = e.torch
    o = dict(z_last=t.empty((P, M), dtype=t.float32, device=e.device), score=t.empty(P, dtype=t.float32, device=e.device),
             n_exceed=t.empty(P, dtype=t.int32, device=e.device), flags=t.empty(P, dtype=t.uint8, device=e.device))
    if six:
        dt = dict(onset=t.int32, last=t.int32, count=t.int32, peak=t.float32, lead=t.int8, n_metrics=t.uint8)
        o.update({k: t.empty(P, dtype=dt[k], device=e.device) for k in SIX})
    return o


def call_timeline(e, xd, P, M, d, t0, W, H, state, ep_state, o, gap=SR.GAP, minc=SR.MINC):
    return e.lib.krca_stream_timeline(e.ptr(xd), P, M, d, t0, W, H, SR.THR, gap, minc, e.ptr(state),
                                      ep_state if ep_state is None else e.ptr(ep_state), e.ptr(o["z_last"]),
                                      e.ptr(o["score"]), e.ptr(o["n_exceed"]), e.ptr(o["flags"]), e.ptr(o["onset"]),
                                      e.ptr(o["last"]), e.ptr(o["count"]), e.ptr(o["peak"]), e.ptr(o["lead"]),
                                      e.ptr(o["n_metrics"]), e._stream())


def state_parts(st, S, W, H, t0):
    """The defined bytes of the rolling state after t0 steps: sums and counts, the ring rows written
    so far, the exceedance bits."""
    ring0, bits0 = 20 * S, 20 * S + 4 * W * S
    return dict(sums=st[:ring0], ring=st[ring0:ring0 + 4 * S * min(t0, W)],
                bits=st[bits0:bits0 + 4 * ((H + 31) // 32) * S])


def run_timeline(e, x, W, H, wins, with_state=False):
    """One krca_stream_timeline stream over x in calls of `wins` steps -> per window a dict of host
    arrays (ten outputs; with_state: the rolling state's defined parts and the episode state)."""
    T, P, M = x.shape
    t = e.torch
    state = t.empty(int(e.lib.krca_stream_state_size(P, M, W, H)), dtype=t.uint8, device=e.device)
    ep_state = t.empty(int(e.lib.krca_stream_episode_state_size(P, M)), dtype=t.uint8, device=e.device)
    xd = e._dev(np.array(x))  # a writable copy of the shared fixture
    rows, t0 = [], 0
    for d in wins:
        o = new_outputs(e, P, M, True)
        native._check(call_timeline(e, xd[t0:t0 + d], P, M, d, t0, W, H, state, ep_state, o), "krca_stream_timeline")
        t0 += d
        row = {k: host(v) for k, v in o.items()}
        if with_state:
            row.update(state_parts(host(state), P * M, W, H, t0), episodes=host(ep_state))
        rows.append(row)
    return rows


def run_score(e, x, W, H, wins):
    T, P, M = x.shape
    t = e.torch
    state = t.empty(int(e.lib.krca_stream_state_size(P, M, W, H)), dtype=t.uint8, device=e.device)
    xd = e._dev(np.array(x))  # a writable copy of the shared fixture
    rows, t0 = [], 0
    for d in wins:
        o = new_outputs(e, P, M, False)
        native._check(e.lib.krca_stream_score(e.ptr(xd[t0:t0 + d]), P, M, d, t0, W, H, SR.THR, e.ptr(state),
                                              e.ptr(o["z_last"]), e.ptr(o["score"]), e.ptr(o["n_exceed"]),
                                              e.ptr(o["flags"]), e._stream()), "krca_stream_score")
        t0 += d
        row = {k: host(v) for k, v in o.items()}
        row.update(state_parts(host(state), P * M, W, H, t0))
        rows.append(row)
    return rows


def assert_six(got, ref, where):
    for k in SIX:
        assert same_bytes(got[k], ref[k]), (k, where)


# ---- 1. the call against the reference and against a parallel krca_stream_score stream ----------
@pytest.mark.parametrize("case", SR.CASES, ids=CASE_IDS)
def test_stream_timeline_matches_reference_and_stream_score(eng, case):
    P, M, W, H, seed, wins = case
    x, ref = SR.case_data(case)
    got = run_timeline(eng, x, W, H, wins, with_state=True)
    sc = run_score(eng, x, W, H, wins)
    for i in range(len(wins)):
        assert_six(got[i], ref[i], i)
        for k in FOUR + ("sums", "ring", "bits"):
            assert same_bytes(got[i][k], sc[i][k]), (k, i)
    assert any((r["onset"] >= 0).any() for r in ref)


# ---- 2. a horizon larger than the stream: the batch timeline over the series so far ---------------
def test_large_horizon_equals_rolling_timeline(eng):
    case = SR.CASES[2]
    P, M, W, H, seed, wins = case
    assert H > sum(wins)
    x, _ = SR.case_data(case)
    got = run_timeline(eng, x, W, H, wins)
    xd = eng._dev(np.array(x))
    n = 0
    for i, t0 in enumerate(np.cumsum(wins)):
        if t0 <= W:
            continue
        batch = eng.rolling_timeline_device(xd[:t0], W, SR.THR, SR.GAP, SR.MINC)
        for k in SIX + FOUR:
            assert same_bytes(got[i][k], host(batch[k])), (k, t0)
        n += 1
    assert n >= 5


# ---- 3. partitions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SR.CASES[0], SR.CASES[3]], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_partition_independence(eng, case):
    P, M, W, H, seed, wins = case
    x, ref = SR.case_data(case)
    T = sum(wins)
    a = run_timeline(eng, x, W, H, wins, with_state=True)
    ones = run_timeline(eng, x, W, H, [1] * T, with_state=True)
    whole = run_timeline(eng, x, W, H, [T], with_state=True)
    keys = SIX + FOUR + ("sums", "ring", "bits", "episodes")
    for i, t in enumerate(np.cumsum(wins)):
        for k in keys:
            assert same_bytes(a[i][k], ones[t - 1][k]), (k, t)
    for k in keys:
        assert same_bytes(a[-1][k], whole[0][k]), k


# ---- 4. poisoned states, guard bands ----------------------------------------------------------------
@pytest.mark.parametrize("case", SR.CASES[:2], ids=CASE_IDS[:2])
def test_stream_timeline_poisoned_state(eng, case):
    """state and ep_state are poisoned before the t0 = 0 call only (later calls carry them); after
    every window the canaries are checked; the outputs, the rolling state's defined part and the
    whole episode state are compared across the poisons, the outputs with the reference."""
    P, M, W, H, seed, wins = case
    x, ref = SR.case_data(case)
    size = int(eng.lib.krca_stream_state_size(P, M, W, H))
    ep_size = int(eng.lib.krca_stream_episode_state_size(P, M))
    assert ep_size == 32 * P * M

    def call(e):
        t = e.torch
        state = e._workspace("stream_state", size)
        ep_state = e._workspace("episode_state", ep_size)
        xd = e._dev(np.array(x))  # a writable copy of the shared fixture
        out, t0 = {}, 0
        for w, d in enumerate(wins):
            o = new_outputs(e, P, M, True)
            native._check(call_timeline(e, xd[t0:t0 + d], P, M, d, t0, W, H, state, ep_state, o),
                          "krca_stream_timeline")
            t0 += d
            t.cuda.synchronize()
            e._arena.check()
            for k, v in o.items():
                out[f"w{w}_{k}"] = host(v)
            for k, v in state_parts(host(state), P * M, W, H, t0).items():
                out[f"w{w}_state_{k}"] = v
            out[f"w{w}_episodes"] = host(ep_state)
        return out

    out = run_poisons(eng, call)
    for w in range(len(wins)):
        assert_six({k: out[f"w{w}_{k}"] for k in SIX}, ref[w], w)


# ---- 5. argument errors -----------------------------------------------------------------------------
def test_argument_errors_launch_nothing(eng):
    P, M, W, H = 37, 8, 10, 33
    t = torch
    state = t.zeros(int(eng.lib.krca_stream_state_size(P, M, W, H)), dtype=t.uint8, device=eng.device)
    ep_state = t.full((int(eng.lib.krca_stream_episode_state_size(P, M)),), 0x5B, dtype=t.uint8, device=eng.device)
    xd = t.zeros((1, P, M), dtype=t.float32, device=eng.device)
    o = new_outputs(eng, P, M, True)
    for v in o.values():
        v.view(t.uint8).fill_(0x5B)
    before = {k: host(v) for k, v in o.items()}
    bad = [(dict(gap=-1), b"gap"), (dict(minc=0), b"min_count"), (dict(t0=2**31 - 1), b"INT32_MAX"),
           (dict(ep_state=None), b"null")]
    for kw, word in bad:
        a = dict(d=1, t0=0, ep_state=ep_state)
        a.update(kw)
        rc = call_timeline(eng, xd, P, M, a["d"], a["t0"], W, H, state, a["ep_state"], o,
                           gap=a.get("gap", SR.GAP), minc=a.get("minc", SR.MINC))
        assert rc < 0 and word in eng.lib.krca_last_error(), (kw, eng.lib.krca_last_error())
    t.cuda.synchronize()
    for k, v in o.items():
        assert same_bytes(host(v), before[k]), k  # nothing was launched
    assert bool((ep_state == 0x5B).all().item()) and bool((state == 0).all().item())
    assert call_timeline(eng, xd, 0, M, 1, 0, W, H, state, None, o) == 0  # P = 0: nothing to do
    ep_state.zero_()  # no episode open or kept
    assert call_timeline(eng, xd, P, M, 1, 2**31 - 2, W, H, state, ep_state, o) == 0  # t0 + delta == INT32_MAX
    t.cuda.synchronize()


# ---- 6. / 7. StreamingRCA(timeline=True) end to end -------------------------------------------------
E2E_W, E2E_H, E2E_WINDOWS = 60, 120, [61, 40, 99, 1, 12, 30, 57]


@pytest.fixture(scope="module")
def e2e():
    """The 2000-pod mesh with planted onsets (roots at t = 200, each hop 12 steps later), quantised to
    1/16; the streaming reference after every window and the batch timeline of the whole series."""
    m = synth.make_graph(2000, avg_degree=16, seed=3)
    hops = synth.caller_hops(m, m.roots, hops=2, cap=150)
    x, planted = synth.make_metrics_onsets(2000, 8, 300, seed=9, roots=m.roots, hop_sets=hops, t_root=200, delay=12,
                                           jitter=2)
    x = (torch.round(x * 16.0) / 16.0).contiguous()
    ref = SR.stream_timeline(x.numpy(), E2E_W, 3.0, SR.GAP, SR.MINC, E2E_H, E2E_WINDOWS)
    return m, x, ref, R.timeline(x.numpy(), E2E_W, 3.0, SR.GAP, SR.MINC)


def make_stream(eng, m):
    return StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, 8, Config(window=E2E_W), horizon=E2E_H, tol=1e-9,
                        max_iter=60, timeline=True, gap=SR.GAP, min_count=SR.MINC)


def stream_rows(s, xd, start, t):
    rows = []
    for d in E2E_WINDOWS[start:]:
        o = s.window(xd[t:t + d].contiguous())
        t += d
        row = {k: host(v) for k, v in o["scores"].items()}
        row.update(r=host(s.shard.r[:2000]), iters=o["iters"], top=[int(i) for i in o["top"][0]],
                   movers=s.first_movers(k=10, slack=2))
        rows.append(row)
    return rows


def assert_movers(got, want, where):
    for k in ("idx", "onset", "lead", "peak", "followers"):
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, (k, where)


def test_streaming_rca_timeline_end_to_end(e2e):
    eng = native.NativeEngine()
    m, x, ref, batch = e2e
    # the horizon matters on this fixture: fewer pods report an onset than in the batch timeline, the
    # first-mover top-10 differs from the batch one, and it holds all 10 planted roots
    want_last = R.first_movers(ref[-1], m.row_ptr, m.col, 2, 10)
    assert int((ref[-1]["onset"] >= 0).sum()) == 315 and int((batch["onset"] >= 0).sum()) == 320
    assert want_last["idx"].tolist() != R.first_movers(batch, m.row_ptr, m.col, 2, 10)["idx"].tolist()
    assert len(m.roots) == 10 and set(int(r) for r in m.roots) <= set(want_last["idx"].tolist())
    s = make_stream(eng, m)
    with pytest.raises(ValueError, match="no window"):
        s.first_movers()
    rows = stream_rows(s, x.cuda(), 0, 0)
    assert set(rows[0]) >= set(SIX + FOUR)
    for i in range(len(E2E_WINDOWS) - 3, len(E2E_WINDOWS)):
        assert_six(rows[i], ref[i], i)
        assert_movers(rows[i]["movers"], R.first_movers(ref[i], m.row_ptr, m.col, 2, 10), i)
    assert len(rows[-1]["movers"]["idx"]) == 10


def test_streaming_rca_timeline_snapshot(e2e, tmp_path):
    """A snapshot after window 4 (t = 201, episodes open) restored into a fresh StreamingRCA: the
    remaining windows' scores, timeline outputs, ranks, iteration counts and first movers are those of
    the uninterrupted stream."""
    eng = native.NativeEngine()
    m, x, ref, _ = e2e
    xd = x.cuda()
    whole = stream_rows(make_stream(eng, m), xd, 0, 0)
    s, t = make_stream(eng, m), 0
    for d in E2E_WINDOWS[:4]:
        s.window(xd[t:t + d].contiguous())
        t += d
    assert t == 201
    path = str(tmp_path / "timeline_rank0.npz")
    s.snapshot(path)
    with np.load(path) as z:
        ep = z["episode_state"].view(np.int32).reshape(8, -1)
    assert int(((ep[2] > 0) & (t - 1 - ep[1] <= SR.GAP)).sum()) > 0  # episodes are open at the snapshot
    del s
    s2 = make_stream(eng, m)
    s2.restore(path)
    rest = stream_rows(s2, xd, 4, t)
    for i, (a, b) in enumerate(zip(whole[4:], rest)):
        for k in SIX + FOUR + ("r",):
            assert same_bytes(a[k], b[k]), (k, i)
        assert a["iters"] == b["iters"] and a["top"] == b["top"], i
        assert_movers(a["movers"], b["movers"], i)
    with pytest.raises(ValueError, match="timeline"):
        StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, 8, Config(window=E2E_W), horizon=E2E_H, tol=1e-9,
                     max_iter=60).restore(path)
