"""Anomaly timeline without a GPU: the reference (tests/timeline_ref.py) on hand-made fixtures whose
answers are written out here, the exported ABI, and the MetricsAgent switch's default."""
import ctypes

import numpy as np

import timeline_cases as C
import timeline_ref as R
from krca import native, synth, timeline


# ---- episode semantics ------------------------------------------------------------------------
def test_series_episodes_by_hand():
    z = np.float32
    # gap of exactly G continues, G + 1 splits
    eps, kept = R.series_episodes([5, 8, 11, 15], [4, 5, 4, 9], G=3, R=3)
    assert eps == [(5, 11, 3, z(5)), (15, 15, 1, z(9))] and kept == (5, 11, 3, z(5))
    # cnt R - 1 is not sustained; equal peaks: the later sustained episode is kept
    eps, kept = R.series_episodes([1, 2, 10, 11, 12, 20, 21, 22], [9, 9, 4, 6, 5, 6, 4, 4], G=3, R=3)
    assert [e[2] for e in eps] == [2, 3, 3] and kept == (20, 22, 3, z(6))
    # the strongest wins over a later weaker one
    _, kept = R.series_episodes([10, 11, 12, 20, 21, 22], [4, 7, 5, 6, 4, 4], G=3, R=3)
    assert kept == (10, 12, 3, z(7))
    # G = 0, R = 1: adjacent steps do not merge, every exceedance is a sustained episode
    eps, kept = R.series_episodes([3, 4, 9], [4, 5, 5], G=0, R=1)
    assert eps == [(3, 3, 1, z(4)), (4, 4, 1, z(5)), (9, 9, 1, z(5))] and kept == (9, 9, 1, z(5))
    assert R.series_episodes([], [], 3, 3) == ([], None)


def test_pod_combine_by_hand():
    z = np.float32
    kept = [(50, 60, 5, z(4)), (48, 52, 3, z(9)), None, (10, 12, 3, z(8)), (56, 70, 4, z(9))]
    # anchor: peak 9, lowest m = 1 ([48, 52]); m0 overlaps; m3 is far; m4 starts at 56 > 52 + 3: out
    assert R.pod_combine(kept, G=3)[:6] == (48, 60, 8, z(9), 1, 2)
    assert R.pod_combine(kept, G=4)[:6] == (48, 70, 12, z(9), 1, 3)  # 56 <= 52 + 4
    # lead: the earliest onset, ties to the lowest m
    assert R.pod_combine([(7, 9, 3, z(4)), (7, 8, 3, z(5))], G=0)[:6] == (7, 9, 6, z(5), 0, 2)
    assert R.pod_combine([None, None], 3)[:6] == (-1, -1, 0, z(0), -1, 0)


def test_episode_fixture_covers_every_named_case():
    x = C.episode_fixture()
    assert np.array_equal(x, R.quantise(x))  # the exactness condition of timeline_ref
    ex, _ = R.rolling_exceed(x.reshape(C.T, -1), C.W, C.THR)
    for p in range(C.P):
        for m in range(C.M):
            assert np.flatnonzero(ex[:, p * C.M + m]).tolist() == C.PLAN.get((p, m), []), (p, m)
    r = R.timeline(x, C.W, C.THR, C.G, C.MINC, detail=True)
    eps = [e for p in range(C.P) for m in range(C.M) for e in r["episodes"][p][m]]
    sus = [e for e in eps if e[2] >= C.MINC]
    # each named case occurs in the reference's own intermediate output
    assert any(e[0] == C.W for e in eps), "exceedance at the first evaluated step"
    assert any(e[1] == C.T - 1 and e[2] >= C.MINC for e in eps), "episode ending at T - 1"
    steps01 = C.PLAN[(0, 1)]
    assert C.G in np.diff(steps01) and C.G + 1 in np.diff(steps01)
    assert r["episodes"][0][1] == [(80, 86, 3, r["episodes"][0][1][0][3]), (90, 91, 2, r["episodes"][0][1][1][3])]
    assert any(e[2] == C.MINC for e in eps) and any(e[2] == C.MINC - 1 for e in eps)
    e00 = r["episodes"][0][0]
    assert len(e00) == 3 and e00[0][3] == e00[1][3] == e00[2][3], "sustained episodes of equal peak"
    assert r["kept"][0][0] == e00[2], "the later one wins"
    assert r["kept"][0][2] is not None and 2 not in r["members"][0], "a kept episode that is no member"
    assert r["members"][0] == [0, 1]
    assert r["n_exceed"][2] == 0 and r["n_exceed"][3] == 2 and len(sus) == 6
    # the pod outputs, by hand
    assert r["onset"].tolist() == [80, C.T - 3, -1, -1]
    assert r["last"].tolist() == [86, C.T - 1, -1, -1]
    assert r["count"].tolist() == [6, 3, 0, 0]
    assert r["lead"].tolist() == [0, 3, -1, -1]
    assert r["n_metrics"].tolist() == [2, 1, 0, 0]
    assert r["peak"][0] == e00[2][3] and r["peak"][2] == 0 and r["peak"][3] == 0
    # G = 0, R = 1: every exceedance is its own sustained episode
    r0 = R.timeline(x, C.W, C.THR, 0, 1, detail=True)
    assert [e[:3] for e in r0["episodes"][3][1]] == [(50, 50, 1), (52, 52, 1)]
    assert r0["onset"][3] in (50, 52) and r0["count"][3] == 1 and r0["n_metrics"][3] == 1
    assert [e[:3] for e in r0["episodes"][0][0]][:2] == [(10, 10, 1), (11, 11, 1)]
    # T <= W: no evaluated step
    for t in (C.W, C.W - 3):
        e = R.timeline(x[:t], C.W, C.THR, C.G, C.MINC)
        assert (e["onset"] == -1).all() and (e["last"] == -1).all() and (e["count"] == 0).all()
        assert (e["peak"] == 0).all() and (e["lead"] == -1).all() and (e["n_metrics"] == 0).all()


def test_nan_never_exceeds():
    x = C.episode_fixture().copy()
    x[C.T - 2, 1, 3] = np.nan
    r = R.timeline(x, C.W, C.THR, C.G, C.MINC, detail=True)
    assert r["episodes"][1][3] == [(C.T - 3, C.T - 3, 1, r["episodes"][1][3][0][3])]  # the NaN poisons the sums after it


# ---- precedence on the known-answer graph ---------------------------------------------------------
def test_precede_known_answer_graph():
    rp, col = C.csr(C.EDGES, len(C.ONSET))
    assert rp.tolist() == [0, 3, 5, 5, 6, 6, 7, 8, 10] and col.tolist() == [0, 1, 2, 2, 6, 4, 6, 7, 5, 6]
    for slack, want in C.EXPECT.items():
        got = R.precede(C.ONSET, rp, col, slack)
        for k in ("dep_earlier", "dep_concurrent", "caller_later", "caller_concurrent", "caller_earlier", "dep_first"):
            assert got[k].tolist() == want[k], (slack, k)
        key = R.first_mover_key(C.ONSET, C.PEAK, got)
        assert np.flatnonzero(key).tolist() == want["first_movers"]
        assert int(key[0]) == (2 << 32) | int(np.float32(5.0).view(np.uint32))
        fm = R.first_movers(dict(onset=C.ONSET, peak=C.PEAK, lead=np.zeros(8, np.int8)), rp, col, slack, k=8,
                            explain=[2, 6, 0, 5])
        assert fm["idx"].tolist() == want["top"]
        assert fm["explained"] == {2: (0, 20), 6: (1, 40)}
        assert R.first_movers(dict(onset=C.ONSET, peak=C.PEAK, lead=np.zeros(8, np.int8)), rp, col, slack,
                              k=2)["idx"].tolist() == want["top"][:2]


def test_timeline_host_helpers():
    assert timeline.decode_dep_first(C.first(110, 1)) == (110, 1)
    assert timeline.decode_dep_first(R.NO_DEP) is None and timeline.NO_DEP == R.NO_DEP
    e = timeline.entry("db-0", 1380, 1439, 57, 2, 3, peak=9.5)
    assert e == {"resource": "Pod/db-0", "onset_step": 1380, "last_step": 1439, "episode_count": 57, "lead_metric": 2,
                 "n_metrics": 3, "peak": 9.5}
    assert timeline.format_entry(e, n_steps=1440, metric_names=["cpu", "mem", "lat"]) == (
        "Pod/db-0: anomalous from step 1380 (59 steps before the end) to 1439, 57 samples beyond the threshold "
        "on 3 metrics, lat first, peak |z| 9.50")
    assert timeline.entry("x", -1, -1, 0, -1, 0) is None
    assert timeline.format_follower("api-1", "db-0", 12) == "Pod/api-1 followed Pod/db-0 by 12 steps"


# ---- synthetic onsets -----------------------------------------------------------------------------
def test_make_metrics_onsets_keeps_the_background_and_plants_shifts():
    roots, hops = [3, 40], [[5, 6], [7]]
    x, on = synth.make_metrics_onsets(64, 4, 200, seed=5, roots=roots, hop_sets=hops, t_root=100, delay=10, jitter=2)
    bg = synth.make_metrics(64, 4, 200, seed=5)
    planted = np.flatnonzero(on >= 0)
    assert planted.tolist() == [3, 5, 6, 7, 40]
    assert all(abs(int(on[r]) - 100) <= 2 for r in roots) and all(abs(int(on[p]) - 110) <= 2 for p in hops[0])
    assert abs(int(on[7]) - 120) <= 2
    clean = np.setdiff1d(np.arange(64), planted)
    assert np.array_equal(x[:, clean].numpy(), bg[:, clean].numpy())
    for p in planted:
        assert np.array_equal(x[:on[p], p].numpy(), bg[:on[p], p].numpy())
        assert (x[on[p]:, p] >= bg[on[p]:, p]).all() and (x[on[p]:, p] > bg[on[p]:, p]).any()
    x2, on2 = synth.make_metrics_onsets(64, 4, 200, seed=5, roots=roots, hop_sets=hops, t_root=100, delay=10, jitter=2)
    assert np.array_equal(on, on2) and np.array_equal(x.numpy(), x2.numpy())
    # the reference finds the planted onsets of the roots (a 12 sigma shift) within a few steps
    r = R.timeline(R.quantise(x.numpy()), 60, 3.0)
    assert all(abs(int(r["onset"][p]) - int(on[p])) <= 3 for p in roots)


# ---- ABI --------------------------------------------------------------------------------------------
def test_timeline_symbols_exported():
    """Fails without the feature: the four calls are exported and bound."""
    lib = native.load_library()
    for name in ("krca_rolling_timeline", "krca_rca_precede_ws_size", "krca_rca_precede", "krca_rca_first_mover_key"):
        assert name in native.SIGNATURES and hasattr(lib, name), name
    assert lib.krca_rca_precede_ws_size(1 << 20) > lib.krca_rca_precede_ws_size(1 << 10) >= 4 << 10
    # argument checks need no device
    vp = ctypes.c_void_p
    one = np.zeros(16, np.int64)
    p = one.ctypes.data_as(vp)
    bad = lambda gap, minc, M=8: lib.krca_rolling_timeline(p, 1, M, 100, 60, 3.0, gap, minc, p, p, p, p, p, p, p, p, p,  # noqa: E731
                                                           p, None)
    assert bad(-1, 3) != 0 and b"gap" in lib.krca_last_error()
    assert bad(3, 0) != 0 and bad(3, 3, M=6) != 0
    assert lib.krca_rolling_timeline(None, 0, 8, 100, 60, 3.0, 3, 3, *([None] * 11)) == 0  # P = 0: nothing to do
    assert lib.krca_rca_precede(p, 8, -1, p, p, p, p, p, p, p, p, p, p, None) != 0 and b"slack" in lib.krca_last_error()


# ---- agent ------------------------------------------------------------------------------------------
def test_metrics_agent_default_is_unchanged():
    import agent_cases as A
    from oracle_engine import OracleEngine
    gold = A.load("metrics_scaled.json")
    client = A.DictClient(pod_metrics=gold["pod_metrics"], node_metrics=gold["node_metrics"])
    for kw in ({}, {"timeline": False}):
        res = A.MetricsAgent(client, engine=OracleEngine(), **kw).analyze("scaled")
        assert A.same(res, gold["result"]) and "anomaly_timeline" not in res
    # bulk path: timeline=False never asks the engine for a timeline (the oracle engine has none)
    m = synth.make_graph(200, avg_degree=4, seed=1)
    x = synth.make_metrics(200, 4, 100, seed=1, roots=m.roots)
    names = m.names()
    a = A.strip(A.MetricsAgent(C.BulkClient(names, x), engine=OracleEngine()).analyze("ns"))
    b = A.strip(A.MetricsAgent(C.BulkClient(names, x), engine=OracleEngine(), timeline=False).analyze("ns"))
    assert a == b and a["anomalies"] and "anomaly_timeline" not in a and "error" not in a
