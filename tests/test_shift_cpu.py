"""Level-shift score without a GPU: the NumPy restatement (tests/shift_ref.py) against a plain-Python
brute force on hand cases, the MetricsAgent / Coordinator options over an engine that answers
shift_score from the restatement, and the recall fixture of DESIGN.md §3.19 on the restatement."""
import functools
import math
import struct

import numpy as np
import pytest

import agent_cases as A
import oracle
import shift_ref as S
from krca import rca, synth
from krca.agents.coordinator import Coordinator
from krca.agents.metrics import MetricsAgent
from krca.mock import MeshClient
from oracle_engine import OracleEngine

NS = A.NS


# ---- plain-Python brute force ------------------------------------------------------------------------
def f32(v):
    return struct.unpack("<f", struct.pack("<f", v))[0]


def bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def key(v):
    b = bits(v)
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else b | 0x80000000


def lmed(vals):
    return sorted(vals, key=key)[(len(vals) - 1) // 2]


def sub32(a, b):
    """float32 a - b, one rounding (scalar float32 arithmetic)."""
    with np.errstate(all="ignore"):
        return float(np.float32(a) - np.float32(b))


def brute(series, B, R, G, min_scale):
    """One series (list of float32-valued Python floats) -> (shift, base_med, base_mad, recent_med)."""
    T = len(series)
    base, rec = series[T - R - G - B:T - R - G], series[T - R:]
    med = lmed(base)
    mad = lmed([abs(sub32(v, med)) for v in base])
    rmed = lmed(rec)
    den = 1.4826 * mad
    ms = f32(min_scale)
    if not den > ms:
        den = ms
    if den > 0:
        with np.errstate(all="ignore"):
            shift = float(np.float32((rmed - med) / den))  # float64 division, then one rounding to float32
    else:
        shift = 0.0
    return shift, med, mad, rmed


def eq(a, b):
    return (math.isnan(a) and math.isnan(b)) or bits(a) == bits(b)


def check_against_brute(x, B, R, G=0, min_scale=0.0):
    x = np.asarray(x, np.float32)
    T, P, M = x.shape
    ref = S.shift_score(x, B, R, G, min_scale)
    for p in range(P):
        best, lead = 0.0, -1
        for m in range(M):
            want = brute([float(v) for v in x[:, p, m]], B, R, G, min_scale)
            got = tuple(float(ref[k][p, m]) for k in ("shift", "base_med", "base_mad", "recent_med"))
            assert all(eq(w, g) for w, g in zip(want, got)), (p, m, want, got)
            a = abs(want[0])
            if not math.isnan(a) and a > best:
                best, lead = a, m
        assert eq(float(ref["score"][p]), best) and int(ref["lead"][p]) == lead, (p, ref["score"][p], best, lead)
    return ref


def column(*series):
    """series of equal length -> x [T, 1, M] (M padded to a power of two with the first series)."""
    M = 1 << (len(series) - 1).bit_length()
    cols = list(series) + [series[0]] * (M - len(series))
    return np.array(cols, np.float32).T.reshape(len(series[0]), 1, M)


def test_key_order():
    nan_pos = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    nan_neg = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    order = np.array([nan_neg, -np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf, nan_pos], np.float32)
    k = S.to_key(order)
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert S.from_key(k).view(np.uint32).tolist() == order.view(np.uint32).tolist()
    assert [key(float(v)) for v in order] == k.tolist()


@pytest.mark.parametrize("B", [2, 3, 4, 5, 8])
def test_ties_even_and_odd_baselines(B):
    base = [1.0, 3.0, 3.0, 2.0, 3.0, 1.0, 2.0, 7.0][:B]
    ref = check_against_brute(column(base + [9.0, 9.5, 8.0], [5.0] * B + [5.0, 4.0, 4.0]), B, 3)
    assert float(ref["base_med"][0, 0]) == sorted(base)[(B - 1) // 2]  # the lower median, no averaging
    assert float(ref["recent_med"][0, 0]) == 9.0 and float(ref["recent_med"][0, 1]) == 4.0


def test_signed_zeros():
    x = column([0.0, -0.0, 0.0, -0.0, -0.0, 0.0], [-0.0, 0.0, -0.0, 0.0, 1.0, -1.0])
    ref = check_against_brute(x, 4, 2)
    assert bits(float(ref["base_med"][0, 0])) == 0x80000000  # rank 1 of {-0, -0, +0, +0}
    assert bits(float(ref["recent_med"][0, 0])) == 0x80000000 and bits(float(ref["recent_med"][0, 1])) == bits(-1.0)
    assert ref["shift"][0].tolist()[:2] == [0.0, 0.0] and ref["score"][0] == 0 and ref["lead"][0] == -1


@pytest.mark.parametrize("min_scale,want", [(0.0, 0.0), (0.5, 4.0)])
def test_mad_zero(min_scale, want):
    """More than half of the baseline equal: MAD 0.  min_scale = 0 scores 0, min_scale > 0 divides by it."""
    x = column([1.0, 1.0, 1.0, 1.0, 2.0, 0.0, 1.0, 3.0, 3.0, 4.0])
    ref = check_against_brute(x, 7, 3, 0, min_scale)
    assert float(ref["base_mad"][0, 0]) == 0.0 and float(ref["shift"][0, 0]) == want
    assert float(ref["score"][0]) == want and int(ref["lead"][0]) == (0 if want else -1)


def test_guard_rows_are_not_read():
    a = [1.0, 2.0, 3.0, 2.0, 1e9, -1e9, 6.0, 6.0]
    ref = check_against_brute(column(a), 4, 2, 2)
    assert float(ref["base_med"][0, 0]) == 2.0 and float(ref["recent_med"][0, 0]) == 6.0


def test_nan_and_inf_samples():
    nan = float("nan")
    x = column([1.0, nan, 2.0, 3.0, 2.5, 4.0, 4.0, 4.0],        # one NaN in the baseline: sorts last, finite answer
               [1.0, math.inf, 2.0, -math.inf, 2.5, 4.0, math.inf, 4.0],
               [nan, nan, nan, 1.0, 2.0, 5.0, 5.0, 5.0],        # the median itself is NaN
               [math.inf, math.inf, math.inf, 1.0, 2.0, math.inf, math.inf, 1.0])  # Inf - Inf
    ref = check_against_brute(x, 5, 3)
    # a NaN MAD is no scale: den falls back to min_scale, and min_scale = 0 scores the series 0
    assert np.isfinite(ref["shift"][0, :2]).all() and np.isnan(ref["base_mad"][0, 2:]).all()
    assert ref["shift"][0, 2:].tolist() == [0.0, 0.0] and ref["lead"][0] == 0
    ref = check_against_brute(x, 5, 3, 0, 0.5)
    assert np.isfinite(ref["shift"][0, :2]).all() and np.isnan(ref["shift"][0, 2:]).all()
    assert np.isfinite(ref["score"][0]) and ref["lead"][0] == 0  # NaN shifts are skipped
    allnan = check_against_brute(column([nan] * 8), 5, 3)
    assert allnan["score"][0] == 0 and allnan["lead"][0] == -1


@pytest.mark.parametrize("kind", ["noise", "ties", "signs", "nonfinite"])
def test_random_data_against_brute_force(kind):
    x = S.data(kind, 40, 3, 4, seed=5)
    check_against_brute(x, 16, 5, 2, 0.0)
    check_against_brute(x, 33, 4, 0, 0.5)


def test_refusals():
    x = np.zeros((10, 2, 2), np.float32)
    for kw in (dict(baseline=1), dict(baseline=257), dict(recent=0), dict(recent=65), dict(guard=-1),
               dict(baseline=8, recent=3), dict(min_scale=-1.0), dict(min_scale=float("inf")), dict(min_scale=float("nan"))):
        with pytest.raises(ValueError):
            S.shift_score(x, **{**dict(baseline=4, recent=2), **kw})
    with pytest.raises(ValueError):
        S.shift_score(np.zeros((10, 2, 3), np.float32), 4, 2)
    assert S.shift_score(np.zeros((10, 0, 2), np.float32), 4, 2)["score"].shape == (0,)


# ---- agents ----------------------------------------------------------------------------------------------
class ShiftOracleEngine(OracleEngine):
    """OracleEngine that answers shift_score from the restatement (NativeEngine.shift_score's keys)."""

    def shift_score(self, x, baseline=120, recent=3, guard=0, min_scale=0.0):
        x = np.asarray(x.cpu() if hasattr(x, "cpu") else x, np.float32)
        r = S.shift_score(x, baseline, recent, guard, min_scale)
        out = dict(r)
        for k in S.KEYS:
            out[k + "_host"] = r[k]
        return out


@functools.lru_cache(maxsize=None)
def mesh_case(n=256, T=300):
    m = synth.make_graph(n, avg_degree=4, seed=6)
    hops = synth.caller_hops(m, m.roots, hops=2, cap=150)
    x, _ = synth.make_metrics_onsets(n, 8, T, seed=6, roots=m.roots, hop_sets=hops, t_root=T - 30, delay=5)
    return m, x.numpy()


def expected_level_shifts(names, x, topk=10, B=120, R=3, G=0, min_scale=0.0, thr=None, z_threshold=3.0):
    """The "level_shifts" rows from the restatement alone."""
    T, P, M = x.shape
    ref = S.shift_score(x, B, R, G, min_scale)
    thr = max(z_threshold, rca.null_floor(P * M)) if thr is None else thr
    order = sorted(range(P), key=lambda p: (-float(ref["score"][p]), p))[:topk]
    rows = []
    for p in order:
        s = float(ref["score"][p])
        if not s > thr:
            break
        m = int(ref["lead"][p])
        den = max(1.4826 * float(ref["base_mad"][p, m]), float(np.float32(min_scale)))
        rows.append({"resource": f"Pod/{names[p]}", "metric": m, "shift": float(ref["shift"][p, m]),
                     "baseline": float(ref["base_med"][p, m]), "recent": float(ref["recent_med"][p, m]), "scale": den,
                     "severity": "high" if s > 2 * thr else "medium"})
    return rows, ref


def check_level_shifts_key(key, names, x, **kw):
    want, ref = expected_level_shifts(names, x, **kw)
    assert len(key) == len(want) > 0
    for row, w in zip(key, want):
        assert set(row) == {"resource", "metric", "shift", "baseline", "recent", "scale", "description", "severity"}
        assert {k: row[k] for k in w} == w
        assert isinstance(row["description"], str) and row["description"]
        assert abs(row["shift"] - (row["recent"] - row["baseline"]) / row["scale"]) <= 1e-6 * abs(row["shift"])
    scores = [abs(r["shift"]) for r in key]
    assert scores == sorted(scores, reverse=True)
    return ref


def check_shift_root_causes(rows, names, m, ref, x, engine=None):
    """The Coordinator's key = rank_root_causes seeded with the shift score, in _rank_root_causes' schema."""
    idx, val, rank = (engine or OracleEngine()).rank_root_causes(ref["score"], m.row_ptr, m.col, m.outdeg, rca.RANKING,
                                                                 n_metrics=x.shape[2])
    assert len(rows) == len(idx) > 0
    for r, (row, i, v) in enumerate(zip(rows, idx.tolist(), val.tolist())):
        assert set(row) == {"component", "rank", "score", "pagerank", "anomaly"}
        assert row == {"component": f"Pod/{names[i]}", "rank": r + 1, "score": float(v), "pagerank": float(rank[i]),
                       "anomaly": float(ref["score"][i])}


def test_metrics_agent_level_shifts():
    m, x = mesh_case()
    names = m.names()
    plain = A.strip(MetricsAgent(MeshClient(m, x), engine=ShiftOracleEngine()).analyze(NS))
    agent = MetricsAgent(MeshClient(m, x), engine=ShiftOracleEngine(), level_shift=True)
    res = A.strip(agent.analyze(NS))
    assert "error" not in res and "level_shifts" not in plain
    key = res.pop("level_shifts")
    assert res == plain  # the option adds one key and changes nothing else
    ref = check_level_shifts_key(key, names, x)
    assert {r["resource"] for r in key} <= {f"Pod/{names[i]}" for i in np.flatnonzero(ref["score"] > 4.0)}
    assert set(agent.last_shift) >= set(S.KEYS) and np.array_equal(agent.last_shift["score_host"], ref["score"])


def test_metrics_agent_level_shift_options():
    m, x = mesh_case()
    names = m.names()
    kw = dict(shift_baseline=64, shift_recent=8, shift_guard=5, shift_min_scale=0.25, shift_threshold=4.5)
    res = MetricsAgent(MeshClient(m, x), engine=ShiftOracleEngine(), level_shift=True, anomaly_topk=20, **kw).analyze(NS)
    check_level_shifts_key(res["level_shifts"], names, x, topk=20, B=64, R=8, G=5, min_scale=0.25, thr=4.5)
    assert {"medium", "high"} == {r["severity"] for r in res["level_shifts"]}


def test_metrics_agent_short_history():
    m, x = mesh_case()
    plain = A.strip(MetricsAgent(MeshClient(m, x[-100:]), engine=ShiftOracleEngine()).analyze(NS))
    agent = MetricsAgent(MeshClient(m, x[-100:]), engine=ShiftOracleEngine(), level_shift=True)
    res = A.strip(agent.analyze(NS))
    assert "error" not in res and res["level_shifts"] == [] and agent.last_shift is None
    why = [s for s in res["reasoning_steps"] if s not in plain["reasoning_steps"]]
    assert len(why) == 1 and "100 steps" in why[0]["observation"] and "level shifts" in why[0]["conclusion"]


def test_coordinator_level_shift_root_causes():
    m, x = mesh_case()
    names = m.names()
    plain = A.strip(Coordinator(MeshClient(m, x), engine=OracleEngine()).run_analysis("comprehensive", NS))
    off = A.strip(Coordinator(MeshClient(m, x), engine=ShiftOracleEngine()).run_analysis("comprehensive", NS))
    res = A.strip(Coordinator(MeshClient(m, x), engine=ShiftOracleEngine(), level_shifts=True)
                  .run_analysis("comprehensive", NS))
    assert "error" not in plain and "error" not in res and off == plain
    assert "level_shift_root_causes" not in plain and "level_shifts" not in plain["agent_results"]["metrics"]
    rows = res.pop("level_shift_root_causes")
    key = res["agent_results"]["metrics"].pop("level_shifts")
    assert res == plain and len(res["ranked_root_causes"]) > 0  # the z-score keys stay as they are
    ref = check_level_shifts_key(key, names, x)
    check_shift_root_causes(rows, names, m, ref, x)


def test_coordinator_short_history_has_no_shift_ranking():
    m, x = mesh_case()
    res = Coordinator(MeshClient(m, x[-100:]), engine=ShiftOracleEngine(), level_shifts=True).run_analysis(
        "comprehensive", NS)
    assert "error" not in res and "level_shift_root_causes" not in res
    assert res["agent_results"]["metrics"]["level_shifts"] == []


# ---- recall fixture -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recall_case(seed):
    """2 000 pods / 40 000 edges, M = 8, T = 300, the roots' level shifting 30 steps before the end and
    their callers' 5 steps per hop later."""
    m = synth.make_graph(2000, n_edges=40000, seed=seed)
    hops = synth.caller_hops(m, m.roots)
    x, _ = synth.make_metrics_onsets(2000, 8, 300, seed=seed, roots=m.roots, hop_sets=hops, t_root=270, delay=5)
    return m, x.numpy()


def top10(v):
    v = np.asarray(v)
    return set(sorted(range(len(v)), key=lambda i: (-float(v[i]), i))[:10])


def check_recall(m, shift, z, engine):
    roots = set(int(r) for r in m.roots)
    assert len(roots) == 10
    assert top10(shift) == roots            # the shift score finds exactly the planted roots
    assert not (top10(z) & roots)           # the last-step z-score finds none of them
    idx, _, _ = engine.rank_root_causes(shift, m.row_ptr, m.col, m.outdeg, rca.RANKING, n_metrics=8)
    assert len(set(int(i) for i in idx) & roots) >= 9


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_recall_fixture_on_the_restatement(seed):
    m, x = recall_case(seed)
    shift = S.shift_score(x, 120, 3, 0)["score"]
    z = oracle.c_rolling_score(x, rca.RANKING.window, rca.RANKING.z_threshold)["score"]
    check_recall(m, shift, z, OracleEngine())
