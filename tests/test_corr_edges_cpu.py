"""Lead/lag correlation along dependency edges without a GPU: the NumPy reference on hand fixtures,
the header / ctypes / library symbols, the Coordinator's `correlations` key on an engine backed by
the reference, and the dep_best decoding."""
import os
import re

import numpy as np

import agent_cases as A
import corr_edges_cases as C
import corr_edges_ref as R
from conftest import ROOT
from krca import leadlag, native, synth
from krca.agents.coordinator import Coordinator
from krca.mock import MeshClient
from oracle_engine import OracleEngine

NS = "test-microservices"


def bits(v):
    return int(np.abs(np.float32(v)).view(np.uint32))


# ---- the reference alone -------------------------------------------------------------------------
def test_hand_fixture_lags_counts_and_key():
    z = C.hand_fixture()
    rp, col = C.csr(C.HAND_EDGES, 4)
    out = R.edges(z, rp, col, L=C.HAND_L, tau=0.5, slack=0, detail=True)
    where = {}  # (caller, dep) -> CSR position
    for k in range(4):
        for e in range(rp[k], rp[k + 1]):
            where[(int(col[e]), k)] = e
    for edge, want in C.HAND_LAGS.items():
        assert out["lag"][where[edge]] == want, edge
    peak = np.float32(float((z[0].astype(np.float64) ** 2).sum()) / C.HAND_T)
    assert out["r_lag"][where[(1, 0)]] == peak and out["r_lag"][where[(1, 2)]] == -peak
    assert out["r_lag"][where[(2, 0)]] == -peak  # z2 is the negated series: r_lag of 2 -> 0 is negative
    for edge in ((3, 0), (0, 0)):  # the zero pod and the self loop
        e = where[edge]
        assert out["r0"][e] == 0 and out["r_lag"][e] == 0 and out["lag"][e] == 0
    # the definition, term by term, on one edge: S_l = sum_t z[j][t + l] z[k][t]
    for l in (-8, -1, 0, 3, 8):
        s = sum(float(z[1][t + l]) * float(z[0][t]) for t in range(max(0, -l), min(C.HAND_T, C.HAND_T - l)))
        assert out["c"][where[(1, 0)], C.HAND_L + l] == s / C.HAND_T
    # 1 -> 0 (+3) and 1 -> 2 (+5) are DEP_LEADS, 2 -> 0 (-2) is CALLER_LEADS, nothing is SYNC
    assert out["dep_lead"].tolist() == [0, 2, 0, 0] and out["dep_sync"].tolist() == [0, 0, 0, 0]
    assert out["caller_follow"].tolist() == [1, 0, 1, 0] and out["caller_lead"].tolist() == [1, 0, 0, 0]
    assert out["caller_sync"].tolist() == [0, 0, 0, 0]
    # pod 1's two leading dependencies have the same |r|: the lower id wins
    assert out["dep_best"].tolist() == [0, (bits(peak) << 32) | 0x7FFFFFFF, 0, 0]
    assert leadlag.decode_dep_best(out["dep_best"][1])[0] == 0
    score = np.array([5.0, 1.0, 2.0, 0.0], np.float32)
    key = R.lead_key(out["dep_lead"], out["caller_follow"], score)
    assert key.tolist() == [(1 << 32) | bits(5.0), 0, (1 << 32) | bits(2.0), 0]
    nan = R.lead_key(out["dep_lead"], out["caller_follow"], np.array([np.nan, 1, -2.0, 0], np.float32))
    assert nan.tolist() == [0, 0, 0, 0]
    # slack: with slack 3 the +3 edge is SYNC, the +5 edge still leads
    s3 = R.edges(z, rp, col, L=C.HAND_L, tau=0.5, slack=3)
    assert s3["dep_lead"].tolist() == [0, 1, 0, 0] and s3["dep_sync"].tolist() == [0, 1, 1, 0]
    assert s3["caller_sync"].tolist() == [2, 0, 0, 0] and s3["caller_lead"].tolist() == [0, 0, 0, 0]
    assert leadlag.decode_dep_best(s3["dep_best"][1])[0] == 2
    # a mask on pod 2 silences both of its edges
    m = R.edges(z, rp, col, L=C.HAND_L, tau=0.5, mask=np.array([1, 1, 0, 1], np.uint8))
    assert m["dep_lead"].tolist() == [0, 1, 0, 0] and m["caller_lead"].tolist() == [0, 0, 0, 0]
    assert m["lag"][where[(1, 2)]] == 0 and m["r_lag"][where[(2, 0)]] == 0
    # a window shorter than the shift: L = 2 cannot see +3
    assert R.edges(z, rp, col, L=2)["lag"][where[(1, 0)]] != 3


def test_tie_rule_prefers_the_positive_lag():
    z, (rp, col) = C.tie_fixture()
    out = R.edges(z, rp, col, L=8, tau=0.0, detail=True)
    c = out["c"][0]
    assert c[8 + 2] == c[8 - 2] == 12.0 / 32 and np.count_nonzero(c) == 2
    assert out["lag"].tolist() == [2] and out["dep_lead"].tolist() == [0, 1]
    # all sums zero: lag 0
    assert R.edges(np.zeros((2, 32), np.float32), rp, col, L=8, tau=0.0)["lag"].tolist() == [0]
    assert R.lag_order(3) == [0, 1, -1, 2, -2, 3, -3]


def test_dyadic_fixture_plants_its_ties():
    z, rp, col, ties = C.dyadic_case(64, long_row=2 * C.CHUNK + 1)
    deg = np.diff(rp)
    assert set(C.FORCED_DEGREES) <= set(deg.tolist()) and deg[-1] == 2 * C.CHUNK + 1
    out = R.edges(z, rp, col, L=8, tau=0.0)
    caller, callee, on = R.active_edges(rp, col, len(z))
    assert (~on).sum() >= 10  # self loops
    assert len(np.unique(np.stack([caller, callee]), axis=1).T) < len(caller)  # duplicate edges
    for j, k, m in ties:
        e = rp[k] + np.flatnonzero(col[rp[k]:rp[k + 1]] == j)[-1]
        assert out["lag"][e] == m, (j, k, m)
    assert np.abs(z).max() <= 8 and np.array_equal(z, np.round(z))


def test_float_fixture_margin():
    """The reference alone recovers every planted lag, the best |c| clear of the second by far more
    than 4 tol, so a float32 device cannot legitimately pick another lag on a planted edge."""
    z, rp, col, planted = C.float_case()
    out = R.edges(z, rp, col, L=8, tau=0.5, detail=True)
    assert len(planted) == 300 and len(col) == 600
    np.testing.assert_allclose((z.astype(np.float64) ** 2).mean(axis=1), 1.0, atol=1e-5)
    margin = []
    for k in range(len(z)):
        for e in range(rp[k], rp[k + 1]):
            lag = planted.get((int(col[e]), k))
            if lag is None:
                continue
            assert out["lag"][e] == lag
            a = np.sort(np.abs(out["c"][e]))
            margin.append(a[-1] - a[-2])
    assert len(margin) == 300 and min(margin) > 4 * C.tol(1440) and min(margin) > 0.05, min(margin)
    assert (np.abs(out["c"]) <= 1.0 + 1e-6).all()


# ---- header, ctypes table, library ---------------------------------------------------------------
def test_header_and_signatures_declare_the_calls():
    with open(os.path.join(ROOT, "include", "krca.h")) as f:
        src = f.read()
    assert re.search(r"^#define KRCA_CORR_MAX_LAG 16$", src, re.M)
    lib = native.load_library()
    for name, nargs in (("krca_corr_edges_ws_size", 2), ("krca_corr_edges", 20), ("krca_corr_lead_key", 6)):
        assert re.search(r"^\w+ " + name + r"\(", src, re.M), name
        assert len(native.SIGNATURES[name][1]) == nargs and hasattr(lib, name), name
    # host-only size helper: room for the chunks past the first of every long row
    assert lib.krca_corr_edges_ws_size(10, 0) >= 8
    assert lib.krca_corr_edges_ws_size(1000, 20_000_000) >= 8 * (20_000_000 // C.CHUNK)


# ---- decoding ------------------------------------------------------------------------------------
def test_decode_dep_best_round_trip():
    assert leadlag.decode_dep_best(0) is None
    for r, dep in ((0.83, 0), (-0.5, 7), (1.0, 2 ** 31 - 2), (1e-3, 123456)):
        v = leadlag.encode_dep_best(r, dep)
        d, mag, b = leadlag.decode_dep_best(v)
        assert d == dep and mag == float(np.abs(np.float32(r))) and b == bits(r) and 0 < v < 2 ** 63
    # ordering: larger |r| first, then the lower id
    assert leadlag.encode_dep_best(0.9, 5) > leadlag.encode_dep_best(-0.8, 1)
    assert leadlag.encode_dep_best(0.9, 1) > leadlag.encode_dep_best(0.9, 5)
    f = leadlag.follower("a", "b", 4, 0.8312)
    assert leadlag.describe(f) == "Pod/a follows Pod/b by 4 steps (r = 0.83)"
    assert leadlag.describe(leadlag.follower("a", "b", 1, -0.5)) == "Pod/a follows Pod/b by 1 step (r = -0.50)"


# ---- Coordinator ---------------------------------------------------------------------------------
class RefCorrEngine(OracleEngine):
    """The oracle engine plus the two calls the Coordinator's correlations make, from the reference."""

    def corr_edges(self, x, row_ptr, col, channel=0, span=None, max_lag=8, tau=0.5, slack=0, mask=None, host=True):
        x = np.asarray(x.cpu() if hasattr(x, "cpu") else x, np.float32)
        if span is not None:
            x = x[x.shape[0] - span:]
        self.z32 = C.standardise(x[:, :, channel].T)
        return R.edges(self.z32, row_ptr, col, max_lag, tau, slack, mask)

    def lead_roots(self, edges_out, score, k=10, explain=(), row_ptr=None, col=None):
        score = np.asarray(score.cpu() if hasattr(score, "cpu") else score, np.float32)
        return R.lead_roots(edges_out, score, row_ptr, col, k, explain)


def mesh_case(n=400, T=300):
    m = synth.make_graph(n, avg_degree=4, seed=6)
    hops = synth.caller_hops(m, m.roots, hops=2, cap=150)
    x, _ = synth.make_metrics_onsets(n, 8, T, seed=6, roots=m.roots, hop_sets=hops, t_root=T - 100, delay=5, jitter=0)
    return m, x.numpy()


def test_coordinator_correlations_key():
    m, x = mesh_case()
    eng = RefCorrEngine()
    plain = A.strip(Coordinator(MeshClient(m, x), engine=OracleEngine()).run_analysis("comprehensive", NS))
    res = A.strip(Coordinator(MeshClient(m, x), engine=eng, correlations=True, corr_span=240, corr_tau=0.3)
                  .run_analysis("comprehensive", NS))
    assert "error" not in plain and "correlations" not in plain and "error" not in res
    corr = res.pop("correlations")
    assert res == plain  # nothing else changes
    assert set(corr) == {"lead_roots", "followers", "params"}
    assert corr["params"] == {"channel": 0, "span": 240, "max_lag": 8, "tau": 0.3, "slack": 0}
    assert eng.z32.shape == (400, 240)
    names = m.names()
    from krca.rca import RANKING
    score = np.asarray(OracleEngine().rolling_score(x, RANKING.window, RANKING.z_threshold)["score"])
    ref = R.edges(eng.z32, m.row_ptr, m.col, 8, 0.3, 0)
    ranked = [names.index(r["component"][len("Pod/"):]) for r in res["ranked_root_causes"]]
    want = R.lead_roots(ref, score, m.row_ptr, m.col, 10, ranked)
    assert len(corr["lead_roots"]) == len(want["idx"]) > 0
    for rank, (row, i) in enumerate(zip(corr["lead_roots"], want["idx"].tolist())):
        assert row == {"component": f"Pod/{names[i]}", "rank": rank + 1,
                       "followers": int(ref["caller_follow"][i]), "anomaly": float(score[i])}
        assert set(row) == {"component", "rank", "followers", "anomaly"}
    assert corr["followers"] == [leadlag.follower(names[p], names[want["explained"][p][0]], *want["explained"][p][1:])
                                 for p in ranked if p in want["explained"]]
    for f in corr["followers"]:
        assert set(f) == {"component", "follows", "lag_steps", "r"} and f["lag_steps"] > 0 and abs(f["r"]) > 0.3
        assert leadlag.describe(f).startswith(f["component"] + " follows " + f["follows"])


def test_coordinator_default_and_fallbacks_unchanged():
    """Off by default; on, a client without the bulk accessors gets no key and no error; an engine
    without the call reports through the error dict."""
    res = Coordinator(A.Shim(), engine=OracleEngine(), correlations=True).run_analysis("comprehensive", A.NS)
    ref = Coordinator(A.Shim(), engine=OracleEngine()).run_analysis("comprehensive", A.NS)
    assert "error" not in res and "correlations" not in res and A.strip(res) == A.strip(ref)
    m, x = mesh_case(200, 200)
    bad = Coordinator(MeshClient(m, x), engine=OracleEngine(), correlations=True).run_analysis("comprehensive", NS)
    assert set(bad) == {"error"} and "corr_edges" in bad["error"]
