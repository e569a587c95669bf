"""Blast radius without a GPU: the host restatement (tests/blast_ref.py) against networkx itself, the
histogram clamp and the max_hops cut, the cover's tie rule, the BlastRadius walkers on restated arrays,
the Coordinator's `blast_radius` key over a restating engine, and the host-side contract of the C entry
points (exports, sizes, KRCA_EINVAL before any device work)."""
import ctypes

import networkx as nx
import numpy as np
import pytest

import agent_cases as A
import blast_ref as B
import graph_structure_ref as R
from krca import blast, native, synth
from krca.agents.coordinator import Coordinator
from krca.mock import MeshClient
from oracle_engine import OracleEngine

NS = "test-microservices"


def csr(n, edges):
    src, dst = (np.array(x, np.int64) for x in zip(*edges)) if edges else (np.zeros(0, np.int64),) * 2
    return R.csr_from_edges(n, src, dst)


def nx_graph(rp, col, pull=False):
    src, dst, _ = R.edge_list(rp, col, pull)
    g = nx.DiGraph()
    g.add_nodes_from(range(len(rp) - 1))
    g.add_edges_from(zip(src.tolist(), dst.tolist()))
    return g


def check_against_networkx(rp, col, sources, H=80):
    """H above every distance: the histogram is the exact distance distribution."""
    n = len(rp) - 1
    g = nx_graph(rp, col)
    mark = (np.arange(n) % 3 == 0).astype(np.uint8)
    for direction, graph, closure in ((B.DEPENDENCIES, g, nx.descendants), (B.DEPENDENTS, g.reverse(), nx.ancestors)):
        words, hist, depth = B.reach(rp, col, False, sources, direction, 0, mark, H)
        rp_t, col_t = R.transpose_csr(rp, col)
        other = B.reach(rp_t, col_t, True, sources, direction, 0, mark, H)
        assert all(np.array_equal(a, b) for a, b in zip((words, hist, depth), other))  # the layout does not show
        for k, s in enumerate(sources):
            members = np.flatnonzero((words >> np.uint64(k)) & np.uint64(1)).tolist()
            assert set(members) == closure(g, s) | {s}
            dist = nx.single_source_shortest_path_length(graph, s)
            assert set(dist) == set(members)
            want = np.bincount(list(dist.values()), minlength=H)
            assert hist[0, k].tolist() == want.tolist()
            assert hist[1, k].tolist() == np.bincount([d for v, d in dist.items() if mark[v]], minlength=H).tolist()
            assert depth[k] == max(dist.values())
        assert not (words >> np.uint64(len(sources))).any() if len(sources) < 64 else True


# ---- the restatement alone -------------------------------------------------------------------------
def test_hand_built_against_networkx():
    """Two cycles sharing node 4, a tail in, a tail out, a self-loop singleton, an isolated node, a
    duplicate edge (the graph of test_graph_structure's hand-built case)."""
    edges = [(11, 0), (0, 1), (0, 1), (1, 2), (2, 3), (3, 4), (4, 2), (4, 5), (5, 6), (6, 4), (6, 7), (7, 8), (9, 9)]
    rp, col = csr(12, edges)
    check_against_networkx(rp, col, list(range(12)))
    words, hist, depth = B.reach(rp, col, False, [8, 10], B.DEPENDENTS, bins=16)
    assert np.flatnonzero(words & np.uint64(1)).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 11]  # everything upstream of 8
    assert np.flatnonzero(words & np.uint64(2)).tolist() == [10] and depth.tolist() == [9, 0]
    assert hist[0, 0].tolist() == [1] * 10 + [0] * 6  # 8, 7, 6, 5, 4, 3, 2, 1, 0, 11: one per hop


@pytest.mark.parametrize("n", [20, 65])
def test_random_against_networkx(n):
    for seed in range(4):
        rp, col = R.random_digraph(n, 1.5, seed)
        rng = np.random.default_rng(seed)
        check_against_networkx(rp, col, rng.integers(0, n, min(n, 64)).tolist())


def test_clamp_and_max_hops():
    """A 12-node chain 0 -> 1 -> ... -> 11, source 0 along the edges."""
    n = 12
    rp, col = csr(n, [(i, i + 1) for i in range(n - 1)])
    words, hist, depth = B.reach(rp, col, False, [0], B.DEPENDENCIES, 0, None, 5)
    assert hist[0, 0].tolist() == [1, 1, 1, 1, 8] and depth.tolist() == [11]  # the last bin: 4 hops or more
    assert np.array_equal(hist[0], hist[1])  # mark = None: every node is marked
    for hops, want in ((3, [1, 1, 1, 1, 0]), (4, [1, 1, 1, 1, 1]), (6, [1, 1, 1, 1, 3])):
        words, hist, depth = B.reach(rp, col, False, [0], B.DEPENDENCIES, hops, None, 5)
        assert hist[0, 0].tolist() == want and depth.tolist() == [hops]
        assert np.flatnonzero(words).tolist() == list(range(hops + 1))  # the cut is exact
    words, _, depth = B.reach(rp, col, False, [0], B.DEPENDENTS, 0, None, 5)
    assert np.flatnonzero(words).tolist() == [0] and depth.tolist() == [0]


def test_cover_tie_rule_and_tail():
    # bit 0: nodes 0-3; bit 1: nodes 2-5 (a tie with bit 0: the lower k wins); bit 2: inside bit 0; bit 3: node 6
    words = np.array([0b0101, 0b0101, 0b0011, 0b0011, 0b0010, 0b0010, 0b1000, 0], np.uint64)
    order, gain, exclusive, totals = B.cover(words, None, 4)
    assert order.tolist() == [0, 1, 3, -1] and gain.tolist() == [4, 2, 1, 0]
    assert exclusive.tolist() == [0, 2, 0, 1] and totals.tolist() == [8, 7]
    mark = np.array([0, 0, 0, 0, 1, 1, 0, 1], np.uint8)
    order, gain, exclusive, totals = B.cover(words, mark, 4)
    assert order.tolist() == [1, -1, -1, -1] and gain.tolist() == [2, 0, 0, 0]
    assert exclusive.tolist() == [0, 2, 0, 0] and totals.tolist() == [3, 2]
    order, gain, _, totals = B.cover(words, np.zeros(8, np.uint8), 4)
    assert order.tolist() == [-1] * 4 and gain.tolist() == [0] * 4 and totals.tolist() == [0, 0]
    words64 = np.array([1 << 63, (1 << 63) | 1, 1], np.uint64)  # the sign bit is a bit like any other
    order, gain, exclusive, _ = B.cover(words64, None, 64)
    assert order[:2].tolist() == [0, 63] and gain[:2].tolist() == [2, 1] and exclusive[[0, 63]].tolist() == [1, 1]


# ---- BlastRadius -----------------------------------------------------------------------------------
def test_walkers_and_summary():
    # callers -> callees: a, b -> c -> d;  e -> d;  f alone
    rp, col = csr(6, [(0, 2), (1, 2), (2, 3), (4, 3)])
    mark = np.array([1, 0, 1, 1, 0, 0], np.uint8)
    sources = [3, 2, 5]
    o = B.restate(rp, col, False, sources, B.DEPENDENTS, 0, mark, 4)
    br = B.as_blast(o, sources)
    assert br.k == 3 and br.members(0) == [0, 1, 2, 3, 4] and br.members(1) == [0, 1, 2] and br.members(2) == [5]
    assert (br.reached(0), br.reached_marked(0), br.reached(1), br.reached_marked(1)) == (5, 3, 3, 2)
    assert br.rollup(0, ["x", "x", "y", "z", "x", "w"]) == [("x", 3), ("y", 1), ("z", 1)]
    assert br.cover() == [(0, 3)]
    names = list("abcdef")
    s = br.summary(names)
    assert s["candidates"][0] == {"component": "d", "rank": 1, "dependents": 4, "anomalous_dependents": 2,
                                  "share_of_anomalous": 1.0, "depth": 2, "exclusive_anomalous": 1,
                                  "by_hop": [1, 2, 2, 0], "anomalous_by_hop": [1, 1, 1, 0]}
    assert s["candidates"][1]["dependents"] == 2 and s["candidates"][1]["anomalous_dependents"] == 1
    assert s["candidates"][2]["dependents"] == 0 and s["candidates"][2]["share_of_anomalous"] == 0.0
    assert s["cover"] == [{"component": "d", "rank": 1, "gain": 3, "cumulative_share": 1.0}]
    assert s["anomalous"] == 3 and s["unreached"] == 0
    assert s["params"] == {"direction": "dependents", "max_hops": 0, "bins": 4}
    assert br.summary()["candidates"][0]["component"] == 3
    assert blast.DIRECTIONS == {"dependents": B.DEPENDENTS, "dependencies": B.DEPENDENCIES}


# ---- the C entry points on the host -----------------------------------------------------------------
def test_size_function_and_signatures():
    lib = native.load_library()
    for s in ("krca_graph_reach_ws_size", "krca_graph_reach", "krca_graph_reach_cover"):
        assert s in native.SIGNATURES and hasattr(lib, s)
    sizes = [lib.krca_graph_reach_ws_size(n) for n in (0, 1, 2, 1000, 1 << 20, (1 << 31) - 2)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[3] < sizes[4]
    assert sizes[4] >= 2 * 8 * (1 << 20) and lib.krca_graph_reach_ws_size(-1) == 0


def test_invalid_arguments_need_no_device():
    """Every refusal comes before any device work: the pointers are never touched (they are bogus)."""
    lib = native.load_library()
    vp = ctypes.c_void_p
    bogus = vp(4096)
    src = (ctypes.c_int32 * 65)(*([0] * 65))
    hist, depth = (ctypes.c_int64 * (2 * 64 * 64))(), (ctypes.c_int32 * 64)()

    def call(N=10, pull=1, K=1, direction=0, H=16, s0=0):
        src[0] = s0
        return lib.krca_graph_reach(bogus, bogus, N, pull, src, K, direction, 0, None, H, bogus, bogus, hist, depth,
                                    None, None)
    for kw in (dict(K=0), dict(K=65), dict(H=1), dict(H=65), dict(direction=2), dict(direction=-1), dict(pull=2),
               dict(s0=-1), dict(s0=10), dict(N=0), dict(N=(1 << 31) - 1), dict(N=-3)):
        assert call(**kw) == -22, kw
        assert b"krca_graph_reach" in lib.krca_last_error()
    order, gain = (ctypes.c_int32 * 64)(), (ctypes.c_int64 * 64)()
    for N, K in ((10, 0), (10, 65), (0, 1), ((1 << 31) - 1, 1)):
        assert lib.krca_graph_reach_cover(bogus, None, N, K, bogus, order, gain, gain, gain, None) == -22


# ---- the coordinator ---------------------------------------------------------------------------------
class RefBlastEngine(OracleEngine):
    """OracleEngine plus blast_radius from the restatement."""

    def blast_radius(self, row_ptr, col, sources, mark=None, score=None, floor=None, pull=True, direction="dependents",
                     max_hops=0, bins=16, cover=True):
        src = np.asarray(sources, np.int64)
        src = src[src != -1]
        if score is not None and floor is not None:
            mark = np.asarray(score.cpu() if hasattr(score, "cpu") else score, np.float32) > np.float32(floor)
        self.calls = getattr(self, "calls", 0) + 1
        self.last = dict(sources=src, mark=None if mark is None else np.asarray(mark).astype(np.uint8))
        o = B.restate(row_ptr, col, pull, src, blast.DIRECTIONS[direction], max_hops, mark, bins)
        return B.as_blast(o, src, direction, max_hops)


def mesh_case(n=256):
    m = synth.make_graph(n, avg_degree=4, seed=6)
    hops = synth.caller_hops(m, m.roots, hops=2, cap=150)
    x = synth.make_metrics(n, 8, 300, seed=6, roots=m.roots, hop_sets=hops)
    return m, x.numpy()


def check_blast_key(key, names, rp, col, sources, mark, bins):
    """The coordinator's key against the restatement of the same sources and mark."""
    o = B.restate(rp, col, True, sources, B.DEPENDENTS, 0, mark, bins)
    want = B.as_blast(o, sources).summary(names=[f"Pod/{n}" for n in names])
    assert key == want
    assert set(key) == {"candidates", "cover", "anomalous", "unreached", "params"}
    for c in key["candidates"]:
        assert set(c) == {"component", "rank", "dependents", "anomalous_dependents", "share_of_anomalous", "depth",
                          "exclusive_anomalous", "by_hop", "anomalous_by_hop"}
    for c in key["cover"]:
        assert set(c) == {"component", "rank", "gain", "cumulative_share"}
    assert key["anomalous"] == int((np.asarray(mark) != 0).sum())
    return o


def test_coordinator_blast_radius_key():
    from krca.rca import RANKING
    m, x = mesh_case()
    eng = RefBlastEngine()
    plain = A.strip(Coordinator(MeshClient(m, x), engine=OracleEngine()).run_analysis("comprehensive", NS))
    res = A.strip(Coordinator(MeshClient(m, x), engine=eng, blast_radius=True, blast_bins=8)
                  .run_analysis("comprehensive", NS))
    assert "error" not in plain and "blast_radius" not in plain and "error" not in res
    key = res.pop("blast_radius")
    assert res == plain  # ranked_root_causes and every other key: unchanged
    names = m.names()
    ranked = [names.index(r["component"][len("Pod/"):]) for r in res["ranked_root_causes"]]
    score = np.asarray(OracleEngine().rolling_score(x, RANKING.window, RANKING.z_threshold)["score"])
    mark = score > np.float32(RANKING.floor(len(names), x.shape[2]))
    assert eng.last["sources"].tolist() == ranked and np.array_equal(eng.last["mark"], mark.astype(np.uint8))
    o = check_blast_key(key, names, m.row_ptr, m.col, ranked, mark, 8)
    assert key["params"]["bins"] == 8 and 0 < key["anomalous"] < len(names) and o["order"][0] >= 0


def test_coordinator_without_the_flag_makes_no_call():
    m, x = mesh_case()
    eng = RefBlastEngine()
    res = Coordinator(MeshClient(m, x), engine=eng).run_analysis("comprehensive", NS)
    assert "error" not in res and "blast_radius" not in res and "ranked_root_causes" in res
    assert getattr(eng, "calls", 0) == 0
    # the C1 service path: mark = error rate > 0 over the service CSR
    ref = Coordinator(A.Shim(), engine=OracleEngine()).run_analysis("comprehensive", A.NS)
    got = Coordinator(A.Shim(), engine=eng, blast_radius=True).run_analysis("comprehensive", A.NS)
    assert "error" not in got and "blast_radius" not in ref
    if "ranked_root_causes" in ref:
        key = got.pop("blast_radius")
        assert [c["component"] for c in key["candidates"]] == [r["component"] for r in ref["ranked_root_causes"]]
        assert key["anomalous"] == int(eng.last["mark"].sum()) > 0
    assert A.strip(got) == A.strip(ref)
