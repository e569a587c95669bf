"""Graph structure on the device (csrc/graph_struct.hip): every array and every stat of krca_graph_scc /
krca_graph_chain / krca_graph_cycle bit for bit against tests/graph_structure_ref.py, in both CSR
layouts; guard bands and poisons; the agents' structure=True paths."""
import ctypes
import functools

import numpy as np
import pytest

import agent_cases as A
import graph_structure_ref as R
from guarded import GuardedEngine, run_poisons
from krca import native, tracecols
from krca.agents.traces import TracesAgent
from test_graph_structure_cpu import check_topology_structure
from test_trace_cpu import ColumnsClient

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


@pytest.fixture(scope="module")
def geng():
    return GuardedEngine()


def check(eng, rp, col, pull, want=None):
    """Runs the three calls in the given layout and in the other one; both must equal the restatement
    (hence each other) byte for byte.  -> (restated dict, GraphStructure)."""
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int32)
    ref = R.restate(rp, col, pull)
    if want is not None:
        for k, v in want.items():
            assert np.asarray(ref[k]).tolist() == v, ("restatement", k)
    rp_t, col_t = R.transpose_csr(rp, col)
    first = None
    for a, b, p in ((rp, col, pull), (rp_t, col_t, not pull)):
        gs = eng.graph_structure(a, b, pull=p)
        got = R.structure_arrays(gs)
        for k in R.STRUCT_KEYS:
            w, g = np.asarray(ref[k]), np.asarray(got[k])
            assert w.dtype == g.dtype and w.shape == g.shape, (k, p, w.dtype, g.dtype, w.shape, g.shape)
            assert w.tobytes() == g.tobytes(), (k, "pull" if p else "push", np.flatnonzero(w != g)[:5], w[w != g][:5],
                                                g[w != g][:5])
        first = first or gs
    return ref, first


def csr(n, edges):
    src, dst = (np.array(x, np.int64) for x in zip(*edges)) if edges else (np.zeros(0, np.int64),) * 2
    return R.csr_from_edges(n, src, dst)


# ---- trivial shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,edges,stats,chain", [
    (0, [], [0, 0, 0, 0, -1, 0], [0, -1]),
    (1, [], [1, 0, 0, 1, -1, 0], [1, 0]),
    (1, [(0, 0)], [1, 1, 1, 1, 0, 0], [1, 0]),
    (2, [(0, 1), (1, 0)], [1, 1, 2, 2, 0, 0], [1, 0]),
])
def test_trivial(eng, n, edges, stats, chain):
    ref, gs = check(eng, *csr(n, edges), False, want=dict(scc_stats=stats, chain_stats=chain))
    if n == 2:
        assert gs.first_cycle() == [0, 1]
    if edges == [(0, 0)]:
        assert gs.first_cycle() == [0] and gs.flags.tolist() == [7]


def test_hand_built(eng):
    """Two cycles sharing node 4 (2-3-4, 4-5-6), a tail in (11 -> 0 -> 1 -> 2), a tail out (6 -> 7 -> 8),
    a self-loop singleton (9), an isolated node (10), a duplicate edge (0 -> 1 twice)."""
    edges = [(11, 0), (0, 1), (0, 1), (1, 2), (2, 3), (3, 4), (4, 2), (4, 5), (5, 6), (6, 4), (6, 7), (7, 8), (9, 9)]
    want = dict(comp=[0, 1, 2, 2, 2, 2, 2, 7, 8, 9, 10, 11],
                flags=[4, 4, 5, 1, 1, 1, 1, 4, 4, 7, 4, 4],
                scc_stats=[8, 2, 6, 5, 2, 0],
                depth_dn=[5, 4, 3, 3, 3, 3, 3, 2, 1, 1, 1, 6],
                depth_up=[2, 3, 4, 4, 4, 4, 4, 5, 6, 1, 1, 1],
                next=[1, 2, 7, 7, 7, 7, 7, 8, -1, -1, -1, 0],
                chain_stats=[6, 11], root=2,
                hop=[-1, -1, 3, 4, 2, 6, 4, -1, -1, -1, -1, -1])
    _, gs = check(eng, *csr(12, edges), False, want=want)
    assert gs.first_cycle() == [2, 3, 4] and gs.longest_chain() == [11, 0, 1, 2, 7, 8]
    assert gs.cyclic_groups() == [2, 9] and gs.members(2) == [2, 3, 4, 5, 6]


# ---- random graphs around the giant-component threshold, duplicates and stray columns -----------
@pytest.mark.parametrize("per_node", [1.0, 1.5, 3.0])
@pytest.mark.parametrize("n", [63, 64, 65, 257, 4097])
def test_random(eng, n, per_node):
    for seed in range(3):
        rp, col = R.random_digraph(n, per_node, seed)
        ref, _ = check(eng, rp, col, False)
        assert ref["scc_stats"][5] >= 1  # stray columns are in and counted


@pytest.mark.parametrize("n", [65, 257])
def test_dense_rows(eng, n):
    """40 entries per row on average: at 32 or more a wave walks each row (16 lanes below)."""
    rp, col = R.random_digraph(n, 40.0, 4)
    ref, _ = check(eng, rp, col, False)
    assert ref["scc_stats"][3] >= n - 2


def test_adjacent_long_rows(eng):
    """Four neighbouring rows of 600 to 900 entries in a graph of short rows: the 16-lane walk hands
    each of them to the whole wave, one after the other (pull layout), and a short row follows them."""
    n = 1000
    rng = np.random.default_rng(8)
    src = [rng.choice(np.arange(8, n), 600 + 100 * h, replace=False) for h in range(4)]
    dst = [np.full(len(x), h) for h, x in enumerate(src)]
    back_src, back_dst = np.array([0, 1, 2, 3, 4, 4]), np.array([500, 501, 0, 2, 3, 4])  # cycles through the hubs
    src, dst = np.concatenate(src + [back_src]), np.concatenate(dst + [back_dst])
    rp, col = R.csr_from_edges(n, dst, src)  # rows = callees
    assert np.diff(rp)[:4].min() > 512 and rp[-1] < 32 * n
    ref, gs = check(eng, rp, col, True)
    assert ref["scc_stats"][1] >= 2 and gs.first_cycle() is not None


def test_random_with_a_capped_grid(eng):
    """KRCA_GRAPH_GRID = 3: three workgroups stride over 4 097 rows and nodes."""
    rp, col = R.random_digraph(4097, 3.0, 1)
    with native.tune(eng.lib, KRCA_GRAPH_GRID=3):
        ref, _ = check(eng, rp, col, False)
    assert ref["scc_stats"][3] > 1000  # above the threshold: a giant component


# ---- as many rounds as nodes ----------------------------------------------------------------------
def test_ring_and_chord(eng):
    n = 5000
    ring = [(i, (i + 1) % n) for i in range(n)]
    ref, gs = check(eng, *csr(n, ring), False)
    assert ref["scc_stats"].tolist() == [1, 1, n, n, 0, 0] and gs.first_cycle() == list(range(n))
    assert gs.rounds["passes"] == 1 and gs.rounds["reach"] >= 1 and gs.rounds["cycle"] >= 1
    ref, gs = check(eng, *csr(n, ring + [(1000, 4000)]), False)
    assert gs.first_cycle() == list(range(1001)) + list(range(4000, n))


def test_path(eng):
    n = 5000
    perm = np.random.default_rng(3).permutation(n)
    ref, gs = check(eng, *csr(n, [(int(perm[i]), int(perm[i + 1])) for i in range(n - 1)]), False)
    assert ref["chain_stats"].tolist() == [n, int(perm[0])] and gs.longest_chain() == perm.tolist()
    assert gs.first_cycle() is None


def test_hub_row(eng):
    """70 000 callers of one hub, 100 of which it calls back: a row longer than any tile (pull layout)
    and a 101-node group."""
    n, hub = 70_001, 35_000
    others = np.setdiff1d(np.arange(n), [hub])
    back = np.random.default_rng(5).choice(others, 100, replace=False)
    src = np.concatenate([others, np.full(100, hub)])
    dst = np.concatenate([np.full(len(others), hub), back])
    rp, col = R.csr_from_edges(n, dst, src)  # rows = callees
    assert np.diff(rp).max() == 70_000
    ref, gs = check(eng, rp, col, True)
    assert ref["scc_stats"].tolist() == [n - 100, 1, 101, 101, int(back.min() if back.min() < hub else hub), 0]
    assert len(gs.first_cycle()) == 2


# ---- service meshes with reversed edges -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_case(n, k):
    return R.reversed_mesh(n, k, seed=0)


@pytest.mark.parametrize("n,k", [(2000, 0), (2000, 3), (2000, 40), (70_000, 0), (70_000, 25), (70_000, 2000)])
def test_mesh(eng, n, k):
    rp, col = mesh_case(n, k)
    ref, gs = check(eng, rp, col, True)
    n_cyclic, largest = int(ref["scc_stats"][1]), int(ref["scc_stats"][3])
    if k == 0:
        assert n_cyclic == 0 and gs.first_cycle() is None
    else:
        src, dst, _ = R.edge_list(rp, col, True)
        assert R.is_path(src, dst, gs.first_cycle(), closed=True)
    if n == 70_000 and k:
        assert n_cyclic >= 2 and largest >= 1000  # a regenerated mesh must not turn these trivial


# ---- buffers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pull", [False, True])
def test_guard_bands_and_poisons(geng, pull):
    rp, col = R.random_digraph(4097, 1.5, 2)
    if pull:
        rp, col = R.transpose_csr(rp, col)
    ref = R.restate(rp, col, pull)
    assert ref["root"] >= 0 and ref["scc_stats"][5] > 0
    out = run_poisons(geng, lambda e: R.structure_arrays(e.graph_structure(rp, col, pull=pull)))
    for k in R.STRUCT_KEYS:
        assert np.asarray(ref[k]).tobytes() == np.asarray(out[k]).tobytes(), k


def test_chain_rejects_a_labelling_with_a_cycle(eng):
    """comp = own id on a ring is no component labelling: its condensation is the ring.  The rounds are
    bounded, the call fails and nothing is indexed out of range; a label outside [0, N) likewise."""
    torch = eng.torch
    n = 50
    rp, col = csr(n, [(i, (i + 1) % n) for i in range(n)])
    rp_d, col_d = eng._dev_n(rp, np.int64), eng._dev_n(col, np.int32)
    out = [torch.empty(n, dtype=torch.int32, device=eng.device) for _ in range(3)]
    ws = torch.empty(int(eng.lib.krca_graph_chain_ws_size(n)), dtype=torch.uint8, device=eng.device)
    stats = (ctypes.c_int64 * 2)()
    for comp in (np.arange(n, dtype=np.int32), np.full(n, n, np.int32), np.full(n, -5, np.int32)):
        comp_d = eng._dev_n(comp, np.int32)
        rc = eng.lib.krca_graph_chain(eng.ptr(rp_d), eng.ptr(col_d), n, 0, eng.ptr(comp_d), eng.ptr(ws),
                                      *(eng.ptr(t) for t in out), stats, None, eng._stream())
        assert rc in (-22, native.KRCA_ENOTCONV), rc
        assert b"krca_graph_chain" in eng.lib.krca_last_error()
    for root in (-1, n):  # a root outside [0, N): refused before any device work
        assert eng.lib.krca_graph_cycle(eng.ptr(rp_d), eng.ptr(col_d), n, 0, eng.ptr(comp_d), root, eng.ptr(ws),
                                        eng.ptr(out[0]), None, eng._stream()) == -22


# ---- agents ------------------------------------------------------------------------------------------
def test_topology_agent(eng):
    seen = check_topology_structure(eng)
    assert seen["cycle"] >= 1 and seen["chain"] >= 1
    assert A.check_topology(eng) == []  # structure=False: the goldens, unchanged


def _spans(cyclic):
    """gateway -> a -> b -> c (-> a when cyclic): one trace."""
    names = ["gateway", "a", "b", "c"]
    svc = [0, 1, 2, 3] + ([1] if cyclic else [])
    parent = [-1, 0, 1, 2] + ([3] if cyclic else [])
    n = len(svc)
    return tracecols.SpanColumns(np.array(svc, np.int32), np.array(parent, np.int32), np.array(svc, np.int32),
                                 np.full(n, 1000, np.uint32), np.zeros(n, np.uint8), names,
                                 [(i, "op") for i in range(len(names))])


@pytest.mark.parametrize("cyclic", [False, True])
def test_traces_agent(eng, cyclic):
    cols = _spans(cyclic)
    st = eng.trace_analyze(cols)
    want = tracecols.first_cycle(len(cols.services), st.edge_src.tolist(), st.edge_dst.tolist())
    assert (want is not None) == cyclic
    res = TracesAgent(ColumnsClient(cols=cols), engine=eng, structure=True).analyze("mesh")
    assert "error" not in res
    found = [f for f in res["findings"] if f["issue"] == "Circular dependency detected between services"]
    assert len(found) == (1 if cyclic else 0)
    if cyclic:
        names = found[0]["evidence"].split(": ", 1)[1].split(" → ")
        ids = [cols.services.index(x) for x in names]
        assert ids[0] == ids[-1] == min(ids) and R.is_path(st.edge_src, st.edge_dst, ids[:-1], closed=True)
    plain = TracesAgent(ColumnsClient(cols=cols), engine=eng).analyze("mesh")
    assert A.strip(plain) == A.strip(res)  # one cycle in this graph: both routes report it
