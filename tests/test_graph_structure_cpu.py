"""Graph structure without a GPU: the host restatement (tests/graph_structure_ref.py) against networkx
itself, the GraphStructure walkers on restated arrays, the agents' structure path over a restating
engine, and the host-side contract of the three C entry points (exports, sizes, KRCA_EINVAL)."""
import ctypes

import networkx as nx
import numpy as np
import pytest

import agent_cases as A
import graph_structure_ref as R
from krca import graphstruct, native
from krca.agents.topology import TopologyAgent
from oracle_engine import OracleEngine


def small_graphs():
    """About 50 seeded digraphs of 1..14 nodes: sparse to dense, acyclic ones, self-loops, duplicates."""
    out = []
    for seed in range(52):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(1, 15))
        e = int(rng.integers(0, 3 * n + 1))
        src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
        if seed % 3 == 0:  # acyclic: edges from the lower to the higher id only
            keep = src != dst
            src, dst = np.minimum(src, dst)[keep], np.maximum(src, dst)[keep]
        if seed % 5 == 0 and e:
            src, dst = np.concatenate([src, src[:2]]), np.concatenate([dst, dst[:2]])  # duplicate edges
        out.append((n, src.astype(np.int64), dst.astype(np.int64)))
    return out


GRAPHS = small_graphs()


def nx_graph(n, src, dst):
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(src.tolist(), dst.tolist()))
    return g


@pytest.mark.parametrize("case", range(len(GRAPHS)))
def test_restatement_against_networkx(case):
    n, src, dst = GRAPHS[case]
    g = nx_graph(n, src, dst)
    rp, col = R.csr_from_edges(n, src, dst)
    o = R.restate(rp, col, pull=False)
    # the other layout restates to the same arrays
    o_pull = R.restate(*R.transpose_csr(rp, col), pull=True)
    for k in R.STRUCT_KEYS:
        assert np.array_equal(o[k], o_pull[k]), k
    # components: networkx's, labelled by their minimum
    want = np.zeros(n, np.int32)
    for c in nx.strongly_connected_components(g):
        want[list(c)] = min(c)
    assert np.array_equal(o["comp"], want)
    loops = set(nx.nodes_with_selfloops(g))
    sizes = np.bincount(want, minlength=n)[want]
    for v in range(n):
        assert bool(o["flags"][v] & 1) == (sizes[v] >= 2 or v in loops)
        assert bool(o["flags"][v] & 2) == (v in loops)
        assert bool(o["flags"][v] & 4) == (want[v] == v)
    cyclic = sorted({int(want[v]) for v in range(n) if o["flags"][v] & 1})
    assert o["scc_stats"].tolist() == [len(set(want.tolist())), len(cyclic), int((o["flags"] & 1).sum()),
                                       int(sizes.max()), cyclic[0] if cyclic else -1, 0]
    # depths: the longest path of networkx's condensation, from every component
    cond = nx.condensation(g)
    assert o["chain_stats"][0] == nx.dag_longest_path_length(cond) + 1
    label = {c: min(cond.nodes[c]["members"]) for c in cond}
    dn = {}
    for c in reversed(list(nx.topological_sort(cond))):
        dn[c] = 1 + max((dn[d] for d in cond.successors(c)), default=0)
    up = {}
    for c in nx.topological_sort(cond):
        up[c] = 1 + max((up[d] for d in cond.predecessors(c)), default=0)
    for c in cond:
        assert o["depth_dn"][label[c]] == dn[c] and o["depth_up"][label[c]] == up[c]
    # walkers: the chain is a path of the condensation of the right length, the cycle a cycle of g
    gs = R.as_structure(o)
    chain = gs.longest_chain()
    assert len(chain) == gs.longest and chain[0] == gs.start
    cedges = {(label[a], label[b]) for a, b in cond.edges}
    assert all(p in cedges for p in zip(chain, chain[1:]))
    assert gs.cyclic_groups() == cyclic
    for lab in cyclic:
        assert gs.members(lab) == [v for v in range(n) if want[v] == lab]
    cyc = gs.first_cycle()
    if not cyclic:
        assert cyc is None and nx.is_directed_acyclic_graph(g)
        # on an acyclic graph `longest` is the agent's own all-pairs longest simple path
        best = 0
        for s in g:
            for t in g:
                if s != t:
                    best = max([best] + [len(p) for p in nx.all_simple_paths(g, s, t)])
        assert gs.longest == max(best, 1)
    else:
        assert cyc[0] == cyclic[0] and len(set(cyc)) == len(cyc)
        assert R.is_path(src, dst, cyc, closed=True)
        # a shortest cycle through the root
        if cyc[0] in loops:
            assert cyc == [cyc[0]]
        else:
            assert len(cyc) == min(len(c) for c in nx.simple_cycles(g) if cyc[0] in c)
    s = gs.summary()
    assert s["cycle"] == cyc and s["chain"] == chain and s["longest_chain_exact"] == (not cyclic)
    assert all(type(x) is int for x in s["chain"] + s["cyclic_group_labels"])


def test_restatement_bad_edges_and_hop_rule():
    # 0 -> 1 -> 2 -> 0, 2 -> 3 -> 0 (two cycles sharing 0 and 2), entries outside [0, N) in three rows
    rp = np.array([0, 2, 4, 7, 9], np.int64)
    col = np.array([1, -1, 2, 4, 0, 3, 2**31 - 1, 0, -2**31], np.int32)
    o = R.restate(rp, col)
    assert o["scc_stats"].tolist() == [1, 1, 4, 4, 0, 4]
    assert o["hop"].tolist() == [1, 2, 0, 0]  # d = [0, 2, 1, 1]
    assert R.as_structure(o).first_cycle() == [0, 1, 2]
    o2 = R.restate(*R.transpose_csr(rp, col), pull=True)
    assert all(np.array_equal(o[k], o2[k]) for k in R.STRUCT_KEYS)
    assert graphstruct.rotate_to_lowest([3, 1, 2]) == [1, 2, 3]


class RestatingEngine(OracleEngine):
    """The oracle engine plus graph_structure from the restatement (no GPU)."""

    def graph_structure(self, row_ptr, col, pull=False, chain=True, cycle=True):
        return R.as_structure(R.restate(np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), pull), chain, cycle)


def check_topology_structure(engine):
    """TopologyAgent(structure=True) on the inputs of topology_small.json, against the goldens."""
    gold = A.load("topology_small.json")
    seen = {"cycle": 0, "chain": 0}
    for name, case in gold.items():
        agent = TopologyAgent(A.DictClient(**case["inputs"]), engine=engine, structure=True)
        res = agent.analyze("shop")
        assert "error" not in res, (name, res.get("error"))
        g = agent.service_graph
        want = {f["issue"]: f for f in case["result"]["findings"]}
        got = {f["issue"]: f for f in res["findings"]}
        circ, long_ = "Circular dependency detected in service architecture", "Long dependency chain detected"
        assert (circ in got) == (circ in want), name
        s = res.get("topology_structure")
        assert (s is not None) == (g.number_of_nodes() > 0), name  # no graph, no structure call
        if circ in got:
            seen["cycle"] += 1
            assert {k: got[circ][k] for k in ("component", "severity", "recommendation")} == \
                {k: want[circ][k] for k in ("component", "severity", "recommendation")}
            names = got[circ]["evidence"][len("Dependency cycle: "):].split(" → ")
            assert names[0] == names[-1] and all(g.has_edge(a, b) for a, b in zip(names, names[1:])), name
        else:  # acyclic: the chain finding iff the golden has it, with as many nodes
            assert (long_ in got) == (long_ in want), name
            if long_ in got:
                seen["chain"] += 1
                path = got[long_]["evidence"][len("Long dependency path: "):].split(" → ")
                assert len(path) == len(want[long_]["evidence"][len("Long dependency path: "):].split(" → ")), name
                assert all(g.has_edge(a, b) for a, b in zip(path, path[1:])), name
                assert s["longest_chain_exact"] and s["longest_chain"] == len(path)
        # everything the structure path does not touch is the golden's
        other = lambda fs: [f for f in A.normalize(A.strip(fs)) if f["issue"] not in (circ, long_)]  # noqa: E731
        assert other(res["findings"]) == other(case["result"]["findings"]), name
    return seen


def test_topology_agent_structure_path_on_the_goldens():
    seen = check_topology_structure(RestatingEngine())
    assert seen["cycle"] >= 1 and seen["chain"] >= 1  # the goldens exercise both findings
    assert A.check_topology(RestatingEngine()) == []  # structure=False: the goldens, unchanged


def test_new_symbols_sizes_and_einval_without_a_device():
    lib = native.load_library()
    for fn in ("krca_graph_scc", "krca_graph_chain", "krca_graph_cycle", "krca_graph_scc_ws_size",
               "krca_graph_chain_ws_size", "krca_graph_cycle_ws_size"):
        assert hasattr(lib, fn) and fn in native.SIGNATURES
    for n in (0, 1, 1000, 2**31 - 2):
        assert lib.krca_graph_scc_ws_size(n) >= 8 * n
        assert lib.krca_graph_chain_ws_size(n) >= 12 * n
        assert lib.krca_graph_cycle_ws_size(n) >= 12 * n
    v = ctypes.c_int32(-1)
    assert lib.krca_tune_get(b"KRCA_GRAPH_GRID", ctypes.byref(v)) == 0 and v.value == 0
    stats, cstats = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 2)()
    for n in (-1, 2**31 - 1, 2**40):
        assert lib.krca_graph_scc(None, None, n, 0, None, None, None, stats, None, None) == -22
        assert b"krca_graph_scc" in lib.krca_last_error()
        assert lib.krca_graph_chain(None, None, n, 0, None, None, None, None, None, cstats, None, None) == -22
        assert lib.krca_graph_cycle(None, None, n, 0, None, 0, None, None, None, None) == -22
    assert lib.krca_graph_scc(None, None, 5, 2, None, None, None, stats, None, None) == -22  # pull in {0, 1}
    # N = 0: the empty answer, no device work, no pointer touched
    assert lib.krca_graph_scc(None, None, 0, 0, None, None, None, stats, None, None) == 0
    assert list(stats) == [0, 0, 0, 0, -1, 0]
    assert lib.krca_graph_chain(None, None, 0, 1, None, None, None, None, None, cstats, None, None) == 0
    assert list(cstats) == [0, -1]
    assert lib.krca_graph_cycle(None, None, 0, 0, None, 0, None, None, None, None) == 0
