"""Host restatement of krca_graph_scc / krca_graph_chain / krca_graph_cycle (include/krca.h g1): scipy's
strong components relabelled to the minimum id, a level peel of the condensation for both depths, and
the `next` / `hop` rules as the header words them.  Vectorised: a 70 000-node mesh costs about a second.
Tests only; tests/test_graph_structure_cpu.py checks it against networkx itself."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components, shortest_path

INF = np.iinfo(np.int32).max


def edge_list(row_ptr, col, pull):
    """-> (src, dst int64 arrays of the valid edges u -> v in CSR order, n_bad)."""
    row_ptr = np.asarray(row_ptr, np.int64)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    c = np.asarray(col, np.int32)[:int(row_ptr[-1]) if n >= 0 and len(row_ptr) else 0].astype(np.int64)
    ok = (c >= 0) & (c < n)
    src, dst = (c[ok], rows[ok]) if pull else (rows[ok], c[ok])
    return src, dst, int((~ok).sum())


def transpose_csr(row_ptr, col):
    """The same edge set in the other layout.  Entries outside [0, N) are no edges: they stay in the
    row they were in (they only have to be counted again)."""
    row_ptr = np.asarray(row_ptr, np.int64)
    n = len(row_ptr) - 1
    col = np.asarray(col, np.int32)[:int(row_ptr[-1])]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    c = col.astype(np.int64)
    ok = (c >= 0) & (c < n)
    new_row = np.where(ok, c, rows)
    new_col = np.where(ok, rows, c).astype(np.int32)
    order = np.argsort(new_row, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    if len(new_row):
        np.cumsum(np.bincount(new_row, minlength=n), out=rp[1:])
    return rp, new_col[order]


def csr_from_edges(n, src, dst):
    """Out-edge CSR (pull = 0) of an edge list, edges kept in order inside a row."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.argsort(src, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    if len(src):
        np.cumsum(np.bincount(src, minlength=n), out=rp[1:])
    return rp, dst[order].astype(np.int32)


def _peel(n, reps, es, ed):
    """depth[x] = 1 + max depth over the edges x -> y (1 without one), for x in reps, by peeling levels."""
    depth = np.zeros(n, np.int32)
    deg = np.bincount(es, minlength=n) if len(es) else np.zeros(n, np.int64)
    frontier = reps[deg[reps] == 0]
    isf = np.zeros(n, bool)
    level = 1
    while len(frontier):
        depth[frontier] = level
        isf[frontier] = True
        hit = isf[ed]
        isf[frontier] = False
        u, cnt = np.unique(es[hit], return_counts=True)
        deg[u] -= cnt
        frontier = u[deg[u] == 0]
        es, ed = es[~hit], ed[~hit]
        level += 1
    assert len(es) == 0, "the condensation has a cycle"
    return depth


def restate(row_ptr, col, pull=False, root="first"):
    """-> dict: comp, flags, scc_stats [6], depth_dn, depth_up, next, chain_stats [2], root, hop
    (root="first": first_cyclic_label, hop all -1 when there is none; an int: that root)."""
    n = len(row_ptr) - 1
    src, dst, n_bad = edge_list(row_ptr, col, pull)
    ids = np.arange(n, dtype=np.int64)
    out = {}
    if n == 0:
        z = np.zeros(0, np.int32)
        return dict(comp=z, flags=np.zeros(0, np.uint8), scc_stats=np.array([0, 0, 0, 0, -1, n_bad], np.int64),
                    depth_dn=z, depth_up=z, next=z, chain_stats=np.array([0, -1], np.int64), root=-1, hop=z)
    loop = np.zeros(n, bool)
    loop[src[src == dst]] = True
    if len(src):  # distinct edges: duplicates change nothing below
        key = np.unique(src * n + dst)
        src, dst = key // n, key % n
    a = csr_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(n, n))
    _, lab = connected_components(a, directed=True, connection="strong")
    _, first = np.unique(lab, return_index=True)  # ids ascend: the first occurrence is the minimum id
    comp = first[lab].astype(np.int64)
    size = np.bincount(lab)[lab]
    cyc = (size >= 2) | loop
    rep = comp == ids
    out["comp"] = comp.astype(np.int32)
    out["flags"] = (cyc * 1 + loop * 2 + rep * 4).astype(np.uint8)
    cyc_reps = ids[rep & cyc]
    out["scc_stats"] = np.array([rep.sum(), len(cyc_reps), cyc.sum(), size.max(),
                                 cyc_reps[0] if len(cyc_reps) else -1, n_bad], np.int64)
    # condensation
    es, ed = comp[src], comp[dst]
    keep = es != ed
    es, ed = es[keep], ed[keep]
    if len(es):
        key = np.unique(es * n + ed)
        es, ed = key // n, key % n
    reps = ids[rep]
    ddn = _peel(n, reps, es, ed)
    dup = _peel(n, reps, ed, es)
    nx = np.full(n, INF, np.int64)
    sel = ddn[ed] == ddn[es] - 1
    np.minimum.at(nx, es[sel], ed[sel])
    nx[nx == INF] = -1
    out["depth_dn"], out["depth_up"], out["next"] = ddn[comp], dup[comp], nx[comp].astype(np.int32)
    longest = int(ddn.max())
    out["chain_stats"] = np.array([longest, int(np.flatnonzero(rep & (ddn == longest))[0])], np.int64)
    # witness cycle
    if root == "first":
        root = int(out["scc_stats"][4])
    out["root"] = int(root)
    hop = np.full(n, -1, np.int32)
    if root >= 0:
        inside = (comp[src] == comp[root]) & (comp[dst] == comp[root])
        s, d = src[inside], dst[inside]
        back = csr_matrix((np.ones(len(s), np.int8), (d, s)), shape=(n, n))  # reversed edges
        dist = shortest_path(back, method="D", unweighted=True, indices=int(root))
        dist = np.where(np.isfinite(dist), dist, -1).astype(np.int64)  # d(v): v -> root
        # v != root: the smallest-id successor one step closer
        m = (s != root) & (dist[d] == dist[s] - 1)
        best = np.full(n, INF, np.int64)
        np.minimum.at(best, s[m], d[m])
        # root: the successor with the smallest d, ties to the smallest id
        m = s == root
        if m.any():
            k = dist[d[m]] * (1 << 32) + d[m]
            best[root] = int(k.min()) & 0xFFFFFFFF
        hop = np.where(best == INF, -1, best).astype(np.int32)
    out["hop"] = hop
    return out


def is_path(src, dst, nodes, closed=False):
    """Every consecutive pair of `nodes` (and the last back to the first when closed) is an edge."""
    edges = set(zip(np.asarray(src).tolist(), np.asarray(dst).tolist()))
    pairs = list(zip(nodes, nodes[1:])) + ([(nodes[-1], nodes[0])] if closed else [])
    return all(p in edges for p in pairs)


def random_digraph(n, edges_per_node, seed, dup=0.01, bad=0.01):
    """Out-edge CSR of a seeded random digraph: n * edges_per_node edges (self-loops allowed), a share
    `dup` of them duplicated, then a share `bad` of the col entries set to -1, N, 2^31 - 1 or -2^31."""
    rng = np.random.default_rng(seed)
    e = int(round(n * edges_per_node))
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    k = int(np.ceil(dup * e))
    pick = rng.integers(0, e, k)
    src, dst = np.concatenate([src, src[pick]]), np.concatenate([dst, dst[pick]])
    rp, col = csr_from_edges(n, src, dst)
    nb = int(np.ceil(bad * len(col)))
    where = rng.choice(len(col), nb, replace=False)
    col[where] = np.array([-1, n, 2**31 - 1, -2**31], np.int64)[rng.integers(0, 4, nb)].astype(np.int32)
    return rp, col


def reversed_mesh(n_pods, k, seed=0):
    """synth.make_graph(n_pods, seed) with k randomly chosen edges reversed (back edges): pull-CSR."""
    from krca import synth
    m = synth.make_graph(n_pods, seed=seed)
    if k == 0:
        return m.row_ptr, m.col
    src, dst, _ = edge_list(m.row_ptr, m.col, True)
    pick = np.random.default_rng(seed + 7).choice(len(src), k, replace=False)
    src, dst = src.copy(), dst.copy()
    src[pick], dst[pick] = dst[pick], src[pick]
    rp, col = csr_from_edges(n_pods, dst, src)  # rows = destinations: the pull layout
    return rp, col


def as_structure(o, chain=True, cycle=True):
    """krca.graphstruct.GraphStructure from restate()'s dict (what NativeEngine.graph_structure returns)."""
    from krca.graphstruct import GraphStructure
    gs = GraphStructure(len(o["comp"]), o["comp"], o["flags"], *(int(x) for x in o["scc_stats"]))
    if chain:
        gs.depth_dn, gs.depth_up, gs.next = o["depth_dn"], o["depth_up"], o["next"]
        gs.longest, gs.start = int(o["chain_stats"][0]), int(o["chain_stats"][1])
    if cycle:
        gs.root, gs.hop = int(o["root"]), o["hop"]
    return gs


STRUCT_KEYS = ("comp", "flags", "scc_stats", "depth_dn", "depth_up", "next", "chain_stats", "root", "hop")


def structure_arrays(gs):
    """The same dict from a GraphStructure the engine returned (for bit-for-bit comparison)."""
    return dict(comp=gs.comp, flags=gs.flags,
                scc_stats=np.array([gs.n_components, gs.n_cyclic, gs.n_cyclic_nodes, gs.largest_size,
                                    gs.first_cyclic_label, gs.n_bad_edges], np.int64),
                depth_dn=gs.depth_dn, depth_up=gs.depth_up, next=gs.next,
                chain_stats=np.array([gs.longest, gs.start], np.int64), root=np.int64(gs.root), hop=gs.hop)
