"""Blast radius on the device (csrc/graph_reach.hip): reach, both histograms, depth and the cover's
order / gain / exclusive / totals of krca_graph_reach / krca_graph_reach_cover bit for bit against
tests/blast_ref.py, in both CSR layouts and both directions; refusals under a guard band; poisons; the
Coordinator's `blast_radius` key."""
import ctypes

import numpy as np
import pytest

import agent_cases as A
import blast_ref as B
import graph_structure_ref as R
from guarded import GuardedEngine, run_poisons
from krca import native
from test_blast_cpu import NS, check_blast_key, csr, mesh_case

pytestmark = pytest.mark.gpu

DIRS = ((B.DEPENDENTS, "dependents"), (B.DEPENDENCIES, "dependencies"))


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


@pytest.fixture(scope="module")
def geng():
    return GuardedEngine()


def same(ref, got, what):
    for k in B.KEYS:
        w, g = np.asarray(ref[k]), np.asarray(got[k])
        assert w.dtype == g.dtype and w.shape == g.shape, (k, what, w.dtype, g.dtype, w.shape, g.shape)
        assert w.tobytes() == g.tobytes(), (k, what, np.argwhere(w != g)[:5].tolist(), w[w != g][:5], g[w != g][:5])


def check(eng, rp, col, pull, sources, mark=None, bins=16, max_hops=0):
    """Both directions, each in the given layout and in the transposed one: all equal the restatement
    (hence each other) byte for byte.  -> {direction code: restated dict}."""
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int32)
    rp_t, col_t = R.transpose_csr(rp, col)
    out = {}
    for d, name in DIRS:
        ref = out[d] = B.restate(rp, col, pull, sources, d, max_hops, mark, bins)
        for a, b, p in ((rp, col, pull), (rp_t, col_t, not pull)):
            br = eng.blast_radius(a, b, sources, mark=mark, pull=p, direction=name, max_hops=max_hops, bins=bins)
            same(ref, B.blast_arrays(br), (name, "pull" if p else "push"))
    return out


def random_case(n, per_node, seed, k=64):
    rp, col = R.random_digraph(n, per_node, seed)
    rng = np.random.default_rng(1000 + seed)
    return rp, col, rng.integers(0, n, k).astype(np.int32), (rng.random(n) < 0.05).astype(np.uint8)


# ---- trivial shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,edges", [(1, []), (1, [(0, 0)]), (2, [(0, 1), (1, 0)])])
def test_trivial(eng, n, edges):
    out = check(eng, *csr(n, edges), False, [0], bins=2)
    for d, _ in DIRS:
        assert out[d]["hist"].tolist() == [[1, n - 1]] and out[d]["depth"].tolist() == [n - 1]
        assert out[d]["order"].tolist() == [0] and out[d]["gain"].tolist() == [n]


def test_invalid_arguments_leave_reach_untouched(eng):
    torch = eng.torch
    n = 50
    rp, col = csr(n, [(i, (i + 1) % n) for i in range(n)])
    rp_d, col_d = eng._dev_n(rp, np.int64), eng._dev_n(col, np.int32)
    band = torch.full((n + 128,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=eng.device)
    before = band.clone()
    reach = band[64:64 + n]
    ws = torch.empty(int(eng.lib.krca_graph_reach_ws_size(n)), dtype=torch.uint8, device=eng.device)
    hist, depth = (ctypes.c_int64 * (2 * 64 * 64))(), (ctypes.c_int32 * 64)()
    src = (ctypes.c_int32 * 65)()

    def call(K=1, H=16, direction=0, s0=0):
        src[0] = s0
        return eng.lib.krca_graph_reach(eng.ptr(rp_d), eng.ptr(col_d), n, 0, src, K, direction, 0, None, H, eng.ptr(ws),
                                        eng.ptr(reach), hist, depth, None, eng._stream())
    for kw in (dict(K=0), dict(K=65), dict(H=1), dict(direction=2), dict(s0=-1), dict(s0=n)):
        assert call(**kw) == -22, kw
        assert b"krca_graph_reach" in eng.lib.krca_last_error()
        torch.cuda.synchronize()
        assert torch.equal(band, before), kw
    assert call() == 0  # the same buffers, valid arguments: the ring from node 0, and only reach is written
    torch.cuda.synchronize()
    assert torch.equal(band[:64], before[:64]) and torch.equal(band[64 + n:], before[64 + n:])
    assert reach.cpu().tolist() == [1] * n and depth[0] == n - 1


# ---- source counts ------------------------------------------------------------------------------------
def test_one_source_and_sixty_four(eng):
    rp, col, src, mark = random_case(257, 3.0, 5)
    out = check(eng, rp, col, False, src[:1], mark)
    assert int(out[B.DEPENDENCIES]["reach"].max()) == 1
    src = np.arange(64, dtype=np.int32) * 4  # distinct sources: bit 63 is source 252's alone
    out = check(eng, rp, col, False, src, mark)
    for d, _ in DIRS:
        words = out[d]["reach"]
        assert words[252] >> np.uint64(63) == 1 and (words.view(np.int64) < 0).sum() > 1  # the sign bit travels
        assert out[d]["hist"][63].sum() == (words >> np.uint64(63)).sum() > 1
    # a cover that needs bit 63: only source 63 reaches an otherwise isolated marked pair
    n = 80
    rp, col = csr(n, [(i, i + 1) for i in range(60)] + [(78, 79)])
    src = np.concatenate([np.arange(63), [78]]).astype(np.int32)
    out = check(eng, rp, col, False, src, None)
    o = out[B.DEPENDENCIES]
    assert o["order"][:2].tolist() == [0, 63] and o["gain"][:2].tolist() == [61, 2] and o["exclusive"][63] == 2


def test_duplicate_sources(eng):
    rp, col, _, mark = random_case(257, 1.5, 6)
    src = np.array([7, 100, 7, 7, 200, 100], np.int32)
    out = check(eng, rp, col, False, src, mark)
    for d, _ in DIRS:
        o = out[d]
        for a, b in ((0, 2), (0, 3), (1, 5)):
            assert np.array_equal((o["reach"] >> np.uint64(a)) & np.uint64(1), (o["reach"] >> np.uint64(b)) & np.uint64(1))
            assert o["hist"][a].tolist() == o["hist"][b].tolist() and o["depth"][a] == o["depth"][b]
            assert o["exclusive"][a] == 0 and o["exclusive"][b] == 0


# ---- as many levels as nodes; the clamp and the cut ----------------------------------------------------
@pytest.mark.parametrize("max_hops", [0, 5, 6, 7])
def test_chain(eng, max_hops):
    """70 nodes in a row, H = 8: the last bin accumulates, the cut is exact, and the 70-level host loop
    crosses its read-back batches (2, 4, 8, 16, 32 rounds)."""
    n = 70
    perm = np.random.default_rng(3).permutation(n)
    rp, col = csr(n, [(int(perm[i]), int(perm[i + 1])) for i in range(n - 1)])
    mark = (np.arange(n) % 2).astype(np.uint8)
    out = check(eng, rp, col, False, [int(perm[0]), int(perm[n - 1]), int(perm[30])], mark, bins=8, max_hops=max_hops)
    o = out[B.DEPENDENCIES]
    far = max_hops if max_hops else n - 1
    assert o["depth"].tolist() == [far, 0, min(far, n - 1 - 30)]
    assert o["hist"][0].tolist() == [int(h <= far) for h in range(7)] + [max(far - 6, 0)]
    assert sorted(np.flatnonzero(o["reach"] & np.uint64(1)).tolist()) == sorted(perm[:far + 1].tolist())


# ---- random graphs around the giant-component threshold, duplicates and stray columns --------------------
@pytest.mark.parametrize("per_node", [1.0, 1.5, 3.0])
@pytest.mark.parametrize("n", [63, 64, 65, 257, 4097])
def test_random(eng, n, per_node):
    rp, col, src, mark = random_case(n, per_node, n % 7)
    assert R.edge_list(rp, col, False)[2] >= 1  # stray columns are in
    out = check(eng, rp, col, False, src, mark)
    assert out[B.DEPENDENTS]["totals"][0] == mark.sum()


@pytest.mark.parametrize("n", [20_000, 262_145])
def test_read_back_batches(eng, n):
    """The host loop reads back after up to 32 levels below 16 384 nodes, up to 4 below 262 144 and after
    every level from there on: one graph in each of the two upper classes."""
    rp, col, src, mark = random_case(n, 1.5, 3, k=10)
    out = check(eng, rp, col, False, src, mark)
    assert out[B.DEPENDENCIES]["depth"].max() >= 8  # several batches


def test_dense_rows(eng):
    """40 entries per row on average: at 32 or more a wave walks each row (16 lanes below)."""
    rp, col, src, mark = random_case(257, 40.0, 4)
    out = check(eng, rp, col, False, src, mark)
    assert out[B.DEPENDENCIES]["hist"][:, :4].sum() >= 64 * 250


def test_random_with_a_capped_grid(eng):
    """KRCA_GRAPH_GRID = 3: three workgroups stride over 4 097 rows and nodes."""
    rp, col, src, mark = random_case(4097, 3.0, 1)
    with native.tune(eng.lib, KRCA_GRAPH_GRID=3):
        check(eng, rp, col, False, src, mark)


# ---- long rows and hubs ---------------------------------------------------------------------------------
def test_adjacent_long_rows(eng):
    """Four neighbouring rows of 600 to 900 entries in a graph of short rows (pull layout): asked for
    dependents the rows are the senders, and the 16-lane walk hands each long one to the whole wave."""
    n = 1000
    rng = np.random.default_rng(8)
    src = [rng.choice(np.arange(8, n), 600 + 100 * h, replace=False) for h in range(4)]
    dst = [np.full(len(x), h) for h, x in enumerate(src)]
    back_src, back_dst = np.array([0, 1, 2, 3, 4, 4]), np.array([500, 501, 0, 2, 3, 4])
    src, dst = np.concatenate(src + [back_src]), np.concatenate(dst + [back_dst])
    rp, col = R.csr_from_edges(n, dst, src)  # rows = callees
    assert np.diff(rp)[:4].min() > 512 and rp[-1] < 32 * n
    mark = (rng.random(n) < 0.3).astype(np.uint8)
    out = check(eng, rp, col, True, [0, 1, 2, 3, 4, 500, 999], mark)
    assert out[B.DEPENDENTS]["hist"][0, 1] >= 600  # hub 0's callers, one level


def test_hub_with_marked_callers(eng):
    """source 0 <- 1 <- hub 2 <- 5 000 marked callers: one level gains 5 000 marked nodes for one bit."""
    n = 5003
    callers = np.arange(3, n)
    src = np.concatenate([[1, 2], callers])
    dst = np.concatenate([[0, 1], np.full(len(callers), 2)])
    rp, col = R.csr_from_edges(n, dst, src)  # rows = callees: the hub's row has 5 000 entries
    mark = np.zeros(n, np.uint8)
    mark[3:] = 1
    out = check(eng, rp, col, True, [0, 2, 4], mark, bins=4)
    o = out[B.DEPENDENTS]
    assert o["hist"][0].tolist() == [1, 1, 1, 5000] and o["hist_marked"][0].tolist() == [0, 0, 0, 5000]
    assert o["order"].tolist() == [0, -1, -1] and o["gain"].tolist() == [5000, 0, 0] and o["depth"].tolist() == [3, 1, 0]


# ---- cover ----------------------------------------------------------------------------------------------
def test_cover_skips_a_radius_inside_another(eng):
    # callers -> callees: 3, 4 -> 1 -> 0;  5 -> 0;  6 -> 2.  Dependents of 0 include all of 1's.
    rp, col = csr(7, [(3, 1), (4, 1), (1, 0), (5, 0), (6, 2)])
    out = check(eng, rp, col, False, [0, 1, 2], None)
    o = out[B.DEPENDENTS]
    assert o["order"].tolist() == [0, 2, -1] and o["gain"].tolist() == [5, 2, 0]
    assert o["exclusive"].tolist() == [2, 0, 2] and o["totals"].tolist() == [7, 7]


def test_mark_none_is_all_ones(eng):
    rp, col, src, _ = random_case(257, 1.5, 9)
    a = eng.blast_radius(rp, col, src, mark=None, pull=False)
    b = eng.blast_radius(rp, col, src, mark=np.ones(257, np.uint8), pull=False)
    same(B.blast_arrays(a), B.blast_arrays(b), "mark")
    assert np.array_equal(a.hist, a.hist_marked) and a.n_marked == 257


def test_score_and_floor_make_the_mark(eng):
    rp, col, src, _ = random_case(257, 1.5, 9)
    src[5] = -1  # a top-k with fewer than k keys
    score = np.random.default_rng(2).random(257).astype(np.float32) * 10
    br = eng.blast_radius(rp, col, src, score=eng._dev(score), floor=7.5, pull=False)
    kept = src[src != -1]
    assert br.sources.tolist() == kept.tolist()
    same(B.restate(rp, col, False, kept, B.DEPENDENTS, 0, score > np.float32(7.5), 16), B.blast_arrays(br), "score")


# ---- buffers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pull", [False, True])
def test_guard_bands_and_poisons(geng, pull):
    rp, col, src, mark = random_case(4097, 1.5, 2)
    if pull:
        rp, col = R.transpose_csr(rp, col)
    for d, name in DIRS:
        ref = B.restate(rp, col, pull, src, d, 0, mark, 16)
        out = run_poisons(geng, lambda e: B.blast_arrays(e.blast_radius(rp, col, src, mark=mark, pull=pull,
                                                                        direction=name)))
        same(ref, out, (name, pull))


# ---- end to end ---------------------------------------------------------------------------------------------
def test_coordinator_blast_radius_end_to_end(eng):
    from krca.agents.coordinator import Coordinator
    from krca.mock import MeshClient
    from krca.rca import RANKING
    m, x = mesh_case(256)
    xd = eng._dev(x)
    plain = A.strip(Coordinator(MeshClient(m, xd), engine=eng).run_analysis("comprehensive", NS))
    res = A.strip(Coordinator(MeshClient(m, xd), engine=eng, blast_radius=True).run_analysis("comprehensive", NS))
    assert "error" not in plain and "error" not in res and "blast_radius" not in plain
    key = res.pop("blast_radius")
    assert res == plain and len(res["ranked_root_causes"]) > 0
    names = m.names()
    ranked = [names.index(r["component"][len("Pod/"):]) for r in res["ranked_root_causes"]]
    score = eng.rolling_score_device(xd, RANKING.window, RANKING.z_threshold)["score"].cpu().numpy()
    mark = score > np.float32(RANKING.floor(len(names), x.shape[2]))
    check_blast_key(key, names, m.row_ptr, m.col, ranked, mark, 16)
