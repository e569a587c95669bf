"""Host restatement of krca_graph_reach / krca_graph_reach_cover (include/krca.h g1), worded after the
header: the edge set of graph_structure_ref.edge_list, one np.bitwise_or.at per BFS level over a
uint64 word per node, the histograms counted per level, the greedy cover as a loop.
Tests only; tests/test_blast_cpu.py checks it against networkx itself."""
import numpy as np

import graph_structure_ref as R

DEPENDENTS, DEPENDENCIES = 0, 1
KEYS = ("reach", "hist", "hist_marked", "depth", "order", "gain", "exclusive", "totals")


def _marked(mark, n):
    return np.ones(n, bool) if mark is None else np.asarray(mark).reshape(-1)[:n] != 0


def reach(row_ptr, col, pull, sources, direction=DEPENDENTS, max_hops=0, mark=None, bins=16):
    """-> (reach uint64 [N], hist int64 [2][K][H], depth int32 [K])."""
    n = len(row_ptr) - 1
    src, dst, _ = R.edge_list(row_ptr, col, pull)
    sender, receiver = (src, dst) if direction == DEPENDENCIES else (dst, src)  # bits flow sender -> receiver
    sources = np.asarray(sources, np.int64)
    K, H = len(sources), int(bins)
    marked = _marked(mark, n)
    seen = np.zeros(n, np.uint64)
    np.bitwise_or.at(seen, sources, np.uint64(1) << np.arange(K, dtype=np.uint64))
    hist = np.zeros((2, K, H), np.int64)
    depth = np.zeros(K, np.int32)
    shifts = np.arange(K, dtype=np.uint64)

    def tally(new, level):
        has = ((new[:, None] >> shifts[None, :]) & np.uint64(1)).astype(bool)  # [N][K]
        h = min(level, H - 1)
        hist[0, :, h] += has.sum(0)
        hist[1, :, h] += has[marked].sum(0)
        depth[has.any(0)] = level

    front, level = seen.copy(), 0
    tally(front, 0)
    while front.any() and (max_hops <= 0 or level < max_hops):
        level += 1
        nxt = np.zeros(n, np.uint64)
        np.bitwise_or.at(nxt, receiver, front[sender])
        front = nxt & ~seen
        seen |= front
        tally(front, level)
    return seen, hist, depth


def cover(reach_words, mark, K):
    """-> (order int32 [K], gain int64 [K], exclusive int64 [K], totals int64 [2])."""
    reach_words = np.asarray(reach_words, np.uint64)
    n = len(reach_words)
    marked = _marked(mark, n)
    full = np.uint64((1 << K) - 1)
    words = (reach_words & full)[marked]
    order, gain = np.full(K, -1, np.int32), np.zeros(K, np.int64)
    exclusive = np.array([(words == np.uint64(1 << k)).sum() for k in range(K)], np.int64)
    totals = np.array([len(words), (words != 0).sum()], np.int64)
    left = words
    for j in range(K):
        counts = [int(((left >> np.uint64(k)) & np.uint64(1)).sum()) for k in range(K)]
        best = int(np.argmax(counts))  # the first (lowest k) of the largest
        if counts[best] == 0:
            break
        order[j], gain[j] = best, counts[best]
        left = left[((left >> np.uint64(best)) & np.uint64(1)) == 0]
    return order, gain, exclusive, totals


def restate(row_ptr, col, pull, sources, direction=DEPENDENTS, max_hops=0, mark=None, bins=16):
    """-> dict over KEYS."""
    words, hist, depth = reach(row_ptr, col, pull, sources, direction, max_hops, mark, bins)
    order, gain, exclusive, totals = cover(words, mark, len(sources))
    return dict(reach=words, hist=hist[0].copy(), hist_marked=hist[1].copy(), depth=depth, order=order, gain=gain,
                exclusive=exclusive, totals=totals)


def as_blast(o, sources, direction="dependents", max_hops=0):
    """krca.blast.BlastRadius from restate()'s dict (what NativeEngine.blast_radius returns)."""
    from krca.blast import BlastRadius
    return BlastRadius(o["reach"], o["hist"], o["hist_marked"], o["depth"], o["order"], o["gain"], o["exclusive"],
                       int(o["totals"][0]), int(o["totals"][1]), np.asarray(sources, np.int32), direction, int(max_hops))


def blast_arrays(br):
    """The same dict from a BlastRadius the engine returned (for bit-for-bit comparison)."""
    return dict(reach=br.reach, hist=br.hist, hist_marked=br.hist_marked, depth=br.depth, order=br.order, gain=br.gain,
                exclusive=br.exclusive, totals=np.array([br.n_marked, br.n_covered], np.int64))
