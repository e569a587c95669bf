"""krca_trace_critical on the device (csrc/trace_critical.hip): every output bit-exact against
tests/trace_critical_ref.py."""
import numpy as np
import pytest

import agent_cases as A
import trace_critical_ref as R
import trace_ref
from guarded import GuardedEngine, run_poisons
from krca import native, tracecols
from krca.agents.traces import TracesAgent
from test_gpu_trace import _link_case
from test_trace_cpu import ColumnsClient

pytestmark = pytest.mark.gpu
NAMES = ("crit_us", "path", "n_bad")
LIM = 2 ** 62


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


@pytest.fixture(scope="module")
def small_max(eng):
    return int(eng.lib.krca_trace_critical_small_max())


def check(eng, svc, parent, start, dur, S, ref=None):
    got = eng.trace_critical(svc, parent, start, dur, S)
    ref = R.critical(svc, parent, start, dur, S) if ref is None else ref
    for g, r, what in zip(got, ref, NAMES):
        assert np.array_equal(g, r), what
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint8
    return got


def _case(N, seed=0):
    """_link_case's garbage (self parents, parents out of range both ways, bad services used as
    parents, random parent indices with cycles, dur = 2^32 - 1) plus starts: most inside one
    stretch so that intervals overlap, some at both ends of the valid range and just outside."""
    svc, parent, dur, _, S = _link_case(N, seed=seed)
    rng = np.random.default_rng(1000 + seed + N)
    start = rng.integers(-2 ** 19, 2 ** 21, N).astype(np.int64)
    kind = rng.random(N)
    for lo, v in ((0.00, -LIM), (0.01, LIM - 1), (0.02, LIM), (0.03, -LIM - 1), (0.04, LIM - 2 ** 32), (0.05, 2 ** 63 - 1),
                  (0.055, -2 ** 63)):
        start[(kind >= lo) & (kind < lo + 0.01)] = v
    return svc, parent, start, dur, S


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 70_000])
def test_garbage(eng, N):
    svc, parent, start, dur, S = _case(N)
    crit, path, n_bad = check(eng, svc, parent, start, dur, S)
    if N >= 257:
        assert n_bad > 0 and {0, 3, 6} <= set(np.unique(path).tolist())
        assert (crit[(path & 2) == 0] == 0).all()
    if N == 70_000:
        assert n_bad > trace_ref.link(svc, parent, dur, np.zeros(N, np.uint8), S)[3]  # bad by start alone as well
        assert ((path == 1).sum() > 100)  # selected but off the path: hidden parents and cycles


def _family(rng, n_children, p_start, p_dur, div=40):
    """Children of a parent [p_start, p_start + p_dur): random intervals, some reaching out at either end."""
    s = rng.integers(p_start - p_dur // 20, p_start + p_dur, n_children)
    d = rng.integers(0, max(p_dur // div, 2), n_children)
    return s, d


def test_one_parent_with_5000_children(eng, small_max):
    rng = np.random.default_rng(5)
    n = 5000
    assert n > small_max
    s, d = _family(rng, n, 10 ** 6, 10 ** 6, div=200)
    s[(s < 1_500_000) & (s + d > 1_500_000)] = 1_500_000  # nobody straddles the shared end: the cursor stops on it
    same_end = rng.choice(n, 300, replace=False)  # a few hundred share one end time ...
    d[same_end] = rng.integers(1, 3000, 300)
    d[same_end[:20]] = 3000  # ... and twenty of them one interval, the earliest start of that end
    s[same_end] = 1_500_000 - d[same_end]
    start = np.concatenate([[10 ** 6], s]).astype(np.int64)
    dur = np.concatenate([[10 ** 6], d]).astype(np.uint32)
    parent = np.concatenate([[-1], np.zeros(n)]).astype(np.int32)
    perm = rng.permutation(n + 1)  # the parent somewhere in the middle
    inv = np.argsort(perm)
    parent = np.where(parent[perm] >= 0, inv[0], -1).astype(np.int32)
    crit, path, _ = check(eng, np.zeros(n + 1, np.int32), parent, start[perm], dur[perm], 1)
    n_sel = int((path & 1).sum())
    assert 50 < n_sel < n and path[inv[0]] == 6
    twins = np.sort(inv[1 + same_end[:20]])
    assert path[twins[0]] & 1 and not (path[twins[1:]] & 1).any()  # the lowest index of identical intervals
    assert int(crit.astype(np.int64).sum()) >= 10 ** 6  # overrunning children keep their own time


def test_child_counts_around_small_max_and_across_a_wave(eng, small_max):
    """Parents with small_max - 1, small_max and small_max + 1 children (the last is the workgroup
    path's), then 64 consecutive parents with 0 .. 63 children: one wave's lanes, every count."""
    rng = np.random.default_rng(9)
    counts = [small_max - 1, small_max, small_max + 1] + list(range(64))
    P = len(counts)
    p_start = rng.integers(0, 10 ** 6, P)
    p_dur = rng.integers(10 ** 4, 10 ** 5, P)
    parent, start, dur = [np.full(P, -1)], [p_start], [p_dur]
    for p, c in enumerate(counts):
        s, d = _family(rng, c, int(p_start[p]), int(p_dur[p]))
        parent.append(np.full(c, p))
        start.append(s)
        dur.append(d)
    parent, start, dur = np.concatenate(parent), np.concatenate(start), np.concatenate(dur)
    N = len(parent)
    got = check(eng, np.zeros(N, np.int32), parent.astype(np.int32), start.astype(np.int64), dur.astype(np.uint32), 1)
    # back to back children: every one selected, whatever the count
    for p, c in enumerate(counts):
        kids = np.flatnonzero(parent == p)
        dur[kids] = p_dur[p] // max(c, 1)
        start[kids] = p_start[p] + np.arange(c) * (p_dur[p] // max(c, 1))
    crit, path, _ = check(eng, np.zeros(N, np.int32), parent.astype(np.int32), start.astype(np.int64),
                          dur.astype(np.uint32), 1)
    assert (path[P:] == 3).all() and (path[:P] == 6).all()
    assert int(crit.astype(np.int64).sum()) == int(p_dur.sum()) and got[2] == 0


def test_chain_deeper_than_the_limit(eng):
    D = int(eng.lib.krca_trace_critical_max_depth())
    assert D == R.D
    n = D + 2
    parent = np.arange(-1, n - 1, dtype=np.int32)
    start, dur = np.zeros(n, np.int64), np.full(n, 10, np.uint32)
    crit, path, _ = check(eng, np.zeros(n, np.int32), parent, start, dur, 1)
    assert path[D] == 3 and path[D + 1] == 1 and path[0] == 6
    leaf_first = np.arange(1, n + 1, dtype=np.int32)  # the same chain stored leaf first
    leaf_first[-1] = -1
    crit, path, _ = check(eng, np.zeros(n, np.int32), leaf_first, start, dur, 1)
    assert path[n - 1 - D] == 3 and path[0] == 1 and path[n - 1] == 6


def _per_trace_sums(cols, crit):
    top = np.arange(len(cols))
    for _ in range(8):
        top = np.where(cols.parent[top] >= 0, cols.parent[top], top)
    return np.bincount(top, crit.astype(np.int64), len(cols))


@pytest.fixture(scope="module")
def mesh():
    return tracecols.make_spans(20_000, 200, seed=11)[0]


@pytest.mark.parametrize("p_parallel", [0.0, 0.5])
def test_critical_times_sum_to_the_root_durations(eng, mesh, p_parallel):
    cols = tracecols.add_starts(mesh, seed=3, p_parallel=p_parallel)
    assert R.nested(cols) and len(cols) > 200_000
    crit, path, n_bad = check(eng, cols.svc, cols.parent, cols.start_us, cols.dur_us, len(cols.services))
    roots = (path & 4) != 0
    assert n_bad == 0 and roots.sum() == 20_000
    assert np.array_equal(_per_trace_sums(cols, crit)[roots], cols.dur_us[roots])
    assert ((path & 2) != 0).all() == (p_parallel == 0)


def _tables_equal(got, ref, names):
    for name in names:
        assert np.array_equal(getattr(got, name + "_rec"), getattr(ref, name + "_rec")), name
        assert np.array_equal(getattr(got, name + "_q"), getattr(ref, name + "_q")), name


def test_trace_analyze_equals_the_reference_engine(eng):
    base, planted = tracecols.make_spans(2000, 60, seed=4)
    cols = tracecols.add_starts(base, seed=2, p_parallel=0.5)
    cols.svc[::97] = 99  # bad spans stay out of the critical tables too
    ref = R.NumpyTraceEngine().trace_analyze(cols)
    got = eng.trace_analyze(cols)
    assert got.n_bad == ref.n_bad > 0 and got.n_roots == ref.n_roots and np.array_equal(got.edge_key, ref.edge_key)
    _tables_equal(got, ref, ("svc", "self", "edge", "op", "crit", "critedge"))
    assert got.summary() == ref.summary() and got.summary()["critical_path"]
    assert ref.crit_rec[:, tracecols.R_N].sum() < ref.svc_rec[:, tracecols.R_N].sum()
    dev = TracesAgent(ColumnsClient(cols=cols), engine=eng).analyze("mesh")
    host = TracesAgent(ColumnsClient(cols=cols), engine=R.NumpyTraceEngine()).analyze("mesh")
    assert "error" not in dev and A.strip(dev) == A.strip(host) and dev["trace_stats"] == host["trace_stats"]
    # without the column: no critical tables, today's four
    plain = eng.trace_analyze(base)
    assert not plain.has_critical and "critical_path" not in plain.summary()
    _tables_equal(plain, trace_ref.NumpyTraceEngine().trace_analyze(base), ("svc", "self", "edge", "op"))


def test_second_window_merges_with_accumulate(eng):
    S = 40
    wins = [tracecols.add_starts(tracecols.make_spans(700, S, seed=20 + w)[0], seed=w, p_parallel=0.5) for w in range(2)]
    prev_dev = prev_ref = None
    for cols in wins:
        flags = trace_ref.link(cols.svc, cols.parent, cols.dur_us, cols.err, S)[2]
        crit, path, _ = eng.trace_critical(cols.svc, cols.parent, cols.start_us, cols.dur_us, S)
        rcrit, rpath, _ = R.critical(cols.svc, cols.parent, cols.start_us, cols.dur_us, S)
        rec, hist, q = eng.trace_stats(np.where(path & 2, cols.svc, -1), crit, flags, S, tracecols.PERMILLE,
                                       accumulate=prev_dev is not None, prev=prev_dev)
        rrec, rhist = trace_ref.stats(np.where(rpath & 2, cols.svc, -1), rcrit, flags, S, prev_ref)
        prev_dev, prev_ref = (rec, hist), (rrec, rhist)
        assert np.array_equal(rec, rrec) and np.array_equal(hist, rhist)
        assert np.array_equal(q, trace_ref.quantiles(rrec, rhist, tracecols.PERMILLE))
    both = sum(int((R.critical(c.svc, c.parent, c.start_us, c.dur_us, S)[1] & 2 != 0).sum()) for c in wins)
    assert int(prev_dev[0][:, tracecols.R_N].sum()) == both


@pytest.fixture(scope="module")
def geng():
    return GuardedEngine()


@pytest.mark.parametrize("N", [65, 257, 6000])
def test_guard_bands_and_poisons(geng, N):
    """Under GuardedEngine the workspace and both outputs are carved at exactly their sizes and filled
    with 0x00 / 0xFF / 0x5B: identical outputs, canaries intact, inputs unchanged."""
    svc, parent, start, dur, S = _case(N, seed=3)
    out = run_poisons(geng, lambda e: {k: np.asarray(v) for k, v in zip(NAMES, e.trace_critical(svc, parent, start, dur, S))})
    for name, r in zip(NAMES, R.critical(svc, parent, start, dur, S)):
        assert np.array_equal(out[name], r), name
    if N >= 6000:
        # the workgroup-per-parent path was guarded too
        assert np.bincount(parent[(parent >= 0) & (parent < N)]).max() > 100 * geng.lib.krca_trace_critical_small_max()


def test_two_launches_give_equal_bytes(eng):
    svc, parent, start, dur, S = _case(70_000, seed=1)
    a = eng.trace_critical(svc, parent, start, dur, S)
    b = eng.trace_critical(svc, parent, start, dur, S)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
