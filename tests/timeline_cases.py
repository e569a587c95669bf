"""Hand-made fixtures of the anomaly timeline, shared by tests/test_timeline_cpu.py (the reference
alone) and tests/test_gpu_timeline.py (the kernels against it)."""
import numpy as np

import timeline_ref as R
from agent_cases import DictClient

# ---- episode fixture ------------------------------------------------------------------------
W, THR, G, MINC = 10, 3.0, 3, 3
T, P, M = 130, 4, 4
# exceedance steps planted per (pod, metric); every other series is pure background
PLAN = {
    # pod 0: the anchor m0 has three sustained episodes of equal peak (windows of pure background in
    # the same phase before each), the first at the first evaluated step t = W; the last one wins
    (0, 0): [10, 11, 12, 40, 41, 42, 80, 81, 82],
    # gaps of exactly G continue (80, 83, 86: one episode of cnt R); a gap of G + 1 splits, and the
    # new episode has cnt R - 1 (not sustained); overlaps the anchor: a member
    (0, 1): [80, 83, 86, 90, 91],
    # a sustained episode far from the anchor's kept one: not a member
    (0, 2): [20, 21, 22],
    # pod 1: an episode that ends at T - 1
    (1, 3): [T - 3, T - 2, T - 1],
    # pod 2: nothing.  pod 3: exceedances but no sustained episode (cnt R - 1)
    (3, 1): [50, 52],
}


def plant(xs, steps, W_, thr=THR, strict=True):
    """In place: at each step (ascending) of the float64 series xs, add the smallest value of a fixed
    ladder that makes the step exceed, given the series so far (clipped at 100).  -> the steps planted."""
    done = []
    for t in steps:
        w = xs[t - W_:t]
        s1, s2 = w.sum(), (w * w).sum()
        B = W_ * s2 - s1 * s1
        for d in (4.0, 8.0, 16.0, 32.0, 64.0):
            v = min(xs[t] + d, 100.0)
            A = W_ * v - s1
            if B > 1e-12 * W_ * W_ and A * A - thr * thr * B > 0:
                xs[t] = v
                done.append(t)
                break
        else:
            assert not strict, f"no ladder value exceeds at step {t}"
    return done


def episode_fixture():
    """x float32 [T, P, M] (multiples of 1/16): background alternating 10 / 11, and at each planned
    step the smallest ladder value that exceeds."""
    x = np.empty((T, P, M), np.float32)
    x[0::2] = 10.0
    x[1::2] = 11.0
    for (p, m), steps in PLAN.items():
        xs = x[:, p, m].astype(np.float64)
        plant(xs, steps, W)
        x[:, p, m] = xs
    assert x.max() <= 100.0
    return x


# ---- known-answer graph ---------------------------------------------------------------------
# caller -> dependency.  2 -> 1 -> 0 chain (onsets 120 / 110 / 100) with the shortcut 2 -> 0; a self
# loop on 0; the pair 4 -> 3 three steps apart; 6 -> 5 -> 7 with 5 not anomalous; 6 calls 1 and 7,
# both earlier with the same onset (dep_first: the lower id); 7 -> 6: a caller earlier than its callee.
EDGES = [(2, 1), (1, 0), (0, 0), (2, 0), (4, 3), (6, 5), (5, 7), (6, 1), (6, 7), (7, 6)]
ONSET = np.array([100, 110, 120, 200, 203, -1, 150, 110], np.int32)
PEAK = np.array([5.0, 4.0, 6.0, 3.0, 7.0, 0.0, 4.0, 8.0], np.float32)


def csr(edges, n):
    """Pull-CSR (row k = callers of k, ascending) from (caller, callee) pairs."""
    e = sorted((k, j) for j, k in edges)
    col = np.array([j for _, j in e], np.int32)
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount([k for k, _ in e], minlength=n), out=row_ptr[1:])
    return row_ptr, col


def first(onset, pod):
    return (int(onset) << 32) | int(pod)


NO = R.NO_DEP
# the expected arrays, by hand, per slack
EXPECT = {
    5: dict(dep_earlier=[0, 1, 2, 0, 0, 0, 2, 0], dep_concurrent=[0, 0, 0, 0, 1, 0, 0, 0],
            caller_later=[2, 2, 0, 0, 0, 0, 0, 1], caller_concurrent=[0, 0, 0, 1, 0, 0, 0, 0],
            caller_earlier=[0, 0, 0, 0, 0, 0, 1, 0],
            dep_first=[NO, first(100, 0), first(100, 0), NO, NO, NO, first(110, 1), NO],
            first_movers=[0, 3, 4, 7], top=[0, 7, 3, 4]),
    0: dict(dep_earlier=[0, 1, 2, 0, 1, 0, 2, 0], dep_concurrent=[0, 0, 0, 0, 0, 0, 0, 0],
            caller_later=[2, 2, 0, 1, 0, 0, 0, 1], caller_concurrent=[0, 0, 0, 0, 0, 0, 0, 0],
            caller_earlier=[0, 0, 0, 0, 0, 0, 1, 0],
            dep_first=[NO, first(100, 0), first(100, 0), NO, first(200, 3), NO, first(110, 1), NO],
            first_movers=[0, 3, 7], top=[0, 7, 3]),
}


# ---- seeded dyadic tensors with planted level shifts ----------------------------------------
def dyadic_metrics(P_, M_, T_, W_, seed, n_shift=None):
    """Multiples of 1/16 in [0, 100]: per-series level + noise.  A third of the pods get, on some of
    their metrics, a level shift (persisting to the end or returning after a few steps) followed by a
    run of planted exceedances with gaps of 1 .. G + 1 steps (`plant`), at onsets spread over [W, T)
    -- so episodes start, continue and end across the kernels' W-step block and chunk boundaries."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(25, 55, (1, P_, M_))
    sig = rng.uniform(0.5, 3.0, (1, P_, M_))
    x = R.quantise(base + sig * rng.standard_normal((T_, P_, M_))).astype(np.float64)
    if T_ > W_ + 1:
        pods = rng.choice(P_, n_shift if n_shift is not None else max(1, P_ // 3), replace=False)
        for p in pods:
            on = int(rng.integers(W_, T_))
            dur = int(rng.choice([2, 5, W_ // 2 + 1, T_]))
            ms = rng.choice(M_, int(rng.integers(1, M_ + 1)), replace=False)
            lag = rng.integers(0, 4, len(ms))
            for m, l in zip(ms, lag):
                a, b = min(on + l, T_ - 1), min(on + l + dur, T_)
                x[a:b, p, m] = np.minimum(x[a:b, p, m] + np.round(rng.uniform(4, 12) * sig[0, p, m] * 16) / 16, 100.0)
                steps = a + 1 + np.cumsum(rng.integers(1, G + 2, int(rng.integers(2, 7))))
                plant(x[:, p, m], [int(t) for t in steps if t < T_], W_, strict=False)
    return R.quantise(x)


class BulkClient(DictClient):
    """A client with the bulk metric tensor of krca/agents/metrics.py and nothing else to report."""

    def __init__(self, names, x):
        super().__init__()
        self.names, self.x = names, x

    def get_pod_metric_tensor(self, ns):
        return self.names, self.x
