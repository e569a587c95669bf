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


# ---- scorer threshold cases -------------------------------------------------------------------
# Thresholds that float32 does not hold exactly (2.7, 3.3, 1.1, 1e-3), ones it does (0.5, 0.0, 1000.0),
# one that nearly everything exceeds (1e-3), the strict `>` at 0.0 and one nothing reaches (1000.0).
THRS = (2.7, 3.3, 1.1, 0.5, 1e-3, 0.0, 1000.0)
THR_SHAPE = (300, 8, 200, 60)  # P, M, T, W
THR_WINDOWS = (60, 7)          # W = 60: the kernels of pipe_window(); W = 7: the re-reading kernel
THR_STREAM_WINDOWS = [1, 7, 45, 60, 87]
THR_STREAM_HORIZONS = (50, 32, 64)  # 32 and 64: whole exceedance-bit words
THR_STREAM_THRS = (2.7, 0.5)
THR_MAX_DISAGREE = 0.005  # share of pods on which the C twin and the float64 reference may differ
# sum over pods of the float64 reference's n_exceed at W = 60, recorded from the two host references
THR_TOTALS_W60 = {2.7: 4692, 3.3: 988, 0.5: 218754, 1e-3: 335748, 0.0: 336000, 1000.0: 0}
_thr_cache = {}


def threshold_series(dyadic=False):
    """x float32 [T, P, M] of the threshold cases, read-only and shared; dyadic: the same series
    rounded to multiples of 1/16 in [0, 100] (timeline_ref.quantise), on which the NumPy timeline
    references are exact for any threshold: A^2 is exact, and both sides round thr^2 B once."""
    from krca import synth
    if "x" not in _thr_cache:
        P, M, T_, W_ = THR_SHAPE
        m = synth.make_graph(P, 8, seed=3)
        x = synth.make_metrics(P, M, T_, window=W_, seed=4, roots=m.roots).numpy().copy()
        xq = R.quantise(x)
        x.setflags(write=False)
        xq.setflags(write=False)
        _thr_cache["x"], _thr_cache["xq"] = x, xq
    return _thr_cache["xq" if dyadic else "x"]


def threshold_refs(W_, thr):
    """-> (the C twin's dict, the float64 reference's n_exceed int64 [P], agree bool [P]) on
    threshold_series() at window W_; the float64 reference gets the threshold float32 holds."""
    import oracle
    key = ("ref", W_, thr)
    if key not in _thr_cache:
        x = threshold_series()
        twin = oracle.c_rolling_score(x, W_, thr)
        n64 = oracle.rolling_score_f64(x, W_, float(np.float32(thr)))[2]
        _thr_cache[key] = (twin, n64, twin["n_exceed"] == n64)
    return _thr_cache[key]


THR_STREAM_PODS = THR_SHAPE[0]  # pods of the series the streaming-timeline reference walks: all of them


def threshold_stream_ref(thr, H):
    """tests/stream_timeline_ref.py over the first THR_STREAM_PODS pods of the dyadic threshold series
    in THR_STREAM_WINDOWS at W = 60, gap 3, min_count 3: the six outputs after every window."""
    import stream_timeline_ref as SR
    key = ("stream", thr, H)
    if key not in _thr_cache:
        x = threshold_series(dyadic=True)[:, :THR_STREAM_PODS]
        _thr_cache[key] = SR.stream_timeline(x, THR_SHAPE[3], thr, 3, 3, H, THR_STREAM_WINDOWS)
    return _thr_cache[key]


# ---- follower clamp of krca_rca_first_mover_key --------------------------------------------------
CLAMP = (1 << 20) - 1
FOLLOWERS = (0, 1, CLAMP - 1, CLAMP, CLAMP + 1, CLAMP + 6, 2 ** 31 - 1)
# (caller_later, caller_concurrent): each count alone in either place, then sums that cross the clamp
# while both addends stay below it, and a sum that leaves int32
FOLLOWER_PAIRS = tuple((f, 0) for f in FOLLOWERS) + tuple((0, f) for f in FOLLOWERS[1:]) + (
    (1 << 19, (1 << 19) - 2), (1 << 19, (1 << 19) - 1), (1 << 19, 1 << 19), (CLAMP - 1, 1), (CLAMP, CLAMP), (1, CLAMP - 1),
    (2 ** 31 - 1, 2 ** 31 - 1))
DENORMAL = float(np.float32(2.0 ** -149))
KEY_PEAKS = (0.0, DENORMAL, 1.5, float("inf"))  # include/krca.h: peak >= 0


def first_mover_key_case():
    """Fabricated inputs of krca_rca_first_mover_key, the cross product of FOLLOWER_PAIRS, dep_earlier
    in {0, 1}, onset in {-1, 0, 5} and KEY_PEAKS -> (onset int32, peak float32, prec dict of int32)."""
    rows = [(on, pk, de, cl, cc) for cl, cc in FOLLOWER_PAIRS for de in (0, 1) for on in (-1, 0, 5) for pk in KEY_PEAKS]
    on, pk, de, cl, cc = (np.array(c) for c in zip(*rows))
    prec = dict(dep_earlier=de.astype(np.int32), caller_later=cl.astype(np.int32), caller_concurrent=cc.astype(np.int32))
    return on.astype(np.int32), pk.astype(np.float32), prec
