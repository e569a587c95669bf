"""NumPy restatement of krca_shift_score (include/krca.h), the reference of the level-shift tests.

Per series of a time-major [T, P, M] float32 tensor: the lower median of the last R samples against
the lower median and MAD of the B samples that end R + G steps before the end.  Order = the unsigned
order of the key k(x) = (bits & 0x80000000) ? ~bits : bits | 0x80000000; the lower median of n
values is the element of 0-based rank (n - 1) // 2, with its own bits; distances are float32
subtractions; the division is float64.
"""
import numpy as np

KEYS = ("shift", "base_med", "base_mad", "recent_med", "score", "lead")
MAX_BASELINE, MAX_RECENT = 256, 64


def to_key(x):
    """float32 array -> uint32 keys whose unsigned order is the total order of the contract."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def from_key(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def lower_median(v):
    """v float32 [n, ...] -> the element of rank (n - 1) // 2 along axis 0, bits kept."""
    k = np.sort(to_key(v), axis=0)
    return from_key(k[(v.shape[0] - 1) // 2])


def shift_score(x, baseline=120, recent=3, guard=0, min_scale=0.0):
    """x float32 [T, P, M] -> dict of KEYS (shift / base_med / base_mad / recent_med float32 [P, M],
    score float32 [P], lead int8 [P]).  Raises ValueError where the C call refuses."""
    x = np.asarray(x, np.float32)
    T, P, M = x.shape
    B, R, G = int(baseline), int(recent), int(guard)
    ms = np.float32(min_scale)
    if not (1 <= M <= 64 and M & (M - 1) == 0):
        raise ValueError("M must be a power of two <= 64")
    if not (2 <= B <= MAX_BASELINE and 1 <= R <= MAX_RECENT and G >= 0 and B + G + R <= T):
        raise ValueError("bad windows")
    if not (np.isfinite(ms) and ms >= 0):
        raise ValueError("bad min_scale")
    base = x[T - R - G - B:T - R - G]
    rec = x[T - R:]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        med = lower_median(base)
        mad = lower_median(np.abs((base - med[None]).astype(np.float32)))
        rmed = lower_median(rec)
        den = 1.4826 * mad.astype(np.float64)
        den = np.where(den > np.float64(ms), den, np.float64(ms))
        pos = den > 0
        q = (rmed.astype(np.float64) - med.astype(np.float64)) / np.where(pos, den, 1.0)
        shift = np.where(pos, q.astype(np.float32), np.float32(0.0)).astype(np.float32)
    a = np.where(np.isnan(shift), np.float32(0.0), np.abs(shift)).astype(np.float32)
    score = a.max(axis=1) if P else np.zeros(0, np.float32)
    lead = np.where(score > 0, a.argmax(axis=1) if P else 0, -1).astype(np.int8)  # argmax: the lowest m
    return dict(shift=shift, base_med=med, base_mad=mad, recent_med=rmed, score=score.astype(np.float32), lead=lead)


def same(ref, got, what=""):
    """Every key: NaN where the reference is NaN, the same bits elsewhere."""
    for k in KEYS:
        w, g = np.asarray(ref[k]), np.asarray(got[k])
        assert w.dtype == g.dtype and w.shape == g.shape, (k, what, w.dtype, g.dtype, w.shape, g.shape)
        if w.dtype == np.float32:
            wn, gn = np.isnan(w), np.isnan(g)
            assert np.array_equal(wn, gn), (k, what, "NaN positions", np.argwhere(wn != gn)[:5].tolist())
            w, g = np.where(wn, np.float32(0), w), np.where(gn, np.float32(0), g)
        bad = w.view(np.uint8 if w.dtype == np.int8 else np.uint32) != g.view(np.uint8 if g.dtype == np.int8 else np.uint32)
        assert not bad.any(), (k, what, np.argwhere(bad)[:5].tolist(), w[bad][:5], g[bad][:5])


# ---- data of the listed kinds (shared by the CPU and the device tests) ---------------------------
def data(kind, T, P, M, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":  # synth.make_metrics-like: level + daily sinusoid + noise, clamped to [0, 100]
        b, a = rng.random((P, M)) * 30 + 25, rng.random((P, M)) * 12
        sig, phi = rng.random((P, M)) * 2.5 + 0.5, rng.random((P, 1)) * 2 * np.pi
        t = np.arange(T).reshape(-1, 1, 1)
        x = b + a * np.sin(2 * np.pi * t / 1440.0 + phi) + sig * rng.standard_normal((T, P, M))
        return np.clip(x, 0, 100).astype(np.float32)
    if kind == "ties":  # {0, 1, 2} drawn 80 / 10 / 10 %: heavy ties, MAD 0
        return rng.choice(np.array([0, 1, 2], np.float32), size=(T, P, M), p=[0.8, 0.1, 0.1])
    if kind == "signs":  # mixed signs with +-0 and denormals
        x = rng.standard_normal((T, P, M)).astype(np.float32)
        u = rng.random((T, P, M))
        x[u < 0.15] = 0.0
        x[(u >= 0.15) & (u < 0.3)] = -0.0
        den = (rng.integers(1, 1 << 22, (T, P, M)).astype(np.uint32) | (rng.integers(0, 2, (T, P, M)).astype(np.uint32) << 31))
        sel = (u >= 0.3) & (u < 0.5)
        x[sel] = den.view(np.float32)[sel]
        return x
    if kind == "nonfinite":  # noise with NaN (both signs) and +-Inf sprinkled in
        x = data("noise", T, P, M, seed)
        u = rng.random((T, P, M))
        x[u < 0.02] = np.nan
        x[(u >= 0.02) & (u < 0.03)] = np.inf
        x[(u >= 0.03) & (u < 0.04)] = -np.inf
        neg_nan = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
        x[(u >= 0.04) & (u < 0.05)] = neg_nan
        return x
    raise ValueError(kind)
