"""Plain NumPy restatement of the trace analytics (include/krca.h t1, krca/tracecols.py): the
checker of csrc/trace.hip.  Quantiles are also available as TRUE nearest-rank values from np.sort,
independent of the histogram buckets."""
import numpy as np

from krca import tracecols

NB = 896


def bucket(d):
    """Vectorised bucket rule: d < 64 -> d; else 64 + (e-6)*32 + ((d >> (e-5)) - 32), e = floor(log2 d)."""
    d = np.asarray(d, np.uint64)
    e = np.zeros(d.shape, np.int64)
    for k in range(1, 33):  # e = floor(log2 d) without floating point
        e[d >= (np.uint64(1) << np.uint64(k))] = k
    sh = np.maximum(e - 5, 0).astype(np.uint64)
    big = 64 + (e - 6) * 32 + (d >> sh).astype(np.int64) - 32
    return np.where(d < 64, d.astype(np.int64), big)


def bounds(b):
    """(lo, hi) of bucket b as Python ints."""
    b = int(b)
    if b < 64:
        return b, b
    e, m = 6 + (b - 64) // 32, 32 + (b - 64) % 32
    return m << (e - 5), ((m + 1) << (e - 5)) - 1


HI = np.array([bounds(b)[1] for b in range(NB)], np.int64)
LO = np.array([bounds(b)[0] for b in range(NB)], np.int64)


def link(svc, parent, dur_us, err, S):
    """-> (caller_svc int32, self_us uint32, flags uint8, n_bad)."""
    svc, parent = np.asarray(svc, np.int64), np.asarray(parent, np.int64)
    dur, err = np.asarray(dur_us, np.int64), np.asarray(err) != 0
    N = len(svc)
    idx = np.arange(N)
    ok = (svc >= 0) & (svc < S)
    in_range = (parent >= 0) & (parent < N) & (parent != idx)
    p = np.where(in_range, parent, 0)
    valid = ok & in_range & ok[p]
    child_sum = np.zeros(N, np.int64)
    np.add.at(child_sum, p[valid], dur[valid])
    child_err = np.zeros(N, bool)
    child_err[p[valid & err]] = True
    caller = np.where(valid & (svc[p] != svc), svc[p], -1)
    self_us = np.maximum(dur - child_sum, 0)
    flags = err.astype(np.uint8) | ((err & ~child_err).astype(np.uint8) << 1) \
        | ((err & valid & err[p] & (caller >= 0)).astype(np.uint8) << 2)
    caller, self_us, flags = (np.where(ok, a, z) for a, z in ((caller, -1), (self_us, 0), (flags, 0)))
    return caller.astype(np.int32), self_us.astype(np.uint32), flags.astype(np.uint8), int((~ok).sum())


def edges(caller_svc, svc, S):
    """-> (edge_key int64[E] ascending, edge_slot int32[N])."""
    c, s = np.asarray(caller_svc, np.int64), np.asarray(svc, np.int64)
    has = (c >= 0) & (c < S) & (s >= 0) & (s < S)
    key = c * S + s
    uniq = np.unique(key[has])
    slot = np.where(has, np.searchsorted(uniq, np.where(has, key, 0)), -1)
    return uniq.astype(np.int64), slot.astype(np.int32)


def stats(slot, val, flags, S, prev=None):
    """-> (rec int64[S, 8], hist uint32[S, NB]); prev = (rec, hist) to accumulate into."""
    slot, val, flags = np.asarray(slot, np.int64), np.asarray(val, np.int64), np.asarray(flags, np.int64)
    rec = np.zeros((S, 8), np.int64) if prev is None else np.array(prev[0], np.int64)
    hist = np.zeros((S, NB), np.int64) if prev is None else np.array(prev[1], np.int64)
    ok = (slot >= 0) & (slot < S)
    s, v, f = slot[ok], val[ok], flags[ok]
    rec[:, 0] += np.bincount(s, minlength=S)
    np.add.at(rec[:, 1], s, v)
    np.maximum.at(rec[:, 2], s, v)
    for bit in range(3):
        rec[:, 3 + bit] += np.bincount(s[(f >> bit) & 1 == 1], minlength=S)
    np.add.at(hist, (s, bucket(v)), 1)
    return rec, hist.astype(np.uint32)


def quantiles(rec, hist, permille):
    """Nearest rank over the buckets: min(hi(first bucket whose cumulative count reaches k), max)."""
    rec, hist = np.asarray(rec, np.int64), np.asarray(hist, np.int64)
    S = len(rec)
    out = np.zeros((S, len(permille)), np.uint32)
    cum = np.cumsum(hist, axis=1)
    for j, q in enumerate(permille):
        k = (q * rec[:, 0] + 999) // 1000
        b = np.minimum((cum < k[:, None]).sum(axis=1), NB - 1)
        out[:, j] = np.where(rec[:, 0] > 0, np.minimum(HI[b], rec[:, 2]), 0)
    return out


def quantile_bucket(rec, hist, permille):
    """The bucket b* each quantile falls in (for the lo(b*) <= true <= out property); -1 where n = 0."""
    rec, hist = np.asarray(rec, np.int64), np.asarray(hist, np.int64)
    cum = np.cumsum(hist, axis=1)
    out = np.full((len(rec), len(permille)), -1, np.int64)
    for j, q in enumerate(permille):
        k = (q * rec[:, 0] + 999) // 1000
        out[:, j] = np.where(rec[:, 0] > 0, np.minimum((cum < k[:, None]).sum(axis=1), NB - 1), -1)
    return out


def true_quantiles(slot, val, S, permille):
    """True nearest-rank quantiles by sorting (no buckets): the k-th smallest value of the slot,
    k = (q*n + 999) // 1000; 0 where the slot is empty."""
    slot, val = np.asarray(slot, np.int64), np.asarray(val, np.int64)
    ok = (slot >= 0) & (slot < S)
    s, v = slot[ok], val[ok]
    v = np.sort((s << 32) | v) & 0xFFFFFFFF  # by slot, then by value
    n = np.bincount(s, minlength=S)
    start = np.cumsum(n) - n
    out = np.zeros((S, len(permille)), np.int64)
    for j, q in enumerate(permille):
        k = (q * n + 999) // 1000
        pos = np.minimum(start + np.maximum(k, 1) - 1, max(len(v) - 1, 0))
        out[:, j] = np.where(n > 0, v[pos] if len(v) else 0, 0)
    return out


class NumpyTraceEngine:
    """Host engine with NativeEngine's trace_analyze (the agents' checker)."""

    def trace_analyze(self, cols):
        S, n_ops = len(cols.services), len(cols.ops)
        caller, self_us, flags, n_bad = link(cols.svc, cols.parent, cols.dur_us, cols.err, S)
        edge_key, edge_slot = edges(caller, cols.svc, S)
        ok = (cols.svc >= 0) & (cols.svc < S)
        op = np.where(ok, cols.op, -1)
        out = {}
        for name, slot, val, n in (("svc", cols.svc, cols.dur_us, S), ("self", cols.svc, self_us, S),
                                   ("edge", edge_slot, cols.dur_us, len(edge_key)), ("op", op, cols.dur_us, n_ops)):
            rec, hist = stats(slot, val, flags, n)
            out[name] = (rec, quantiles(rec, hist, tracecols.PERMILLE))
        return tracecols.TraceStats(cols.services, cols.ops, len(cols), n_bad, edge_key, out)
