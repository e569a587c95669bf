"""NumPy float64 restatement of krca_corr_edges / krca_corr_lead_key (include/krca.h) -- TESTS ONLY.

z float32 [N][T] pod-major; the pull-CSR (row k = the callers j of k, edges j -> k).  For the edge at
CSR position e, in row k with j = col[e], and l in [-L, L]:
    S_l = sum_{t = max(0,-l)}^{min(T, T-l) - 1} z[j][t+l] * z[k][t],    c_l = S_l / T
evaluated in float64 over the float32 inputs (as one matrix product per row: the order of a float64
sum is far below every tolerance used, and exact on the dyadic fixtures)."""
import numpy as np

from krca.leadlag import ID_BASE, decode_dep_best, edge_of

POD_KEYS = ("dep_lead", "dep_sync", "dep_best", "caller_follow", "caller_sync", "caller_lead")
EDGE_KEYS = ("r0", "lag", "r_lag")


def lag_order(L):
    """0, +1, -1, +2, -2, ..."""
    out = [0]
    for m in range(1, L + 1):
        out += [m, -m]
    return out


def lag_sums(z, row_ptr, col, L):
    """-> S float64 [E, 2L+1], column l + L."""
    z = np.asarray(z, np.float32).astype(np.float64)
    N, T = z.shape
    E = int(row_ptr[N])
    S = np.zeros((E, 2 * L + 1))
    for k in range(N):
        e0, e1 = int(row_ptr[k]), int(row_ptr[k + 1])
        if e0 == e1:
            continue
        pad = np.zeros(T + 2 * L)
        pad[L:L + T] = z[k]
        # with u = t + l:  S_l = sum_u z[j][u] * z[k][u - l],  z[k] = 0 outside [0, T)
        K = np.stack([pad[L - l:L - l + T] for l in range(-L, L + 1)])
        S[e0:e1] = z[np.asarray(col[e0:e1], np.int64)] @ K.T
    return S


def active_edges(row_ptr, col, N, mask=None):
    callee = np.repeat(np.arange(N, dtype=np.int64), np.diff(np.asarray(row_ptr, np.int64)))
    caller = np.asarray(col[:len(callee)], np.int64)
    on = caller != callee
    if mask is not None:
        m = np.asarray(mask) != 0
        on &= m[caller] & m[callee]
    return caller, callee, on


def classify(r_lag, lag, row_ptr, col, N, tau, slack):
    """Counts, dep_best from the per-edge r_lag (float32) and lag: what the device derives from the
    values it stores (an inactive edge stores 0 and |0| > tau never holds)."""
    caller, callee, _ = active_edges(row_ptr, col, N)
    r_lag = np.asarray(r_lag, np.float32)
    lag = np.asarray(lag, np.int64)
    corr = np.abs(r_lag) > np.float32(tau)
    dep = corr & (lag > slack)
    cal = corr & (lag < -slack)
    syn = corr & ~dep & ~cal
    cnt = lambda idx, sel: np.bincount(idx[sel], minlength=N).astype(np.int32)  # noqa: E731
    out = dict(dep_lead=cnt(caller, dep), dep_sync=cnt(caller, syn), caller_follow=cnt(callee, dep),
               caller_sync=cnt(callee, syn), caller_lead=cnt(callee, cal))
    best = np.zeros(N, np.int64)
    word = (np.abs(r_lag).view(np.uint32).astype(np.int64) << 32) | (ID_BASE - callee)
    np.maximum.at(best, caller[dep], word[dep])
    out["dep_best"] = best
    return out


def edges(z, row_ptr, col, L=8, tau=0.5, slack=0, mask=None, detail=False):
    """Everything krca_corr_edges writes.  detail: also 'c' float64 [E, 2L+1] (column l + L)."""
    z = np.asarray(z, np.float32)
    N, T = z.shape
    S = lag_sums(z, row_ptr, col, L)
    E = len(S)
    _, _, on = active_edges(row_ptr, col, N, mask)
    best = np.abs(S[:, L]).copy()
    lag = np.zeros(E, np.int64)
    for l in lag_order(L)[1:]:
        a = np.abs(S[:, L + l])
        better = a > best  # strictly: ties keep the earlier visit
        lag[better] = l
        best[better] = a[better]
    c = S / float(T)
    r0 = np.where(on, c[:, L], 0.0).astype(np.float32)
    r_lag = np.where(on, c[np.arange(E), L + lag], 0.0).astype(np.float32)
    lag = np.where(on, lag, 0)
    out = dict(r0=r0, lag=lag.astype(np.int8), r_lag=r_lag)
    out.update(classify(r_lag, lag, row_ptr, col, N, tau, slack))
    if detail:
        out["c"] = c
    return out


def lead_key(dep_lead, caller_follow, score):
    score = np.asarray(score, np.float32)
    f = np.minimum(np.asarray(caller_follow, np.int64), (1 << 20) - 1)
    key = (f << 32) | score.view(np.uint32).astype(np.int64)
    with np.errstate(invalid="ignore"):
        sel = (np.asarray(dep_lead) == 0) & (np.asarray(caller_follow) > 0) & (score > 0)
    return np.where(sel, key, 0).astype(np.int64)


def topk(key, k):
    """Descending key, ties to the lower index."""
    order = np.lexsort((np.arange(len(key)), -np.asarray(key, np.int64)))[:k]
    return order.astype(np.int32), np.asarray(key)[order]


def lead_roots(out, score, row_ptr, col, k=10, explain=()):
    """What NativeEngine.lead_roots returns, from an edges() result."""
    score = np.asarray(score, np.float32)
    key = lead_key(out["dep_lead"], out["caller_follow"], score)
    idx, val = topk(key, min(k, len(key)))
    idx = idx[val > 0]
    res = dict(idx=idx, followers=out["caller_follow"][idx], score=score[idx], explained={})
    for p in explain:
        dep = decode_dep_best(out["dep_best"][p])
        if dep is not None:
            e = edge_of(row_ptr, col, out["lag"], out["r_lag"], int(p), dep[0], dep[2])
            res["explained"][int(p)] = (dep[0], int(out["lag"][e]), float(out["r_lag"][e]))
    return res
