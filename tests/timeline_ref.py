"""NumPy / pure-Python restatement of the anomaly timeline (include/krca.h: krca_rolling_timeline,
krca_rca_precede, krca_rca_first_mover_key) -- TESTS ONLY, written from the semantics, not from the
kernels.

Exactness.  The kernels' decisions go through explicit fma()s; NumPy has none.  Every bit-exact
fixture therefore uses samples that are multiples of 1/16 in [0, 100] and thresholds whose square
is dyadic (3.0, 2.5).  For W <= 60 the window sums s1 (multiples of 1/16, <= 6000) and s2 (multiples
of 1/256, <= 6e5), A = W x - s1, B = W s2 - s1^2, A^2 and thr^2 B are then all exact in float64, so
fused and unfused arithmetic agree bit for bit; peak = (float32)(|A| / sqrt(B)) uses one correctly
rounded float64 division and square root on both sides.  `quantise` makes such samples."""
import numpy as np

NO_DEP = np.iinfo(np.int64).max


def quantise(x):
    """float array -> float32 multiples of 1/16 in [0, 100]."""
    return (np.round(np.clip(np.asarray(x, np.float64), 0.0, 100.0) * 16.0) / 16.0).astype(np.float32)


def rolling_exceed(x, W, thr):
    """x [T, S] float32 -> (exceed bool [T, S], z float32 [T, S] = (float32)(|A| / sqrt(B)) where
    exceed, 0 elsewhere), t in [W, T) evaluated against the trailing window x[t-W .. t-1]."""
    x = np.asarray(x, np.float32).astype(np.float64)
    T, S = x.shape
    ex = np.zeros((T, S), bool)
    z = np.zeros((T, S), np.float32)
    if T <= W:
        return ex, z
    Wd = float(W)
    thr2 = float(np.float32(thr)) ** 2
    epsB = 1e-12 * Wd * Wd
    s1 = np.zeros(S)
    s2 = np.zeros(S)
    for j in range(W):
        s1 = s1 + x[j]
        s2 = s2 + x[j] * x[j]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(W, T):
            v, o = x[t], x[t - W]
            A = Wd * v - s1
            B = Wd * s2 - s1 * s1
            e = (B > epsB) & ((A * A - thr2 * B) > 0.0)  # NaN compares false: a NaN sample never exceeds
            ex[t] = e
            if e.any():
                z[t, e] = (np.abs(A[e]) / np.sqrt(B[e])).astype(np.float32)
            s1 = (s1 + v) - o
            s2 = (s2 + v * v) - o * o
    return ex, z


def series_episodes(steps, zs, G, R):
    """Exceedance steps (ascending) and their z -> (episodes [(onset, last, cnt, peak)], kept or None).
    kept = the sustained episode (cnt >= R) of the largest peak, the later one on equal peaks."""
    eps = []
    for t, zv in zip(steps, zs):
        t, zv = int(t), np.float32(zv)
        if eps and t - eps[-1][1] <= G:
            on, _, c, pk = eps[-1]
            eps[-1] = (on, t, c + 1, max(pk, zv))
        else:
            eps.append((t, t, 1, zv))
    kept = None
    for e in eps:
        if e[2] >= R and (kept is None or e[3] >= kept[3]):
            kept = e
    return eps, kept


def pod_combine(kept, G):
    """kept[m] (or None) of a pod's M series -> (onset, last, count, peak, lead, n_metrics, members)."""
    have = [(m, e) for m, e in enumerate(kept) if e is not None]
    if not have:
        return -1, -1, 0, np.float32(0), -1, 0, []
    a_m, a = have[0]
    for m, e in have[1:]:
        if e[3] > a[3]:  # ties: lowest m
            a_m, a = m, e
    mem = [(m, e) for m, e in have if e[0] <= a[1] + G and a[0] <= e[1] + G]
    onset = min(e[0] for _, e in mem)
    lead = min(m for m, e in mem if e[0] == onset)
    return (onset, max(e[1] for _, e in mem), sum(e[2] for _, e in mem), np.float32(a[3]), lead, len(mem),
            [m for m, _ in mem])


def timeline(x, W, thr, G=3, R=3, detail=False):
    """x [T, P, M] -> dict of per-pod arrays (onset, last, count int32; peak float32; lead int8;
    n_metrics uint8) and n_exceed int32.  detail: also 'episodes' [P][M] (all episodes of the
    series), 'kept' [P][M] and 'members' [P] -- the intermediate output the tests inspect."""
    x = np.asarray(x, np.float32)
    T, P, M = x.shape
    ex, z = rolling_exceed(x.reshape(T, P * M), W, thr)
    out = dict(onset=np.full(P, -1, np.int32), last=np.full(P, -1, np.int32), count=np.zeros(P, np.int32),
               peak=np.zeros(P, np.float32), lead=np.full(P, -1, np.int8), n_metrics=np.zeros(P, np.uint8),
               n_exceed=ex.reshape(T, P, M).sum(axis=(0, 2)).astype(np.int32))
    if detail:
        out.update(episodes=[[[] for _ in range(M)] for _ in range(P)], kept=[[None] * M for _ in range(P)],
                   members=[[] for _ in range(P)])
    for p in np.flatnonzero(out["n_exceed"] > 0).tolist():
        kept = []
        for m in range(M):
            s = p * M + m
            steps = np.flatnonzero(ex[:, s])
            eps, k = series_episodes(steps, z[steps, s], G, R)
            kept.append(k)
            if detail:
                out["episodes"][p][m] = eps
        on, la, c, pk, lead, nm, mem = pod_combine(kept, G)
        out["onset"][p], out["last"][p], out["count"][p] = on, la, c
        out["peak"][p], out["lead"][p], out["n_metrics"][p] = pk, lead, nm
        if detail:
            out["kept"][p], out["members"][p] = kept, mem
    return out


def precede(onset, row_ptr, col, slack):
    """Edge by edge over the pull-CSR (row k = the callers j of k)."""
    onset = np.asarray(onset, np.int64)
    N = len(onset)
    out = {k: np.zeros(N, np.int32) for k in ("dep_earlier", "dep_concurrent", "caller_later", "caller_concurrent",
                                              "caller_earlier")}
    out["dep_first"] = np.full(N, NO_DEP, np.int64)
    for k in np.flatnonzero(onset >= 0).tolist():
        ok = int(onset[k])
        for j in np.asarray(col[row_ptr[k]:row_ptr[k + 1]], np.int64).tolist():
            if j == k or onset[j] < 0:
                continue
            oj = int(onset[j])
            if ok + slack < oj:
                out["caller_later"][k] += 1
                out["dep_earlier"][j] += 1
                out["dep_first"][j] = min(int(out["dep_first"][j]), (ok << 32) | k)
            elif oj + slack < ok:
                out["caller_earlier"][k] += 1
            else:
                out["caller_concurrent"][k] += 1
                out["dep_concurrent"][j] += 1
    return out


def first_mover_key(onset, peak, prec):
    onset = np.asarray(onset)
    f = np.minimum(prec["caller_later"].astype(np.int64) + prec["caller_concurrent"].astype(np.int64), (1 << 20) - 1)
    key = (f << 32) | np.asarray(peak, np.float32).view(np.uint32).astype(np.int64)
    return np.where((onset >= 0) & (prec["dep_earlier"] == 0), key, 0).astype(np.int64)


def topk(key, k):
    """Descending key, ties to the lower index."""
    order = np.lexsort((np.arange(len(key)), -np.asarray(key, np.int64)))[:k]
    return order.astype(np.int32), np.asarray(key)[order]


def first_movers(tl, row_ptr, col, slack=0, k=10, explain=()):
    """What NativeEngine.first_movers returns, from a timeline() result."""
    prec = precede(tl["onset"], row_ptr, col, slack)
    key = first_mover_key(tl["onset"], tl["peak"], prec)
    idx, val = topk(key, min(k, len(key)))
    idx = idx[val > 0]
    res = dict(idx=idx, onset=tl["onset"][idx], lead=tl["lead"][idx], peak=tl["peak"][idx],
               followers=prec["caller_later"][idx] + prec["caller_concurrent"][idx], explained={})
    for p in explain:
        f = int(prec["dep_first"][p])
        if f != NO_DEP:
            res["explained"][int(p)] = (f & 0xFFFFFFFF, int(tl["onset"][p]) - (f >> 32))
    return res
