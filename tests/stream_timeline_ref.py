"""NumPy / pure-Python restatement of the streaming anomaly timeline (include/krca.h:
krca_stream_timeline) -- TESTS ONLY, written from the semantics, not from the kernel.

Per series the state is the open episode and the kept one, carried from call to call; `H` is the
horizon after which an episode stops being reported.  With `now` the global step being processed:

  hit(t, z)   an open episode with t - last <= gap is extended; otherwise close(t), then a new
              episode opens at t.
  close(now)  the open episode replaces the kept one when it is sustained (cnt >= min_count) and
              the kept one is absent or expired (now - k_last >= H), or c_peak >= k_peak.
  view(now)   at the end of a call (now = its last step), without touching the state: the kept
              episode is valid when it exists and now - k_last < H, the open one when it is sustained
              and now - c_last < H; the series reports the open one when it is valid and the kept
              one is invalid or c_peak >= k_peak, else the kept one if valid, else none.

The pod's M views are combined by timeline_ref.pod_combine, as the batch timeline combines kept
episodes.  Exactness as in timeline_ref: the fixtures' samples are multiples of 1/16."""
import numpy as np

import timeline_ref as R

KEYS = ("onset", "last", "count", "peak", "lead", "n_metrics")


class SeriesState:
    """Open (c_*) and kept (k_*) episode of S series; cnt == 0: none."""
    FIELDS = ("c_on", "c_last", "c_cnt", "c_peak", "k_on", "k_last", "k_cnt", "k_peak")

    def __init__(self, S):
        self.c_on = np.full(S, -1, np.int64)
        self.c_last = np.full(S, -1, np.int64)
        self.c_cnt = np.zeros(S, np.int64)
        self.c_peak = np.zeros(S, np.float32)
        self.k_on = np.full(S, -1, np.int64)
        self.k_last = np.full(S, -1, np.int64)
        self.k_cnt = np.zeros(S, np.int64)
        self.k_peak = np.zeros(S, np.float32)

    def arrays(self):
        return {f: getattr(self, f).copy() for f in self.FIELDS}


def close(st, s, now, min_count, H):
    if st.c_cnt[s] >= min_count and (st.k_cnt[s] == 0 or now - st.k_last[s] >= H or st.c_peak[s] >= st.k_peak[s]):
        st.k_on[s], st.k_last[s], st.k_cnt[s], st.k_peak[s] = st.c_on[s], st.c_last[s], st.c_cnt[s], st.c_peak[s]


def hit(st, s, t, z, gap, min_count, H):
    z = np.float32(z)
    if st.c_cnt[s] > 0 and t - st.c_last[s] <= gap:
        st.c_last[s] = t
        st.c_cnt[s] += 1
        st.c_peak[s] = max(st.c_peak[s], z)
    else:
        close(st, s, t, min_count, H)
        st.c_on[s] = st.c_last[s] = t
        st.c_cnt[s] = 1
        st.c_peak[s] = z


def view(st, s, now, min_count, H):
    """The episode (onset, last, cnt, peak) series s reports at step `now`, or None."""
    k_ok = st.k_cnt[s] > 0 and now - st.k_last[s] < H
    c_ok = st.c_cnt[s] >= min_count and now - st.c_last[s] < H
    if c_ok and (not k_ok or st.c_peak[s] >= st.k_peak[s]):
        return int(st.c_on[s]), int(st.c_last[s]), int(st.c_cnt[s]), np.float32(st.c_peak[s])
    if k_ok:
        return int(st.k_on[s]), int(st.k_last[s]), int(st.k_cnt[s]), np.float32(st.k_peak[s])
    return None


def outputs(st, now, P, M, gap, min_count, H):
    """The six per-pod arrays at step `now` (the state is not modified)."""
    out = dict(onset=np.full(P, -1, np.int32), last=np.full(P, -1, np.int32), count=np.zeros(P, np.int32),
               peak=np.zeros(P, np.float32), lead=np.full(P, -1, np.int8), n_metrics=np.zeros(P, np.uint8))
    any_ep = ((st.c_cnt > 0) | (st.k_cnt > 0)).reshape(P, M).any(axis=1)
    for p in np.flatnonzero(any_ep).tolist():
        views = [view(st, p * M + m, now, min_count, H) for m in range(M)]
        on, la, c, pk, lead, nm, _ = R.pod_combine(views, gap)
        out["onset"][p], out["last"][p], out["count"][p] = on, la, c
        out["peak"][p], out["lead"][p], out["n_metrics"][p] = pk, lead, nm
    return out


def stream_timeline(x, W, thr, gap, min_count, H, windows, with_state=False):
    """x float32 [T, P, M], consumed in calls of windows[i] steps (sum(windows) <= T) -> the six
    per-pod arrays after every window (a list of dicts; with_state: each dict also holds the series
    state under SeriesState.FIELDS)."""
    x = np.asarray(x, np.float32)
    T, P, M = x.shape
    S = P * M
    assert sum(windows) <= T and all(d >= 1 for d in windows)
    ex, z = R.rolling_exceed(x.reshape(T, S), W, thr)  # causal: row t depends on x[:t + 1] only
    st = SeriesState(S)
    res, t0 = [], 0
    for d in windows:
        for t in range(t0, t0 + d):
            for s in np.flatnonzero(ex[t]).tolist():
                hit(st, s, t, z[t, s], gap, min_count, H)
        t0 += d
        o = outputs(st, t0 - 1, P, M, gap, min_count, H)
        if with_state:
            o.update(st.arrays())
        res.append(o)
    return res


def differing(a, b, keys=KEYS):
    """The names of the outputs that differ between two results (bytes compared)."""
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()
            or np.asarray(a[k]).dtype != np.asarray(b[k]).dtype]


# ---- the cases of the streaming tests (tests/test_stream_timeline_cpu.py, test_gpu_stream_timeline.py)
THR, GAP, MINC = 3.0, 3, 3
LIST_A = [1, 8, 1, 1, 25, 7, 3, 20, 13, 27]  # T = 106
LIST_B = [59, 1, 1, 30, 9, 3, 50, 47]        # T = 200
# (P, M, W, H, seed, windows)
CASES = [(37, 8, 10, 33, 1, LIST_A), (33, 1, 7, 5, 2, LIST_A), (9, 64, 10, 1000, 3, LIST_A),
         (70, 4, 60, 40, 4, LIST_B)]
_cache = {}


def case_data(case):
    """(x [T, P, M], reference results after every window) of a case; computed once and shared."""
    import timeline_cases as C
    key = tuple(case[:5]) + (tuple(case[5]),)
    if key not in _cache:
        P, M, W, H, seed, wins = case
        x = C.dyadic_metrics(P, M, sum(wins), W, seed)
        x.setflags(write=False)
        _cache[key] = (x, stream_timeline(x, W, THR, GAP, MINC, H, wins))
    return _cache[key]
