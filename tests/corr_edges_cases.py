"""Fixtures for krca_corr_edges (tests/test_corr_edges_cpu.py, tests/test_gpu_corr_edges.py).

Dyadic fixtures: rows of integers in [-8, 8], so |S_l| <= 64 T < 2^24 for T <= 1440 and float32
accumulation in any order is exact; the device must then equal tests/corr_edges_ref.py bit for bit."""
import numpy as np

CHUNK = 512  # callers per wave work item of csrc/corr_edges.hip (rows past it are split)


def csr(edges, N):
    """[(caller, callee)] -> pull-CSR (row callee = its callers in list order)."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    order = np.argsort(e[:, 1], kind="stable")
    rp = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(e[:, 1], minlength=N), out=rp[1:])
    return rp, e[order, 0].astype(np.int32)


# ---- hand fixture --------------------------------------------------------------------------------
HAND_T, HAND_L = 64, 8
# 32 digits of pi minus 4: no period, both signs; placed at steps 16 .. 47, at least L = 8 steps from both ends
_PI = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8, 4, 6, 2, 6, 4, 3, 3, 8, 3, 2, 7, 9, 5]
HAND_EDGES = [(1, 0), (2, 0), (3, 0), (0, 0), (1, 2)]  # caller -> dependency
HAND_LAGS = {(1, 0): 3, (2, 0): -2, (3, 0): 0, (0, 0): 0, (1, 2): 5}


def hand_fixture():
    """z [4, 64]: z1[t] = z0[t - 3], z2[t] = -z0[t + 2], z3 = 0."""
    z = np.zeros((4, HAND_T), np.float32)
    z[0, 16:48] = np.asarray(_PI, np.float32) - 4.0
    z[1, 3:] = z[0, :-3]
    z[2, :-2] = -z[0, 2:]
    return z


def tie_fixture():
    """Pod 0 (dependency): one impulse at t = 8; pod 1 (caller): equal impulses at t = 6 and 10.
    S_l = z1[8 + l] z0[8]: equal at l = -2 and l = +2, zero elsewhere -> lag +2."""
    z = np.zeros((2, 32), np.float32)
    z[0, 8] = 4.0
    z[1, 6] = z[1, 10] = 3.0
    return z, csr([(1, 0)], 2)


# ---- dyadic random graphs ------------------------------------------------------------------------
FORCED_DEGREES = (0, 1, 63, 64, 65)


def dyadic_case(T, N=300, seed=0, long_row=0):
    """-> z float32 [N, T] (integers in [-8, 8]), row_ptr, col, ties [(caller, callee, lag or None)].
    Degrees random in 0 .. 70 with rows of degree 0, 1, 63, 64 and 65 forced; callers drawn with
    replacement (duplicate edges), self loops planted in every eighth row; long_row > 0 gives the
    last row that many callers.  Planted exact ties (T >= 5): a dependency with one impulse and a caller with
    two equal impulses m steps before and after it (lag +m for m <= L, all-zero sums otherwise), and
    an all-zero pod (every sum ties at 0: lag 0)."""
    rng = np.random.default_rng(1000 * T + seed)
    z = rng.integers(-8, 9, (N, T)).astype(np.float32)
    deg = rng.integers(0, 71, N)
    deg[:len(FORCED_DEGREES)] = FORCED_DEGREES
    rng.shuffle(deg)
    if long_row:
        deg[N - 1] = long_row
    edges, ties = [], []
    for k in range(N):
        callers = rng.integers(0, N, deg[k])
        if k % 8 == 0 and deg[k]:
            callers[rng.integers(0, deg[k])] = k  # a self loop
        edges += [(int(j), k) for j in callers]
    if T >= 5:
        t0 = T // 2
        for i, m in enumerate((1, 2, 3, 4)):
            dep, caller = 10 + 2 * i, 11 + 2 * i
            if t0 - m < 0 or t0 + m >= T:
                continue
            z[dep] = 0
            z[dep, t0] = 4
            z[caller] = 0
            z[caller, t0 - m] = z[caller, t0 + m] = 3
            edges.append((caller, dep))
            ties.append((caller, dep, m))
        z[20] = 0
        edges += [(20, 21), (21, 20)]
        ties += [(20, 21, 0), (21, 20, 0)]
    rp, col = csr(edges, N)
    return z, rp, col, ties


DYADIC_SHAPES = [(1, 0), (1, 16), (5, 8), (5, 16), (63, 1), (64, 8), (64, 16), (65, 0), (65, 8), (257, 16), (257, 1),
                 (1440, 8)]  # (T, L): every T and every L of the issue, L > T included


# ---- float data ----------------------------------------------------------------------------------
def standardise(x):
    """Rows to zero mean and unit population std (float64), as float32; a flat row becomes zeros."""
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=1, keepdims=True)
    sd = x.std(axis=1, keepdims=True)
    return np.where(sd > 0, (x - mu) / np.where(sd > 0, sd, 1.0), 0.0).astype(np.float32)


def float_case(N=400, T=1440, L=8, seed=0, phi=0.6):
    """AR(1) rows.  Pods 0 .. 99 are dependencies; caller 100 + i follows dependency i % 100:
    caller[t] = 0.8 dep[t - lag_i] + 0.6 noise, lag_i in [-L, L] planted (300 planted edges), plus 300
    unrelated edges (caller 100 + i -> dependency (i + 37) % 100).
    -> z float32 [N, T] standardised, row_ptr, col, planted {(caller, dep): lag}."""
    rng = np.random.default_rng(seed)
    pad = 2 * L
    n_dep = 100

    def ar1(n, length):
        e = rng.standard_normal((n, length + 50))
        out = np.zeros_like(e)
        for t in range(1, e.shape[1]):
            out[:, t] = phi * out[:, t - 1] + e[:, t]
        return out[:, 50:] / np.sqrt(1.0 / (1.0 - phi * phi))

    dep = ar1(n_dep, T + 2 * pad)
    noise = ar1(N - n_dep, T)
    lags = rng.integers(-L, L + 1, N - n_dep)
    x = np.zeros((N, T))
    x[:n_dep] = dep[:, pad:pad + T]
    planted, edges = {}, []
    for i in range(N - n_dep):
        d, lag = i % n_dep, int(lags[i])
        x[n_dep + i] = 0.8 * dep[d, pad - lag:pad - lag + T] + 0.6 * noise[i]
        planted[(n_dep + i, d)] = lag
        edges.append((n_dep + i, d))
        edges.append((n_dep + i, (i + 37) % n_dep))
    rp, col = csr(edges, N)
    return standardise(x), rp, col, planted


def tol(T):
    """|r - ref| bound of the issue: float32 accumulation in any order errs by at most T u sum|ab| / T
    with sum|ab| / T <= 1 for standardised rows (Cauchy-Schwarz), plus two final roundings."""
    return (T + 2) * 2.0 ** -24


# ---- launch forms of krca_corr_edges ---------------------------------------------------------------
# (T, L) at N = 40.  A wave's LDS row holds stride = T + 2 LT floats rounded up to 4 (LT = L rounded
# up to 0 / 4 / 8 / 16); a workgroup runs four waves while 4 rows fit 64 KiB, else one; a call whose
# single row does not fit is refused; 16-byte loads need T % 4 == 0 and a 16-byte-aligned z.
LAUNCH_N = 40
LAUNCH_SHAPES = [(4080, 8), (4081, 8), (4084, 8), (16368, 8), (16384, 0), (4068, 16)]
REFUSED_SHAPES = [(16369, 8), (16385, 0), (16353, 16)]
MISALIGNED_T = (64, 4084)
LAUNCH_TAU = 0.125  # below the scale of c = S / T on these rows (variance 24: |c| ~ 24 / sqrt(T) >= 0.18)
LDS_BYTES = 65536


def launch_form(T, L, aligned=True):
    """-> (waves per workgroup, bytes per load) krca_corr_edges takes for these sizes by the rule of
    include/krca.h, or None when the call is refused."""
    lt = 0 if L == 0 else 4 if L <= 4 else 8 if L <= 8 else 16
    stride = (T + 2 * lt + 3) & ~3
    if 4 * stride > LDS_BYTES:
        return None
    return (4 if 16 * stride <= LDS_BYTES else 1), (16 if T % 4 == 0 and aligned else 4)


def launch_case(T):
    """dyadic_case(T, N = 40) without the tie list, computed once per T."""
    if T not in _launch_cache:
        z, rp, col, _ = dyadic_case(T, N=LAUNCH_N)
        _launch_cache[T] = (z, rp, col)
    return _launch_cache[T]


_launch_cache = {}


# ---- follower clamp of krca_corr_lead_key ----------------------------------------------------------
CLAMP = (1 << 20) - 1
FOLLOWERS = (0, 1, CLAMP - 1, CLAMP, CLAMP + 1, CLAMP + 6, 2 ** 31 - 1)
DENORMAL = float(np.float32(2.0 ** -149))
KEY_SCORES = (0.0, DENORMAL, 1.5, float("inf"), float("nan"), -1.0)


def lead_key_case():
    """Fabricated inputs of krca_corr_lead_key: FOLLOWERS x dep_lead in {0, 1} x KEY_SCORES
    -> (dep_lead int32, caller_follow int32, score float32)."""
    rows = [(d, f, s) for f in FOLLOWERS for d in (0, 1) for s in KEY_SCORES]
    d, f, s = (np.array(c) for c in zip(*rows))
    return d.astype(np.int32), f.astype(np.int32), s.astype(np.float32)
