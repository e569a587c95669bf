"""NumPy restatement of krca_peer_score (include/krca.h), the reference of the peer-deviation tests, with
the data kinds and group layouts both suites share.

Per group (CSR grp_ptr / member; ids outside [0, P) ignored) and metric: the lower median and MAD of
v [P, M] over the valid members in krca_shift_score's key order (tests/shift_ref.py), each member's
float64 deviation over 1.4826 * MAD (at least min_scale) rounded once to float32; per pod the largest
|deviation| and its lowest metric.
"""
import numpy as np

import shift_ref as S

KEYS = ("peer", "score", "lead", "grp_med", "grp_mad", "grp_out")
SMALL_MAX, LDS_CAP = 64, 4096


def peer_score(v, grp_ptr, member, min_members=4, min_scale=0.0, out_thr=3.0):
    """v float32 [P, M] -> dict of KEYS (peer float32 [P, M], score float32 [P], lead int8 [P], grp_med /
    grp_mad float32 [G, M], grp_out int32 [G, M]).  Raises ValueError where the C call refuses.  Pods
    listed twice are the caller's business (the contract leaves their values open)."""
    v = np.asarray(v, np.float32)
    P, M = v.shape
    gp = np.asarray(grp_ptr, np.int64)
    mem = np.asarray(member, np.int64)
    G = len(gp) - 1
    ms, thr = np.float32(min_scale), np.float32(out_thr)
    if not (1 <= M <= 64 and M & (M - 1) == 0):
        raise ValueError("M must be a power of two <= 64")
    if int(min_members) < 1:
        raise ValueError("min_members must be >= 1")
    if not (np.isfinite(ms) and ms >= 0 and np.isfinite(thr) and thr >= 0):
        raise ValueError("bad min_scale / out_thr")
    if G < 0 or P * M >= 1 << 32:
        raise ValueError("bad sizes")
    peer = np.zeros((P, M), np.float32)
    med = np.zeros((G, M), np.float32)
    mad = np.zeros((G, M), np.float32)
    out = np.zeros((G, M), np.int32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for g in range(G if P else 0):
            ids = mem[gp[g]:gp[g + 1]]
            ids = ids[(ids >= 0) & (ids < P)]
            if not len(ids):
                continue
            x = v[ids]
            med[g] = S.lower_median(x)
            mad[g] = S.lower_median(np.abs((x - med[g][None]).astype(np.float32)))
            if len(ids) < int(min_members):
                continue
            den = 1.4826 * mad[g].astype(np.float64)
            den = np.where(den > np.float64(ms), den, np.float64(ms))
            pos = den > 0
            q = (x.astype(np.float64) - med[g].astype(np.float64)[None]) / np.where(pos, den, 1.0)[None]
            pr = np.where(pos[None], q.astype(np.float32), np.float32(0.0)).astype(np.float32)
            peer[ids] = pr
            out[g] = (np.abs(pr) > thr).sum(axis=0)
    a = np.where(np.isnan(peer), np.float32(0.0), np.abs(peer)).astype(np.float32)
    score = a.max(axis=1) if P else np.zeros(0, np.float32)
    lead = np.where(score > 0, a.argmax(axis=1) if P else 0, -1).astype(np.int8)  # argmax: the lowest m
    return dict(peer=peer, score=score.astype(np.float32), lead=lead, grp_med=med, grp_mad=mad, grp_out=out)


def same(ref, got, what=""):
    """Every key: NaN where the reference is NaN, the same bits elsewhere."""
    for k in KEYS:
        w, g = np.asarray(ref[k]), np.asarray(got[k])
        assert w.dtype == g.dtype and w.shape == g.shape, (k, what, w.dtype, g.dtype, w.shape, g.shape)
        if w.dtype == np.float32:
            wn, gn = np.isnan(w), np.isnan(g)
            assert np.array_equal(wn, gn), (k, what, "NaN positions", np.argwhere(wn != gn)[:5].tolist())
            w, g = np.where(wn, np.float32(0), w), np.where(gn, np.float32(0), g)
        view = {np.dtype(np.int8): np.uint8, np.dtype(np.int32): np.uint32, np.dtype(np.float32): np.uint32}[w.dtype]
        bad = w.view(view) != g.view(view)
        assert not bad.any(), (k, what, np.argwhere(bad)[:5].tolist(), w[bad][:5], g[bad][:5])


# ---- data and layouts (shared by the CPU and the device tests) -----------------------------------------
def data(kind, P, M, seed=0):
    """One time step of shift_ref.data's kind: float32 [P, M]."""
    return np.ascontiguousarray(S.data(kind, 3, P, M, seed)[1])


def layout(sizes, P, seed=0, sentinels=0):
    """Groups of the given sizes over distinct pods drawn without order from [0, P) (members shuffled
    over non-contiguous pods; the pods left over are in no group).  sentinels > 0 inserts that many
    out-of-range ids (-1 and P alternating) at seeded positions of every group that has members.
    -> (grp_ptr int64, member int32)."""
    rng = np.random.default_rng(seed)
    total = int(sum(sizes))
    assert total <= P, (total, P)
    pods = rng.permutation(P)[:total]
    rows, k = [], 0
    for n in sizes:
        ids = pods[k:k + n].astype(np.int64)
        k += n
        if sentinels and n:
            at = np.sort(rng.integers(0, n + 1, sentinels))
            ids = np.insert(ids, at, [(-1, P)[i % 2] for i in range(sentinels)])
        rows.append(ids)
    gp = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=gp[1:])
    mem = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    return gp, mem
