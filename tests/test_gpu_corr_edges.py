"""krca_corr_edges and krca_corr_lead_key on the device against tests/corr_edges_ref.py: bit-exact on
dyadic fixtures, within the float32 accumulation bound on float data, under masks / tau / slack,
inside guard bands, and end to end through the Coordinator's `correlations` key."""
import numpy as np
import pytest
import torch

import agent_cases as A
import corr_edges_cases as C
import corr_edges_ref as R
from guarded import GuardedEngine, run_poisons
from krca import native, synth

pytestmark = pytest.mark.gpu

ALL = R.EDGE_KEYS + R.POD_KEYS


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


def run(eng, z, rp, col, L, tau=0.5, slack=0, mask=None, score=None):
    """Device outputs as host arrays, plus 'key' for `score`."""
    zd = torch.from_numpy(z).cuda()
    rpd, cld = eng._csr_dev(rp, col)
    md = None if mask is None else torch.from_numpy(mask).cuda()
    out = eng.corr_edges_device(zd, rpd, cld, L, tau, slack, md)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    if score is not None:
        got["key"] = eng.corr_lead_key_device(out, torch.from_numpy(score).cuda()).cpu().numpy()
    return got


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_exact(eng, z, rp, col, L, tau=0.5, slack=0, mask=None, seed=0):
    score = np.random.default_rng(seed).integers(-16, 160, len(z)).astype(np.float32) / 16
    got = run(eng, z, rp, col, L, tau, slack, mask, score)
    ref = R.edges(z, rp, col, L, tau, slack, mask)
    ref["key"] = R.lead_key(ref["dep_lead"], ref["caller_follow"], score)
    for name in ALL + ("key",):
        g, w = got[name], ref[name]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if not same(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError((name, z.shape, L, tau, slack, bad[:5], g[bad[:5]], w[bad[:5]]))
    return ref


# ---- bit-exact on dyadic fixtures ------------------------------------------------------------------
@pytest.mark.parametrize("T,L", C.DYADIC_SHAPES)
def test_dyadic_matches_reference(eng, T, L):
    z, rp, col, ties = C.dyadic_case(T)
    ref = check_exact(eng, z, rp, col, L, tau=0.25, slack=1 if L >= 2 else 0)
    for j, k, m in ties:
        e = rp[k] + np.flatnonzero(col[rp[k]:rp[k + 1]] == j)[-1]
        assert ref["lag"][e] == (m if m <= L else 0)
    if T > 1 and L > 0:
        assert (ref["dep_lead"] > 0).any() and (ref["caller_lead"] > 0).any() and (ref["dep_best"] > 0).any()


@pytest.mark.parametrize("L", [0, 8, 16])
def test_dyadic_long_row(eng, L):
    """One row of 2 * chunk + 1 callers: three work items, per-callee counts summed across them."""
    z, rp, col, _ = C.dyadic_case(64, long_row=2 * C.CHUNK + 1)
    ref = check_exact(eng, z, rp, col, L, tau=0.25)
    n = len(z) - 1
    assert ref["caller_follow"][n] + ref["caller_sync"][n] + ref["caller_lead"][n] > C.CHUNK


# ---- launch forms: one wave per workgroup, the largest T, a misaligned z ----------------------------
@pytest.mark.parametrize("T,L", C.LAUNCH_SHAPES)
def test_launch_forms_match_reference(eng, T, L):
    """T + 2 LT around 4096 (four waves per workgroup -> one) and at the 16384-float limit of a
    wave's LDS row, with 4-byte and 16-byte loads: bit-equal on integer rows (|S| <= 64 T < 2^24)."""
    assert C.launch_form(T, L) is not None
    z, rp, col = C.launch_case(T)
    ref = check_exact(eng, z, rp, col, L, tau=C.LAUNCH_TAU, slack=1 if L >= 2 else 0)
    if L > 0:  # (tests/test_argument_cases_cpu.py holds the counts the reference finds)
        assert ref["dep_lead"].sum() > 100 and ref["caller_lead"].sum() > 100


@pytest.mark.parametrize("T,L", C.REFUSED_SHAPES)
def test_launch_refused_past_the_largest_T(eng, T, L):
    assert C.launch_form(T, L) is None and C.launch_form(T - 1, L) is not None
    zd = torch.zeros((C.LAUNCH_N, T), dtype=torch.float32, device="cuda")
    rpd, cld = eng._csr_dev(*C.launch_case(64)[1:])
    with pytest.raises(native.KrcaError, match=f"T={T}"):
        eng.corr_edges_device(zd, rpd, cld, L, C.LAUNCH_TAU, 0)


@pytest.mark.parametrize("T", C.MISALIGNED_T)
def test_misaligned_z_takes_the_4_byte_loads(eng, T):
    """T % 4 == 0 with z 4-byte but not 16-byte aligned: byte-equal to the aligned call and the reference."""
    z, rp, col = C.launch_case(T)
    score = np.random.default_rng(T).integers(-16, 160, len(z)).astype(np.float32) / 16
    ref = R.edges(z, rp, col, 8, C.LAUNCH_TAU, 1)
    ref["key"] = R.lead_key(ref["dep_lead"], ref["caller_follow"], score)
    rpd, cld = eng._csr_dev(rp, col)
    sd = torch.from_numpy(score).cuda()
    buf = torch.empty(z.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    outs = []
    for shift in (0, 1, 2, 3):
        zd = buf[shift:shift + z.size].view(z.shape)
        zd.copy_(torch.from_numpy(z))
        assert zd.data_ptr() % 16 == 4 * shift and zd.is_contiguous()
        out = eng.corr_edges_device(zd, rpd, cld, 8, C.LAUNCH_TAU, 1)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["key"] = eng.corr_lead_key_device(out, sd).cpu().numpy()
        outs.append(got)
    for shift, got in enumerate(outs):
        for name in ALL + ("key",):
            assert same(got[name], ref[name]), (name, shift)
            assert same(got[name], outs[0][name]), (name, shift)


# ---- the follower clamp of the key -----------------------------------------------------------------
def test_lead_key_follower_clamp(eng):
    """Fabricated counts around 2^20 - 1 (the key's follower field holds 20 bits) crossed with dep_lead,
    and scores 0, denormal, 1.5, inf, NaN and -1: bit-equal to the reference's formula."""
    d, f, s = C.lead_key_case()
    out = dict(dep_lead=torch.from_numpy(d).cuda(), caller_follow=torch.from_numpy(f).cuda())
    key = eng.corr_lead_key_device(out, torch.from_numpy(s).cuda()).cpu().numpy()
    ref = R.lead_key(d, f, s)
    assert same(key, ref), np.flatnonzero(key != ref)[:5]
    at = lambda fv: key[(d == 0) & (f == fv) & (s == np.float32(1.5))][0]  # noqa: E731
    assert at(C.CLAMP + 1) == at(C.CLAMP + 6) == at(2 ** 31 - 1) == at(C.CLAMP)  # counts above the clamp tie
    assert 0 < at(1) < at(C.CLAMP - 1) < at(C.CLAMP)
    assert (key[np.isnan(s) | (s <= 0) | (d != 0) | (f == 0)] == 0).all() and (key >= 0).all()


def test_no_edges(eng):
    z = C.dyadic_case(64, N=40)[0]
    got = run(eng, z, np.zeros(41, np.int64), np.zeros(0, np.int32), 8, score=np.ones(40, np.float32))
    assert all(len(got[k]) == 0 for k in R.EDGE_KEYS)
    assert all(not got[k].any() and len(got[k]) == 40 for k in R.POD_KEYS + ("key",))


def test_arguments_are_validated(eng):
    z, rp, col, _ = C.dyadic_case(5, N=40)
    zd = torch.from_numpy(z).cuda()
    rpd, cld = eng._csr_dev(rp, col)
    for kw in (dict(max_lag=17), dict(max_lag=-1), dict(max_lag=4, slack=5), dict(slack=-1), dict(tau=-0.5)):
        with pytest.raises(native.KrcaError):
            eng.corr_edges_device(zd, rpd, cld, **kw)
    with pytest.raises(native.KrcaError):
        eng.corr_edges(np.zeros((5, 40, 1), np.float32), rp, np.full(len(col), 40, np.int32))  # column out of range


# ---- float data ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def float_case():
    z, rp, col, planted = C.float_case()
    return z, rp, col, planted, R.edges(z, rp, col, 8, 0.5, 0, detail=True)


def test_float_within_the_accumulation_bound(eng, float_case):
    z, rp, col, planted, ref = float_case
    T, tol = z.shape[1], C.tol(z.shape[1])
    score = np.abs(z[:, -1]).astype(np.float32)
    got = run(eng, z, rp, col, 8, 0.5, 0, None, score)
    err0 = np.abs(got["r0"].astype(np.float64) - ref["c"][:, 8]).max()
    cdev = ref["c"][np.arange(len(col)), 8 + got["lag"].astype(np.int64)]  # the reference's c at the device's lag
    errl = np.abs(got["r_lag"].astype(np.float64) - cdev).max()
    print(f"T={T} tol={tol:.3e} max|r0-ref|={err0:.3e} max|r_lag-ref|={errl:.3e}")
    assert err0 <= tol and errl <= tol
    callee = np.repeat(np.arange(len(z)), np.diff(rp))
    is_planted = np.array([(int(j), int(k)) in planted for j, k in zip(col, callee)])
    want = np.array([planted.get((int(j), int(k)), 0) for j, k in zip(col, callee)])
    assert is_planted.sum() == 300 and np.array_equal(got["lag"][is_planted], want[is_planted])
    assert (np.abs(cdev) >= np.abs(ref["c"]).max(axis=1) - 2 * tol).all()
    # counts, dep_best and key follow from the device's own r_lag and lag exactly
    host = R.classify(got["r_lag"], got["lag"], rp, col, len(z), 0.5, 0)
    for name in R.POD_KEYS:
        assert same(got[name], host[name]), name
    assert same(got["key"], R.lead_key(host["dep_lead"], host["caller_follow"], score))
    assert (got["dep_lead"] > 0).sum() > 100 and (got["caller_lead"] > 0).sum() > 50 and (got["key"] > 0).any()
    again = run(eng, z, rp, col, 8, 0.5, 0, None, score)
    for name in ALL + ("key",):
        assert same(got[name], again[name]), name


# ---- mask, tau, slack ------------------------------------------------------------------------------
@pytest.mark.parametrize("slack", [0, 2, 8])
@pytest.mark.parametrize("tau", [0.0, 0.5, 2.0])
def test_mask_tau_slack(eng, slack, tau):
    z, rp, col, _ = C.dyadic_case(65)
    z = (z / 8).astype(np.float32)  # still dyadic; |z| <= 1 gives |c| <= 1, so tau = 2 correlates nothing
    rng = np.random.default_rng(5)
    for k in range(0, 120, 3):  # pairs with |c| >= 62 / 65: a +-1 row and its first caller, the row rolled by <= 3 steps
        if rp[k + 1] > rp[k] and col[rp[k]] != k:
            z[k] = rng.choice(np.array([-1.0, 1.0], np.float32), z.shape[1])
            z[col[rp[k]]] = np.roll(z[k], int(rng.integers(-3, 4)))
    mask = (np.arange(len(z)) % 3 != 1).astype(np.uint8)
    ref = check_exact(eng, z, rp, col, 8, tau, slack, mask)
    check_exact(eng, z, rp, col, 8, tau, slack, None)
    _, _, on = R.active_edges(rp, col, len(z), mask)
    assert 0.3 < on.mean() < 0.6 and not ref["r_lag"][~on].any() and not ref["dep_lead"][mask == 0].any()
    n_corr = sum(int(ref[k].sum()) for k in ("caller_follow", "caller_sync", "caller_lead"))
    assert (n_corr == 0) == (tau == 2.0)
    if slack == 8:
        assert not ref["dep_lead"].any() and not ref["dep_best"].any()


# ---- guard bands -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T,L,long_row", [(64, 8, 2 * C.CHUNK + 1), (257, 16, 0)])
def test_guard_bands_and_poisons(T, L, long_row):
    geng = GuardedEngine()
    z, rp, col, _ = C.dyadic_case(T, long_row=long_row)
    score = (np.arange(len(z)) % 7).astype(np.float32)
    mask = (np.arange(len(z)) % 5 != 2).astype(np.uint8)

    def call(e):
        zd = e._dev(z)
        rpd, cld = e._csr_dev(rp, col)
        out = e.corr_edges_device(zd, rpd, cld, L, 0.25, 1, e._dev(mask))
        key = e.corr_lead_key_device(out, e._dev(score))
        res = {k: v.cpu().numpy() for k, v in out.items()}
        res["key"] = key.cpu().numpy()
        return res

    got = run_poisons(geng, call)
    ref = R.edges(z, rp, col, L, 0.25, 1, mask)
    ref["key"] = R.lead_key(ref["dep_lead"], ref["caller_follow"], score)
    for name in ALL + ("key",):
        assert same(got[name], ref[name]), name


# ---- end to end ------------------------------------------------------------------------------------
def test_coordinator_correlations_end_to_end(eng):
    from krca.agents.coordinator import Coordinator
    from krca.mock import MeshClient
    n, T, span = 2000, 300, 240
    m = synth.make_graph(n, avg_degree=4, seed=8)
    hops = synth.caller_hops(m, m.roots, hops=2, cap=150)
    x, _ = synth.make_metrics_onsets(n, 8, T, seed=8, roots=m.roots, hop_sets=hops, t_root=T - 120, delay=5, jitter=0)
    xd = x.cuda()
    ns = "test-microservices"
    plain = A.strip(Coordinator(MeshClient(m, xd), engine=eng).run_analysis("comprehensive", ns))
    res = A.strip(Coordinator(MeshClient(m, xd), engine=eng, correlations=True, corr_span=span)
                  .run_analysis("comprehensive", ns))
    assert "error" not in res and "correlations" not in plain
    corr = res.pop("correlations")
    assert res == plain
    # the reference, from the rows the device standardised (krca_corr_prepare's z32 times sqrt(T))
    z32 = eng.corr_unit_variance_device(xd[T - span:], 0).cpu().numpy()
    np.testing.assert_allclose((z32.astype(np.float64) ** 2).mean(axis=1), 1.0, atol=1e-4)
    ref = R.edges(z32, m.row_ptr, m.col, 8, 0.5, 0)
    score = eng.rolling_score_device(xd)["score"].cpu().numpy()
    names = m.names()
    ranked = [names.index(r["component"][len("Pod/"):]) for r in res["ranked_root_causes"]]
    want = R.lead_roots(ref, score, m.row_ptr, m.col, 10, ranked)
    assert corr["lead_roots"] == [{"component": f"Pod/{names[i]}", "rank": r + 1, "followers": int(f),
                                   "anomaly": float(s)}
                                  for r, (i, f, s) in enumerate(zip(want["idx"].tolist(), want["followers"].tolist(),
                                                                    want["score"].tolist()))]
    assert len(corr["lead_roots"]) > 0 and corr["params"]["span"] == span
    assert [(f["component"], f["follows"], f["lag_steps"]) for f in corr["followers"]] == [
        (f"Pod/{names[p]}", f"Pod/{names[want['explained'][p][0]]}", want["explained"][p][1])
        for p in ranked if p in want["explained"]]
    # NativeEngine.lead_roots on host copies of the outputs gives the same answer as the device path
    host = eng.corr_edges(xd, m.row_ptr, m.col, span=span)
    lr = eng.lead_roots(host, score, k=10, explain=ranked, row_ptr=m.row_ptr, col=m.col)
    assert lr["idx"].tolist() == want["idx"].tolist() and set(lr["explained"]) == set(want["explained"])
