"""The fixtures of the GPU tests that move an argument off the one value the suite held it at
(scorer threshold, correlation launch forms, follower clamp, top-k ties), checked on the host alone:
the references agree with each other and the shapes reach what they are meant to reach, so a
failing device test points at the device."""
import numpy as np
import pytest

import corr_edges_cases as CC
import corr_edges_ref as CR
import oracle
import timeline_cases as TC
import timeline_ref as TR


# ---- scorer threshold ------------------------------------------------------------------------------
@pytest.mark.parametrize("W", TC.THR_WINDOWS)
@pytest.mark.parametrize("thr", TC.THRS)
def test_threshold_twin_and_float64_agree(W, thr):
    """oracle/krca_oracle.c (the arithmetic the device mirrors) and the independent float64 prefix-sum
    formulation count the same exceedances on all but 0.5 % of the pods, at every threshold."""
    P, M, T, _ = TC.THR_SHAPE
    twin, n64, agree = TC.threshold_refs(W, thr)
    bad = int((~agree).sum())
    print(f"W={W} thr={thr!r}: twin total {int(twin['n_exceed'].sum())}, float64 total {int(n64.sum())}, "
          f"pods that differ {bad} of {P}")
    assert bad <= TC.THR_MAX_DISAGREE * P
    if W == 60 and thr in TC.THR_TOTALS_W60:
        assert int(n64.sum()) == TC.THR_TOTALS_W60[thr]
    if thr == 0.0:  # strict '>': only A == 0 or a flat window fails to exceed
        assert int(n64.sum()) > 0.99 * P * M * (T - W)
    if thr == 1000.0:
        assert int(n64.sum()) == 0 and not twin["n_exceed"].any()


def test_threshold_narrowing_matters_on_this_series():
    """The thresholds float32 does not hold are told apart from their float64 values by the C twin's
    argument type alone: it takes z_thr as float, so a float64 threshold handed to it is rounded."""
    for thr in (2.7, 3.3, 1.1, 1e-3):
        assert float(np.float32(thr)) != thr
    for thr in (0.5, 0.0, 1000.0):
        assert float(np.float32(thr)) == thr
    x = TC.threshold_series()
    a = oracle.c_rolling_score(x, 60, 2.7)
    b = oracle.c_rolling_score(x, 60, float(np.float32(2.7)))
    assert np.array_equal(a["n_exceed"], b["n_exceed"])


def test_threshold_series_dyadic_timeline_is_not_vacuous():
    """The quantised series holds episodes at both timeline thresholds and both windows, and the
    NumPy timeline counts what the C twin counts on it (the twin runs the kernels' fma arithmetic)."""
    xq = TC.threshold_series(dyadic=True)
    assert np.array_equal(xq * 16, np.round(xq * 16)) and xq.min() >= 0 and xq.max() <= 100
    for W in (10, 7):
        for thr in TC.THR_STREAM_THRS:
            ref = TR.timeline(xq, W, thr, 3, 3)
            assert np.array_equal(ref["n_exceed"], oracle.c_rolling_score(xq, W, thr)["n_exceed"]), (W, thr)
            assert (ref["onset"] >= 0).sum() > 5, (W, thr)


@pytest.mark.parametrize("thr", TC.THR_STREAM_THRS)
def test_threshold_stream_reference_is_not_vacuous(thr):
    """The streaming reference over the stream cases: episodes at every horizon, the horizon changes
    what is reported, and every window of the list ends at a different phase of the series."""
    assert sum(TC.THR_STREAM_WINDOWS) == TC.THR_SHAPE[2]
    last = {}
    for H in TC.THR_STREAM_HORIZONS:
        ref = TC.threshold_stream_ref(thr, H)
        n = [int((r["onset"] >= 0).sum()) for r in ref]
        print(f"thr={thr} H={H}: pods with an episode after each window {n}")
        assert len(ref) == len(TC.THR_STREAM_WINDOWS) and n[:3] == [0, 0, 0] and n[3] > 0 and n[4] > 0, H  # t = 53 <= W
        last[H] = ref[-1]
    if thr == 0.5:  # most steps exceed: every pod holds episodes that a horizon of 32 steps has dropped
        assert any(last[32][k].tobytes() != last[64][k].tobytes() for k in ("onset", "count"))


# ---- correlation launch forms ----------------------------------------------------------------------
def test_corr_launch_shapes_reach_every_form():
    forms = {s: CC.launch_form(*s) for s in CC.LAUNCH_SHAPES}
    assert forms == {(4080, 8): (4, 16), (4081, 8): (1, 4), (4084, 8): (1, 16), (16368, 8): (1, 16),
                     (16384, 0): (1, 16), (4068, 16): (1, 16)}
    for T, L in CC.LAUNCH_SHAPES:
        assert 64 * T < 2 ** 24  # |S| <= 64 T: float32 accumulation is exact in any order
    # the largest accepted shapes: one more step is refused
    assert all(CC.launch_form(T, L) is None for T, L in CC.REFUSED_SHAPES)
    assert {(T - 1, L) for T, L in CC.REFUSED_SHAPES} <= set(CC.LAUNCH_SHAPES) | {(16352, 16)}
    assert CC.launch_form(16352, 16) == (1, 16)
    for T in CC.MISALIGNED_T:
        assert T % 4 == 0 and CC.launch_form(T, 8, aligned=False)[1] == 4 and CC.launch_form(T, 8)[1] == 16
    assert CC.launch_form(64, 8)[0] == 4 and CC.launch_form(4084, 8)[0] == 1
    assert all(CC.launch_form(T, L) == (4, 16 if T % 4 == 0 else 4) for T, L in CC.DYADIC_SHAPES)  # what ran before


@pytest.mark.parametrize("T,L", CC.LAUNCH_SHAPES)
def test_corr_launch_shapes_are_exact_and_not_vacuous(T, L):
    z, rp, col = CC.launch_case(T)
    assert z.shape == (CC.LAUNCH_N, T) and np.abs(z).max() <= 8 and np.array_equal(z, np.round(z))
    S = CR.lag_sums(z, rp, col, L)
    print(f"T={T} L={L}: max|S| = {int(np.abs(S).max())}")
    assert np.abs(S).max() <= 64 * T < 2 ** 24
    ref = CR.edges(z, rp, col, L, CC.LAUNCH_TAU, 1 if L >= 2 else 0)
    if L > 0:
        print(f"  dep_lead {int(ref['dep_lead'].sum())}, caller_lead {int(ref['caller_lead'].sum())}")
        # ~1400 edges whose best lag is spread over the 2 L + 1 lags: 7 / 17 of them past slack = 1 on
        # either side at L = 8, less what tau cuts; a fifth of that share is asked for
        n_edges = int(rp[-1])
        assert n_edges > 1000 and min(ref["dep_lead"].sum(), ref["caller_lead"].sum()) >= n_edges * 7 // 17 // 5 > 100
        assert (ref["dep_lead"] > 0).sum() > 20 and (ref["caller_lead"] > 0).sum() > 20
        assert 0 < (np.abs(ref["r_lag"]) > CC.LAUNCH_TAU).sum() < n_edges  # tau decides on both sides
    else:
        assert ref["caller_sync"].sum() > 100 and not ref["dep_lead"].any()


# ---- follower clamp --------------------------------------------------------------------------------
def test_follower_clamp_references():
    """The two restatements of the key formulas against hand-written keys at the clamp."""
    bits = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
    for f, want in ((1, 1), (CC.CLAMP - 1, CC.CLAMP - 1), (CC.CLAMP, CC.CLAMP), (CC.CLAMP + 1, CC.CLAMP),
                    (2 ** 31 - 1, CC.CLAMP)):
        key = CR.lead_key(np.array([0], np.int32), np.array([f], np.int32), np.array([1.5], np.float32))
        assert int(key[0]) == (want << 32) | bits(1.5)
        prec = dict(dep_earlier=np.zeros(1, np.int32), caller_later=np.array([f], np.int32),
                    caller_concurrent=np.zeros(1, np.int32))
        assert int(TR.first_mover_key(np.array([5], np.int32), np.array([1.5], np.float32), prec)[0]) == \
            (want << 32) | bits(1.5)
    d, f, s = CC.lead_key_case()
    key = CR.lead_key(d, f, s)
    assert len(key) == len(CC.FOLLOWERS) * 2 * len(CC.KEY_SCORES)
    sel = (d == 0) & (f > 0) & (s > 0)
    assert sel.sum() == 6 * 3 and (key[~sel] == 0).all() and (key[sel] > 0).all()  # denormal, 1.5, inf
    assert int(key[sel & (s == np.float32(CC.DENORMAL))].min()) == (1 << 32) | 1
    on, pk, prec = TC.first_mover_key_case()
    key = TR.first_mover_key(on, pk, prec)
    assert len(key) == len(TC.FOLLOWER_PAIRS) * 2 * 3 * len(TC.KEY_PEAKS)
    total = prec["caller_later"].astype(np.int64) + prec["caller_concurrent"]
    assert total.max() == 2 ** 32 - 2 and ((total > TC.CLAMP) & (prec["caller_later"] <= TC.CLAMP)
                                            & (prec["caller_concurrent"] <= TC.CLAMP)).any()
    assert ((key >> 32) <= TC.CLAMP).all() and (key >= 0).all()
    assert ((key >> 32)[(on >= 0) & (prec["dep_earlier"] == 0)] == np.minimum(total, TC.CLAMP)[
        (on >= 0) & (prec["dep_earlier"] == 0)]).all()


# ---- template histograms on given hashes -------------------------------------------------------------
def test_template_slot_reference_and_layouts():
    import test_gpu_kernels as K
    PAD = np.uint64(2 ** 64 - 1)
    h = np.array([5, 5, PAD, 0, 7, 7, 7, 9], np.uint64)
    oh, oc, nt = oracle.template_hist_slots(h, [3, 0, 4], [0, 3, 4], 111, -7)
    assert oh.tolist() == [5, int(PAD), 0, 111, 7, 9, 0, 0] and oc.tolist() == [2, 1, 0, -7, 3, 1, 0, 0]
    assert nt.tolist() == [2, 0, 2]
    oh, oc, nt = oracle.template_hist_slots(h, [1, 2], [3, 0], 111, -7)  # a real hash 0, ranges out of order
    assert oh.tolist() == [5, 0, 111, 0, 111, 111, 111, 111] and oc.tolist() == [2, 0, -7, 1, -7, -7, -7, -7]
    for name, (hash_, dl, d0) in K.template_layouts().items():
        assert len(dl) == len(d0) and (d0 >= 0).all() and (d0 + dl <= len(hash_)).all(), name
        used = np.zeros(len(hash_), np.int32)
        for n, lo in zip(dl.tolist(), d0.tolist()):
            used[lo:lo + n] += 1
        assert used.max() == 1, name  # ranges never overlap
        assert (used.min() == 0) == (name == "gaps"), name
        span = int((d0 + dl).max() - d0.min())
        consecutive = bool((d0[1:] == (d0 + dl)[:-1]).all())
        # a 256-container block is staged in LDS iff its ranges are consecutive and span <= 1024 lines
        want = dict(order=(False, True), gaps=(False, False), reverse=(False, False), span1024=(True, True),
                    span1025=(False, True), mixed1090=(False, True), mixed1024=(True, True))[name]
        assert (len(dl) == 256 and span <= 1024, consecutive) == want, (name, span)
    lay = K.template_layouts()
    assert sorted(set(lay["order"][1].tolist())) == sorted(K.TMPL_SIZES)
    for name in ("mixed1090", "mixed1024"):
        assert {9, 65} <= set(lay[name][1].tolist())


# ---- top-k -------------------------------------------------------------------------------------------
def test_topk_ref_treats_the_two_zeros_as_equal():
    v = np.array([0.0, -0.0, -0.0, 0.0, -1.0, 0.0], np.float32)
    idx, val = oracle.topk_ref(v, 5)
    assert idx.tolist() == [0, 1, 2, 3, 5]
    assert val.view(np.uint32).tolist() == v[[0, 1, 2, 3, 5]].view(np.uint32).tolist()
    vi = np.array([np.iinfo(np.int64).min, 3, np.iinfo(np.int64).min, -5], np.int64)
    idx, val = oracle.topk_ref(vi, 4)  # INT64_MIN is the smallest key (its negation wraps onto itself)
    assert idx.tolist() == [1, 3, 0, 2] and val.tolist() == vi[[1, 3, 0, 2]].tolist()
