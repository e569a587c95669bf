"""krca_rolling_timeline, krca_rca_precede and krca_rca_first_mover_key on the device against
tests/timeline_ref.py (bit-exact: the fixtures are dyadic, see that file), and the timeline call's
four scoring outputs against krca_rolling_score bit for bit."""
import numpy as np
import pytest
import torch

import timeline_cases as C
import timeline_ref as R
from krca import native, synth

pytestmark = pytest.mark.gpu

SIX = ("onset", "last", "count", "peak", "lead", "n_metrics")
PREC = ("dep_earlier", "dep_concurrent", "caller_later", "caller_concurrent", "caller_earlier", "dep_first")


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


def check_timeline(eng, x, W, thr, G, Rm, variant=None):
    """The six timeline outputs and n_exceed equal the reference's; the scoring outputs equal
    krca_rolling_score's."""
    T, P, M = x.shape
    if variant is not None:
        assert native.SCORE_VARIANTS[eng.lib.krca_rolling_score_variant(P, M, T, W)] == variant, (T, P, M, W)
    xd = torch.from_numpy(x).cuda()
    got = eng.rolling_timeline_device(xd, W, thr, G, Rm)
    ref = R.timeline(x, W, thr, G, Rm)
    for k in SIX + ("n_exceed",):
        g = got[k].cpu().numpy()
        assert g.dtype == ref[k].dtype and g.shape == ref[k].shape, k
        bad = np.flatnonzero(g.view(np.uint32) != ref[k].view(np.uint32)) if k == "peak" else np.flatnonzero(g != ref[k])
        assert len(bad) == 0, (k, (T, P, M, W), bad[:5], g[bad[:5]], ref[k][bad[:5]])
    sc = eng.rolling_score_device(xd, W, thr)
    for k in ("z_last", "score", "n_exceed", "flags"):
        assert torch.equal(got[k].view(torch.uint8), sc[k].view(torch.uint8)), k
    return ref


@pytest.mark.parametrize("W,variant", [(60, "pipe"), (30, "pipe"), (10, "pipe"), (7, "reread")])
def test_timeline_matches_reference_over_T(eng, W, variant):
    """P*M = 296: a partly filled second workgroup.  T straddles the pipelined kernel's full-block /
    final-block split; T = W is the empty result (the re-reading form: no pipelined kernel runs at
    T <= W)."""
    n_eps = 0
    for T in (W, W + 1, 2 * W, 2 * W + 1, 3 * W - 1, 200):
        x = C.dyadic_metrics(37, 8, T, W, seed=100 * W + T)
        ref = check_timeline(eng, x, W, 3.0, 3, 3, variant if T > W else None)
        n_eps += int((ref["onset"] >= 0).sum())
        if T == W:
            assert (ref["onset"] == -1).all()
    assert n_eps > 20  # the fixtures do plant episodes


@pytest.mark.parametrize("P,M,T,W", [(300, 1, 200, 30), (150, 2, 121, 60), (9, 64, 200, 10), (70, 4, 150, 7),
                                     (5, 64, 100, 7)])
def test_timeline_matches_reference_over_M(eng, P, M, T, W):
    ref = check_timeline(eng, C.dyadic_metrics(P, M, T, W, seed=P + M, n_shift=max(1, P // 2)), W, 2.5, 3, 3)
    assert (ref["onset"] >= 0).any() and ((ref["n_metrics"] > 1).any() or M == 1)


@pytest.mark.parametrize("G,Rm", [(0, 1), (5, 2), (200, 1), (3, 1000)])
def test_timeline_gap_and_count_parameters(eng, G, Rm):
    check_timeline(eng, C.dyadic_metrics(37, 8, 200, 60, seed=G + Rm), 60, 3.0, G, Rm, "pipe")


def test_timeline_per_row_descriptors(eng):
    x = C.dyadic_metrics(37, 8, 200, 60, seed=4)
    with native.tune(eng.lib, KRCA_SCORE_IMPL=4):
        check_timeline(eng, x, 60, 3.0, 3, 3, "pipe_rows")
        check_timeline(eng, C.dyadic_metrics(37, 8, 61, 30, seed=5), 30, 3.0, 3, 3, "pipe_rows")
    with native.tune(eng.lib, KRCA_SCORE_IMPL=1):  # a variant with no timeline form: the re-reading kernel
        check_timeline(eng, x, 60, 3.0, 3, 3, "ring")


@pytest.mark.parametrize("W,variant", [(10, "pipe"), (7, "reread")])
@pytest.mark.parametrize("thr", C.THR_STREAM_THRS)
def test_timeline_thresholds(eng, thr, W, variant):
    """Thresholds off 3.0 / 2.5 (2.7 is no float32 value and its square is not dyadic; 0.5 makes most
    steps exceed, so episodes chain and split everywhere) on the threshold series rounded to 1/16."""
    ref = check_timeline(eng, np.array(C.threshold_series(dyadic=True)), W, thr, 3, 3, variant)
    assert (ref["onset"] >= 0).sum() > 5  # (tests/test_argument_cases_cpu.py: the reference alone)


def test_first_mover_key_follower_clamp(eng):
    """Fabricated follower counts around 2^20 - 1 (the key's follower field holds 20 bits), alone and
    as sums of two counts below it, crossed with dep_earlier, onset and peak: bit-equal to the
    reference's formula; counts above the clamp tie, 2^20 - 2 still ranks below 2^20 - 1."""
    onset, peak, prec = C.first_mover_key_case()
    dev = {k: torch.from_numpy(v).cuda() for k, v in prec.items()}
    key = eng.first_mover_key_device(torch.from_numpy(onset).cuda(), torch.from_numpy(peak).cuda(), dev).cpu().numpy()
    ref = R.first_mover_key(onset, peak, prec)
    assert key.dtype == ref.dtype and np.array_equal(key, ref), np.flatnonzero(key != ref)[:5]

    def at(later, conc):
        sel = (onset == 5) & (prec["dep_earlier"] == 0) & (peak == np.float32(1.5)) \
            & (prec["caller_later"] == later) & (prec["caller_concurrent"] == conc)
        return int(key[sel][0])

    top = at(C.CLAMP, 0)
    assert top == (C.CLAMP << 32) | int(np.float32(1.5).view(np.uint32))
    assert at(C.CLAMP + 1, 0) == at(C.CLAMP + 6, 0) == at(2 ** 31 - 1, 0) == at(0, C.CLAMP + 1) == top
    assert at(1 << 19, 1 << 19) == at(C.CLAMP, C.CLAMP) == at(2 ** 31 - 1, 2 ** 31 - 1) == top
    assert at(1 << 19, (1 << 19) - 1) == at(C.CLAMP - 1, 1) == at(1, C.CLAMP - 1) == top
    assert 0 < at(1, 0) < at(C.CLAMP - 1, 0) == at(1 << 19, (1 << 19) - 2) < top
    assert (key[(onset < 0) | (prec["dep_earlier"] != 0)] == 0).all()


def test_timeline_hand_fixture(eng):
    x = C.episode_fixture()
    ref = check_timeline(eng, x, C.W, C.THR, C.G, C.MINC, "pipe")
    assert ref["onset"].tolist() == [80, C.T - 3, -1, -1] and ref["n_metrics"].tolist() == [2, 1, 0, 0]
    check_timeline(eng, x, C.W, C.THR, 0, 1)
    check_timeline(eng, x[:C.W], C.W, C.THR, C.G, C.MINC)
    xn = x.copy()
    xn[C.T - 2, 1, 3] = np.nan  # a NaN never exceeds
    got = eng.rolling_timeline_device(torch.from_numpy(xn).cuda(), C.W, C.THR, C.G, C.MINC)
    assert got["onset"].tolist() == [80, -1, -1, -1] and got["count"].tolist() == [6, 0, 0, 0]


@pytest.mark.parametrize("W", [60, 7])
def test_scoring_outputs_bit_identical_to_rolling_score(eng, W):
    """Ordinary float32 data: z_last, score, n_exceed, flags of the timeline call == krca_rolling_score."""
    m = synth.make_graph(1000, avg_degree=4, seed=2)
    x = synth.make_metrics(1000, 8, 500, seed=W, roots=m.roots, spike_steps=30).cuda()
    x[7, 3, 2] = float("nan")
    tl = eng.rolling_timeline_device(x, W, 3.0, 3, 3)
    sc = eng.rolling_score_device(x, W, 3.0)
    for k in ("z_last", "score", "n_exceed", "flags"):
        assert torch.equal(tl[k].view(torch.uint8), sc[k].view(torch.uint8)), k
    assert int(sc["n_exceed"].sum()) > 1000
    if W == 60:
        # the roots' 12 sigma spike starts at T - 30; an onset is earlier only through noise exceedances
        # chained in front of it, each at most G = 3 steps before the next (two of them: 6 steps)
        on = tl["onset"].cpu().numpy()
        assert all(470 - 6 <= on[r] <= 470 for r in m.roots), on[m.roots]


# ---- precedence ---------------------------------------------------------------------------------
def check_precede(eng, onset, peak, rp, col, slack, k=10):
    got = eng.rca_precede(onset, rp, col, slack)
    ref = R.precede(onset, rp, col, slack)
    for name in PREC:
        assert got[name].dtype == ref[name].dtype and np.array_equal(got[name], ref[name]), (name, slack)
    dev = {n: torch.from_numpy(got[n]).cuda() for n in PREC}
    key = eng.first_mover_key_device(torch.from_numpy(onset).cuda(), torch.from_numpy(peak).cuda(), dev)
    rkey = R.first_mover_key(onset, peak, ref)
    assert np.array_equal(key.cpu().numpy(), rkey)
    idx, val = eng.topk_device(key, k)
    ridx, rval = R.topk(rkey, k)
    assert idx.cpu().numpy().tolist() == ridx.tolist() and val.cpu().numpy().tolist() == rval.tolist()
    return ref, rkey


@pytest.mark.parametrize("slack", [0, 5])
def test_precede_hand_graph(eng, slack):
    rp, col = C.csr(C.EDGES, len(C.ONSET))
    ref, key = check_precede(eng, C.ONSET, C.PEAK, rp, col, slack, k=8)
    want = C.EXPECT[slack]
    for name in PREC:
        assert ref[name].tolist() == want[name]
    fm = eng.first_movers(dict(onset=torch.from_numpy(C.ONSET).cuda(), peak=torch.from_numpy(C.PEAK).cuda(),
                               lead=torch.zeros(8, dtype=torch.int8).cuda()), rp, col, slack, k=8, explain=[2, 6, 0, 5])
    assert fm["idx"].tolist() == want["top"] and fm["explained"] == {2: (0, 20), 6: (1, 40)}


@pytest.fixture(scope="module")
def mesh():
    """2000 pods; one row is given 2100 more (repeated) callers, so lanes stride and a row passes 2048."""
    m = synth.make_graph(2000, avg_degree=16, seed=3)
    rng = np.random.default_rng(3)
    deg = np.diff(m.row_ptr)
    big = int(np.argmax(deg))
    callee = np.concatenate([np.repeat(np.arange(2000), deg), np.full(2100, big)])
    caller = np.concatenate([m.col.astype(np.int64), rng.integers(0, 2000, 2100)])
    rp, col = C.csr(list(zip(caller.tolist(), callee.tolist())), 2000)
    d = np.diff(rp)
    assert d.max() > 2048 and (d > 64).sum() > 5
    return m, rp, col


@pytest.mark.parametrize("slack", [0, 5])
def test_precede_mesh(eng, mesh, slack):
    m, rp, col = mesh
    rng = np.random.default_rng(11)
    onset = np.where(rng.random(2000) < 1 / 3, rng.integers(100, 140, 2000), -1).astype(np.int32)
    onset[np.argmax(np.diff(rp))] = 120
    peak = np.where(onset >= 0, rng.integers(48, 200, 2000) / 16.0, 0).astype(np.float32)
    ref, key = check_precede(eng, onset, peak, rp, col, slack, k=16)
    assert (ref["dep_earlier"] > 0).sum() > 50 and (ref["caller_concurrent"] > 0).sum() > 50
    assert 0 < (key > 0).sum() < (onset >= 0).sum()


# ---- end to end ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def onsets_case(mesh):
    """make_metrics_onsets over the 2000-pod mesh, quantised to 1/16, and the reference's timeline."""
    m, rp, col = mesh
    hops = synth.caller_hops(m, m.roots, hops=2, cap=150)
    x, planted = synth.make_metrics_onsets(2000, 8, 300, seed=9, roots=m.roots, hop_sets=hops, t_root=200, delay=12,
                                           jitter=2)
    x = (torch.round(x * 16.0) / 16.0).contiguous()
    return x, planted, R.timeline(x.numpy(), 60, 3.0, 3, 3)


def test_first_movers_end_to_end(eng, mesh, onsets_case):
    m, rp, col = mesh
    x, planted, ref = onsets_case
    tl = eng.rolling_timeline(x.cuda(), 60, 3.0, 3, 3)
    for k in SIX:
        assert np.array_equal(tl[k + "_host"], ref[k]), k
    # the planted roots are found where they were planted
    assert all(abs(int(ref["onset"][r]) - int(planted[r])) <= 3 for r in m.roots)
    some = [int(p) for p in np.flatnonzero(planted >= 0)[:40]]
    for slack in (0, 5):
        got = eng.first_movers(tl, rp, col, slack, k=10, explain=some)
        want = R.first_movers(ref, rp, col, slack, k=10, explain=some)
        for k in ("idx", "onset", "lead", "peak", "followers"):
            assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, (k, slack)
        assert got["explained"] == want["explained"] and len(got["idx"]) == 10
    assert want["explained"]


def test_metrics_agent_timeline_key(eng, mesh):
    """Roots shifted by 12 sigma three steps before the end: three exceedances each (a sustained
    episode) and the largest scores at T - 1, so they lead the reported anomalies; the rest of the 16
    are noise maxima, most without an episode."""
    import agent_cases as A
    m, _, _ = mesh
    T = 300
    x, _ = synth.make_metrics_onsets(2000, 8, T, seed=10, roots=m.roots, t_root=T - 3, jitter=0)
    x = (torch.round(x * 16.0) / 16.0).contiguous()
    ref = R.timeline(x.numpy(), 60, 3.0, 3, 3)
    names = m.names()
    xd = x.cuda()
    plain = A.strip(A.MetricsAgent(C.BulkClient(names, xd), engine=eng, anomaly_topk=16).analyze("ns"))
    res = A.strip(A.MetricsAgent(C.BulkClient(names, xd), engine=eng, anomaly_topk=16, timeline=True).analyze("ns"))
    assert "error" not in plain and "anomaly_timeline" not in plain
    rows = res.pop("anomaly_timeline")
    assert res == plain and len(rows) == len(res["anomalies"]) == 16
    for a, row in zip(res["anomalies"], rows):
        p = names.index(a["resource"][len("Pod/"):])
        assert row == {"resource": a["resource"], "onset_step": int(ref["onset"][p]), "last_step": int(ref["last"][p]),
                       "episode_count": int(ref["count"][p]), "lead_metric": int(ref["lead"][p]),
                       "n_metrics": int(ref["n_metrics"][p])}
    found = {r["resource"]: r for r in rows}
    for r in m.roots:  # onset: the shift's first step, or earlier by chained noise exceedances (2 x G)
        row = found[f"Pod/{names[r]}"]
        assert T - 3 - 6 <= row["onset_step"] <= T - 3 and row["last_step"] == T - 1 and row["n_metrics"] >= 1
