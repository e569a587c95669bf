"""The pipelined scorer's rotating sample ring (csrc/score_walk.h, rolling_score_pipe) on the device,
where the ring's phases meet the end of the series: T around W + D, around one and two rounds of
R = W + D steps past the window, and the benchmark's T = 1440; P*M is never a multiple of the
256-series workgroup.  Under both row sources (KRCA_SCORE_IMPL 0: span descriptors, 4: one
descriptor per row) krca_rolling_score's n_exceed and flags equal oracle.c_rolling_score's, its
z_last and score equal the KRCA_SCORE_IMPL=1 kernel's in bits, and krca_rolling_timeline's six
outputs equal tests/timeline_ref.py's with its four scoring outputs equal to the scorer's in bits.
The CPU side of the same walk is tests/test_score_walk_cpu.py."""
import numpy as np
import pytest
import torch

import oracle
import timeline_cases as C
import timeline_ref as R
from krca import native

pytestmark = pytest.mark.gpu

PODS = (1, 33, 129, 1000)
M = 8
PREFETCH = {60: 20, 30: 15, 20: 10, 15: 15, 10: 10}  # csrc/score_walk.h prefetch_rows()
SIX = ("onset", "last", "count", "peak", "lead", "n_metrics")
FOUR = ("z_last", "score", "n_exceed", "flags")
IMPLS = ((0, "pipe"), (4, "pipe_rows"))


def _ring_edge_T(W):
    D = PREFETCH[W]
    Rr = W + D
    return (W + 1, W + D - 1, W + D, W + D + 1, Rr + W - 1, Rr + W, Rr + W + 1, 2 * Rr + W + 1, 1440)


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


def _bits(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def check(eng, x, W, timeline=True):
    """x float32 [T, P, M] on the host.  The references are computed once and serve both row sources."""
    T, P, Mm = x.shape
    xd = torch.from_numpy(x).cuda()
    want = oracle.c_rolling_score(x, W, 3.0)
    with native.tune(eng.lib, KRCA_SCORE_IMPL=1):
        assert native.SCORE_VARIANTS[eng.lib.krca_rolling_score_variant(P, Mm, T, W)] == "ring"
        ring = {k: v.clone() for k, v in eng.rolling_score_device(xd, W, 3.0).items()}
    tl = R.timeline(x, W, 3.0, 3, 3) if timeline else None
    for impl, variant in IMPLS:
        where = (variant, T, P, W)
        with native.tune(eng.lib, KRCA_SCORE_IMPL=impl):
            assert native.SCORE_VARIANTS[eng.lib.krca_rolling_score_variant(P, Mm, T, W)] == variant, where
            got = eng.rolling_score_device(xd, W, 3.0)
            assert np.array_equal(got["n_exceed"].cpu().numpy(), want["n_exceed"]), where
            assert np.array_equal(got["flags"].cpu().numpy(), want["flags"]), where
            for k in FOUR:
                assert _bits(got[k], ring[k]), (k,) + where
            if not timeline:
                continue
            gt = eng.rolling_timeline_device(xd, W, 3.0, 3, 3)
            for k in SIX:
                g = gt[k].cpu().numpy()
                assert g.dtype == tl[k].dtype and g.shape == tl[k].shape, (k,) + where
                assert np.array_equal(g.view(np.uint32) if k == "peak" else g,
                                      tl[k].view(np.uint32) if k == "peak" else tl[k]), (k,) + where
            for k in FOUR:
                assert _bits(gt[k], got[k]), (k,) + where
    return want


@pytest.mark.parametrize("T", _ring_edge_T(60))
def test_ring_meets_the_end_of_the_series_w60(eng, T):
    n = 0
    for P in PODS:
        want = check(eng, C.dyadic_metrics(P, M, T, 60, seed=7 * T + P), 60)
        n += int(want["n_exceed"].sum())
    assert n > 0 or T < 62  # the fixtures do plant exceedances


@pytest.mark.parametrize("W", (30, 20, 15, 10))
def test_other_pipelined_windows_just_past_the_prefetch(eng, W):
    T = W + PREFETCH[W] + 2
    for P in PODS:
        check(eng, C.dyadic_metrics(P, M, T, W, seed=11 * W + P), W)


def test_non_finite_samples(eng):
    """NaN and +-Inf in the window, leaving it, and at the last step: the scorer's outputs stay the
    oracle's and the ring kernel's (the timeline reference is defined on finite fixtures only)."""
    W, T, P = 60, 221, 129
    x = C.dyadic_metrics(P, M, T, W, seed=3).copy()
    rng = np.random.default_rng(5)
    for v in (np.nan, np.inf, -np.inf):
        for _ in range(40):
            x[rng.integers(0, T), rng.integers(0, P), rng.integers(0, M)] = v
    x[T - 1, 0, 2] = np.inf
    x[T - 1, 1, 3] = np.nan
    check(eng, x, W, timeline=False)
