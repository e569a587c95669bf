"""The pipelined scorer's per-series walk (csrc/score_walk.h: prologue, unrolled rounds over the
rotating sample ring, guarded final round, slot and row schedule) instantiated on the CPU over a
plain array (tests/host/score_walk_host.cpp, built here as host code) for every shipped (W, D) and
the W = 60 candidates of the prefetch-distance A/B.

For every T in [W + 1, W + 3R + 1], R = W + D, so that every phase of the ring meets the end of the
series: s1, s2, the exceedance count and the last-step A and B equal, bit for bit, the plain loop
of oracle/krca_oracle.c (restated in the host file); the count and z_last computed from A and B
equal oracle.c_rolling_score's; every row < T is requested exactly once; and a row >= T never
contributes (the source returns NaN for such a row in a second walk, and nothing changes)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kubernetes-rca-system_amd", "csrc")
SHIPPED_W = (60, 30, 20, 15, 10)
CANDIDATES_60 = (16, 20, 24)
THR = 3.0


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("swalk") / "libswalk.so")
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                    "-Wall", "-I", CSRC, os.path.join(HERE, "host", "score_walk_host.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    lib.swalk_prefetch_rows.restype = i32
    lib.swalk_prefetch_rows.argtypes = [i32]
    lib.swalk_run.restype = i32
    lib.swalk_run.argtypes = [i32, i32, vp, i64, i32, f64, i32, vp, vp, vp, i32]
    lib.swalk_ref.restype = None
    lib.swalk_ref.argtypes = [i32, vp, i64, i32, f64, vp, vp]
    return lib


def _series(T, seed):
    """[T][8] float32: noise around a level, a series with spikes (exceedances), a constant one
    (variance under the floor), a huge-magnitude one, and series holding NaN, +Inf, -Inf."""
    rng = np.random.default_rng(seed)
    x = (50.0 + 10.0 * rng.standard_normal((T, 8))).astype(np.float32)
    spikes = rng.random(T) < 0.08
    x[spikes, 1] += 80.0
    x[:, 2] = 42.5
    x[:, 3] *= np.float32(3e18)
    x[rng.integers(0, T), 4] = np.nan
    x[rng.integers(0, T), 5] = np.inf
    x[rng.integers(0, T), 6] = -np.inf
    x[T - 1, 7] = np.inf  # a non-finite last step
    return np.ascontiguousarray(x)


def _same_bits(a, b):
    """Equal as bit patterns; two NaNs are equal whatever their payloads."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _pairs(lib):
    shipped = [(W, lib.swalk_prefetch_rows(W)) for W in SHIPPED_W]
    return shipped + [(60, D) for D in CANDIDATES_60 if (60, D) not in shipped]


def test_shipped_prefetch_distances(walk):
    """One D per pipelined window; W = 60's keeps krca_rolling_score_variant's answers at 1M x 8 and
    4M x 8 pods (the rule 4*S*D < 2^31 of the span descriptors)."""
    for W in SHIPPED_W:
        assert 1 <= walk.swalk_prefetch_rows(W) <= 24
    D = walk.swalk_prefetch_rows(60)
    assert D in CANDIDATES_60
    assert 4 * 8_000_000 * D < 2 ** 31 <= 4 * 32_000_000 * D


def test_walk_matches_plain_loop_and_requests_each_row_once(walk):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    thr2 = float(np.float32(THR)) ** 2
    checked = 0
    for W, D in _pairs(walk):
        R = W + D
        for T in range(W + 1, W + 3 * R + 2):
            x = _series(T, 1000 * W + T)
            M = x.shape[1]
            ref = oracle.c_rolling_score(x.reshape(T, M, 1), W, THR)  # every series a pod of its own
            for m in range(M):
                xs = x[:, m:]
                got, want, poisoned = np.zeros(4), np.zeros(4), np.zeros(4)
                cg, cw, cp = (np.zeros(1, np.int32) for _ in range(3))
                log = np.full(T + 2 * R, -1, np.int32)
                n = walk.swalk_run(W, D, p(xs), M, T, thr2, 0, p(got), p(cg), p(log), log.size)
                assert 0 <= n <= log.size, (W, D, T, n)
                walk.swalk_ref(W, p(xs), M, T, thr2, p(want), p(cw))
                where = f"W={W} D={D} T={T} series {m}"
                assert _same_bits(got, want) and cg[0] == cw[0], where
                # the oracle's outputs from the same state
                epsB = 1e-12 * W * W
                z = np.float32(got[2] / np.sqrt(got[3])) if got[3] > epsB else np.float32(0)
                assert cg[0] == ref["n_exceed"][m], where
                assert _same_bits(np.float64(z), np.float64(ref["z_last"][m, 0])), where
                # every row < T exactly once; requests past T - 1 stay within one round
                req = log[:n]
                assert np.array_equal(np.sort(req[req < T]), np.arange(T)), where
                assert req.max() < T + R, where
                # ... and what a request past the end returns is never used
                n2 = walk.swalk_run(W, D, p(xs), M, T, thr2, 1, p(poisoned), p(cp), p(log), log.size)
                assert n2 == n and _same_bits(poisoned, got) and cp[0] == cg[0], where
                checked += 1
    assert checked == sum(3 * (W + D) + 1 for W, D in _pairs(walk)) * 8


def test_unknown_pair_is_refused(walk):
    assert walk.swalk_run(60, 7, None, 1, 100, 9.0, 0, None, None, None, 0) == -1
