"""Trace analytics on the device (csrc/trace.hip): every output bit-exact against tests/trace_ref.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import agent_cases as A
import trace_ref
from conftest import GOLDEN
from krca import native, tracecols
from krca.agents.traces import TracesAgent
from test_trace_cpu import ColumnsClient, boundary_values
from trace_ref import NumpyTraceEngine

pytestmark = pytest.mark.gpu
PERMILLE = tracecols.PERMILLE


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


@pytest.fixture(scope="module")
def lds_max(eng):
    return int(eng.lib.krca_trace_lds_max_slots())


# ---- link ------------------------------------------------------------------------------------
def _link_case(N, S=7, seed=0):
    rng = np.random.default_rng(seed + N)
    svc = rng.integers(0, S, N).astype(np.int32)
    parent = rng.integers(0, max(N, 1), N).astype(np.int32)  # forward and backward indices, chains deeper than 1
    kind = rng.random(N)
    parent[kind < 0.2] = -1
    self_ref = np.flatnonzero((kind >= 0.2) & (kind < 0.25))
    parent[self_ref] = self_ref
    parent[(kind >= 0.25) & (kind < 0.3)] = N + rng.integers(0, 5)      # out of range above
    parent[(kind >= 0.3) & (kind < 0.35)] = -2 - rng.integers(0, 1000)  # and below
    parent[(kind >= 0.35) & (kind < 0.37)] = 2 ** 31 - 1
    bad = rng.random(N) < 0.05  # bad-service spans, also used as parents by the random draw above
    svc[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1 - rng.integers(0, 9), S + rng.integers(0, 9))
    dur = rng.integers(0, 2 ** 20, N).astype(np.uint32)
    dur[rng.random(N) < 0.02] = 2 ** 32 - 1
    err = (rng.random(N) < 0.3).astype(np.uint8)
    if N >= 6000:  # one parent with 5 000 children whose durations sum past 2^32 (and past the parent's own)
        kids = rng.choice(np.arange(1, N), 5000, replace=False)
        parent[kids] = 0
        parent[0], svc[0], dur[0] = -1, 0, 2 ** 32 - 1
        svc[kids[:4000]] = rng.integers(0, S, 4000)
        dur[kids] = 2 ** 31
        # and one whose children stay below it (no clamp)
        few = np.setdiff1d(np.arange(2, N), kids)[:3]
        parent[parent == 1] = -1
        parent[few], parent[1], svc[1], dur[1] = 1, -1, 1, 10_000
        svc[few], dur[few] = [0, 2, 1], [1000, 2000, 3000]
    return svc, parent, dur, err, S


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 70_000])
def test_link(eng, N):
    svc, parent, dur, err, S = _link_case(N)
    got = eng.trace_link(svc, parent, dur, err, S)
    ref = trace_ref.link(svc, parent, dur, err, S)
    for g, r, what in zip(got, ref, ("caller_svc", "self_us", "flags", "n_bad")):
        assert np.array_equal(g, r), what
    if N >= 6000:
        assert ref[1][0] == 0 and ref[1][1] == 10_000 - 6000  # the clamp at 0, and a plain difference
        assert {0, 1, 3, 5, 7} == set(np.unique(ref[2]).tolist())  # every reachable flag combination


# ---- edges -----------------------------------------------------------------------------------
def _edge_case(N, S, seed=0, n_pairs=None):
    rng = np.random.default_rng(seed + S)
    svc = rng.integers(0, S, N).astype(np.int32)
    if n_pairs:  # draw from a limited set of pairs so that keys repeat
        pc, ps = rng.integers(0, S, n_pairs), rng.integers(0, S, n_pairs)
        pick = rng.integers(0, n_pairs, N)
        caller, svc = pc[pick].astype(np.int32), ps[pick].astype(np.int32)
    else:
        caller = rng.integers(0, S, N).astype(np.int32)
    caller[rng.random(N) < 0.3] = -1
    caller[rng.random(N) < 0.02] = S + 3      # off-contract callers are no edges
    svc[rng.random(N) < 0.02] = -4
    return caller, svc


@pytest.mark.parametrize("N,S,n_pairs", [(5000, 1, None), (5000, 2, None), (60_000, 300, 7000), (70_000, 50_000, 20_000),
                                         (65, 300, None)])
def test_edges(eng, N, S, n_pairs):
    caller, svc = _edge_case(N, S, n_pairs=n_pairs)
    rkey, rslot = trace_ref.edges(caller, svc, S)
    key, slot, E = eng.trace_edges(caller, svc, S)
    assert E == len(rkey) and np.array_equal(key, rkey) and np.array_equal(slot, rslot)
    assert (np.diff(key) > 0).all()
    # cap exactly E works; cap = E - 1 reports more than cap and does not fault
    key, slot, E2 = eng.trace_edges(caller, svc, S, cap=E)
    assert E2 == E and np.array_equal(key, rkey) and np.array_equal(slot, rslot)
    if E >= 1:
        key, slot, E3 = eng.trace_edges(caller, svc, S, cap=E - 1)
        assert key is None and E3 > E - 1


def test_edges_none_and_all_pairs(eng):
    svc = np.arange(100, dtype=np.int32) % 9
    key, slot, E = eng.trace_edges(np.full(100, -1, np.int32), svc, 9)  # zero edges
    assert E == 0 and len(key) == 0 and (slot == -1).all()
    key, slot, E = eng.trace_edges(np.zeros(0, np.int32), np.zeros(0, np.int32), 9)
    assert E == 0 and len(slot) == 0
    S = 40  # every pair present (self pairs included: the kernel takes caller_svc as given), three times over
    pairs = np.tile(np.arange(S * S), 3)
    np.random.default_rng(1).shuffle(pairs)
    caller, callee = (pairs // S).astype(np.int32), (pairs % S).astype(np.int32)
    key, slot, E = eng.trace_edges(caller, callee, S)
    assert E == S * S and np.array_equal(key, np.arange(S * S)) and np.array_equal(slot, pairs)


# ---- stats / quantiles -----------------------------------------------------------------------
def _stats_case(N, S, seed=0, hot=False):
    rng = np.random.default_rng(seed + 7 * N + S)
    slot = rng.integers(-1, S + 2, N).astype(np.int32)  # includes ignored -1 and >= S
    if hot:  # 5 % of the slots receive 90 % of the records
        h = rng.random(N) < 0.9
        slot[h] = rng.integers(0, max(S // 20, 1), int(h.sum()))
    val = (2.0 ** rng.uniform(0, 32, N)).astype(np.uint64)
    bv = boundary_values()
    k = min(len(bv), N)
    val[rng.choice(N, k, replace=False)] = bv[:k] if k < len(bv) else bv
    val = np.minimum(val, 2 ** 32 - 1).astype(np.uint32)
    flags = rng.choice(np.array([0, 0, 0, 1, 3, 5, 7], np.uint8), N)
    return slot, val, flags


def _check_stats(eng, slot, val, flags, S, impls):
    rrec, rhist = trace_ref.stats(slot, val, flags, S)
    rq = trace_ref.quantiles(rrec, rhist, PERMILLE)
    for impl in impls:
        with native.tune(KRCA_TRACE_IMPL=impl):
            rec, hist, q = eng.trace_stats(slot, val, flags, S, PERMILLE)
        assert np.array_equal(rec, rrec), ("rec", impl)
        assert np.array_equal(hist, rhist), ("hist", impl)
        assert np.array_equal(q, rq), ("quantiles", impl)
    # the quantile property against TRUE nearest-rank values: lo(b*) <= true <= out
    true = trace_ref.true_quantiles(slot, val, S, PERMILLE)
    b = trace_ref.quantile_bucket(rrec, rhist, PERMILLE)
    lo = np.where(b >= 0, trace_ref.LO[np.maximum(b, 0)], 0)
    assert (lo <= true).all() and (true <= rq).all()
    # two halves with accumulate = 1 equal the whole
    h = len(slot) // 2
    with native.tune(KRCA_TRACE_IMPL=impls[0]):
        first = eng.trace_stats(slot[:h], val[:h], flags[:h], S, PERMILLE)
        rec, hist, q = eng.trace_stats(slot[h:], val[h:], flags[h:], S, PERMILLE, accumulate=True, prev=first[:2])
    assert np.array_equal(rec, rrec) and np.array_equal(hist, rhist) and np.array_equal(q, rq)


@pytest.mark.parametrize("N", [1, 63, 65, 5000, 200_000])
@pytest.mark.parametrize("S_kind", ["1", "5", "lds_max", "lds_max+1", "3000"])
def test_stats_and_quantiles(eng, lds_max, N, S_kind):
    S = {"1": 1, "5": 5, "lds_max": lds_max, "lds_max+1": lds_max + 1, "3000": 3000}[S_kind]
    slot, val, flags = _stats_case(N, S)
    # 0 = by size; 1 = LDS tables (small S only); 2 = folded global atomics; 3 = one atomic set per lane
    impls = (0, 1, 2, 3) if S <= lds_max else (0, 2, 3)
    _check_stats(eng, slot, val, flags, S, impls)


# permille lists off (500, 900, 950, 990): one entry, the two ends, unsorted, and the limit of 16
# entries, descending with repeats
PERMILLE_LISTS = [(1,), (1000,), (1, 500, 1000), (999, 1000, 1, 2),
                  (1000, 1000, 999, 990, 950, 950, 900, 750, 500, 500, 250, 100, 10, 2, 1, 1)]
FORCED_COUNTS = (1, 999, 1000, 1001, 2000)  # the rank k = (q n + 999) / 1000 around n = 1000


def _forced_case(N, S, n_forced):
    """_stats_case with the records of slot S - 1 replaced by exactly n_forced records."""
    slot, val, flags = _stats_case(N, S)
    rng = np.random.default_rng(n_forced + S)
    slot[slot == S - 1] = -1
    slot = np.concatenate([slot, np.full(n_forced, S - 1, np.int32)])
    val = np.concatenate([val, (2.0 ** rng.uniform(0, 32, n_forced)).astype(np.uint64).clip(0, 2 ** 32 - 1).astype(np.uint32)])
    flags = np.concatenate([flags, np.zeros(n_forced, np.uint8)])
    order = rng.permutation(len(slot))
    return slot[order], val[order], flags[order]


@pytest.mark.parametrize("N", [1, 65, 5000])
@pytest.mark.parametrize("S_kind", ["1", "lds_max", "lds_max+1", "300"])
def test_quantiles_permille_lists(eng, lds_max, N, S_kind):
    S = {"1": 1, "lds_max": lds_max, "lds_max+1": lds_max + 1, "300": 300}[S_kind]
    assert len(PERMILLE_LISTS[-1]) == 16
    for n_forced in FORCED_COUNTS:
        slot, val, flags = _forced_case(N, S, n_forced)
        rrec, rhist = trace_ref.stats(slot, val, flags, S)
        assert rrec[S - 1, 0] == n_forced
        rec, hist = eng.trace_stats_device(eng._dev_n(slot, np.int32), eng._dev_n(val, np.uint32),
                                           eng._dev_n(flags, np.uint8), len(slot), S)
        assert np.array_equal(rec[:S].cpu().numpy(), rrec) and np.array_equal(hist[:S].cpu().numpy().view(np.uint32), rhist)
        for permille in PERMILLE_LISTS:
            q = eng.trace_quantiles_device(rec, hist, S, permille)[:S].cpu().numpy().view(np.uint32)
            rq = trace_ref.quantiles(rrec, rhist, permille)
            assert q.shape == rq.shape and np.array_equal(q, rq), (n_forced, permille)
            true = trace_ref.true_quantiles(slot, val, S, permille)
            b = trace_ref.quantile_bucket(rrec, rhist, permille)
            lo = np.where(b >= 0, trace_ref.LO[np.maximum(b, 0)], 0)
            assert (lo <= true).all() and (true <= rq).all(), (n_forced, permille)
            if permille == (1, 500, 1000):  # the smallest value's bucket, and exactly the largest value
                v = np.sort(val[slot == S - 1].astype(np.int64))
                assert rq[S - 1, 2] == v[-1] and trace_ref.bucket(v[0]) == b[S - 1, 0]
                assert true[S - 1, 1] == v[(500 * n_forced + 999) // 1000 - 1]


def test_quantiles_refusals(eng):
    """permille outside [1, 1000] and Q outside [1, 16]: KRCA_EINVAL naming the argument, nothing written."""
    slot, val, flags = _stats_case(100, 5)
    rec, hist = eng.trace_stats_device(eng._dev_n(slot, np.int32), eng._dev_n(val, np.uint32),
                                       eng._dev_n(flags, np.uint8), 100, 5)
    out = torch.full((5 * 17,), 0x5B5B5B5B, dtype=torch.int32, device="cuda")

    def call(permille):
        q = (ctypes.c_int32 * max(len(permille), 1))(*permille)
        return eng.lib.krca_trace_quantiles(eng.ptr(rec), eng.ptr(hist), 5, q, len(permille), eng.ptr(out), eng._stream())

    for permille, word in (((0,), b"permille[0]=0"), ((500, 1001), b"permille[1]=1001"), ((500, -1, 2), b"permille[1]=-1"),
                           ((), b"Q=0"), ((500,) * 17, b"Q=17")):
        assert call(permille) == -22 and word in eng.lib.krca_last_error(), (permille, eng.lib.krca_last_error())
    with pytest.raises(native.KrcaError):
        eng.trace_quantiles_device(rec, hist, 5, (1001,))
    torch.cuda.synchronize()
    assert bool((out == 0x5B5B5B5B).all().item())  # no refused call launched anything
    assert call((500,) * 16) == 0  # the limit itself is accepted
    torch.cuda.synchronize()
    want = trace_ref.quantiles(*trace_ref.stats(slot, val, flags, 5), (500,) * 16)
    assert np.array_equal(out[:80].cpu().numpy().view(np.uint32).reshape(5, 16), want)
    assert bool((out[80:] == 0x5B5B5B5B).all().item())


def test_stats_hot_slots_50k(eng):
    slot, val, flags = _stats_case(200_000, 50_000, hot=True)
    _check_stats(eng, slot, val, flags, 50_000, (0, 3))
    # a single slot and bucket for every lane: the fold's deepest case
    n = 5000
    _check_stats(eng, np.full(n, 123, np.int32), np.full(n, 77_777, np.uint32), np.ones(n, np.uint8), 300, (2, 3))


def test_stats_forced_lds_above_its_limit_is_an_error(eng, lds_max):
    slot, val, flags = _stats_case(100, lds_max + 1)
    with native.tune(KRCA_TRACE_IMPL=1):
        with pytest.raises(native.KrcaError):
            eng.trace_stats(slot, val, flags, lds_max + 1, PERMILLE)


# ---- end to end ------------------------------------------------------------------------------
def test_agent_device_equals_numpy_and_finds_the_planted_services(eng):
    cols, planted = tracecols.make_spans(13_000, 200, seed=11)
    assert 150_000 <= len(cols) <= 300_000
    ref = NumpyTraceEngine().trace_analyze(cols)
    slow, origin = planted["slow"], planted["origin"]
    # the restatement alone finds what was planted ...
    assert int(np.argmax(ref.self_q[:, tracecols.Q95])) == slow
    callers = ref.edge_src[ref.edge_dst == slow]
    assert ref.svc_q[callers, tracecols.Q95].max() > ref.svc_q[slow, tracecols.Q95]
    assert int(np.argmax(ref.svc_q[:, tracecols.Q95])) != slow
    assert int(np.argmax(ref.svc_rec[:, tracecols.R_ORIGIN])) == origin
    # ... and the device computes the same numbers and the same report
    got = eng.trace_analyze(cols)
    assert np.array_equal(got.edge_key, ref.edge_key) and got.n_bad == ref.n_bad == 0
    for name in ("svc", "self", "edge", "op"):
        assert np.array_equal(getattr(got, name + "_rec"), getattr(ref, name + "_rec")), name
        assert np.array_equal(getattr(got, name + "_q"), getattr(ref, name + "_q")), name
    dev = TracesAgent(ColumnsClient(cols=cols), engine=eng).analyze("mesh")
    host = TracesAgent(ColumnsClient(cols=cols), engine=NumpyTraceEngine()).analyze("mesh")
    assert "error" not in dev and A.strip(dev) == A.strip(host)
    assert len(dev["findings"]) > 3


def test_analyze_with_bad_spans(eng):
    cols, _ = tracecols.make_spans(300, 12, seed=3)
    cols.svc[::17] = 99  # bad spans: out of everything, operations included
    ref = NumpyTraceEngine().trace_analyze(cols)
    got = eng.trace_analyze(cols)
    assert got.n_bad == ref.n_bad > 0 and np.array_equal(got.edge_key, ref.edge_key)
    for name in ("svc", "self", "edge", "op"):
        assert np.array_equal(getattr(got, name + "_rec"), getattr(ref, name + "_rec")), name
        assert np.array_equal(getattr(got, name + "_q"), getattr(ref, name + "_q")), name


def test_pagerank_from_traces(eng):
    """Spans whose derived call graph is exactly the six edges of ppr_known.json, with 1 / 5 / 15 / 25
    / 2 erroring spans of 100 per service: PageRank over dependency_csr() seeded with
    error_rate_by_service() reproduces the file's vector and ranking."""
    with open(os.path.join(GOLDEN, "ppr_known.json")) as f:
        g = json.load(f)
    names = g["nodes"]
    pos = {n: i for i, n in enumerate(names)}
    n_err = {"frontend": 1, "backend": 5, "database": 15, "api-gateway": 25, "resource-service": 2}
    into = {n: [pos[a] for a, b in g["edges"] if b == n] for n in names}
    svc, parent, err = [], [], []
    anchor = {}  # one span per service for the others to hang from
    for n in names:
        anchor[n] = len(svc)
        svc.append(pos[n])
        parent.append(-1)
        err.append(0)
    for n in names:
        for k in range(99):
            callers = into[n]
            svc.append(pos[n])
            parent.append(anchor[names[callers[k % len(callers)]]] if callers else -1)
            err.append(0)
    svc, parent, err = np.array(svc, np.int32), np.array(parent, np.int32), np.array(err, np.uint8)
    for n, k in n_err.items():
        err[np.flatnonzero(svc == pos[n])[-k:]] = 1
    cols = tracecols.SpanColumns(svc, parent, np.array(svc), np.full(len(svc), 1000, np.uint32), err, names,
                                 [(i, "op") for i in range(len(names))])
    st = eng.trace_analyze(cols)
    deps = st.service_dependencies()
    assert sorted((a, b) for a, bs in deps.items() for b in bs) == sorted(map(tuple, g["edges"]))
    rates = st.error_rate_by_service()
    assert {n: round(r * 100) for n, r in rates.items()} == n_err and (st.svc_rec[:, tracecols.R_N] == 100).all()
    nm, rp, col, od = st.dependency_csr()
    seed = np.array([rates[n] for n in nm], np.float32)
    r, _, _ = eng.ppr(rp, col, od, seed, g["alpha"])
    r = r.cpu().numpy()
    want = np.array([g["pagerank"][n] for n in nm])
    assert np.allclose(r, want, rtol=1e-5, atol=0)
    assert [nm[i] for i in np.argsort(-r, kind="stable")] == g["ranking"]
