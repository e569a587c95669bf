"""Guard bands and poisoned buffers around every device call of the C ABI (tests/guarded.py).

Each call runs three times, its outputs and workspaces filled with 0x00, 0xFF and 0x5B before it,
every buffer carved out of a canary-filled arena at exactly the size include/krca.h (or its size
function) gives.  Asserted per call and shape: (a) no byte outside the buffers changed, (b) the
inputs are unchanged, (c) the outputs are bit-identical across the three poisons over their logical
extent, (d) they equal the reference the call's own test uses.  A kernel that overruns its size
function, leaves an output slot unwritten or reads a workspace word before writing it fails one of
them whatever the allocator handed out before.  DESIGN.md "Buffer contracts" names, per buffer, the
write that makes the poison harmless; a buffer the header tells the caller to zero is zeroed here.

Out of scope: DeviceShard, StreamingRCA and corr_dist allocate zero-filled buffers of their own
with the module-level torch, so the shim does not reach them.
"""
import networkx as nx
import numpy as np
import pytest

import oracle
import timeline_cases as C
import timeline_ref as R
import trace_ref
from guarded import GuardedEngine, run_poisons, same_bytes
from krca import native, podstate, synth, tracecols
from krca.agents.logs import pack_documents
from krca.agents.topology import csr_from_edges
from test_gpu_groupby import _records
from test_gpu_kernels import _explain_graph, scan_two_calls
from test_gpu_topograph import _rand_sets
from test_gpu_trace import _edge_case, _link_case, _stats_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return GuardedEngine()


def host(t):
    return t.cpu().numpy().copy()


# ---- a1/a2 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 257])
def test_usage_flags(eng, P):
    rng = np.random.default_rng(P)
    u = rng.uniform(0, 100, (P, 2)).astype(np.float32)
    edge = np.array([80, 90, np.nextafter(np.float32(80), 100), np.nan, np.inf], np.float32)[:P]
    u[:len(edge), 0], u[:len(edge), 1] = edge, edge[::-1]
    out = run_poisons(eng, lambda e: {"flags": e.usage_flags(u)})
    assert np.array_equal(out["flags"], oracle.c_usage_flags(u))


# ---- a5 / a5t ---------------------------------------------------------------------------------
SIX = ("onset", "last", "count", "peak", "lead", "n_metrics")
FOUR = ("z_last", "score", "n_exceed", "flags")
# (P, M, T, W, KRCA_SCORE_IMPL, the scorer's kernel); the timeline has no ring form: it re-reads at T <= W
SCORE_CASES = [(37, 8, 121, 60, 0, "pipe"), (37, 8, 60, 60, 0, "ring"), (33, 1, 50, 7, 0, "reread"),
               (9, 64, 61, 10, 0, "pipe"), (37, 8, 61, 30, 4, "pipe_rows")]


@pytest.mark.parametrize("P,M,T,W,impl,variant", SCORE_CASES)
def test_rolling_score_and_timeline(eng, P, M, T, W, impl, variant):
    x = C.dyadic_metrics(P, M, T, W, seed=1000 * W + T + P)

    def call(e):
        xd = e._dev(x)
        tl = e.rolling_timeline_device(xd, W, 3.0, 3, 3)
        sc = e.rolling_score_device(xd, W, 3.0)
        out = {"tl_" + k: host(v) for k, v in tl.items()}
        out.update({"sc_" + k: host(v) for k, v in sc.items()})
        return out

    with native.tune(eng.lib, KRCA_SCORE_IMPL=impl):
        assert native.SCORE_VARIANTS[eng.lib.krca_rolling_score_variant(P, M, T, W)] == variant
        out = run_poisons(eng, call)
    ref = R.timeline(x, W, 3.0, 3, 3)
    for k in SIX + ("n_exceed",):
        assert same_bytes(out["tl_" + k], ref[k]), k
    for k in FOUR:
        assert same_bytes(out["tl_" + k], out["sc_" + k]), k
    c = oracle.c_rolling_score(x, W, 3.0)
    assert np.array_equal(out["sc_n_exceed"], c["n_exceed"]) and np.array_equal(out["sc_flags"], c["flags"])
    assert np.allclose(out["sc_z_last"], c["z_last"], rtol=1e-5, atol=1e-6)
    assert np.allclose(out["sc_score"], c["score"], rtol=1e-5, atol=1e-6)
    if T > W + 1:
        assert int(c["n_exceed"].sum()) > 0


# ---- streaming state --------------------------------------------------------------------------
STREAM_WINDOWS = [1, 8, 1, 1, 25, 70]  # end a window at t = W - 1 and at t = W, fill inside a call, delta > H


def _n_prefix(x, t, W):
    return oracle.c_rolling_score(x[:t], W)["n_exceed"] if t > W else np.zeros(x.shape[1], np.int32)


@pytest.mark.parametrize("P,M,W,H", [(37, 8, 10, 33), (33, 1, 7, 1)])
def test_stream_score_poisoned_state(eng, P, M, W, H):
    """The state is poisoned before the t0 = 0 call only (later calls carry it); after every window
    the canaries are checked and the state's defined part -- sums, counts, the ring rows written so
    far, the exceedance bits -- is compared across the poisons with the outputs."""
    T, S = sum(STREAM_WINDOWS), P * M
    x = C.dyadic_metrics(P, M, T, W, seed=7 * P + H)
    size = int(eng.lib.krca_stream_state_size(P, M, W, H))
    ring0, bits0 = 20 * S, 20 * S + 4 * W * S
    bits1 = bits0 + 4 * ((H + 31) // 32) * S
    assert size == bits1 + 64

    def call(e):
        t = e.torch
        state = e._workspace("stream_state", size)
        out, t0 = {}, 0
        for w, d in enumerate(STREAM_WINDOWS):
            xd = e._dev(np.ascontiguousarray(x[t0:t0 + d]))
            o = dict(z_last=t.empty((P, M), dtype=t.float32, device=e.device),
                     score=t.empty(P, dtype=t.float32, device=e.device),
                     n_exceed=t.empty(P, dtype=t.int32, device=e.device),
                     flags=t.empty(P, dtype=t.uint8, device=e.device))
            native._check(e.lib.krca_stream_score(e.ptr(xd), P, M, d, t0, W, H, 3.0, e.ptr(state), e.ptr(o["z_last"]),
                                                  e.ptr(o["score"]), e.ptr(o["n_exceed"]), e.ptr(o["flags"]),
                                                  e._stream()), "krca_stream_score")
            t0 += d
            t.cuda.synchronize()
            e._arena.check()
            st = host(state)
            for k, v in o.items():
                out[f"w{w}_{k}"] = host(v)
            out[f"w{w}_state_sums"] = st[:ring0]
            out[f"w{w}_state_ring"] = st[ring0:ring0 + 4 * S * min(t0, W)]
            out[f"w{w}_state_bits"] = st[bits0:bits1]
        assert t0 == T
        return out

    out = run_poisons(eng, call)
    t0 = 0
    for w, d in enumerate(STREAM_WINDOWS):
        t0 += d
        ref = oracle.c_rolling_score(x[:t0], W)
        assert np.array_equal(out[f"w{w}_flags"], ref["flags"]), t0
        assert np.allclose(out[f"w{w}_z_last"], ref["z_last"], rtol=1e-5, atol=1e-6), t0
        assert np.allclose(out[f"w{w}_score"], ref["score"], rtol=1e-5, atol=1e-6), t0
        want = _n_prefix(x, t0, W) - _n_prefix(x, t0 - H, W) if t0 - H > W else _n_prefix(x, t0, W)
        assert np.array_equal(out[f"w{w}_n_exceed"], want), t0
    assert int(oracle.c_rolling_score(x, W)["n_exceed"].sum()) > 0  # the fixture does exceed


# ---- top-k ------------------------------------------------------------------------------------
def _topk_ref(v, k):
    """Descending, ties to the lower index, NaN never selected; missing slots (-1, lowest)."""
    v = np.asarray(v)
    ok = np.flatnonzero(~np.isnan(v)) if v.dtype.kind == "f" else np.arange(len(v))
    order = ok[np.lexsort((ok, -v[ok].astype(np.float64) if v.dtype.kind == "f" else -v[ok]))][:k]
    idx = np.full(k, -1, np.int32)
    val = np.full(k, -np.inf if v.dtype.kind == "f" else np.iinfo(np.int64).min, v.dtype)
    idx[:len(order)], val[:len(order)] = order, v[order]
    return idx, val


@pytest.mark.parametrize("N,k", [(1, 1), (777, 5), (5000, 10), (5000, 16)])
def test_topk(eng, N, k):
    rng = np.random.default_rng(N + k)
    vf = rng.integers(0, 9, N).astype(np.float32)  # tie-heavy
    if N > 1:
        vf[rng.random(N) < 0.3] = np.nan
        vf[N // 2] = -np.inf
    vi = rng.integers(-3, 4, N).astype(np.int64) << 40
    if N >= 5000:
        assert int(eng.lib.krca_topk_workspace_size(N, k)) == 3 * k * 12 + 256  # three stage-1 blocks

    def call(e):
        fi, fv = e.topk(vf, k)
        ii, iv = e.topk(vi, k)
        return dict(f_idx=fi, f_val=fv, i_idx=ii, i_val=iv)

    out = run_poisons(eng, call)
    for name, v in (("f", vf), ("i", vi)):
        ridx, rval = _topk_ref(v, k)
        assert np.array_equal(out[name + "_idx"], ridx) and same_bytes(out[name + "_val"], rval), name
    # fewer than k non-NaN keys: the rest are the sentinel whatever the buffers held
    if N == 777:
        few = np.full(N, np.nan, np.float32)
        few[[3, 700]] = [1.0, 2.0]
        out = run_poisons(eng, lambda e: dict(zip(("idx", "val"), e.topk(few, k))))
        assert out["idx"].tolist() == [700, 3, -1, -1, -1] and np.isneginf(out["val"][2:]).all()


# ---- a10 PageRank -----------------------------------------------------------------------------
def _ppr_graph(case):
    rng = np.random.default_rng(3)
    if case == "mesh5000":
        m = synth.make_graph(5000, avg_degree=8, seed=5000)
        seed = (np.random.default_rng(5000).random(5000) ** 8).astype(np.float32)
        return m.row_ptr, m.col, m.outdeg, seed, ((100, 1e-6),)
    n = 1 if case == "single" else 50
    src, dst = [], []
    if case == "self_loops":
        src, dst = list(range(0, 50, 2)) + list(range(50)), list(range(0, 50, 2)) + list((np.arange(50) + 1) % 50)
    pairs = sorted(set(zip(src, dst)))
    rp, col, od = csr_from_edges(n, [a for a, _ in pairs], [b for _, b in pairs])
    return rp, col, od, (rng.random(n) ** 4).astype(np.float32), ((60, 0.0), (200, 1e-9))


@pytest.mark.parametrize("case", ["self_loops", "no_edges", "single", "mesh5000"])
def test_ppr(eng, case):
    rp, col, od, seed, runs = _ppr_graph(case)
    for iters, tol in runs:
        def call(e):
            r, rf, q, it = e._ppr_full(rp, col, od, seed, 0.85, iters, tol, 0.0)
            return dict(r=host(r), r_fixed=host(rf), q=host(q), iters=np.array([it]))

        out = run_poisons(eng, call)
        _, ro, ito, qo = oracle.c_ppr(rp, col, od, seed, 0.85, iters, tol, return_q=True)
        assert np.array_equal(out["r_fixed"], ro) and np.array_equal(out["q"], qo), (case, iters)
        assert int(out["iters"][0]) == abs(ito) and ito > 0, (case, iters)
        assert np.allclose(out["r"], ro / 2.0 ** 60, rtol=1e-6, atol=0)


# ---- explanation pass -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 3000])
def test_rca_explain(eng, n):
    rng = np.random.default_rng(n)
    rp, col, _ = _explain_graph(n, rng)
    ranges = ((0, n), (n // 3, n - n // 4))
    for frac, floor in ((0.02, 4.0), (0.5, 1.0)):
        score = np.where(rng.random(n) < frac, 4.0 + rng.integers(0, 6, n) * 0.5, rng.random(n) * 3.0).astype(np.float32)

        def call(e):
            sd, rpd, cold = e._dev(score), e._dev(rp), e._dev(col)
            return {f"d_{lo}_{hi}": host(e.rca_explain_device(sd, floor, rpd, cold, lo, hi)[:hi - lo]) for lo, hi in ranges}

        out = run_poisons(eng, call)
        for lo, hi in ranges:
            assert np.array_equal(out[f"d_{lo}_{hi}"], oracle.c_rca_explain(score, floor, rp, col, lo, hi)), (frac, lo, hi)
        if frac == 0.02 and n >= 3000:  # the rule fires on some pods, not on all
            assert 0 < int((out[f"d_0_{n}"] > 0).sum()) < n


# ---- onset precedence -------------------------------------------------------------------------
PREC = ("dep_earlier", "dep_concurrent", "caller_later", "caller_concurrent", "caller_earlier", "dep_first")


def _precede(eng, onset, peak, rp, col, slack, **guard_kw):
    def call(e):
        on, pk = e._dev(onset), e._dev(peak)
        rpd, cold = e._csr_dev(rp, col)
        prec = e.rca_precede_device(on, rpd, cold, slack)
        out = {k: host(v) for k, v in prec.items()}
        out["key"] = host(e.first_mover_key_device(on, pk, prec))
        return out

    out = run_poisons(eng, call, **guard_kw)
    ref = R.precede(onset, rp, col, slack)
    for name in PREC:
        assert same_bytes(out[name], ref[name]), (name, slack)
    assert same_bytes(out["key"], R.first_mover_key(onset, peak, ref))
    return ref


@pytest.mark.parametrize("slack", [0, 5])
def test_precede_hand_graph(eng, slack):
    rp, col = C.csr(C.EDGES, len(C.ONSET))
    ref = _precede(eng, C.ONSET, C.PEAK, rp, col, slack)
    for name in PREC:
        assert ref[name].tolist() == C.EXPECT[slack][name]


def test_precede_mesh(eng):
    """2000 pods, one row past 2048 callers (as test_gpu_timeline's mesh)."""
    m = synth.make_graph(2000, avg_degree=16, seed=3)
    rng = np.random.default_rng(3)
    deg = np.diff(m.row_ptr)
    big = int(np.argmax(deg))
    callee = np.concatenate([np.repeat(np.arange(2000), deg), np.full(2100, big)])
    caller = np.concatenate([m.col.astype(np.int64), rng.integers(0, 2000, 2100)])
    rp, col = C.csr(list(zip(caller.tolist(), callee.tolist())), 2000)
    onset = np.where(rng.random(2000) < 1 / 3, rng.integers(100, 140, 2000), -1).astype(np.int32)
    onset[big] = 120
    peak = np.where(onset >= 0, rng.integers(48, 200, 2000) / 16.0, 0).astype(np.float32)
    ref = _precede(eng, onset, peak, rp, col, 5)
    assert np.diff(rp).max() > 2048 and (ref["dep_earlier"] > 0).sum() > 50


def test_precede_grid_stride_loops(eng):
    """N = 600 000 > 2048 x 256 pods (precede_list strides) and about 10 000 pods with an onset >
    1024 x 4 waves (precede_rows strides); half the callers of a pod with an onset have one too."""
    N, E, n_on = 600_000, 2_400_000, 10_000
    rng = np.random.default_rng(6)
    with_onset = np.sort(rng.choice(N, n_on, replace=False))
    with_onset[-1] = N - 1  # the last pod of the last stride is listed
    callee = np.sort(rng.integers(0, N, E))
    rp = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(callee, minlength=N), out=rp[1:])
    col = rng.integers(0, N, E).astype(np.int32)
    listed_edge = np.isin(callee, with_onset) & (rng.random(E) < 0.5)
    col[listed_edge] = with_onset[rng.integers(0, n_on, int(listed_edge.sum()))]
    onset = np.full(N, -1, np.int32)
    onset[with_onset] = rng.integers(100, 140, n_on)
    peak = np.where(onset >= 0, rng.integers(48, 200, N) / 16.0, 0).astype(np.float32)
    ref = _precede(eng, onset, peak, rp, col, 3, capacity=96 << 20)
    assert (ref["dep_earlier"] > 0).sum() > 1000 and (ref["caller_concurrent"] > 0).sum() > 1000


# ---- f3 betweenness ---------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [7, 1024])
def test_betweenness(eng, batch):
    """batch = 7: several batches, scratch and dep rows reused; 1024: batch > N."""
    g = nx.gnp_random_graph(30, 0.1, seed=1, directed=True)
    nodes = list(g.nodes)
    pos = {n: i for i, n in enumerate(nodes)}
    rp, col = [0], []
    for n in nodes:
        col.extend(pos[m] for m in g.successors(n))
        rp.append(len(col))
    out = run_poisons(eng, lambda e: {"bc": e.betweenness(rp, col, batch=batch)})
    ref = nx.betweenness_centrality(g)
    want = np.array([ref[n] for n in nodes])
    assert np.allclose(out["bc"], want, rtol=1e-12, atol=1e-15) and want.max() > 0


# ---- f2 service graph -------------------------------------------------------------------------
def test_selector_match(eng):
    rng = np.random.default_rng(3)
    lab, lab_off = _rand_sets(rng, 300, 0, 6, 40)
    sel, sel_off = _rand_sets(rng, 65, 0, 3, 40)  # two mask words
    out = run_poisons(eng, lambda e: {"bits": e.selector_match(lab, lab_off, sel, sel_off)})
    assert out["bits"].shape == (300, 2)
    assert np.array_equal(out["bits"], oracle.selector_match_ref(lab, lab_off, sel, sel_off))


def test_substr_match_cap_grown_once(eng):
    """300 values x 40 keys with more than 4096 occurrences: the first output buffer (4096 slots,
    canary right behind) overflows, the call is repeated once with the reported count."""
    names = ["svc%d" % i for i in range(36)] + ["a", "ü-db", "db", ""]
    rng = np.random.default_rng(11)
    values = []
    for v in range(300):
        pick = rng.choice(36, int(rng.integers(10, 36)), replace=False)
        values.append(("ünï " if v % 7 == 0 else "") + ",".join(names[i] + ".shop" for i in pick) +
                      (" a-db ü-db" if v % 5 == 0 else ""))
    vb, kb = [v.encode() for v in values], [k.encode() for k in names]
    text, pat = b"".join(vb), b"".join(kb)
    val_off = np.concatenate([[0], np.cumsum([len(b) for b in vb])]).astype(np.int64)
    pat_off = np.concatenate([[0], np.cumsum([len(b) for b in kb])]).astype(np.int64)
    allocs = []

    def call(e):
        pairs = e.substr_match(text, val_off, pat, pat_off)
        allocs.append(sum(1 for p in e._arena.payloads if p.label.startswith("empty int64") and p.nbytes >= 8 * 4096))
        return {"pairs": pairs}

    out = run_poisons(eng, call)
    ref = oracle.substr_match_ref(text, val_off, pat, pat_off)
    assert np.array_equal(out["pairs"], ref) and len(ref) > 4096 + 300
    assert allocs == [2, 2, 2]  # the 4096-slot buffer, then one of the reported size


# ---- f1 / f4 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [255, 300])
def test_pod_classify(eng, P):
    pc, off, cc = podstate.make_pod_states(P, seed=P)
    out = run_poisons(eng, lambda e: dict(zip(("mask", "hist"), e.pod_classify(pc, off, cc))))
    ref_mask, ref_hist = oracle.pod_classify_ref(pc, off, cc)
    assert np.array_equal(out["mask"], ref_mask) and np.array_equal(out["hist"], ref_hist)


@pytest.mark.parametrize("N,S,R,hot,ranked", [(63, 5, 3, 0, 1), (5000, 40, 3, 0.5, 1), (5000, 3000, 3, 0.1, 0.5)])
def test_group_reduce(eng, N, S, R, hot, ranked):
    slot, key = _records(np.random.default_rng(N + S + R), N, S, hot)
    n_ranked = int(N * ranked)
    names = ("first", "count", "n_key", "top")
    out = run_poisons(eng, lambda e: dict(zip(names, e.group_reduce(slot, key, S, R, n_ranked=n_ranked))))
    for name, r in zip(names, oracle.group_reduce_ref(slot, key, S, R, n_ranked)):
        assert np.array_equal(out[name], r), name


# ---- t1 trace analytics -----------------------------------------------------------------------
@pytest.mark.parametrize("N", [65, 257])
def test_trace_link(eng, N):
    svc, parent, dur, err, S = _link_case(N)
    names = ("caller_svc", "self_us", "flags", "n_bad")
    out = run_poisons(eng, lambda e: {k: np.asarray(v) for k, v in zip(names, e.trace_link(svc, parent, dur, err, S))})
    for name, r in zip(names, trace_ref.link(svc, parent, dur, err, S)):
        assert np.array_equal(out[name], r), name
    assert N < 257 or int(out["n_bad"]) > 0


@pytest.mark.parametrize("N,S", [(5000, 2), (65, 300)])
def test_trace_edges(eng, N, S):
    """The growing form, then cap = E exactly: edge_key is a payload of E slots, the canary starts
    right behind key[E - 1]; edge_slot is written whole (-1 for the spans that are no edge)."""
    caller, svc = _edge_case(N, S)
    rkey, rslot = trace_ref.edges(caller, svc, S)
    E = len(rkey)
    assert E >= 1

    def call(e):
        k0, s0, e0 = e.trace_edges(caller, svc, S)
        k1, s1, e1 = e.trace_edges(caller, svc, S, cap=E)
        assert sum(1 for p in e._arena.payloads if p.label == f"empty int64[{E}]") == 1
        return dict(key=k0, slot=s0, E=np.array([e0]), key_cap=k1, slot_cap=s1, E_cap=np.array([e1]))

    out = run_poisons(eng, call)
    for sfx in ("", "_cap"):
        assert int(out["E" + sfx][0]) == E
        assert np.array_equal(out["key" + sfx], rkey) and np.array_equal(out["slot" + sfx], rslot)


@pytest.mark.parametrize("S_kind", ["lds_max", "lds_max+1"])
def test_trace_stats_and_quantiles(eng, S_kind):
    lds_max = int(eng.lib.krca_trace_lds_max_slots())
    S = lds_max + (S_kind == "lds_max+1")
    N, nb, permille = 5000, int(eng.lib.krca_trace_nbuckets()), tracecols.PERMILLE
    slot, val, flags = _stats_case(N, S)
    rrec, rhist = trace_ref.stats(slot, val, flags, S)
    rq = trace_ref.quantiles(rrec, rhist, permille)
    for impl in ((0, 1, 2, 3) if S <= lds_max else (0, 2, 3)):
        def call(e):
            t = e.torch
            rec, hist, q = e.trace_stats(slot, val, flags, S, permille)
            # the accumulate form adds into what is there: rec / hist zeroed by the caller (here)
            sd, vd, fd = e._dev_n(slot, np.int32), e._dev_n(val, np.uint32), e._dev_n(flags, np.uint8)
            rec0 = t.zeros((S, 8), dtype=t.int64, device=e.device)
            hist0 = t.zeros((S, nb), dtype=t.int32, device=e.device)
            e.trace_stats_device(sd, vd, fd, N, S, True, rec0, hist0)
            qa = e.trace_quantiles_device(rec0, hist0, S, permille)
            return dict(rec=rec, hist=hist, q=q, rec_acc=host(rec0), hist_acc=host(hist0).view(np.uint32),
                        q_acc=host(qa).view(np.uint32))

        with native.tune(KRCA_TRACE_IMPL=impl):
            out = run_poisons(eng, call)
        for sfx in ("", "_acc"):
            assert np.array_equal(out["rec" + sfx], rrec), (impl, sfx)
            assert np.array_equal(out["hist" + sfx], rhist), (impl, sfx)
            assert np.array_equal(out["q" + sfx], rq), (impl, sfx)


# ---- a11/a12 log scan -------------------------------------------------------------------------
DEGENERATE = [[""], ["", "", ""], ["x" * 15 + "\n"], ["\n"], ["\r\n" * 7 + "\x85"], ["a" * 32767 + "\n"],
              ["Error " * 5461 + "ab"], ["b" * 65535 + "\n", ""], ["", "Killed", ""]]  # test_log_scan_degenerate_texts


def _fuzz_docs():
    """The corpus of test_log_scan_fragment_fuzz: pattern halves scattered over lines and containers."""
    import re as _re
    from krca.patterns import ERROR_PATTERNS
    lits = [a for _, p in ERROR_PATTERNS for a in p.strip("()").split("|")]
    lits = [_re.sub(r"\\d", "7", a).replace("\\", "") for a in lits]
    rng = np.random.default_rng(21)
    seps = ["\n", "\r", "\r\n", "\x0b", "\x0c", "\x1c", "\x1d", "\x1e", "\x85", "\u2028", "\u2029", ""]
    other = ["\u00e9", "\u0130", "\u212a", "\u017f", "x", " ", "0", "a" * 13, "q" * 40]
    docs = []
    for _ in range(1500):
        parts = []
        for _ in range(int(rng.integers(0, 12))):
            r = rng.random()
            if r < 0.45:
                a = lits[int(rng.integers(0, len(lits)))]
                cut = int(rng.integers(0, len(a) + 1))
                parts.append(a[:cut] if rng.random() < 0.5 else a[cut:])
            elif r < 0.6:
                parts.append(lits[int(rng.integers(0, len(lits)))])
            elif r < 0.8:
                parts.append(seps[int(rng.integers(0, len(seps)))])
            else:
                parts.append(other[int(rng.integers(0, len(other)))] * int(rng.integers(1, 4)))
        docs.append("".join(parts))
    return docs


@pytest.fixture(scope="module")
def log_cases():
    """(docs, blob, doc_off, oracle.log_hist per container), computed once for every walk."""
    return [(docs, *pack_documents(docs), [oracle.log_hist(t) for t in docs]) for docs in DEGENERATE + [_fuzz_docs()]]


LOG_KEYS = ("line_start", "line_end", "line_mask", "doc_lines", "doc_line0", "hist", "examples")


def _scan_one_call(e, blob, off, cap):
    """NativeEngine.log_scan_device with line arrays of `cap` lines: krca_log_scan, and krca_log_match
    over the index it left when the arrays were too small."""
    e._log_cap = cap
    r = e.log_scan_device(e.upload_blob(blob), e._dev(np.asarray(off, np.int64)), validate=False, dense_examples=True)
    return {k: host(r[k]) for k in LOG_KEYS}


def _check_scan(out, docs, blob, ref):
    assert out["doc_lines"].tolist() == [n for n, _, _ in ref]
    assert out["hist"].tolist() == [h for _, h, _ in ref]
    assert np.array_equal(out["doc_line0"], np.cumsum([0] + [n for n, _, _ in ref])[:-1])
    ls, le = out["line_start"], out["line_end"]
    assert len(ls) == sum(n for n, _, _ in ref)
    # the example lines: the dense table, and the same ids from the line masks' example bits
    assert np.array_equal(native.example_ids(out["line_mask"], out["doc_line0"], out["doc_lines"]), out["examples"])
    for d, (_, _, ex) in enumerate(ref):
        for c in range(native.NCAT):
            got = [blob[ls[i]:le[i]].decode("utf-8", "surrogatepass") for i in out["examples"][d, c] if i >= 0]
            assert got == ex[c], (d, c)


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_log_scan(eng, log_cases, fused):
    """krca_log_scan in one call (arrays larger than the line count: the logical extent is the lines),
    its fallback through krca_log_match after a scan into arrays of 1024 lines, and the two-call
    protocol krca_log_index + krca_log_match into arrays of exactly the line count."""
    n_fallback = 0
    with native.tune(eng.lib, KRCA_LOG_FUSED=fused):
        for docs, blob, off, ref in log_cases:
            L = sum(n for n, _, _ in ref)
            out = run_poisons(eng, lambda e: _scan_one_call(e, blob, off, 1 << 15))
            _check_scan(out, docs, blob, ref)
            walks = [out]
            if L > 1024:
                walks.append(run_poisons(eng, lambda e: _scan_one_call(e, blob, off, 0)))
                n_fallback += 1
            if fused == 0:  # the two-call protocol has no fused form
                walks.append(run_poisons(eng, lambda e: scan_two_calls(e, blob, off)))
            for w in walks[1:]:
                _check_scan(w, docs, blob, ref)
                for k in LOG_KEYS:
                    assert same_bytes(w[k], out[k]), k
    assert n_fallback == 1  # the fuzz corpus


# ---- a13 templates ----------------------------------------------------------------------------
def test_template_hash_and_hist(eng):
    """The corpus of test_template_hist_writes_every_slot: containers on the lane (<= 8 lines), wave
    (<= 64), workgroup (<= krca_template_max_lines()) and huge paths.  Every slot of tmpl_hash /
    tmpl_count over the lines is written (templates, then 0), so the whole arrays are compared."""
    docs = ["a 1\na 2\nb", "x\n" * 5 + "y", "\n".join("t %d" % (i % 3) for i in range(50)),
            "\n".join("u %s" % ("k" * (i % 7)) for i in range(3000)), "\n".join("v" for _ in range(5000)), "", "z"]
    assert max(len(d.splitlines()) for d in docs) > eng.lib.krca_template_max_lines()
    blob, off = pack_documents(docs)

    def call(e):
        scan = e.log_scan_device(e.upload_blob(blob), e._dev(np.asarray(off, np.int64)), validate=False)
        r = e.template_hist_device(scan)
        assert sum(1 for (key, _) in e._guard_ws if key == "tmpl_huge") == 1  # one container on the huge path
        out = {k: host(r[k]) for k in ("hash", "tmpl_hash", "tmpl_count", "n_templates")}
        out.update(doc_line0=host(scan["doc_line0"]), doc_lines=host(scan["doc_lines"]))
        return out

    out = run_poisons(eng, call)
    th, tc = out["tmpl_hash"].view(np.uint64), out["tmpl_count"]
    for d, text in enumerate(docs):
        lo, n, nl = int(out["doc_line0"][d]), int(out["n_templates"][d]), int(out["doc_lines"][d])
        assert list(zip(th[lo:lo + n].tolist(), tc[lo:lo + n].tolist())) == oracle.template_hist(text), d
        assert not th[lo + n:lo + nl].any() and not tc[lo + n:lo + nl].any(), d
        lines = text.splitlines()
        assert out["hash"].view(np.uint64)[lo:lo + nl].tolist() == \
            [oracle.fnv1a64(oracle.template_of(ln.encode("utf-8", "surrogatepass"))) for ln in lines], d


# ---- a9 correlation ---------------------------------------------------------------------------
@pytest.mark.parametrize("P,T,group,k", [(2, 30, 0, 1), (33, 5, 0, 7), (257, 64, 0, 5), (130, 200, 7, 16)])
def test_corr_prepare_and_topk(eng, P, T, group, k):
    """zh is allocated with its padding rows and steps and poisoned like everything else: the call
    writes all of it, the padding as zeros.  No candidate buffer overflows at these sizes, so the
    certificates are compared bit for bit too."""
    from test_gpu_corr import TAU, check_rows
    x = synth.make_metrics(P, 2, T, seed=P + T, group_size=group)
    x[:, 3 % P, 0] = 42.0  # a flat series
    if P > 20:
        x[:, 17, 0] = x[:, 5, 0]  # duplicate pods
        x[:, 18, 0] = x[:, 5, 0]
    Pp, Tp = int(eng.lib.krca_corr_pad_rows(P)), int(eng.lib.krca_corr_pad_steps(T))

    def call(e):
        z = e.corr_prepare_device(e._dev(x), 0)
        r = e.corr_topk_device(z, k, TAU)
        out = {key: host(z[key]) for key in ("mean", "scale", "z32", "zh")}
        out.update({key: host(v) for key, v in r.items()})
        return out

    out = run_poisons(eng, call)
    z32, mean, scale = oracle.c_corr_z32(x.numpy(), 0)
    assert same_bytes(out["z32"], z32.reshape(P, T)) and same_bytes(out["mean"], mean) and same_bytes(out["scale"], scale)
    zh = out["zh"].view(np.float16)
    assert zh.shape == (Pp, Tp) and (Pp > P or Tp > T)
    assert same_bytes(zh[:P, :T], z32.reshape(P, T).astype(np.float16))
    assert not out["zh"][P:].any() and not out["zh"][:, T:].any()
    check_rows(out, z32.reshape(P, T), np.arange(P), k)


# ---- the harness on the device ----------------------------------------------------------------
def test_harness_reports_on_the_device(eng):
    """The checks themselves, with device tensors: a byte written behind a payload (inside the arena:
    no memory outside it is touched) is reported, and a real kernel asked for one element fewer than
    its output holds leaves that element to the poison, which the comparison across poisons catches."""
    with eng.guard(0x5B) as arena:
        t = eng.torch.empty(100, dtype=eng.torch.uint8, device=eng.device)
        assert t.is_cuda and bool((t == 0x5B).all()) and t.data_ptr() % 256 == 0
        arena.buf[arena.payloads[-1].end] = 0
    with pytest.raises(AssertionError, match=r"0 byte\(s\) past the end of payload #0"):
        arena.check()
    u = np.random.default_rng(0).uniform(0, 100, (64, 2)).astype(np.float32)

    def short_call(e):
        ud = e._dev(u)
        flags = e.torch.empty(64, dtype=e.torch.uint8, device=e.device)
        native._check(e.lib.krca_usage_flags(e.ptr(ud), 63, e.ptr(flags), e._stream()), "krca_usage_flags")
        return {"flags": host(flags)}

    with pytest.raises(AssertionError, match="output 'flags' differs between poison 0x00 and 0xFF: element 63"):
        run_poisons(eng, short_call)
