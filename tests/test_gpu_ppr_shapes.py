"""The PageRank step on the plan shapes the synthetic meshes never reach (tests/ppr_shapes.py):
long rows (more than 2,048 callers: chunks, tickets, row accumulators) under a tolerance, in
multi-step settings, sharded, warm-started and replayed from a captured graph; short blocks that
meet the row and edge budgets exactly; dictionary blocks at the accept / reject edge.

Why these cases: packed on the CPU (tests/test_ppr_pack_cpu.py asserts it), the four
synth.make_graph meshes every other PageRank test uses -- (5000, 8), (20000, 20), (3000, 3),
(40000, 12, seed 5) -- hold long rows: 0, chunks: 0, tight dictionary blocks (dw + 4 * ceil(ne / 8)
== ne): 0.

References.  The fixed point and the iteration count are bit-identical to oracle.c_ppr / c_ppr_ex
(warm: r_start) / rca_keys.  The float result is compared with oracle.ppr_f64 (float64, fed the
2^-32-quantised seeds) at the bounds of test_ppr_bit_exact_vs_oracle: 1e-5 relative on ranks >=
1e-9, 1e-13 absolute below.  The C oracle alone against ppr_f64 on these builders (CPU; seeds
rand^8, all ones, one-hot on the first node, the last node and a hub's caller; alpha 0.85 and 0.5;
60 fixed iterations and tol 1e-9 capped at 300) deviates at worst 1.08e-6 relative (multi_self; the
float32 output 1.11e-6) and 2.35e-16 absolute below 1e-9 (rows_256x1): 9x and 400x inside the
bounds.  Every tolerance run converged (no negative count); a case whose oracle does not converge
would have to raise KrcaError on the device.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
import ppr_shapes as ps
from krca import native

pytestmark = pytest.mark.gpu

RUNS = ((60, 0.0), (300, 1e-9))


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


def _hub(rp):
    return int(np.argmax(np.diff(rp)))


@functools.lru_cache(maxsize=None)
def _seed(name, kind):
    rp, col, od = ps.case(name)
    N = len(od)
    if kind == "pow8":
        s = (np.random.default_rng(N).random(N) ** 8).astype(np.float32)
    else:  # one-hot on the first caller of the row with the most callers
        s = np.zeros(N, np.float32)
        s[int(col[rp[_hub(rp)]])] = 1.0
    return s  # shared between the tests: never written


@functools.lru_cache(maxsize=None)
def _ref(name, kind, alpha, iters, tol):
    """oracle.c_ppr's (r int64, iteration count) and the float64 restatement at that count."""
    rp, col, od = ps.case(name)
    seed = _seed(name, kind)
    _, r, it = oracle.c_ppr(rp, col, od, seed, alpha, iters, tol)
    qs = np.floor(seed.astype(np.float64) * 2.0 ** 32) / 2.0 ** 32
    x, _ = oracle.ppr_f64(rp, col, od, qs, alpha, abs(it), 0.0)
    for a in (r, x):
        a.setflags(write=False)
    return r, it, x


def _solve_equals_oracle(eng, name, kind, alpha, iters, tol, floats=False):
    rp, col, od = ps.case(name)
    ro, ito, x = _ref(name, kind, alpha, iters, tol)
    what = (name, kind, alpha, iters, tol)
    if ito < 0:  # no convergence in the oracle: the device call raises
        with pytest.raises(native.KrcaError):
            eng.ppr(rp, col, od, _seed(name, kind), alpha, iters, tol)
        return
    r, rf, it = eng.ppr(rp, col, od, _seed(name, kind), alpha, iters, tol)
    assert it == ito, what
    got = rf.cpu().numpy()
    assert np.array_equal(got, ro), (what, np.nonzero(got != ro)[0][:8])
    if floats:
        rr = r.cpu().numpy().astype(np.float64)
        big = x >= 1e-9
        rel = float(np.max(np.abs(rr[big] - x[big]) / x[big])) if big.any() else 0.0
        ab = float(np.max(np.abs(rr[~big] - x[~big]))) if (~big).any() else 0.0
        print(f"{what}: rel {rel:.3e} abs {ab:.3e}")
        assert rel < 1e-5 and ab < 1e-13, what


# ---- 1. every case through eng.ppr -------------------------------------------------------------
@pytest.mark.parametrize("name", list(ps.CASES))
def test_case_bit_identical_and_within_float64_bounds(eng, name):
    for alpha in (0.85, 0.5) if name in ps.HUB_CASES else (0.85,):
        for kind in ("pow8", "hub_caller"):
            for iters, tol in RUNS:
                _solve_equals_oracle(eng, name, kind, alpha, iters, tol, floats=True)


# ---- 2. knobs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ps.KNOB_CASES)
def test_knobs_bit_identical(eng, name):
    """Dictionary blocks on / off, non-temporal streaming on / off, grids of 1, 2 and 3 workgroups
    (one workgroup pipelines chunks and short blocks back to back; its clamped prefetch past the
    last entry lands on hub_last's final chunk) and 8 with the XCD entry map."""
    assert ps.PREDICATES[name](ps.pack(ps.bind(eng.lib), *ps.case(name)[:2]))
    for dict_on in (0, 1):
        for nt in (0, 1):
            for grid, xcd in ((1, 0), (2, 0), (3, 0), (8, 1)):
                with native.tune(eng.lib, KRCA_PPR_DICT=dict_on, KRCA_PPR_NT=nt, KRCA_PPR_GRID=grid, KRCA_PPR_XCD=xcd):
                    for iters, tol in RUNS:
                        _solve_equals_oracle(eng, name, "pow8", 0.85, iters, tol)


# ---- 3. RcaStep on one device --------------------------------------------------------------------
M, T, W = 4, 48, 30


def _metrics(P, seed, hot):
    """[T, P, M] float32: unit noise, and a 40-sigma step on the last sample of the pods `hot`."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, P, M)).astype(np.float32)
    x[-1, hot, :] += 40.0
    return torch.from_numpy(x)


def _hot(name, k, of=1):
    """Anomalous pods: the two rows with the most callers, callers of the first, a few others; part
    k of `of` disjoint parts (a pod then spikes in one window only: a second spike inside the
    rolling window would halve both z-scores)."""
    rp, col, od = ps.case(name)
    N = len(od)
    hubs = np.argsort(-np.diff(rp), kind="stable")[:2]
    rng = np.random.default_rng(k if of == 1 else 0)
    base = np.unique(np.concatenate([hubs, rng.choice(col[rp[hubs[0]]:rp[hubs[0] + 1]], 12 * of),
                                     rng.integers(0, N, 12 * of)]))
    return base[k % of::of]


def _cfg(tol):
    from krca.rca import Config
    return Config(window=W, alpha=0.85, iters=100 if tol > 0 else 20, tol=tol)


@pytest.mark.parametrize("tol", [0.0, 1e-9])
@pytest.mark.parametrize("name", ["two_hubs", "hub_last"])
def test_rca_step_long_rows_rerun_and_solo_step(eng, name, tol):
    """RcaStep (folded steps) and the unfolded krca_ppr_solo_step loop with KRCA_PPR_FUSE 0 / 1, each
    run twice on the same buffers: the second run meets the tickets and row accumulators the first
    one left, and both equal the oracle fed the device's scores."""
    from krca.rca import Comm, DeviceShard, RcaStep, step_flags
    rp, col, od = ps.case(name)
    n = len(od)
    cfg = _cfg(tol)
    floor = cfg.floor(n, M)
    x = _metrics(n, 1, _hot(name, 1)).cuda()
    sh = DeviceShard(eng, x, rp, col, od, n, n, 1, cfg)
    assert any(not e["short"] for e in ps.Packed(rp, col, n, sh.plan.cpu().numpy()[:sh.plan_len].reshape(-1, 4), None,
                                                  None, sh.n_dict).entries)
    step = RcaStep(sh, Comm(), cfg, 0)
    idx, key = step.run()
    score = sh.score_out["score"].cpu().numpy()[:n]
    assert int((score > floor).sum()) >= 5
    kref, o = oracle.rca_keys(rp, col, od, score, cfg.alpha, cfg.iters, floor, tol=tol)
    ridx = oracle.topk_ref(kref, cfg.k)[0]
    assert tol == 0 or o["it"] > 0
    for run in range(2):
        if run:
            idx, key = step.run()
        assert np.array_equal(sh.r[:n].cpu().numpy(), o["r"]), run
        assert np.array_equal(sh.key[:n].cpu().numpy(), kref), run
        assert [int(i) for i in idx] == ridx.tolist(), run
        assert tol == 0 or step.last_iters == o["it"], run
    # the unfolded loop: init, exchange, first reduction, then (solo step, exchange) per iteration;
    # under a tolerance the steps past convergence exit on the device-held flag
    comm = Comm()
    for fuse in (0, 1):
        with native.tune(eng.lib, KRCA_PPR_FUSE=fuse):
            s = DeviceShard(eng, x, rp, col, od, n, n, 1, cfg)
            assert s.fused
            for run in range(2):
                s.score()
                s.init(cfg.alpha, floor)
                comm.exchange(s)
                s.reduce(cfg.alpha, tol, 1)
                for it in range(1, cfg.iters + 1):
                    s.step(cfg.alpha, step_flags(tol, it == cfg.iters))
                    comm.exchange(s)
                    s.reduce(cfg.alpha, tol, 0)
                assert s.ctl_read() == ((o["it"], True) if tol > 0 else (cfg.iters, False)), (fuse, run)
                assert np.array_equal(s.r[:n].cpu().numpy(), o["r"]), (fuse, run)


@pytest.mark.parametrize("tol", [0.0, 1e-9])
@pytest.mark.parametrize("name", ["two_hubs", "hub_last"])
def test_rca_step_long_rows_graph_replay_equals_eager(eng, name, tol):
    from krca.rca import Comm, DeviceShard, RcaStep
    rp, col, od = ps.case(name)
    n = len(od)
    cfg = _cfg(tol)
    xs = [_metrics(n, s, _hot(name, s)).cuda() for s in (1, 2)]
    res = {}
    for graph in (False, True):
        x = xs[0].clone()
        step = RcaStep(DeviceShard(eng, x, rp, col, od, n, n, 1, cfg), Comm(), cfg, 0, graph=graph)
        assert step.graph == graph
        out = []
        for xi in xs + xs[:1]:
            x.copy_(xi)  # changed metrics under the captured buffers
            idx, key = step.run()
            out.append(([int(i) for i in idx], [int(v) for v in key], step.s.r[:n].cpu().numpy().copy(), step.last_iters))
        res[graph] = out
    for (ia, ka, ra, na), (ib, kb, rb, nb) in zip(res[False], res[True]):
        assert ia == ib and ka == kb and np.array_equal(ra, rb) and na == nb
    assert np.array_equal(res[True][0][2], res[True][2][2]) and not np.array_equal(res[True][0][2], res[True][1][2])


# ---- 4. emulated shards ----------------------------------------------------------------------------
def _exchange(shards):
    """The all-gather of G ranks on one device, done by copies."""
    wall = torch.cat([s.send for s in shards])
    for s in shards:
        s.w_all.copy_(wall)


def _host_pack(s):
    """The shard's packed plan as the device holds it."""
    rp, colv = s.host_csr
    return ps.Packed(np.asarray(rp, np.int64), np.asarray(colv, np.int64), s.n_max,
                     s.plan.cpu().numpy()[:s.plan_len].reshape(-1, 4), s.col.cpu().numpy(),
                     s.lane.cpu().numpy().view(np.uint16).reshape(-1, 2, ps.TPB), s.n_dict)


@pytest.mark.parametrize("mode", ["unfolded", "folded", "folded_tol"])
@pytest.mark.parametrize("G", [2, 3])
def test_sharded_hub_rows_emulated_on_one_gpu(eng, G, mode):
    """G ranks on one device (krca.rca.Partition ranges, the exchange done by copies) over a hub
    graph where a long row is a rank's first row, another a rank's last row, one rank holds only
    long rows (acc_long / ticket are indexed by the local row) and dictionary blocks name callers of
    several ranks' slices: ranks, iteration count and explained keys bit-identical to the
    single-process oracle."""
    from krca.rca import Config, DeviceShard, Explain, Partition, shard_graph
    rp_all, col_all, od_all, bounds = ps.shard_case(G)
    n = len(od_all)
    part = Partition(bounds)
    rng = np.random.default_rng(G)
    seed = (rng.random(n) * 2.0).astype(np.float32)
    cfg = Config(alpha=0.85, seed_floor=1.0)
    floor = cfg.floor(n)
    tol, iters = (1e-9, 200) if mode == "folded_tol" else (0.0, 15)
    shards = []
    for g in range(G):
        lo, hi, n_slot = part.range(g)
        rp, colv, od = shard_graph(rp_all, col_all, od_all, lo, hi, part)
        s = DeviceShard(eng, None, rp, colv, od, n, n_slot, G, cfg)
        s.score_out = {"score": torch.from_numpy(np.concatenate([seed[lo:hi], np.zeros(1, np.float32)])).cuda()}
        shards.append(s)
    # the arrangement, read from the plans the device holds
    packs = [_host_pack(s) for s in shards]
    weights = rng.integers(1, 1 << 40, G * part.n_slot)
    for p in packs:  # a rank's plan still means its rows (virtual column ids)
        sums, updates = p.replay(weights)
        assert np.all(updates == 1) and np.array_equal(sums, ps.expected_sums(p.row_ptr, p.col, weights))
    ents = [p.entries for p in packs]
    assert any(not e[0]["short"] and e[0]["rb"] == 0 and any(x["short"] for x in e) for e in ents)  # first row long
    assert any(not e[-1]["short"] and e[-1]["rb"] == p.N - 1 and any(x["short"] for x in e)
               for e, p in zip(ents, packs))                                                       # last row long
    assert any(all(not x["short"] for x in e) for e in ents)                                       # long rows only
    spans = [len(np.unique(ps.unmap(p.pk[x["e0"]:x["e0"] + x["nu"]], p.n_max) // p.n_max))
             for e, p in zip(ents, packs) for x in e if x["nu"] > 0]
    assert spans and max(spans) >= 2  # a dictionary block's distinct callers span two ranks' slices

    for s in shards:
        s.init(cfg.alpha, floor)
    _exchange(shards)
    if mode == "unfolded":
        for s in shards:
            s.reduce(cfg.alpha, tol, 1)
        for _ in range(iters):
            for s in shards:
                s.step(cfg.alpha)
            _exchange(shards)
            for s in shards:
                s.reduce(cfg.alpha, tol, 0)
        done = iters
    else:
        it = 0
        while it < iters:
            it += 1
            for s in shards:
                s.step_folded(cfg.alpha, tol, it, 3)
            _exchange(shards)
            states = {s.ctl_read() for s in shards}
            assert len(states) == 1, (it, states)
            if states.pop()[1]:
                break
        for s in shards:
            s.finish(cfg.alpha, tol, it)
        done = it
    key_ref, o = oracle.rca_keys(rp_all, col_all, od_all, seed, cfg.alpha, iters, floor, tol=tol)
    if tol > 0:
        assert o["it"] > 0 and {s.ctl_read() for s in shards} == {(o["it"], True)}
    else:
        assert done == iters and {s.ctl_read() for s in shards} == {(iters, False)}
    got = np.concatenate([s.r[:s.n].cpu().numpy() for s in shards])
    assert np.array_equal(got, o["r"]), np.nonzero(got != o["r"])[0][:8]
    ex, sall = Explain(rp_all, col_all), torch.from_numpy(seed).cuda()
    for g, s in enumerate(shards):
        lo = part.range(g)[0]
        s.local_topk_explained(cfg.k, sall, floor, ex, lo)
        assert np.array_equal(s.key[:s.n].cpu().numpy(), key_ref[lo:lo + s.n]), g


# ---- 5. warm start ----------------------------------------------------------------------------------
def test_streaming_warm_start_on_two_hubs(eng):
    """StreamingRCA over three windows: each re-rank starts from the previous ranks (and meets the
    previous solve's long-row tickets); ranks and iteration counts equal c_ppr_ex(r_start=previous)."""
    from krca.rca import Config
    from krca.stream import StreamingRCA
    rp, col, od = ps.case("two_hubs")
    P = len(od)
    rng = np.random.default_rng(8)
    Tn = W + 26
    x = rng.standard_normal((Tn, P, M)).astype(np.float32)
    windows = (W + 20, 5, 1)
    for k, last in enumerate(np.cumsum(windows) - 1):  # other pods spike at each window's last step
        x[last, _hot("two_hubs", k, 3), :] += 40.0
    cfg = Config(window=W)
    floor = cfg.floor(P, M)
    s = StreamingRCA(eng, rp, col, od, M, cfg, tol=1e-9, max_iter=60)
    xd = torch.from_numpy(x).cuda()
    r_ref, t = None, 0
    for d in windows:
        out = s.window(xd[t:t + d].contiguous())
        t += d
        score = out["scores"]["score"].cpu().numpy()[:P]
        assert int((score > floor).sum()) >= 5, t
        o = oracle.c_ppr_ex(rp, col, od, score, cfg.alpha, 60, 1e-9, floor, r_start=r_ref)
        r_ref = o["r"]
        assert np.array_equal(s.shard.r[:P].cpu().numpy(), r_ref), t
        assert out["iters"] == o["it"], (t, out["iters"], o["it"])
        ridx, _ = oracle.topk_ref(oracle.rca_keys_from(o, score, floor, rp, col), cfg.k)
        assert [int(i) for i in out["top"][0]] == [int(i) for i in ridx], t
    assert t == Tn
