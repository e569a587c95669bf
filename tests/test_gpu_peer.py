"""Peer deviation score on the device (csrc/peer.hip): every output of krca_peer_score bit for bit against
tests/peer_ref.py (NaN where it is NaN) over the group sizes, shapes and data kinds of DESIGN.md §3.20;
work lists longer than the fixed grids; out-of-range ids; refusals; guard bands and poisons; the node
chain, the agents' keys and both recall fixtures equal to the CPU results."""
import itertools

import numpy as np
import pytest

import peer_ref as R
from guarded import GuardedEngine, run_poisons
from krca import native

pytestmark = pytest.mark.gpu

CAP = R.LDS_CAP
SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 255, 256, 257, 1000, CAP - 1, CAP, CAP + 1, 5000]
SHAPES = [(1, 1), (37, 2), (130, 8), (5, 64), (6000, 8)]
KINDS = ["noise", "ties", "signs", "nonfinite"]
# (data kind, min_scale)
DATA = [("noise", 0.0), ("ties", 0.0), ("ties", 0.5), ("signs", 0.0), ("nonfinite", 0.0), ("nonfinite", 0.5)]


@pytest.fixture(scope="module")
def eng():
    e = native.NativeEngine()
    assert e.lib.krca_peer_small_max() == R.SMALL_MAX and e.lib.krca_peer_lds_cap() == R.LDS_CAP
    return e


@pytest.fixture(scope="module")
def geng():
    return GuardedEngine()


def device_outputs(eng, v, gp, mem, mm, ms, thr):
    d = eng.peer_score(v, (gp, mem), min_members=mm, min_scale=ms, out_thr=thr)
    assert (d["min_members"], d["min_scale"], d["out_thr"]) == (mm, ms, thr)
    for k in R.KEYS:
        assert d[k].device.type == "cuda" and np.array_equal(d[k].cpu().numpy().view(np.uint8),
                                                            d[k + "_host"].view(np.uint8))
    return {k: d[k + "_host"] for k in R.KEYS}


def check(eng, v, gp, mem, mm=4, ms=0.0, thr=3.0, what=""):
    ref = R.peer_score(v, gp, mem, mm, ms, thr)
    R.same(ref, device_outputs(eng, v, gp, mem, mm, ms, thr), (what, v.shape, len(gp) - 1, mm, ms, thr))
    return ref


def pods_for(total):
    """A pod count that leaves 10 % of the pods in no group."""
    return max(1, -(-total * 10 // 9) + 1)


@pytest.mark.parametrize("n", SIZES)
def test_each_group_size_alone(eng, n):
    i = SIZES.index(n)
    P = pods_for(n)
    for j, (kind, ms) in enumerate(DATA):
        M = (8, 1, 2, 64, 4, 16)[(i + j) % 6] if n <= 1000 else (8, 2)[(i + j) % 2]
        gp, mem = R.layout([n], P, seed=i)
        ref = check(eng, R.data(kind, P, M, seed=10 * i + j), gp, mem, (1, 4, 21)[(i + j) % 3], ms, (0.0, 3.0)[j % 2])
        assert ref["peer"].shape == (P, M) and ref["grp_out"].shape == (1, M)


def test_all_group_sizes_in_one_call(eng):
    P = pods_for(sum(SIZES))
    gp, mem = R.layout(SIZES, P, seed=1)
    for j, (kind, ms) in enumerate(DATA):
        ref = check(eng, R.data(kind, P, 8, seed=j), gp, mem, (1, 4, 21)[j % 3], ms, (0.0, 3.0)[j % 2], "mixed")
    assert (ref["lead"][np.setdiff1d(np.arange(P), mem)] == -1).all()  # pods in no group: the defaults


MIXED = [0, 1, 2, 3, 4, 5, 20, 21, 22, 63, 64, 65, 300, CAP + 1]


@pytest.mark.parametrize("kind", KINDS)
def test_data_kinds_and_arguments(eng, kind):
    P = pods_for(sum(MIXED))
    gp, mem = R.layout(MIXED, P, seed=2)
    v = R.data(kind, P, 8, seed=3)
    for ms, mm, thr in itertools.product((0.0, 0.5), (1, 4, 21), (0.0, 3.0)):
        check(eng, v, gp, mem, mm, ms, thr, kind)


def split(total, pattern=(1, 2, 3, 5, 70, 4, 300, 64, 65, 9, 4200)):
    """Group sizes from the pattern, in turn, until `total` pods are used."""
    sizes, k = [], 0
    while total > 0:
        n = min(pattern[k % len(pattern)], total)
        sizes.append(n)
        total -= n
        k += 1
    return sizes


@pytest.mark.parametrize("P,M", SHAPES)
def test_shapes(eng, P, M):
    gp, mem = R.layout(split(P - P // 10), P, seed=P)
    for j, (kind, ms) in enumerate(DATA):
        check(eng, R.data(kind, P, M, seed=j), gp, mem, (1, 4)[j % 2], ms)


def test_all_metric_widths(eng):
    for M in (1, 2, 4, 8, 16, 32, 64):
        P = 700
        gp, mem = R.layout([5, 40, 64, 90, 400], P, seed=M)
        v = R.data("noise", P, M, seed=M)
        v[mem[::3], M - 1] += 500.0  # a third of the members far out in the last metric: lead = M - 1
        ref = check(eng, v, gp, mem, 4, 0.0, 3.0)
        assert (ref["lead"][mem[::3]] == M - 1).all()


def test_lists_longer_than_the_grids(eng):
    """3 000 groups of 5 (waves), 300 groups of 65 and 40 groups of cap + 1 at M = 8: 2 400 and 320
    (group, metric) items for the 1 024 and 256 workgroups of the two selection grids, so their drain
    loops iterate; the groups' order in the lists is whatever the appends made it."""
    sizes = [5] * 3000 + [65] * 300 + [CAP + 1] * 40
    rng = np.random.default_rng(4)
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    P = pods_for(sum(sizes))
    gp, mem = R.layout(sizes, P, seed=5)
    check(eng, R.data("noise", P, 8, seed=6), gp, mem, 4, 0.0, 3.0, "lists")


def test_out_of_range_ids_are_ignored(eng):
    sizes = [0, 3, 5, 61, 64, 65, 255, 300, CAP - 2, CAP + 1]
    P = pods_for(sum(sizes))
    gp, mem = R.layout(sizes, P, seed=7, sentinels=3)
    assert (mem == -1).any() and (mem == P).any()
    clean_gp, clean_mem = R.layout(sizes, P, seed=7)
    for j, (kind, ms) in enumerate(DATA):
        v = R.data(kind, P, 8, seed=j)
        ref = check(eng, v, gp, mem, 4, ms, 3.0, "sentinels")
        R.same(R.peer_score(v, clean_gp, clean_mem, 4, ms, 3.0), ref, "as if not listed")
    only = np.array([-1, P, -1, P + 7, -5], np.int32)  # groups of nothing but sentinels: n = 0
    check(eng, R.data("noise", P, 8), np.array([0, 2, 5], np.int64), only, 1, 0.0, 3.0, "n = 0")


def test_no_groups_and_no_pods(eng):
    v = R.data("noise", 300, 8)
    ref = check(eng, v, np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert not ref["peer"].any() and (ref["lead"] == -1).all() and ref["grp_med"].shape == (0, 8)
    d = eng.peer_score(np.zeros((0, 8), np.float32), (np.array([0, 0], np.int64), np.zeros(0, np.int32)))
    assert d["peer_host"].shape == (0, 8) and d["score_host"].shape == (0,)


def test_refusals_leave_the_outputs_untouched(eng):
    torch = eng.torch
    P, M, sizes = 400, 8, [5, 70, 200]
    gp, mem = R.layout(sizes, P, seed=8)
    G = len(sizes)
    v = R.data("noise", P, M)
    vd, gpd, memd = eng._dev(v), eng._dev(gp), eng._dev(mem)
    band = torch.full((6, P * M + 128), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    before = band.clone()
    outs = [band[i, 64:64 + P * M] for i in range(6)]  # peer, score, lead, grp_med, grp_mad, grp_out
    ws = eng._workspace("peer_score", eng.lib.krca_peer_ws_size(P, M, G, len(mem)))

    def call(P=P, M=M, G=G, n=len(mem), mm=4, ms=0.0, thr=3.0):
        return eng.lib.krca_peer_score(eng.ptr(vd), P, M, eng.ptr(gpd), eng.ptr(memd), G, n, mm, ms, thr,
                                       *(eng.ptr(o) for o in outs), eng.ptr(ws), eng._stream())
    for kw in (dict(M=3), dict(M=128), dict(M=0), dict(mm=0), dict(mm=-4), dict(ms=-1.0), dict(ms=float("inf")),
               dict(ms=float("nan")), dict(thr=-0.5), dict(thr=float("inf")), dict(thr=float("nan")), dict(P=-1),
               dict(G=-1), dict(n=-1), dict(P=1 << 29)):
        assert call(**kw) == -22, kw
        assert b"krca_peer_score" in eng.lib.krca_last_error()
        torch.cuda.synchronize()
        assert torch.equal(band, before), kw
    assert call(P=0) == 0  # a no-op
    torch.cuda.synchronize()
    assert torch.equal(band, before)
    assert call() == 0  # the same buffers, valid arguments: exactly the outputs' elements are written
    torch.cuda.synchronize()
    assert torch.equal(band[:, :64], before[:, :64]) and torch.equal(band[:, 64 + P * M:], before[:, 64 + P * M:])
    f32 = lambda t, *shape: t.cpu().numpy().view(np.float32)[:int(np.prod(shape))].reshape(shape)  # noqa: E731
    got = dict(peer=f32(outs[0], P, M), score=f32(outs[1], P), lead=outs[2].cpu().numpy().view(np.int8)[:P],
               grp_med=f32(outs[3], G, M), grp_mad=f32(outs[4], G, M),
               grp_out=outs[5].cpu().numpy()[:G * M].reshape(G, M))
    R.same(R.peer_score(v, gp, mem), got, "band")
    inner = slice(64, 64 + P * M)
    assert torch.equal(band[1, 64 + P:], before[1, 64 + P:])  # score: P floats
    assert torch.equal(band[2, inner].view(torch.int8)[P:], before[2, inner].view(torch.int8)[P:])  # lead: P bytes
    for i in (3, 4, 5):
        assert torch.equal(band[i, 64 + G * M:], before[i, 64 + G * M:])  # the group outputs: G * M words


def test_guard_bands_and_poisons(geng):
    sizes = [0, 1, 3, 5, 63, 64, 65, 257, 1000, CAP, CAP + 1]
    P = pods_for(sum(sizes))
    gp, mem = R.layout(sizes, P, seed=9, sentinels=2)
    v = R.data("nonfinite", P, 8, seed=9)
    out = run_poisons(geng, lambda e: {k: e.peer_score(v, (gp, mem), 4, 0.5, 3.0)[k + "_host"] for k in R.KEYS})
    R.same(R.peer_score(v, gp, mem, 4, 0.5, 3.0), out, "poisons")


# ---- the node chain, the agents and the recall fixtures: equal to the CPU results ---------------------
def same_chain(a, b):
    for k in ("effect", "deviation", "score", "lead", "pods", "out"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype == np.float32), k


def test_node_chain(eng):
    from krca.peers import PeerGroups, node_effects
    from test_peer_cpu import PeerOracleEngine
    P, M = 3000, 8
    v = R.data("noise", P, M, seed=11)
    rng = np.random.default_rng(12)
    service = (np.arange(P) // 20).astype(np.int32)
    service[rng.random(P) < 0.1] = -1       # pods in no service
    service[service == 7] = 3000            # ... and a service of 3: below min_members, left out of the node medians
    service[:3] = 7
    node = rng.integers(0, 70, P).astype(np.int32)
    node[rng.random(P) < 0.05] = -1
    cpu = PeerOracleEngine()
    got, want = {}, {}
    for e, out in ((eng, got), (cpu, want)):
        lab = np.where(service == 3000, -1, service)
        sg, ng = PeerGroups.from_labels(e, lab), PeerGroups.from_labels(e, node)
        peer = e.peer_score(v, sg, 4, 0.5, 3.0)
        out["peer"] = {k: peer[k + "_host"] for k in R.KEYS}
        out["chain"] = node_effects(e, peer["peer"], sg, ng)
        out["raw"] = node_effects(e, v, None, ng, min_members=2, min_scale=0.25, out_thr=2.0)
    R.same(want["peer"], got["peer"], "service call")
    same_chain(want["chain"], got["chain"])
    same_chain(want["raw"], got["raw"])
    assert got["chain"]["score"].shape == (70,) and got["chain"]["pods"].sum() < (node >= 0).sum()


def test_agents_end_to_end(eng):
    import agent_cases as A
    from krca.agents.coordinator import Coordinator
    from krca.agents.metrics import MetricsAgent
    from krca.mock import MeshClient
    from test_peer_cpu import NS, PeerOracleEngine, check_peer_keys, check_peer_root_causes, labels_of, mesh_case
    m, x, info = mesh_case()
    names, xd, groups = m.names(), eng._dev(x), labels_of(info)
    keys = ("peer_deviations", "service_wide", "node_deviations")
    for kw in (dict(), dict(peer_value="level", level_shift=True, peer_min_members=5, anomaly_topk=16)):
        agent = MetricsAgent(MeshClient(m, xd, groups=groups), engine=eng, peer_deviation=True, **kw)
        res = agent.analyze(NS)
        want = MetricsAgent(MeshClient(m, x, groups=groups), engine=PeerOracleEngine(), peer_deviation=True,
                            **kw).analyze(NS)
        assert "error" not in res and all(res[k] == want[k] for k in keys) and len(res["peer_deviations"]) >= 3
    plain = A.strip(Coordinator(MeshClient(m, xd, groups=groups), engine=eng).run_analysis("comprehensive", NS))
    res = A.strip(Coordinator(MeshClient(m, xd, groups=groups), engine=eng, peer_deviations=True)
                  .run_analysis("comprehensive", NS))
    assert "error" not in plain and "error" not in res and "peer_root_causes" not in plain
    rows, lifted = res.pop("peer_root_causes"), res.pop("node_deviations")
    got = {k: res["agent_results"]["metrics"].pop(k) for k in keys}
    assert res == plain and lifted == got["node_deviations"]
    ref, _ = check_peer_keys(got, names, x, info)
    check_peer_root_causes(rows, names, m, ref, x, engine=eng)
    short = MetricsAgent(MeshClient(m, xd[-100:].contiguous(), groups=groups), engine=eng, peer_deviation=True).analyze(NS)
    assert "error" not in short and all(short[k] == [] for k in keys)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_recall_fixtures(eng, seed):
    import shift_ref as S
    from krca.agents.metrics import MetricsAgent
    from krca.mock import MeshClient
    from test_peer_cpu import (NS, PeerOracleEngine, check_node_recall, check_replica_recall, labels_of, node_case,
                               replica_case)
    x, info = replica_case(seed)
    agent = MetricsAgent(MeshClient(None, eng._dev(x), names=[f"pod-{i}" for i in range(2000)], groups=labels_of(info)),
                         engine=eng, peer_deviation=True)
    res = agent.analyze(NS)
    assert "error" not in res
    shift, peer = agent.last_peer["shift"], agent.last_peer["service"]
    check_replica_recall(info, {"score": shift["score_host"]}, {"score": peer["score_host"]}, res["service_wide"])
    ref = S.shift_score(x, 120, 3, 0)
    R.same(R.peer_score(ref["shift"], *agent_groups(info), 4, agent.last_peer["min_scale"], agent.last_peer["threshold"]),
           {k: peer[k + "_host"] for k in R.KEYS}, "replica mesh")
    x, info = node_case(seed)
    shift = eng.shift_score(x, 120, 3, 0)
    chain, raw = check_node_recall(info, shift, eng)
    cpu_chain, cpu_raw = check_node_recall(info, S.shift_score(x, 120, 3, 0), PeerOracleEngine())
    same_chain(cpu_chain, chain)
    same_chain(cpu_raw, raw)


def agent_groups(info):
    from krca.peers import groups_from_labels
    return groups_from_labels(info["service"])
