"""Peer deviation score without a GPU: the NumPy restatement (tests/peer_ref.py) against a plain-Python
brute force on hand cases, the group helpers of krca/peers.py, the MetricsAgent / Coordinator options over an
engine that answers peer_score from the restatement, and the two recall fixtures of DESIGN.md §3.20."""
import functools
import math

import numpy as np
import pytest

import agent_cases as A
import peer_ref as R
import shift_ref as S
from krca import rca, synth
from krca.agents.coordinator import Coordinator
from krca.agents.metrics import NODE_THRESHOLD, PEER_DEFAULTS, MetricsAgent
from krca.mock import MeshClient
from krca.peers import PeerGroups, groups_from_labels, node_effects
from oracle_engine import OracleEngine
from test_shift_cpu import ShiftOracleEngine, bits, eq, f32, lmed, sub32

NS = A.NS


# ---- plain-Python brute force ------------------------------------------------------------------------
def brute(v, gp, mem, mm, ms, thr):
    P, M = v.shape
    G = len(gp) - 1
    peer = [[0.0] * M for _ in range(P)]
    med, mad, out = ([[0.0] * M for _ in range(G)], [[0.0] * M for _ in range(G)], [[0] * M for _ in range(G)])
    for g in range(G):
        ids = [int(i) for i in mem[gp[g]:gp[g + 1]] if 0 <= int(i) < P]
        for m in range(M if ids else 0):
            vals = [float(v[i, m]) for i in ids]
            md = lmed(vals)
            ma = lmed([abs(sub32(x, md)) for x in vals])
            med[g][m], mad[g][m] = md, ma
            if len(ids) < mm:
                continue
            den = 1.4826 * ma
            if not den > f32(ms):
                den = f32(ms)
            for i, x in zip(ids, vals):
                with np.errstate(all="ignore"):
                    pr = float(np.float32((np.float64(x) - np.float64(md)) / np.float64(den))) if den > 0 else 0.0
                peer[i][m] = pr
                out[g][m] += abs(pr) > f32(thr)
    score, lead = [], []
    for p in range(P):
        best, bm = 0.0, -1
        for m in range(M):
            a = abs(peer[p][m])
            if not math.isnan(a) and a > best:
                best, bm = a, m
        score.append(best)
        lead.append(bm)
    return peer, score, lead, med, mad, out


def check_against_brute(v, gp, mem, mm=4, ms=0.0, thr=3.0):
    v = np.asarray(v, np.float32)
    gp, mem = np.asarray(gp, np.int64), np.asarray(mem, np.int32)
    ref = R.peer_score(v, gp, mem, mm, ms, thr)
    peer, score, lead, med, mad, out = brute(v, gp, mem, mm, ms, thr)
    for name, want in (("peer", peer), ("grp_med", med), ("grp_mad", mad)):
        for i, row in enumerate(want):
            assert all(eq(w, float(g)) for w, g in zip(row, ref[name][i])), (name, i, row, ref[name][i])
    assert all(eq(w, float(g)) for w, g in zip(score, ref["score"])), (score, ref["score"])
    assert lead == ref["lead"].tolist() and out == ref["grp_out"].tolist()
    return ref


def one_group(*columns, mm=1, ms=0.0, thr=3.0):
    """Columns of equal length -> one group of all pods over v [n, M] (M padded with the first column)."""
    M = 1 << (len(columns) - 1).bit_length()
    cols = list(columns) + [columns[0]] * (M - len(columns))
    v = np.array(cols, np.float32).T.copy()
    n = v.shape[0]
    return check_against_brute(v, [0, n], np.arange(n), mm, ms, thr)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8])
def test_ties_even_and_odd_groups(n):
    col = [1.0, 3.0, 3.0, 2.0, 3.0, 1.0, 2.0, 7.0][:n]
    ref = one_group(col, [5.0] * n)
    assert float(ref["grp_med"][0, 0]) == sorted(col)[(n - 1) // 2]  # the lower median, no averaging
    assert not ref["peer"][:, 1].any()  # all equal: MAD 0, no floor, deviation 0


@pytest.mark.parametrize("min_scale,want", [(0.0, 0.0), (0.5, 4.0)])
def test_mad_zero(min_scale, want):
    ref = one_group([1.0, 1.0, 1.0, 1.0, 3.0, 0.0, 1.0], ms=min_scale)
    assert float(ref["grp_mad"][0, 0]) == 0.0 and float(ref["peer"][4, 0]) == want
    assert float(ref["score"][4]) == want and int(ref["lead"][4]) == (0 if want else -1)
    assert int(ref["grp_out"][0, 0]) == (1 if want else 0)


def test_signed_zeros():
    ref = one_group([0.0, -0.0, 0.0, -0.0], [-0.0, 0.0, 1.0, -1.0])
    assert bits(float(ref["grp_med"][0, 0])) == 0x80000000  # rank 1 of {-0, -0, +0, +0}
    assert bits(float(ref["grp_med"][0, 1])) == 0x80000000  # rank 1 of {-1, -0, +0, 1}
    assert not ref["peer"][:, 0].any() and ref["score"][0] == 0 and ref["lead"][0] == -1


def test_nan_and_inf_members():
    nan = float("nan")
    cols = ([1.0, nan, 2.0, 3.0, 2.5],                 # one NaN: sorts last, the medians stay finite
            [1.0, math.inf, 2.0, -math.inf, 2.5],
            [nan, nan, nan, 1.0, 2.0],                 # the median itself is NaN
            [math.inf, math.inf, math.inf, 1.0, 2.0])  # Inf - Inf
    ref = one_group(*cols)
    assert np.isfinite(ref["grp_med"][0, :2]).all() and np.isnan(ref["peer"][1, 0])
    assert np.isnan(ref["grp_mad"][0, 2:]).all() and not ref["peer"][:, 2:].any()  # a NaN MAD is no scale
    ref = one_group(*cols, ms=0.5, thr=0.0)
    assert np.isnan(ref["peer"][:, 2]).all() and ref["grp_out"][0, 2] == 0  # a NaN does not count
    assert not np.isnan(ref["score"]).any()  # NaN deviations are skipped (an Inf member's score is Inf)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("mm", [1, 4])
def test_small_groups_and_min_members(n, mm):
    """n in {0, 1, 2, 3, min_members - 1, min_members}: below min_members the medians are written, the
    deviations and the counts are not."""
    v = R.data("noise", 12, 4, seed=n)
    gp, mem = [0, n, n + 5], np.arange(n + 5)
    ref = check_against_brute(v, gp, mem, mm, 0.0, 0.0)
    if n == 0:
        assert not ref["grp_med"][0].any() and not ref["grp_mad"][0].any()
    elif n < mm:
        assert ref["grp_med"][0].all() and not ref["peer"][:n].any() and not ref["grp_out"][0].any()
        assert (ref["lead"][:n] == -1).all()
    else:
        assert ref["grp_med"][0].all() and (n < 3 or ref["peer"][:n].any())  # n = 2: the MAD is 0
    assert not ref["peer"][n + 5:].any() and (ref["lead"][n + 5:] == -1).all()  # pods in no group


def test_out_of_range_ids_and_pods_in_no_group():
    v = R.data("noise", 30, 2, seed=1)
    mem = np.array([3, -1, 7, 30, 9, 11, 12, -7, 1 << 20, 20, 21, 22, 23, 24], np.int32)
    ref = check_against_brute(v, [0, 9, 9, 14], mem, 4, 0.0, 0.0)
    clean = R.peer_score(v, [0, 5, 5, 10], [3, 7, 9, 11, 12, 20, 21, 22, 23, 24], 4, 0.0, 0.0)
    R.same(clean, ref, "as if not listed")
    listed = [3, 7, 9, 11, 12, 20, 21, 22, 23, 24]
    rest = np.setdiff1d(np.arange(30), listed)
    assert not ref["peer"][rest].any() and not ref["score"][rest].any() and (ref["lead"][rest] == -1).all()


@pytest.mark.parametrize("kind", ["noise", "ties", "signs", "nonfinite"])
def test_random_data_against_brute_force(kind):
    sizes = [0, 1, 2, 3, 4, 5, 8, 21]
    gp, mem = R.layout(sizes, 50, seed=3, sentinels=1)
    v = R.data(kind, 50, 4, seed=5)
    check_against_brute(v, gp, mem, 4, 0.0, 3.0)
    check_against_brute(v, gp, mem, 1, 0.5, 0.0)
    check_against_brute(v, gp, mem, 21, 0.5, 3.0)


def test_refusals():
    v = np.zeros((6, 2), np.float32)
    gp, mem = [0, 6], np.arange(6)
    for kw in (dict(min_members=0), dict(min_scale=-1.0), dict(min_scale=float("inf")), dict(min_scale=float("nan")),
               dict(out_thr=-1.0), dict(out_thr=float("inf")), dict(out_thr=float("nan"))):
        with pytest.raises(ValueError):
            R.peer_score(v, gp, mem, **kw)
    with pytest.raises(ValueError):
        R.peer_score(np.zeros((6, 3), np.float32), gp, mem)
    assert R.peer_score(np.zeros((0, 2), np.float32), gp, mem)["score"].shape == (0,)
    none = R.peer_score(v, [0], [])  # no groups: every pod gets the defaults
    assert none["grp_med"].shape == (0, 2) and not none["peer"].any() and (none["lead"] == -1).all()


# ---- krca/peers.py -------------------------------------------------------------------------------------
def test_groups_from_labels():
    gp, mem = groups_from_labels([2, 0, -1, 2, 0, 3, -5, 2])
    assert gp.dtype == np.int64 and mem.dtype == np.int32
    assert gp.tolist() == [0, 2, 2, 5, 6] and mem.tolist() == [1, 4, 0, 3, 7, 5]  # stable inside a group
    gp, mem = groups_from_labels([-1, -1])
    assert gp.tolist() == [0] and mem.tolist() == []
    gp, mem = groups_from_labels([1, 0], n_groups=4)
    assert gp.tolist() == [0, 1, 2, 2, 2]
    with pytest.raises(ValueError):
        groups_from_labels([0, 5], n_groups=3)


def test_peer_groups_validation():
    g = PeerGroups(None, [0, 2, 2, 5], [4, 1, 0, -1, 3], 6)
    assert g.n_groups == 3 and g.sizes().tolist() == [2, 0, 2] and g.group_of().tolist() == [2, 0, -1, 2, 0, -1]
    assert g.without(np.arange(6) == 4).member_host.tolist() == [-1, 1, 0, -1, 3]
    assert PeerGroups.from_labels(None, [1, -1, 0, 1]).member_host.tolist() == [2, 0, 3]
    for gp, mem in (([1, 2], [0, 1]), ([0, 3], [0, 1]), ([0, 2, 1, 2], [0, 1]), ([0, 2], [0, 6]), ([0, 2], [0, -2]),
                    ([0, 1, 2], [3, 3]), ([], [])):
        with pytest.raises(ValueError):
            PeerGroups(None, gp, mem, 6)


# ---- agents ----------------------------------------------------------------------------------------------
class PeerOracleEngine(ShiftOracleEngine):
    """OracleEngine that answers shift_score and peer_score from the restatements (NativeEngine's keys)."""

    def peer_score(self, v, groups, min_members=4, min_scale=0.0, out_thr=3.0):
        v = np.asarray(v.cpu() if hasattr(v, "cpu") else v, np.float32)
        gp, mem = (groups.grp_ptr_host, groups.member_host) if hasattr(groups, "grp_ptr_host") else groups
        r = R.peer_score(v, gp, mem, min_members, min_scale, out_thr)
        out = dict(r)
        for k in R.KEYS:
            out[k + "_host"] = r[k]
        return out


@functools.lru_cache(maxsize=None)
def mesh_case(n=400, T=200):
    """400 pods in 20 services over 16 nodes with a dependency mesh: 2 surging services, 3 faulted
    replicas (one of them inside a surging service), 1 bad node."""
    m = synth.make_graph(n, avg_degree=4, seed=6)
    x, info = synth.make_metrics_replicas(n, 8, T, seed=6, n_nodes=16, n_surges=2, n_faults=3, faults_in_surges=1,
                                          n_bad_nodes=1, walk_sigma=0.6, node_units=8.0)
    return m, x.numpy(), info


def labels_of(info):
    return {"service": info["service"], "node": info["node"]}


PEER_ROW = {"resource", "service", "metric", "deviation", "group_median", "scale", "peers_out", "group_size",
            "description", "severity"}
WIDE_ROW = {"service", "metric", "shift", "members", "description"}
NODE_ROW = {"node", "metric", "deviation", "effect", "pods", "description", "severity"}


def check_peer_keys(res, names, x, info, value="shift", topk=10, floor=None, thr=None, node_thr=None, mm=4):
    """The three keys against the restatement alone: schema, order, thresholds and every number."""
    T, P, M = x.shape
    floor = PEER_DEFAULTS[value][0] if floor is None else floor
    thr = PEER_DEFAULTS[value][1] if thr is None else thr
    node_thr = NODE_THRESHOLD if node_thr is None else node_thr
    sh = S.shift_score(x, 120, 3, 0)
    sg, ng = groups_from_labels(info["service"]), groups_from_labels(info["node"])
    ref = R.peer_score(sh["shift" if value == "shift" else "recent_med"], *sg, mm, floor, thr)
    order = sorted(range(P), key=lambda p: (-float(ref["score"][p]), p))[:topk]
    want = [p for p in order if ref["score"][p] > thr]
    rows = res["peer_deviations"]
    assert [r["resource"] for r in rows] == [f"Pod/{names[p]}" for p in want]
    for row, p in zip(rows, want):
        assert set(row) == PEER_ROW
        m, g = int(ref["lead"][p]), int(info["service"][p])
        den = max(1.4826 * float(ref["grp_mad"][g, m]), float(np.float32(floor)))
        assert (row["service"], row["metric"], row["deviation"], row["group_median"], row["scale"]) == \
            (g, m, float(ref["peer"][p, m]), float(ref["grp_med"][g, m]), den)
        assert row["peers_out"] == int(ref["grp_out"][g, m]) - 1 and row["group_size"] == 20
        assert row["severity"] == ("high" if ref["score"][p] > 2 * thr else "medium") and row["description"]
        assert abs(row["deviation"] - (float(sh["shift" if value == "shift" else "recent_med"][p, m])
                                       - row["group_median"]) / row["scale"]) <= 1e-5 * abs(row["deviation"])
    own = R.peer_score(sh["shift"], *sg, mm, floor, thr)["grp_med"]
    shift_thr = max(3.0, rca.null_floor(P * M))
    moved = np.abs(own).max(axis=1)
    wide = sorted(np.flatnonzero(moved > shift_thr).tolist(), key=lambda g: (-float(moved[g]), g))
    assert [r["service"] for r in res["service_wide"]] == wide
    for row in res["service_wide"]:
        assert set(row) == WIDE_ROW and row["members"] == 20 and row["description"]
        assert abs(row["shift"]) == float(moved[row["service"]]) == abs(float(own[row["service"], row["metric"]]))
    by_node = R.peer_score(ref["peer"], *ng, 1, 0.0, thr)
    N = len(ng[0]) - 1
    nodes = R.peer_score(by_node["grp_med"], [0, N], np.arange(N), mm, 0.0, thr)
    order = sorted(range(N), key=lambda n: (-float(nodes["score"][n]), n))[:topk]
    want = [n for n in order if nodes["score"][n] > node_thr]
    assert [r["node"] for r in res["node_deviations"]] == want
    for row in res["node_deviations"]:
        n, m = row["node"], int(nodes["lead"][row["node"]])
        assert set(row) == NODE_ROW and row["description"]
        assert (row["metric"], row["deviation"], row["effect"], row["pods"]) == \
            (m, float(nodes["peer"][n, m]), float(by_node["grp_med"][n, m]), int((info["node"] == n).sum()))
        assert row["severity"] == ("high" if nodes["score"][n] > 2 * node_thr else "medium")
    return ref, nodes


def test_metrics_agent_peer_deviations():
    m, x, info = mesh_case()
    names = m.names()
    client = lambda: MeshClient(m, x, groups=labels_of(info))  # noqa: E731
    plain = A.strip(MetricsAgent(MeshClient(m, x), engine=PeerOracleEngine()).analyze(NS))
    off = A.strip(MetricsAgent(client(), engine=PeerOracleEngine()).analyze(NS))
    agent = MetricsAgent(client(), engine=PeerOracleEngine(), peer_deviation=True)
    res = A.strip(agent.analyze(NS))
    assert "error" not in res and off == plain and not {"peer_deviations", "service_wide", "node_deviations"} & set(plain)
    keys = {k: res.pop(k) for k in ("peer_deviations", "service_wide", "node_deviations")}
    assert res == plain  # the option adds three keys and changes nothing else
    ref, nodes = check_peer_keys(keys, names, x, info)
    # the faulted replicas, and pods of the bad node: they deviate from their replicas too
    found = {r["resource"] for r in keys["peer_deviations"]}
    assert found >= {f"Pod/{names[p]}" for p in info["faults"]}
    assert found <= {f"Pod/{names[p]}" for p in set(info["faults"]) | set(np.flatnonzero(info["node"] == info["bad_nodes"][0]))}
    assert {r["service"] for r in keys["service_wide"]} >= set(info["surges"].tolist())
    assert [r["node"] for r in keys["node_deviations"]] == info["bad_nodes"].tolist()
    assert np.array_equal(agent.last_peer["service"]["score_host"], ref["score"])
    assert np.array_equal(agent.last_peer["nodes"]["score"], nodes["score"])


def test_metrics_agent_peer_options():
    m, x, info = mesh_case()
    names = m.names()
    kw = dict(peer_value="level", peer_min_members=5, peer_min_scale=0.25, peer_threshold=4.0, node_threshold=3.0)
    res = MetricsAgent(MeshClient(m, x, groups=labels_of(info)), engine=PeerOracleEngine(), peer_deviation=True,
                       level_shift=True, anomaly_topk=20, **kw).analyze(NS)
    assert "error" not in res and len(res["level_shifts"]) > 0
    check_peer_keys(res, names, x, info, value="level", topk=20, floor=0.25, thr=4.0, node_thr=3.0, mm=5)
    assert len(res["peer_deviations"]) > 3 and {"medium", "high"} == {r["severity"] for r in res["peer_deviations"]}
    with pytest.raises(ValueError):
        MetricsAgent(MeshClient(m, x), peer_value="median")


class NoGroupsClient(MeshClient):
    get_pod_groups = None  # a client without the accessor


def test_metrics_agent_peer_fallbacks():
    m, x, info = mesh_case()
    empty = {"peer_deviations": [], "service_wide": [], "node_deviations": []}
    plain = A.strip(MetricsAgent(MeshClient(m, x), engine=PeerOracleEngine()).analyze(NS))
    for client, word in ((NoGroupsClient(m, x), "get_pod_groups"), (MeshClient(m, x), "get_pod_groups"),
                         (MeshClient(m, x, groups={"node": info["node"]}), "get_pod_groups"),
                         (MeshClient(m, x[-100:], groups=labels_of(info)), "100 steps")):
        agent = MetricsAgent(client, engine=PeerOracleEngine(), peer_deviation=True)
        res = A.strip(agent.analyze(NS))
        assert "error" not in res and {k: res[k] for k in empty} == empty and agent.last_peer is None
        why = [s for s in res["reasoning_steps"] if s not in plain["reasoning_steps"]]
        assert len(why) == 1 and word in why[0]["observation"] and "peer deviations" in why[0]["conclusion"], why
    res = MetricsAgent(MeshClient(m, x, groups={"service": info["service"]}), engine=PeerOracleEngine(),
                       peer_deviation=True).analyze(NS)  # service labels alone: no node step
    assert len(res["peer_deviations"]) >= 3 and res["node_deviations"] == []


def check_peer_root_causes(rows, names, m, ref, x, engine=None):
    idx, val, rank = (engine or OracleEngine()).rank_root_causes(ref["score"], m.row_ptr, m.col, m.outdeg, rca.RANKING,
                                                                 n_metrics=x.shape[2])
    assert len(rows) == len(idx) > 0
    for r, (row, i, v) in enumerate(zip(rows, idx.tolist(), val.tolist())):
        assert row == {"component": f"Pod/{names[i]}", "rank": r + 1, "score": float(v), "pagerank": float(rank[i]),
                       "anomaly": float(ref["score"][i])}


def test_coordinator_peer_root_causes():
    m, x, info = mesh_case()
    names = m.names()
    client = lambda: MeshClient(m, x, groups=labels_of(info))  # noqa: E731
    plain = A.strip(Coordinator(MeshClient(m, x), engine=OracleEngine()).run_analysis("comprehensive", NS))
    off = A.strip(Coordinator(client(), engine=PeerOracleEngine()).run_analysis("comprehensive", NS))
    res = A.strip(Coordinator(client(), engine=PeerOracleEngine(), peer_deviations=True)
                  .run_analysis("comprehensive", NS))
    assert "error" not in plain and "error" not in res and off == plain
    rows, lifted = res.pop("peer_root_causes"), res.pop("node_deviations")
    keys = {k: res["agent_results"]["metrics"].pop(k) for k in ("peer_deviations", "service_wide", "node_deviations")}
    assert res == plain and lifted == keys["node_deviations"] and len(lifted) == 1
    ref, _ = check_peer_keys(keys, names, x, info)
    check_peer_root_causes(rows, names, m, ref, x)
    short = Coordinator(MeshClient(m, x[-100:], groups=labels_of(info)), engine=PeerOracleEngine(),
                        peer_deviations=True).run_analysis("comprehensive", NS)
    assert "error" not in short and "peer_root_causes" not in short and short["node_deviations"] == []


# ---- recall fixtures -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def replica_case(seed):
    """(a) 2 000 pods in services of 20 over 80 nodes, M = 8, T = 200: 10 whole services surge and 10 single
    replicas of other services fault, 30 steps before the end."""
    x, info = synth.make_metrics_replicas(2000, 8, 200, seed=seed, n_nodes=80, n_surges=10, n_faults=10)
    return x.numpy(), info


@functools.lru_cache(maxsize=None)
def node_case(seed):
    """(b) the same shape under strong shared load walks, two bad nodes."""
    x, info = synth.make_metrics_replicas(2000, 8, 200, seed=seed, n_nodes=80, n_bad_nodes=2, walk_sigma=0.6)
    return x.numpy(), info


def top(v, k):
    v = np.asarray(v)
    return set(sorted(range(len(v)), key=lambda i: (-float(v[i]), i))[:k])


def check_replica_recall(info, shift, peer, service_wide):
    """shift: shift_score's outputs; peer: the service call's on its "shift"; service_wide: the agent's key."""
    planted = set(info["faults"].tolist())
    assert len(planted) == 10 and len(info["surges"]) == 10
    assert top(peer["score"], 10) == planted              # the peer score finds exactly the planted replicas
    assert len(top(shift["score"], 10) & planted) <= 4    # the score against the pod's own past is buried
    assert set(info["surges"].tolist()) <= {r["service"] for r in service_wide}


def check_node_recall(info, shift, engine):
    floor = PEER_DEFAULTS["shift"][0]
    sg = PeerGroups.from_labels(engine, info["service"])
    ng = PeerGroups.from_labels(engine, info["node"])
    peer = engine.peer_score(shift["shift"], sg, 4, floor, 3.0)
    chain = node_effects(engine, peer["peer"], sg, ng)
    bad = set(info["bad_nodes"].tolist())
    assert len(bad) == 2 and top(chain["score"], 2) == bad  # the chain finds exactly the bad nodes
    raw = node_effects(engine, shift["shift"], None, ng)    # node medians of the raw shift, no service step
    assert top(raw["score"], 2) != bad
    return chain, raw


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_replica_recall_on_the_restatement(seed):
    x, info = replica_case(seed)
    eng = PeerOracleEngine()
    agent = MetricsAgent(MeshClient(None, x, names=[f"pod-{i}" for i in range(2000)], groups=labels_of(info)),
                         engine=eng, peer_deviation=True)
    res = agent.analyze(NS)
    assert "error" not in res
    check_replica_recall(info, agent.last_peer["shift"], agent.last_peer["service"], res["service_wide"])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_node_recall_on_the_restatement(seed):
    x, info = node_case(seed)
    check_node_recall(info, S.shift_score(x, 120, 3, 0), PeerOracleEngine())
