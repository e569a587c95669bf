#!/usr/bin/env python3
"""Peer deviation bench: what the three krca_peer_score calls of the chain service ->
node -> nodes-against-nodes cost beside krca_shift_score, and what they recall where a score against the
pod's own past is buried.

  python tools/bench_peer.py [--pods 1000000] [--out profiles/r18/peer_score.json]
  python tools/bench_peer.py --skip-cost | --skip-recall

Cost: C4, 1M pods x 8 metrics in 50 000 services of 20 and 40 000 nodes of 25 (make_metrics_replicas; only
the last baseline + recent steps are generated, krca_shift_score reads no others).  The three calls and
krca_shift_score are launched alternately in one process, each launch between HIP events (warm-up, then 20
timed launches: median and p95).  One more call runs over a Zipf-skewed grouping whose largest group has at
least 100 000 members, and single groups of 40 000 (the nodes-against-nodes call), 50 000 and 1 000 000
members time the workspace path.  Each time is reported against the byte model: v read and peer written,
4 bytes each per element, 5 bytes per pod, the group arrays (8 (G + 1) + 4 n_member) and 12 bytes per
(group, metric).  No time is gated.

Recall: C2-size replica meshes (10 000 pods, 200 000 edges, 500 services of 20, 400 nodes, seeds 0..2), 10
whole services surging and 10 single replicas faulting 30 steps before the end, the faulted replicas
outside the surging services and half of them inside: top-10 recall of the planted replicas by the z-score,
the shift score and the peer score, and by the shipped ranking seeded with each; and the node case (two
bad nodes, strong load walks): the two bad nodes' scores and the largest other node's, for the chain and
for node medians of the raw shift.  Recorded, not gated.  Needs an MI355X.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-rca-system_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_timeline import timed  # noqa: E402  (alternating launches between HIP events)


def byte_model(P, M, G, n_member):
    return 8 * P * M + 5 * P + 8 * (G + 1) + 4 * n_member + 12 * G * M


def cost(a):
    import torch
    from krca import native, synth
    from krca.peers import PeerGroups
    eng = native.NativeEngine(0)
    P, M, B, R = a.pods, 8, a.baseline, a.recent
    n_nodes = max(1, P // 25)
    x, info = synth.make_metrics_replicas(P, M, B + R, seed=a.seed, n_nodes=n_nodes, device=eng.device)
    services = PeerGroups.from_labels(eng, info["service"])
    nodes = PeerGroups.from_labels(eng, info["node"])
    N = nodes.n_groups
    every = PeerGroups(eng, [0, N], np.arange(N, dtype=np.int32), N)
    sh = eng.shift_score_device(x, B, R, 0, 0.0)
    o1 = eng.peer_score_device(sh["shift"], services, 4, 0.5, 6.5)
    o2 = eng.peer_score_device(o1["peer"], nodes, 1, 0.0, 6.5)
    o3 = eng.peer_score_device(o2["grp_med"], every, 4, 0.0, 6.5)
    t = timed(torch, {"shift_score": lambda: eng.shift_score_device(x, B, R, 0, 0.0, out=sh),
                      "peer_service": lambda: eng.peer_score_device(sh["shift"], services, 4, 0.5, 6.5, out=o1),
                      "peer_by_node": lambda: eng.peer_score_device(o1["peer"], nodes, 1, 0.0, 6.5, out=o2),
                      "peer_nodes": lambda: eng.peer_score_device(o2["grp_med"], every, 4, 0.0, 6.5, out=o3)},
              a.warmup, a.runs)
    chain = dict(t, groups={"services": services.n_groups, "nodes": N},
                 bytes={"peer_service": byte_model(P, M, services.n_groups, P), "peer_by_node": byte_model(P, M, N, P),
                        "peer_nodes": byte_model(N, M, 1, N)})
    for k, b in chain["bytes"].items():
        chain[k]["model_gb_per_s"] = b / chain[k]["median_ms"] / 1e6
    print(json.dumps(chain), flush=True)
    # a Zipf-skewed grouping: sizes ~ 1 / rank, the largest at least a tenth of the pods
    rng = np.random.default_rng(a.seed)
    w = 1.0 / np.arange(1, 10001)
    sizes = np.maximum(1, (w / w.sum() * P).astype(np.int64))
    sizes[0] += P - sizes.sum()
    lab = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)[rng.permutation(P)]
    zipf = PeerGroups.from_labels(eng, lab)
    oz = eng.peer_score_device(sh["shift"], zipf, 4, 0.5, 6.5)
    tz = timed(torch, {"peer_zipf": lambda: eng.peer_score_device(sh["shift"], zipf, 4, 0.5, 6.5, out=oz)},
               a.warmup, a.runs)
    cap, small = eng.lib.krca_peer_lds_cap(), eng.lib.krca_peer_small_max()
    skew = dict(tz, groups=int(zipf.n_groups), largest=int(sizes.max()), above_small=int((sizes > small).sum()),
                above_cap=int((sizes > cap).sum()), bytes=byte_model(P, M, zipf.n_groups, P))
    skew["peer_zipf"]["model_gb_per_s"] = skew["bytes"] / skew["peer_zipf"]["median_ms"] / 1e6
    print(json.dumps(skew), flush=True)
    single = []
    for n in (40_000, 50_000, 1_000_000):
        if n > P:
            continue
        g = PeerGroups(eng, [0, n], np.arange(n, dtype=np.int32), n)
        v = sh["shift"][:n]
        o = eng.peer_score_device(v, g, 4, 0.0, 6.5)
        ts = timed(torch, {"peer_one_group": lambda: eng.peer_score_device(v, g, 4, 0.0, 6.5, out=o)},  # noqa: B023
                   a.warmup, a.runs)
        single.append(dict(ts, members=n, key_reads=64 * n * M))
        print(json.dumps(single[-1]), flush=True)
    return {"shape": {"pods": P, "metrics": M, "baseline": B, "recent": R}, "warmup": a.warmup, "runs": a.runs,
            "chain": chain, "zipf": skew, "single_group": single}


def recall(a):
    import torch
    from krca import native, synth
    from krca.peers import PeerGroups, node_effects
    from krca.rca import RANKING
    eng = native.NativeEngine(0)
    P, E, T = 10_000, 200_000, 200
    rows, node_rows = [], []
    for inside in (0, 5):
        hit = {k: [] for k in ("z_score", "shift_score", "peer_score", "z_ranking", "shift_ranking", "peer_ranking")}
        for seed in range(a.seeds):
            m = synth.make_graph(P, n_edges=E, seed=seed)
            x, info = synth.make_metrics_replicas(P, 8, T, seed=seed, n_nodes=400, n_surges=10, n_faults=10,
                                                  faults_in_surges=inside, device=eng.device)
            planted = set(info["faults"].tolist())
            rec = lambda idx: len(planted & set(int(i) for i in idx)) / len(planted)  # noqa: E731
            z = eng.rolling_score_device(x, RANKING.window, RANKING.z_threshold)["score"]
            sh = eng.shift_score_device(x, a.baseline, a.recent, 0, 0.0)
            pr = eng.peer_score_device(sh["shift"], PeerGroups.from_labels(eng, info["service"]), 4, 0.5, 6.5)
            for name, s in (("z", z), ("shift", sh["score"]), ("peer", pr["score"])):
                hit[name + "_score"].append(rec(eng.topk_device(s, 10)[0].cpu().numpy()))
                hit[name + "_ranking"].append(rec(eng.rank_root_causes(s, m.row_ptr, m.col, m.outdeg, RANKING,
                                                                      n_metrics=8)[0]))
            del x
            torch.cuda.empty_cache()
        row = dict(faults_inside_surging_services=inside, **{k: float(np.mean(v)) for k, v in hit.items()}, per_seed=hit)
        rows.append(row)
        print(json.dumps(row), flush=True)
    for seed in range(a.seeds):
        x, info = synth.make_metrics_replicas(P, 8, T, seed=seed, n_nodes=400, n_bad_nodes=2, walk_sigma=0.6,
                                              device=eng.device)
        sh = eng.shift_score_device(x, a.baseline, a.recent, 0, 0.0)
        sg, ng = PeerGroups.from_labels(eng, info["service"]), PeerGroups.from_labels(eng, info["node"])
        pr = eng.peer_score_device(sh["shift"], sg, 4, 0.5, 6.5)
        chain, raw = node_effects(eng, pr["peer"], sg, ng), node_effects(eng, sh["shift"], None, ng)
        bad = info["bad_nodes"]
        row = dict(seed=seed, **{k: {"bad_nodes": [float(s) for s in r["score"][bad]],
                                     "largest_other": float(np.delete(r["score"], bad).max())}
                                 for k, r in (("chain", chain), ("raw_shift_node_medians", raw))})
        node_rows.append(row)
        print(json.dumps(row), flush=True)
    return {"mesh": f"C2: {P} pods / {E} edges, 8 metrics x {T} steps, 500 services of 20, 400 nodes, "
                    f"seeds 0..{a.seeds - 1}", "baseline": a.baseline, "recent": a.recent,
            "peer": "krca_peer_score of shift, min_members 4, min_scale 0.5",
            "metric": "top-10 recall of the planted replicas (10 per mesh)", "rows": rows, "node_case": node_rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--baseline", type=int, default=120)
    ap.add_argument("--recent", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-recall", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from krca import native
    out = {"device": torch.cuda.get_device_name(0), "library": native.library_info()}
    if not a.skip_cost:
        out["cost"] = cost(a)
        torch.cuda.empty_cache()
    if not a.skip_recall:
        out["recall"] = recall(a)
    path = a.out or os.path.join(ROOT, "profiles", "r18", "peer_score.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(path, ROOT))


if __name__ == "__main__":
    main()
