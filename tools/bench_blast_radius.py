#!/usr/bin/env python3
"""Blast-radius bench: krca_graph_reach / krca_graph_reach_cover on the C2 (10 000 pods / 200 000 edges)
and C4 (1 000 000 / 20 000 000) service meshes of krca.synth.make_graph, as generated and with 2 000
randomly chosen edges reversed, in both CSR layouts and both directions, for K = 10 (the ranking's own
top-10 on a planted failure) and K = 64 random sources; mark = anomaly score above the ranking's floor.

  python tools/bench_blast_radius.py [--pods 10000 1000000] [--out profiles/r15/blast_radius.json]

Per case: the levels run, the HIP-event time of a whole krca_graph_reach call and of a whole
krca_graph_reach_cover call (5 warm-ups + 20 timed calls, median and p95; a call includes its host loop
and read-backs: the calls synchronise), and the reach time per level.  The yardstick for a level is one
BFS round of krca_graph_cycle over the same arrays (32-bit words where a level here moves 64-bit ones),
re-timed in this process on the reversed mesh (the generated one is acyclic: it has no witness cycle).
Up to --ref-max-pods every output is compared with the NumPy restatement (tests/blast_ref.py), whose
host time is reported beside it.  `usefulness`: on the default and the spread failure model at the first
size, the share of the anomalous pods inside rank 1's radius, the cover and whether the planted roots
are its picks.  Needs an MI355X; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-rca-system_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_graph_structure import reverse_edges  # noqa: E402
from bench_trace import timed  # noqa: E402

DIRS = (("dependents", 0), ("dependencies", 1))


def failure(eng, synth, cfg, mesh, model, seed, steps):
    """Planted failure on `mesh` -> (score device tensor, floor, the ranking's top-k pod ids)."""
    hops = synth.spread_hops(mesh, mesh.roots, seed=seed) if model == "spread" else synth.caller_hops(mesh, mesh.roots)
    kw = synth.SPREAD_SIGMAS if model == "spread" else {}
    x = synth.make_metrics(mesh.n_pods, 8, steps, seed=seed, roots=mesh.roots, hop_sets=hops, device=eng.device, **kw)
    score = eng.rolling_score_device(x, cfg.window, cfg.z_threshold)["score"]
    del x
    idx, _, _ = eng.rank_root_causes(score, mesh.row_ptr, mesh.col, mesh.outdeg, cfg, n_metrics=8)
    return score, cfg.floor(mesh.n_pods, 8), np.asarray(idx, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, nargs="+", default=[10_000, 1_000_000])
    ap.add_argument("--reversed", type=int, nargs="+", default=[0, 2000])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300, help="metric samples per pod of the planted failure")
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--ref-max-pods", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "blast_radius.json"))
    a = ap.parse_args()
    import torch
    import blast_ref as B
    import graph_structure_ref as R
    from krca import native, synth
    from krca.rca import RANKING
    eng = native.NativeEngine(0)
    results, yard, useful = [], [], []
    for n in a.pods:
        t0 = time.perf_counter()
        mesh = synth.make_graph(n, seed=0)
        print(f"# mesh of {n} pods / {mesh.n_edges} edges generated in {time.perf_counter() - t0:.1f} s", flush=True)
        score, floor, top = failure(eng, synth, RANKING, mesh, "default", 0, a.steps)
        mark = (score[:n] > float(np.float32(floor))).to(torch.uint8)
        mark_h = mark.cpu().numpy()
        sets = {"top10": top[top >= 0], "random64": np.random.default_rng(64).integers(0, n, 64).astype(np.int32)}
        for k in a.reversed:
            rp, col = reverse_edges(R, n, mesh.row_ptr, mesh.col, k, 0)
            rp_t, col_t = R.transpose_csr(rp, col)
            E = int(rp[-1])
            for layout, (h_rp, h_col, pull) in (("pull", (rp, col, True)), ("push", (rp_t, col_t, False))):
                rp_d, col_d = eng._dev_n(h_rp, np.int64), eng._dev_n(h_col, np.int32)
                if k:  # the yardstick: krca_graph_cycle's BFS rounds over the same arrays
                    comp, _, stats, _ = eng.graph_scc_device(rp_d, col_d, n, pull)
                    if stats[4] >= 0:
                        _, rounds = eng.graph_cycle_device(rp_d, col_d, n, pull, comp, stats[4])
                        t = timed(torch, lambda: eng.graph_cycle_device(rp_d, col_d, n, pull, comp, stats[4]),
                                  a.warmup, a.runs)
                        t.update(pods=n, edges=E, reversed_edges=k, layout=layout, rounds=rounds,
                                 us_per_round=1000 * t["median_ms"] / max(rounds, 1))
                        yard.append(t)
                        print(json.dumps({"yardstick": t}), flush=True)
                    del comp
                for dname, d in DIRS:
                    for sname, src in sets.items():
                        K = len(src)
                        r = {"pods": n, "edges": E, "reversed_edges": k, "layout": layout, "direction": dname,
                             "row_role": "receiver (gather)" if int(pull) == d else "sender (scatter)",
                             "sources": sname, "K": K, "marked": int(mark_h.sum())}
                        o = eng.graph_reach_device(rp_d, col_d, n, pull, src, d, 0, mark, a.bins)
                        r["levels"] = o["rounds"]
                        r["radius_min_max"] = [int(o["hist"][0].sum(1).min()), int(o["hist"][0].sum(1).max())]
                        r["cover_steps"] = int((o["order"] >= 0).sum())
                        r["marked_covered"] = int(o["totals"][1])
                        if n <= a.ref_max_pods:
                            t0 = time.perf_counter()
                            ref = B.restate(h_rp, h_col, pull, src, d, 0, mark_h, a.bins)
                            r["host_numpy_restatement_s"] = time.perf_counter() - t0
                            got = dict(o, reach=o["reach"][:n].cpu().numpy().view(np.uint64), hist=o["hist"][0],
                                       hist_marked=o["hist"][1])
                            r["matches_restatement"] = bool(all(
                                np.ascontiguousarray(ref[key]).tobytes() == np.ascontiguousarray(got[key]).tobytes()
                                for key in B.KEYS))
                        else:
                            r["matches_restatement"] = None  # not compared at this size
                        reach = o["reach"]
                        r["reach"] = timed(torch, lambda: eng.graph_reach_device(rp_d, col_d, n, pull, src, d, 0, mark,
                                                                                 a.bins, cover=False), a.warmup, a.runs)
                        r["reach"]["us_per_level"] = 1000 * r["reach"]["median_ms"] / max(r["levels"], 1)
                        r["cover"] = timed(torch, lambda: eng.graph_reach_cover_device(reach, mark, n, K), a.warmup,
                                           a.runs)
                        results.append(r)
                        print(json.dumps(r), flush=True)
                del rp_d, col_d
                torch.cuda.empty_cache()
        if n == a.pods[0]:  # what the radii say about a planted failure
            for model in ("default", "spread"):
                sc, fl, idx = (score, floor, top) if model == "default" else failure(eng, synth, RANKING, mesh, model, 0,
                                                                                       a.steps)
                br = eng.blast_radius(mesh.row_ptr, mesh.col, idx, score=sc, floor=fl, pull=True, bins=a.bins)
                picks = [int(br.sources[s]) for s, _ in br.cover()]
                roots = [int(x) for x in mesh.roots]
                useful.append({
                    "pods": n, "model": model, "anomalous": br.n_marked, "ranked": [int(x) for x in br.sources],
                    "planted_roots": roots, "ranked_roots": len(set(roots) & set(int(x) for x in br.sources)),
                    "rank1_share_of_anomalous": br.reached_marked(0) / max(br.n_marked, 1),
                    "largest_share_of_anomalous": max(br.reached_marked(s) for s in range(br.k)) / max(br.n_marked, 1),
                    "cover_size": len(picks), "cover_cumulative_share": br.n_covered / max(br.n_marked, 1),
                    "cover_picks": picks, "cover_gains": [g for _, g in br.cover()],
                    "picks_that_are_planted_roots": len(set(picks) & set(roots)),
                    "radius_sizes": [br.reached(s) for s in range(br.k)], "depths": br.depth.tolist()})
                print(json.dumps({"usefulness": useful[-1]}), flush=True)
        del score, mark
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "library": native.library_info(), "warmup": a.warmup,
           "timing": "HIP events around a whole call: kernels, the host level / step loop and its read-backs",
           "results": results, "graph_cycle_yardstick": yard, "usefulness": useful}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
