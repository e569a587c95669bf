#!/usr/bin/env python3
"""Graph-structure bench: krca_graph_scc / krca_graph_chain / krca_graph_cycle on the C2 (10 000 pods /
200 000 edges) and C4 (1 000 000 / 20 000 000) service meshes of krca.synth.make_graph, as generated
(acyclic) and with 25 and with 2 000 randomly chosen edges reversed (back edges), in the pull layout
the mesh is kept in.

  python tools/bench_graph_structure.py [--pods 10000 1000000] [--out profiles/r13/graph_structure.json]

Per input: the rounds per phase, and for each of the three entry points the HIP-event time of a whole
call (5 warm-ups + 20 timed calls, median and p95; a call includes its host round loop and read-backs:
the calls synchronise) and that time per round (one round = one pass over the live rows; a trim round
is two launches).  Beside them, the host time on the same box of the restatement's route
(scipy.sparse.csgraph.connected_components(connection='strong') + a vectorised level peel:
tests/graph_structure_ref.py) and of tracecols.first_cycle (networkx; only up to --nx-max-edges, its
graph of 20 M edges takes minutes and gigabytes to build).  comp is verified against scipy at every
size, the other arrays against the restatement up to --ref-max-pods.  Needs an MI355X; there is no
CPU fallback.
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

from bench_trace import timed  # noqa: E402

PPR_ITERATION_US = 33.8  # one PageRank working iteration on the same 20 M-edge arrays


def reverse_edges(R, n, row_ptr, col, k, seed):
    """The pull-CSR with k edges reversed, chosen as tests/graph_structure_ref.reversed_mesh chooses them."""
    if k == 0:
        return row_ptr, col
    src, dst, _ = R.edge_list(row_ptr, col, True)
    pick = np.random.default_rng(seed + 7).choice(len(src), k, replace=False)
    src, dst = src.copy(), dst.copy()
    src[pick], dst[pick] = dst[pick], src[pick]
    return R.csr_from_edges(n, dst, src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, nargs="+", default=[10_000, 1_000_000])
    ap.add_argument("--reversed", type=int, nargs="+", default=[0, 25, 2000])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--ref-max-pods", type=int, default=10_000)
    ap.add_argument("--nx-max-edges", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "graph_structure.json"))
    a = ap.parse_args()
    import torch
    import graph_structure_ref as R
    from krca import native, synth, tracecols
    eng = native.NativeEngine(0)
    results = []
    for n in a.pods:
        t0 = time.perf_counter()
        mesh = synth.make_graph(n, seed=0)
        print(f"# mesh of {n} pods / {mesh.n_edges} edges generated in {time.perf_counter() - t0:.1f} s", flush=True)
        for k in a.reversed:
            rp, col = reverse_edges(R, n, mesh.row_ptr, mesh.col, k, 0)
            E = int(rp[-1])
            r = {"pods": n, "edges": E, "reversed_edges": k, "layout": "pull"}
            rp_d, col_d = eng._dev_n(rp, np.int64), eng._dev_n(col, np.int32)
            gs = eng.graph_structure(rp_d, col_d, pull=True)
            r["rounds"] = dict(gs.rounds)
            r["summary"] = {key: v for key, v in gs.summary().items() if key not in ("chain", "cycle", "cyclic_group_labels")}
            cyc = gs.first_cycle()
            r["summary"]["cycle_length"] = len(cyc) if cyc else 0
            # host routes on the same box
            t0 = time.perf_counter()
            ref = R.restate(rp, col, True, root=-1)
            r["host_scipy_scc_and_level_peel_s"] = time.perf_counter() - t0
            r["comp_matches_scipy"] = bool(np.array_equal(gs.comp, ref["comp"]))
            if n <= a.ref_max_pods:
                full = R.restate(rp, col, True)
                got = R.structure_arrays(gs)
                r["matches_restatement"] = bool(all(np.asarray(full[key]).tobytes() == np.asarray(got[key]).tobytes()
                                                    for key in R.STRUCT_KEYS))
            else:
                r["matches_restatement"] = None  # not compared at this size (comp is, above)
            if E <= a.nx_max_edges:
                src, dst, _ = R.edge_list(rp, col, True)
                t0 = time.perf_counter()
                nx_cycle = tracecols.first_cycle(n, src.tolist(), dst.tolist())
                r["host_first_cycle_s"] = time.perf_counter() - t0
                r["host_first_cycle_length"] = len(nx_cycle) if nx_cycle else 0
            else:
                r["host_first_cycle_s"] = None  # not measured at this size
            # device calls
            comp, _, stats, rounds = eng.graph_scc_device(rp_d, col_d, n, True)
            per_call = {"scc": rounds[1] + rounds[2] + rounds[3], "chain": gs.rounds["chain"],
                        "cycle": gs.rounds.get("cycle", 0)}
            calls = {"scc": lambda: eng.graph_scc_device(rp_d, col_d, n, True),
                     "chain": lambda: eng.graph_chain_device(rp_d, col_d, n, True, comp)}
            if stats[4] >= 0:
                calls["cycle"] = lambda: eng.graph_cycle_device(rp_d, col_d, n, True, comp, stats[4])
            for name, fn in calls.items():
                t = timed(torch, fn, a.warmup, a.runs)
                t["rounds"] = per_call[name]
                t["us_per_round"] = 1000 * t["median_ms"] / max(per_call[name], 1)
                t["rounds_of_a_pagerank_iteration"] = t["us_per_round"] / PPR_ITERATION_US
                r[name] = t
            r["device_total_median_ms"] = sum(r[name]["median_ms"] for name in calls)
            results.append(r)
            print(json.dumps(r), flush=True)
            del rp_d, col_d, comp
            torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "library": native.library_info(), "warmup": a.warmup,
           "pagerank_iteration_us": PPR_ITERATION_US,
           "timing": "HIP events around a whole call: kernels, the host round loop and its read-backs",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
