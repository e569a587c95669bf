#!/usr/bin/env python3
"""Level-shift score bench: what krca_shift_score costs beside the scorer, and what it
recalls where the last-step z-score is blind.

  python tools/bench_shift.py [--pods 1000000] [--out profiles/r17/shift_score.json]
  python tools/bench_shift.py --skip-cost | --skip-recall

Cost: the C4 tensor, 1M pods x 8 metrics x 1440 steps, resident in HBM.  krca_shift_score and
krca_rolling_score (W = 60) are launched alternately on it in one process, each launch between HIP
events (warm-up, then 20 timed launches: median and p95), for B in {60, 120, 256} x R in {3, 8}.  The
yardstick is the scorer in the same process: the shift score reads (B + R) * 4 bytes per series
against the scorer's 4 T, so its byte model is (B + R) / T of the scorer's -- but it is bound by
selection (32 * (2 B + R) key compares per series out of LDS), so the ratio of the times is reported
beside the byte ratio and no bandwidth fraction is claimed.

Recall: the table of DESIGN.md §3.13 (C2-size meshes, 10k pods / 200k edges, 3 seeds, default / spread /
held-out chain roots, hop delay 0 / 5 / 20, root onsets 3 and 30 steps before the end): top-10 recall of
the shift score alone and of the shipped ranking seeded with it, beside the z-score and the shipped
ranking seeded with the z-score, re-measured in the same run.  Recorded, not gated.  Needs an MI355X.
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


def next_profile_dir():
    base = os.path.join(ROOT, "profiles")
    n = max([int(d[1:]) for d in os.listdir(base) if d[0] == "r" and d[1:].isdigit()] + [0])
    return os.path.join(base, f"r{n + 1}")


def cost(a):
    import torch
    from krca import native, synth
    eng = native.NativeEngine(0)
    P, M, T, W = a.pods, 8, a.tsteps, 60
    x = synth.make_metrics(P, M, T, seed=a.seed, device=eng.device)
    sc = eng.rolling_score_device(x, W, 3.0)
    rows = []
    for B in (60, 120, 256):
        for R in (3, 8):
            sh = eng.shift_score_device(x, B, R, 0, 0.0)
            t = timed(torch, {"rolling_score": lambda: eng.rolling_score_device(x, W, 3.0, out=sc),
                              "shift_score": lambda: eng.shift_score_device(x, B, R, 0, 0.0, out=sh)},  # noqa: B023
                      a.warmup, a.runs)
            b_sc, b_sh = 4 * P * M * T + 4 * P * M + 9 * P, 4 * P * M * (B + R) + 16 * P * M + 5 * P
            row = dict(t, baseline=B, recent=R, guard=0, bytes_rolling_score=b_sc, bytes_shift_score=b_sh,
                       byte_model_ratio=b_sh / b_sc,
                       time_ratio_shift_over_score=t["shift_score"]["median_ms"] / t["rolling_score"]["median_ms"],
                       key_compares_per_series=32 * (2 * B + R), lds_bytes_per_wave=256 * max(B, R),
                       max_shift_score_clean=float(sh["score"].max()))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return {"shape": {"pods": P, "metrics": M, "tsteps": T, "window": W}, "warmup": a.warmup, "runs": a.runs,
            "scorer_kernel": native.SCORE_VARIANTS[eng.lib.krca_rolling_score_variant(P, M, T, W)], "rows": rows}


def recall(a):
    import torch
    from krca import native, synth
    from krca.rca import RANKING
    eng = native.NativeEngine(0)
    P, E, T, B, R = 10_000, 200_000, 1440, a.baseline, a.recent
    rows = []
    for model in ("default", "spread", "chain"):
        for t_back in (3, 30):
            for delay in (0, 5, 20):
                hit = {"z_score": [], "z_ranking": [], "shift_score": [], "shift_ranking": []}
                for seed in range(a.seeds):
                    m = synth.make_graph(P, n_edges=E, seed=seed)
                    if model == "chain":
                        m.roots = synth.chain_roots(m, seed=seed)
                    hops = synth.spread_hops(m, m.roots, seed=seed) if model == "spread" else synth.caller_hops(m, m.roots)
                    kw = synth.SPREAD_SIGMAS if model == "spread" else {}
                    x, _ = synth.make_metrics_onsets(P, 8, T, seed=seed, roots=m.roots, hop_sets=hops, device=eng.device,
                                                     t_root=T - t_back, delay=delay, jitter=2, **kw)
                    roots = set(int(r) for r in m.roots)
                    rec = lambda idx: len(roots & set(int(i) for i in idx)) / len(roots)  # noqa: E731
                    z = eng.rolling_score_device(x, RANKING.window, RANKING.z_threshold)["score"]
                    sh = eng.shift_score_device(x, B, R, 0, 0.0)["score"]
                    for name, seed_score in (("z", z), ("shift", sh)):
                        hit[name + "_score"].append(rec(eng.topk_device(seed_score, 10)[0].cpu().numpy()))
                        hit[name + "_ranking"].append(rec(eng.rank_root_causes(seed_score, m.row_ptr, m.col, m.outdeg,
                                                                              RANKING, n_metrics=8)[0]))
                    del x
                    torch.cuda.empty_cache()
                row = dict(model=model, root_onset_steps_before_end=t_back, delay=delay,
                           **{k: float(np.mean(v)) for k, v in hit.items()}, per_seed=hit)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return {"mesh": f"C2: {P} pods / {E} edges, 8 metrics x {T} steps, seeds 0..{a.seeds - 1}",
            "baseline": B, "recent": R, "guard": 0, "ranking": "NativeEngine.rank_root_causes, krca.rca.RANKING",
            "metric": "top-10 recall of the planted roots (10 per mesh)", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--tsteps", type=int, default=1440)
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
    path = a.out or os.path.join(next_profile_dir(), "shift_score.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(path, ROOT))


if __name__ == "__main__":
    main()
