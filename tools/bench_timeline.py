#!/usr/bin/env python3
"""Anomaly timeline bench: what the timeline costs on top of the scorer, what the
precedence pass costs, and what first-mover ranking recalls.

  python tools/bench_timeline.py [--pods 1000000 --edges 20000000] [--out profiles/r8/timeline_bench.json]
  python tools/bench_timeline.py --recall [--out profiles/r8/timeline_recall.json]

Cost (default): the C4 shape, 1M pods x 8 metrics x 1440 steps (W = 60) resident in HBM and its 20M-edge
graph.  krca_rolling_timeline and krca_rolling_score are launched alternately on the same tensor in
one process, each launch between HIP events (warm-up, then median and p95); the byte model is the
tensor read once either way, 4 P M T bytes, plus 4 P M + 9 P bytes written by the scorer and 18 P more
by the timeline, so the predicted ratio is 1.00.  krca_rca_precede + krca_rca_first_mover_key +
krca_topk_i64 are timed on the timeline's own onsets (the anomalous fraction synth.make_metrics_onsets
produces) and on seeded onsets for 1 %, 10 % and 30 % of the pods.

--recall: top-10 recall of the planted roots on C2-size meshes (10k pods / 200k edges, 3 seeds) under
synth.make_metrics_onsets, for the default, spread and held-out chain root sets, hop delay 0 / 5 / 20
steps and root onsets 3 and 30 steps before the end: NativeEngine.first_movers beside the score alone
and the shipped RcaStep ranking (key "explained").  Recorded, not gated.  Needs an MI355X.

--recall --stream-horizon H adds the first movers of the streaming timeline (krca_stream_timeline,
episodes reported for H steps after their last exceedance) as `first_movers_stream`.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-rca-system_amd"))

HBM_SPEC = 8.0e12  # B/s


def stats(ms):
    return {"median_ms": float(np.median(ms)), "p95_ms": float(np.percentile(ms, 95)), "min_ms": float(np.min(ms)),
            "runs": len(ms)}


def timed(torch, fns, warmup, runs):
    """The callables of `fns` launched alternately, each launch between its own pair of events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: stats(v) for k, v in ms.items()}


def cost(a):
    import torch
    from krca import native, synth
    eng = native.NativeEngine(0)
    P, M, T, W = a.pods, 8, a.tsteps, 60
    mesh = synth.make_graph(P, n_edges=a.edges, seed=a.seed)
    hops = synth.caller_hops(mesh, mesh.roots)
    x, planted = synth.make_metrics_onsets(P, M, T, seed=a.seed, roots=mesh.roots, hop_sets=hops, device=eng.device,
                                           delay=5)
    out = {"device": torch.cuda.get_device_name(0), "library": native.library_info(), "hbm_spec_Bps": HBM_SPEC,
           "shape": {"pods": P, "metrics": M, "tsteps": T, "window": W, "edges": int(mesh.n_edges)},
           "warmup": a.warmup, "runs": a.runs, "planted_pods": int((planted >= 0).sum())}
    variant = native.SCORE_VARIANTS[eng.lib.krca_rolling_score_variant(P, M, T, W)]
    sc = eng.rolling_score_device(x, W, 3.0)
    tl = eng.rolling_timeline_device(x, W, 3.0, 3, 3)
    same = all(torch.equal(sc[k].view(torch.uint8), tl[k].view(torch.uint8)) for k in ("z_last", "score", "n_exceed", "flags"))
    t = timed(torch, {"rolling_score": lambda: eng.rolling_score_device(x, W, 3.0, out=sc),
                      "rolling_timeline": lambda: eng.rolling_timeline_device(x, W, 3.0, 3, 3, out=tl)}, a.warmup, a.runs)
    b_sc = 4 * P * M * T + 4 * P * M + 9 * P
    for k, extra in (("rolling_score", 0), ("rolling_timeline", 18 * P)):
        t[k]["algorithmic_bytes"] = b_sc + extra
        t[k]["fraction_of_hbm_spec"] = (b_sc + extra) / (t[k]["median_ms"] * 1e-3) / HBM_SPEC
    out["scorer"] = dict(t, kernel=variant, scoring_outputs_bit_identical=bool(same),
                         ratio_timeline_over_score=t["rolling_timeline"]["median_ms"] / t["rolling_score"]["median_ms"],
                         byte_model_ratio=(b_sc + 18 * P) / b_sc,
                         pods_with_episode=int((tl["onset"] >= 0).sum()), exceedances=int(sc["n_exceed"].sum()))
    print(json.dumps(out["scorer"]), flush=True)
    del x
    torch.cuda.empty_cache()
    # precedence: the timeline's own onsets, then seeded fractions
    rp, col = eng._csr_dev(mesh.row_ptr, mesh.col)
    g = torch.Generator(device=eng.device)
    g.manual_seed(a.seed)
    cases = [("make_metrics_onsets", tl["onset"], tl["peak"])]
    for frac in (0.01, 0.10, 0.30):
        on = torch.where(torch.rand(P, generator=g, device=eng.device) < frac,
                         torch.randint(T - 240, T, (P,), generator=g, device=eng.device, dtype=torch.int32),
                         torch.full((P,), -1, dtype=torch.int32, device=eng.device))
        cases.append((f"{frac:.0%}", on, (on >= 0).to(torch.float32) * 4.0))
    out["precedence"] = []
    for name, on, pk in cases:
        def full():
            prec = eng.rca_precede_device(on, rp, col, a.slack)
            return eng.topk_device(eng.first_mover_key_device(on, pk, prec), 10)
        prec = eng.rca_precede_device(on, rp, col, a.slack)
        r = timed(torch, {"precede": lambda: eng.rca_precede_device(on, rp, col, a.slack),
                          "precede_key_topk": full}, a.warmup, a.runs)
        n = int((on >= 0).sum())
        r.update(onsets=name, anomalous_pods=n, anomalous_fraction=n / P, slack=a.slack,
                 classified_edges=int(prec["caller_later"].sum() + prec["caller_concurrent"].sum()
                                      + prec["caller_earlier"].sum()),
                 atomic_edges=int(prec["dep_earlier"].sum() + prec["dep_concurrent"].sum()),
                 first_movers=int(((on >= 0) & (prec["dep_earlier"] == 0)).sum()))
        out["precedence"].append(r)
        print(json.dumps(r), flush=True)
    return out


def recall(a):
    import torch
    from krca import native, synth
    from krca.rca import Comm, Config, DeviceShard, RcaStep, shard_graph
    from krca.stream import StreamingRCA
    eng = native.NativeEngine(0)
    P, E, T = 10_000, 200_000, 1440
    rows = []
    for model in ("default", "spread", "chain"):
        for t_back in (3, 30):
            for delay in (0, 5, 20):
                hit = {"first_movers": [], "score": [], "explained": []}
                if a.stream_horizon:  # the streaming timeline: episodes older than the horizon are not reported
                    hit["first_movers_stream"] = []
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
                    tl = eng.rolling_timeline_device(x, 60, 3.0, 3, 3)
                    hit["first_movers"].append(rec(eng.first_movers(tl, m.row_ptr, m.col, slack=a.slack, k=10)["idx"]))
                    hit["score"].append(rec(eng.topk_device(tl["score"], 10)[0].cpu().numpy()))
                    if a.stream_horizon:  # one call: the outputs do not depend on how the steps are split
                        s = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, 8, Config(), horizon=a.stream_horizon,
                                         timeline=True)
                        s.push_metrics(x)
                        hit["first_movers_stream"].append(rec(s.first_movers(k=10, slack=a.slack)["idx"]))
                        del s
                    c = Config().replace(seed_floor=None)
                    step = RcaStep(DeviceShard(eng, x, *shard_graph(m.row_ptr, m.col, m.outdeg, 0, P), P, P, 1, c),
                                   Comm(), c, 0)
                    hit["explained"].append(rec(step.run()[0]))
                    del x, step, tl
                    torch.cuda.empty_cache()
                row = dict(model=model, root_onset_steps_before_end=t_back, delay=delay, slack=a.slack,
                           **{k: float(np.mean(v)) for k, v in hit.items()}, per_seed=hit)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return {"device": torch.cuda.get_device_name(0), "library": native.library_info(),
            **({"stream_horizon": a.stream_horizon} if a.stream_horizon else {}),
            "mesh": f"C2: {P} pods / {E} edges, 8 metrics x {T} steps, seeds 0..{a.seeds - 1}",
            "metric": "top-10 recall of the planted roots (10 per mesh)", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recall", action="store_true")
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--tsteps", type=int, default=1440)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--slack", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--stream-horizon", type=int, default=0,
                    help="--recall: also rank the first movers of StreamingRCA(timeline=True, horizon=H)")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = recall(a) if a.recall else cost(a)
    path = a.out or os.path.join(ROOT, "profiles", "r8", "timeline_recall.json" if a.recall else "timeline_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
