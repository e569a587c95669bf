#!/usr/bin/env python3
"""Lead/lag correlation along dependency edges: what krca_corr_edges costs and what
lead-root ranking recalls.

  python tools/bench_corr_edges.py [--shapes C2,C4] [--context] [--out profiles/r11/corr_edges.json]
  python tools/bench_corr_edges.py --recall [--out profiles/r11/corr_edges_recall.json]

Cost (default): at C2 (10k pods / 200k edges) and C4 (1M / 20M), T = 1440, one metric channel of
synth.make_metrics_onsets standardised on the device; krca_corr_edges between HIP events (3 warm-up, 20
timed launches, median and p95) at L = 8, L = 8 with a mask keeping 3 % of the pods, L = 0 and L = 16.
Byte model: every active edge reads its caller's row, every walked row its own, 4 T (E_active + rows
walked), plus 9 E per-edge outputs and 28 N per-pod outputs; the fraction is against 8 TB/s.
--context also times krca_corr_topk at C3 (100k pods) for comparison.

--recall: top-10 recall of the planted roots on C2-size meshes (3 seeds) under
synth.make_metrics_onsets, for the root sets, onset ages and hop delays of DESIGN.md §3.13's table:
NativeEngine.lead_roots (the last --span steps, --max-lag, --tau) beside first_movers and the shipped
RcaStep ranking (key "explained").  Recorded, not gated.  Needs an MI355X.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-rca-system_amd"))

HBM_SPEC = 8.0e12  # B/s
SHAPES = {"C2": (10_000, 200_000), "C3": (100_000, 2_000_000), "C4": (1_000_000, 20_000_000)}


def stats(ms):
    return {"median_ms": float(np.median(ms)), "p95_ms": float(np.percentile(ms, 95)), "min_ms": float(np.min(ms)),
            "runs": len(ms)}


def timed(torch, fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return stats(ms)


def byte_model(row_ptr, col, T, mask=None):
    N = len(row_ptr) - 1
    callee = np.repeat(np.arange(N, dtype=np.int64), np.diff(row_ptr))
    on = col != callee
    if mask is not None:
        on &= (mask[col] != 0) & (mask[callee] != 0)
    rows = int(np.count_nonzero(np.bincount(callee[on], minlength=N)))
    E = len(col)
    return {"active_edges": int(on.sum()), "rows_walked": rows,
            "algorithmic_bytes": int(4 * T * (int(on.sum()) + rows) + 9 * E + 28 * N)}


def cost(a):
    import torch
    from krca import native, synth
    eng = native.NativeEngine(0)
    T = a.tsteps
    out = {"device": torch.cuda.get_device_name(0), "library": native.library_info(), "hbm_spec_Bps": HBM_SPEC,
           "warmup": a.warmup, "runs": a.runs, "tau": a.tau, "shapes": []}
    for name in a.shapes.split(","):
        P, E = SHAPES[name]
        mesh = synth.make_graph(P, n_edges=E, seed=a.seed)
        hops = synth.caller_hops(mesh, mesh.roots)
        x, _ = synth.make_metrics_onsets(P, 1, T, seed=a.seed, roots=mesh.roots, hop_sets=hops, device=eng.device,
                                         delay=5)
        z = eng.corr_unit_variance_device(x, 0)
        del x
        torch.cuda.empty_cache()
        rp, col = eng._csr_dev(mesh.row_ptr, mesh.col)
        deg = np.diff(mesh.row_ptr)
        rng = np.random.default_rng(a.seed)
        keep = (rng.random(P) < 0.03).astype(np.uint8)
        keep[np.argsort(-deg)[:P // 100]] = 1  # the well-called pods stay in, as anomalous dependencies would
        rows = []
        for label, L, mask in (("L8", 8, None), ("L8_mask3pct", 8, keep), ("L0", 0, None), ("L16", 16, None)):
            md = None if mask is None else torch.from_numpy(mask).to(eng.device)
            r = timed(torch, lambda: eng.corr_edges_device(z, rp, col, L, a.tau, 0, md), a.warmup, a.runs)
            res = eng.corr_edges_device(z, rp, col, L, a.tau, 0, md)
            r.update(case=label, max_lag=L, **byte_model(mesh.row_ptr, mesh.col, T, mask))
            r["fraction_of_hbm_spec"] = r["algorithmic_bytes"] / (r["median_ms"] * 1e-3) / HBM_SPEC
            r["correlated_edges"] = int(res["caller_follow"].sum() + res["caller_sync"].sum() + res["caller_lead"].sum())
            r["dep_leads_edges"] = int(res["caller_follow"].sum())
            rows.append(r)
            print(json.dumps(dict(shape=name, **r)), flush=True)
            del res
        out["shapes"].append({"shape": name, "pods": P, "edges": int(mesh.n_edges), "tsteps": T,
                              "max_in_degree": int(deg.max()), "rows_over_512": int((deg > 512).sum()), "cases": rows})
        del z
        torch.cuda.empty_cache()
    if a.context:
        P, E = SHAPES["C3"]
        x = synth.make_metrics(P, 1, T, seed=a.seed, device=eng.device, group_size=20)
        zz = eng.corr_prepare_device(x, 0)
        out["context_corr_topk_C3"] = timed(torch, lambda: eng.corr_topk_device(zz, 10, 0.9), 1, 3)
        print(json.dumps(out["context_corr_topk_C3"]), flush=True)
    return out


def recall(a):
    import torch
    from krca import native, synth
    from krca.rca import Comm, Config, DeviceShard, RcaStep, shard_graph
    eng = native.NativeEngine(0)
    P, E = SHAPES["C2"]
    T = 1440
    rows = []
    for model in ("default", "spread", "chain"):
        for t_back in (3, 30):
            for delay in (0, 5, 20):
                hit = {"lead_roots": [], "first_movers": [], "explained": []}
                n_lead = []
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
                    edges = eng.corr_edges(x, m.row_ptr, m.col, channel=a.channel, span=a.span, max_lag=a.max_lag,
                                           tau=a.tau, slack=a.slack, host=False)
                    lr = eng.lead_roots(edges, tl["score"], k=10)
                    hit["lead_roots"].append(rec(lr["idx"]))
                    n_lead.append(len(lr["idx"]))
                    hit["first_movers"].append(rec(eng.first_movers(tl, m.row_ptr, m.col, slack=2, k=10)["idx"]))
                    c = Config().replace(seed_floor=None)
                    step = RcaStep(DeviceShard(eng, x, *shard_graph(m.row_ptr, m.col, m.outdeg, 0, P), P, P, 1, c),
                                   Comm(), c, 0)
                    hit["explained"].append(rec(step.run()[0]))
                    del x, step, tl, edges
                    torch.cuda.empty_cache()
                row = dict(model=model, root_onset_steps_before_end=t_back, delay=delay,
                           **{k: float(np.mean(v)) for k, v in hit.items()}, lead_roots_returned=n_lead, per_seed=hit)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return {"device": torch.cuda.get_device_name(0), "library": native.library_info(),
            "params": {"channel": a.channel, "span": a.span, "max_lag": a.max_lag, "tau": a.tau, "slack": a.slack},
            "mesh": f"C2: {P} pods / {E} edges, 8 metrics x {T} steps, seeds 0..{a.seeds - 1}",
            "metric": "top-10 recall of the planted roots (10 per mesh)", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recall", action="store_true")
    ap.add_argument("--shapes", default="C2,C4")
    ap.add_argument("--context", action="store_true", help="also time krca_corr_topk at C3")
    ap.add_argument("--tsteps", type=int, default=1440)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--channel", type=int, default=0)
    ap.add_argument("--span", type=int, default=240)
    ap.add_argument("--max-lag", type=int, default=8)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--slack", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    out = recall(a) if a.recall else cost(a)
    path = a.out or os.path.join(ROOT, "profiles", "r11", "corr_edges_recall.json" if a.recall else "corr_edges.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
