#!/usr/bin/env python3
"""Trace analytics bench: krca_trace_link / _edges / _stats / _quantiles at window sizes of millions
of spans over 50 000 services with Zipf-skewed service popularity.

  python tools/bench_trace.py [--spans 10000000 100000000] [--services 50000] [--out profiles/r7/trace_bench.json]

Per size: HIP-event time per stage (5 warm-up + 20 timed runs, median and p95), the algorithmic bytes
of each stats launch -- 9 B read per span (slot 4, value 4, flags 1) plus the slot tables
S * (896 * 4 + 64) B read and written -- and the fraction of the 8 TB/s HBM spec those bytes
achieve.  The NumPy restatement (tests/trace_ref.py) is timed on the same host as the CPU figure, up
to --ref-max-spans (above it the CPU figure is reported as not measured).  Spans are generated on
the device from a seed: a fixed call graph (4 Zipf-drawn callees per service), traces of 10 spans with
a Zipf-drawn root service, each later span called by a random earlier span of its trace, log-normal
durations, 2 % errors.  Needs an MI355X; there is no CPU fallback.
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

HBM_SPEC = 8.0e12  # B/s
TRACE_LEN = 10
CALLEES = 4


def make_device_spans(torch, dev, N, S, n_ops_per_svc, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    w = 1.0 / torch.arange(1, S + 1, dtype=torch.float64, device=dev)  # Zipf, exponent 1
    perm = torch.randperm(S, generator=g, device=dev)                  # popularity is not sorted by id
    cdf = torch.cumsum(w / w.sum(), 0)

    def zipf(*shape):
        u = torch.rand(*shape, generator=g, device=dev, dtype=torch.float64)
        return perm[torch.searchsorted(cdf, u).clamp_(max=S - 1)]

    callees = zipf(S, CALLEES)  # a fixed call graph of at most CALLEES * S edges, popular services called most
    T = (N + TRACE_LEN - 1) // TRACE_LEN
    svc2 = torch.empty((T, TRACE_LEN), dtype=torch.int64, device=dev)
    par2 = torch.full((T, TRACE_LEN), -1, dtype=torch.int64, device=dev)
    svc2[:, 0] = zipf(T)
    row = torch.arange(T, device=dev, dtype=torch.int64)
    for j in range(1, TRACE_LEN):  # span j of a trace: called by a random earlier span of the trace
        back = (torch.rand(T, generator=g, device=dev) * j).to(torch.int64).clamp_(max=j - 1)
        pick = torch.randint(0, CALLEES, (T,), generator=g, device=dev)
        svc2[:, j] = callees[svc2[row, back], pick]
        par2[:, j] = row * TRACE_LEN + back
    svc = svc2.reshape(-1)[:N].to(torch.int32)
    parent = par2.reshape(-1)[:N].to(torch.int32)
    del svc2, par2
    i = torch.arange(N, device=dev, dtype=torch.int64)
    dur = torch.exp(torch.randn(N, generator=g, device=dev) * 0.8 + 9.9).clamp_(1, 2.0e9).to(torch.int32)
    err = (torch.rand(N, generator=g, device=dev) < 0.02).to(torch.uint8)
    op = svc * n_ops_per_svc + (i % n_ops_per_svc).to(torch.int32)
    return svc, parent, op, dur, err


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
    return {"median_ms": float(np.median(ms)), "p95_ms": float(np.percentile(ms, 95)), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spans", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--services", type=int, default=50_000)
    ap.add_argument("--ops-per-service", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--ref-max-spans", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "trace_bench.json"))
    a = ap.parse_args()
    import torch
    from krca import native, tracecols
    eng = native.NativeEngine(0)
    dev = eng.device
    S, NB = a.services, int(eng.lib.krca_trace_nbuckets())
    n_ops = S * a.ops_per_service
    results = []
    for N in a.spans:
        svc, parent, op, dur, err = make_device_spans(torch, dev, N, S, a.ops_per_service, seed=N % 1000 + 1)
        caller, self_us, flags, ws = eng.trace_link_device(svc, parent, dur, err, N, S)
        edge_key, edge_slot, E = eng.trace_edges_device(caller, svc, N, S)  # sizes the edge capacity once
        cap = E
        r = {"spans": N, "services": S, "edges": E, "ops": n_ops, "bad_spans": int(ws[0].item())}
        r["link"] = timed(torch, lambda: eng.trace_link_device(svc, parent, dur, err, N, S), a.warmup, a.runs)
        r["edges_sync"] = timed(torch, lambda: eng.trace_edges_device(caller, svc, N, S, cap=cap), a.warmup, a.runs)
        launches = (("svc", svc, dur, S), ("self", svc, self_us, S), ("edge", edge_slot, dur, E), ("op", op, dur, n_ops))
        for name, slot, val, n_slots in launches:
            rec, hist = eng.trace_stats_device(slot, val, flags, N, n_slots)
            t = timed(torch, lambda: eng.trace_stats_device(slot, val, flags, N, n_slots, rec=rec, hist=hist),
                      a.warmup, a.runs)
            t["slots"] = n_slots
            t["algorithmic_bytes"] = 9 * N + 2 * n_slots * (NB * 4 + 64)
            t["fraction_of_hbm_spec"] = t["algorithmic_bytes"] / (t["median_ms"] * 1e-3) / HBM_SPEC
            r[f"stats_{name}"] = t
            r[f"quantiles_{name}"] = timed(torch, lambda: eng.trace_quantiles_device(rec, hist, n_slots, tracecols.PERMILLE),
                                           a.warmup, a.runs)
            del rec, hist
        with native.tune(KRCA_TRACE_IMPL=3):  # A/B: the same launch without the per-wave fold
            rec, hist = eng.trace_stats_device(svc, dur, flags, N, S)
            r["stats_svc_unfolded"] = timed(torch, lambda: eng.trace_stats_device(svc, dur, flags, N, S, rec=rec, hist=hist),
                                            a.warmup, a.runs)
            del rec, hist
        stages = ["link", "edges_sync"] + [f"{k}_{n}" for n in ("svc", "self", "edge", "op") for k in ("stats", "quantiles")]
        r["sum_of_stage_medians_ms"] = sum(r[s]["median_ms"] for s in stages)
        if N <= a.ref_max_spans:
            import trace_ref
            h = [x.cpu().numpy() for x in (svc, parent, op, dur, err)]
            cols = tracecols.SpanColumns(h[0], h[1], h[2], h[3].view(np.uint32), h[4], [""] * S, [(0, "")] * n_ops)
            t0 = time.perf_counter()
            ref = trace_ref.NumpyTraceEngine().trace_analyze(cols)
            r["numpy_ref_s"] = time.perf_counter() - t0
            got = eng.trace_analyze(cols)
            r["matches_numpy_ref"] = bool(np.array_equal(got.edge_key, ref.edge_key) and all(
                np.array_equal(getattr(got, f"{n}_{k}"), getattr(ref, f"{n}_{k}"))
                for n in ("svc", "self", "edge", "op") for k in ("rec", "q")))
        else:
            r["numpy_ref_s"] = None  # not measured at this size
        results.append(r)
        print(json.dumps(r), flush=True)
        del svc, parent, op, dur, err, caller, self_us, flags, ws, edge_key, edge_slot
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "library": native.library_info(), "hbm_spec_Bps": HBM_SPEC,
           "warmup": a.warmup, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
