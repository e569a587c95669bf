#!/usr/bin/env python3
"""Critical-path bench: krca_trace_critical beside krca_trace_link on the spans of tools/bench_trace.py
(50 000 services, Zipf-skewed popularity), with starts from tracecols.add_starts.

  python tools/bench_trace_critical.py [--spans 10000000 100000000] [--out profiles/r12/trace_critical.json]

Per size and p_parallel (0 and 0.5): HIP-event time (5 warm-up + 20 timed runs, median and p95) of
the new call, of krca_trace_link in the same process, and of the two extra stats launches
trace_analyze makes (critical time per service and per edge).  The byte model of the new call
(DESIGN 3.15): 25 B per span are compulsory (20 in, 5 out); its nine passes move 90 B per span and
62 B per valid child in useful bytes; both fractions are those bytes over the 8 TB/s HBM spec.  Up to
--ref-max-spans the outputs are compared with tests/trace_critical_ref.py (``matches_ref``).

Also recorded, on a make_spans mesh with p_parallel = 0.5: the rank of the planted slow service by
summed self time and by critical share, and the same for a decoy service added here: one span
beside every span of the slow service (same parent, same start, 0.8 of its duration), so it is slow
but only ever beside a slower sibling.  Needs an MI355X; there is no CPU fallback.
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

from bench_trace import HBM_SPEC, make_device_spans, timed  # noqa: E402

BYTES_COMPULSORY, BYTES_PER_SPAN, BYTES_PER_CHILD = 25, 90, 62


def rank_of(values, s):
    """1-based rank of service s by descending value (ties to the lower id)."""
    order = sorted(range(len(values)), key=lambda i: (-values[i], i))
    return order.index(s) + 1


def decoy_ranks(eng, tracecols, n_traces, n_services, seed):
    base, planted = tracecols.make_spans(n_traces, n_services, seed=seed)
    cols = tracecols.add_starts(base, seed=seed, p_parallel=0.5)
    slow = planted["slow"]
    twin = np.flatnonzero((cols.svc == slow) & (cols.parent >= 0))
    decoy = n_services
    n_ops = len(cols.ops)
    cat = np.concatenate
    aug = tracecols.SpanColumns(cat([cols.svc, np.full(len(twin), decoy)]), cat([cols.parent, cols.parent[twin]]),
                                cat([cols.op, np.full(len(twin), n_ops)]),
                                cat([cols.dur_us, (cols.dur_us[twin].astype(np.int64) * 4 // 5).astype(np.uint32)]),
                                cat([cols.err, np.zeros(len(twin), np.uint8)]), cols.services + ["decoy"],
                                cols.ops + [(decoy, "op-0")], start_us=cat([cols.start_us, cols.start_us[twin]]))
    st = eng.trace_analyze(aug)
    self_sum = st.self_rec[:, tracecols.R_SUM].tolist()
    crit_sum = st.crit_rec[:, tracecols.R_SUM].tolist()
    total = sum(crit_sum)
    out = {"traces": n_traces, "services": n_services + 1, "spans": len(aug), "decoy_spans": len(twin)}
    for name, s in (("slow", slow), ("decoy", decoy)):
        out[name] = {"service": s, "rank_by_self_time": rank_of(self_sum, s), "rank_by_critical_share": rank_of(crit_sum, s),
                     "self_ms": self_sum[s] / 1000, "critical_ms": crit_sum[s] / 1000,
                     "critical_share": crit_sum[s] / total if total else 0.0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spans", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--services", type=int, default=50_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--ref-max-spans", type=int, default=10_000_000)
    ap.add_argument("--mesh-traces", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "trace_critical.json"))
    a = ap.parse_args()
    import torch
    from krca import native, tracecols
    eng = native.NativeEngine(0)
    dev, S = eng.device, a.services
    results = []
    for N in a.spans:
        svc, parent, op, dur0, err = make_device_spans(torch, dev, N, S, 2, seed=N % 1000 + 1)
        h = [x.cpu().numpy() for x in (svc, parent, op, dur0, err)]
        plain = tracecols.SpanColumns(h[0], h[1], h[2], h[3].view(np.uint32), h[4], [""] * S, [(0, "")] * (2 * S))
        del dur0
        for p_par in (0.0, 0.5):
            t0 = time.perf_counter()
            cols = tracecols.add_starts(plain, seed=1, p_parallel=p_par)
            r = {"spans": N, "services": S, "p_parallel": p_par, "add_starts_host_s": time.perf_counter() - t0}
            dur, start = eng._dev_n(cols.dur_us, np.uint32), eng._dev_n(cols.start_us, np.int64)
            caller, self_us, flags, _ = eng.trace_link_device(svc, parent, dur, err, N, S)
            edge_key, edge_slot, E = eng.trace_edges_device(caller, svc, N, S)
            crit, path, ws = eng.trace_critical_device(svc, parent, start, dur, N, S)
            n_children = int((parent >= 0).sum().item())
            r.update(edges=E, bad_spans=int(ws[0].item()), children=n_children,
                     on_path=int(((path & 2) != 0).sum().item()), roots=int(((path & 4) != 0).sum().item()))
            r["critical"] = timed(torch, lambda: eng.trace_critical_device(svc, parent, start, dur, N, S), a.warmup, a.runs)
            r["link"] = timed(torch, lambda: eng.trace_link_device(svc, parent, dur, err, N, S), a.warmup, a.runs)
            model = BYTES_PER_SPAN * N + BYTES_PER_CHILD * n_children
            r["critical"]["byte_model"] = model
            r["critical"]["fraction_of_hbm_spec"] = model / (r["critical"]["median_ms"] * 1e-3) / HBM_SPEC
            r["critical"]["compulsory_bytes"] = BYTES_COMPULSORY * N
            r["critical"]["compulsory_fraction_of_hbm_spec"] = BYTES_COMPULSORY * N / (r["critical"]["median_ms"] * 1e-3) / HBM_SPEC
            r["critical_over_link"] = r["critical"]["median_ms"] / r["link"]["median_ms"]
            on = (path & 2) != 0
            neg = torch.full_like(svc, -1)
            for name, slot, n_slots in (("crit", torch.where(on, svc, neg), S), ("critedge", torch.where(on, edge_slot, neg), E)):
                rec, hist = eng.trace_stats_device(slot, crit, flags, N, n_slots)
                r[f"stats_{name}"] = timed(torch, lambda: eng.trace_stats_device(slot, crit, flags, N, n_slots, rec=rec, hist=hist),
                                           a.warmup, a.runs)
                del rec, hist
            if N <= a.ref_max_spans:
                import trace_critical_ref
                t0 = time.perf_counter()
                ref = trace_critical_ref.critical(cols.svc, cols.parent, cols.start_us, cols.dur_us, S)
                r["python_ref_s"] = time.perf_counter() - t0
                r["matches_ref"] = bool(np.array_equal(crit[:N].cpu().numpy().view(np.uint32), ref[0])
                                        and np.array_equal(path[:N].cpu().numpy(), ref[1]) and int(ws[0].item()) == ref[2])
                r["sum_crit_equals_sum_root_dur"] = bool(int(ref[0].astype(np.int64).sum()) == int(
                    cols.dur_us[(ref[1] & 4) != 0].astype(np.int64).sum()))
            else:
                r["matches_ref"] = None  # not measured at this size
            results.append(r)
            print(json.dumps(r), flush=True)
            del cols, dur, start, caller, self_us, flags, edge_key, edge_slot, crit, path, ws, on, neg
            torch.cuda.empty_cache()
        del svc, parent, op, err, plain, h
        torch.cuda.empty_cache()
    ranks = decoy_ranks(eng, tracecols, a.mesh_traces, 200, seed=11)
    print(json.dumps(ranks), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "library": native.library_info(), "hbm_spec_Bps": HBM_SPEC,
           "warmup": a.warmup, "link_yardstick": "profiles/r7/trace_bench.json: 0.34 ms at 10M spans", "results": results,
           "planted_ranks_p_parallel_0.5": ranks}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
