#!/usr/bin/env python3
"""C5 streaming replay bench (BASELINE configs[4]): per-window latency of incremental rescoring +
13-pattern log histograms + error-template histograms + warm-started re-ranking, pod-sharded.

  python tools/bench_stream.py [--pods 1000000] [--windows 8] [--lines-per-window 2500000]
  python -m torch.distributed.run --nproc-per-node G --master-addr 127.0.0.1 tools/bench_stream.py

History: T = 1440 steps are streamed in first (one krca_stream_score call per rank, timed
separately).  Each window then brings delta = 1 new metric step per pod (one sample per 15 s), the
window's log text (10M lines/min over 15 s windows = 2.5M lines, one container per pod, the rank's
pods only) and a warm-started PageRank to the networkx stop rule (tol 1e-9) with one all-gather per
iteration.  The window's log text is uploaded host -> device every window (pinned staging buffer)
and timed on its own line (h2d_ms); window_ms is the device work with the text resident.
Synthetic data (krca/synth.py); the log corpus is generated once and re-sent every window.  Rank 0
prints one JSON line; times are the max over ranks.

  python tools/bench_stream.py --timeline [--windows 400] [--warmup 20] [--other-lib LIB] [--out FILE]

times the rescoring call alone, krca_stream_score against krca_stream_timeline (and against a second
library's krca_stream_score), on the same history and windows: timeline_ab below.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-rca-system_amd"))


def timeline_ab(eng, x, T, delta, windows, warmup, cfg, gap, min_count, other_lib=None):
    """--timeline: krca_stream_score against krca_stream_timeline, window by window.

    Each call owns a stream of its own (rolling state, and the episode state for the timeline), all
    primed with the same T steps of history, so every timed call finds the resident state a C5 window
    finds; every window feeds the same `delta` new steps to each of them, one after the other, in a
    fresh random order every window.  One device-event pair per call; medians over the timed
    windows (after `warmup` untimed ones).  other_lib: a second libkrca.so (the parent commit's
    build) whose krca_stream_score joins the rotation -- the same-box check that the scoring-only
    instantiation did not change."""
    import ctypes

    import torch

    from krca import native
    from krca.stream import timeline_window_bytes, window_bytes
    P, M = int(x.shape[1]), int(x.shape[2])
    W, H, thr = cfg.window, T, float(cfg.z_threshold)
    dev, p = eng.device, eng.ptr
    new = lambda dt, *shape: torch.empty(shape or (P,), dtype=dt, device=dev)  # noqa: E731
    o = dict(z_last=new(torch.float32, P, M), score=new(torch.float32), n_exceed=new(torch.int32),
             flags=new(torch.uint8), onset=new(torch.int32), last=new(torch.int32), count=new(torch.int32),
             peak=new(torch.float32), lead=new(torch.int8), n_metrics=new(torch.uint8))
    four = [p(o[k]) for k in ("z_last", "score", "n_exceed", "flags")]
    six = [p(o[k]) for k in ("onset", "last", "count", "peak", "lead", "n_metrics")]
    nstate = int(eng.lib.krca_stream_state_size(P, M, W, H))

    def score_call(lib, name):
        state = torch.empty(nstate, dtype=torch.uint8, device=dev)

        def call(xw, d, t0):
            rc = lib.krca_stream_score(p(xw), P, M, d, t0, W, H, thr, p(state), *four, eng._stream())
            if rc != 0:
                raise native.KrcaError(f"{name}: krca_stream_score failed ({rc}): {lib.krca_last_error().decode()}")
        return call

    calls = {"score": score_call(eng.lib, "score")}
    ep_state = torch.empty(int(eng.lib.krca_stream_episode_state_size(P, M)), dtype=torch.uint8, device=dev)
    tl_state = torch.empty(nstate, dtype=torch.uint8, device=dev)

    def timeline_call(xw, d, t0):
        native._check(eng.lib.krca_stream_timeline(p(xw), P, M, d, t0, W, H, thr, gap, min_count, p(tl_state),
                                                   p(ep_state), *four, *six, eng._stream()), "krca_stream_timeline",
                      eng.lib)
    calls["timeline"] = timeline_call
    if other_lib:
        lib2 = ctypes.CDLL(other_lib)
        for name in ("krca_stream_score", "krca_last_error"):
            fn = getattr(lib2, name)
            fn.restype, fn.argtypes = native.SIGNATURES[name]
        calls["score_other"] = score_call(lib2, "other library")
    names = list(calls)
    for n in names:  # the history, one call each
        calls[n](x[:T], T, 0)
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    order = np.random.default_rng(0)  # every window in a fresh order: no call always follows the same one
    t = T
    for w in range(warmup + windows):
        xw = x[t:t + delta]
        evs = []
        for n in order.permutation(names):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            calls[n](xw, delta, t)
            e1.record()
            evs.append((n, e0, e1))
        torch.cuda.synchronize()
        if w >= warmup:
            for n, e0, e1 in evs:
                ms[n].append(e0.elapsed_time(e1))
        t += delta
    med = {n: float(np.median(v)) for n, v in ms.items()}
    wb, tb = window_bytes(P, M, delta), timeline_window_bytes(P, M, delta)
    res = {"metric": "krca_stream_timeline over krca_stream_score, median time of one window's call",
           "value": med["timeline"] / med["score"], "unit": "ratio", "higher_is_better": False,
           "config": {"pods": P, "metrics": M, "history": T, "delta": delta, "window": W, "horizon": H, "gap": gap,
                      "min_count": min_count, "windows": windows, "warmup": warmup},
           "score_ms": med["score"], "timeline_ms": med["timeline"], "ratio": med["timeline"] / med["score"],
           "score_bytes": wb, "timeline_bytes": tb, "modelled_ratio": tb / wb,
           "score_gbs": wb / (med["score"] * 1e-3) / 1e9, "timeline_gbs": tb / (med["timeline"] * 1e-3) / 1e9,
           "p10_p90_ms": {n: [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for n, v in ms.items()},
           "pods_reporting_an_episode": int((o["onset"] >= 0).sum().item()),
           "data": "synthetic (krca/synth.py)", "library": native.library_info()}
    if other_lib:
        res.update(score_other_ms=med["score_other"], score_over_other=med["score"] / med["score_other"],
                   other_library=other_lib)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--metrics", type=int, default=8)
    ap.add_argument("--tsteps", type=int, default=1440)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--no-prime", action="store_true", help="skip StreamingRCA.prime (the first window then "
                    "pays the log pass's kernel loads and workspace sizing)")
    ap.add_argument("--delta", type=int, default=1)
    ap.add_argument("--lines-per-window", type=int, default=2_500_000)
    ap.add_argument("--no-templates", action="store_true")
    ap.add_argument("--phases", action="store_true",
                    help="run the window's three parts one after another with events between them (per-part "
                         "times) instead of StreamingRCA.window (log pass beside the re-ranking)")
    ap.add_argument("--timeline", action="store_true",
                    help="time krca_stream_score against krca_stream_timeline windows instead (timeline_ab; one "
                         "rank, no logs, no re-ranking); --windows timed windows after --warmup untimed ones")
    ap.add_argument("--warmup", type=int, default=10, help="--timeline: untimed windows before the timed ones")
    ap.add_argument("--other-lib", help="--timeline: a second libkrca.so whose krca_stream_score is timed beside "
                                        "this build's (same process, alternating)")
    ap.add_argument("--out", help="--timeline: also write the JSON result to this file")
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    from krca import native, synth
    from krca.agents.logs import pack_documents
    from krca.rca import Comm, Config, shard_range
    from krca.stream import StreamingRCA, window_bytes
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("KRCA_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    eng = native.NativeEngine(local)
    P, M, T = a.pods, a.metrics, a.tsteps
    mesh = synth.make_graph(P, n_edges=a.edges, seed=0)
    hops = synth.caller_hops(mesh, mesh.roots)
    lo, hi, _ = shard_range(P, world, rank)
    n_win = a.windows + (a.warmup if a.timeline else 0)
    x = synth.make_metrics_range(lo, hi, M, T + n_win * a.delta, seed=0, roots=mesh.roots, hop_sets=hops,
                                 device=torch.device("cuda", local))
    cfg = Config()
    if a.timeline:
        if world != 1:
            raise SystemExit("--timeline times one rank's kernels: run it without torch.distributed.run")
        res = timeline_ab(eng, x, T, a.delta, a.windows, a.warmup, cfg, 3, 3, a.other_lib)
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        return
    s = StreamingRCA(eng, mesh.row_ptr, mesh.col, mesh.outdeg, M, cfg, horizon=T, tol=1e-9, max_iter=100,
                     comm=Comm(world, rank))
    docs = synth.make_log_corpus(hi - lo, lines_per_doc=a.lines_per_window / P, seed=1 + rank, hazard_rate=0.001)
    blob, off = pack_documents(docs)
    native.check_doc_off(off, len(blob))
    eng.check_log_unicode(blob)
    n_lines = sum(d.count("\n") + (1 if d and not d.endswith("\n") else 0) for d in docs)
    if not a.no_prime:  # the log pass's kernel loads and workspace sizing, before the first window
        s.prime(len(blob), len(docs), lines_per_doc=n_lines / max(len(docs), 1), templates=not a.no_templates)
    host = torch.empty(max(len(blob), 1), dtype=torch.uint8).pin_memory()
    host[:len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
    text = torch.empty(max(len(blob), 1), dtype=torch.uint8, device=eng.device)
    offd = torch.from_numpy(off).to(eng.device)
    torch.cuda.synchronize()

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def max_over_ranks(v):
        if world == 1:
            return v
        t = torch.tensor([v], dtype=torch.float64, device=eng.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    e0, e1 = ev(), ev()
    e0.record()
    s.push_metrics(x[:T])
    e1.record()
    torch.cuda.synchronize()
    prefill_ms = max_over_ranks(e0.elapsed_time(e1))
    s.rerank()  # cold solve on the history
    torch.cuda.synchronize()
    rows = []
    t = T
    for w in range(a.windows):
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        es = [ev() for _ in range(5)]
        es[0].record()
        text[:len(blob)].copy_(host[:len(blob)], non_blocking=True)  # the window's log text, PCIe
        es[1].record()
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        es[2].record()
        if a.phases:
            s.push_metrics(x[t:t + a.delta])
            es[3].record()
            s.push_logs(text[:len(blob)], offd, templates=not a.no_templates, validate=False)
            es4 = ev()
            es4.record()
            s.rerank()
        else:
            s.window(x[t:t + a.delta], text[:len(blob)], offd, validate=False, templates=not a.no_templates)
        es[4].record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) * 1e3
        t += a.delta
        row = dict(h2d_ms=max_over_ranks(es[0].elapsed_time(es[1])), iters=s.last_iters,
                   device_ms=max_over_ranks(es[2].elapsed_time(es[4])), window_ms=max_over_ranks(wall))
        if a.phases:
            row.update(score_ms=max_over_ranks(es[2].elapsed_time(es[3])),
                       logs_ms=max_over_ranks(es[3].elapsed_time(es4)),
                       rerank_ms=max_over_ranks(es4.elapsed_time(es[4])))
        rows.append(row)
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    p95 = {k: float(np.percentile([r[k] for r in rows], 95)) for k in rows[0]}
    wb = window_bytes(hi - lo, M, a.delta)
    if rank == 0:
        res = {
            "metric": "C5 streaming window latency (ms): rescoring + log histograms + templates + warm re-ranking",
            "value": med["window_ms"], "unit": "ms/window", "higher_is_better": False, "n_gpus": world,
            "config": {"workload": "C5: 1M pods x 8 metrics, 1 new step per 15 s window, 2.5M log lines per window "
                                   "(10M/min), warm-started PPR to tol 1e-9, pod-sharded", "pods": P,
                       "edges": mesh.n_edges, "metrics": M, "history": T, "delta": a.delta,
                       "log_lines_per_window_rank0": n_lines, "log_bytes_per_window_rank0": len(blob),
                       "windows": a.windows, "templates": not a.no_templates, "ranks": world, "primed": not a.no_prime},
            "median": med, "p95": p95, "windows": rows, "prefill_ms": prefill_ms,
            "prefill_gbs_rank0": (4 * (hi - lo) * M * T) / (prefill_ms * 1e-3) / 1e9,
            "mode": "phases (sequential, per-part events)" if a.phases else "StreamingRCA.window (log pass on a side stream)",
            "stream_score_bytes_rank0": wb,
            "stream_score_gbs_rank0": wb / (med["score_ms"] * 1e-3) / 1e9 if a.phases else None,
            "logs_gbs_rank0": len(blob) / (med["logs_ms"] * 1e-3) / 1e9 if a.phases else None,
            "h2d_gbs_rank0": len(blob) / (med["h2d_ms"] * 1e-3) / 1e9,
            "window_incl_h2d_ms": med["window_ms"] + med["h2d_ms"],
            "data": "synthetic (krca/synth.py; one log window re-sent every window)",
        }
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
