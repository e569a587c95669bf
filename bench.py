#!/usr/bin/env python3
"""Headline benchmark: pod·timesteps scored/s + end-to-end RCA top-k latency on a 1M-pod mesh.

BASELINE.json metric, configs[3] shape: synthetic 1M-pod / ~20M-edge mesh, 8 metrics x 1440
steps (46 GB of float32 metrics — it fits one MI355X, so N=1 runs the whole mesh).  One step =
the full RCA hot path (krca/rca.py): rolling z-scores of every pod -> seeded personalized
PageRank (integer fixed point to networkx's L1 stop rule, tol 1e-10, at most 30 iterations: 11
at C4) -> root-cause top-10 on the host.  Inputs are resident in HBM before timing; nothing is
cached across steps.

Multi-GPU: `python bench.py --gpus N` starts N ranks itself (a `torch.distributed.run` child
process, before anything touches the GPU); under an external launcher (WORLD_SIZE set) it must
equal --gpus.  The mesh is sharded by pod (strong scaling: the same 1M pods over N GPUs), one
all-gather over RCCL per PageRank iteration.  Rank 0 prints ONE JSON line.

Steps are pipelined over two HIP streams (two shard states over the same resident metrics): step
i+1's HBM-bound scoring runs while step i's latency-bound PageRank iterates (the scoring kernels
themselves stay one at a time, ordered by an event), and step i's top-10 is merged on the host
after step i+1 has been enqueued.  Every step still does all of its work.

A plain run sets up, warms up, times --steps steps and prints the line (`value`, `ms_per_step`).
`--full` adds what takes runs of its own: `e2e_rca_latency_ms` (one step at a time) and the
scoring kernel alone, the verification against the C oracle, the spread-model recall, the CPU
baseline and the correlation leg.  `--dump-outputs DIR` writes the last timed step's results as
DIR/<name>.npy, so that two builds can be compared output for output on the same seeded inputs.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-rca-system_amd"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec


def parse(argv=None):
    from krca.rca import EDGE_SLACK, RANKING
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--metrics", type=int, default=8)
    ap.add_argument("--tsteps", type=int, default=1440)
    ap.add_argument("--window", type=int, default=RANKING.window)
    ap.add_argument("--iters", type=int, default=RANKING.iters, help="PageRank iteration cap")
    ap.add_argument("--tol", type=float, default=RANKING.tol,
                    help="networkx L1 stop rule (sum |r - r_prev| < N * tol); 0 = exactly --iters iterations")
    ap.add_argument("--alpha", type=float, default=RANKING.alpha)
    ap.add_argument("--seed-floor", type=float, default=RANKING.seed_floor,
                    help="personalization floor in |z| units (default: krca.rca.Config's scale-aware floor)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu-sample-pods", type=int, default=25_000)
    ap.add_argument("--cpu-warmup", type=int, default=5)  # 5 warm-up + >= 20 timed runs
    ap.add_argument("--cpu-runs", type=int, default=20)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-full-mesh", action="store_true", default=True,
                    help="(default) also time the C restatement's scoring once over EVERY pod of this rank (chunks "
                         "copied to the host outside the timing; ~5 s of CPU work at C4), beside the scaled sample")
    ap.add_argument("--no-cpu-full-mesh", dest="cpu_full_mesh", action="store_false",
                    help="skip that whole-mesh pass (the sample x pods/sample only)")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--pmc", default=os.path.join(ROOT, "profiles", "pmc_latest.json"))
    ap.add_argument("--no-corr", action="store_true", help="skip the correlation leg (C4's second half)")
    ap.add_argument("--corr-pods", type=int, default=None, help="pods of the correlation leg (default: --pods)")
    ap.add_argument("--corr-tau", type=float, default=0.5)
    ap.add_argument("--corr-k", type=int, default=10)
    ap.add_argument("--corr-runs", type=int, default=3, help="timed correlation calls (after one warm-up call)")
    ap.add_argument("--corr-check-rows", type=int, default=512)
    ap.add_argument("--ppr-partition", choices=("auto", "balanced", "uniform", "replicated"), default="auto",
                    help="G > 1: PageRank rows on Partition.balanced ranges (scores all-gathered once per step, "
                         "krca.rca.SplitShard), on the scoring's uniform ranges, or the whole mesh's solve on "
                         "every rank (scores all-gathered, no collective inside the solve); auto = the sharded "
                         "solve (balanced at G >= 4, uniform below: measured, DESIGN.md §5) unless the all-gather "
                         "measured at startup costs more per solve than the replicated step's measured margin")
    ap.add_argument("--ppr-edge-slack", type=float, default=EDGE_SLACK,
                    help="Partition.balanced's in-edge cap per rank, in multiples of E / G")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="run steps back to back on one stream (default: two streams, step i+1's scoring "
                         "overlaps step i's PageRank)")
    ap.add_argument("--profile", action="store_true",
                    help="after the timed steps, one unpipelined step per rank with a HIP event around every "
                         "launch (scoring, PageRank init / folded step / exchange / finish, key + top-k) and roctx "
                         "ranges for rocprofv3 --marker-trace; per-kernel times go to the JSON line's 'profile'")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run everything beside the headline figure: the unpipelined "
                         "latency steps (e2e_rca_latency_ms, the scoring kernel alone), the oracle verification, the "
                         "spread-model recall, the CPU baseline and the correlation leg (each still has its --no-* "
                         "switch); without it the run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed as DIR/<name>.npy (float32 / "
                         "float64; rank 0 writes the whole mesh's arrays): the top-k pods and their keys, every pod's "
                         "score / n_exceed / flags and fixed-point rank; a fixed seeded sample of the pods above 64 MB")
    a = ap.parse_args(argv)
    a.corr_pods = 0 if a.no_corr or not a.full else (a.pods if a.corr_pods is None else a.corr_pods)
    return a


def launch_ranks(n, argv):
    """Start n ranks of this script (one per GPU) with torch.distributed.run as a CHILD process —
    nothing in this process has touched the GPU — and return rank 0's launcher exit status."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + list(argv)
    log(f"bench: starting {n} ranks: {' '.join(cmd)}")
    return subprocess.run(cmd).returncode


def cpu_model():
    try:
        for ln in subprocess.run(["lscpu"], capture_output=True, text=True, check=True).stdout.splitlines():
            if ln.startswith("Model name:"):
                return ln.split(":", 1)[1].strip()
    except (OSError, subprocess.CalledProcessError):
        pass
    import platform
    return platform.processor()


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# the replicated step's measured cost over the sharded one per G (ms; DESIGN.md §5, single-GPU
# emulations with a device copy standing in for the all-gather, 30-step solves): the budget the
# sharded solve's iters x (all-gather - device copy) may spend before replicating the solve is
# cheaper.  Both sides scale with the steps a solve runs: the 12-step emulation at G = 8 (the stop
# rule's count + 1, profiles/r5/g8_step_emulation_R5i.json) gave 0.22 ms, the same ~18 us per
# iteration break-even as 0.50 ms over 30 (17 us), so the rule keeps the cap (--iters) and these
# margins.
REPLICATED_MARGIN_MS = {2: 0.155, 4: 0.39, 8: 0.50}


def exchange_probe(world, n_slot, dev, reps=50):
    """The PageRank exchange at its real size, measured after init: `reps` all-gathers of one rank's
    slice (krca_ppr_slice_words(n_slot) int64) through the same call Comm makes, and a device copy of
    the gathered bytes (what the single-GPU emulations stood in for it).  Per call: the wall time of
    the back-to-back sequence (host dispatch included: the solve's iterations are issued the same
    way) and the HIP-event time; max over ranks."""
    import types

    import torch
    import torch.distributed as dist
    from krca.rca import Comm, slice_words
    words = slice_words(n_slot)
    send = torch.zeros(words, dtype=torch.int64, device=dev)
    out = torch.zeros(world * words, dtype=torch.int64, device=dev)
    comm = Comm(world, dist.get_rank())  # the solve's own exchange (RCCL: the direct _allgather_base)
    slot = types.SimpleNamespace(send=send, w_all=out)
    for _ in range(5):
        comm.exchange(slot)
    res = {}
    for name, fn in (("allgather", lambda: comm.exchange(slot)),
                     ("copy", lambda: out.view(world, -1).copy_(send.expand(world, -1)))):
        torch.cuda.synchronize()
        dist.barrier()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t1 = time.perf_counter()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        res[name + "_us"] = max_over_ranks((time.perf_counter() - t1) / reps * 1e6, world)
        res[name + "_event_us"] = max_over_ranks(a.elapsed_time(b) / reps * 1e3, world)
    res["bytes_per_rank"] = words * 8
    res["reps"] = reps
    res["direct_calls"] = comm.direct_calls
    return res


def choose_ppr_mode(args, world, probe):
    """--ppr-partition auto: the sharded solve (balanced PageRank ranges at G >= 4, the scoring's
    uniform ranges below) unless iters x (all-gather - device copy) exceeds the replicated step's
    measured margin at this G, then the replicated solve."""
    if args.ppr_partition != "auto":
        return args.ppr_partition, None
    sharded = "balanced" if world >= 4 else "uniform"
    if probe is None:
        return sharded, None
    margin = REPLICATED_MARGIN_MS.get(world, 0.4)
    extra_ms = args.iters * max(probe["allgather_us"] - probe["copy_us"], 0.0) / 1e3
    mode = "replicated" if extra_ms > margin else sharded
    return mode, {"iters_x_extra_ms": extra_ms, "margin_ms": margin,
                  "rule": f"replicated when iters x (all-gather - device copy) > {margin} ms (DESIGN.md §5)"}


def profile_step(step, stream, world):
    """One unpipelined RCA step with a HIP event pair around every launch on `stream` (and a roctx
    range per phase): {phase: [ms per launch]} summarised as count / total / mean, plus the step."""
    import torch
    import torch.distributed as dist
    try:
        from torch.cuda import nvtx  # roctx on ROCm builds
        push, pop = nvtx.range_push, nvtx.range_pop
        push("krca.probe")
        pop()
    except Exception:  # noqa: BLE001
        push = pop = lambda *a: None  # noqa: E731
    s, c, cfg = step.s, step.comm, step.cfg
    from krca.rca import step_flags
    rec = []

    def timed(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        push(name)
        a.record()
        fn()
        b.record()
        pop()
        rec.append((name, a, b))

    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        if hasattr(s, "score_local"):  # SplitShard: the scoring, then the score all-gather
            timed("krca_rolling_score", s.score_local)
            timed("score_exchange", s.exchange_scores)
        else:
            timed("krca_rolling_score", s.score)
        # the sequence RcaStep.propagate runs: init, exchange, n x (folded step, exchange), finish, with
        # n = the planned steps (under the stop rule: the previous solve's count + 1)
        n = step.plan_iters()
        timed("krca_ppr_shard_init", lambda: s.init(cfg.alpha, cfg.floor(s.N, s.M)))
        timed("exchange", lambda: c.exchange(s))
        for it in range(1, n + 1):
            timed("krca_ppr_shard_step_folded",
                  lambda: s.step_folded(cfg.alpha, cfg.tol, it, step_flags(cfg.tol, it == n)))
            timed("exchange", lambda: c.exchange(s))
        timed("krca_ppr_shard_finish", lambda: s.finish(cfg.alpha, cfg.tol, n))
        timed("key+topk", lambda: step.local_candidates())
        t1.record()
    torch.cuda.synchronize()
    out = {}
    for name, a, b in rec:
        out.setdefault(name, []).append(a.elapsed_time(b))
    summ = {k: {"launches": len(v), "total_ms": float(np.sum(v)), "mean_ms": float(np.mean(v))} for k, v in out.items()}
    summ["step_ms"] = t0.elapsed_time(t1)
    summ["note"] = ("HIP events on the launch stream around each call (host launch gaps included in step_ms, "
                    "not in the per-call times); 'exchange' is the all-gather at G > 1, a buffer swap at G = 1")
    return summ


MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense fp16/bf16 MFMA


def score_bytes(pods, metrics, tsteps):
    """Algorithmic HBM bytes of one krca_rolling_score launch: the series once,
    z_last, and score / n_exceed / flags per pod."""
    return 4 * pods * metrics * tsteps + 4 * pods * metrics + 9 * pods


def max_over_ranks(v, world):
    if world == 1:
        return float(v)
    import torch
    import torch.distributed as dist
    t = torch.tensor([float(v)], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(vals, world):
    if world == 1:
        return [float(v) for v in vals]
    import torch
    import torch.distributed as dist
    t = torch.tensor([float(v) for v in vals], dtype=torch.float64, device="cuda")
    dist.all_reduce(t)
    return [float(v) for v in t.tolist()]


def gather_rows(t, n_max, world):
    """This rank's rows (<= n_max of them) -> every rank's rows, each rank's slice padded to n_max
    (krca.rca.Partition.unpad puts them back in pod order)."""
    import torch
    from krca.rca import all_gather_flat
    pad = torch.zeros(n_max, dtype=t.dtype, device=t.device)
    pad[:t.numel()] = t
    if world == 1:
        return pad
    out = torch.empty(world * n_max, dtype=t.dtype, device=t.device)
    all_gather_flat(out, pad, world)
    return out


DUMP_BYTES = 64 * 2 ** 20  # --dump-outputs writes at most this much
DUMP_ROW_BYTES = 4 + 4 + 4 + 8 + 8  # score, n_exceed, flags (float32), ppr_rank, sample_pods (float64) per pod


def dump_outputs(out_dir, shard, top_idx, top_key, part, ppart, rank):
    """--dump-outputs: the last timed step's results as <name>.npy, every rank's rows gathered to
    rank 0 in pod order.  top_idx / top_key are what the step returns (the root-cause pods, best
    first, and their keys' r*q values); score / n_exceed / flags are the scoring's outputs per pod
    and ppr_rank the PageRank fixed point (int64 units of 2^-60, rounded to float64).  When the
    per-pod arrays exceed DUMP_BYTES they hold a seeded sample of the pods, listed in sample_pods."""
    from krca.rca import key_to_score
    lo, hi, n_max = part.range(rank)
    plo, phi, p_slot = ppart.range(rank if ppart.world > 1 else 0)
    so = shard.score_out
    cols = {k: part.unpad(gather_rows(so[k][:hi - lo], n_max, part.world).cpu().numpy())
            for k in ("score", "n_exceed", "flags")}
    cols["ppr_rank"] = ppart.unpad(gather_rows(shard.r[:phi - plo], p_slot, ppart.world).cpu().numpy())
    if rank != 0:
        return
    n = len(cols["score"])
    keep = (DUMP_BYTES - 4096) // DUMP_ROW_BYTES
    pods = np.arange(n) if n <= keep else np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    out = {"top_idx": np.asarray(top_idx, np.float64), "top_key": key_to_score(top_key).astype(np.float64),
           "score": cols["score"][pods].astype(np.float32), "n_exceed": cols["n_exceed"][pods].astype(np.float32),
           "flags": cols["flags"][pods].astype(np.float32), "ppr_rank": cols["ppr_rank"][pods].astype(np.float64),
           "sample_pods": pods.astype(np.float64)}
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    log(f"bench: wrote {len(out)} arrays ({sum(a.nbytes for a in out.values()) / 2 ** 20:.1f} MiB, {len(pods)} of "
        f"{n} pods) to {out_dir}")


def pmc_traffic(args, bytes_alg, world):
    """HBM bytes per scoring launch from the counters of profiles/pmc_latest.json: as measured when
    the run's per-rank shape is the measured one (N = 1 at 1M pods), else the measured
    bytes / algorithmic ratio applied to this rank's algorithmic bytes (the kernel streams each
    series once, so the ratio does not depend on the pod count)."""
    if not os.path.exists(args.pmc):
        return None, None
    try:
        pm = json.load(open(args.pmc))
        meas = pm.get("krca_rolling_score_bytes_per_launch")
        if meas is None:
            return None, None
        alg = score_bytes(pm.get("pods"), pm.get("metrics", 8), pm.get("tsteps", 1440))
        if pm.get("pods") == args.pods and world == 1 and (args.metrics, args.tsteps) == (8, 1440):
            return meas, "measured: rocprofv3 PMC pass at this shape (" + os.path.relpath(args.pmc, ROOT) + ")"
        return meas / alg * bytes_alg, "scaled: measured/algorithmic ratio of the 1M-pod PMC pass x this rank's bytes"
    except Exception:  # noqa: BLE001
        return None, None


def corr_pmc(P):
    """The correlation's counters at P pods from profiles/pmc_mfma_latest.json (tools/gpu_pmc_mfma.sh):
    DRAM-side bytes per call and the main pass's MFMA-busy fraction at the held clock, or Nones."""
    f = os.path.join(ROOT, "profiles", "pmc_mfma_latest.json")
    try:
        e = json.load(open(f))["pods"][str(P)]
        m = e["main_pass"]
        return {"traffic": e["dram_bytes_per_call"],
                "traffic_source": f"measured: rocprofv3 PMC passes at this shape ({os.path.relpath(f, ROOT)}, "
                                  f"call {json.load(open(f))['source']})",
                "mfma_busy_main_pass": m["mfma_busy_at_held_clock"], "mfma_busy_main_pass_vs_2p4ghz": m["mfma_busy_vs_2p4ghz"],
                "main_pass_clock_ghz": m["clock_ghz"]}
    except Exception:  # noqa: BLE001
        return {"traffic": None}


def verify_step(args, cfg, mesh, shard, x, part, ppart, rank):
    """Untimed parity of the last step at any N: every rank's fixed-point ranks (its rows of
    `ppart`) and scores (its pods of `part`) are gathered to rank 0 and compared with the C oracle
    run on the whole mesh (ranks bit for bit, top-10 identical); each rank checks n_exceed / flags /
    scores of its own sampled pods against the oracle's scoring (bit-exact / 1e-5), summed over ranks."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    lo, hi, n_max = part.range(rank)
    world, n_loc = part.world, hi - lo
    plo, phi, p_slot = ppart.range(rank if ppart.world > 1 else 0)  # one range: the replicated solve
    r_all = ppart.unpad(gather_rows(shard.r[:phi - plo], p_slot, ppart.world).cpu().numpy())
    sc_all = part.unpad(gather_rows(shard.score_out["score"][:n_loc], n_max, world).cpu().numpy())
    ns = min(max(1, 2000 // world), n_loc)
    samp = np.sort(np.random.default_rng(1 + rank).choice(n_loc, size=ns, replace=False))
    st = torch.from_numpy(samp).to(x.device)
    ref = oracle.c_rolling_score(x[:, st, :].cpu().numpy(), args.window)
    dev = {k: shard.score_out[k][st].cpu().numpy() for k in ("n_exceed", "flags", "score")}
    bad = int(np.sum(dev["n_exceed"] != ref["n_exceed"]) + np.sum(dev["flags"] != ref["flags"]))
    rel = float(np.max(np.abs(dev["score"] - ref["score"]) / np.maximum(ref["score"], 1e-6)))
    bad_all, ns_all = sum_over_ranks([bad, ns], world)
    rel = max_over_ranks(rel, world)
    if rank != 0:
        return {}
    ridx, _, r = oracle.rca_rank(mesh.row_ptr, mesh.col, mesh.outdeg, sc_all, cfg.alpha, cfg.iters, cfg.seed_floor,
                                 cfg.k, key=cfg.key, tol=cfg.tol)
    return {"ppr_fixed_point_bit_identical": bool(np.array_equal(r_all, r)),
            "oracle_top10": [int(i) for i in ridx],
            "ranks_gathered": world, "score_sample_pods": int(ns_all),
            "n_exceed_flags_bit_exact": bad_all == 0, "score_max_rel_err": rel}


def cpu_baseline(args, cfg, mesh, shard, x, n_loc):
    """The C restatement (oracle/krca_oracle.c, OpenMP) on the host cores: scoring of a bounded
    pod sample scaled to the whole mesh, plus PageRank + top-10 on the whole graph (rank 0)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    ps = min(args.cpu_sample_pods, n_loc)
    xs = x[:, :ps, :].cpu().numpy()
    cores = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    score = shard.score_out["score"].cpu().numpy()
    if len(score) < args.pods:  # N > 1: PageRank seeds of the whole mesh from the oracle's own scoring
        score = np.concatenate([score[:n_loc], np.zeros(args.pods - n_loc, np.float32)])
    t_sc, t_pr = [], []
    for i in range(args.cpu_warmup + args.cpu_runs):  # BASELINE.md §3 protocol
        t1 = time.perf_counter()
        oracle.c_rolling_score(xs, args.window)
        t2 = time.perf_counter()
        oracle.rca_rank(mesh.row_ptr, mesh.col, mesh.outdeg, score, cfg.alpha, cfg.iters, cfg.seed_floor, cfg.k,
                        key=cfg.key, tol=cfg.tol)
        t3 = time.perf_counter()
        if i >= args.cpu_warmup:
            t_sc.append(t2 - t1)
            t_pr.append(t3 - t2)
    # whole step on the CPU at the same mesh size, scoring time scaled from the sample
    t_step = np.asarray(t_sc) * (args.pods / ps) + np.asarray(t_pr)
    med = float(np.median(t_step))
    out = {
        "value": args.pods * args.tsteps / med, "unit": "pod·timesteps/s", "cores": cores, "kind": "port",
        "sample": f"scoring: oracle/krca_oracle.c on {ps} pods x {args.metrics} x {args.tsteps} "
                  f"(median {np.median(t_sc):.3f} s, scaled x{args.pods / ps:.0f} to {args.pods} pods); PPR+top-10: "
                  f"full {args.pods}-node graph (median {np.median(t_pr):.3f} s); OpenMP threads = {cores}; "
                  f"{args.cpu_warmup} warm-up + {args.cpu_runs} timed runs",
        "ms_per_step": med * 1e3, "ms_per_step_p95": float(np.percentile(t_step, 95)) * 1e3,
        "cpu_model": cpu_model(),
    }
    if args.cpu_full_mesh:  # one pass of the scoring over the whole mesh, to check the sample's scaling
        chunk, t_full = 50_000, 0.0
        for a in range(0, n_loc, chunk):
            xc = x[:, a:min(a + chunk, n_loc), :].cpu().numpy()
            t1 = time.perf_counter()
            oracle.c_rolling_score(xc, args.window)
            t_full += time.perf_counter() - t1
            del xc
        out["full_mesh_scoring"] = {
            "pods": int(n_loc), "seconds": t_full, "scaled_sample_seconds": float(np.median(t_sc)) * (n_loc / ps),
            "note": f"oracle.c_rolling_score over all {n_loc} pods in chunks of {chunk} (host copies untimed), once"}
    ref_t = os.path.join(ROOT, "tests", "golden", "ref_cpu_timings.json")
    if os.path.exists(ref_t):  # the reference's own Python, timed in the build container
        rt = json.load(open(ref_t))
        out["reference_python"] = {
            "where": "build container (reference code never runs on the GPU box): " + rt["host"]["cpu_model"],
            "cores": 1, "timings": {k: {kk: v[kk] for kk in ("median_s", "p95_s", "units", "unit") if kk in v}
                                    for k, v in rt["timings"].items()},
            "note": "the reference has no rolling scoring or PageRank; these are its per-pod threshold "
                    "loop, 13-regex line histogram, SPOF betweenness and C1 comprehensive analysis"}
    return out


def spread_recall(eng, cfg, seed, pods=10_000, edges=200_000):
    """Untimed: the ranking on a C2-size mesh of the 'spread' failure model (synth.spread_hops: the
    callers of each planted root carry larger symptoms than the root), one device through RcaStep:
    recall@k of the planted roots and the top-k against the oracle."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    from krca import synth
    from krca.rca import Comm, DeviceShard, RcaStep, shard_graph
    m = synth.make_graph(pods, n_edges=edges, seed=seed)
    hops = synth.spread_hops(m, m.roots, seed=seed)
    x = synth.make_metrics(pods, 8, 1440, seed=seed, roots=m.roots, hop_sets=hops, **synth.SPREAD_SIGMAS).to(eng.device)
    c = cfg.replace(seed_floor=None)
    step = RcaStep(DeviceShard(eng, x, *shard_graph(m.row_ptr, m.col, m.outdeg, 0, pods), pods, pods, 1, c), Comm(), c, 0)
    idx, _ = step.run()
    top = [int(i) for i in idx]
    ref, _, _ = oracle.rca_rank(m.row_ptr, m.col, m.outdeg, step.s.score_out["score"].cpu().numpy(), c.alpha, c.iters,
                                c.floor(pods, 8), c.k, key=c.key, tol=c.tol)
    del x, step
    torch.cuda.empty_cache()
    return {"recall": len(set(top) & set(m.roots.tolist())) / len(m.roots), "top10_identical": top == ref.tolist(),
            "mesh": f"C2 spread: {pods} pods / {edges} edges, mesh seed {seed} (synth.spread_hops, synth.SPREAD_SIGMAS)"}


def corr_check(z32, rows, res_idx, res_val, res_cnt, res_cert, k, tau, band=1e-12):
    """Rows of the device result against float64 products of the device's own standardized rows
    (krca_corr_prepare's z32, bit-identical to the C twin: tests/test_gpu_corr.py): counts exact
    outside a 1e-12 band of tau, the top-k set exact wherever the k-th and (k+1)-th |r| are more
    than the band apart, values the float32 rounding of the exact r, certificates positive.
    Returns (bad counts, bad sets, bad values, bad certificates) over the rows."""
    import torch
    bad = [0, 0, 0, 0]
    z64 = z32.double()
    for i in range(0, len(rows), 128):
        rr = rows[i:i + 128]
        R = torch.mm(z64[rr], z64.T)
        R[torch.arange(len(rr), device=R.device), rr] = 0.0
        a = R.abs()
        cnt = res_cnt[rr]
        lo, hi = (a > tau + band).sum(1), (a > tau - band).sum(1)
        bad[0] += int(((cnt < lo) | (cnt > hi)).sum())
        gi = res_idx[rr].long()
        ex = torch.gather(R, 1, gi)
        bad[2] += int(((res_val[rr].double() - ex).abs() > 1.2e-7 * ex.abs() + 1e-12).sum())
        a[torch.arange(len(rr), device=R.device), rr] = -1.0
        top = torch.topk(a, k + 1, dim=1)
        gap = top.values[:, k - 1] - top.values[:, k]
        want = torch.sort(top.indices[:, :k], dim=1).values
        got = torch.sort(gi, dim=1).values
        bad[1] += int(((want != got).any(1) & (gap > band)).sum())
        bad[3] += int((res_cert[rr] <= 0).sum())
        del R, a
    del z64
    return bad


def corr_leg(args, eng, world, rank, local):
    """C4's correlation half (BASELINE configs[3] "... PageRank + correlation"): per-pod top-k |r|
    partners and exact |r| > tau counts over P pods x T steps of one metric channel, MFMA
    screening (csrc/corr.hip).  One warm-up call, then `corr_runs` timed calls, each from the
    metric tensor to the device results (krca_corr_prepare + krca_corr_topk; at N > 1 the
    pod-sharded krca/corr_dist.py run with its RCCL all-gathers and all-to-all), HIP events on the
    launch stream at N = 1, wall time behind a barrier and the device synchronisation at N > 1
    (max over ranks).  Roofline: P(P+1) T flops (the upper triangle incl. the diagonal, 2 per MAC)
    against the dense fp16 MFMA peak.  Then `corr_check_rows` sampled rows checked exactly."""
    import torch
    import torch.distributed as dist

    from krca import synth
    from krca.corr_dist import CorrShard, TorchComm, corr_shard_range
    P, T, k, tau = args.corr_pods, args.tsteps, args.corr_k, args.corr_tau
    dev = torch.device("cuda", local)
    t_gen = time.time()
    lo, hi, _ = corr_shard_range(P, world, rank) if world > 1 else (0, P, P)
    x = synth.make_metrics_range(lo, hi, 1, T, seed=2, group_size=20, device=dev)
    torch.cuda.synchronize()
    log(f"[rank {rank}] corr data [{lo},{hi}) x {T} generated in {time.time() - t_gen:.1f}s")
    times, res = [], None
    cs = CorrShard(eng, P, T, k, tau, world, rank) if world > 1 else None
    comm = TorchComm(world, rank) if world > 1 else None
    for i in range(1 + args.corr_runs):
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t1 = time.perf_counter()
        a.record()
        if world == 1:
            z = eng.corr_prepare_device(x, 0)
            res = eng.corr_topk_device(z, k, tau, out=res)
        else:
            res = cs.run(x, comm)
        b.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t1) * 1e3
        if i >= 1:
            times.append(a.elapsed_time(b) if world == 1 else max_over_ranks(wall, world))
    ms = float(np.median(times))
    flop = float(P) * (P + 1) * T
    tflops = flop / (ms * 1e-3) / 1e12
    # exactness of sampled rows (own rows of every rank), against the device's standardized rows
    z32 = z["z32"] if world == 1 else cs.z32[:P]
    n_loc = hi - lo
    nrow = min(max(1, args.corr_check_rows // world), n_loc)
    rows_l = np.sort(np.random.default_rng(7 + rank).choice(n_loc, size=nrow, replace=False))
    rows = torch.from_numpy(rows_l + lo).to(dev)
    full = dict(idx=torch.zeros((P, k), dtype=torch.int32, device=dev), val=torch.zeros((P, k), device=dev),
                cnt=torch.zeros(P, dtype=torch.int32, device=dev), cert=torch.zeros(P, device=dev))
    full["idx"][lo:hi], full["val"][lo:hi] = res["idx"][:n_loc], res["val"][:n_loc]
    full["cnt"][lo:hi], full["cert"][lo:hi] = res["count"][:n_loc], res["cert"][:n_loc]
    bad = corr_check(z32, rows, full["idx"], full["val"], full["cnt"], full["cert"], k, tau)
    bad = sum_over_ranks(bad + [nrow], world)
    del x, z32, full
    torch.cuda.empty_cache()
    return {"workload": f"C4 correlation half: {P} pods x {T} steps (one metric channel, 20-pod service groups), "
                        f"top-{k} |Pearson r| partners + exact |r| > {tau} counts per pod",
            "pods": P, "tsteps": T, "k": k, "tau": tau, "ms": ms, "ms_runs": times,
            "timing": "HIP events on the launch stream" if world == 1 else "wall clock behind barrier + sync, max over ranks",
            "parallelism": "one device" if world == 1 else f"pod-sharded super-tiles x{world} (krca/corr_dist.py)",
            "roofline": {"kernel": "krca_corr_topk (prepare + screening + merges + exact-count re-score)",
                         "bound": "mfma", "achieved": tflops, "peak": MFMA_PEAK_TFLOPS * world, "unit": "TFLOP/s",
                         "frac": tflops / (MFMA_PEAK_TFLOPS * world), "algorithmic_flop": flop,
                         **(corr_pmc(P) if world == 1 else {"traffic": None})},
            "verify": {"rows_checked": int(bad[4]), "counts_exact": bad[0] == 0, "sets_exact": bad[1] == 0,
                       "values_exact": bad[2] == 0, "all_certified": bad[3] == 0,
                       "reference": "float64 products of the device's z32 rows (bit-identical to the C twin)"}}


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        log(f"bench: WORLD_SIZE={os.environ.get('WORLD_SIZE')} but --gpus {args.gpus}")
        sys.exit(2)
    import torch
    import torch.distributed as dist

    from krca import native, synth
    from krca.rca import Comm, Config, DeviceShard, Explain, Partition, RcaStep, SplitShard, shard_graph

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # KRCA_BENCH_BACKEND=gloo rehearses N ranks on fewer GPUs (ranks share devices round-robin);
    # the real multi-GPU run is one rank per GPU over RCCL ("nccl")
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
    cfg = Config(window=args.window, seed_floor=args.seed_floor, alpha=args.alpha, iters=args.iters, tol=args.tol)
    cfg = cfg.replace(seed_floor=cfg.floor(args.pods, args.metrics))  # resolved once: every rank, the oracle

    # ---- synthetic mesh (host graph, device metrics; not timed) --------------------------
    t0 = time.time()
    mesh = synth.make_graph(args.pods, n_edges=args.edges, seed=args.seed)
    hops = synth.caller_hops(mesh, mesh.roots)
    # the scoring: contiguous ranges of ceil(N / G) pods (equal HBM streams per rank)
    part = Partition.uniform(args.pods, world)
    lo, hi, n_max = part.range(rank)
    # the PageRank rows: at G >= 4 by default Partition.balanced ranges, so that the hub services'
    # in-edges do not all land on rank 0 (10.6M of 20M at G = 8 with uniform ranges); the scores
    # then travel in one all-gather per step (krca.rca.SplitShard)
    probe = None
    if world > 1:  # the all-gather at the balanced ranges' slice size (the largest of the modes)
        probe = exchange_probe(world, Partition.balanced(mesh.row_ptr, world, edge_slack=args.ppr_edge_slack).n_slot,
                               torch.device("cuda", local))
    mode, why = choose_ppr_mode(args, world, probe)
    split = world > 1 and mode in ("balanced", "replicated")
    replicated = split and mode == "replicated"
    ppart = (Partition([0, args.pods]) if replicated else
             Partition.balanced(mesh.row_ptr, world, edge_slack=args.ppr_edge_slack) if split else part)
    plo, phi, p_slot = ppart.range(rank if ppart.world > 1 else 0)
    rp, col, od = shard_graph(mesh.row_ptr, mesh.col, mesh.outdeg, plo, phi, ppart)
    x = synth.make_metrics_range(lo, hi, args.metrics, args.tsteps, window=args.window, seed=args.seed,
                                 roots=mesh.roots, hop_sets=hops, device=torch.device("cuda", local))
    n_pipe = 1 if args.no_pipeline else 2
    # one engine per pipeline slot: workspaces are per engine, and the slots run concurrently
    engs = [eng] + [native.NativeEngine(local) for _ in range(n_pipe - 1)]
    comms = [Comm(world, rank) for _ in range(n_pipe)]
    if split:
        nograph = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
        shards = [SplitShard(DeviceShard(e, x, *nograph, args.pods, n_max, world, cfg),
                             DeviceShard(e, None, rp, col, od, args.pods, p_slot, ppart.world, cfg), part, ppart, rank, c)
                  for e, c in zip(engs, comms)]
    else:
        shards = [DeviceShard(e, x, rp, col, od, args.pods, n_max, world, cfg) for e in engs]
    # the replicated solve iterates without a collective (its exchange is the one-rank buffer swap);
    # the default ranking key walks the whole graph (one device copy shared by the pipeline slots)
    explain = Explain(mesh.row_ptr, mesh.col) if cfg.key == "explained" else None
    steps = [RcaStep(sh, Comm(1, 0) if replicated else c, cfg, plo, explain=explain, part=part)
             for sh, c in zip(shards, comms)]
    streams = [torch.cuda.Stream() for _ in range(n_pipe)]
    shard, step = shards[0], steps[0]
    torch.cuda.synchronize()
    log(f"[rank {rank}] mesh N={args.pods} E={mesh.n_edges} scoring=[{lo},{hi}) pagerank=[{plo},{phi}) "
        f"({int(mesh.row_ptr[phi] - mesh.row_ptr[plo])} in-edges) setup {time.time() - t0:.1f}s")

    score_done = [None]  # the scoring kernels run one at a time; only PageRank overlaps them

    def enqueue(i, events=None):
        j = i % n_pipe
        with torch.cuda.stream(streams[j]):
            if score_done[0] is not None:
                streams[j].wait_event(score_done[0])
            if events is not None:
                events[0].record()
            if split:  # the next step's scoring waits for this kernel, not for the score all-gather
                shards[j].score_local()
            else:
                shards[j].score()
            if events is not None:
                events[1].record()
            score_done[0] = torch.cuda.Event()
            score_done[0].record()
            if split:
                shards[j].exchange_scores()
            steps[j].propagate()
            return j, *steps[j].local_candidates()

    def finish(j, idx, val):
        with torch.cuda.stream(streams[j]):
            return steps[j].merge(*steps[j].settle(idx, val))

    def run_steps(n, events=None, marks=None):
        """marks: host time after each step's top-10 is on the host (per-step spacing)."""
        pending, top = None, None
        for i in range(n):
            cur = enqueue(i, events[i] if events else None)
            if pending is not None:
                top = finish(*pending)
                if marks is not None:
                    marks.append(time.perf_counter())
            pending = cur
        top = finish(*pending)
        if marks is not None:
            marks.append(time.perf_counter())
        return top

    # ---- warmup + timed steps ------------------------------------------------------------
    if args.warmup:
        run_steps(args.warmup)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    marks = [t_start]
    # HIP events on the stream each scoring kernel is launched on
    top_idx, top_key = run_steps(args.steps, ev, marks)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start
    step_ms = np.diff(np.asarray(marks)) * 1e3  # completion spacing of consecutive steps
    if world > 1:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:  # the last timed step ran on pipeline slot (steps - 1) % n_pipe
        dump_outputs(args.dump_outputs, shards[(args.steps - 1) % n_pipe], top_idx, top_key, part, ppart, rank)
    # end-to-end latency of one step (scores -> PageRank -> top-10 on the host), not pipelined (--full)
    lat = []
    ev_solo = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(5 if args.full else 0)]
    for e_solo in ev_solo:
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        with torch.cuda.stream(streams[0]):
            top_idx, top_key = step.run(score_events=e_solo)
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t1)
    solo_ms = latency_ms = latency_p95_ms = None
    if args.full:
        solo_ms = float(np.median([a.elapsed_time(b) for a, b in ev_solo]))
        latency_ms = float(np.median(lat)) * 1e3
        latency_p95_ms = float(np.percentile(lat, 95)) * 1e3
        if world > 1:
            t = torch.tensor([latency_ms], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            latency_ms = float(t.item())
    score_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    prof = profile_step(step, streams[0], world) if args.profile else None

    # ---- roofline of the dominant kernel (krca_rolling_score) ----------------------------
    # per rank: this rank's algorithmic bytes over its own average launch; the aggregate is every
    # rank's bytes over the slowest rank's average launch (at N = 1 the two are the same)
    n_loc = hi - lo
    bytes_score = score_bytes(n_loc, args.metrics, args.tsteps)
    achieved = bytes_score / (score_ms * 1e-3) / 1e9
    score_ms_max = max_over_ranks(score_ms, world)
    agg_achieved = score_bytes(args.pods, args.metrics, args.tsteps) / (score_ms_max * 1e-3) / 1e9
    traffic, traffic_src = pmc_traffic(args, bytes_score, world)

    result = None
    if rank == 0:
        value = args.pods * args.tsteps * args.steps / elapsed
        result = {
            "metric": "pod·timesteps scored/s + end-to-end RCA top-k latency (ms), 1M-pod mesh",
            "value": value, "unit": "pod·timesteps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32 (f64 window sums, int64 fixed-point ranks)",
            "data": "synthetic (seeded mesh generator krca/synth.py; no network)",
            "config": {"workload": "C4: synthetic 1M-pod / 20M-edge mesh, 8 metrics x 1440 steps, full RCA step "
                                   "(rolling z-score -> seeded PPR to networkx's L1 stop rule -> top-10), ranking of "
                                   "krca.rca.Config",
                       "pods": args.pods, "edges": mesh.n_edges, "metrics": args.metrics, "tsteps": args.tsteps,
                       "window": args.window, "ppr_iter_cap": args.iters, "ppr_tol": args.tol,
                       "alpha": args.alpha,
                       "seed_floor": cfg.seed_floor, "parallelism": f"pod-sharded x{world}",
                       "partition": "uniform contiguous pod ranges (krca.rca.Partition.uniform)",
                       "shard_bounds": [int(b) for b in part.bounds],
                       "ppr_partition": ("replicated: the whole mesh's solve on every rank, scores all-gathered once "
                                         "per step (krca.rca.SplitShard)") if replicated else
                                        (f"Partition.balanced(edge_slack={args.ppr_edge_slack}), scores all-gathered "
                                         "once per step (krca.rca.SplitShard)") if split else "the scoring's ranges",
                       "ppr_bounds": [int(b) for b in ppart.bounds], "ranking_key": cfg.key},
            "ppr_exchange_us": probe["allgather_us"] if probe else None,
            "ppr_mode": mode if world > 1 else "single device (buffer swap)",
            "ppr_exchange": dict(probe or {"allgather_us": None}, **(why or {})),
            "e2e_rca_latency_ms": latency_ms, "e2e_rca_latency_p95_ms": latency_p95_ms,
            "step_ms_median": float(np.median(step_ms)), "step_ms_p95": float(np.percentile(step_ms, 95)),
            "pipelined_streams": n_pipe,
            "scoring_variant": native.SCORE_VARIANTS[eng.lib.krca_rolling_score_variant(n_loc, args.metrics,
                                                                                      args.tsteps, args.window)],
            "roofline": {"kernel": "krca_rolling_score", "bound": "hbm", "achieved": achieved,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": bytes_score, "per_rank": True,
                         "avg_launch_ms": score_ms,
                         # the timed steps are pipelined: each scoring launch shares the GPU with the
                         # previous step's PageRank; the same kernel alone (--full's latency steps, same run):
                         "solo_avg_launch_ms": solo_ms,
                         "solo_frac": bytes_score / (solo_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if solo_ms else None,
                         "aggregate": {"achieved": agg_achieved, "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                                       "frac": agg_achieved / (HBM_PEAK_GBS * world),
                                       "bytes_per_step": score_bytes(args.pods, args.metrics, args.tsteps),
                                       "slowest_rank_avg_launch_ms": score_ms_max}},
            "rca_top10": [int(i) for i in top_idx],
            "ppr_iters_run": step.last_iters,
            "world_ranks": world, "backend": backend if world > 1 else None,
            "planted_root_recall": len(set(int(i) for i in top_idx) & set(mesh.roots.tolist())) / len(mesh.roots),
        }

    # ---- verification (not timed): bit-exact PageRank / top-10 vs the C oracle, any N -------
    if args.full and not args.no_verify:
        try:
            v = verify_step(args, cfg, mesh, shard, x, part, ppart, rank)
            if rank == 0:
                v["top10_identical"] = v.pop("oracle_top10") == result["rca_top10"]
        except Exception as e:  # reported, never a lost line (a failed check is not a passed one)
            log(f"[rank {rank}] verify failed: {e!r}")
            v = {"error": repr(e)[:500], "ppr_fixed_point_bit_identical": False, "top10_identical": False}
        if rank == 0:
            result["verify"] = v

    # ---- the ranking on the spread failure model (untimed, C2 size, rank 0) ------------------
    if rank == 0 and args.full and not args.no_verify:
        try:
            # three meshes (the C2 ablation's seeds): the mean is the recall the ranking is held to
            runs = [spread_recall(eng, cfg, args.seed + k) for k in range(3)]
            result["planted_root_recall_spread"] = float(np.mean([r["recall"] for r in runs]))
            result["spread_check"] = {"recall_per_seed": [r["recall"] for r in runs],
                                      "top10_identical": all(r["top10_identical"] for r in runs),
                                      "meshes": [r["mesh"] for r in runs]}
        except Exception as e:  # noqa: BLE001
            log(f"[rank 0] spread recall failed: {e!r}")
            result["planted_root_recall_spread"] = None
            result["spread_check"] = {"error": repr(e)[:500]}

    # ---- CPU baseline: the C restatement on the host cores, bounded sample (rank 0) -------
    if rank == 0 and args.full and not args.no_cpu_baseline:
        try:
            result["cpu_baseline"] = cpu_baseline(args, cfg, mesh, shard, x, n_loc)
        except Exception as e:
            log(f"[rank 0] cpu_baseline failed: {e!r}")
            result["cpu_baseline"] = {"error": repr(e)[:500]}

    # ---- C4's correlation half: 1M pods x 1440 steps, MFMA (after the main leg) ------------
    if args.corr_pods > 0:
        del x, shards, steps, shard, step
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        try:
            corr = corr_leg(args, eng, world, rank, local)
        except Exception as e:  # the headline line is printed whatever befalls its second leg
            log(f"[rank {rank}] corr leg failed: {e!r}")
            corr = {"error": repr(e)[:500]}
        if rank == 0:
            result["corr"] = corr

    if rank == 0 and prof is not None:
        result["profile"] = prof
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
