#!/usr/bin/env python3
"""Cost of unbounded quantifiers in run-time log pattern tables.

Default mode, the C5 window of tools/bench_stream.py (1M containers, ~2.45M lines).  Each round times, in
a fresh random order, one krca_log_scan_tables call per variant between HIP events:
  tables_S13   the 13 shipped patterns compiled at run time, this build
  parent_S13   the same image through a second library (--parent-lib: the parent commit's build): the
               fixed-length path must not move (the 3 % gate of DESIGN §3.7, on medians)
  tables_U1    S13 with exception -> Exception.*at              (737 states)
  tables_U2    U1 with two \\d+-style categories                  (719 states)

--long: what carrying the state costs on lines over 1 KiB.  Corpora of 8 KiB and of 64 KiB lines, and
one single 64 KiB line, each "best" (no state survives a segment boundary) and "worst" ("error" in the
first segment of every line: 63 rounds, one serial walk of the line).  Each text is scanned with U4
(log_dfa_long<TabRt, true>) and with F4, a fixed-length set of the same shape (log_dfa_long<TabRt, false>), --reps
times, in that order; whole-scan times between HIP events.  The schedule is printed with the result.
Per-kernel times: run `rocprofv3 --kernel-trace --stats -- python tools/bench_log_unbounded.py --long`
in a run of its own, then `--long --trace <..._kernel_trace.csv> --schedule <result json>` assigns the
long-line kernels' dispatches, in start order, to the schedule.
"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-rca-system_amd"))

U4 = [("err_timeout", r"error.*timeout"), ("retry", r"retry \d+/\d+"), ("xrun", r"x{3,}"), ("warn", r"warn[a-z]*:")]
F4 = [("err_timeout", r"error timeout"), ("retry", r"retry \d\d/\d"), ("xrun", r"x{3}"), ("warn", r"warn[a-z]{1,3}:")]


def swap(base, name, rx):
    return [(n, rx if n == name else p) for n, p in base]


def long_line(nbytes, worst):
    """A line of nbytes bytes of filler with a short match every 512 bytes; worst: "error" at its start
    and "timeout" at its end."""
    body = ("retry 12/3 " + "q" * 501) * (nbytes // 512 + 1)
    if not worst:
        return body[:nbytes]
    return "error " + body[:nbytes - 14] + " timeout"


def long_cases():
    cases = {}
    for name, nbytes, n in (("8k", 8192, 2048), ("64k", 65536, 256), ("one64k", 65536, 1)):
        for kind in ("best", "worst"):
            lines = [long_line(nbytes, kind == "worst")] * n
            cases[f"{name}_{kind}"] = ["\n".join(lines[i:i + 64]) for i in range(0, n, 64)]
    return cases


def stats(np, v):
    return {"median_us": round(float(np.median(v)), 1), "p95_us": round(float(np.percentile(v, 95)), 1),
            "min_us": round(float(np.min(v)), 1), "n": len(v)}


def timed(torch, fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) * 1e3


def run_long(a, np, torch, native, eng, pack_documents):
    tb = {"carry_U4": eng.log_tables(U4, unbounded=True), "fixed_F4": eng.log_tables(F4)}
    res, schedule = {}, []
    eng._log_cap = 4096  # every corpus fits the one call: one long-line dispatch per scan
    for case, docs in long_cases().items():
        blob, off = pack_documents(docs)
        text, offd = eng.upload_blob(blob), eng._dev(off)
        res[case] = {"text_bytes": len(blob), "lines": sum(d.count("\n") + 1 for d in docs)}
        for variant, t in tb.items():
            r = eng.log_scan_device(text, offd, validate=False, tables=t)  # warm-up, and the result
            hist = r["hist"].sum(0).tolist()
            if variant == "carry_U4":
                assert hist[0] == (res[case]["lines"] if case.endswith("worst") else 0), (case, hist)
            us = [timed(torch, lambda: eng.log_scan_device(text, offd, validate=False, tables=t)) for _ in range(a.reps)]
            schedule.append({"case": case, "variant": variant, "dispatches": a.reps + 1})
            res[case][variant] = {"scan": stats(np, us), "hist": hist}
        res[case]["scan_ratio_carry_vs_fixed"] = round(res[case]["carry_U4"]["scan"]["median_us"] /
                                                       res[case]["fixed_F4"]["scan"]["median_us"], 3)
    return {"bench": "log scan: carried long-line kernel vs the speculative one", "reps": a.reps, "cases": res,
            "schedule": schedule, "timing": "HIP events around one scan call (index, walk, long-line kernel, histogram)",
            "tables": {k: {"nsym": t.tables.nsym, "nstate": t.tables.nstate, "warm": t.tables.warm, "flags": int(t.dims.flags)}
                       for k, t in tb.items()}, "library": native.library_info()}


def merge_trace(a, np):
    """Long-line kernel durations of a rocprofv3 kernel trace, in start order, onto the schedule."""
    with open(a.schedule) as f:
        res = json.load(f)
    res = res.get("long", res)
    with open(a.trace, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "log_dfa_long" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == sum(s["dispatches"] for s in res["schedule"]), (len(rows), res["schedule"])
    k = 0
    for s in res["schedule"]:
        mine = rows[k:k + s["dispatches"]]
        k += s["dispatches"]
        want = "true>" if s["variant"] == "carry_U4" else "false>"  # log_dfa_long<TabRt<RSL>, CARRY>
        assert all(re.search(r"log_dfa_long<.*TabRt<\d>, " + want, r["Kernel_Name"]) for r in mine), (s, mine[0]["Kernel_Name"])
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine[1:]]  # (the first: warm-up)
        res["cases"][s["case"]][s["variant"]]["kernel"] = stats(np, us)
    for case, c in res["cases"].items():
        c["kernel_ratio_carry_vs_fixed"] = round(c["carry_U4"]["kernel"]["median_us"] / c["fixed_F4"]["kernel"]["median_us"], 3)
    one_b, one_w = res["cases"]["one64k_best"]["carry_U4"]["kernel"]["median_us"], res["cases"]["one64k_worst"]["carry_U4"]["kernel"]["median_us"]
    res["one_line_64k"] = {"best_us": one_b, "worst_us": one_w, "worst_over_best": round(one_w / one_b, 2),
                           "note": "best: 64 lanes walk 1 KiB each side by side, so a single lane walking the 64 KiB "
                                   "alone would take about 64 x best (less the table fill and launch inside it)"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--containers", type=int, default=1_000_000)
    ap.add_argument("--lines", type=int, default=2_500_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--long", action="store_true", help="only the long-line corpora")
    ap.add_argument("--trace", help="with --long --schedule: a rocprofv3 kernel trace CSV of a --long run")
    ap.add_argument("--schedule", help="the JSON a --long run wrote")
    ap.add_argument("--parent-lib", help="a second libkrca.so whose krca_log_scan_tables is timed in the same rounds")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    if a.trace:
        res = merge_trace(a, np)
    else:
        import torch
        from krca import native, patterns, synth
        from krca.agents.logs import pack_documents
        eng = native.NativeEngine()
        if a.long:
            res = run_long(a, np, torch, native, eng, pack_documents)
        else:
            res = run_c5(a, np, torch, native, patterns, synth, eng, pack_documents)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def run_c5(a, np, torch, native, patterns, synth, eng, pack_documents):
    t0 = time.time()
    docs = synth.make_log_corpus(a.containers, lines_per_doc=a.lines / a.containers, seed=1, hazard_rate=0.001)
    blob, off = pack_documents(docs)
    del docs
    native.check_doc_off(off, len(blob))
    text, offd = eng.upload_blob(blob), eng._dev(off)
    gen_s = time.time() - t0
    s13 = list(patterns.ERROR_PATTERNS)
    u1 = swap(s13, "exception", r"Exception.*at")
    u2 = swap(swap(u1, "timeout", r"timed? ?out after \d+ ?m?s"), "api_error", r"StatusCode=5\d+")
    tabs = {"tables_S13": eng.log_tables(s13), "tables_U1": eng.log_tables(u1, unbounded=True),
            "tables_U2": eng.log_tables(u2, unbounded=True)}
    variants = {k: (eng, t) for k, t in tabs.items()}
    if a.parent_lib:
        import ctypes
        par = native.NativeEngine()
        par.lib = ctypes.CDLL(os.path.abspath(a.parent_lib))  # (its krca_log_dims ends before the flag word: unread there)
        for name, (res_t, arg_t) in native.SIGNATURES.items():
            fn = getattr(par.lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res_t, arg_t
        variants["parent_S13"] = (par, par.log_tables(s13))
    ref = eng.log_scan_device(text, offd, validate=False)  # the compiled-in matcher
    n_lines = ref["n_lines_total"]
    for name, (e, tb) in variants.items():
        r = e.log_scan_device(text, offd, validate=False, tables=tb)
        assert r["n_lines_total"] == n_lines, name
        if name.endswith("S13"):
            assert torch.equal(r["hist"], ref["hist"]) and torch.equal(r["line_mask"], ref["line_mask"]), name
        else:  # the twelve (U1) / ten (U2) categories left as they were
            same = [c for c, (p, q) in enumerate(zip(tb.tables.patterns, s13)) if p == q]
            assert torch.equal(r["hist"][:, same], ref["hist"][:, same]), name
    times = {k: [] for k in variants}
    rng = np.random.default_rng(0)
    for rnd in range(a.warmup + a.rounds):
        for k in rng.permutation(list(variants)):
            e, tb = variants[k]
            us = timed(torch, lambda: e.log_scan_device(text, offd, validate=False, tables=tb))
            if rnd >= a.warmup:
                times[k].append(us)
    stat = {k: stats(np, v) for k, v in times.items() if v}
    res = {"bench": "log scan: run-time pattern tables with unbounded quantifiers", "containers": a.containers,
           "lines": int(n_lines), "text_bytes": len(blob), "rounds": a.rounds, "warmup": a.warmup,
           "timing": "HIP events around one krca_log_scan_tables call (line arrays allocated inside), fresh random order per round",
           "variants": stat, "corpus_gen_s": round(gen_s, 1),
           "tables": {k: {"nsym": t.tables.nsym, "nstate": t.tables.nstate, "lds_bytes": int(t.dev.numel()),
                          "flags": int(t.dims.flags)} for k, t in tabs.items()},
           "library": native.library_info()}
    if stat:
        c = stat["tables_S13"]["median_us"]
        res["ratio_vs_tables_S13"] = {k: round(v["median_us"] / c, 4) for k, v in stat.items()}
    return res


if __name__ == "__main__":
    main()
