#!/usr/bin/env python3
"""Cost of run-time pattern tables against the compiled-in log matcher.

Corpus: the C5 window of tools/bench_stream.py (1M containers, ~2.45M lines) and 32 containers of
four lines of 4 to 7 KiB, so that the wave-per-line kernel has work.  Each round times, in a fresh
random order, one scan per variant between HIP events:
  compiled     krca_log_scan (the 13 patterns in constant memory)
  tables_S13   krca_log_scan_tables, the same 13 patterns compiled at run time (32 columns)
  tables_B     krca_log_scan_tables, 16 categories / 36 symbols / 543 states (64 columns)
  tables_U1    krca_log_scan_tables, S13 with exception -> Exception.*at (tests/unbounded_pattern_sets.py:
               the carry flag, 737 states)
  parent, parent_S13, parent_B, parent_U1
               the same four through a second library (--parent-lib: the parent commit's build), in the
               same rounds: no path may move (the 3 % gate of DESIGN §3.7, on medians; ratio_vs_parent)
Medians and p95 go to --out as JSON.  Per-kernel times: run it once under
`rocprofv3 --kernel-trace --stats -- python tools/bench_log_patterns.py --rounds 3 --warmup 1`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-rca-system_amd"))

SET_B = [("quota", r"(quota exceeded|rate limit|429 Too Many Requests)"),
         ("tls", r"(x509: certificate|handshake failure|TLS handshake timeout)"),
         ("disk", r"(No space left on device|disk pressure|I/O error)")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--containers", type=int, default=1_000_000)
    ap.add_argument("--lines", type=int, default=2_500_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", help="a second libkrca.so whose scans are timed in the same rounds")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from krca import logdfa, native, patterns, synth
    from krca.agents.logs import pack_documents

    eng = native.NativeEngine()
    t0 = time.time()
    docs = synth.make_log_corpus(a.containers, lines_per_doc=a.lines / a.containers, seed=1, hazard_rate=0.001)
    long_line = lambda i: ("retry 12/3 Exception in thread " + "q" * 480) * (8 + i % 7) + " at line %d" % i  # noqa: E731
    docs += ["\n".join(long_line(4 * d + j) for j in range(4)) for d in range(32)]
    blob, off = pack_documents(docs)
    del docs
    native.check_doc_off(off, len(blob))
    text, offd = eng.upload_blob(blob), eng._dev(off)
    gen_s = time.time() - t0
    s13 = list(patterns.ERROR_PATTERNS)
    u1 = [(n, r"Exception.*at" if n == "exception" else p) for n, p in s13]
    compile_s = {}
    for name, pats in (("S13", s13), ("B", s13 + SET_B)):
        logdfa._CACHE.clear()
        t0 = time.time()
        logdfa.compile_patterns(pats)
        compile_s[name] = round(time.time() - t0, 3)
    tables = lambda e: {"S13": e.log_tables(s13), "B": e.log_tables(s13 + SET_B), "U1": e.log_tables(u1, unbounded=True)}  # noqa: E731
    tabs = tables(eng)
    tb13, tbB = tabs["S13"], tabs["B"]
    variants = {"compiled": (eng, None), **{"tables_" + k: (eng, t) for k, t in tabs.items()}}
    if a.parent_lib:
        import ctypes
        par = native.NativeEngine()
        par.lib = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name, (res_t, arg_t) in native.SIGNATURES.items():
            fn = getattr(par.lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res_t, arg_t
        variants.update({"parent": (par, None), **{"parent_" + k: (par, t) for k, t in tables(par).items()}})
    # same results first: S13 by tables equals the compiled path, B and U1 in the categories they share with
    # it, and every variant of the parent equals this build's byte for byte
    ref = eng.log_scan_device(text, offd, validate=False)
    n_lines = ref["n_lines_total"]
    assert int((ref["line_end"] - ref["line_start"] > 1024).sum().item()) >= 128  # the long-line kernel has work
    mine = {}
    for name, (e, tb) in variants.items():
        r = e.log_scan_device(text, offd, validate=False, **({"tables": tb} if tb is not None else {}))
        assert r["n_lines_total"] == n_lines, name
        kind = name.split("_")[-1].replace("parent", "compiled")  # compiled, S13, B or U1
        if kind in ("B", "U1"):
            same = [c for c, (p, q) in enumerate(zip(tb.tables.patterns, s13)) if tuple(p) == tuple(q)]
            assert len(same) == (13 if kind == "B" else 12) and torch.equal(r["hist"][:, same], ref["hist"][:, same]), name
        else:
            assert torch.equal(r["hist"], ref["hist"]) and torch.equal(r["line_mask"], ref["line_mask"]), name
        if e is eng:
            mine[kind] = r
        else:
            assert torch.equal(r["hist"], mine[kind]["hist"]) and torch.equal(r["line_mask"], mine[kind]["line_mask"]), name
    times = {k: [] for k in variants}
    rng = np.random.default_rng(0)
    for rnd in range(a.warmup + a.rounds):
        for k in rng.permutation(list(variants)):
            e, tb = variants[k]
            kw = {"tables": tb} if tb is not None else {}
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            e.log_scan_device(text, offd, validate=False, **kw)
            ev1.record()
            ev1.synchronize()
            if rnd >= a.warmup:
                times[k].append(ev0.elapsed_time(ev1) * 1e3)
    stat = {k: {"median_us": round(float(np.median(v)), 1), "p95_us": round(float(np.percentile(v, 95)), 1),
                "min_us": round(float(np.min(v)), 1), "n": len(v)} for k, v in times.items() if v}
    res = {"bench": "log scan: run-time pattern tables vs compiled-in matcher", "containers": a.containers,
           "lines": int(n_lines), "text_bytes": len(blob), "rounds": a.rounds, "warmup": a.warmup,
           "timing": "HIP events around one scan call (line arrays allocated inside), fresh random order per round",
           "variants": stat, "host_compile_s": compile_s, "corpus_gen_s": round(gen_s, 1),
           "tables": {"S13": {"nsym": tb13.tables.nsym, "nstate": tb13.tables.nstate, "lds_bytes": int(tb13.dev.numel())},
                      "B": {"nsym": tbB.tables.nsym, "nstate": tbB.tables.nstate, "lds_bytes": int(tbB.dev.numel())}},
           "library": native.library_info()}
    if stat:
        c = stat["compiled"]["median_us"]
        res["ratio_vs_compiled"] = {k: round(v["median_us"] / c, 4) for k, v in stat.items()}
        if a.parent_lib:  # this build over the parent's, pair by pair
            res["ratio_vs_parent"] = {k: round(stat[k]["median_us"] / stat[k.replace("compiled", "parent").replace("tables", "parent")]
                                               ["median_us"], 4) for k in stat if not k.startswith("parent")}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
