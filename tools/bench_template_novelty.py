#!/usr/bin/env python3
"""Template-novelty bench: krca_template_novelty_update on a C5-sized log window (1 M containers, about
2.5 M lines; krca.synth.make_log_corpus for --corpus-docs containers, tiled to --docs), next to the
template pass it follows (krca_template_hash + krca_template_hist on the same window, in this process)
and to the host restatement (tests/template_novelty_ref.py: the read-back of the four template arrays
and the dict merge).

  python tools/bench_template_novelty.py [--docs 1000000] [--out profiles/r16/template_novelty.json]

Cases, HIP events around whole calls (a call includes its one read-back), 5 warm-ups + 20 calls, median:
  learn     the window into an empty table (every key is new; report off, as a warm-up window)
  steady    the same window again and again (every key known; report on, per-container counts on)
  steady_nodocs  the same without the per-container pass
  planted   steady, with one line's template replaced by one never seen (a new hash per call)
  rehash    the learned table into one of twice the capacity
  pool      synthetic arrays instead of text: --docs containers drawing 1-4 templates from a Zipf pool of
            --pool templates in --groups groups (a table with many more keys than the text's pool)
Needs an MI355X; there is no CPU fallback.
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


def zipf_window(rng, docs, pool, groups):
    """-> host arrays tmpl_hash u64, tmpl_count, n_templates, doc_line0, group of a synthetic window."""
    nt = rng.integers(1, 5, docs).astype(np.int32)
    d0 = np.zeros(docs, np.int64)
    np.cumsum(nt[:-1], out=d0[1:])
    L = int(nt.sum())
    ids = np.minimum(rng.zipf(1.2, L), pool).astype(np.uint64)
    # distinct inside a container: the j-th template of a container is shifted into the j-th quarter of the hash space
    j = (np.arange(L) - np.repeat(d0, nt)).astype(np.uint64)
    th = (ids * np.uint64(0x9E3779B97F4A7C15)) ^ (j << np.uint64(62))
    tc = rng.integers(1, 6, L).astype(np.int32)
    return th, tc, nt, d0, rng.integers(0, groups, docs).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--corpus-docs", type=int, default=50_000)
    ap.add_argument("--lines-per-doc", type=float, default=2.5)
    ap.add_argument("--pool", type=int, default=200_000)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--ref-max-lines", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "template_novelty.json"))
    a = ap.parse_args()
    import torch
    import template_novelty_ref as R
    from krca import native, novelty, synth
    from krca.agents.logs import pack_documents
    eng = native.NativeEngine(0)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms):
        return {"median_ms": float(np.median(ms)), "p95_ms": float(np.percentile(ms, 95)), "runs": len(ms)}

    def cases(name, tm, d0, group, extra):
        D, L = int(d0.numel()), int(tm["tmpl_hash"].numel())
        r = dict(extra, case=name, containers=D, line_slots=L, capacity=a.capacity, grouped=group is not None)
        ms = []
        for _ in range(a.warmup + a.runs):  # an empty table per call; its allocation and init are not timed
            nov = novelty.TemplateNovelty(eng, capacity=a.capacity)
            torch.cuda.synchronize()
            ms.append(event_ms(lambda: nov.update(tm, d0, group=group, report=False)))
        r["learn"] = stats(ms[a.warmup:])
        rep = nov.update(tm, d0, group=group)
        r["counts_steady"] = rep.counts
        r["table_bytes"] = int(nov.state.numel())
        r["steady"] = timed(torch, lambda: nov.update(tm, d0, group=group), a.warmup, a.runs)
        r["steady_nodocs"] = timed(torch, lambda: nov.update(tm, d0, group=group, docs=False), a.warmup, a.runs)
        th2 = tm["tmpl_hash"].clone()
        tm2 = dict(tm, tmpl_hash=th2)
        at = int(d0[D // 2].item())
        fresh = [0x7777000000000000]

        def planted():
            fresh[0] += 1
            th2[at] = fresh[0]
            return nov.update(tm2, d0, group=group)
        r["planted"] = timed(torch, planted, a.warmup, a.runs)
        p = planted()
        r["planted_report"] = {"n_novel": p.counts["n_novel"], "first_doc": p.novel[0].first_doc if p.novel else None,
                               "expected_doc": D // 2}
        ms = []
        for _ in range(5):
            cap = nov.capacity
            ms.append(event_ms(lambda: nov.rehash(2 * cap)))
            nov.rehash(cap)
        r["rehash_to_twice"] = stats(ms)
        if L <= a.ref_max_lines:
            t0 = time.perf_counter()
            arrs = [tm[k].cpu().numpy() for k in ("tmpl_hash", "tmpl_count", "n_templates")] + [d0.cpu().numpy()]
            gh = group.cpu().numpy() if group is not None else None
            t1 = time.perf_counter()
            ref = R.NoveltyRef()
            want = ref.update(*arrs, gh, 0)
            t2 = time.perf_counter()
            r["host_restatement"] = {"read_back_s": t1 - t0, "merge_s": t2 - t1}
            one = novelty.TemplateNovelty(eng, capacity=a.capacity)
            got = one.update(tm, d0, group=group)
            r["matches_restatement"] = bool([got.counts[k] for k in novelty.COUNT_NAMES] == want.counts and
                                            np.array_equal(got.doc_novel.cpu().numpy(), want.doc_novel) and
                                            one.records() == ref.records())
        print(json.dumps(r), flush=True)
        return r

    results = []
    # the text window: the corpus tiled to --docs containers
    t0 = time.perf_counter()
    docs = synth.make_log_corpus(a.corpus_docs, lines_per_doc=a.lines_per_doc, seed=1, hazard_rate=0.001)
    blob1, off1 = pack_documents(docs)
    reps = max(a.docs // a.corpus_docs, 1)
    blob = blob1 * reps
    off = np.concatenate([off1[:-1] + i * len(blob1) for i in range(reps)] + [np.array([reps * len(blob1)], np.int64)])
    print(f"# {len(off) - 1} containers, {len(blob)} bytes of log text built in {time.perf_counter() - t0:.1f} s", flush=True)
    text, offd = eng.upload_blob(blob), torch.from_numpy(off).to(eng.device)
    scan = eng.log_scan_device(text, offd)
    tm = eng.template_hist_device(scan)
    tmpl = timed(torch, lambda: eng.template_hist_device(scan), a.warmup, a.runs)
    n_lines = int(scan["n_lines_total"])
    extra = {"source": "text", "lines": n_lines, "template_pass": tmpl}
    r = cases("c5_text", tm, scan["doc_line0"], None, extra)
    r["update_over_template_pass"] = r["steady"]["median_ms"] / tmpl["median_ms"]
    results.append(r)
    svc = torch.from_numpy((np.arange(len(off) - 1) % 5000).astype(np.int32)).to(eng.device)
    r = cases("c5_text_by_service", tm, scan["doc_line0"], svc, extra)
    r["update_over_template_pass"] = r["steady"]["median_ms"] / tmpl["median_ms"]
    results.append(r)
    del text, scan, tm
    torch.cuda.empty_cache()
    # synthetic arrays over a large pool
    th, tc, nt, d0, g = zipf_window(np.random.default_rng(2), a.docs, a.pool, a.groups)
    tm = dict(tmpl_hash=torch.from_numpy(th.view(np.int64)).to(eng.device), tmpl_count=torch.from_numpy(tc).to(eng.device),
              n_templates=torch.from_numpy(nt).to(eng.device))
    results.append(cases("zipf_pool", tm, torch.from_numpy(d0).to(eng.device), torch.from_numpy(g).to(eng.device),
                         {"source": "synthetic", "pool": a.pool, "groups": a.groups}))
    out = {"device": torch.cuda.get_device_name(0), "library": native.library_info(), "warmup": a.warmup,
           "timing": "HIP events around a whole call (kernels and the call's one read-back)", "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
