"""Log-template novelty on the device (csrc/template_novelty.hip) against the host
restatement (tests/template_novelty_ref.py), bit for bit: the counts, the report as a sorted set, the
per-container counts and the exported live records.  Synthetic template arrays go straight into the C
call; the wrapper, the real log path and the stream are checked on top."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import template_novelty_ref as R
from guarded import GuardedEngine, run_poisons
from krca import native, novelty, synth
from krca.agents.logs import pack_documents
from krca.rca import Config
from krca.stream import StreamingRCA

pytestmark = pytest.mark.gpu

ENOMEM = -12


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


def arrays(docs, gaps=0):
    """docs: per container a list of (hash, count) -> tmpl_hash u64, tmpl_count, n_templates, doc_line0."""
    th, tc, nt, d0 = [], [], [], []
    for ent in docs:
        d0.append(len(th))
        nt.append(len(ent))
        th += [h for h, _ in ent] + [0] * gaps
        tc += [c for _, c in ent] + [0] * gaps
    return (np.array(th, np.uint64), np.array(tc, np.int32), np.array(nt, np.int32), np.array(d0, np.int64))


def with_line(doc, line):
    return doc + ("" if not doc or doc.endswith("\n") else "\n") + line


class Table:
    """The C calls on one state, beside a restatement that sees the same windows."""

    def __init__(self, eng, capacity, ttl=0, ratio=4, smin=8):
        self.eng, self.lib, self.par = eng, eng.lib, (ttl, ratio, smin)
        self.ref = R.NoveltyRef(ttl, ratio, smin)
        self.state = self.alloc(capacity)
        assert self.lib.krca_template_novelty_init(eng.ptr(self.state), capacity, eng._stream()) == 0

    def alloc(self, capacity):
        return torch.empty(self.lib.krca_template_novelty_state_size(capacity), dtype=torch.uint8, device=self.eng.device)

    def call(self, th, tc, nt, d0, group, w, report=True, cap=4096, docs=True):
        """-> (rc, R.Window) of the device."""
        e = self.eng
        D = len(nt)
        dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).to(e.device)
               for a in (th, tc, nt, d0)]
        g = torch.from_numpy(np.asarray(group, np.int32)).to(e.device) if group is not None else None
        rep = torch.full((max(cap, 1) * 48,), 0x77, dtype=torch.uint8, device=e.device)
        dn = torch.full((max(D, 1),), -7, dtype=torch.int32, device=e.device)
        ds = torch.full((max(D, 1),), -7, dtype=torch.int32, device=e.device)
        counts = (ctypes.c_int64 * 6)()
        rc = self.lib.krca_template_novelty_update(
            e.ptr(self.state), e.ptr(dev[0]), e.ptr(dev[1]), len(th), e.ptr(dev[2]), e.ptr(dev[3]),
            e.ptr(g) if g is not None else None, D, w, *self.par, int(report), e.ptr(rep), cap,
            e.ptr(dn) if docs else None, e.ptr(ds) if docs else None, counts, e._stream())
        n = min(int(counts[4]), cap)
        recs = rep.cpu().numpy()[:n * 48].view(novelty.REPORT_DTYPE)
        assert (rep.cpu().numpy()[n * 48:] == 0x77).all()  # nothing past the records written
        report_ = sorted((int(r["hash"]), int(r["group"]), int(r["flags"]), int(r["cur_lines"]), int(r["cur_docs"]),
                          int(r["first_doc"]), int(r["first_win"]), int(r["total_before"])) for r in recs)
        return rc, R.Window(list(counts), report_, dn.cpu().numpy()[:D], ds.cpu().numpy()[:D])

    def records(self):
        return novelty.live_records(self.state.cpu().numpy())

    def window(self, th, tc, nt, d0, group, w, report=True):
        """One window on both sides, compared in full."""
        rc, got = self.call(th, tc, nt, d0, group, w, report)
        assert rc == 0, self.lib.krca_last_error()
        want = self.ref.update(th, tc, nt, d0, group, w, report)
        assert got.counts == want.counts
        assert got.report == want.report
        assert np.array_equal(got.doc_novel, want.doc_novel) and np.array_equal(got.doc_surge, want.doc_surge)
        assert self.records() == self.ref.records()
        return want

    def rehash(self, capacity, min_last=-(1 << 31)):
        new = self.alloc(capacity)
        rc = self.lib.krca_template_novelty_rehash(self.eng.ptr(self.state), self.eng.ptr(new), capacity, min_last,
                                                   self.eng._stream())
        if rc == 0:
            self.state = new
        return rc


H = [0x1000 + 977 * i for i in range(4000)]  # distinct hashes


def test_small_shapes(eng):
    t = Table(eng, 64)
    e = (np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert t.window(*e, None, 0).counts == [0] * 6  # ndocs = 0
    w = t.window(*arrays([[(H[0], 3)]]), None, 1)  # one container, one template
    assert w.counts == [1, 1, 1, 0, 1, 1] and w.report == [(H[0], 0, 1, 3, 1, 0, 1, 0)]
    # a container without templates between others, gaps in the doc_line0 ranges, counts of 0
    w = t.window(*arrays([[(H[0], 9), (H[1], 0)], [], [(H[1], 2), (H[2], 0), (H[3], 1)], []], gaps=3), None, 2)
    assert w.counts[:4] == [3, 3, 2, 0] and w.doc_novel.tolist() == [0, 0, 2, 0]
    # the same hash in two groups; then the same arrays with group = NULL
    g = [0, 5, 5, 0]
    w = t.window(*arrays([[(H[4], 1)], [(H[4], 2)], [(H[4], 4)], [(H[4], 8)]]), g, 3)
    assert w.report == [(H[4], 0, 1, 9, 2, 0, 3, 0), (H[4], 5, 1, 6, 2, 1, 3, 0)]
    w = t.window(*arrays([[(H[5], 1)], [(H[5], 2)], [(H[5], 4)], [(H[5], 8)]]), None, 4)
    assert w.report == [(H[5], 0, 1, 15, 4, 0, 4, 0)]
    # a negative group has no entries
    w = t.window(*arrays([[(H[6], 1)], [(H[7], 1)]]), [-1, 2], 5)
    assert w.counts[:3] == [1, 1, 1] and w.doc_novel.tolist() == [0, 1]


def test_empty_marker_and_hash_zero(eng):
    t = Table(eng, 64)
    w = t.window(*arrays([[(R.EMPTY_HASH, 1), (0, 2)], [(R.EMPTY_HASH - 1, 4)]]), None, 0)
    assert w.report == [(0, 0, 1, 2, 1, 0, 0, 0), (R.EMPTY_HASH - 1, 0, 1, 5, 2, 0, 0, 0)]
    assert t.records() == {(0, 0): (0, 0, 1, 2), (0, R.EMPTY_HASH - 1): (0, 0, 1, 5)}
    w = t.window(*arrays([[(R.EMPTY_HASH, 1)], [(0, 1)]]), [3, 3], 1)
    assert w.counts[2] == 2 and w.doc_novel.tolist() == [1, 1]


def test_contention_on_one_slot(eng):
    t = Table(eng, 128)
    w = t.window(*arrays([[(H[0], 2)]] * 5000), None, 0)
    assert w.report == [(H[0], 0, 1, 10000, 5000, 0, 0, 0)] and int(w.doc_novel.sum()) == 5000
    w = t.window(*arrays([[(H[0], 8)]] * 5000), None, 1)  # 40000 * 1 >= 4 * 10000
    assert w.report == [(H[0], 0, 2, 40000, 5000, 0, 0, 10000)] and int(w.doc_surge.sum()) == 5000


def test_probe_chain_wraps(eng):
    """70 keys whose home slot is slot 120 of a 128-slot table: the chain runs over the end."""
    keys, h = [], 1
    while len(keys) < 70:
        if novelty.home_slot(h, len(keys) % 3, 128) == 120:
            keys.append((h, len(keys) % 3))
        h += 1
    assert all(eng.lib.krca_template_novelty_home_slot(h, g, 128) == 120 for h, g in keys)
    t = Table(eng, 128)
    docs = [[(h, 1 + i)] for i, (h, _) in enumerate(keys)]
    w = t.window(*arrays(docs), [g for _, g in keys], 0)
    assert w.counts == [70, 70, 70, 0, 70, 70]
    _, slots = novelty.decode_state(t.state.cpu().numpy())
    used = np.flatnonzero(slots["group"] != novelty.EMPTY_GROUP)
    assert used.tolist() == list(range(0, 62)) + list(range(120, 128))
    w = t.window(*arrays(docs[::-1]), [g for _, g in keys][::-1], 1)
    assert w.counts[:3] == [70, 70, 0]


def test_capacity_64_overflow_rehash(eng):
    t = Table(eng, 64)
    first = [[(H[i], 1 + i % 3), (H[i + 1], 2)] for i in range(0, 64, 2)]
    assert t.window(*arrays(first), None, 0).counts == [64, 64, 64, 0, 64, 64]  # 64 distinct keys fit
    before = t.records()
    over = arrays([[(H[3], 50), (H[64], 1)], [(H[10], 20)], [(H[64], 2)]])
    rc, _ = t.call(*over, None, 1)
    assert rc == ENOMEM and b"full" in eng.lib.krca_last_error()
    assert t.records() == before == t.ref.records()
    _, slots = novelty.decode_state(t.state.cpu().numpy())
    assert (slots["cur"] == 0).all() and (slots["first_doc"] == np.iinfo(np.int32).max).all()  # rolled back
    assert t.rehash(32 * 2, 0) == 0 and t.records() == before  # the same size holds the 64 records
    assert t.rehash(128) == 0 and t.records() == before
    w = t.window(*over, None, 1)
    assert w.counts == [4, 3, 1, 2, 3, 65]
    # rehash with min_last_window drops exactly the older records (here: all but the three of window 1)
    assert t.rehash(128, 1) == 0
    t.ref.compact(1)
    assert t.records() == t.ref.records() and len(t.records()) == 3
    assert t.window(*arrays(first), None, 2).counts[2] == 62
    assert t.rehash(64, 3) == 0 and t.records() == {}
    big = Table(eng, 128)
    big.window(*arrays([[(H[i], 1)] for i in range(100)]), None, 0)
    small = big.alloc(64)
    assert eng.lib.krca_template_novelty_rehash(eng.ptr(big.state), eng.ptr(small), 64, 0, eng._stream()) == ENOMEM


def test_ttl_and_surge_boundary(eng):
    for ttl in (3, 0):
        t = Table(eng, 64, ttl=ttl, ratio=4, smin=8)
        t.window(*arrays([[(H[0], 5), (H[1], 10)]]), None, 0)
        w = t.window(*arrays([[(H[0], 5), (H[1], 40)]]), None, 3)  # last_win 0 >= 3 - 3: present; 40 * 3 >= 4 * 10
        assert w.report == [(H[1], 0, 2, 40, 1, 0, 0, 10)]
        w = t.window(*arrays([[(H[0], 5)]]), None, 7)  # 3 < 7 - 3: expired with ttl = 3
        assert w.report == ([(H[0], 0, 1, 5, 1, 0, 7, 0)] if ttl else [])
    t = Table(eng, 64)
    t.window(*arrays([[(H[0], 3), (H[1], 10), (H[2], 2)]]), None, 0)
    # equality surges; one line below does not; below surge_min does not
    w = t.window(*arrays([[(H[0], 12), (H[1], 39), (H[2], 7)]]), None, 1)
    assert w.report == [(H[0], 0, 2, 12, 1, 0, 0, 3)]
    w = t.window(*arrays([[(H[1], 98)], [(H[0], 29)]]), None, 2)  # 98 * 2 = 4 * 49; 29 * 2 < 4 * 15
    assert w.report == [(H[1], 0, 2, 98, 1, 0, 0, 49)]
    # products past 64 bits: 2^31 - 1 lines in each of 300 containers, ratio 1, far-apart windows
    t = Table(eng, 64, ratio=1, smin=1)
    many = arrays([[(H[0], (1 << 31) - 1)]] * 300)
    t.window(*many, None, 0)
    assert t.window(*many, None, (1 << 31) - 2).counts[3] == 1


def test_learn_only_and_report_cap(eng):
    t = Table(eng, 256)
    docs = [[(H[i], 1 + i)] for i in range(40)]
    w = t.window(*arrays(docs), None, 0, report=False)
    assert w.counts == [40, 40, 0, 0, 0, 40] and not w.doc_novel.any()
    assert t.window(*arrays(docs), None, 1).counts[2:5] == [0, 0, 0]  # learnt
    fresh = arrays([[(H[100 + i], 1 + i)] for i in range(10)])
    rc, got = t.call(*fresh, None, 2, cap=3)
    want = t.ref.update(*fresh, None, 2)
    assert rc == 0 and got.counts == want.counts and got.counts[4] == 10
    assert len(got.report) == 3 and len(set(got.report)) == 3 and set(got.report) <= set(want.report)
    assert np.array_equal(got.doc_novel, want.doc_novel) and t.records() == t.ref.records()
    rc, got = t.call(*arrays([[(H[200], 1)]]), None, 3, cap=0, docs=False)  # no report buffer use, no doc_*
    assert rc == 0 and got.counts[2:5] == [1, 0, 1] and (got.doc_novel == -7).all()
    t.ref.update(*arrays([[(H[200], 1)]]), None, 3)
    assert t.records() == t.ref.records()


@pytest.mark.parametrize("D", [63, 64, 65, 257])
def test_walk_boundaries(eng, D):
    """Container counts around the wave and the workgroup; templates per container around the lane
    walk's limit (8) and one container of 3 000 templates for the wave's walk."""
    rng = np.random.default_rng(D)
    docs = [[(H[int(k)], int(c)) for k, c in zip(rng.choice(200, n, replace=False), rng.integers(0, 5, n))]
            for n in rng.integers(0, 12, D)]
    docs[D // 2] = [(H[i], 1 + i % 4) for i in range(3000)]
    docs[-1] = [(H[i], 2) for i in range(9)]
    t = Table(eng, 16384)  # the long container lands in up to three groups: 9 000 keys
    g = rng.integers(0, 3, D).astype(np.int32)
    for w in range(3):
        t.window(*arrays(docs if w != 1 else docs[::-1], gaps=w), g, w)


def test_zipf_stream_grows_through_the_wrapper(eng):
    """Six windows of 4 097 containers over a Zipf pool of 3 000 templates in 8 groups, some containers
    silent, through TemplateNovelty from capacity 1 024: the table grows mid-stream."""
    rng = np.random.default_rng(5)
    D = 4097
    group = rng.integers(0, 8, D).astype(np.int32)
    nov = novelty.TemplateNovelty(eng, capacity=1024, report_cap=1 << 15)
    ref = R.NoveltyRef()
    gd = torch.from_numpy(group).cuda()
    grown = []
    for w in range(6):
        docs = []
        for d in range(D):
            if rng.random() < 0.2:
                docs.append([])
                continue
            ks = np.unique(np.minimum(rng.zipf(1.3, rng.integers(1, 6)), 3000) - 1)
            docs.append([(H[int(k)], int(rng.integers(1, 30))) for k in ks])
        th, tc, nt, d0 = arrays(docs)
        tm = dict(tmpl_hash=torch.from_numpy(th.view(np.int64)).cuda(), tmpl_count=torch.from_numpy(tc).cuda(),
                  n_templates=torch.from_numpy(nt).cuda())
        rep = nov.update(tm, torch.from_numpy(d0).cuda(), group=gd, report=w >= 1)
        want = ref.update(th, tc, nt, d0, group, w, report=w >= 1)
        grown += rep.grown
        assert [rep.counts[k] for k in novelty.COUNT_NAMES] == want.counts and rep.window == w
        got = sorted((r.hash, r.group, r.flags, r.cur_lines, r.cur_docs, r.first_doc, r.first_win, r.total_before)
                     for r in rep.novel + rep.surged)
        assert got == want.report and not rep.truncated
        assert [r.cur_lines for r in rep.novel] == sorted((r.cur_lines for r in rep.novel), reverse=True)
        assert np.array_equal(rep.doc_novel.cpu().numpy(), want.doc_novel)
        assert np.array_equal(rep.doc_surge.cpu().numpy(), want.doc_surge)
        assert nov.records() == ref.records()
        if w == 5:
            top = rep.top_containers(5)
            both = want.doc_novel.astype(np.int64) + want.doc_surge
            assert [d for d, _, _ in top] == sorted(range(D), key=lambda d: (-both[d], d))[:len(top)]
    assert grown and nov.capacity > 1024 and nov.capacity == grown[-1]
    with pytest.raises(ValueError):
        nov.update(tm, torch.from_numpy(d0).cuda(), group=gd, window=5)


def _window_of(keys):
    return arrays([[(H[k], 3)] for k in keys])


def _wrapped(rep):
    return ([rep.counts[k] for k in novelty.COUNT_NAMES],
            sorted((r.hash, r.group, r.flags, r.cur_lines, r.cur_docs, r.first_doc, r.first_win, r.total_before)
                   for r in rep.novel + rep.surged))


def _feed(nov, a, window):
    th, tc, nt, d0 = a
    tm = dict(tmpl_hash=torch.from_numpy(th.view(np.int64)).cuda(), tmpl_count=torch.from_numpy(tc).cuda(),
              n_templates=torch.from_numpy(nt).cuda())
    return nov.update(tm, torch.from_numpy(d0).cuda(), window=window)


def test_growth_with_ttl(eng):
    """ttl > 0: the compaction at the same size leaves the table at most half full, yet the live records
    plus the window's new keys exceed it -- the repeated window fails again and the table must double."""
    nov = novelty.TemplateNovelty(eng, capacity=1024, ttl=5)
    ref = R.NoveltyRef(ttl=5)
    a = _window_of(range(400))
    rep = _feed(nov, a, 0)
    want = ref.update(*a, None, 0)
    assert _wrapped(rep) == (want.counts, want.report) and rep.grown == ()
    b = _window_of(range(390, 1100))  # 10 known keys, 700 new: 400 + 700 > 1024
    rep = _feed(nov, b, 1)
    want = ref.update(*b, None, 1)
    assert rep.grown == (1024, 2048) and nov.capacity == 2048
    assert _wrapped(rep) == (want.counts, want.report) and nov.records() == ref.records()
    # expiry makes the room: 40 keys, then 40 others after the ttl ran out, in 64 slots
    nov = novelty.TemplateNovelty(eng, capacity=64, ttl=2)
    ref = R.NoveltyRef(ttl=2)
    for w, keys in ((0, range(40)), (5, range(100, 140))):
        a = _window_of(keys)
        rep = _feed(nov, a, w)
        want = ref.update(*a, None, w)
        if rep.grown:
            ref.compact(w - 2)
            want.counts[5] = len(ref.records())
        assert _wrapped(rep) == (want.counts, want.report) and nov.records() == ref.records()
    assert rep.grown == (64,) and nov.capacity == 64 and len(nov.records()) == 40
    # above 70 % load after a window that fitted: room is made before the next one
    nov = novelty.TemplateNovelty(eng, capacity=64)
    rep = _feed(nov, _window_of(range(50)), 0)
    assert rep.grown == (128,) and nov.capacity == 128 and rep.counts["n_live_slots"] == 50 and len(nov.records()) == 50
    assert _feed(nov, _window_of(range(44)), 1).grown == ()


def test_real_log_path(eng):
    """Text -> log scan -> template histograms -> update, against the restatement fed from
    oracle.template_hist."""
    nov = novelty.TemplateNovelty(eng, capacity=256)
    ref = R.NoveltyRef()
    for w in range(3):
        docs = synth.make_log_corpus(150, lines_per_doc=3, seed=40 + w)
        if w == 2:
            docs[77] = with_line(docs[77], "FATAL disk quota exceeded on volume data-7 for tenant acme")
        blob, off = pack_documents(docs)
        scan = eng.log_scan_device(eng.upload_blob(blob), torch.from_numpy(off).cuda())
        scan["templates"] = eng.template_hist_device(scan)
        rep = nov.update(scan["templates"], scan["doc_line0"])
        hists = [oracle.template_hist(t) for t in docs]
        want = ref.update(*arrays(hists), None, w)
        assert [rep.counts[k] for k in novelty.COUNT_NAMES] == want.counts
        got = sorted((r.hash, r.group, r.flags, r.cur_lines, r.cur_docs, r.first_doc, r.first_win, r.total_before)
                     for r in rep.novel + rep.surged)
        assert got == want.report and nov.records() == ref.records()
        assert np.array_equal(rep.doc_novel.cpu().numpy(), want.doc_novel)
    mine = [r for r in rep.novel if r.first_doc == 77]
    assert any(nov.example(r, scan) == "FATAL disk quota exceeded on volume data-7 for tenant acme" for r in mine)


def test_poisons_and_guard_band():
    """The report buffer, doc_* and the state before init under the three poisons, inside a guard band."""
    geng = GuardedEngine()
    w0 = arrays([[(H[i], 1 + i % 5) for i in range(d % 7)] for d in range(100)])
    w1 = arrays([[(H[i + 2], 9) for i in range(d % 11)] for d in range(100)], gaps=1)

    def call(e):
        nov = novelty.TemplateNovelty(e, capacity=64, report_cap=8)
        out = {}
        for w, (th, tc, nt, d0) in enumerate((w0, w1)):
            tm = dict(tmpl_hash=e._dev(th.view(np.int64)), tmpl_count=e._dev(tc), n_templates=e._dev(nt))
            rep = nov.update(tm, e._dev(d0))
            out[f"counts{w}"] = np.array([rep.counts[k] for k in novelty.COUNT_NAMES])
            out[f"doc_novel{w}"], out[f"doc_surge{w}"] = rep.doc_novel.cpu().numpy(), rep.doc_surge.cpu().numpy()
            out[f"n_records{w}"] = np.array([len(rep.novel), len(rep.surged)])
        recs = nov.records()
        out["records"] = np.array(sorted(k + v for k, v in recs.items()), np.uint64)
        return out

    base = run_poisons(geng, call)
    ref = R.NoveltyRef()
    for w, a in enumerate((w0, w1)):
        want = ref.update(*a, None, w)
        assert base[f"counts{w}"].tolist() == want.counts
        assert np.array_equal(base[f"doc_novel{w}"], want.doc_novel) and np.array_equal(base[f"doc_surge{w}"], want.doc_surge)
    assert base["records"].tolist() == sorted(list(k + v) for k, v in ref.records().items())


def test_stream_end_to_end(eng, tmp_path):
    """StreamingRCA(novelty=True, novelty_warmup=2) on a 64-pod mesh, three windows of log text; the
    third adds one new error line in one container."""
    P, M, W = 64, 4, 20
    m = synth.make_graph(P, avg_degree=4, seed=2)
    x = synth.make_metrics(P, M, W + 30, window=W, seed=3, roots=m.roots).numpy()
    xd = torch.from_numpy(x).cuda()
    docs = synth.make_log_corpus(P, lines_per_doc=4, seed=9)
    line = "PANIC replication lag exceeded on shard orders-eu for leader node-b"
    third = list(docs)
    third[41] = with_line(docs[41], line)
    cuts = [(0, W + 10), (W + 10, W + 20), (W + 20, W + 30)]

    def make():
        return StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, Config(window=W), tol=1e-9, max_iter=60, novelty=True,
                            novelty_warmup=2)

    def run(s, i):
        blob, off = pack_documents(third if i == 2 else docs)
        lo, hi = cuts[i]
        return s.window(xd[lo:hi].contiguous(), eng.upload_blob(blob), torch.from_numpy(off).cuda())

    s = make()
    for i in range(2):
        rep = run(s, i)["logs"]["novelty"]
        assert rep.novel == [] and rep.surged == [] and rep.counts["n_novel"] == 0 and rep.counts["n_entries"] > 0
    path = str(tmp_path / "s.npz")
    s.snapshot(path)
    out = run(s, 2)
    rep = out["logs"]["novelty"]
    assert len(rep.novel) == 1 and rep.surged == [] and rep.window == 2
    r = rep.novel[0]
    assert (r.first_doc, r.cur_docs, r.cur_lines, r.first_win, r.total_before) == (41, 1, 1, 2, 0)
    assert r.hash == novelty.remap(oracle.fnv1a64(oracle.template_of(line.encode())))
    assert s.novelty.example(r, out["logs"]) == line
    dn = rep.doc_novel.cpu().numpy()
    assert dn[41] == 1 and dn.sum() == 1 and not rep.doc_surge.any()
    assert rep.top_containers(3) == [(41, 1, 0)]
    with np.load(path, allow_pickle=False) as z:
        assert {"novelty_slots", "novelty_index", "novelty_header", "novelty_meta"} <= set(z.files)
        assert len(z["novelty_index"]) == rep.counts["n_live_slots"] - 1 and z["novelty_slots"].shape[1] == 64
    s2 = make()
    s2.restore(path)
    out2 = run(s2, 2)
    rep2 = out2["logs"]["novelty"]
    assert rep2.novel == rep.novel and rep2.counts == rep.counts
    assert np.array_equal(rep2.doc_novel.cpu().numpy(), dn)
    assert s2.novelty.records() == s.novelty.records()
    a, b = s.novelty.state_dict(), s2.novelty.state_dict()
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)  # equal tables, equal bytes
    assert [int(v) for v in out2["top"][0]] == [int(v) for v in out["top"][0]]
    plain = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, Config(window=W), tol=1e-9, max_iter=60)
    with pytest.raises(ValueError, match="novelty"):
        plain.restore(path)
    o = plain.window(xd[:W + 10].contiguous(), eng.upload_blob(pack_documents(docs)[0]),
                     torch.from_numpy(pack_documents(docs)[1]).cuda())
    assert "novelty" not in o["logs"]
    # per service: container_group makes a template new once per group
    group = (np.arange(P) % 4).astype(np.int32)
    by = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, Config(window=W), tol=1e-9, max_iter=60,
                      novelty=dict(capacity=4096), container_group=group)
    rep = run(by, 0)["logs"]["novelty"]
    want = R.NoveltyRef().update(*arrays([oracle.template_hist(t) for t in docs]), group, 0)
    assert [rep.counts[k] for k in novelty.COUNT_NAMES] == want.counts and rep.counts["n_novel"] > 0
    assert np.array_equal(rep.doc_novel.cpu().numpy(), want.doc_novel) and by.novelty.capacity == 4096
