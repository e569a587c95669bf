"""Log scan with pattern tables compiled at run time (krca_log_scan_tables / krca_log_match_tables,
NativeEngine.log_tables, LogsAgent(compile_patterns=True)) on an MI355X.

Expected values: the compiled-in path for the 13 shipped patterns (byte-equal arrays), Python's
``re`` per line for every other set (the reference's definition, computed here), and
tests/golden/logs_custom_patterns.json (captured from the reference)."""
import ctypes
import struct

import numpy as np
import pytest

import agent_cases as A
import custom_pattern_sets as S
from guarded import GuardedEngine, run_poisons
from krca import logdfa, native, synth
from krca.agents.logs import pack_documents

pytestmark = pytest.mark.gpu

KEYS = ("line_start", "line_end", "line_mask", "doc_lines", "doc_line0", "hist", "examples")


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


def one_call(e, blob, off, tables=None):
    """log_scan_device with the dense example table (host copies): the one call, and the match call
    over the index it left when the engine's line arrays were too small."""
    r = e.log_scan_device(e.upload_blob(blob), e._dev(np.asarray(off, np.int64)), dense_examples=True, tables=tables)
    return {k: r[k].cpu().numpy() for k in KEYS}


def two_calls(e, blob, off, tables):
    """krca_log_index, then krca_log_match_tables (tables None: krca_log_match, the compiled-in
    patterns) into line arrays of exactly the line count."""
    t = e.torch
    text, offd = e.upload_blob(blob), e._dev(np.asarray(off, np.int64))
    nbytes, D, nc = len(blob), len(off) - 1, tables.ncat if tables is not None else native.NCAT
    ws = e._workspace("logidx", 8 * e.lib.krca_log_index_size(nbytes))
    nl = t.empty(1, dtype=t.int64, device=e.device)
    native._check(e.lib.krca_log_index(e.ptr(text), nbytes, e.ptr(offd), D, e.ptr(ws), e.ptr(nl), e._stream()),
                  "krca_log_index")
    L = int(nl.item())
    new = lambda dt, *shape: t.empty(shape, dtype=dt, device=e.device)  # noqa: E731
    r = dict(line_start=new(t.int64, L), line_end=new(t.int64, L), line_mask=new(t.int32, L), doc_lines=new(t.int32, D),
             doc_line0=new(t.int64, D), hist=new(t.int32, D, nc), examples=new(t.int32, D, nc, 3))
    out = (L, e.ptr(r["line_start"]), e.ptr(r["line_end"]), e.ptr(r["line_mask"]), e.ptr(r["doc_lines"]), e.ptr(r["hist"]),
           e.ptr(r["examples"]), e.ptr(r["doc_line0"]), e._stream())
    if tables is None:
        native._check(e.lib.krca_log_match(e.ptr(text), nbytes, e.ptr(offd), D, e.ptr(ws), *out), "krca_log_match")
    else:
        native._check(e.lib.krca_log_match_tables(
            e.ptr(text), nbytes, e.ptr(offd), D, e.ptr(ws), e.ptr(tables.dev), tables.dev.numel(), ctypes.byref(tables.dims),
            *out), "krca_log_match_tables")
    return {k: r[k].cpu().numpy().copy() for k in KEYS}


def check_docs(e, pats, docs, tables=None):
    """n_lines, hist and the example lines of every container equal re's."""
    tables = tables or e.log_tables(pats)
    scan = e.log_scan(*pack_documents(docs), tables=tables)
    assert scan.hist.shape == (len(docs), len(pats))
    for d, text in enumerate(docs):
        n, h, ex = S.re_hist(pats, text)
        assert scan.n_lines[d] == n, (d, repr(text[:80]))
        assert scan.hist[d].tolist() == h, (d, repr(text[:120]))
        for c in range(len(pats)):
            assert scan.examples(d, c) == ex[c], (d, c)


# ---- the 13 shipped patterns: run-time tables against the compiled-in walk -------------------------
def _golden_docs():
    return [c["text"] for c in A.load("logs_corpus.json")["containers"]]


@pytest.mark.parametrize("corpus", ["golden", "synth"])
def test_s13_runtime_tables_byte_equal_to_compiled_path(eng, corpus):
    docs = _golden_docs() if corpus == "golden" else \
        synth.make_log_corpus(3000, lines_per_doc=4, seed=5, hazard_rate=0.02) + ["x" * 3000 + " Killed " + "é" * 900]
    blob, off = pack_documents(docs)
    tb = eng.log_tables(S.S13)
    assert eng.log_tables(list(S.S13)) is tb  # cached by digest
    want = one_call(eng, blob, off)
    fresh = native.NativeEngine()  # line capacity 1024: the one call falls back to the match call
    for got in (one_call(eng, blob, off, tb), two_calls(eng, blob, off, tb), one_call(fresh, blob, off, fresh.log_tables(S.S13))):
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert len(want["line_start"]) > 1024 and want["hist"].sum() > 0


# ---- edited sets against re ----------------------------------------------------------------------------
def _tile_docs(lits):
    """Containers placed so that one starts exactly on the 64 KiB tile boundary, the text crossing it
    with pattern halves on both sides."""
    a, b = lits[0], lits[-1]
    first = "f" * 100 + "\n" + a + "\n"
    fill = 65536 - len(first.encode()) - len(a[:3].encode())
    return [first + "g" * (fill - 1) + " " + a[:3], a[3:] + " tail\n" + b + "\r\n" + b[:2], b[2:] + "\n" + a]


def _edge_docs(lits):
    """The shape of test_log_scan_block_edges: lines starting at every offset mod 16 with 2-, 3- and
    4-byte code points straddling block and word edges, matches ending at every offset."""
    docs = []
    for k in range(20):
        for i, cp in enumerate(("\u00e9", "\u20ac", "\U0001d400", "\u212a", "\u017f", "\u0663")):
            lit = lits[(k + i) % len(lits)]
            docs.append("a" * k + cp + lit + "\n" + "b" * (k % 7) + lits[(k * 7 + i) % len(lits)] + cp * 3)
        docs.append("c" * k + lits[k % len(lits)])
    return docs


def _end_docs(lits):
    """Pattern halves meeting across a container end without a trailing separator, at every offset
    mod 16, and at the text's last bytes."""
    docs = []
    for pad in range(16):
        for j in range(3):
            lit = lits[(pad * 3 + j) % len(lits)]
            cut = max(1, len(lit) - 1 - j)
            docs += ["p" * pad + " x " + lit[:cut], lit[cut:] + " y"]
    docs.append("tail " + lits[0][:-1])  # the text's last bytes: one short of a match
    return docs


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_edited_sets_equal_re(eng, name):
    """B needs 64 columns (36 symbols) and 543 states (139 KB as 32-bit entries); C has 3 categories, B 16,
    D 12, E 5: output strides other than 13."""
    pats = S.SETS[name]
    lits = S.literals(pats)
    tb = eng.log_tables(pats)
    assert tb.ncat == len(pats)
    docs = _tile_docs(lits) + S.fragment_fuzz(pats, 300, seed=21) + _edge_docs(lits) + _end_docs(lits)
    assert len(docs[0].encode()) == 65536  # the second container starts on the tile boundary
    check_docs(eng, pats, docs, tb)
    for tail in (0, 1, 7, 15, 16):  # texts ending at several offsets mod 16
        check_docs(eng, pats, ["z" * 11 + "\n" + lits[0] * 2 + "q" * tail], tb)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_golden_line_masks(eng, name):
    g = A.load("logs_custom_patterns.json")["sets"][name]
    pats = [tuple(p) for p in g["patterns"]]
    assert pats == S.SETS[name]
    docs = [c["text"] for c in g["containers"]]
    blob, off = pack_documents(docs)
    r = one_call(eng, blob, off, eng.log_tables(pats))
    masks = (r["line_mask"].view(np.uint32) & 0xFFFF).tolist()
    assert masks == [m for c in g["containers"] for m in c["masks"]]
    assert np.array_equal(r["examples"], native.example_ids(r["line_mask"], r["doc_line0"], r["doc_lines"], len(pats)))


# ---- the histogram kernel: one for every category count -------------------------------------------------
HIST_SIZES = (0, 1, 32, 33, 64, 65, 200)   # lines: none; one; the lane loop's last size and the wave path's first;
#                                            one 64-line round, one line past it, several rounds
HIST_SPOTS = (0, 63, 64, 255, 256, 299)    # block lanes 0, 63, 64 and 255; the second block's first; the last container


def _hist_docs(lits_by_cat, rot):
    """300 containers (a full 256-lane block and one of 44).  Container HIST_SPOTS[p] holds
    HIST_SIZES[(p + rot) % 7] lines, so the seven rotations put every size at every spot; the others hold
    1-3 lines.  A container of 32 lines or more matches category a on every third line and b on every
    fourth (both more than three times: the example tables fill up, some lines carry both) and, at 200
    lines, a third on lines 40, 90, 140 and 190 (its examples come from three 64-line rounds)."""
    rng = np.random.default_rng(100 + rot)
    nc = len(lits_by_cat)
    docs = []
    for d in range(300):
        if d in HIST_SPOTS:
            p = HIST_SPOTS.index(d)
            n, a = HIST_SIZES[(p + rot) % 7], (3 * p + rot) % nc  # (every size meets low and high categories)
            lines = []
            for i in range(n):
                ln = "l%d" % i
                if i % 3 == 1:
                    ln += " " + lits_by_cat[a]
                if i % 4 == 2:
                    ln += " " + lits_by_cat[(a + 1) % nc]
                if nc > 3 and i % 50 == 40:
                    ln += " " + lits_by_cat[(a + 3) % nc]
                lines.append(ln)
        else:
            lines = [("s%d " % d) + (lits_by_cat[int(rng.integers(nc))] if rng.random() < 0.5 else "quiet")
                     for _ in range(int(rng.integers(1, 4)))]
        docs.append("\n".join(lines) + ("\n" if d % 2 and lines else ""))
    return docs


@pytest.mark.parametrize("name", ["S13", "C", "B"])
def test_hist_every_container_size_at_every_block_position(eng, name):
    """log_hist<DENSE, Cats> with the category count compiled in (S13 through krca_log_scan /
    krca_log_match) and as an argument (C: 3, B: 16), dense example table, through the one-call scan and
    through index + match: doc_lines, counts and the three example lines of every container equal re's,
    and the example bits of the line masks give the same table."""
    pats = S.SETS[name]
    nc = len(pats)
    tb = None if name == "S13" else eng.log_tables(pats)
    lits = iter(S.literals(pats))  # one per alternative, in pattern order: each category's first
    lits_by_cat = [[next(lits) for _ in logdfa.parse(cat, rx)][0] for cat, rx in pats]
    eng._log_cap = max(eng._log_cap, 4096)  # the one call is not to fall back to the match call
    for rot in range(7):
        docs = _hist_docs(lits_by_cat, rot)
        want = [S.re_hist(pats, text) for text in docs]
        for d, n in zip(HIST_SPOTS, (HIST_SIZES[(p + rot) % 7] for p in range(6))):
            assert want[d][0] == n
            if n >= 32:  # more than three matching lines in two categories or more, none in another
                assert sum(h > 3 for h in want[d][1]) >= 2 and min(want[d][1]) == 0, (rot, d, want[d][1])
        blob, off = pack_documents(docs)
        for got in (one_call(eng, blob, off, tb), two_calls(eng, blob, off, tb)):
            assert got["hist"].shape == (300, nc) and got["examples"].shape == (300, nc, 3)
            assert got["doc_lines"].tolist() == [w[0] for w in want]
            assert got["hist"].tolist() == [w[1] for w in want]
            text_of = [bytes(blob[s:e]).decode() for s, e in zip(got["line_start"].tolist(), got["line_end"].tolist())]
            for d in range(300):
                for c in range(nc):
                    ids = [i for i in got["examples"][d, c].tolist() if i >= 0]
                    assert [text_of[i] for i in ids] == want[d][2][c], (rot, d, c)
                    assert got["examples"][d, c].tolist() == ids + [-1] * (3 - len(ids)), (rot, d, c)
            assert np.array_equal(got["examples"],
                                  native.example_ids(got["line_mask"], got["doc_line0"], got["doc_lines"], nc))


# ---- long lines: the warm-up is the set's, not the compiled walk's 23 ------------------------------------
def _long_line(nbytes, k, alt, filler, back):
    """A line of about nbytes bytes (filler code points of one width) in which `alt` starts `back` of its
    own code points before one of the wave-per-line kernel's segment boundaries: the k-th of 64 when the
    line is long enough for `alt` to fit after it (always at 8000 bytes), else k folded onto those that are."""
    w, ab = len(filler.encode()), len(alt.encode())
    n_fill = (nbytes - ab) // w
    total = n_fill * w + ab
    seg = (total + 63) // 64
    k = 1 + (k - 1) % ((total - ab) // seg)
    before = max(0, -(-(k * seg - len(alt[:back].encode())) // w))  # rounded up: code point `back` is past the boundary
    return filler * before + alt + filler * (n_fill - before)


@pytest.mark.parametrize("multibyte", [False, True])
def test_long_lines_longest_alternative_across_every_segment_boundary(eng, multibyte):
    """Lines of 1025 to 8000 bytes go to log_dfa_long (a wave per line, 64 segments).  The 40 code
    point alternative is placed to straddle each of the 63 inner segment boundaries in turn (8000-byte
    lines; shorter ones fold the boundary index), starting 39, 30 and 2 code points before it: a segment
    warmed up over only 23 code points misses the first two."""
    alt = "abcdefghij" * 4
    pats = S.LONG40
    if multibyte:  # a 2- and a 3-byte code point inside the alternative, 2-byte fillers around it
        alt = "abcdefghij" + "\u00e9" + "bcdefghij" + "a\u20accdefghij" + "abcdefghij"
        pats = [("long40", "(" + alt + "|zq)"), S.LONG40[1]]
    tb = eng.log_tables(pats)
    assert tb.tables.warm == 39 and len(alt) == 40
    lines = []
    for k in range(1, 64):
        fill = "\u00e9" if multibyte and k % 2 else "x"
        lines.append(_long_line(8000, k, alt, fill, 39))
        lines.append(_long_line((1025, 2000, 4099)[k % 3], k, alt, fill, 30))
        lines.append(_long_line((2000, 4099, 1025)[k % 3], k, alt, fill, 2))
    assert all(1025 <= len(ln.encode()) <= 8000 for ln in lines)
    docs = ["\n".join(lines[i:i + 9]) for i in range(0, len(lines), 9)] + ["x" * 2000 + alt[:-1] + "\n" + "x12y" + "w" * 1500]
    check_docs(eng, pats, docs, tb)
    scan = eng.log_scan(*pack_documents(docs), tables=tb)
    assert int(scan.hist[:, 0].sum()) == len(lines)  # every placement found


# ---- knob, degenerate inputs ---------------------------------------------------------------------------
def test_log_fused_knob_does_not_apply_to_tables_calls(eng):
    pats = S.SETS["C"]
    docs = S.fragment_fuzz(pats, 200, seed=3) + ["k" * 1500 + " status=503"]
    blob, off = pack_documents(docs)
    tb = eng.log_tables(pats)
    base = one_call(eng, blob, off, tb)
    for fused in (1, 2):
        with native.tune(eng.lib, KRCA_LOG_FUSED=fused):
            got = one_call(eng, blob, off, tb)
        for k in KEYS:
            assert np.array_equal(got[k], base[k]), (fused, k)


def test_degenerate_inputs(eng):
    one = [("one", "x")]  # ncat = 1, a set of one one-character pattern
    for pats in (one, S.SETS["C"]):
        tb = eng.log_tables(pats)
        for docs in ([""], ["", "", ""], ["x\nabc\nX", "", "status=500 x"], ["", "x"], ["\n"], ["x" * 15 + "\n"]):
            check_docs(eng, pats, docs, tb)
        r = one_call(eng, *pack_documents(["", ""]), tb)
        assert r["hist"].shape == (2, len(pats)) and not r["hist"].any() and (r["examples"] == -1).all()
        assert not r["doc_lines"].any() and not r["doc_line0"].any()
    assert eng.log_tables(one).tables.nstate == 2


def test_upload_refuses_a_corrupt_image_before_any_device_work(eng):
    """(host-side refusal: nothing is launched and the device buffer keeps its bytes)"""
    t = eng.log_tables(S.SETS["C"]).tables
    im = bytearray(t.image())
    struct.pack_into("<H", im, 48 + 128 + 12 * t.nrange + 2 * 9, t.nstate)  # a transition to state nstate
    dev = eng.torch.full((1 << 16,), 0x5B, dtype=eng.torch.uint8, device=eng.device)
    dims = native.LogDims()
    buf = (ctypes.c_char * len(im)).from_buffer_copy(bytes(im))
    rc = eng.lib.krca_log_tables_upload(buf, len(im), eng.ptr(dev), dev.numel(), ctypes.byref(dims), eng._stream())
    assert rc == -22 and b"goes to state" in eng.lib.krca_last_error()
    assert bool((dev == 0x5B).all().item())
    # dimensions past the limits are refused by the scan call itself
    good = eng.log_tables(S.SETS["C"])
    bad = native.LogDims.from_buffer_copy(good.dims)
    bad.nstate = 1025
    blob, off = pack_documents(["status=500"])
    with pytest.raises(native.KrcaError, match="outside the limits"):
        eng.log_scan_device(eng.upload_blob(blob), eng._dev(off), tables=native.DeviceLogTables(good.tables, good.dev, bad))


# ---- guard bands and poisoned buffers ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def geng():
    return GuardedEngine()


def _guarded_call(pats, docs):
    blob, off = pack_documents(docs)

    def call(e):
        e.__dict__.pop("_log_tables", None)  # the device form is carved from this guard's arena too
        tb = e.log_tables(pats)
        r = e.log_scan_device(e.upload_blob(blob), e._dev(off), dense_examples=True, tables=tb)
        return {k: r[k].cpu().numpy().copy() for k in KEYS}
    return call


@pytest.mark.parametrize("name,n_docs", [("C", 60), ("B", 900)])
def test_guard_bands_and_poisons(geng, name, n_docs):
    """Outputs and workspace poisoned 0x00 / 0xFF / 0x5B, every buffer carved at exactly its size:
    nothing written outside, inputs unchanged, outputs identical across poisons and equal to re.
    60 containers stay under the engine's 1024-line arrays (the one call); 900 go past them (the
    one call, then krca_log_match_tables)."""
    pats = S.SETS[name]
    lits = S.literals(pats)
    docs = S.fragment_fuzz(pats, n_docs, seed=9) + ["y" * 1100 + lits[0] + "\n" + "é" * 700 + lits[-1] + "z" * 2000, ""]
    out = run_poisons(geng, _guarded_call(pats, docs))
    assert (len(out["line_start"]) > 1024) == (name == "B")
    for d, text in enumerate(docs):
        n, h, _ = S.re_hist(pats, text)
        assert out["doc_lines"][d] == n and out["hist"][d].tolist() == h, d
    assert np.array_equal(out["examples"], native.example_ids(out["line_mask"], out["doc_line0"], out["doc_lines"], len(pats)))


@pytest.mark.parametrize("name", ["C", "B"])
def test_guard_bands_no_text(geng, name):
    pats = S.SETS[name]
    out = run_poisons(geng, _guarded_call(pats, ["", "", ""]))
    assert out["hist"].shape == (3, len(pats)) and not out["hist"].any() and (out["examples"] == -1).all()
    assert not out["doc_lines"].any() and len(out["line_start"]) == 0


# ---- the agent ------------------------------------------------------------------------------------------------
def test_agent_compile_patterns_equals_reference_findings(eng):
    gold = A.load("logs_custom_patterns.json")["mock_cluster_A"]
    agent = A.LogsAgent(A.Shim(), engine=eng, compile_patterns=True)
    agent.error_patterns = dict(S.SETS["A"])
    assert A.same(agent.analyze(gold["namespace"]), gold["result"])
    refused = A.LogsAgent(A.Shim(), engine=eng)
    refused.error_patterns = dict(S.SETS["A"])
    assert "error" in refused.analyze(gold["namespace"])
