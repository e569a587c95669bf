"""Log scan with unbounded quantifiers in run-time pattern sets on an MI355X:
NativeEngine.log_tables(patterns, unbounded=True), the long-line kernel that carries the DFA state
from segment to segment (log_dfa_long<TabRt, CARRY>, taken for tables with KRCA_LOG_FLAG_CARRY),
LogsAgent(unbounded=True) and StreamingRCA(log_tables=).

Expected values: Python's ``re`` per line (the reference's definition, ref:agents/logs_agent.py:147-149),
computed here; for the carried kernel on fixed-length sets, the existing long-line kernel's arrays."""
import numpy as np
import pytest

import agent_cases as A
import custom_pattern_sets as S
import unbounded_pattern_sets as U
from guarded import GuardedEngine, run_poisons
from krca import logdfa, native, synth
from krca.agents.logs import pack_documents
from krca.rca import Config
from krca.stream import StreamingRCA
from test_gpu_log_tables import KEYS, _edge_docs, _end_docs, _golden_docs, _long_line, _tile_docs, check_docs, one_call
from test_logdfa_unbounded_cpu import LOGS, OneLog, ReEngineU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


@pytest.fixture(scope="module")
def u4(eng):
    return eng.log_tables(U.U4, unbounded=True)


def line_masks(e, tb, lines):
    """The category mask of every line (one container per line)."""
    blob, off = pack_documents(lines)
    r = e.log_scan_device(e.upload_blob(blob), e._dev(np.asarray(off, np.int64)), tables=tb)
    assert r["n_lines_total"] == len(lines)
    return (r["line_mask"].cpu().numpy().view(np.uint32) & 0xFFFF).tolist()


# ---- sets against re ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["U1", "U2", "U4", "UB2"])
def test_sets_equal_re(eng, name):
    """U1 / U2: 31 symbols, 737 / 719 states; UB2: 64 columns and 1002 states (a 130 KB table, one
    workgroup per CU); U4: 4 categories.  Lines up to 1 KiB: a lane per line from its first byte."""
    pats = U.SETS[name]
    lits = U.literals(pats)
    tb = eng.log_tables(pats, unbounded=True)
    assert tb.ncat == len(pats) and tb.dims.flags == logdfa.FLAG_CARRY
    assert (tb.tables.ncat, tb.tables.nsym, tb.tables.nstate) == U.SIZES[name]
    docs = _tile_docs(lits) + U.fragment_fuzz(pats, 300, seed=21) + _edge_docs(lits) + _end_docs(lits)
    assert len(docs[0].encode()) == 65536  # the second container starts on the tile boundary
    check_docs(eng, pats, docs, tb)
    for tail in (0, 1, 7, 15, 16):  # texts ending at several offsets mod 16
        check_docs(eng, pats, ["z" * 11 + "\n" + lits[0] * 2 + "q" * tail], tb)


# ---- long lines against re ---------------------------------------------------------------------------------
def test_long_lines_equal_re(eng, u4):
    """Every line of unbounded_pattern_sets.long_lines_u4 (1 025 to 8 000 bytes: a wave per line): the
    state armed in segment i is seen in segment j, never the other way round; digit runs and x{3,} cross
    the boundaries; 2- and 3-byte code points straddle them."""
    tagged = U.long_lines_u4()
    lines = [ln for _, ln in tagged]
    want = [S.re_masks(U.U4, ln)[0] for ln in lines]
    got = line_masks(eng, u4, lines)
    bad = [(tag, g, w) for (tag, _), g, w in zip(tagged, got, want) if g != w]
    assert not bad, bad[:10]
    assert {1, 0, 2, 4} <= set(want)
    docs = ["\n".join(lines[i:i + 9]) for i in range(0, len(lines), 9)]  # and as containers: hist and examples
    check_docs(eng, U.U4, docs, u4)


def test_long_lines_of_other_sets_equal_re(eng):
    for name in ("U1", "UB2"):
        pats = U.SETS[name]
        lits = U.literals(pats)
        tb = eng.log_tables(pats, unbounded=True)
        lines = ["Exception" + "é" * 700 + "at", "at" + "q" * 2000 + "Exception", "Exception " + "w" * 5000 + " timeout at",
                 "y" * 1100 + lits[0] + "z" * 40 + lits[-1], "StatusCode=5" + "٣" * 800, "€" * 400 + lits[3][:-1]]
        assert line_masks(eng, tb, lines) == [S.re_masks(pats, ln)[0] for ln in lines], name


@pytest.mark.timeout(120, method="thread")  # its own limit (the kernel's loop is bounded: 63 rounds of one segment)
def test_worst_case_60000_byte_line(eng, u4):
    """"error" in the first segment, "timeout" in the last: 63 rounds, lane r walking alone in round r
    (tests/test_logdfa_unbounded_cpu.py pins the round count on the kernel's Python restatement)."""
    hit, miss = U.worst_case_lines()
    assert line_masks(eng, u4, [hit, miss, hit, "error timeout"]) == [1, 0, 1, 1]


# ---- the carried kernel against the existing one, on fixed-length sets --------------------------------------------
def _long40_docs(multibyte):
    alt = "abcdefghij" * 4
    pats = S.LONG40
    if multibyte:
        alt = "abcdefghij" + "é" + "bcdefghij" + "a€cdefghij" + "abcdefghij"
        pats = [("long40", "(" + alt + "|zq)"), S.LONG40[1]]
    lines = []
    for k in range(1, 64):
        fill = "é" if multibyte and k % 2 else "x"
        lines.append(_long_line(8000, k, alt, fill, 39))
        lines.append(_long_line((1025, 2000, 4099)[k % 3], k, alt, fill, 30))
        lines.append(_long_line((2000, 4099, 1025)[k % 3], k, alt, fill, 2))
    docs = ["\n".join(lines[i:i + 9]) for i in range(0, len(lines), 9)] + ["x" * 2000 + alt[:-1] + "\n" + "x12y" + "w" * 1500]
    return pats, docs


@pytest.mark.parametrize("case", ["long40", "long40-multibyte", "s13-golden", "s13-long"])
def test_carry_flag_forced_on_fixed_sets_is_byte_equal(eng, case):
    """The same tables uploaded with KRCA_LOG_FLAG_CARRY forced on (LogTables.image(flags=)): long lines
    go through the carrying log_dfa_long and every output array equals the unflagged tables' byte for byte."""
    if case.startswith("long40"):
        pats, docs = _long40_docs(case.endswith("multibyte"))
    else:
        pats = S.S13
        docs = _golden_docs() if case == "s13-golden" else \
            ["x" * 3000 + " Killed " + "é" * 900, "connect: connec" + "t" * 1500 + "ion refused\nCrashLoopBackOff " + "€" * 600 + " Forbidden"]
    plain = eng.log_tables(pats)
    forced = eng.upload_log_tables(plain.tables, flags=logdfa.FLAG_CARRY)
    assert plain.dims.flags == 0 and forced.dims.flags == 1
    blob, off = pack_documents(docs)
    want, got = one_call(eng, blob, off, plain), one_call(eng, blob, off, forced)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert want["hist"].sum() > 0
    if case != "s13-golden":
        assert int((want["line_end"] - want["line_start"]).max()) > 1024


# ---- guard bands and poisoned buffers ---------------------------------------------------------------------------
def test_guard_bands_and_poisons():
    geng = GuardedEngine()
    hit, _ = U.worst_case_lines(9000)
    tagged = dict(U.long_lines_u4())
    docs = U.fragment_fuzz(U.U4, 60, seed=9) + [tagged["fwd-0-63-2"], tagged["retry-5-3-2"] + "\n" + hit, ""]
    blob, off = pack_documents(docs)

    def call(e):
        e.__dict__.pop("_log_tables", None)  # the device form is carved from this guard's arena too
        tb = e.log_tables(U.U4, unbounded=True)
        r = e.log_scan_device(e.upload_blob(blob), e._dev(off), dense_examples=True, tables=tb)
        return {k: r[k].cpu().numpy().copy() for k in KEYS}

    out = run_poisons(geng, call)
    assert int((out["line_end"] - out["line_start"] > 1024).sum()) == 3
    for d, text in enumerate(docs):
        n, h, _ = S.re_hist(U.U4, text)
        assert out["doc_lines"][d] == n and out["hist"][d].tolist() == h, d
    assert np.array_equal(out["examples"], native.example_ids(out["line_mask"], out["doc_line0"], out["doc_lines"], 4))


# ---- the agent ----------------------------------------------------------------------------------------------------
def test_agent_unbounded_on_the_device_equals_the_cpu_result(eng):
    def run(engine, **kw):
        agent = A.LogsAgent(OneLog(), engine=engine, compile_patterns=True, **kw)
        agent.error_patterns = dict(U.U1)
        return agent.analyze(A.NS)
    got, want = run(eng, unbounded=True), run(ReEngineU(), unbounded=True)
    assert "error" not in got and A.strip(got) == A.strip(want)
    assert sum("Exception in logs" in f["issue"] for f in got["findings"]) > 0 and "Exception" in LOGS
    refused = run(eng)
    assert "error" in refused and "unbounded quantifier '*'" in refused["error"] and "exception" in refused["error"]


def test_golden_set_u1_on_the_device(eng):
    """tests/golden/logs_unbounded_patterns.json (the reference's LogsAgent with set U1): per-line masks
    and the agent's result on the mock cluster."""
    g = A.load("logs_unbounded_patterns.json")
    tb = eng.log_tables(U.U1, unbounded=True)
    blob, off = pack_documents([c["text"] for c in g["containers"]])
    r = one_call(eng, blob, off, tb)
    assert (r["line_mask"].view(np.uint32) & 0xFFFF).tolist() == [m for c in g["containers"] for m in c["masks"]]
    agent = A.LogsAgent(A.Shim(), engine=eng, compile_patterns=True, unbounded=True)
    agent.error_patterns = dict(U.U1)
    assert A.same(agent.analyze(g["mock_cluster"]["namespace"]), g["mock_cluster"]["result"])


# ---- the stream -----------------------------------------------------------------------------------------------------
def test_stream_push_logs_with_unbounded_tables(eng, u4):
    P, M, W = 1500, 8, 60  # the smallest mesh of tests/test_gpu_stream.py
    m = synth.make_graph(P, avg_degree=8, seed=3)
    docs = U.fragment_fuzz(U.U4, 200, seed=4) + ["error " + "q" * 1500 + " timeout\nretry 1/2", "xx\nwarnings: xxx"]
    blob, off = pack_documents(docs)
    text, offd = eng.upload_blob(blob), eng._dev(off)
    s = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, Config(window=W), log_tables=u4)
    s.prime(len(blob), len(docs))  # primes the tables' kernels: no stream state changes
    got = s.push_logs(text, offd)
    want = eng.log_scan(blob, off, tables=u4)
    hist = got["hist"].cpu().numpy()
    assert hist.shape == (len(docs), 4) and np.array_equal(hist, want.hist) and hist.sum() > 0
    assert hist[-2].tolist() == [1, 1, 0, 0] and hist[-1].tolist() == [0, 0, 1, 1]
    default = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, Config(window=W))
    base = default.push_logs(text, offd)
    assert base["hist"].shape == (len(docs), 13)
    for k in ("n_templates", "tmpl_hash", "tmpl_count", "hash"):  # the template pass does not depend on the patterns
        assert np.array_equal(got["templates"][k].cpu().numpy(), base["templates"][k].cpu().numpy()), k
    per_call = default.push_logs(text, offd, templates=False, tables=u4)
    assert np.array_equal(per_call["hist"].cpu().numpy(), hist)
