"""Run-time log pattern compiler (krca/logdfa.py), the table image's host validator
(krca_log_tables_check) and LogsAgent(compile_patterns=True), without a GPU.

Expected values come from Python's ``re`` (the reference's definition of a match), from the
committed csrc/log_dfa_tables.h (what csrc/gen_log_dfa.py emits for the 13 shipped patterns) and
from tests/golden/logs_custom_patterns.json (captured from the reference)."""
import os
import re
import struct
import sys

import numpy as np
import pytest

import agent_cases as A
import custom_pattern_sets as S
from conftest import ROOT
from krca import logdfa, native, patterns as P
from oracle_engine import OracleEngine

CSRC = os.path.join(ROOT, "kubernetes-rca-system_amd", "csrc")


def gen_log_dfa():
    if CSRC not in sys.path:
        sys.path.insert(0, CSRC)
    import gen_log_dfa as g
    return g


def test_s13_emits_the_committed_header_byte_for_byte(tmp_path):
    """compile_patterns(S13) fed to gen_log_dfa.emit() gives csrc/log_dfa_tables.h byte for byte: every
    field (symbols, ranges, transitions, masks, SEP, OTHER, counts) equals what gen_log_dfa.build()
    produced for the committed header, under the interpreter the header names.  (A fresh build() takes
    12 s -- a fullmatch per code point and atom -- and emits this very file.)"""
    t = logdfa.compile_patterns(S.S13)
    out = tmp_path / "tables.h"
    gen_log_dfa().emit(t.as_dict(), str(out))
    with open(os.path.join(CSRC, "log_dfa_tables.h"), "rb") as f:
        assert out.read_bytes() == f.read()
    assert t.digest == P.pattern_digest() and t.warm == 26  # "connect: connection refused" is 27 code points


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_set_sizes_as_measured_with_the_generator(name):
    t = logdfa.compile_patterns(S.SETS[name])
    assert (t.ncat, t.nsym, t.nstate) == S.SIZES[name]


def test_set_e_within_limits():
    """Set E (every supported construct).  Sizes recorded: 5 categories, 26 symbols, 89 states,
    739 ranges (\\w and \\s classes split the non-ASCII code points), warm 5."""
    t = logdfa.compile_patterns(S.SETS["E"])
    assert t.ncat == 5 and t.nsym <= logdfa.MAX_NSYM and t.nstate <= logdfa.MAX_NSTATE
    assert t.nrange <= logdfa.MAX_NRANGE and t.warm == 5
    assert (t.nsym, t.nstate, t.nrange) == (26, 89, 739)


@pytest.mark.parametrize("name", ["S13", "A", "B", "C", "D", "E"])
def test_table_walk_equals_re_search_on_fragment_fuzz(name):
    pats = S.SETS[name]
    t = logdfa.compile_patterns(pats)
    assert logdfa.compile_patterns(list(pats)) is t  # cached per process by digest
    n = 0
    for text in S.fragment_fuzz(pats, 400, seed=31):
        for line, want in zip(text.splitlines(), S.re_masks(pats, text)):
            assert logdfa.simulate(t, line) == want, (name, line)
            n += want != 0
    assert n > 100
    hazards = ["KeeperErrorCode Killed", "acceſſ denied zookeeper ſeſſion expired",
               "StatusCode=5٣٤ status=5๑๒ n=٣;", "AUTHENTİCATION FAILED", "id=中 x id=é -",
               "id=_ 7 id=٣ ٣", "aézzz aéZZZ bxzzz", "0a٣f-é 0A0F- ", "plaiɴ OTHER"]
    for line in hazards:
        assert logdfa.simulate(t, line) == S.re_masks(pats, line)[0], (name, line)


UNSUPPORTED = [("a*b", "quantifier '*'"), ("a+", "quantifier '+'"), ("ab{2,}", "{2,}"), ("^start", "anchor '^'"),
               ("end$", "anchor '$'"), (r"\bword", "word boundary"), ("a(b|c)d", "nested group"), (r"(a)\1", "back-reference"),
               ("(?=x)y", "look-ahead"), ("(?<!x)y", "look-behind"), ("(?i)abc", "inline flags"), ("(?:ab)c", "nested group"),
               ("a(b", "re.compile rejects"), ("[z-a]", "re.compile rejects"), ("ab|", "empty alternative"),
               ("a??", "lazy"), ("(a|b)(c|d)", "nested group"), (r"\Aab", "anchor")]


@pytest.mark.parametrize("rx,what", UNSUPPORTED)
def test_unsupported_constructs_name_the_construct_and_category(rx, what):
    with pytest.raises(logdfa.PatternsUnsupported) as e:
        logdfa.compile_patterns([("ok", "fine"), ("mycat", rx)])
    assert what in str(e.value) and "mycat" in str(e.value)
    assert isinstance(e.value, P.PatternsChanged)


def test_limits_raise_with_the_measured_value():
    with pytest.raises(logdfa.PatternsUnsupported, match="17 categories"):
        logdfa.compile_patterns([(f"c{i}", f"word{i}") for i in range(17)])
    with pytest.raises(logdfa.PatternsUnsupported, match="65 code points"):
        logdfa.compile_patterns([("long", "x" * 65)])
    logdfa.compile_patterns([("long", "xy" * 32)])  # 64 code points fit
    with pytest.raises(logdfa.PatternsUnsupported, match=r"64 symbols"):  # 63 distinct letters/signs + OTHER
        logdfa.compile_patterns([("many", "".join(re.escape(chr(c)) for c in range(33, 33 + 26)) + "|" +
                                  "".join(re.escape(chr(c)) for c in range(91, 91 + 6)) + "|" +
                                  "".join(chr(c) for c in range(0x3b1, 0x3b1 + 17)) + "|" +
                                  "".join(chr(c) for c in range(0x430, 0x430 + 14)))])
    rng = np.random.default_rng(5)  # 60 random 20-letter words share no prefixes: ~1140 trie states
    words = ["".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), 20)) for _ in range(60)]
    with pytest.raises(logdfa.PatternsUnsupported, match=r"\d{4} states"):
        logdfa.compile_patterns([("w%d" % i, "|".join(words[6 * i:6 * i + 6])) for i in range(10)])
    with pytest.raises(logdfa.PatternsUnsupported, match="alternatives"):
        logdfa.compile_patterns([("q", "a?b?c?d?e?f?g?h?i?z")])  # 512 alternatives after expansion


# ---- the image and its host validator ------------------------------------------------------------
def _image(name):
    return bytearray(logdfa.compile_patterns(S.SETS[name]).image())


def _check(image):
    return native.check_log_image(bytes(image))


@pytest.mark.parametrize("name", ["S13", "A", "B", "C", "D", "E"])
def test_validator_accepts_every_set(name):
    t = logdfa.compile_patterns(S.SETS[name])
    d = _check(t.image())
    assert (d.ncat, d.nsym, d.nstate, d.nrange, d.warm, d.other, d.digest) == \
        (t.ncat, t.nsym, t.nstate, t.nrange, t.warm, t.OTHER, t.digest)
    lib = native.load_library()
    import ctypes
    size = lib.krca_log_tables_dev_size(ctypes.byref(d))
    cols = 32 if t.nsym <= 31 else 64
    assert size >= t.nstate * cols * 2 + t.nstate * 2 + 256 + 12 * t.nrange and size % 16 == 0 and size < 160 * 1024


def test_validator_rejects_single_field_corruptions():
    t = logdfa.compile_patterns(S.SETS["C"])
    off_ranges = 48 + 128
    off_trans = off_ranges + 12 * t.nrange
    off_out = off_trans + 2 * t.nstate * t.nsym

    def put(fmt, off, *v):
        im = _image("C")
        struct.pack_into(fmt, im, off, *v)
        return im
    lo1, = struct.unpack_from("<I", _image("C"), off_ranges + 12)
    cases = {
        "magic": put("<I", 0, 0x12345678), "version": put("<I", 4, 2), "ncat": put("<I", 8, 17),
        "nsym": put("<I", 12, 64), "nstate": put("<I", 16, 1025), "nrange": put("<I", 20, 1025),
        "warm": put("<I", 24, 64), "unlisted code points": put("<I", 28, t.nsym), "header says": put("<I", 40, 8),
        "goes to state": put("<H", off_trans + 2 * 7, t.nstate), "at or above ncat": put("<H", off_out + 2 * 5, 1 << t.ncat),
        "not sorted": put("<I", off_ranges, lo1 + 1),          # range 0 now starts after range 1
        "inside 0x80": put("<I", off_ranges, 0x41),             # a range over ASCII
        "has symbol": put("<I", off_ranges + 8, t.nsym), "is no symbol": put("<B", 48 + ord("a"), t.nsym),
        "truncated": _image("C")[:-8], "shorter than its header": _image("C")[:40],
    }
    lib = native.load_library()
    for what, im in cases.items():
        with pytest.raises(native.KrcaError) as e:
            _check(im)
        assert what in str(e.value), (what, str(e.value))
        assert what.encode() in lib.krca_last_error()
    _check(_image("C"))  # and the untouched image still passes


# ---- the agent, on CPU: an engine that answers tables= by re -------------------------------------------
class ReLogScan:
    def __init__(self, pats, docs):
        rows = [S.re_hist(pats, text) for text in docs]
        self.n_lines = np.asarray([r[0] for r in rows], np.int32)
        self.hist = np.asarray([r[1] for r in rows], np.int32).reshape(-1, len(pats))
        self._ex = [r[2] for r in rows]

    def examples(self, d, c):
        return self._ex[d][c]


class ReEngine(OracleEngine):
    """OracleEngine plus the run-time tables interface: log_tables() runs the real compiler (so an
    unsupported set raises as on the device path), log_scan(tables=) matches with re."""

    def log_tables(self, pats):
        return logdfa.compile_patterns(pats)

    def log_scan(self, blob, doc_off, tables=None):
        if tables is None:
            return super().log_scan(blob, doc_off)
        docs = [blob[doc_off[i]:doc_off[i + 1]].decode("utf-8", "surrogatepass") for i in range(len(doc_off) - 1)]
        return ReLogScan(tables.patterns, docs)


GOLD = A.load("logs_custom_patterns.json")


def _agent(pats, **kw):
    agent = A.LogsAgent(A.Shim(), engine=ReEngine(), **kw)
    agent.error_patterns = dict(pats)
    return agent


def test_agent_with_set_a_equals_the_reference_findings():
    assert [tuple(p) for p in GOLD["sets"]["A"]["patterns"]] == S.SETS["A"]
    res = _agent(S.SETS["A"], compile_patterns=True).analyze(A.NS)
    assert A.same(res, GOLD["mock_cluster_A"]["result"])


def test_agent_default_still_refuses_and_unedited_dict_takes_the_compiled_path():
    res = _agent(S.SETS["A"]).analyze(A.NS)
    assert "error" in res and "krca/patterns.py" in res["error"]

    class NoTables(ReEngine):
        def log_tables(self, pats):
            raise AssertionError("an unedited dict must not be compiled")
    agent = A.LogsAgent(A.Shim(), engine=NoTables(), compile_patterns=True)
    default = A.LogsAgent(A.Shim(), engine=OracleEngine()).analyze(A.NS)
    assert default["findings"] and A.strip(agent.analyze(A.NS)) == A.strip(default)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_agent_reports_golden_containers_in_dict_order(name):
    g = GOLD["sets"][name]
    pats = [tuple(p) for p in g["patterns"]]
    assert pats == S.SETS[name]
    agent = _agent(pats, compile_patterns=True)
    scan = ReLogScan(pats, [c["text"] for c in g["containers"]])
    for i, c in enumerate(g["containers"]):
        assert S.re_masks(pats, c["text"]) == c["masks"]
        agent.reset()
        agent._report_container(scan, i, c["pod"], c["container"], tuple(n for n, _ in pats))
        assert A.strip(agent.get_results()) == c["result"], i


def test_agent_deleted_category_disappears_and_unknown_name_is_info():
    logs = "x\nKilled by signal\nwidget jammed\nrequest timeout\n"

    class OneLog(A.Shim):
        def get_pod_logs(self, pod_name, namespace, container_name=None, tail_lines=100, previous=False):
            return logs
    pats = [p for p in S.S13 if p[0] != "timeout"] + [("widget_jam", "widget jammed|gear stuck")]
    agent = A.LogsAgent(OneLog(), engine=ReEngine(), compile_patterns=True)
    agent.error_patterns = dict(pats)
    res = agent.analyze(A.NS)
    issues = [f for f in res["findings"] if "in logs" in f["issue"]]
    assert issues and not any("Timeout" in f["issue"] for f in issues)
    jam = [f for f in issues if f["issue"] == "Detected 1 instances of Widget Jam in logs"]
    assert jam and all(f["severity"] == "info" and
                       f["recommendation"] == "Investigate the logs in detail to identify the root cause" for f in jam)
    assert any(f["issue"] == "Detected 1 instances of Oom Kill in logs" for f in issues)


def test_agent_unsupported_regex_gives_the_error_dict():
    pats = S.S13[:-1] + [("exception", r"Exception.*at")]
    res = _agent(pats, compile_patterns=True).analyze(A.NS)
    assert "error" in res and "unbounded quantifier '*'" in res["error"] and "exception" in res["error"]
