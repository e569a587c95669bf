"""Unbounded quantifiers in run-time log pattern sets (krca.logdfa.compile_patterns(..., unbounded=True)),
the carry flag of the table image and its host validator, simulate_segments (the specification of the
long-line kernel that carries the state from segment to segment) and LogsAgent(unbounded=True),
without a GPU.

Expected values come from Python's ``re`` per line (the reference's definition of a match,
ref:agents/logs_agent.py:147-149) and from tests/golden/logs_unbounded_patterns.json (captured from the
reference's LogsAgent with set U1 by tests/golden/capture_unbounded_patterns.py).

What loops cost: the tables are ONE product DFA.  A ``\\d+``-style loop is nearly free (U2 has fewer
states than U1), but each ``.*`` between two literals keeps "the first literal was seen" alive beside
every position of every other pattern and roughly doubles the state count: one ``.*`` fits beside the
13 shipped patterns (U1: 737 of 1024 states), two do not (U3: 4408; U8, eight of them alone: 2814)."""
import re
import struct

import pytest

import agent_cases as A
import custom_pattern_sets as S
import unbounded_pattern_sets as U
from krca import logdfa, native, patterns as P
from krca.agents.logs import format_examples
from test_logdfa_cpu import ReEngine, ReLogScan


def _tables(name):
    return logdfa.compile_patterns(U.SETS[name], unbounded=True)


@pytest.mark.parametrize("name", ["U1", "U2", "U4", "UB2"])
def test_sets_compile_with_pinned_sizes(name):
    """UB2 (set B, 36 symbols, with two loops) stays under 1024 states with all 16 categories: 1002."""
    t = _tables(name)
    assert (t.ncat, t.nsym, t.nstate) == U.SIZES[name]
    assert t.flags == logdfa.FLAG_CARRY and 0 <= t.warm <= 63
    assert logdfa.compile_patterns(list(U.SETS[name]), unbounded=True) is t  # cached per process by digest


def test_warm_counts_loops_at_their_minimum():
    assert _tables("U4").warm == 11  # "error.*timeout": 12 atoms besides the loop
    assert _tables("U1").warm == 26  # "connect: connection refused", as S13
    t = logdfa.compile_patterns([("long", "a" * 59 + "b{4,}c+")], unbounded=True)
    assert t.warm == 63  # 64 code points with the loops at their minimum, the limit of an alternative
    with pytest.raises(logdfa.PatternsUnsupported, match="65 code points"):
        logdfa.compile_patterns([("long", "a" * 60 + "b{4,}c+")], unbounded=True)


@pytest.mark.parametrize("name", ["U1", "U2", "U4", "UB2"])
def test_table_walk_equals_re_search(name):
    pats = U.SETS[name]
    t = _tables(name)
    n = 0
    for text in U.fragment_fuzz(pats, 400, seed=31):
        for line, want in zip(text.splitlines(), S.re_masks(pats, text)):
            assert logdfa.simulate(t, line) == want, (name, line)
            n += want != 0
    assert n > 100
    for line in U.loop_examples(pats) + U.gap_examples(pats) + U.HAZARDS:
        assert logdfa.simulate(t, line) == S.re_masks(pats, line)[0], (name, line)
    # every example of a pattern is a match of it: the loops taken 0 (their minimum), 1, 5 and 40 times
    assert all(S.re_masks(pats, s)[0] for s in U.loop_examples(pats))


def test_loops_at_the_start_and_end_of_an_alternative():
    pats = [("lead", r"\d*ab"), ("trail", r"cd\s+"), ("both", r"x+yz{2,}"), ("mid", r"p{,}q[0-9]{1,}r?")]
    t = logdfa.compile_patterns(pats, unbounded=True)
    for line in ["ab", "77ab", "٣ab", "a", "cd", "cd ", "cd \t x", "yzz", "xyzz", "xxxyzzzz", "xyz", "q7", "ppq٣٣r", "pq", "q",
                 "cdab  xyz"]:
        assert logdfa.simulate(t, line) == S.re_masks(pats, line)[0], line


@pytest.mark.parametrize("name", ["U3", "U8"])
def test_too_many_states_raises_with_the_measured_count(name):
    pats, nstate = U.TOO_LARGE[name]
    with pytest.raises(logdfa.PatternsUnsupported, match=rf"{nstate} states; the device matcher holds at most 1024"):
        logdfa.compile_patterns(pats, unbounded=True)


REFUSED = [("(ab)*c", "on anything but one atom"), ("(ab|c)+", "on anything but one atom"), ("a*?b", "lazy or possessive"),
           ("a+?b", "lazy or possessive"), ("a{2,}?b", "lazy or possessive"),
           ("a*+b", ("lazy or possessive", "re.compile rejects")),  # (possessive forms: a syntax error before Python 3.11)
           ("^a+", "anchor '^'"), ("a+$", "anchor '$'"), (r"\ba+", "word boundary"), ("a(b+|c)d", "nested group"),
           (r"(a+)\1", "back-reference"), ("(?=x+)y", "look-ahead"), ("(?<!x)y+", "look-behind"), ("(?i)ab+", "inline flags"),
           ("a*", "empty alternative"), ("x*y?", "empty alternative"), ("ab|c*", "empty alternative"), ("a{,}", "empty alternative")]


@pytest.mark.parametrize("rx,what", REFUSED)
def test_still_refused_constructs_name_the_construct_and_category(rx, what):
    with pytest.raises(logdfa.PatternsUnsupported) as e:
        logdfa.compile_patterns([("ok", "fine+"), ("mycat", rx)], unbounded=True)
    assert any(w in str(e.value) for w in ([what] if isinstance(what, str) else what)) and "mycat" in str(e.value)
    assert isinstance(e.value, P.PatternsChanged)


def test_default_still_refuses_with_todays_messages():
    for rx, what in (("a*b", "unbounded quantifier '*'"), ("a+", "unbounded quantifier '+'"), ("ab{2,}", "unbounded quantifier '{2,}'")):
        for kw in ({}, {"unbounded": False}):
            with pytest.raises(logdfa.PatternsUnsupported, match=re.escape(what)):
                logdfa.compile_patterns([("mycat", rx)], **kw)
    with pytest.raises(logdfa.PatternsUnsupported, match="unbounded quantifier"):
        logdfa.parse("mycat", "a+")


@pytest.mark.parametrize("name", ["S13", "B", "C", "E"])
def test_fixed_length_set_gives_the_same_image_byte_for_byte(name):
    want = logdfa.compile_patterns(S.SETS[name]).image()
    logdfa._CACHE.clear()  # compile again, not the cached object
    t = logdfa.compile_patterns(S.SETS[name], unbounded=True)
    assert t.flags == 0 and t.image() == want and struct.unpack_from("<I", want, 44)[0] == 0
    assert t.image(flags=logdfa.FLAG_CARRY)[:44] == want[:44] and t.image(flags=logdfa.FLAG_CARRY)[48:] == want[48:]
    assert t.image() == want  # forcing the flag leaves the set's own image as it was


# ---- the image and its host validator ------------------------------------------------------------------
def test_validator_accepts_a_carry_image_and_reports_the_flag():
    for name in U.SETS:
        t = _tables(name)
        d = native.check_log_image(t.image())
        assert (d.ncat, d.nsym, d.nstate, d.nrange, d.warm, d.other, d.digest, d.flags) == \
            (t.ncat, t.nsym, t.nstate, t.nrange, t.warm, t.OTHER, t.digest, logdfa.FLAG_CARRY)
    fixed = logdfa.compile_patterns(S.SETS["C"])
    assert native.check_log_image(fixed.image()).flags == 0
    assert native.check_log_image(fixed.image(flags=logdfa.FLAG_CARRY)).flags == 1
    assert native.LogDims.flags.offset == 32 and native.LogDims.digest.offset == 24  # a trailing field


@pytest.mark.parametrize("flags", [2, 3, 0x80000000])
def test_validator_rejects_unknown_flag_bits(flags):
    im = bytearray(_tables("U4").image())
    struct.pack_into("<I", im, 44, flags)
    with pytest.raises(native.KrcaError, match="flags"):
        native.check_log_image(bytes(im))
    assert b"flags" in native.load_library().krca_last_error()


# ---- simulate_segments: the carried long-line kernel's specification --------------------------------------
@pytest.fixture(scope="module")
def u4():
    return _tables("U4")


def test_simulate_segments_equals_simulate_on_the_long_lines(u4):
    lines = U.long_lines_u4()
    assert len(lines) > 150 and all(1025 <= len(ln.encode()) <= 8000 for _, ln in lines)
    hit = {"fwd": 0, "rev": 0, "retry": 0, "x": 0, "x2": 0}
    most = 0
    for tag, line in lines:
        want = S.re_masks(U.U4, line)[0]
        assert logdfa.simulate(u4, line) == want, tag
        mask, rounds = logdfa.simulate_segments(u4, line)
        assert mask == want and rounds <= 63, (tag, rounds)
        most = max(most, rounds)
        kind = tag.split("-")[0]
        hit[kind] += 1
        assert want == {"fwd": 1, "rev": 0, "retry": 2, "x": 4, "x2": 0}[kind], tag  # the generator built what it says
    assert all(hit.values()) and most >= 50  # (0, 63) of an 8000-byte line: the state crosses 62 boundaries


def test_simulate_segments_on_other_sets_and_segment_counts():
    t = _tables("U1")
    lits = U.literals(U.U1)
    for k, line in enumerate(["y" * 1100 + lits[0] + "z" * 40, "Exception" + "é" * 900 + "at", "at" + "q" * 2000 + "Exception",
                              "Exception " + "w" * 5000 + " timeout at", "short Exception at"]):
        want = S.re_masks(U.U1, line)[0]
        for nseg in (64, 7, 1):
            mask, rounds = logdfa.simulate_segments(t, line, nseg=nseg)
            assert mask == want and rounds <= nseg - 1, (k, nseg)
    assert logdfa.simulate_segments(t, "") == (0, 0)


def test_simulate_segments_worst_case_runs_the_whole_chain(u4):
    hit, miss = U.worst_case_lines()
    assert len(hit.encode()) == len(miss.encode()) == 60000
    assert S.re_masks(U.U4, hit) == [1] and S.re_masks(U.U4, miss) == [0]
    mask, rounds = logdfa.simulate_segments(u4, hit)
    assert mask == 1 and 60 <= rounds <= 63
    assert logdfa.simulate_segments(u4, miss) == (0, 0)  # no state survives a boundary: the first walk is final


# ---- the agent, on CPU: an engine that answers tables= by re ---------------------------------------------------
class ReEngineU(ReEngine):
    def log_tables(self, pats, unbounded=False):
        return logdfa.compile_patterns(pats, unbounded=unbounded)


LOGS = ("2023-04-18T10:00:00Z INFO: starting\n"
        "java.lang.IllegalStateException: pool closed at com.example.Pool.take(Pool.java:41)\n"
        "ERROR: Database initialization failed\n"          # the shipped regex's "Error": no longer a match
        "NullPointerException\n"                            # no "at" after it
        "at startup: Exception\n"                           # the wrong order
        "EXCEPTION in worker 7: request timeout AT stage 2\n"
        "Killed by signal\r\nException\u2028at the next line\n" + "Exception " + "p" * 300 + " at the far end\n")


class OneLog(A.Shim):
    def get_pod_logs(self, pod_name, namespace, container_name=None, tail_lines=100, previous=False):
        return LOGS


def test_agent_unbounded_gives_the_findings_re_gives():
    agent = A.LogsAgent(OneLog(), engine=ReEngineU(), compile_patterns=True, unbounded=True)
    agent.error_patterns = dict(U.U1)
    res = agent.analyze(A.NS)
    assert "error" not in res
    got = [(f["issue"], f["evidence"]) for f in res["findings"] if "in logs" in f["issue"]]
    n_lines, hist, ex = S.re_hist(U.U1, LOGS)
    want = [(f"Detected {n} instances of {P.title(cat)} in logs", "Log entries:\n" + format_examples(e, n))
            for (cat, _), n, e in zip(U.U1, hist, ex) if n]
    n_containers = sum(len(p["spec"]["containers"]) for p in A.Shim().get_pods(A.NS))
    assert got == want * n_containers  # per container, in the dict's order
    assert dict(zip((n for n, _ in U.U1), hist)) == {**{n: 0 for n, _ in U.U1}, "exception": 3, "timeout": 1, "oom_kill": 1}
    assert n_lines == 10 and ex[-1][2].startswith("Exception ppp") and got[-1][1].count("...") == 1  # 200-character cut


GOLD = A.load("logs_unbounded_patterns.json")


def test_golden_masks_equal_re_and_the_table_walk():
    pats = [tuple(p) for p in GOLD["patterns"]]
    assert pats == U.U1
    t = _tables("U1")
    n = 0
    for c in GOLD["containers"]:
        assert S.re_masks(pats, c["text"]) == c["masks"]
        for line, m in zip(c["text"].splitlines(), c["masks"]):
            assert logdfa.simulate(t, line) == m, line
            n += (m >> 12) & 1
    assert n >= 5  # lines the edited category matches


def test_agent_equals_the_reference_with_set_u1():
    agent = A.LogsAgent(A.Shim(), engine=ReEngineU(), compile_patterns=True, unbounded=True)
    agent.error_patterns = dict(U.U1)
    assert A.same(agent.analyze(A.NS), GOLD["mock_cluster"]["result"])
    scan = ReLogScan(U.U1, [c["text"] for c in GOLD["containers"]])
    for i, c in enumerate(GOLD["containers"]):
        agent.reset()
        agent._report_container(scan, i, c["pod"], c["container"], tuple(n for n, _ in U.U1))
        assert A.strip(agent.get_results()) == c["result"], i


def test_agent_without_unbounded_gives_the_pinned_error_text():
    for eng in (ReEngineU(), ReEngine()):  # (ReEngine: log_tables takes one argument, and gets one)
        agent = A.LogsAgent(A.Shim(), engine=eng, compile_patterns=True)
        agent.error_patterns = dict(U.U1)
        res = agent.analyze(A.NS)
        assert "error" in res and "unbounded quantifier '*'" in res["error"] and "exception" in res["error"]
    fixed = A.LogsAgent(A.Shim(), engine=ReEngine(), compile_patterns=True, unbounded=False)
    fixed.error_patterns = dict(S.SETS["A"])
    assert "error" not in fixed.analyze(A.NS)


def test_agent_unbounded_needs_compile_patterns():
    with pytest.raises(ValueError, match="compile_patterns=True"):
        A.LogsAgent(A.Shim(), engine=ReEngineU(), unbounded=True)


def test_stream_takes_log_tables_without_a_gpu():
    """StreamingRCA(log_tables=) / push_logs(tables=) hand the tables to log_scan_device(tables=); without
    them the call is the one-argument form it always was."""
    from krca.stream import StreamingRCA

    class Eng:
        def __init__(self):
            self.calls = []

        def log_scan_device(self, text, doc_off, validate=True, **kw):
            self.calls.append(kw)
            return {}

    s = StreamingRCA.__new__(StreamingRCA)
    s.eng, s.log_tables = Eng(), None
    s.push_logs(b"", [0], templates=False)
    s.push_logs(b"", [0], templates=False, tables="T1")
    s.log_tables = "T0"
    s.push_logs(b"", [0], templates=False)
    s.push_logs(b"", [0], templates=False, tables="T1")
    assert s.eng.calls == [{}, {"tables": "T1"}, {"tables": "T0"}, {"tables": "T1"}]
