"""Critical path of traces: the reference restatement (tests/trace_critical_ref.py) on hand cases with
the answers written out, and the host logic around it (add_starts, encode_spans, TraceStats, the
agent).  The device kernel is checked against the same restatement in test_gpu_trace_critical.py."""
import copy

import numpy as np
import pytest

import agent_cases as A
import trace_critical_ref as R
from krca import tracecols
from krca.agents.traces import TracesAgent
from test_trace_cpu import ColumnsClient

SEL, ON, ROOT = R.SELECTED, R.ON_PATH, R.ROOT


def run(spans, S=3, **kw):
    """spans: [(parent, start, dur)] -> (crit list, path list)."""
    parent, start, dur = zip(*spans)
    crit, path, n_bad = R.critical(np.zeros(len(spans), np.int32), parent, start, dur, S, **kw)
    assert n_bad == 0
    return crit.tolist(), path.tolist()


def test_sequential_children():
    crit, path = run([(-1, 0, 100), (0, 10, 20), (0, 40, 50)])
    assert crit == [30, 20, 50]
    assert path == [ROOT | ON, SEL | ON, SEL | ON]


def test_parallel_children_hide_the_earlier_one():
    crit, path = run([(-1, 0, 100), (0, 10, 50), (0, 20, 70)])
    assert crit == [30, 0, 70]
    assert path == [ROOT | ON, 0, SEL | ON]


def test_equal_ends_take_the_earlier_start():
    crit, path = run([(-1, 0, 100), (0, 10, 40), (0, 30, 20)])
    assert path == [ROOT | ON, SEL | ON, 0] and crit == [60, 40, 0]
    crit, path = run([(-1, 0, 100), (0, 30, 20), (0, 10, 40)])  # whichever comes first in the table
    assert path == [ROOT | ON, 0, SEL | ON] and crit == [60, 0, 40]


def test_identical_intervals_take_the_lower_index():
    crit, path = run([(1, 10, 40), (-1, 0, 100), (1, 10, 40)])
    assert path == [SEL | ON, ROOT | ON, 0] and crit == [40, 60, 0]


def test_overrunning_child_keeps_its_own_time():
    crit, path = run([(-1, 0, 100), (0, 50, 100)])
    assert crit == [50, 100] and path == [ROOT | ON, SEL | ON]
    assert sum(crit) > 100  # the stated exception to the sum property
    # a child wholly outside its parent is clipped to nothing
    crit, path = run([(-1, 0, 100), (0, 100, 10), (0, -20, 20)])
    assert crit == [100, 0, 0] and path == [ROOT | ON, 0, 0]


def test_zero_length_child_is_never_selected():
    crit, path = run([(-1, 0, 100), (0, 50, 0), (0, 100, 0), (0, 20, 30)])
    assert path == [ROOT | ON, 0, 0, SEL | ON] and crit == [70, 0, 0, 30]


def test_two_cycle_is_off_the_path():
    crit, path = run([(1, 5, 10), (0, 5, 10), (-1, 0, 50)])
    assert path == [SEL, SEL, ROOT | ON] and crit == [0, 0, 50]  # each selected by the other, neither reaches a root


def test_grandchildren_need_every_link_selected():
    # root [0,100): A [0,40) hidden behind B [10,100); A's child is selected by A but off the path
    crit, path = run([(-1, 0, 100), (0, 0, 40), (0, 10, 90), (1, 5, 20), (2, 20, 30)])
    assert path == [ROOT | ON, 0, SEL | ON, SEL, SEL | ON]
    assert crit == [10, 0, 60, 0, 30] and sum(crit) == 100


def test_chain_deeper_than_the_limit():
    n = R.D + 2
    spans = [(i - 1, 0, 10) for i in range(n)]  # span i at depth i, every link selected
    crit, path = run(spans)
    assert path[0] == ROOT | ON and all(b == SEL | ON for b in path[1:R.D + 1])
    assert path[R.D + 1] == SEL and crit[R.D + 1] == 0  # depth D + 1: selected, off the path
    assert crit[R.D] == 0  # its only child is off the path but still SELECTED: no own time left
    crit, path = run(spans[:6], max_depth=3)
    assert path == [ROOT | ON, SEL | ON, SEL | ON, SEL | ON, SEL, SEL]


def test_bad_spans():
    svc = np.array([0, 5, 0, 0, -1], np.int32)
    parent = np.array([-1, 0, 1, 0, 0], np.int32)
    start = np.array([0, 0, 0, 2 ** 62, 0], np.int64)
    crit, path, n_bad = R.critical(svc, parent, start, np.full(5, 10, np.uint32), 3)
    assert n_bad == 3 and path.tolist() == [ROOT | ON, 0, ROOT | ON, 0, 0]  # a bad parent is no parent
    assert crit.tolist() == [10, 0, 10, 0, 0]
    start[3] = -2 ** 62  # the lowest valid start
    _, path, n_bad = R.critical(svc, parent, start, np.full(5, 10, np.uint32), 3)
    assert n_bad == 2 and path[3] == 0 and path[0] == ROOT | ON  # clipped to nothing, not bad


# ---- add_starts -------------------------------------------------------------------------------
@pytest.mark.parametrize("p_parallel", [0.0, 0.5])
def test_add_starts_nests_and_the_critical_times_sum_to_the_roots(p_parallel):
    base, _ = tracecols.make_spans(400, 30, seed=5)
    cols = tracecols.add_starts(base, seed=1, p_parallel=p_parallel)
    assert cols.start_us.dtype == np.int64 and base.start_us is None
    assert R.nested(cols)
    assert np.array_equal(cols.parent, base.parent) and np.array_equal(cols.svc, base.svc)
    if p_parallel == 0:
        assert np.array_equal(cols.dur_us, base.dur_us)
    else:
        assert (cols.dur_us <= base.dur_us).all() and (cols.dur_us < base.dur_us).any()
    crit, path, n_bad = R.critical(cols.svc, cols.parent, cols.start_us, cols.dur_us, len(cols.services))
    roots = (path & ROOT) != 0
    assert n_bad == 0 and roots.sum() == 400
    assert int(crit.astype(np.int64).sum()) == int(cols.dur_us[roots].astype(np.int64).sum())
    # per trace, not only in total
    top = np.arange(len(cols))
    for _ in range(8):
        top = np.where(cols.parent[top] >= 0, cols.parent[top], top)
    per_trace = np.bincount(top, crit.astype(np.int64), len(cols))
    assert np.array_equal(per_trace[roots], cols.dur_us[roots])
    if p_parallel == 0:
        assert ((path & ON) != 0).all()  # back to back: everything is waited for
    else:
        assert 0 < ((path & ON) == 0).sum()
    again = tracecols.add_starts(base, seed=1, p_parallel=p_parallel)
    assert np.array_equal(again.start_us, cols.start_us) and np.array_equal(again.dur_us, cols.dur_us)


def test_make_spans_is_unchanged_by_the_new_column():
    a, _ = tracecols.make_spans(50, 9, seed=2)
    assert a.start_us is None


# ---- encode_spans -----------------------------------------------------------------------------
def _trace(starts):
    spans = [{"id": "a", "name": "GET /", "service": "web", "duration": 100},
             {"id": "b", "name": "q", "service": "db", "duration": 30, "parentId": "a"},
             {"id": "c", "name": "q", "service": "db", "duration": 50, "parentId": "a"}]
    for sp, st in zip(spans, starts):
        if st != "absent":
            sp["startTime"] = st
    return [{"spans": spans}]


def test_encode_spans_with_and_without_start_time():
    cols = tracecols.encode_spans(_trace([1000, 1010, 1040]))
    assert cols.start_us.tolist() == [1_000_000, 1_010_000, 1_040_000] and cols.start_us.dtype == np.int64
    crit, path, _ = R.critical(cols.svc, cols.parent, cols.start_us, cols.dur_us, 2)
    assert crit.tolist() == [20_000, 30_000, 50_000]
    none = tracecols.encode_spans(_trace(["absent"] * 3))
    assert none.start_us is None and np.array_equal(none.dur_us, cols.dur_us) and np.array_equal(none.parent, cols.parent)
    for odd in ("absent", None, 1.5, "1010", True, 2 ** 62):  # one span without an integer start in range: no column
        part = tracecols.encode_spans(_trace([1000, odd, 1040]))
        assert part is not None and part.start_us is None and len(part) == 3
    assert tracecols.encode_spans(_trace([-5, 0, 2 ** 62 // 1000])).start_us.tolist() == [-5000, 0, 2 ** 62 // 1000 * 1000]
    assert tracecols.encode_spans([]).start_us is None


# ---- TraceStats / analyze / agent -------------------------------------------------------------
def _planted():
    """One request shape, 40 times: gateway calls 'slow' [0, 80) and 'decoy' [0, 60) together, then
    'tail' [80, 90) -- the decoy never delays a request."""
    svc, parent, start, dur = [], [], [], []
    for t in range(40):
        r, t0 = len(svc), 1000 * t
        svc += [0, 1, 2, 3]
        parent += [-1, r, r, r]
        start += [t0, t0, t0, t0 + 80_000]
        dur += [100_000, 80_000, 60_000, 10_000]
    n = len(svc)
    return tracecols.SpanColumns(svc, parent, svc, dur, np.zeros(n, np.uint8), ["gateway", "slow", "decoy", "tail"],
                                 [(i, "op") for i in range(4)], start_us=start)


def test_critical_path_rows_and_summary():
    st = R.NumpyTraceEngine().trace_analyze(_planted())
    assert st.n_roots == 40
    rows = st.critical_path()
    assert [r["service"] for r in rows] == ["slow", "gateway", "tail", "decoy"]
    slow, gw, tail, decoy = rows
    assert slow == {"service": "slow", "critical_ms": 3200.0, "share": 0.8, "spans_on_path": 40,
                    "p95_critical_ms": 80.0, "self_ms": 3200.0, "hidden_ms": 0.0}
    assert gw["critical_ms"] == 400.0 and gw["share"] == 0.1 and gw["self_ms"] == 0.0 and gw["hidden_ms"] == -400.0
    assert tail["critical_ms"] == 400.0 and tail["spans_on_path"] == 40
    assert decoy == {"service": "decoy", "critical_ms": 0.0, "share": 0.0, "spans_on_path": 0,
                     "p95_critical_ms": 0.0, "self_ms": 2400.0, "hidden_ms": 2400.0}
    assert st.summary()["critical_path"] == rows
    # the call edges on the path: gateway -> slow and gateway -> tail, never gateway -> decoy
    on_edges = {(int(a), int(b)): int(n) for a, b, n in zip(st.edge_src, st.edge_dst, st.critedge_rec[:, tracecols.R_N])}
    assert on_edges == {(0, 1): 40, (0, 2): 0, (0, 3): 40}


def test_agent_reports_the_service_that_dominates_the_critical_path():
    res = TracesAgent(ColumnsClient(cols=_planted()), engine=R.NumpyTraceEngine()).analyze("mesh")
    assert "error" not in res
    hits = [f for f in res["findings"] if f["issue"] == "Service dominates the critical path of requests"]
    assert [f["component"] for f in hits] == ["Service/slow"] and hits[0]["severity"] == "medium"
    assert "80.0%" in hits[0]["evidence"] and "3200.0ms" in hits[0]["evidence"] and "40 spans" in hits[0]["evidence"]
    steps = [s["observation"] for s in res["reasoning_steps"]]
    assert "Analyzing the critical path of 40 requests" in steps
    assert steps[-1] == "1 of 4 services hold more than 25% of the critical path time"
    assert steps.index("Analyzing the critical path of 40 requests") > steps.index(
        "Analyzing service dependencies among 4 services")
    assert res["trace_stats"]["critical_path"][0]["service"] == "slow"


def test_columns_without_starts_analyze_as_before():
    """Same call on a copy with the attribute removed: the result of today's code path."""
    cols, _ = tracecols.make_spans(300, 12, seed=3)
    assert cols.start_us is None
    old = copy.copy(cols)
    del old.start_us
    eng = R.NumpyTraceEngine()
    a, b = eng.trace_analyze(cols), eng.trace_analyze(old)
    assert not a.has_critical and not hasattr(a, "crit_rec") and not hasattr(a, "n_roots")
    assert repr(a.summary()) == repr(b.summary()) and "critical_path" not in a.summary()
    assert repr(tracecols.analyze(a)) == repr(tracecols.analyze(b))
    ra = TracesAgent(ColumnsClient(cols=cols), engine=eng).analyze("mesh")
    rb = TracesAgent(ColumnsClient(cols=old), engine=eng).analyze("mesh")
    assert repr(A.strip(ra)) == repr(A.strip(rb)) and repr(ra["trace_stats"]) == repr(rb["trace_stats"])
    # and with starts, everything that was there before is still there, unchanged
    c = eng.trace_analyze(tracecols.add_starts(cols))
    sc = c.summary()
    assert list(sc)[:-1] == list(a.summary()) and list(sc)[-1] == "critical_path"
    assert {k: v for k, v in sc.items() if k != "critical_path"} == a.summary()
    assert tracecols.analyze(c)[:len(tracecols.analyze(a))] == tracecols.analyze(a)
