"""Trace analytics without a GPU: the bucket helpers of libkrca (host functions), the span encoding,
and TracesAgent's data path on the NumPy restatement (tests/trace_ref.py) against a hand-built
fixture; a client without spans keeps the canned path."""
import ctypes

import numpy as np

import agent_cases as A
import trace_ref
from krca import native, tracecols
from krca.agents.traces import TracesAgent
from trace_ref import NumpyTraceEngine


def boundary_values():
    v = {0, 63, 64, 65, 2 ** 32 - 1}
    for k in range(33):
        v |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    return np.array(sorted(x for x in v if 0 <= x < 2 ** 32), np.uint64)


def _lib_bounds(lib, b):
    lo, hi = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert lib.krca_trace_bucket_bounds(int(b), ctypes.byref(lo), ctypes.byref(hi)) == 0
    return lo.value, hi.value


def test_bucket_helpers():
    lib = native.load_library()
    NB = lib.krca_trace_nbuckets()
    assert NB == 896 == trace_ref.NB
    rng = np.random.default_rng(0)
    rnd = np.concatenate([rng.integers(0, 2 ** 32, 50_000, dtype=np.uint64),
                          (2.0 ** rng.uniform(0, 32, 50_000)).astype(np.uint64)])  # every octave
    d = np.unique(np.concatenate([boundary_values(), np.minimum(rnd, 2 ** 32 - 1)]))
    b = np.array([lib.krca_trace_bucket(int(x)) for x in d.tolist()])
    assert np.array_equal(b, trace_ref.bucket(d))           # library == restatement
    assert (np.diff(b) >= 0).all() and b[0] == 0 and b[-1] == NB - 1   # monotone in d (d ascending)
    bnd = [_lib_bounds(lib, i) for i in range(NB)]
    assert bnd == [trace_ref.bounds(i) for i in range(NB)]
    lo, hi = np.array(bnd, np.int64).T
    assert (lo[b] <= d.astype(np.int64)).all() and (d.astype(np.int64) <= hi[b]).all()
    assert (hi[:-1] + 1 == lo[1:]).all() and lo[0] == 0 and hi[-1] == 2 ** 32 - 1
    assert (32 * (hi[64:] - lo[64:]) < lo[64:]).all()        # hi - lo < lo/32 above 64
    assert (hi[:64] == lo[:64]).all()
    assert lib.krca_trace_bucket_bounds(NB, ctypes.byref(ctypes.c_uint32()), ctypes.byref(ctypes.c_uint32())) != 0
    assert lib.krca_trace_lds_max_slots() >= 1
    assert lib.krca_trace_link_ws_size(1000) >= 12 * 1000 and lib.krca_trace_edge_ws_size(100) >= 12 * 200
    v = ctypes.c_int32(-1)
    assert lib.krca_tune_get(b"KRCA_TRACE_IMPL", ctypes.byref(v)) == 0 and v.value == 0


def test_encode_spans_round_trip():
    gold = A.load("trace_small.json")
    cols = tracecols.encode_spans(gold["traces"])
    assert cols is not None and cols.has_parents and len(cols) == 38
    assert cols.services == gold["expected"]["services"]
    flat = [(t, sp) for t, tr in enumerate(gold["traces"]) for sp in tr["spans"]]
    pos = {(t, sp["id"]): i for i, (t, sp) in enumerate(flat)}
    for i, (t, sp) in enumerate(flat):
        assert cols.services[cols.svc[i]] == sp["service"]
        assert cols.ops[cols.op[i]] == (cols.svc[i], sp["name"])
        assert cols.dur_us[i] == 1000 * sp["duration"] and cols.err[i] == int(sp["error"])
        assert cols.parent[i] == (pos[(t, sp["parentId"])] if "parentId" in sp else -1)
    # a parent outside the window is a root; no parentId anywhere -> has_parents False
    one = [{"spans": [{"id": 1, "parentId": "gone", "name": "x", "service": "a", "duration": 2, "error": True}]}]
    c = tracecols.encode_spans(one)
    assert c.parent.tolist() == [-1] and c.has_parents and c.err.tolist() == [1] and c.dur_us.tolist() == [2000]
    assert not tracecols.encode_spans([{"spans": [{"id": 1, "name": "x", "service": "a", "duration": 2}]}]).has_parents
    # anything that is not plain str / int / bool -> None
    for bad in ({"id": 1, "name": "x", "service": "a", "duration": 2.5}, {"id": 1, "name": "x", "service": 7, "duration": 2},
                {"id": 1, "name": None, "service": "a", "duration": 2}, {"id": (1,), "name": "x", "service": "a", "duration": 2},
                {"id": 1, "name": "x", "service": "a", "duration": 2, "error": "yes"},
                {"id": 1, "name": "x", "service": "a", "duration": -1}, {"id": 1, "name": "x", "service": "a", "duration": 2 ** 40},
                ["not a span"]):
        assert tracecols.encode_spans([{"spans": [bad]}]) is None, bad
    assert tracecols.encode_spans([["not a trace"]]) is None


class TraceClient(A.DictClient):
    """Serves the fixture's traces through get_trace_ids / get_trace_details."""

    def get_trace_ids(self, service_name=None, error_only=False, limit=10):
        return [t["traceId"] for t in self.d["traces"]]

    def get_trace_details(self, trace_id):
        return next(t for t in self.d["traces"] if t["traceId"] == trace_id)


class ColumnsClient(A.DictClient):
    def get_span_columns(self, ns):
        return self.d["cols"]


def test_traces_agent_small_fixture():
    gold = A.load("trace_small.json")
    exp = gold["expected"]
    res = TracesAgent(TraceClient(traces=gold["traces"]), engine=NumpyTraceEngine()).analyze(gold["namespace"])
    assert "error" not in res
    got = A.strip(res)
    assert got["findings"] == exp["findings"]
    assert got["reasoning_steps"] == exp["reasoning_steps"]
    ts = res["trace_stats"]
    assert ts["spans"] == 38 and ts["bad_spans"] == 0 and ts["edges"] == 5
    assert ts["latency_stats"]["db"] == exp["latency_stats_db"]
    deps = ts["service_dependencies"]
    assert sorted((a, b) for a, bs in deps.items() for b in bs) == sorted(map(tuple, exp["edges"]))
    for name, r in exp["error_rate_by_service"].items():
        assert abs(ts["error_rate_by_service"][name] - r) < 1e-6
    # the bulk accessor gives the same result as the dict path
    cols = tracecols.encode_spans(gold["traces"])
    res2 = TracesAgent(ColumnsClient(cols=cols), engine=NumpyTraceEngine()).analyze(gold["namespace"])
    assert A.strip(res2) == got
    # slow operations: "charge" averages (600+550+150+300+380+100+60+90)/8 = 278.75 ms ("GET /stock", 260 ms, stays under 270)
    st = NumpyTraceEngine().trace_analyze(cols)
    slow = st.slow_operations(threshold_ms=270)
    assert [(r["service"], r["operation"]) for r in slow] == [("gateway", "GET /checkout"), ("orders", "create order"),
                                                              ("payments", "charge")]
    assert slow[2]["average_duration_ms"] == 278.75 and slow[2]["count"] == 8 and slow[2]["p95_duration_ms"] == 600.0
    names, rp, col, od = st.dependency_csr()
    assert names == exp["services"] and rp.tolist() == [0, 0, 2, 3, 4, 5] and col.tolist() == [0, 4, 1, 2, 1]
    assert od.tolist() == [1, 2, 1, 0, 1]


def test_client_without_spans_keeps_canned_path():
    """The mock's trace template has no parentId, and a DictClient has no trace accessors at all:
    both give exactly the canned result (the C1 golden), without touching the engine."""
    from krca.mock import MockK8sClient

    class NoEngine:
        def trace_analyze(self, cols):
            raise AssertionError("the canned path must not reach the engine")

    gold = A.load("c1_raw.json")
    res = A.Coordinator(MockK8sClient(), engine=NoEngine()).run_analysis("traces", A.NS)
    res.pop("ranked_root_causes", None)
    assert A.same(res, gold["traces"])
    direct = TracesAgent(MockK8sClient(), engine=NoEngine()).analyze(A.NS)
    assert "trace_stats" not in direct and "error" not in direct
    assert direct["findings"] and not any("spans" in s["observation"] for s in direct["reasoning_steps"])

    class NoParents(TraceClient):
        pass
    spans = [{"spans": [{"id": "a", "name": "x", "service": "s", "duration": 5, "error": False}], "traceId": "t"}]
    res = TracesAgent(NoParents(traces=spans), engine=NoEngine()).analyze("x")
    assert "trace_stats" not in res


def test_make_spans_plants_what_it_says():
    """The generator's planted services stand out in the restatement alone (the GPU end-to-end test
    relies on it): largest self-time p95 at the slow service, whose total p95 is below a caller's;
    most origin errors at the origin service."""
    cols, planted = tracecols.make_spans(3000, 60, seed=5)
    assert len(cols) > 10_000 and (cols.parent >= 0).any() and (cols.parent > np.arange(len(cols))).any()
    st = NumpyTraceEngine().trace_analyze(cols)
    slow, origin = planted["slow"], planted["origin"]
    assert int(np.argmax(st.self_q[:, tracecols.Q95])) == slow
    callers = st.edge_src[st.edge_dst == slow]
    assert len(callers) and st.svc_q[callers, tracecols.Q95].max() > st.svc_q[slow, tracecols.Q95]
    assert int(np.argmax(st.svc_q[:, tracecols.Q95])) != slow
    assert int(np.argmax(st.svc_rec[:, tracecols.R_ORIGIN])) == origin
    # true quantiles (np.sort) bracket the bucketed ones
    true = trace_ref.true_quantiles(cols.svc, cols.dur_us, len(cols.services), tracecols.PERMILLE)
    assert (st.svc_q >= true).all() and (32 * (st.svc_q.astype(np.int64) - true) <= true).all()
