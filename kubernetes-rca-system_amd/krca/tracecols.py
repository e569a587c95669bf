"""Columnar spans and the TracesAgent analyses computed from them (include/krca.h t1).

The reference's TracesAgent emits canned findings (ref:agents/traces_agent.py:209-381: "p95 latency
above 500ms", "5% of traces show HTTP 500", "high latency (>200ms) in calls from service_a to
service_b"); its data-access layer fixes the schemas a trace backend serves
(ref:utils/mock_k8s_client.py:1146-1311).  Here those numbers are measured: the spans are encoded
into columns once, ``engine.trace_analyze(cols)`` (csrc/trace.hip) links children to parents, finds
the call edges and reduces per service / edge / operation, and :func:`analyze` replays the
reference's analyses in its order with the measured values in the evidence.

Columns (``SpanColumns``), one entry per span, ids into per-column tables:
  svc int32 (service that executed the span), parent int32 (index of the parent span in this table;
  -1 = root, or a parent outside the window), op int32 (interned (service, operation name) pair;
  ``ops = [(svc_id, name)]``), dur_us uint32, err uint8 (0 / 1).  Tables: ``services``, ``ops``.
  Optional: start_us int64 (any common origin).  With it ``trace_analyze`` also extracts the critical
  path of every trace (krca_trace_critical): which service each request was waiting on.
"""
import numpy as np

# thresholds of the reference's canned evidence strings (ref:agents/traces_agent.py:209-381)
SERVICE_P95_US = 500_000      # "p95 latency above 500ms"
EDGE_P95_US = 200_000         # "high latency (>200ms) in calls from service_a to service_b"
ERROR_RATE_PCT = 5            # "5% of traces show HTTP 500"
DEPENDENCY_SHARE = 0.5        # an edge carrying more than half of a caller's outgoing calls ...
DEPENDENCY_MIN_CALLEES = 2    # ... of a caller with at least two callees
CRITICAL_SHARE = 0.25         # a service holding more than a quarter of all critical-path time
TOP_FINDINGS = 20             # findings emitted per analysis (the total goes in the reasoning step)
PERMILLE = (500, 900, 950, 990)
Q50, Q90, Q95, Q99 = range(4)
# record words of krca_trace_stats
R_N, R_SUM, R_MAX, R_ERR, R_ORIGIN, R_PROP = range(6)


class SpanColumns:
    """Columnar spans (see module docstring).  ``services`` is a list of str, ``ops`` a list of
    (service id, operation name)."""

    def __init__(self, svc, parent, op, dur_us, err, services, ops, has_parents=True, start_us=None):
        self.svc, self.parent = np.asarray(svc, np.int32), np.asarray(parent, np.int32)
        self.op, self.dur_us = np.asarray(op, np.int32), np.asarray(dur_us, np.uint32)
        self.err = np.asarray(err, np.uint8)
        self.services, self.ops = list(services), list(ops)
        self.has_parents = has_parents  # some span carried a parentId (encode_spans)
        self.start_us = None if start_us is None else np.asarray(start_us, np.int64)  # switches the critical path on

    def __len__(self):
        return len(self.svc)


def _plain_int(x):
    return type(x) in (int, bool)


def encode_spans(traces):
    """Trace dicts shaped like get_trace_details (``spans: [{id, name, service, duration, error}]``
    plus an optional ``parentId``; duration in ms) -> SpanColumns, or None when a value is not a
    plain str / int / bool.  Parent ids resolve to indices within their trace; an unknown parent id
    is a parent outside the window (-1).  ``start_us`` is filled when EVERY span carries an integer
    ``startTime`` (ms, as duration) inside +-2^62 us; otherwise it stays None."""
    svc_t, op_t = {}, {}
    svc, op, dur, err, pid, index = [], [], [], [], [], {}
    start, has_starts = [], True
    has_parents = False
    if type(traces) not in (list, tuple):
        return None
    for t, tr in enumerate(traces):
        if type(tr) is not dict or type(tr.get('spans', [])) not in (list, tuple):
            return None
        for sp in tr.get('spans', []):
            if type(sp) is not dict:
                return None
            sid, name, service = sp.get('id'), sp.get('name', ''), sp.get('service')
            d, e, p = sp.get('duration', 0), sp.get('error', False), sp.get('parentId')
            if type(sid) not in (str, int) or type(name) is not str or type(service) is not str:
                return None
            if not _plain_int(d) or not 0 <= d * 1000 < 2 ** 32 or not _plain_int(e):
                return None
            if p is not None and type(p) not in (str, int):
                return None
            has_parents = has_parents or 'parentId' in sp
            st = sp.get('startTime')
            if has_starts and type(st) is int and -2 ** 62 <= st * 1000 < 2 ** 62:
                start.append(st * 1000)
            else:
                has_starts = False
            s = svc_t.setdefault(service, len(svc_t))
            index[(t, sid)] = len(svc)
            svc.append(s)
            op.append(op_t.setdefault((s, name), len(op_t)))
            dur.append(d * 1000)
            err.append(1 if e else 0)
            pid.append(None if p is None else (t, p))
    parent = [-1 if p is None else index.get(p, -1) for p in pid]
    return SpanColumns(svc, parent, op, dur, err, list(svc_t), list(op_t), has_parents,
                       start if has_starts and svc else None)


def make_spans(n_traces, n_services, seed=0, depth=4, max_calls=3, fanout=3, ops_per_service=3,
               slow_service=None, slow_factor=25.0, origin_service=None, p_origin=0.3, p_propagate=0.6,
               p_background=0.0005, p_internal=0.1, median_us=20000.0, sigma=0.6):
    """Seeded call trees over a service DAG (service s calls only services > s) with log-normal
    SELF times; a span's duration is its self time plus its children's durations.
    Planted: ``slow_service``'s self time is multiplied by ``slow_factor``; errors originate in
    ``origin_service`` with probability ``p_origin`` (elsewhere ``p_background``) and a caller of an
    erroring span errors with probability ``p_propagate``.  Defaults plant mid-DAG services.
    Returns (SpanColumns, dict(slow=..., origin=...))."""
    rng = np.random.default_rng(seed)
    S = int(n_services)
    n_roots = max(1, min(4, S))
    # callees[s]: up to `fanout` distinct services above s (the last service is a leaf)
    callees = [np.sort(rng.choice(np.arange(s + 1, S), size=min(fanout, S - 1 - s), replace=False)) for s in range(S)]
    if slow_service is None or origin_service is None:
        # plant on services that root traffic reaches: a callee of root 0 and a callee of that one
        a = int(callees[0][0]) if len(callees[0]) else 0
        b = int(callees[a][-1]) if len(callees[a]) else a
        slow_service = a if slow_service is None else slow_service
        origin_service = b if origin_service is None else origin_service
    deg = np.array([len(c) for c in callees])
    ctab = np.full((S, max(fanout, 1)), -1, np.int64)
    for s, c in enumerate(callees):
        ctab[s, :len(c)] = c
    levels = []  # (svc, parent index) per level
    svc = rng.integers(0, n_roots, n_traces)
    parent = np.full(n_traces, -1, np.int64)
    base = 0
    while True:
        levels.append((svc, parent, base))
        if len(levels) > depth:
            break
        can_call = deg[svc] > 0
        n_child = np.where(can_call, rng.integers(0, max_calls + 1, len(svc)), 0)
        n_int = (rng.random(len(svc)) < p_internal).astype(np.int64)  # one child span inside the same service
        tot = n_child + n_int
        if tot.sum() == 0:
            break
        par_local = np.repeat(np.arange(len(svc)), tot)
        first = np.cumsum(tot) - tot
        k = np.arange(len(par_local)) - first[par_local]
        psvc = svc[par_local]
        pick = ctab[psvc, rng.integers(0, 1 << 30, len(par_local)) % np.maximum(deg[psvc], 1)]
        internal = k >= n_child[par_local]
        csvc = np.where(internal, psvc, pick)
        nxt_base = base + len(svc)
        svc, parent, base = csvc, par_local + base, nxt_base
    svc_all = np.concatenate([lv[0] for lv in levels])
    par_all = np.concatenate([lv[1] for lv in levels])
    N = len(svc_all)
    self_us = np.exp(rng.normal(np.log(median_us), sigma, N))
    self_us[svc_all == slow_service] *= slow_factor
    self_us = np.maximum(self_us, 1.0).astype(np.int64)
    p_err = np.where(svc_all == origin_service, p_origin, p_background)
    err = rng.random(N) < p_err
    prop = rng.random(N) < p_propagate  # whether this span's error reaches its parent
    dur = self_us.copy()
    for lsvc, lpar, lbase in reversed(levels[1:]):  # children before parents
        sl = slice(lbase, lbase + len(lsvc))
        np.add.at(dur, lpar, dur[sl])
        hit = np.zeros(N, bool)
        hit[lpar[err[sl] & prop[sl]]] = True
        err |= hit
    dur = np.minimum(dur, 2 ** 32 - 1)
    ops = [(s, f"op-{r}") for s in range(S) for r in range(ops_per_service)]
    op = svc_all * ops_per_service + rng.integers(0, ops_per_service, N)
    # shuffle so that parents sit before and after their children
    perm = rng.permutation(N)
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    par_new = np.where(par_all[perm] >= 0, inv[np.maximum(par_all[perm], 0)], -1)
    cols = SpanColumns(svc_all[perm], par_new, op[perm], dur[perm], err[perm],
                       [f"svc-{i:05d}" for i in range(S)], ops)
    return cols, dict(slow=int(slow_service), origin=int(origin_service))


def span_depths(parent):
    """Depth of every span of a parent FOREST (roots = -1 or out of range: depth 0); ValueError on a
    parent cycle."""
    parent = np.asarray(parent, np.int64)
    N = len(parent)
    has = (parent >= 0) & (parent < N) & (parent != np.arange(N))
    depth = np.where(has, -1, 0)
    todo = np.flatnonzero(has)
    while len(todo):
        d = depth[parent[todo]]
        done = d >= 0
        if not done.any():
            raise ValueError("span_depths: the parent links hold a cycle")
        depth[todo[done]] = d[done] + 1
        todo = todo[~done]
    return depth


def add_starts(cols, seed=0, p_parallel=0.0, window_us=600_000_000):
    """SpanColumns (a parent forest, as make_spans gives) -> new SpanColumns with ``start_us`` set so
    that every child's interval lies inside its parent's.  A span's self time is recovered as
    dur - sum of its children's.  A parent drawn "parallel" (probability ``p_parallel``) starts all its
    children together after a head gap, and its duration becomes self + the longest child (durations
    are recomputed bottom-up, so ``dur_us`` shrinks on those chains); the others run their children
    back to back in span order with the self time split into the gaps before, between and after
    them.  Root starts are spread over ``window_us``.  Draws are independent of make_spans'."""
    rng = np.random.default_rng(seed)
    N = len(cols)
    parent = np.asarray(cols.parent, np.int64)
    has = (parent >= 0) & (parent < N) & (parent != np.arange(N))
    depth = span_depths(parent)
    kids = np.flatnonzero(has)
    kpar = parent[kids]
    dur = np.asarray(cols.dur_us, np.int64).copy()
    child_sum = np.zeros(N, np.int64)
    np.add.at(child_sum, kpar, dur[kids])
    self_us = np.maximum(dur - child_sum, 0)
    parallel = rng.random(N) < p_parallel
    levels = [np.flatnonzero(has & (depth == d)) for d in range(1, int(depth.max(initial=0)) + 1)]
    for lv in reversed(levels):  # children before parents: dur = self + (longest | all) children
        acc_sum, acc_max = np.zeros(N, np.int64), np.zeros(N, np.int64)
        np.add.at(acc_sum, parent[lv], dur[lv])
        np.maximum.at(acc_max, parent[lv], dur[lv])
        ps = np.unique(parent[lv])
        dur[ps] = self_us[ps] + np.where(parallel[ps], acc_max[ps], acc_sum[ps])
    if N and int(dur.max()) >= 2 ** 32:  # only where children outlast a parent whose duration was capped
        raise ValueError("add_starts: a recomputed duration does not fit dur_us (uint32)")
    # gaps: integer shares of the parent's self time, one weight per child and one for the tail
    order = kids[np.lexsort((kids, kpar))]  # by parent, then span index
    opar = parent[order]
    weight = rng.integers(1, 1025, len(order))
    tail_w = rng.integers(1, 1025, N)
    wsum = tail_w.copy()
    np.add.at(wsum, opar, weight)
    gap = self_us[opar] * weight // wsum[opar]  # floors: their sum stays within the self time
    first = np.ones(len(order), bool)
    first[1:] = opar[1:] != opar[:-1]
    run = np.cumsum(gap + dur[order]) - dur[order]  # gaps so far + the earlier siblings' durations
    head = np.maximum.accumulate(np.where(first, np.arange(len(order)), 0)) if len(order) else first.astype(np.int64)
    base = (run - gap)[head]  # the running total before each group's first child
    seq_off = run - base
    offset = np.zeros(N, np.int64)
    offset[order] = np.where(parallel[opar], gap[head], seq_off)
    start = np.zeros(N, np.int64)
    roots = np.flatnonzero(~has)
    start[roots] = rng.integers(0, max(int(window_us), 1), len(roots))
    for lv in levels:  # parents before children
        start[lv] = start[parent[lv]] + offset[lv]
    return SpanColumns(cols.svc, cols.parent, cols.op, dur, cols.err, cols.services, cols.ops,
                       getattr(cols, "has_parents", True), start)


class TraceStats:
    """Results of ``engine.trace_analyze``: per service (``svc`` on duration, ``self`` on self
    time), per call edge (``edge``) and per operation (``op``) the (rec int64 [n, 8], q uint32
    [n, 4]) arrays of krca_trace_stats / krca_trace_quantiles, the ascending edge keys
    caller * S + callee, and the reference's four trace schemas built from them.  Columns with
    ``start_us`` add ``crit`` (per service) and ``critedge`` (per call edge) on the critical time of
    the spans on the critical path (krca_trace_critical) and ``n_roots``; absent otherwise."""

    def __init__(self, services, ops, n_spans, n_bad, edge_key, tables, n_roots=None):
        self.services, self.ops = list(services), list(ops)
        self.n_spans, self.n_bad = int(n_spans), int(n_bad)
        self.edge_key = np.asarray(edge_key, np.int64)
        S = max(len(self.services), 1)
        self.edge_src, self.edge_dst = self.edge_key // S, self.edge_key % S
        names = ("svc", "self", "edge", "op")
        if "crit" in tables:
            names += ("crit", "critedge")
            self.n_roots = int(n_roots)
        for name in names:
            rec, q = tables[name]
            setattr(self, f"{name}_rec", np.asarray(rec, np.int64).reshape(-1, 8))
            setattr(self, f"{name}_q", np.asarray(q, np.uint32).reshape(-1, len(PERMILLE)))

    @staticmethod
    def _ms(us):
        return int(us) / 1000

    def latency_stats(self):
        """get_service_latency_stats: {service: {p50, p90, p95, p99, count}} in ms."""
        out = {}
        for s, name in enumerate(self.services):
            n = int(self.svc_rec[s, R_N])
            if n:
                q = self.svc_q[s]
                out[name] = {"p50": self._ms(q[Q50]), "p90": self._ms(q[Q90]), "p95": self._ms(q[Q95]),
                             "p99": self._ms(q[Q99]), "count": n}
        return out

    def error_rates(self):
        """float32 n_err / n per service id (0 where a service has no span)."""
        n = self.svc_rec[:, R_N].astype(np.float32)
        e = self.svc_rec[:, R_ERR].astype(np.float32)
        return np.divide(e, n, out=np.zeros(len(n), np.float32), where=n > 0)

    def error_rate_by_service(self):
        """get_error_rate_by_service: {service: error rate}."""
        return {name: float(r) for name, r in zip(self.services, self.error_rates())}

    def service_dependencies(self):
        """get_service_dependencies: {service: [callees]} (the call graph derived from the spans)."""
        out = {name: [] for name in self.services}
        for a, b in zip(self.edge_src.tolist(), self.edge_dst.tolist()):
            out[self.services[a]].append(self.services[b])
        return out

    def slow_operations(self, threshold_ms=1000):
        """find_slow_operations: operations whose average duration exceeds threshold_ms, slowest
        first: [{service, operation, average_duration_ms, p95_duration_ms, count}]."""
        rows = []
        for o, (s, name) in enumerate(self.ops):
            n = int(self.op_rec[o, R_N])
            if n and int(self.op_rec[o, R_SUM]) > threshold_ms * 1000 * n:
                rows.append((-(int(self.op_rec[o, R_SUM]) / n), o, s, name, n))
        return [{"service": self.services[s], "operation": name, "average_duration_ms": -neg / 1000,
                 "p95_duration_ms": self._ms(self.op_q[o, Q95]), "count": n} for neg, o, s, name, n in sorted(rows)]

    def dependency_csr(self):
        """(names, row_ptr, col, outdeg): the call graph as the pull-CSR Coordinator and
        ``engine.ppr`` take (rows = callees, columns = callers)."""
        from .agents.topology import csr_from_edges
        return (list(self.services),) + csr_from_edges(len(self.services), self.edge_src, self.edge_dst)

    @property
    def has_critical(self):
        return hasattr(self, "crit_rec")

    def critical_path(self):
        """Which service the requests were waiting on: one row per service with spans, by critical
        time descending (ties to the lower id): {service, critical_ms, share, spans_on_path,
        p95_critical_ms, self_ms, hidden_ms}.  share = the service's critical time / all services';
        hidden_ms = sum of self time - sum of critical time: the own time that ran beside something
        slower.  Self time is krca_trace_link's (duration minus ALL children), so the difference is
        exact for sequential traces only: a span that waited on overlapping children has more
        critical than self time."""
        crit, n_on = self.crit_rec[:, R_SUM], self.crit_rec[:, R_N]
        total = int(crit.sum())
        rows = sorted((-int(crit[s]), s) for s in range(len(self.services)) if self.svc_rec[s, R_N] > 0)
        return [{"service": self.services[s], "critical_ms": self._ms(-neg), "share": (-neg / total) if total else 0.0,
                 "spans_on_path": int(n_on[s]), "p95_critical_ms": self._ms(self.crit_q[s, Q95]),
                 "self_ms": self._ms(self.self_rec[s, R_SUM]),
                 "hidden_ms": self._ms(int(self.self_rec[s, R_SUM]) + neg)} for neg, s in rows]

    def summary(self):
        """The additive ``trace_stats`` result key (``critical_path`` only for columns with start_us)."""
        out = {"spans": self.n_spans, "bad_spans": self.n_bad, "services": len(self.services),
               "edges": len(self.edge_key), "latency_stats": self.latency_stats(),
               "error_rate_by_service": self.error_rate_by_service(),
               "service_dependencies": self.service_dependencies(), "slow_operations": self.slow_operations()}
        if self.has_critical:
            out["critical_path"] = self.critical_path()
        return out


def _worst(rows):
    """rows of (value, id tuple, payload) -> (the TOP_FINDINGS worst: descending value, ties to the
    lower id; total)."""
    rows = sorted(rows, key=lambda r: (-r[0], r[1]))
    return rows[:TOP_FINDINGS], len(rows)


def first_cycle(n, src, dst):
    """First cycle of the call graph by the routine TopologyAgent uses (networkx simple_cycles,
    ref:agents/topology_agent.py:262-287), over integer node ids so the order does not depend on
    string hashing; rotated to start at its lowest id.  None when the graph is acyclic."""
    import networkx as nx
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(src, dst))
    cyc = next(iter(nx.simple_cycles(g)), None)
    if cyc:
        k = cyc.index(min(cyc))
        cyc = cyc[k:] + cyc[:k]
    return cyc


def analyze(st, cycle=None):
    """TraceStats -> findings and reasoning steps in the reference's order of analyses
    (ref:agents/traces_agent.py:209-381: latency, errors, dependencies), with its component / issue /
    recommendation strings and measured values in the evidence: a list of ('finding' | 'step', kwargs).
    cycle: None -> first_cycle (networkx, host) finds the call graph's circular dependency; a list of
    service ids -> that cycle is reported and first_cycle is not called; False -> the caller found the
    graph acyclic (NativeEngine.graph_structure), first_cycle is not called either."""
    out = []
    names = st.services
    S = len(names)
    ms = lambda us: f"{int(us) / 1000:.1f}ms"  # noqa: E731

    def step(obs, concl):
        out.append(('step', dict(observation=obs, conclusion=concl)))

    def finding(**kw):
        out.append(('finding', kw))

    src, dst = st.edge_src.tolist(), st.edge_dst.tolist()
    # -- latency (ref :209-260) ---------------------------------------------------------------
    step(f"Checking for high-latency traces in {S} services", "Beginning latency analysis")
    rows = [(int(st.svc_q[s, Q95]), (s,), s) for s in range(S)
            if st.svc_rec[s, R_N] > 0 and st.svc_q[s, Q95] > SERVICE_P95_US]
    top, total = _worst(rows)
    for p95, _, s in top:
        finding(component=f"Service/{names[s]}", issue="High latency detected in service calls", severity="medium",
                evidence=f"Trace analysis shows p95 latency {ms(p95)} (above {SERVICE_P95_US // 1000}ms) over "
                         f"{int(st.svc_rec[s, R_N])} spans; p95 of the service's own time {ms(st.self_q[s, Q95])}",
                recommendation="Optimize database queries, add caching, or scale the service horizontally")
        step(f"Detected high latency in {names[s]} service",
             "Service performance may be affecting overall application responsiveness")
    step(f"{total} of {S} services have p95 latency above {SERVICE_P95_US // 1000}ms",
         f"Reported the {len(top)} slowest")
    rows = [(int(st.edge_q[e, Q95]), (src[e], dst[e]), e) for e in range(len(src)) if st.edge_q[e, Q95] > EDGE_P95_US]
    top, total = _worst(rows)
    for p95, _, e in top:
        a, b = names[src[e]], names[dst[e]]
        finding(component=f"Service/{a}→{b}", issue=f"Slow communication between {a} and {b}", severity="medium",
                evidence=f"Trace analysis shows p95 latency {ms(p95)} (>{EDGE_P95_US // 1000}ms) in "
                         f"{int(st.edge_rec[e, R_N])} calls from {a} to {b}",
                recommendation="Investigate network issues, optimize the API between these services, or consider co-locating them")
        step(f"Detected slow communication between {a} and {b}", "Inter-service communication may be a bottleneck")
    step(f"{total} of {len(src)} call edges have p95 latency above {EDGE_P95_US // 1000}ms",
         f"Reported the {len(top)} slowest")
    # -- errors (ref :262-320) ----------------------------------------------------------------
    step(f"Checking for error traces in {S} services", "Beginning error path analysis")
    rate = st.error_rates()
    rows = [(float(rate[s]), (s,), s) for s in range(S)
            if st.svc_rec[s, R_N] > 0 and 100 * int(st.svc_rec[s, R_ERR]) >= ERROR_RATE_PCT * int(st.svc_rec[s, R_N])]
    top, total = _worst(rows)
    for r, _, s in top:
        n, ne, no = (int(st.svc_rec[s, w]) for w in (R_N, R_ERR, R_ORIGIN))
        finding(component=f"Service/{names[s]}", issue="Error traces detected in service", severity="high",
                evidence=f"{100 * r:.1f}% of spans show errors ({ne} of {n}); {no} of them originate in this service",
                recommendation="Check service logs for corresponding errors and fix the underlying issue")
        step(f"Detected error traces in {names[s]} service",
             "Service is experiencing errors that may affect user experience")
    step(f"{total} of {S} services have an error rate of {ERROR_RATE_PCT}% or more", f"Reported the {len(top)} worst")
    prop = st.edge_rec[:, R_PROP].tolist() if len(src) else []
    into = {}  # b -> [(a, propagated calls a -> b)]
    for e, p in enumerate(prop):
        if p > 0:
            into.setdefault(dst[e], []).append((src[e], p))
    rows = []
    for e, p_bc in enumerate(prop):
        b, c = src[e], dst[e]
        if p_bc > 0 and st.svc_rec[c, R_ORIGIN] > 0:
            rows += [(min(p_ab, p_bc), (a, b, c), (p_ab, p_bc)) for a, p_ab in into.get(b, []) if a != c]
    top, total = _worst(rows)
    for _, (a, b, c), (p_ab, p_bc) in top:
        finding(component=f"Services/{names[a]}→{names[b]}→{names[c]}", issue="Cascading failures detected in service chain",
                severity="critical",
                evidence=f"Errors in {names[c]} are causing failures in {names[b]} and {names[a]}: {p_bc} failed calls "
                         f"{names[b]}→{names[c]} and {p_ab} failed calls {names[a]}→{names[b]} propagated to the caller; "
                         f"{int(st.svc_rec[c, R_ORIGIN])} errors originate in {names[c]}",
                recommendation="Implement circuit breakers and fallback mechanisms to prevent cascading failures")
        step(f"Detected cascading failures from {names[c]} to {names[a]}",
             "Failure isolation mechanisms may be missing in the service architecture")
    step(f"{total} service chains propagate errors to their callers", f"Reported the {len(top)} with the most propagated calls")
    # -- dependencies (ref :322-381) ----------------------------------------------------------
    step(f"Analyzing service dependencies among {S} services", "Beginning dependency analysis")
    calls = st.edge_rec[:, R_N].tolist() if len(src) else []
    out_calls, n_callees = {}, {}
    for e, n in enumerate(calls):
        out_calls[src[e]] = out_calls.get(src[e], 0) + n
        n_callees[src[e]] = n_callees.get(src[e], 0) + 1
    rows = [(n / out_calls[src[e]], (src[e], dst[e]), e) for e, n in enumerate(calls)
            if n_callees[src[e]] >= DEPENDENCY_MIN_CALLEES and n > DEPENDENCY_SHARE * out_calls[src[e]]]
    top, total = _worst(rows)
    for share, _, e in top:
        a, b = names[src[e]], names[dst[e]]
        finding(component=f"Service/{a}", issue=f"High dependency on {b}", severity="medium",
                evidence=f"{a} makes {calls[e]} of its {out_calls[src[e]]} outgoing calls ({100 * share:.1f}%) to {b}, "
                         f"creating a tight coupling",
                recommendation="Consider implementing caching, circuit breakers, or redesigning the interaction pattern")
        step(f"Detected high dependency of {a} on {b}",
             "Service coupling may lead to reliability issues if the dependency fails")
    step(f"{total} call edges carry more than half of their caller's outgoing calls", f"Reported the {len(top)} largest")
    cyc = first_cycle(S, src, dst) if cycle is None else cycle
    if cyc:
        cn = [names[i] for i in cyc]
        finding(component=f"Services/{'↔'.join(cn)}", issue="Circular dependency detected between services",
                severity="high", evidence=f"Traces show a circular call pattern: {' → '.join(cn + [cn[0]])}",
                recommendation="Refactor the service architecture to remove circular dependencies")
        step(f"Detected circular dependency between {', '.join(cn)}",
             "Circular dependencies may lead to deadlocks and complicate scaling")
    # -- critical path (the reference names the duty, ref:agents/mcp_traces_agent.py:175; no canned text) --
    if getattr(st, "crit_rec", None) is not None:
        step(f"Analyzing the critical path of {st.n_roots} requests", "Beginning critical path analysis")
        crit = st.crit_rec[:, R_SUM].tolist()
        all_crit = sum(crit)
        rows = [(crit[s] / all_crit, (s,), s) for s in range(S) if all_crit and crit[s] > CRITICAL_SHARE * all_crit]
        top, total = _worst(rows)
        for share, _, s in top:
            hidden = int(st.self_rec[s, R_SUM]) - crit[s]
            finding(component=f"Service/{names[s]}", issue="Service dominates the critical path of requests",
                    severity="medium",
                    evidence=f"{100 * share:.1f}% of the time requests spent waiting lies in {names[s]}: "
                             f"{ms(crit[s])} on the critical path over {int(st.crit_rec[s, R_N])} spans, "
                             f"{ms(hidden)} of its own time hidden behind slower siblings",
                    recommendation="Optimize this service first: time saved here shortens the requests, "
                                   "time saved off the critical path does not")
            step(f"Detected that {names[s]} dominates the critical path", "Requests are waiting on this service")
        step(f"{total} of {S} services hold more than {100 * CRITICAL_SHARE:.0f}% of the critical path time",
             f"Reported the {len(top)} largest")
    return out
