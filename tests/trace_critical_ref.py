"""Plain Python / NumPy restatement of krca_trace_critical (include/krca.h t1): the checker of
csrc/trace_critical.hip.  Per-parent loops, no cleverness."""
import numpy as np

import trace_ref
from krca import tracecols

D = 4096          # krca_trace_critical_max_depth()
LIM = 2 ** 62
SELECTED, ON_PATH, ROOT = 1, 2, 4


def critical(svc, parent, start_us, dur_us, S, max_depth=D):
    """-> (crit_us uint32[N], path uint8[N], n_bad)."""
    svc = [int(x) for x in np.asarray(svc)]
    parent = [int(x) for x in np.asarray(parent)]
    start = [int(x) for x in np.asarray(start_us)]
    dur = [int(x) for x in np.asarray(dur_us)]
    N = len(svc)
    bad = [not (0 <= svc[i] < S and -LIM <= start[i] < LIM) for i in range(N)]
    vp = [-1] * N  # the valid parent, -1 = none
    children = [[] for _ in range(N)]
    for i in range(N):
        p = parent[i]
        if not bad[i] and 0 <= p < N and p != i and not bad[p]:
            vp[i] = p
            children[p].append(i)
    root = [not bad[i] and vp[i] < 0 for i in range(N)]
    selected = [False] * N
    taken = [0] * N  # sum of the selected children's clipped pieces
    for p in range(N):
        if bad[p] or not children[p]:
            continue
        s_p, e_p = start[p], start[p] + dur[p]
        pieces = []
        for c in children[p]:
            cs, ce = max(start[c], s_p), min(start[c] + dur[c], e_p)
            if ce > cs:
                pieces.append((cs, ce, c))
        cursor = e_p
        while True:
            ok = [(-ce, cs, c) for cs, ce, c in pieces if ce <= cursor]
            if not ok:
                break
            nce, cs, c = min(ok)  # largest ce, then smallest cs, then lowest index
            selected[c] = True
            taken[p] += -nce - cs
            cursor = cs
    crit = np.zeros(N, np.uint32)
    path = np.zeros(N, np.uint8)
    for i in range(N):
        if bad[i]:
            continue
        on = root[i]
        if not on and selected[i]:
            a = vp[i]
            for _ in range(max_depth):  # a = the k-th valid ancestor, k = 1 .. max_depth
                if root[a]:
                    on = True
                    break
                if not selected[a]:
                    break
                a = vp[a]
        path[i] = (SELECTED if selected[i] else 0) | (ON_PATH if on else 0) | (ROOT if root[i] else 0)
        if on:
            crit[i] = dur[i] - taken[i]
    return crit, path, sum(bad)


def nested(cols):
    """Every valid child's interval lies inside its parent's."""
    p = np.asarray(cols.parent, np.int64)
    has = p >= 0
    s, e = cols.start_us, cols.start_us + cols.dur_us.astype(np.int64)
    return bool((s[has] >= s[p[has]]).all() and (e[has] <= e[p[has]]).all())


def critical_tables(cols, link_out, edge_slot, n_edges, prev=None):
    """The two critical-path tables of trace_analyze: name -> (rec, hist) and the number of roots."""
    S = len(cols.services)
    crit, path, _ = critical(cols.svc, cols.parent, cols.start_us, cols.dur_us, S)
    on = (path & ON_PATH) != 0
    flags = link_out[2]
    out = {}
    for name, slot, n in (("crit", np.where(on, cols.svc, -1), S), ("critedge", np.where(on, edge_slot, -1), n_edges)):
        out[name] = trace_ref.stats(slot, crit, flags, n, None if prev is None else prev[name])
    return out, int(((path & ROOT) != 0).sum())


class NumpyTraceEngine(trace_ref.NumpyTraceEngine):
    """Host engine whose trace_analyze adds the critical tables for columns with start_us."""

    def trace_analyze(self, cols):
        st = super().trace_analyze(cols)
        if getattr(cols, "start_us", None) is None:
            return st
        S = len(cols.services)
        lk = trace_ref.link(cols.svc, cols.parent, cols.dur_us, cols.err, S)
        edge_key, edge_slot = trace_ref.edges(lk[0], cols.svc, S)
        tabs, n_roots = critical_tables(cols, lk, edge_slot, len(edge_key))
        tables = {name: (getattr(st, name + "_rec"), getattr(st, name + "_q")) for name in ("svc", "self", "edge", "op")}
        for name, (rec, hist) in tabs.items():
            tables[name] = (rec, trace_ref.quantiles(rec, hist, tracecols.PERMILLE))
        return tracecols.TraceStats(cols.services, cols.ops, len(cols), st.n_bad, edge_key, tables, n_roots)
