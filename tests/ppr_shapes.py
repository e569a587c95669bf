"""PageRank step shapes the synthetic meshes never reach, and a host-side replay of a packed plan.

Shared by tests/test_ppr_pack_cpu.py (no GPU: the bytes krca_ppr_pack writes) and
tests/test_gpu_ppr_shapes.py (the same graphs through the device step).

* :func:`replay_plan` restates, in numpy, what csrc/ppr.hip's ppr_step does with one packed plan
  (plan entries, packed columns, lane words: csrc/ppr_pack.cpp) -- stage / sum / update of a short
  block, the per-chunk sum of a long row -- and asserts the layout invariants the kernel relies on.
  A broken invariant raises :class:`PlanError`.
* ``CASES[name]()`` builds a pull-CSR ``(row_ptr, col, outdeg)`` that hits one boundary of the
  plan (row / edge budgets, long-row chunk counts, the dictionary's accept / reject edge, ...), and
  ``PREDICATES[name](packed)`` says whether a packed plan really contains that boundary, so a case
  cannot silently stop hitting it when a budget changes.

Two shapes differ from their first description, because the description could not hold:
``seg_7_9`` uses runs of 7-edge and of 9-edge rows ([7]*200 + [9]*200): alternating 7, 9 sums to 16
and only ever starts a row at edge positions 0 and 7 of a lane, while the runs start rows at every
position 1..7; and the ``dict_*[o]`` cases shift e0 with a leading row of 2048 + o callers (e0 % 4
== o; 2049 + o would give (o + 1) % 4 and never reach e0 % 4 == 1).  ``hub_2048``'s block holds
the one 2,048-edge row and the empty rows behind it (empty rows cost no edge budget), so its
predicate asks for one non-empty row.
"""
import ctypes

import numpy as np

TPB = 256
SEG = 8
EDGE_BUDGET = 2048
ROW_BUDGET = 256
NSLOT = 3 * 3 * 32
PK_PAD = 64  # int32 words native.ppr_pack allocates behind the E packed columns


class PlanError(AssertionError):
    """A layout invariant of (plan, pk, lane) does not hold."""


def _need(cond, *what):
    if not cond:
        raise PlanError(" ".join(str(w) for w in what))


# ---- the exchange layout (csrc/ppr_layout.h) ---------------------------------------------------
def slice_words(n_max):
    return (n_max + 1) // 2 + NSLOT


def remap(j, n_max):
    j = np.asarray(j, np.int64)
    return j + (j // n_max) * (2 * slice_words(n_max) - n_max)


def unmap(v, n_max):
    """Inverse of :func:`remap`; -1 where v is no node's code (a slice's padding or slots)."""
    v = np.asarray(v, np.int64)
    stride = 2 * slice_words(n_max)
    g, off = v // stride, v % stride
    return np.where((v >= 0) & (off < n_max), g * n_max + off, -1)


def dict_words(e0, nu):
    return ((e0 + nu + 3) & ~3) - e0


# ---- packing through the C ABI -----------------------------------------------------------------
class Packed:
    """One krca_ppr_pack result on the host: plan [nblk, 4] int64, pk int32 [E + PK_PAD], lane
    uint16 [nblk, 2, TPB], with the CSR it was packed from."""

    def __init__(self, row_ptr, col, n_max, plan, pk, lane, n_dict):
        self.row_ptr, self.col, self.n_max = row_ptr, col, n_max
        self.plan, self.pk, self.lane, self.n_dict = plan, pk, lane, n_dict
        self.N, self.E = len(row_ptr) - 1, int(row_ptr[-1])

    def copy(self):
        return Packed(self.row_ptr, self.col, self.n_max, self.plan.copy(), self.pk.copy(), self.lane.copy(),
                      self.n_dict)

    @property
    def entries(self):
        """Plan entries as dicts: rb, nu, code, e0, e1, ne, short, nrows (short blocks)."""
        out = []
        for h, code, e0, e1 in self.plan.tolist():
            rb, nu = h & 0xFFFFFFFF, h >> 32
            out.append(dict(rb=rb, nu=nu, code=code, e0=e0, e1=e1, ne=e1 - e0, short=code > 0,
                            nrows=code - rb if code > 0 else 1))
        return out

    def chunks(self):
        """Edge counts of the long-row chunks, in plan order, per long row: {row: [ne, ...]}."""
        out = {}
        for e in self.entries:
            if not e["short"]:
                out.setdefault(e["rb"], []).append(e["ne"])
        return out

    def replay(self, weights):
        return replay_plan(self.row_ptr, self.col, self.plan, self.pk, self.lane, self.n_max, weights)


def bind(lib):
    """ctypes prototypes of the packing entry points (a host-only build or libkrca itself)."""
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.krca_last_error.restype = ctypes.c_char_p
    lib.krca_tune_set.restype = i32
    lib.krca_tune_set.argtypes = [ctypes.c_char_p, i32]
    lib.krca_tune_get.restype = i32
    lib.krca_tune_get.argtypes = [ctypes.c_char_p, ctypes.POINTER(i32)]
    lib.krca_ppr_plan_size.restype = i64
    lib.krca_ppr_plan_size.argtypes = [vp, i64]
    lib.krca_ppr_lane_size.restype = i64
    lib.krca_ppr_lane_size.argtypes = [i64]
    lib.krca_ppr_pack.restype = i64
    lib.krca_ppr_pack.argtypes = [vp, vp, i64, i64, vp, i64, vp, vp]
    lib.krca_ppr_slice_words.restype = i64
    lib.krca_ppr_slice_words.argtypes = [i64]
    return lib


def pack(lib, row_ptr, col, n_max=None, dict_on=1):
    """krca_ppr_pack on host arrays (buffers sized as native.NativeEngine.ppr_pack sizes them),
    with KRCA_PPR_DICT set to dict_on for the call."""
    rp = np.ascontiguousarray(row_ptr, np.int64)
    cl = np.ascontiguousarray(col, np.int32)
    N = len(rp) - 1
    n_max = int(n_max or N)
    old = ctypes.c_int32(0)
    assert lib.krca_tune_get(b"KRCA_PPR_DICT", ctypes.byref(old)) == 0
    assert lib.krca_tune_set(b"KRCA_PPR_DICT", int(dict_on)) == 0
    try:
        n = lib.krca_ppr_plan_size(rp.ctypes.data, N)
        plan = np.zeros(max(n, 4), np.int64)
        pk = np.zeros(len(cl) + PK_PAD, np.int32)
        lane = np.zeros(max(lib.krca_ppr_lane_size(n), 1), np.uint16)
        nd = lib.krca_ppr_pack(rp.ctypes.data, cl.ctypes.data, N, n_max, plan.ctypes.data, n, pk.ctypes.data,
                               lane.ctypes.data)
    finally:
        lib.krca_tune_set(b"KRCA_PPR_DICT", old.value)
    assert nd >= 0, lib.krca_last_error()
    assert lib.krca_ppr_slice_words(n_max) == slice_words(n_max)
    return Packed(rp, cl, n_max, plan[:n].reshape(-1, 4), pk, lane[:n // 4 * 2 * TPB].reshape(-1, 2, TPB), int(nd))


# ---- the replay --------------------------------------------------------------------------------
def replay_plan(row_ptr, col, plan, pk, lane, n_max, weights):
    """What ppr_step computes from one packed plan, on the host.

    row_ptr / col: the pull-CSR the plan was packed from (col: node ids of the exchange layout's
    id space); plan int64 [nblk, 4] (or flat), pk int32 (the packed columns, at least E words),
    lane uint16 [nblk, 2, TPB] (or flat); weights int64, one per node id.  Returns (sums int64 [N],
    updates int64 [N]): row i's pulled sum  sum_{e in row i} weights[col[e]]  as the kernel forms
    it, and how many times the row is updated in one step.  Raises PlanError when an invariant the
    kernel relies on is broken (see the module docstring of tests/test_ppr_pack_cpu.py)."""
    rp = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    N, E = len(rp) - 1, int(rp[-1])
    plan = np.asarray(plan, np.int64).reshape(-1, 4)
    nblk = len(plan)
    lane = np.asarray(lane, np.uint16).reshape(-1)
    _need(lane.size >= nblk * 2 * TPB, "lane words for", nblk, "entries:", lane.size)
    lane = lane[:nblk * 2 * TPB].reshape(nblk, 2, TPB)
    pk = np.asarray(pk, np.int32).reshape(-1)
    _need(pk.size >= E, "pk holds", pk.size, "words for", E, "edges")
    pku = pk.view(np.uint32).astype(np.int64)
    weights = np.asarray(weights, np.int64)
    readable = E + PK_PAD  # what the device buffer holds

    # the gathered table in the exchange layout: a word that is no node's code is poison
    POISON = -(1 << 52)
    top = int(remap(len(weights) - 1, n_max)) + 1
    table = np.full(top, POISON, np.int64)
    table[remap(np.arange(len(weights)), n_max)] = weights

    def gather(cols, where):
        _need(cols.size == 0 or (cols.min() >= 0 and cols.max() < (1 << 30)), where, "column past the 2^30-word table")
        _need(cols.size == 0 or cols.max() < top, where, "column past the exchange table")
        v = table[cols]
        _need(not np.any(v == POISON), where, "column that is no node's code")
        return v

    sums = np.zeros(N, np.int64)
    updates = np.zeros(N, np.int64)
    row, edge = 0, 0  # next row / edge the plan has to cover
    chunk_of = None   # (long row, next chunk index) while inside a long row
    for b in range(nblk):
        h, code, e0, e1 = (int(v) for v in plan[b])
        rb, nu = h & 0xFFFFFFFF, h >> 32
        ne = e1 - e0
        where = f"entry {b}:"
        _need(e0 == edge and 0 <= ne <= EDGE_BUDGET and e1 <= E, where, "edges", (e0, e1), "do not continue", edge)
        edge = e1
        li, rs = lane[b, 0].astype(np.int64), lane[b, 1].astype(np.int64)
        nlane = (ne + SEG - 1) // SEG
        if code <= 0:  # chunk -code of long row rb
            deg = int(rp[rb + 1] - rp[rb]) if 0 <= rb < N else -1
            _need(nu == 0 and rb == row and deg > EDGE_BUDGET, where, "chunk of row", rb, "expected row", row)
            c = 0 if chunk_of is None else chunk_of[1]
            _need(code == -c, where, "chunk code", code, "expected", -c)
            _need(e0 == rp[rb] + c * EDGE_BUDGET and e1 == min(rp[rb + 1], e0 + EDGE_BUDGET), where, "chunk edges")
            _need(not li.any() and np.all(rs == ROW_BUDGET), where, "lane words of a chunk are not empty")
            # load_rows reads 16 bytes per lane at the block's 16-byte-aligned start (unused)
            _need((e0 & ~3) + 4 * nlane <= readable, where, "slot-word read past pk")
            cols = pku[e0:e1]
            _need(np.array_equal(unmap(cols, n_max), col[e0:e1]), where, "packed columns are not the row's")
            sums[rb] += gather(cols, where).sum()
            if e1 == rp[rb + 1]:
                updates[rb] += 1  # the last chunk's ticket
                row, chunk_of = rb + 1, None
            else:
                chunk_of = (rb, c + 1)
            continue
        # short rows [rb, code)
        _need(chunk_of is None, where, "a long row's chunks are incomplete")
        nrows = code - rb
        _need(rb == row and 0 < nrows <= ROW_BUDGET and code <= N, where, "rows", (rb, code), "expected from", row)
        _need(e0 == rp[rb] and e1 == rp[code], where, "edges are not the rows'")
        row = code
        vals = np.zeros(EDGE_BUDGET, np.int64)  # LDS: slots past the staged count hold column 0's value
        if nu > 0:
            dw = dict_words(e0, nu)
            _need((e0 + dw) % 4 == 0, where, "slot words not 16-byte aligned")
            _need(nu <= ne and e0 + nu <= e1, where, "dictionary of", nu, "columns in", ne, "edges")
            dcols = pku[e0:e0 + nu]
            _need(np.all(np.diff(dcols) > 0), where, "distinct columns not ascending")
            vals[:nu] = gather(dcols, where)
            _need(e0 + dw + 4 * nlane <= e1, where, "a lane's 16-byte slot read leaves the block")
            _need(e0 + dw + 4 * nlane <= readable, where, "slot-word read past pk")
            words = pku[e0 + dw:e0 + dw + 4 * nlane]
            slots = np.stack([words & 0xFFFF, words >> 16], axis=1).reshape(nlane, SEG)
            flat = slots.reshape(-1)[:ne]
            _need(flat.size == 0 or flat.max() < nu, where, "slot >= nu")
            _need(np.array_equal(unmap(dcols[flat], n_max), col[e0:e1]), where, "slots do not name the rows' columns")
            c = vals[slots & (EDGE_BUDGET - 1)]
        else:
            cols = pku[e0:e1]
            _need(np.array_equal(unmap(cols, n_max), col[e0:e1]), where, "packed columns are not the rows'")
            _need((e0 & ~3) + 4 * nlane <= readable, where, "slot-word read past pk")
            vals[:ne] = gather(cols, where)
            c = vals[:nlane * SEG].reshape(nlane, SEG)
        # sum: lane t walks its 8 edges; each head bit 1..7 closes a segment and moves to the next slot
        rowsum = np.zeros(ROW_BUDGET + 1, np.int64)
        if nlane:
            k = np.arange(SEG)
            heads = (li[:nlane, None] >> k[None, :]) & 1
            heads[:, 0] = 0  # bit 0 is never tested: edge 8t continues the lane word's slot
            slot = (li[:nlane, None] >> 8) + np.cumsum(heads, axis=1)
            _need(slot.max() <= ROW_BUDGET - 1, where, "sum slot", int(slot.max()), "past", ROW_BUDGET - 1)
            valid = (np.arange(nlane)[:, None] * SEG + k[None, :]) < ne
            np.add.at(rowsum, slot[valid], c[valid])
        # update: lane t owns row rb + t
        deg = np.diff(rp[rb:code + 1])
        _need(np.all(rs[:nrows] <= ROW_BUDGET), where, "row slot past the zero slot")
        _need(np.array_equal(rs[:nrows] == ROW_BUDGET, deg == 0), where, "zero slot <=> row without edges")
        sums[rb:code] += rowsum[rs[:nrows]]
        updates[rb:code] += 1
    _need(chunk_of is None and row == N and edge == E, "plan ends at row", row, "edge", edge, "of", (N, E))
    return sums, updates


def expected_sums(row_ptr, col, weights):
    rp = np.asarray(row_ptr, np.int64)
    want = np.zeros(len(rp) - 1, np.int64)
    np.add.at(want, np.repeat(np.arange(len(rp) - 1), np.diff(rp)), np.asarray(weights, np.int64)[np.asarray(col, np.int64)])
    return want


# ---- case builders -----------------------------------------------------------------------------
def graph(degs, seed, pools=None, n=None):
    """Pull-CSR of rows with `degs` callers: distinct, ascending, never the row itself, drawn from
    all N nodes -- or, for a row in `pools`, from that array of node ids (all of it when the row's
    degree is its length).  n: node count (default len(degs); more adds rows without callers)."""
    degs = np.asarray(list(degs) + [0] * max(0, (n or 0) - len(degs)), np.int64)
    N = len(degs)
    rp = np.zeros(N + 1, np.int64)
    np.cumsum(degs, out=rp[1:])
    col = np.empty(int(rp[-1]), np.int32)
    rng = np.random.default_rng(seed)
    for i in np.nonzero(degs)[0]:
        d = int(degs[i])
        pool = pools.get(int(i)) if pools else None
        if pool is None:
            c = rng.choice(N - 1, d, replace=False)
            c += c >= i
        else:
            c = np.asarray(pool)[rng.choice(len(pool), d, replace=False)]
        col[rp[i]:rp[i + 1]] = np.sort(c)
    return rp, col, np.bincount(col, minlength=N).astype(np.int32)


def _spread(n, nu):
    """nu node ids spread over [0, n): a dictionary's callers, in every rank's slice when sharded."""
    return np.unique(np.linspace(0, n - 1, nu).astype(np.int64))


DICT_N = 2200


def _dict_case(o, ne):
    """A leading row of 2048 + o callers (o > 0: two chunks, and e0 % 4 == o for what follows), then
    three rows of ne edges in all over nu = 32 - o callers: dw = 32 - o, 4 * ceil(ne / 8) = 32."""
    nu = 32 - o
    lead = [EDGE_BUDGET + o] if o else []
    pool = _spread(DICT_N, nu)
    assert len(pool) == nu
    first = len(lead)
    degs = lead + [nu, 16, ne - nu - 16]
    return graph(degs, 100 + 10 * o + ne, {first: pool, first + 1: pool, first + 2: pool}, n=DICT_N)


def _dict_block(p, o, ne):
    """The short block of a dict_* case that starts at e0 % 4 == o with ne edges."""
    hits = [e for e in p.entries if e["short"] and e["ne"] == ne and e["e0"] == (EDGE_BUDGET + o if o else 0)]
    return hits[0] if len(hits) == 1 and hits[0]["e0"] % 4 == o else None


def _nu_of(p, e):
    return len(np.unique(p.col[e["e0"]:e["e1"]]))


def _dict_cost(e, nu):
    return dict_words(e["e0"], nu) + 4 * ((e["ne"] + SEG - 1) // SEG)


def _multi_self():
    """Duplicate edges and self-loops: row i calls itself twice and 38 draws (with repeats) of 24 nodes."""
    rng = np.random.default_rng(77)
    N, d = 96, 40
    rp = np.arange(N + 1, dtype=np.int64) * d
    col = np.concatenate([np.sort(np.concatenate([[i, i], rng.integers(0, 24, d - 2)])) for i in range(N)]).astype(np.int32)
    return rp, col, np.bincount(col, minlength=N).astype(np.int32)


def _tails():
    degs = []
    for k in range(1, 8):
        degs += [5, 11, 8, k] + [0] * 252  # one 256-row block of 24 + k edges
    return graph(degs, 9)


CASES = {
    "hub_2048": lambda: graph([2048] + [0] * 2100, 1),
    "hub_2049": lambda: graph([3, 2049, 1] + [0] * 2100, 2),
    "hub_4096": lambda: graph([4096, 2] + [0] * 4200, 3),
    "hub_4097": lambda: graph([0, 4097] + [1] * 4200, 4),
    "two_hubs": lambda: graph([5000, 0, 3000] + [2] * 6000, 5),
    "hub_last": lambda: graph([2] * 3000 + [2049], 6),
    "rows_256x8": lambda: graph([8] * 256 + [5] * 40, 7),
    "rows_257x8": lambda: graph([8] * 257, 8),
    "rows_256x1": lambda: graph([1] * 259, 10),
    "empty_300": lambda: graph([0] * 300 + [4] * 8, 11),
    "alternate": lambda: graph([0, 1] * 400, 12),
    "seg_7_9": lambda: graph([7] * 200 + [9] * 200, 13),
    "tails": _tails,
    "dict_2048": lambda: graph([1024] + [8] * 128, 14, {i: _spread(1200, 1024) for i in range(129)}, n=1200),
    "multi_self": _multi_self,
}
for _o in range(4):
    CASES[f"dict_tight[{_o}]"] = (lambda o=_o: _dict_case(o, 64 - o))
    CASES[f"dict_miss[{_o}]"] = (lambda o=_o: _dict_case(o, 63 - o))

HUB_CASES = ("hub_2048", "hub_2049", "hub_4096", "hub_4097", "two_hubs", "hub_last")
KNOB_CASES = ("two_hubs", "hub_last", "rows_256x1", "dict_tight[1]", "dict_2048")


def _short(p):
    return [e for e in p.entries if e["short"]]


def _lane_words(p, b, ne):
    return p.lane[b, 0, :(ne + SEG - 1) // SEG].astype(np.int64)


def _head_positions(p):
    pos = set()
    for b, e in enumerate(p.entries):
        if e["short"]:
            for w in _lane_words(p, b, e["ne"]):
                pos |= {k for k in range(1, 8) if (w >> k) & 1}
    return pos


def _p_hub_2048(p):
    deg = np.diff(p.row_ptr)
    return (not p.chunks() and any(e["ne"] == EDGE_BUDGET and e["rb"] == 0 and deg[0] == EDGE_BUDGET and
                                   np.count_nonzero(deg[e["rb"]:e["code"]]) == 1 for e in _short(p)))


def _p_hub_2049(p):
    ent = p.entries
    first = [i for i, e in enumerate(ent) if not e["short"]]
    return (p.chunks() == {1: [2048, 1]} and ent[first[0] - 1]["short"] and ent[first[0] - 1]["ne"] == 3 and
            ent[first[-1] + 1]["short"] and ent[first[-1] + 1]["ne"] == 1)


def _p_two_hubs(p):
    ent = p.entries
    ch = p.chunks()
    last_chunk = max(i for i, e in enumerate(ent) if not e["short"])
    return (sorted(ch) == [0, 2] and sum(len(v) for v in ch.values()) >= 5 and
            sum(e["short"] for e in ent[last_chunk + 1:]) >= 20)


def _p_rows_256x8(p):
    return any(e["nrows"] == ROW_BUDGET and e["ne"] == EDGE_BUDGET for e in _short(p))


def _p_rows_257x8(p):
    ent = p.entries
    return (len(ent) == 2 and ent[0]["nrows"] == ROW_BUDGET and ent[0]["ne"] == EDGE_BUDGET and ent[1]["short"] and
            ent[1]["nrows"] == 1)


def _p_rows_256x1(p):
    e = p.entries[0]
    return (e["short"] and e["nrows"] == 256 and e["ne"] == 256 and np.all(_lane_words(p, 0, 256) & 0xFF == 0xFE) and
            int(p.lane[0, 1, 255]) == 255 and int(_lane_words(p, 0, 256)[31] >> 8) == 248)


def _p_alternate(p):
    e = p.entries[0]
    rs = p.lane[0, 1, :e["nrows"]].astype(np.int64)
    live = rs != ROW_BUDGET
    return e["short"] and live.any() and np.all(rs[live] != np.arange(e["nrows"])[live])


def _p_tails(p):
    got = {e["ne"] % SEG for e in _short(p) if e["ne"] > SEG}
    return got >= set(range(1, 8))


def _p_dict_tight(p, o):
    e = _dict_block(p, o, 64 - o)
    return e is not None and e["nu"] == 32 - o == _nu_of(p, e) and _dict_cost(e, e["nu"]) == e["ne"]


def _p_dict_miss(p, o):
    e = _dict_block(p, o, 63 - o)
    return e is not None and e["nu"] == 0 and _dict_cost(e, _nu_of(p, e)) == e["ne"] + 1


def _p_dict_2048(p):
    e = p.entries[0]
    if not (e["short"] and e["ne"] == EDGE_BUDGET and e["nu"] == 1024 and _dict_cost(e, 1024) == EDGE_BUDGET):
        return False
    words = p.pk.view(np.uint32)[e["e0"] + dict_words(e["e0"], 1024):e["e1"]].astype(np.int64)
    return int(max(words.max() >> 16, (words & 0xFFFF).max())) == 1023


def _p_multi_self(p):
    rows = np.repeat(np.arange(p.N), np.diff(p.row_ptr))
    dup = np.any((np.diff(p.col) == 0) & (np.diff(rows) == 0))
    return bool(dup) and np.any(p.col == rows) and any(0 < e["nu"] < e["ne"] for e in _short(p))


PREDICATES = {
    "hub_2048": _p_hub_2048,
    "hub_2049": _p_hub_2049,
    "hub_4096": lambda p: p.chunks() == {0: [2048, 2048]},
    "hub_4097": lambda p: p.chunks() == {1: [2048, 2048, 1]},
    "two_hubs": _p_two_hubs,
    "hub_last": lambda p: (not p.entries[-1]["short"]) and p.entries[-1]["ne"] == 1 and p.entries[-1]["code"] == -1,
    "rows_256x8": _p_rows_256x8,
    "rows_257x8": _p_rows_257x8,
    "rows_256x1": _p_rows_256x1,
    "empty_300": lambda p: any(e["nrows"] == ROW_BUDGET and e["ne"] == 0 for e in _short(p)),
    "alternate": _p_alternate,
    "seg_7_9": lambda p: _head_positions(p) == set(range(1, 8)),
    "tails": _p_tails,
    "dict_2048": _p_dict_2048,
    "multi_self": _p_multi_self,
}
for _o in range(4):
    PREDICATES[f"dict_tight[{_o}]"] = (lambda p, o=_o: _p_dict_tight(p, o))
    PREDICATES[f"dict_miss[{_o}]"] = (lambda p, o=_o: _p_dict_miss(p, o))
assert PREDICATES.keys() == CASES.keys()

_built = {}


def case(name):
    """The case's (row_ptr, col, outdeg), built once per process and shared: do not write to it."""
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


# the make_graph meshes of the device tests (test_gpu_kernels.py): (n, avg_degree, seed)
MESHES = ((5000, 8, 5000), (20000, 20, 20000), (3000, 3, 3000), (40000, 12, 5))


def plan_stats(p):
    """Long rows, dictionary blocks and tight dictionary blocks of a packed plan."""
    ent = p.entries
    return dict(long_rows=len(p.chunks()), chunks=sum(not e["short"] for e in ent),
                dict_blocks=sum(e["nu"] > 0 for e in ent),
                tight=sum(e["nu"] > 0 and _dict_cost(e, e["nu"]) == e["ne"] for e in ent))


# ---- sharded hub graphs (emulated ranks) --------------------------------------------------------
def shard_case(G):
    """(row_ptr, col, outdeg, bounds): a hub graph and contiguous rank ranges (krca.rca.Partition
    bounds) such that a long row is a rank's first row, another a rank's last row, one rank holds
    only long rows, and the short rows of one rank draw their callers from 24 nodes spread over
    every rank's slice (dictionary blocks whose distinct columns span ranks)."""
    n_short = 700
    if G == 2:
        # rank 0: rows 0..2, all long; rank 1: long first row, short rows, empty rows, long last row
        degs = [2500, 2049, 4097] + [3000] + [6] * n_short + [0] * 3495 + [2600]
        bounds = [0, 3, len(degs)]
        dict_rows = range(4, 4 + n_short)
    elif G == 3:
        # rank 0: short rows, long last row; rank 1: two long rows; rank 2: long first row, short rows
        degs = [6] * n_short + [2600] + [2049, 4097] + [3000] + [3] * 3500
        bounds = [0, n_short + 1, n_short + 3, len(degs)]
        dict_rows = range(0, n_short)
    else:
        raise ValueError(G)
    pool = _spread(len(degs), 24)
    rp, col, od = graph(degs, 40 + G, {i: pool for i in dict_rows})
    return rp, col, od, bounds
