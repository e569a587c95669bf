"""Log-template novelty without a GPU: the host restatement (tests/template_novelty_ref.py) on a hand
case with every expected record written out, the host-side contract of the C entry points (sizes,
KRCA_EINVAL before any device work), the Python mirror of the table layout and the home-slot function
against the library, the report's sort order, and the StreamingRCA surface (refusal for world > 1,
snapshot keys unchanged without novelty)."""
import ctypes
import json

import numpy as np
import pytest

import template_novelty_ref as R
from krca import native, novelty


def arrays(docs, gaps=0):
    """docs: per container a list of (hash, count) -> (tmpl_hash u64, tmpl_count, n_templates, doc_line0);
    `gaps` unused slots after every container."""
    th, tc, nt, d0 = [], [], [], []
    for ent in docs:
        d0.append(len(th))
        nt.append(len(ent))
        th += [h for h, _ in ent] + [0] * gaps
        tc += [c for _, c in ent] + [0] * gaps
    return (np.array(th, np.uint64), np.array(tc, np.int32), np.array(nt, np.int32), np.array(d0, np.int64))


A, B, C = 0xA, 0xB, 0xC


# ---- the restatement alone -------------------------------------------------------------------------
def test_hand_case_three_windows():
    """surge_ratio 4, surge_min 8.  Window 0: A (2 + 1 lines in containers 0, 2) and B (10 lines) are novel.
    Window 1: A again with 12 lines: 12 * (1 - 0) = 12 >= 4 * 3 -- a surge at equality; B with 39 lines:
    39 * 1 < 4 * 10 -- one line below, no surge; C is novel in container 1.  Window 2: B with 98 lines:
    98 * 2 = 196 = 4 * 49 -- equality again; A with 7 lines is below surge_min."""
    ref = R.NoveltyRef(ttl=0, surge_ratio=4, surge_min=8)
    w0 = ref.update(*arrays([[(A, 2)], [(B, 10)], [(A, 1)]]), None, 0)
    assert w0.counts == [3, 2, 2, 0, 2, 2]
    assert w0.report == [(A, 0, 1, 3, 2, 0, 0, 0), (B, 0, 1, 10, 1, 1, 0, 0)]
    assert w0.doc_novel.tolist() == [1, 1, 1] and w0.doc_surge.tolist() == [0, 0, 0]
    assert ref.records() == {(0, A): (0, 0, 1, 3), (0, B): (0, 0, 1, 10)}
    w1 = ref.update(*arrays([[(A, 12), (B, 39)], [(C, 1)], []]), None, 1)
    assert w1.counts == [3, 3, 1, 1, 2, 3]
    assert w1.report == [(A, 0, 2, 12, 1, 0, 0, 3), (C, 0, 1, 1, 1, 1, 1, 0)]
    assert w1.doc_novel.tolist() == [0, 1, 0] and w1.doc_surge.tolist() == [1, 0, 0]
    assert ref.records() == {(0, A): (0, 1, 2, 15), (0, B): (0, 1, 2, 49), (0, C): (1, 1, 1, 1)}
    w2 = ref.update(*arrays([[], [(B, 98), (A, 7)], []]), None, 2)
    assert w2.counts == [2, 2, 0, 1, 1, 3]
    assert w2.report == [(B, 0, 2, 98, 1, 1, 0, 49)]
    assert w2.doc_novel.tolist() == [0, 0, 0] and w2.doc_surge.tolist() == [0, 1, 0]
    assert ref.records() == {(0, A): (0, 2, 3, 22), (0, B): (0, 2, 3, 147), (0, C): (1, 1, 1, 1)}
    # one line below the equality of window 2
    ref = R.NoveltyRef(0, 4, 8)
    ref.update(*arrays([[(B, 10)]]), None, 0)
    ref.update(*arrays([[(B, 39)]]), None, 1)
    assert ref.update(*arrays([[(B, 97)]]), None, 2).report == []


def test_expiry_groups_and_learn_only():
    # ttl = 3: seen at window 0, again at 3 (last_win 0 >= 3 - 3: present), then at 7 (3 < 7 - 3: expired)
    for ttl, want in ((3, [(A, 0, 1, 5, 1, 0, 7, 0)]), (0, [])):
        ref = R.NoveltyRef(ttl=ttl, surge_ratio=4, surge_min=100)
        assert len(ref.update(*arrays([[(A, 5)]]), None, 0).report) == 1
        assert ref.update(*arrays([[(A, 5)]]), None, 3).report == []
        assert ref.update(*arrays([[(A, 5)]]), None, 7).report == want
        assert ref.records() == {(0, A): (7, 7, 1, 5) if ttl else (0, 7, 3, 15)}
    # the same hash in two groups is two keys; a negative group has no entries; count <= 0 is no entry
    ref = R.NoveltyRef()
    w = ref.update(*arrays([[(A, 1)], [(A, 2)], [(A, 4), (B, 0)], [(A, 8)]]), np.array([0, 1, 0, -1], np.int32), 0)
    assert w.counts == [3, 2, 2, 0, 2, 2] and w.report == [(A, 0, 1, 5, 2, 0, 0, 0), (A, 1, 1, 2, 1, 1, 0, 0)]
    assert w.doc_novel.tolist() == [1, 1, 1, 0]
    # learn-only: the record is committed, nothing is flagged; the next window knows the template
    ref = R.NoveltyRef()
    w = ref.update(*arrays([[(A, 3)]]), None, 0, report=False)
    assert w.counts == [1, 1, 0, 0, 0, 1] and w.report == [] and w.doc_novel.tolist() == [0]
    assert ref.update(*arrays([[(A, 3)]]), None, 1).report == []
    # the empty marker is counted under marker - 1; entries past the arrays' end are not read
    ref = R.NoveltyRef()
    th, tc, nt, d0 = arrays([[(R.EMPTY_HASH, 1)], [(R.EMPTY_HASH - 1, 2)], [(0, 1)]])
    nt[2] = 5
    w = ref.update(th, tc, nt, d0, None, 0)
    assert w.report == [(0, 0, 1, 1, 1, 2, 0, 0), (R.EMPTY_HASH - 1, 0, 1, 3, 2, 0, 0, 0)]
    ref.compact(1)
    assert ref.records() == {}


# ---- the C entry points on the host ----------------------------------------------------------------
def test_state_size_and_layout_mirror():
    lib = native.load_library()
    sizes = [lib.krca_template_novelty_state_size(1 << k) for k in range(6, 31)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] >= 256 + 64 * (64 + 4)
    for bad in (0, -64, 63, 96, 32, (1 << 30) + 1, 1 << 31):
        assert lib.krca_template_novelty_state_size(bad) == 0
    assert lib.krca_template_novelty_layout(0) == novelty.HEADER_DTYPE.itemsize == 256
    assert lib.krca_template_novelty_layout(1) == novelty.SLOT_DTYPE.itemsize == 64
    assert lib.krca_template_novelty_layout(2) == novelty.REPORT_DTYPE.itemsize == 48
    assert lib.krca_template_novelty_layout(3) == 40 and lib.krca_template_novelty_layout(4) == (1 << 24) - 1
    assert lib.krca_template_novelty_layout(99) == -1
    for cap in (64, 128, 1 << 20):
        assert lib.krca_template_novelty_state_size(cap) == novelty.state_size(cap)
    rng = np.random.default_rng(3)
    hashes = [0, 1, novelty.EMPTY_HASH, novelty.EMPTY_HASH - 1, 1 << 63] + [int(h) for h in rng.integers(0, 1 << 63, 200)]
    for h in hashes:
        for g in (0, 1, 7, (1 << 31) - 1):
            for cap in (64, 128, 1 << 20, 1 << 30):
                assert lib.krca_template_novelty_home_slot(h, g, cap) == novelty.home_slot(h, g, cap), (h, g, cap)
    assert novelty.home_slot(novelty.EMPTY_HASH, 2, 128) == novelty.home_slot(novelty.EMPTY_HASH - 1, 2, 128)
    assert lib.krca_template_novelty_home_slot(5, -1, 64) == -1 and lib.krca_template_novelty_home_slot(5, 0, 65) == -1
    assert novelty.remap(novelty.EMPTY_HASH) == R.remap(R.EMPTY_HASH) == R.EMPTY_HASH - 1


def test_invalid_arguments_need_no_device():
    """Every refusal comes before any device work: the pointers are never touched (they are bogus)."""
    lib = native.load_library()
    bogus = ctypes.c_void_p(4096)
    counts = (ctypes.c_int64 * 6)()

    def update(n_lines=10, ndocs=4, window=0, ttl=0, ratio=4, smin=8, report=1, rep=bogus, cap=16, state=bogus, cnt=counts):
        return lib.krca_template_novelty_update(state, bogus, bogus, n_lines, bogus, bogus, None, ndocs, window, ttl, ratio,
                                                smin, report, rep, cap, None, None, cnt, None)
    for kw in (dict(ndocs=-1), dict(window=-1), dict(ttl=-1), dict(cap=-1), dict(n_lines=-1), dict(ratio=0), dict(smin=0),
               dict(rep=None), dict(ndocs=1 << 24), dict(state=None), dict(cnt=None)):
        assert update(**kw) == -22, kw
        assert b"krca_template_novelty_update" in lib.krca_last_error()
    for cap in (0, 63, 96, -128, (1 << 30) + 1, 1 << 31):
        assert lib.krca_template_novelty_init(bogus, cap, None) == -22
        assert lib.krca_template_novelty_rehash(bogus, ctypes.c_void_p(8192), cap, 0, None) == -22
    assert lib.krca_template_novelty_init(None, 64, None) == -22
    assert lib.krca_template_novelty_rehash(bogus, bogus, 64, 0, None) == -22  # aliased


# ---- the Python surface ----------------------------------------------------------------------------
def test_report_sort_order_and_fields():
    rec = novelty.NoveltyRecord
    rs = [rec(9, 1, 1, 5, 1, 3, 2, 0), rec(4, 1, 2, 5, 1, 0, 0, 3), rec(7, 0, 1, 5, 2, 1, 2, 0), rec(1, 3, 1, 70, 1, 9, 2, 0),
          rec(2, 0, 2, 1, 1, 0, 1, 0)]
    order = [(r.cur_lines, r.group, r.hash) for r in novelty.sort_records(rs)]
    assert order == [(70, 3, 1), (5, 0, 7), (5, 1, 4), (5, 1, 9), (1, 0, 2)]
    rep = novelty.NoveltyReport(2, [9, 5, 3, 2, 7, 5], rs, None, None)
    assert [r.hash for r in rep.novel] == [1, 7, 9] and [r.hash for r in rep.surged] == [4, 2]
    assert rep.truncated and rep.counts["n_reported"] == 7 and rep.counts["n_live_slots"] == 5 and rep.window == 2
    assert not novelty.NoveltyReport(0, [5, 5, 3, 2, 5, 5], rs, None, None).truncated
    assert rep.top_containers(3) == []
    raw = np.zeros(1, novelty.REPORT_DTYPE)
    raw[0] = (novelty.EMPTY_HASH - 1, 7, 3, 2, 1, 1, 0, 4, 0)
    assert novelty.records_of(raw) == [rec(novelty.EMPTY_HASH - 1, 2, 1, 3, 1, 0, 4, 7)]


def test_decode_state_of_a_host_built_table():
    cap = 64
    raw = np.zeros(novelty.state_size(cap), np.uint8)
    hdr = raw[:256].view(novelty.HEADER_DTYPE)
    hdr["magic"], hdr["capacity"] = novelty.MAGIC, cap
    slots = raw[256:256 + cap * 64].view(novelty.SLOT_DTYPE)
    slots["hash"], slots["group"] = np.uint64(novelty.EMPTY_HASH), novelty.EMPTY_GROUP
    slots[5] = (A, 2, 1, 4, 3, 30, 0, 0, 0, (0, 0))
    slots[9] = (B, 0, 0, 0, 0, 0, 0, 0, 0, (0, 0))  # claimed, absent
    assert novelty.live_records(raw) == {(2, A): (1, 4, 3, 30)}
    with pytest.raises(ValueError):
        novelty.live_records(raw[:-256])


def _numpy_stream(**kw):
    from krca import synth
    from krca.rca import Comm, Config, shard_graph, shard_range
    from krca.stream import StreamingRCA
    from numpy_shard import NumpyShard
    N, M, W = 200, 4, 10
    m = synth.make_graph(N, avg_degree=4, seed=3)
    x = synth.make_metrics(N, M, W + 8, window=W, seed=4, roots=m.roots, hop_sets=synth.caller_hops(m, m.roots)).numpy()
    cfg = Config(window=W)
    comm = kw.pop("comm", None) or Comm(1, 0)
    lo, hi, n_max = shard_range(N, comm.world, comm.rank)
    rp, col, od = shard_graph(m.row_ptr, m.col, m.outdeg, lo, hi)
    sh = NumpyShard(np.zeros((0, hi - lo, M), np.float32), rp, col, od, N, n_max, comm.world, cfg)
    return StreamingRCA(None, m.row_ptr, m.col, m.outdeg, M, cfg, horizon=30, tol=1e-9, max_iter=60, comm=comm, shard=sh,
                        **kw), x


def test_stream_refuses_novelty_on_several_ranks():
    from krca.rca import Comm
    for arg in (True, dict(capacity=1024), {}):
        with pytest.raises(ValueError, match="world == 1"):
            _numpy_stream(comm=Comm(2, 0), novelty=arg)
    s, _ = _numpy_stream(comm=Comm(2, 0))  # without novelty a second rank is what it was
    assert s.novelty is None


def test_snapshot_keys_unchanged_without_novelty(tmp_path):
    s, x = _numpy_stream()
    s.window(x)
    path = str(tmp_path / "s.npz")
    s.snapshot(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["hist", "meta", "r"]
        meta = json.loads(bytes(z["meta"]).decode())
    assert sorted(meta) == ["H", "M", "N", "cfg", "hi", "last_iters", "lo", "n_max", "rank", "shard", "solved", "t", "tol",
                            "version", "world"]
    other, _ = _numpy_stream()
    other.restore(path)
    assert other.t == s.t and other.novelty is None
