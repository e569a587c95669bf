"""C5 streaming replay (krca/stream.py) against the batch kernels' oracle on the same chain.

* krca_stream_score over any sequence of windows == krca_rolling_score over the whole series so
  far (the C restatement): z_last / score within 1e-5 of it (bit-identical arithmetic), flags
  bit-exact; n_exceed == the exceedances of the last H evaluated steps, i.e. the difference of two
  batch prefix counts, bit-exact.
* warm-started re-ranking: each window's fixed-point ranks and iteration count equal
  oracle.c_ppr_warm started from the oracle's previous ranks; top-k identical.
"""
import numpy as np
import pytest
import torch

import oracle
import timeline_cases as TC
from krca import native, synth
from krca.rca import Config
from krca.stream import StreamingRCA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


def _n_prefix(x, t, W):
    """batch exceedance counts over the evaluated steps of x[:t] (0 while t <= W)."""
    return oracle.c_rolling_score(x[:t], W)["n_exceed"] if t > W else np.zeros(x.shape[1], np.int32)


@pytest.mark.parametrize("H", [10_000, 50])
def test_stream_score_equals_batch_prefix(eng, H):
    P, M, T, W = 1500, 8, 400, 60
    m = synth.make_graph(P, avg_degree=8, seed=3)
    x = synth.make_metrics(P, M, T, window=W, seed=4, roots=m.roots).numpy()
    s = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, Config(window=W), horizon=H)
    xd = torch.from_numpy(x).cuda()
    t = 0
    for d in [1, 7, 45, 1, 3, 60, 2, 100, 1, 180]:
        o = s.push_metrics(xd[t:t + d].contiguous())
        t += d
        ref = oracle.c_rolling_score(x[:t], W)
        assert np.array_equal(o["flags"].cpu().numpy(), ref["flags"]), t
        assert np.allclose(o["z_last"].cpu().numpy(), ref["z_last"], rtol=1e-5, atol=1e-6), t
        assert np.allclose(o["score"].cpu().numpy(), ref["score"], rtol=1e-5, atol=1e-6), t
        want = _n_prefix(x, t, W) - _n_prefix(x, t - H, W) if t - H > W else _n_prefix(x, t, W)
        assert np.array_equal(o["n_exceed"].cpu().numpy(), want), t
    assert t == T


def _stream_rows(eng, x, W, H, thr, wins, episodes):
    """One krca_stream_score (or, episodes: krca_stream_timeline with gap 3, min_count 3) stream over
    x in calls of `wins` steps at threshold thr -> per window a dict of host arrays."""
    T, P, M = x.shape
    t, lib, p = torch, eng.lib, eng.ptr
    new = lambda dt, *shape: t.empty(shape or (P,), dtype=dt, device=eng.device)  # noqa: E731
    state = new(t.uint8, int(lib.krca_stream_state_size(P, M, W, H)))
    ep_state = new(t.uint8, int(lib.krca_stream_episode_state_size(P, M)))
    xd = t.from_numpy(np.array(x)).cuda()
    rows, t0 = [], 0
    for d in wins:
        o = dict(z_last=new(t.float32, P, M), score=new(t.float32), n_exceed=new(t.int32), flags=new(t.uint8))
        four = (p(o["z_last"]), p(o["score"]), p(o["n_exceed"]), p(o["flags"]))
        if episodes:
            o.update(onset=new(t.int32), last=new(t.int32), count=new(t.int32), peak=new(t.float32), lead=new(t.int8),
                     n_metrics=new(t.uint8))
            rc = lib.krca_stream_timeline(p(xd[t0:t0 + d]), P, M, d, t0, W, H, thr, 3, 3, p(state), p(ep_state), *four,
                                          p(o["onset"]), p(o["last"]), p(o["count"]), p(o["peak"]), p(o["lead"]),
                                          p(o["n_metrics"]), eng._stream())
        else:
            rc = lib.krca_stream_score(p(xd[t0:t0 + d]), P, M, d, t0, W, H, thr, p(state), *four, eng._stream())
        native._check(rc, "krca_stream_timeline" if episodes else "krca_stream_score")
        t0 += d
        rows.append({k: v.cpu().numpy() for k, v in o.items()})
    return rows


@pytest.mark.parametrize("H", TC.THR_STREAM_HORIZONS)
@pytest.mark.parametrize("thr", TC.THR_STREAM_THRS)
def test_stream_score_thresholds(eng, thr, H):
    """Thresholds off 3.0 (2.7 is no float32 value) through krca_stream_score, horizons of whole
    exceedance-bit words (32, 64) and a partial one (50): after every window what
    test_stream_score_equals_batch_prefix asserts, with the threshold passed to the C twin."""
    P, M, T, W = TC.THR_SHAPE
    x = TC.threshold_series()
    n_prefix = lambda t: (oracle.c_rolling_score(x[:t], W, thr)["n_exceed"] if t > W  # noqa: E731
                          else np.zeros(P, np.int32))
    t = 0
    for d, o in zip(TC.THR_STREAM_WINDOWS, _stream_rows(eng, x, W, H, thr, TC.THR_STREAM_WINDOWS, False)):
        t += d
        ref = oracle.c_rolling_score(x[:t], W, thr)
        assert np.array_equal(o["flags"], ref["flags"]), t
        assert np.allclose(o["z_last"], ref["z_last"], rtol=1e-5, atol=1e-6), t
        assert np.allclose(o["score"], ref["score"], rtol=1e-5, atol=1e-6), t
        want = n_prefix(t) - n_prefix(t - H) if t - H > W else n_prefix(t)
        assert np.array_equal(o["n_exceed"], want), t
    assert t == T and t - H > W and want.sum() > 0


@pytest.mark.parametrize("H", TC.THR_STREAM_HORIZONS)
@pytest.mark.parametrize("thr", TC.THR_STREAM_THRS)
def test_stream_timeline_thresholds(eng, thr, H):
    """The same through krca_stream_timeline on the series rounded to 1/16 (the NumPy reference is
    exact there): the six episode outputs bit-equal to tests/stream_timeline_ref.py after every window,
    the four scoring outputs bit-equal to a parallel krca_stream_score stream, n_exceed to the twin."""
    import stream_timeline_ref as SR
    P, M, T, W = TC.THR_SHAPE
    x = np.ascontiguousarray(TC.threshold_series(dyadic=True)[:, :TC.THR_STREAM_PODS])
    wins = TC.THR_STREAM_WINDOWS
    ref = TC.threshold_stream_ref(thr, H)
    got = _stream_rows(eng, x, W, H, thr, wins, True)
    sc = _stream_rows(eng, x, W, H, thr, wins, False)
    n_prefix = lambda t: (oracle.c_rolling_score(x[:t], W, thr)["n_exceed"] if t > W  # noqa: E731
                          else np.zeros(x.shape[1], np.int32))
    t = 0
    for i, d in enumerate(wins):
        t += d
        for k in SR.KEYS:
            assert got[i][k].dtype == ref[i][k].dtype and got[i][k].tobytes() == ref[i][k].tobytes(), (k, t)
        for k in ("z_last", "score", "n_exceed", "flags"):
            assert got[i][k].tobytes() == sc[i][k].tobytes(), (k, t)
        want = n_prefix(t) - n_prefix(t - H) if t - H > W else n_prefix(t)
        assert np.array_equal(got[i]["n_exceed"], want), t
    assert (ref[-1]["onset"] >= 0).any()


def test_stream_windows_rerank_warm_started(eng):
    P, M, T, W = 4000, 8, 300, 60
    m = synth.make_graph(P, avg_degree=12, seed=6)
    hops = synth.caller_hops(m, m.roots)
    x = synth.make_metrics(P, M, T, window=W, seed=7, roots=m.roots, hop_sets=hops).numpy()
    cfg = Config(window=W)
    s = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, cfg, tol=1e-9, max_iter=60)
    xd = torch.from_numpy(x).cuda()
    r_ref = None
    t = 0
    for d in [W + 100, 20, 1, 1, 50, 1]:
        out = s.window(xd[t:t + d].contiguous())
        t += d
        score = out["scores"]["score"].cpu().numpy()
        o = oracle.c_ppr_ex(m.row_ptr, m.col, m.outdeg, score, cfg.alpha, 60, 1e-9, cfg.floor(P, M), r_start=r_ref)
        r_ref, it = o["r"], o["it"]
        assert np.array_equal(s.shard.r[:P].cpu().numpy(), r_ref), t
        assert out["iters"] == it, (t, out["iters"], it)
        ridx, _ = oracle.topk_ref(oracle.rca_keys_from(o, score, cfg.floor(P, M), m.row_ptr, m.col), cfg.k)
        assert [int(i) for i in out["top"][0]] == [int(i) for i in ridx], t


def test_stream_snapshot_restore_continues_bit_for_bit(eng, tmp_path):
    """Snapshot after window 2 (rolling state bytes, warm-start ranks, step count), restore into a
    new StreamingRCA (fresh device buffers), continue: scores, ranks, iteration counts and top-k
    identical to the uninterrupted stream."""
    P, M, T, W, H = 3000, 8, 260, 60, 90
    m = synth.make_graph(P, avg_degree=10, seed=12)
    x = synth.make_metrics(P, M, T, window=W, seed=13, roots=m.roots,
                           hop_sets=synth.caller_hops(m, m.roots)).numpy()
    cfg = Config(window=W)
    xd = torch.from_numpy(x).cuda()
    windows = [W + 40, 30, 1, 50, 7, 32]

    def make():
        return StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, cfg, horizon=H, tol=1e-9, max_iter=60)

    def rows(s, start, t):
        out = []
        for d in windows[start:]:
            o = s.window(xd[t:t + d].contiguous())
            t += d
            out.append((o["scores"]["score"].cpu().numpy().copy(), o["scores"]["n_exceed"].cpu().numpy().copy(),
                        s.shard.r[:P].cpu().numpy().copy(), o["iters"], [int(i) for i in o["top"][0]]))
        return out

    ref = rows(make(), 0, 0)
    s = make()
    t = 0
    for d in windows[:2]:
        o = s.window(xd[t:t + d].contiguous())
        t += d
    path = str(tmp_path / "stream_rank0.npz")
    s.snapshot(path)
    del s
    s2 = make()
    s2.restore(path)
    assert s2.t == t
    got = rows(s2, 2, t)
    for i, (a, b) in enumerate(zip(ref[2:], got)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i
        assert np.array_equal(a[2], b[2]), i
        assert a[3] == b[3] and a[4] == b[4], i


def test_stream_window_log_overlap_and_error_path(eng):
    """window(x, text, doc_off) runs the log pass on a side stream beside the re-rank: its 13-bin
    and template histograms equal the log pass run alone (one container above
    krca_template_max_lines() takes the deferred path), its ranks / counts / top-k equal a
    metrics-only stream's; a window whose offsets are refused raises and still completes the
    re-rank, so the next windows stay identical to the metrics-only stream.  The log stream is
    primed first (StreamingRCA.prime), the metrics-only one not."""
    from krca.agents.logs import pack_documents
    P, M, T, W = 2000, 8, 200, 60
    m = synth.make_graph(P, avg_degree=8, seed=31)
    x = synth.make_metrics(P, M, T, window=W, seed=32, roots=m.roots,
                           hop_sets=synth.caller_hops(m, m.roots)).numpy()
    docs = synth.make_log_corpus(P, lines_per_doc=2, seed=33, hazard_rate=0.02)
    docs[5] = "\n".join(["E0101 OOMKilled container worker-7 restarting"] * 5000)
    blob, off = pack_documents(docs)
    native.check_doc_off(off, len(blob))
    text, offd = eng.upload_blob(blob), torch.from_numpy(off).cuda()
    bad = offd.clone()
    bad[1] = bad[2] + 1  # not non-decreasing: refused
    assert int(eng.lib.krca_template_max_lines()) < 5000
    ref = eng.log_scan_device(text, offd)
    ref_t = eng.template_hist_device(ref)
    want = [ref[k].cpu().numpy() for k in ("hist", "doc_line0", "doc_lines", "line_mask", "line_start", "line_end")]
    want_t = [ref_t[k].cpu().numpy() for k in ("n_templates", "tmpl_hash", "tmpl_count")]
    cfg = Config(window=W)
    a = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, cfg, tol=1e-9, max_iter=60)
    a.prime(len(blob), len(docs), lines_per_doc=2)  # changes no stream state: a stays equal to b
    b = StreamingRCA(eng, m.row_ptr, m.col, m.outdeg, M, cfg, tol=1e-9, max_iter=60)
    xd = torch.from_numpy(x).cuda()
    t = 0
    for i, d in enumerate([W + 40, 1, 5, 1, 20]):
        xw = xd[t:t + d].contiguous()
        t += d
        ob = b.window(xw)
        if i == 2:
            with pytest.raises(native.KrcaError):
                a.window(xw, text, bad)
            assert np.array_equal(a.shard.r[:P].cpu().numpy(), b.shard.r[:P].cpu().numpy())
            assert a.last_iters == b.last_iters
            continue
        oa = a.window(xw, text, offd)
        assert np.array_equal(a.shard.r[:P].cpu().numpy(), b.shard.r[:P].cpu().numpy()), i
        assert oa["iters"] == ob["iters"] and [int(v) for v in oa["top"][0]] == [int(v) for v in ob["top"][0]], i
        lg, tm = oa["logs"], oa["logs"]["templates"]
        assert "_pending" not in tm
        for w_, k in zip(want, ("hist", "doc_line0", "doc_lines", "line_mask", "line_start", "line_end")):
            g_ = lg[k].cpu().numpy()
            bad_ = np.nonzero(g_ != w_)[0] if g_.shape == w_.shape else np.arange(1)
            assert len(bad_) == 0, (i, k, g_.shape, w_.shape, bad_[:5].tolist(), g_[bad_[:5]].tolist(),
                                    w_[bad_[:5]].tolist())
        # template slots: container d's histogram is tmpl_*[doc_line0[d] : doc_line0[d] + n_templates[d]]
        # and every slot past it is zero (the histogram kernels write them), so the two
        # streams agree on EVERY slot.  (Round 4 briefly compared only the valid slots: the arrays
        # were allocated uninitialised and the primed stream's tails held the prime text's hashes --
        # calls r4d / r4f / r4g.)
        assert np.array_equal(tm["n_templates"].cpu().numpy(), want_t[0]), i
        valid = np.zeros(len(want_t[1]), bool)
        for a_, n_ in zip(want[1], want_t[0]):
            valid[a_:a_ + n_] = True
        for w_, k in zip(want_t[1:], ("tmpl_hash", "tmpl_count")):
            g_ = tm[k].cpu().numpy()
            assert np.array_equal(g_, w_), (i, k)
            assert not g_[~valid].any(), (i, k)
