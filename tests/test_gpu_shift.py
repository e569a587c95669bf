"""Level-shift score on the device (csrc/shift.hip): every output of krca_shift_score bit for bit against
tests/shift_ref.py (NaN where it is NaN) over the window sizes, shapes and data kinds of DESIGN.md
§3.19; a tensor past 2^31 bytes; refusals; guard bands and poisons; the agents' keys; the recall fixture."""
import numpy as np
import pytest

import agent_cases as A
import shift_ref as S
from guarded import GuardedEngine, run_poisons
from krca import native, rca
from test_shift_cpu import (NS, check_level_shifts_key, check_recall, check_shift_root_causes, mesh_case,
                            recall_case)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (37, 2), (130, 8), (5, 64), (1000, 8)]  # lanes past the last series, a partial wave, M lanes per pod
BASELINES = [2, 3, 4, 31, 32, 33, 64, 65, 120, 128, 129, 255, 256]
RECENTS = [1, 2, 3, 8, 63, 64]
# (data kind, min_scale)
DATA = [("noise", 0.0), ("ties", 0.0), ("ties", 0.5), ("signs", 0.0), ("nonfinite", 0.0)]


@pytest.fixture(scope="module")
def eng():
    return native.NativeEngine()


@pytest.fixture(scope="module")
def geng():
    return GuardedEngine()


def device_outputs(eng, x, B, R, G, min_scale):
    d = eng.shift_score(x, baseline=B, recent=R, guard=G, min_scale=min_scale)
    assert (d["baseline"], d["recent"], d["guard"]) == (B, R, G)
    for k in S.KEYS:
        assert d[k].device.type == "cuda" and np.array_equal(d[k].cpu().numpy().view(np.uint8),
                                                            d[k + "_host"].view(np.uint8))
    return {k: d[k + "_host"] for k in S.KEYS}


def check(eng, x, B, R, G=0, min_scale=0.0):
    ref = S.shift_score(x, B, R, G, min_scale)
    S.same(ref, device_outputs(eng, x, B, R, G, min_scale), (x.shape, B, R, G, min_scale))
    return ref


@pytest.mark.parametrize("B", BASELINES)
def test_window_sizes(eng, B):
    """Each baseline size with R = 1, R = 64 and one more recent size, over every data kind; the shape,
    the guard and the slack before the windows rotate with the case."""
    i = BASELINES.index(B)
    for j, R in enumerate((1, 64, RECENTS[1 + i % 4])):
        G = (0, 5)[(i + j) % 2]
        T = B + G + R + (0, 17)[(i + j // 2) % 2]
        P, M = SHAPES[(i + j) % len(SHAPES)]
        for n, (kind, ms) in enumerate(DATA):
            check(eng, S.data(kind, T, P, M, seed=100 * i + 10 * j + n), B, R, G, ms)


@pytest.mark.parametrize("P,M", SHAPES)
@pytest.mark.parametrize("B,R,G,extra", [(120, 3, 0, 17), (256, 64, 5, 0), (33, 8, 5, 17), (2, 1, 0, 0)])
def test_shapes(eng, P, M, B, R, G, extra):
    for n, (kind, ms) in enumerate(DATA):
        ref = check(eng, S.data(kind, B + G + R + extra, P, M, seed=n), B, R, G, ms)
    assert ref["score"].shape == (P,) and ref["shift"].shape == (P, M)


@pytest.mark.parametrize("R", RECENTS)
@pytest.mark.parametrize("G", [0, 5])
def test_recent_and_guard(eng, R, G):
    x = S.data("noise", 200, 130, 8, seed=R + G)
    ref = check(eng, x, 120, R, G)
    x[:200 - R - G - 120] = np.nan   # rows before the baseline and the guard rows are not read: the window is
    x[200 - R - G:200 - R] = np.nan  # anchored at the end
    S.same(ref, device_outputs(eng, x, 120, R, G, 0.0), "unread rows")


def test_all_metric_widths(eng):
    for M in (1, 2, 4, 8, 16, 32, 64):
        x = S.data("noise", 60, 67, M, seed=M)
        x[-3:, ::3, M - 1] += 40.0  # a shift in the last metric of every third pod: lead = M - 1
        ref = check(eng, x, 48, 3, 2)
        assert (ref["lead"][::3] == M - 1).all()


def test_past_two_gib(eng):
    """A [4200, 16384, 8] tensor (2.2 GB): byte 2^31 falls at row 4096, inside the baseline window (rows
    4072 .. 4191); the rest of it and the recent rows lie past it.  64-bit offsets."""
    torch = eng.torch
    T, P, M, B, R, G = 4200, 16384, 8, 120, 3, 5
    rows = B + G + R
    assert (T - rows) * P * M * 4 < 1 << 31 < (T - R - G - 1) * P * M * 4
    tail = S.data("noise", rows, P, M, seed=9)
    x = torch.empty((T, P, M), dtype=torch.float32, device=eng.device)
    x[T - rows:] = torch.from_numpy(tail).to(eng.device)
    d = eng.shift_score_device(x, B, R, G, 0.0)
    got = {k: d[k].cpu().numpy() for k in S.KEYS}
    assert np.array_equal(x[T - rows:].cpu().numpy().view(np.uint32), tail.view(np.uint32))
    del x
    S.same(S.shift_score(tail, B, R, G, 0.0), got, "past 2^31 bytes")


def test_refusals_leave_the_outputs_untouched(eng):
    torch = eng.torch
    P, M, T = 50, 8, 40
    x = eng._dev(S.data("noise", T, P, M))
    band = torch.full((6, P * M + 128), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    before = band.clone()
    outs = [band[i, 64:64 + P * M] for i in range(6)]

    def call(P=P, M=M, T=T, B=16, R=3, G=0, ms=0.0):
        return eng.lib.krca_shift_score(eng.ptr(x), P, M, T, B, R, G, ms, *(eng.ptr(o) for o in outs), eng._stream())
    assert eng.lib.krca_shift_max_baseline() == S.MAX_BASELINE and eng.lib.krca_shift_max_recent() == S.MAX_RECENT
    for kw in (dict(M=3), dict(M=128), dict(M=0), dict(B=1), dict(B=257), dict(R=0), dict(R=65), dict(G=-1),
               dict(B=30, R=8, G=3), dict(T=18), dict(ms=-1.0), dict(ms=float("inf")), dict(ms=float("nan")),
               dict(P=-1)):
        assert call(**kw) == -22, kw
        assert b"krca_shift_score" in eng.lib.krca_last_error()
        torch.cuda.synchronize()
        assert torch.equal(band, before), kw
    assert call(P=0) == 0  # a no-op
    torch.cuda.synchronize()
    assert torch.equal(band, before)
    assert call() == 0  # the same buffers, valid arguments: exactly the outputs' elements are written
    torch.cuda.synchronize()
    assert torch.equal(band[:, :64], before[:, :64]) and torch.equal(band[:, 64 + P * M:], before[:, 64 + P * M:])
    assert torch.equal(band[4, 64 + P:], before[4, 64 + P:])  # score: P floats
    ref = S.shift_score(x.cpu().numpy(), 16, 3, 0, 0.0)
    got = {k: outs[i].cpu().numpy().view(np.float32).reshape(P, M) for i, k in enumerate(S.KEYS[:4])}
    got["score"] = outs[4][:P].cpu().numpy().view(np.float32)
    got["lead"] = outs[5].cpu().numpy().view(np.int8)[:P]
    S.same(ref, got, "band")
    assert torch.equal(outs[5].view(torch.int8)[P:], before[5, 64:64 + P * M].view(torch.int8)[P:])  # lead: P bytes


@pytest.mark.parametrize("P,M,B,R,G", [(130, 8, 120, 3, 0), (37, 2, 33, 64, 5), (5, 64, 256, 1, 0)])
def test_guard_bands_and_poisons(geng, P, M, B, R, G):
    x = S.data("nonfinite", B + G + R + 17, P, M, seed=3)
    out = run_poisons(geng, lambda e: {k: e.shift_score(x, B, R, G, 0.5)[k + "_host"] for k in S.KEYS})
    S.same(S.shift_score(x, B, R, G, 0.5), out, "poisons")


# ---- agents ----------------------------------------------------------------------------------------------
def test_agents_end_to_end(eng):
    from krca.agents.coordinator import Coordinator
    from krca.agents.metrics import MetricsAgent
    from krca.mock import MeshClient
    m, x = mesh_case()
    names, xd = m.names(), eng._dev(x)
    agent = MetricsAgent(MeshClient(m, xd), engine=eng, level_shift=True)
    res = agent.analyze(NS)
    assert "error" not in res
    ref = check_level_shifts_key(res["level_shifts"], names, x)
    S.same(ref, {k: agent.last_shift[k + "_host"] for k in S.KEYS}, "last_shift")
    plain = A.strip(Coordinator(MeshClient(m, xd), engine=eng).run_analysis("comprehensive", NS))
    res = A.strip(Coordinator(MeshClient(m, xd), engine=eng, level_shifts=True).run_analysis("comprehensive", NS))
    assert "error" not in plain and "error" not in res and "level_shift_root_causes" not in plain
    rows = res.pop("level_shift_root_causes")
    check_level_shifts_key(res["agent_results"]["metrics"].pop("level_shifts"), names, x)
    assert res == plain and len(res["ranked_root_causes"]) > 0
    check_shift_root_causes(rows, names, m, ref, x, engine=eng)
    short = MetricsAgent(MeshClient(m, xd[-100:].contiguous()), engine=eng, level_shift=True).analyze(NS)
    assert "error" not in short and short["level_shifts"] == []


# ---- recall fixture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_recall_fixture(eng, seed):
    m, x = recall_case(seed)
    xd = eng._dev(x)
    got = eng.shift_score(xd, 120, 3, 0)
    S.same(S.shift_score(x, 120, 3, 0), {k: got[k + "_host"] for k in S.KEYS}, "recall mesh")
    z = eng.rolling_score_device(xd, rca.RANKING.window, rca.RANKING.z_threshold)["score"].cpu().numpy()
    check_recall(m, got["score_host"], z, eng)
