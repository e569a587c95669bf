"""The guard-band harness (tests/guarded.py) must be able to fail: every negative case here is a
defect the harness exists to report, planted on CPU tensors, and the test asserts it is reported
for the stated reason."""
import numpy as np
import pytest
import torch

import guarded
from guarded import POISONS, Arena, GuardedEngine, run_poisons


@pytest.fixture()
def eng():
    return GuardedEngine(host_only=True)


def test_arena_layout():
    a = Arena("cpu", capacity=1 << 16)
    p1 = a.alloc(1001, 0x5B, "a")
    p2 = a.alloc(7, 0xFF, "b")
    assert p1.start % 256 == 0 and p2.start % 256 == 0
    assert p1.start >= a.margin and p2.start - p1.end >= a.margin
    assert p1.tensor.numel() == 1001 and p2.tensor.numel() == 7
    # the canary resumes at the very next byte after the payload, no rounding up
    assert int(a.buf[p1.end]) == 0xA5 and int(a.buf[p1.end - 1]) == 0x5B and int(a.buf[p1.start - 1]) == 0xA5
    assert int(a.buf[p2.end]) == 0xA5 and int(a.buf[p2.end - 1]) == 0xFF
    a.check()
    p1.tensor.fill_(0)
    p2.tensor.fill_(0xA5)
    a.check()  # anything may be written inside a payload
    with pytest.raises(MemoryError):
        a.alloc(1 << 16, 0)


def test_write_at_payload_end_is_reported():
    a = Arena("cpu", capacity=1 << 16)
    a.alloc(300, 0, "first")
    p = a.alloc(1001, 0, "victim")
    a.buf[p.end] = 0
    with pytest.raises(AssertionError, match=r"0 byte\(s\) past the end of payload #1 'victim'"):
        a.check()


def test_write_before_payload_start_is_reported():
    a = Arena("cpu", capacity=1 << 16)
    p = a.alloc(64, 0, "victim")
    a.alloc(64, 0, "other")
    a.buf[p.start - 1] = 0x5B
    with pytest.raises(AssertionError, match=r"1 byte\(s\) before the start of payload #0 'victim'"):
        a.check()


def test_canary_valued_write_inside_gap_is_invisible_but_any_other_value_is_not():
    a = Arena("cpu", capacity=1 << 16)
    p = a.alloc(16, 0, "x")
    a.buf[p.end + 5] = 0xA5  # the same byte: nothing changed, nothing to report
    a.check()
    a.buf[p.end + 4095] = 0xA4  # the last byte of the margin
    with pytest.raises(AssertionError, match="4095 byte"):
        a.check()


def test_modified_input_is_reported():
    a = Arena("cpu", capacity=1 << 16)
    x = a.put(np.arange(10, dtype=np.int32), "ids")
    a.inputs_unchanged()
    x[3] = 7
    with pytest.raises(AssertionError, match=r"'ids' .* was modified, first at byte 12"):
        a.inputs_unchanged()


def _good_kernel(eng, x):
    """y = 2x through a workspace it fully writes before reading."""
    t = eng.torch
    xd = eng._dev(x)
    ws = eng._workspace("fake", 4 * len(x)).view(t.int32)
    y = t.empty(len(x), dtype=t.int32, device=eng.device)
    ws.copy_(xd)
    y.copy_(ws * 2)
    return {"y": y.numpy().copy()}


def test_correct_kernel_passes(eng):
    x = np.arange(37, dtype=np.int32)
    out = run_poisons(eng, lambda e: _good_kernel(e, x), capacity=1 << 16)
    assert np.array_equal(out["y"], 2 * x)


def test_skipped_output_element_is_caught(eng):
    x = np.arange(37, dtype=np.int32)

    def kernel(e):
        t = e.torch
        y = t.empty(len(x), dtype=t.int32, device=e.device)
        y[:36] = e._dev(x)[:36] * 2  # the last element is never written
        return {"y": y.numpy().copy()}

    with pytest.raises(AssertionError, match=r"output 'y' differs between poison 0x00 and 0xFF: element 36"):
        run_poisons(eng, kernel, capacity=1 << 16)


def test_unwritten_workspace_word_is_caught(eng):
    x = np.arange(1, 38, dtype=np.int32)

    def kernel(e):
        t = e.torch
        ws = e._workspace("fake", 4 * len(x)).view(t.int32)
        ws[1:] = e._dev(x)[1:]  # word 0 keeps what the buffer held
        y = t.empty(1, dtype=t.int64, device=e.device)
        y[0] = ws.to(t.int64).sum()
        return {"sum": y.numpy().copy()}

    # under the 0x00 poison alone the result is right: the defect shows only across poisons
    with eng.guard(0x00, capacity=1 << 16):
        assert int(kernel(eng)["sum"][0]) == int(x[1:].sum())
    with pytest.raises(AssertionError, match="output 'sum' differs"):
        run_poisons(eng, kernel, capacity=1 << 16)


def test_overrunning_kernel_is_caught(eng):
    def kernel(e):
        ws = e._workspace("fake", 100)
        e._arena.buf[e._guard_ws[("fake", 100)].end] = 0  # one byte more than the size function gave
        return {"n": np.array([ws.numel()])}

    with pytest.raises(AssertionError, match=r"0 byte\(s\) past the end of payload #0 'workspace 'fake''"):
        run_poisons(eng, kernel, capacity=1 << 16)


def test_workspace_identity_and_repoison(eng):
    with eng.guard(0x5B, capacity=1 << 16) as arena:
        a = eng._workspace("k", 100)
        assert a.numel() == 100 and bool((a == 0x5B).all())
        assert eng._workspace("k", 100).data_ptr() == a.data_ptr()  # read back after the call
        assert eng._workspace("k", 101).data_ptr() != a.data_ptr()
        assert eng._workspace("j", 100).data_ptr() != a.data_ptr()
        a.zero_()
        eng.repoison()
        assert bool((a == 0x5B).all())
    arena.check()
    # outside a guard the engine is its base class again
    assert eng._arena is None and eng._workspace("k", 10).numel() >= 10


def test_shim_allocations(eng):
    t = eng.torch
    with eng.guard(0xFF, capacity=1 << 16) as arena:
        e = t.empty((3, 5), dtype=t.float32, device=eng.device)
        assert e.shape == (3, 5) and e.dtype == torch.float32 and bool(torch.isnan(e).all())
        i = t.empty(4, dtype=t.int32, device=eng.device)
        assert i.tolist() == [-1] * 4
        z = t.zeros(7, dtype=t.int64, device=eng.device)
        assert z.tolist() == [0] * 7
        like = t.empty_like(z)
        assert like.dtype == torch.int64 and like.tolist() == [-1] * 7
        n = len(arena.payloads)
        host = t.empty(16, dtype=t.uint8)  # no device: a host allocation passes through
        assert len(arena.payloads) == n and host.numel() == 16
        assert t.empty(0, dtype=t.int32, device=eng.device).numel() == 0
        for p in arena.payloads:
            assert p.start % 256 == 0
    arena.check()
    with eng.guard(0x5B, capacity=1 << 16):
        f = t.empty(2, dtype=t.float32, device=eng.device)
        assert 5e16 < float(f[0]) < 7e16  # the log test's poison: large but finite
        assert int(t.empty(1, dtype=t.int32, device=eng.device)[0]) == 0x5B5B5B5B


def test_shim_forwards_the_module(eng):
    t = eng.torch
    assert t.Tensor is torch.Tensor and isinstance(torch.zeros(1), t.Tensor)
    assert t.float32 is torch.float32 and t.int64 is torch.int64 and t.uint8 is torch.uint8
    assert t.cuda is torch.cuda and t.cuda.current_stream is torch.cuda.current_stream
    assert t.where is torch.where and t.from_numpy is torch.from_numpy
    assert guarded.POISONS == POISONS == (0x00, 0xFF, 0x5B)
