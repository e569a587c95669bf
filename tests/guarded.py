"""Guard bands and poisoned buffers around the device calls of NativeEngine (tests only).

Two questions the value comparisons of the suite do not ask: does a call depend on what its
workspace and output buffers held before it, and does it write outside the bytes it was given?

``Arena`` is one uint8 tensor filled with a canary byte.  Every buffer of one top-level call is
carved out of it: a payload of exactly the requested size at a 256-byte-aligned offset, at least
``margin`` bytes of canary before it, and canary again from the very next byte after its end (no
rounding).  ``check()`` then proves no byte outside the payloads changed; ``inputs_unchanged()``
that no input payload did.

``GuardedEngine`` is a NativeEngine whose ``self.torch`` is a shim: inside ``with eng.guard(poison)``
every device ``empty`` / ``empty_like`` is a payload filled with the poison byte, every device
``zeros`` a zeroed payload, every ``_workspace`` a payload of exactly the size function's bytes, and
every uploaded input (``_dev``, ``_dev_n``, ``upload_blob``) a recorded payload.  Nothing in
krca/native.py changes.  ``run_poisons`` runs one call under each poison and compares the outputs
bit for bit: a kernel that leaves an output element unwritten, or reads a workspace word it never
wrote, gives different bytes under different poisons.
"""
import contextlib

import numpy as np

POISONS = (0x00, 0xFF, 0x5B)  # zeros | int -1, float NaN | large positive ints, float ~6e16
ALIGN = 256


class Payload:
    __slots__ = ("start", "nbytes", "label", "host", "tensor")

    def __init__(self, start, nbytes, label, tensor, host=None):
        self.start, self.nbytes, self.label, self.tensor, self.host = start, nbytes, label, tensor, host

    @property
    def end(self):
        return self.start + self.nbytes


class Arena:
    """One canary-filled uint8 tensor; payloads are views into it.

    margin = 4096 bytes: four times the 1 KiB a 256-thread workgroup writes with dword stores, so a
    stray workgroup-wide store of one row past either end of a payload still lands in canary."""

    def __init__(self, device, canary=0xA5, margin=4096, capacity=32 << 20, torch=None):
        if torch is None:
            import torch
        self.torch = torch
        self.canary, self.margin, self.capacity = int(canary), int(margin), int(capacity)
        self.buf = torch.full((self.capacity,), self.canary, dtype=torch.uint8, device=device)
        self.is_canary = torch.ones(self.capacity, dtype=torch.bool, device=device)  # False inside a payload
        self.payloads = []
        self.top = 0  # end of the last payload

    def alloc(self, nbytes, poison=None, label=""):
        """A payload of exactly nbytes (uint8 view); filled with the byte `poison` unless None."""
        nbytes = int(nbytes)
        start = -(-(self.top + self.margin) // ALIGN) * ALIGN
        if start + nbytes + self.margin > self.capacity:
            raise MemoryError(f"guard arena of {self.capacity} bytes is full ({label}: {nbytes} more); "
                              f"pass a larger capacity to guard()")
        t = self.buf[start:start + nbytes]
        if nbytes:
            self.is_canary[start:start + nbytes] = False
            if poison is not None:
                t.fill_(int(poison))
        p = Payload(start, nbytes, label, t)
        self.payloads.append(p)
        self.top = start + nbytes
        return p

    def put(self, host_array, label="input"):
        """Carve an input, copy host_array (numpy array or tensor) into it -> tensor of its dtype / shape."""
        torch = self.torch
        src = host_array if isinstance(host_array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(host_array))
        src = src.detach().contiguous()
        nbytes = src.numel() * src.element_size()
        p = self.alloc(nbytes, None, label)
        out = p.tensor.view(src.dtype).view(src.shape) if nbytes else torch.empty(src.shape, dtype=src.dtype,
                                                                                  device=self.buf.device)
        if nbytes:
            out.copy_(src)
            p.host = src.cpu().clone().view(-1).view(torch.uint8)
        return out

    def _describe(self, off):
        """The nearest payload to arena offset `off` and the distance from it."""
        best = None
        for i, p in enumerate(self.payloads):
            if not p.nbytes:
                continue
            d = p.start - off if off < p.start else off - p.end
            if best is None or d < best[0]:
                where = f"{p.start - off} byte(s) before the start" if off < p.start else \
                    f"{off - p.end} byte(s) past the end"
                best = (d, f"{where} of payload #{i} '{p.label}' ([{p.start}, {p.end}), {p.nbytes} bytes)")
        return best[1] if best else "no payload allocated"

    def check(self):
        """Every byte outside the payloads still equals the canary (one masked comparison)."""
        bad = (self.buf != self.canary) & self.is_canary
        if bool(bad.any().item()):
            offs = self.torch.nonzero(bad).view(-1)
            first, n = int(offs[0].item()), int(offs.numel())
            raise AssertionError(f"canary overwritten: {n} byte(s), first at arena offset {first} "
                                 f"(value 0x{int(self.buf[first].item()):02X}), {self._describe(first)}")

    def inputs_unchanged(self):
        """Every put() payload still equals its host copy."""
        for i, p in enumerate(self.payloads):
            if p.host is None:
                continue
            now = p.tensor.cpu()
            if not self.torch.equal(now, p.host):
                off = int(self.torch.nonzero(now != p.host).view(-1)[0].item())
                raise AssertionError(f"input payload #{i} '{p.label}' ({p.nbytes} bytes) was modified, "
                                     f"first at byte {off}")


class _TorchShim:
    """Forwards every attribute to the real torch module; inside a guard, device empty / empty_like
    / zeros become arena payloads.  Host and pinned allocations pass through untouched."""

    def __init__(self, torch, engine):
        object.__setattr__(self, "_torch", torch)
        object.__setattr__(self, "_engine", engine)

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def _on_device(self, device, kw):
        eng = self._engine
        if eng._arena is None or device is None or kw.get("pin_memory"):
            return False
        return self._torch.device(device) == eng.device

    def _carve(self, size, dtype, poison, label):
        torch = self._torch
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        size = tuple(int(s) for s in size)
        dtype = dtype or torch.get_default_dtype()
        n = int(np.prod(size, dtype=np.int64)) if size else 1
        if n == 0:
            return torch.empty(size, dtype=dtype, device=self._engine.device)
        item = torch.empty(0, dtype=dtype).element_size()
        p = self._engine._arena.alloc(n * item, poison, f"{label} {str(dtype).replace('torch.', '')}{list(size)}")
        return p.tensor.view(dtype).view(size)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._on_device(device, kw):
            return self._torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._carve(size, dtype, self._engine._poison, "empty")

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._on_device(device, kw):
            return self._torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._carve(size, dtype, 0, "zeros")

    def empty_like(self, t, **kw):
        device = kw.pop("device", t.device)
        dtype = kw.pop("dtype", t.dtype)
        if not self._on_device(device, kw):
            return self._torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._carve(tuple(t.shape), dtype, self._engine._poison, "empty_like")


def _native_engine():
    from krca import native
    return native.NativeEngine


class GuardedEngine(_native_engine()):
    """NativeEngine whose allocations come from an Arena inside ``with eng.guard(poison)``; outside a
    guard it behaves as its base class.  host_only=True builds it on CPU tensors without the library
    (the harness's own tests): only the allocation paths work then."""

    def __init__(self, device=0, host_only=False):
        import torch
        if host_only:
            self.lib, self.device, self._ws, self._log_cap = None, torch.device("cpu"), {}, 0
        else:
            super().__init__(device)
        self.torch = _TorchShim(torch, self)
        self._arena, self._poison, self._guard_ws = None, 0, {}

    @contextlib.contextmanager
    def guard(self, poison, capacity=32 << 20, canary=0xA5, margin=4096):
        assert self._arena is None, "guard() does not nest"
        arena = Arena(self.device, canary, margin, capacity)
        self._arena, self._poison, self._guard_ws = arena, int(poison), {}
        saved = (self._log_cap, getattr(self, "_edge_cap", None))
        try:
            yield arena
            if self.device.type != "cpu":
                self.torch.cuda.synchronize(self.device)
        finally:
            self._arena, self._guard_ws = None, {}
            self._log_cap = saved[0]  # capacities learnt inside a guard do not leak into the next one
            if saved[1] is None:
                self.__dict__.pop("_edge_cap", None)
            else:
                self._edge_cap = saved[1]

    # -- allocation paths of NativeEngine -----------------------------------------------------
    def _workspace(self, key, nbytes):
        if self._arena is None:
            return super()._workspace(key, nbytes)
        k = (key, int(nbytes))
        p = self._guard_ws.get(k)
        if p is None:
            p = self._arena.alloc(int(nbytes), self._poison, f"workspace '{key}'")
            self._guard_ws[k] = p
        return p.tensor

    def repoison(self):
        """Refill every workspace payload of the current guard with its poison."""
        for p in self._guard_ws.values():
            if p.nbytes:
                p.tensor.fill_(self._poison)

    def _put(self, t, label):
        if self._arena is None or t.numel() == 0:
            return t
        return self._arena.put(t, label)

    def _dev(self, a, dtype=None):
        t = super()._dev(a, dtype)
        if self._arena is not None and isinstance(a, self.torch.Tensor) and a.device == self.device and \
                t.data_ptr() == a.data_ptr():
            return t  # already a device tensor of the caller's (an arena payload or the caller's own buffer)
        return self._put(t, "input")

    def upload_blob(self, blob):
        if self._arena is None or len(blob) == 0:
            return super().upload_blob(blob)
        return self._arena.put(np.frombuffer(bytearray(blob), np.uint8), "input text")


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_diff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    x, y = a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1)
    i = int(np.flatnonzero(x != y)[0])
    e = i // max(a.itemsize, 1)
    return f"element {e}: {a.reshape(-1)[e]!r} vs {b.reshape(-1)[e]!r}"


def run_poisons(eng, call, poisons=POISONS, **guard_kw):
    """call(eng) -> dict name -> host numpy array over the output's logical extent.  Runs it once
    under each poison; asserts (a) the canaries are intact, (b) the inputs are unchanged, (c) every
    output is bit-identical across the poisons.  Returns the first poison's outputs for (d), the
    comparison with the reference."""
    base = None
    for poison in poisons:
        with eng.guard(poison, **guard_kw) as arena:
            out = call(eng)
        assert arena.payloads, "the call allocated nothing through the engine: nothing was guarded"
        arena.check()
        arena.inputs_unchanged()
        if base is None:
            base = out
            continue
        assert out.keys() == base.keys()
        for name in base:
            assert same_bytes(base[name], out[name]), \
                f"output '{name}' differs between poison 0x{poisons[0]:02X} and 0x{poison:02X}: " \
                f"{first_diff(base[name], out[name])}"
    return base
