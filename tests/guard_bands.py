"""Guard-band harness: tensors that are views into poisoned, guarded byte buffers, and a way to make painter_amd.ops allocate
every output, side output and scratch buffer from them at its exact size.

    [ guard | payload | guard ]      one flat uint8 buffer per allocation, every byte 0xFF before the kernel runs

0xFF.. is NaN as bf16 and as fp32, -1 as int32 / int64, 255 as uint8.  With a leading dimension the payload is a [rows, ld] matrix and the
tensor handed out is its column slice [:, col_off : col_off + cols]; the columns around the slice ("row gaps") count as guard.  After the
kernels ran, Arena.check() asserts that every guard and row-gap byte is still 0xFF, and Arena.unwritten() counts the elements of a result that
still hold the poison.  A plain module: no conftest, no pytest settings."""
import contextlib
import math
import re

import torch

POISON = 0xFF
GUARD_BYTES = 4 << 20          # each side; more than any overrun a helper of include/painter_hip.h could be short by at the shapes tested
ALIGN = 256                    # bytes: the base of every payload (pa_inst_decode, pa_pano_decode refuse a workspace that is not 256-byte aligned)
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def roundup(n, m):
    return (int(n) + m - 1) // m * m


class GuardViolation(AssertionError):
    pass


class _Alloc:
    def __init__(self, name, buf, guard, payload_bytes, rows, pitch, off, row_bytes, tensor):
        self.name, self.buf, self.guard, self.payload_bytes = name, buf, guard, payload_bytes
        self.rows, self.pitch, self.off, self.row_bytes = rows, pitch, off, row_bytes      # bytes; the tensor owns [off, off + row_bytes) of each row
        self.tensor = tensor

    def bad_bytes(self):
        """bool [len(buf)]: the bytes outside the tensor's own that no longer hold the poison."""
        bad = self.buf != POISON
        pay = bad[self.guard:self.guard + self.payload_bytes]
        if self.payload_bytes:
            pay.view(self.rows, self.pitch)[:, self.off:self.off + self.row_bytes] = False
        return bad


class Arena:
    def __init__(self, device, guard_bytes=GUARD_BYTES):
        assert guard_bytes >= ALIGN and guard_bytes % ALIGN == 0          # (so that the payload starts on the buffer's own alignment)
        self.device = torch.device(device)
        self.guard = guard_bytes
        self.allocs = []

    def owns(self, device):
        return device is not None and torch.device(device).type == self.device.type

    def empty(self, shape, dtype, ld=None, col_off=0, name=None, align=16):
        """A poisoned tensor of `shape`.  ld (elements, 2-D shapes): the tensor is columns [col_off, col_off + shape[1]) of a [shape[0], ld]
        payload.  ld and col_off keep `align` bytes (the C ABI asks for 16 of every base address; a test of a deliberately odd pitch says less)."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        es = torch.empty((), dtype=dtype).element_size()
        if ld is None:
            assert col_off == 0
            n = math.prod(shape) if shape else 1
            rows, pitch, off, row_bytes = (1, n * es, 0, n * es)
        else:
            assert len(shape) == 2 and ld >= col_off + shape[1], (shape, ld, col_off)
            assert ld * es % align == 0 and col_off * es % 16 == 0, "ld = %d, col_off = %d elements of %d bytes break the base alignment" % (ld, col_off, es)
            rows, pitch, off, row_bytes = shape[0], ld * es, col_off * es, shape[1] * es
        payload = rows * pitch
        tail = self.guard + (-payload) % 16                     # (the buffer stays a multiple of 16 bytes; the pad belongs to the guard)
        raw = torch.full((self.guard + payload + tail + ALIGN,), POISON, dtype=torch.uint8, device=self.device)
        skip = -raw.data_ptr() % ALIGN                          # (0 from the device allocator; the host allocator aligns to 64 only)
        buf = raw[skip:skip + self.guard + payload + tail]
        assert (buf.data_ptr() + self.guard) % ALIGN == 0, "the payload of an arena allocation starts on a %d-byte boundary" % ALIGN
        flat = buf[self.guard:self.guard + payload].view(dtype)
        t = flat.view(shape) if ld is None else flat.view(rows, ld)[:, col_off:col_off + shape[1]]
        self.allocs.append(_Alloc(name or "#%d %s %s" % (len(self.allocs), tuple(shape), str(dtype).replace("torch.", "")), buf, self.guard, payload,
                                  rows, pitch, off, row_bytes, t))
        return t

    def place(self, t, ld=None, col_off=0, name=None, align=16):
        """Copy an operand into a (strided) arena view: whatever surrounds it in memory is NaN."""
        v = self.empty(t.shape, t.dtype, ld=ld, col_off=col_off, name=name, align=align)
        v.copy_(t)
        return v

    def check(self):
        """Every guard byte and row-gap byte of every allocation is still 0xFF -- or a GuardViolation that names the allocation and the first
        and last offending byte, as offsets from the start of its payload, and their number."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if not self.allocs:
            return
        counts = torch.stack([a.bad_bytes().sum() for a in self.allocs]).tolist()
        msgs = []
        for a, n in zip(self.allocs, counts):
            if n:
                idx = a.bad_bytes().nonzero().flatten()
                first, last = int(idx[0]) - a.guard, int(idx[-1]) - a.guard
                msgs.append("%s: %d byte(s) written outside the tensor, first at payload offset %d, last at %d (payload %d bytes%s)"
                            % (a.name, n, first, last, a.payload_bytes,
                               "" if a.pitch == a.row_bytes else ", rows of %d bytes at pitch %d from byte %d" % (a.row_bytes, a.pitch, a.off)))
        if msgs:
            raise GuardViolation("guard band violated:\n  " + "\n  ".join(msgs))

    @staticmethod
    def unwritten(t):
        """Number of elements of t that still hold the poison (all bytes 0xFF).  Meaningful where the poison is no legitimate value: NaN for
        the float types; for uint8 / int32 results (255, -1) compare with the unguarded run instead."""
        return int((t.view(_INT_OF_SIZE[t.element_size()]) == (POISON if t.element_size() == 1 else -1)).sum()) if t.numel() else 0


class TorchProxy:
    """Stands in for the name `torch` inside painter_amd.ops: empty / empty_like on the arena's device come from the arena, everything
    else is torch's own."""

    def __init__(self, real, arena):
        self.__dict__["_real"] = real
        self.__dict__["_arena"] = arena

    def __getattr__(self, name):
        return getattr(self._real, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._arena.owns(device):
            return self._real.empty(*size, dtype=dtype, device=device, **kw)
        assert not kw, kw
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        return self._arena.empty(shape, dtype if dtype is not None else self._real.get_default_dtype())

    def empty_like(self, t, dtype=None, device=None, **kw):
        if not self._arena.owns(device if device is not None else t.device):
            return self._real.empty_like(t, dtype=dtype, device=device, **kw)
        fmt = kw.pop("memory_format", torch.preserve_format)               # (the arena's layout is contiguous: torch's own for every tensor met here)
        assert not kw and fmt in (torch.preserve_format, torch.contiguous_format), (kw, fmt)
        return self._arena.empty(t.shape, dtype if dtype is not None else t.dtype)

    # zeros / zeros_like / full: an arena allocation filled afterwards -- the payload holds the value, the guards stay 0xFF
    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._arena.owns(device):
            return self._real.zeros(*size, dtype=dtype, device=device, **kw)
        return self.empty(*size, dtype=dtype, device=device, **kw).zero_()

    def zeros_like(self, t, dtype=None, device=None, **kw):
        if not self._arena.owns(device if device is not None else t.device):
            return self._real.zeros_like(t, dtype=dtype, device=device, **kw)
        return self.empty_like(t, dtype=dtype, device=device, **kw).zero_()

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._arena.owns(device):
            return self._real.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:                                          # torch.full's own rule
            dtype = torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int) else self._real.get_default_dtype()
        return self.empty(size, dtype=dtype, device=device, **kw).fill_(fill_value)


class CountingLib:
    """Stands in for the module-level name `lib` of the module under test: counts the calls per pa_* symbol and forwards everything, so a
    case can prove which C entry points it reached."""

    def __init__(self, real):
        self.__dict__["_real"] = real
        self.__dict__["calls"] = {}

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("pa_") or not callable(f):
            return f

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return f(*a, **k)
        return counted


def abi_symbols(header_text):
    """The pa_* function names declared in the text of include/painter_hip.h.  Comments are dropped first: they quote calls and older
    declarations."""
    src = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S))
    return set(re.findall(r"\b(?:int64_t|int)\s+(pa_\w+)\s*\([^;{}]*\)\s*;", src))


@contextlib.contextmanager
def guarded_ops(monkeypatch, arena, ops=None, exact_workspace=False):
    """For the duration of the block every tensor painter_amd.ops allocates -- outputs, side outputs, scratch -- is an exact-size, poisoned,
    guarded arena tensor: `torch` inside the module is a TorchProxy, and ops.workspace returns exactly the requested bytes (rounded up to
    16, never less than 16).  `ops` may be any module that allocates through its name `torch`; one without a `workspace` attribute
    (painter_engine, seggpt_engine, pair_pipeline) gets none.  exact_workspace: ops.workspace returns the requested bytes without the
    rounding (a helper that returns 8 bytes gets 8).  -> the list of (requested bytes, tensor) of the workspace calls made."""
    if ops is None:
        from painter_amd import ops
    calls = []

    def workspace(nbytes, device, slot=0):
        t = arena.empty((int(nbytes) if exact_workspace else max(roundup(nbytes, 16), 16),), torch.uint8, name="workspace #%d (%d bytes asked, slot %d)" % (len(calls), nbytes, slot))
        calls.append((int(nbytes), t))
        return t

    with monkeypatch.context() as m:
        m.setattr(ops, "torch", TorchProxy(torch, arena))
        if hasattr(ops, "workspace"):
            m.setattr(ops, "workspace", workspace)
        yield calls
