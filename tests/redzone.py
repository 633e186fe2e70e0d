"""Red zones around the vectors a test hands to the library (a plain helper module, like tests/arbiter.py).

torch's caching allocator carves tensors out of larger segments: a store one element past y[n-1] usually lands in rounding
slack nobody looks at, and a load past the end reads whatever is there.  `guarded` allocates ONE buffer

        [front guard | interior of n elements | back guard]

whose interior starts `align_bytes` past a 256-byte boundary, fills the whole buffer with a finite poison value, copies the
caller's data into the interior (inputs) or leaves the poison there (outputs), and remembers the bytes.  `check()` then asserts

  * every guard byte is unchanged (an out-of-range write within the guard band);
  * a read-only input's interior is bit-identical to what it was (a write through the wrong pointer);
  * no interior element of an output still holds the poison (an element the kernel never wrote).

A read past the end meets the poison (about 1e4 where the data are |x| <~ 6): it wins a top-r rank, dominates a norm, moves a
sum -- and the oracle comparison fails.  The poison is finite and integers stay inside [0, n), so a read never steers a kernel
into a path it was not written for (NaN keys, unbounded brackets, wild indices).

Nothing here makes an access fault: the guards are ordinary memory of the same allocation, larger than any tile or DMA piece of
the library (1 MiB from 2^20 elements on; the largest piece is 6144 elements of the team form).

The same layout on the host (`device="cpu"`): `.a` is the numpy view of the interior, for the spx_host_* entry points.
"""
import numpy as np
import torch

POISON_F64 = 0x40C388A5A5A5A5A5  # ~10001.29
POISON_F32 = 0x461C45A5          # ~10001.41
POISON_U8 = 0x01
POISON_U8_OUT = 0xA5             # an output mask's interior: a value spx_build_mask never writes

_BITS = {torch.float64: torch.int64, torch.float32: torch.int32, torch.int64: torch.int64, torch.uint8: torch.uint8}


def guard_bytes(n):
    """bytes of each guard: 64 KiB below 2^20 elements, 1 MiB from 2^20 on"""
    return (1 << 20) if n >= (1 << 20) else (64 << 10)


def poison_value(dtype, n=None):
    """the poison as a Python number of `dtype` (int64: n // 3, a valid index that is wrong for the layout)"""
    if dtype == torch.float64:
        return float(np.array([POISON_F64], dtype=np.int64).view(np.float64)[0])
    if dtype == torch.float32:
        return float(np.array([POISON_F32], dtype=np.int32).view(np.float32)[0])
    if dtype == torch.uint8:
        return POISON_U8
    if dtype == torch.int64:
        assert n is not None, "int64 poison needs the vector length n (poison = n // 3)"
        return int(n) // 3
    raise TypeError(dtype)


class Guarded:
    """One guarded buffer.  .t = the interior (a tensor view), .a = its numpy view (host buffers only)."""

    def __init__(self, n, dtype, align_bytes, data, role, poison, device, name):
        assert role in ("in", "out", "inout"), role
        self.n, self.dtype, self.role, self.name = int(n), dtype, role, name
        self.es = torch.empty(0, dtype=dtype).element_size()
        assert align_bytes % self.es == 0 and 0 <= align_bytes < 256, (align_bytes, dtype)
        self.guard = guard_bytes(self.n)
        total = self.guard + 512 + self.n * self.es + self.guard  # (room for the 256-byte rounding and align_bytes)
        total += (-total) % 256
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        assert base % self.es == 0
        self.start = self.guard + (-(base + self.guard)) % 256 + align_bytes  # byte offset of interior element 0
        self.end = self.start + self.n * self.es
        assert (base + self.start) % 256 == align_bytes and self.end + self.guard <= total
        whole = self.buf.view(dtype)
        self.poison = poison if poison is not None else poison_value(dtype, self.n)
        whole.fill_(self.poison)
        self.t = whole[self.start // self.es: self.end // self.es]
        if data is not None:
            src = torch.as_tensor(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else data
            assert src.numel() == self.n, (name, src.numel(), self.n)
            self.t.copy_(src.reshape(-1).to(dtype))
        else:
            assert role == "out", "%s: an input needs data" % name
        self.a = self.t.numpy() if self.buf.device.type == "cpu" else None
        self.snap = self.buf.clone()

    def ptr(self):
        return self.t.data_ptr()

    def set_input(self, p, value):
        """interior element p of an input rewritten by the test itself: in the buffer and in the snapshot check() compares with"""
        assert 0 <= p < self.n
        self.t[p] = value
        self.snap.view(self.dtype)[self.start // self.es + p] = value

    def _first_bad(self, lo, hi):
        """first byte in [lo, hi) of the buffer that differs from the snapshot, or None"""
        if hi <= lo:
            return None
        d = torch.nonzero(self.buf[lo:hi] != self.snap[lo:hi])
        return None if d.numel() == 0 else lo + int(d[0, 0])

    def _elem(self, byte):
        return (byte - self.start) // self.es  # negative in front of the interior

    def check(self):
        for lo, hi, where in ((0, self.start, "front guard"), (self.end, self.buf.numel(), "back guard")):
            if not torch.equal(self.buf[lo:hi], self.snap[lo:hi]):
                b = self._first_bad(lo, hi)
                raise AssertionError("%s: %s written at element offset %d (interior 0..%d)" % (
                    self.name, where, self._elem(b), self.n - 1))
        if self.role == "in" and not torch.equal(self.buf[self.start:self.end], self.snap[self.start:self.end]):
            b = self._first_bad(self.start, self.end)
            raise AssertionError("%s: read-only input changed at interior element %d" % (self.name, self._elem(b)))
        if self.role == "out" and self.n:
            bits = self.t.view(_BITS[self.dtype])
            pbits = torch.tensor([self.poison], dtype=self.dtype).view(_BITS[self.dtype]).item()
            hit = torch.nonzero(bits == pbits)
            if hit.numel():
                raise AssertionError("%s: interior element %d still holds the poison (%d unwritten)" % (
                    self.name, int(hit[0, 0]), hit.shape[0]))


def guarded(n, dtype, align_bytes=0, data=None, role="in", poison=None, device="cuda", name="buf"):
    """[front guard | interior of n elements | back guard], interior at `align_bytes` past a 256-byte boundary.
    role "in": a read-only input (data copied in, interior must stay bit-identical); "out": an output (interior poisoned, every
    element must be written); "inout": guards only (y aliasing q, a value the call updates)."""
    if role == "out" and poison is None and dtype == torch.uint8:
        poison = POISON_U8_OUT
    return Guarded(n, dtype, align_bytes, data, role, poison, device, name)


class Zone:
    """The guarded buffers of one call: .add(...) is `guarded`, .check() checks them all."""

    def __init__(self, device="cuda"):
        self.device, self.bufs = device, []

    def add(self, n, dtype, align_bytes=0, data=None, role="in", poison=None, name=None):
        g = guarded(n, dtype, align_bytes, data, role, poison, self.device, name or "buf%d" % len(self.bufs))
        self.bufs.append(g)
        return g

    def check(self):
        for g in self.bufs:
            g.check()


# float64 alignment modes: (align of y, align of the inputs); "D": y aliases q (inputs aligned)
F64_MODES = {"A": (0, 0), "B": (8, 8), "C": (0, 8), "D": (0, 0)}
F32_OFFSETS = (0, 4, 8, 12)
