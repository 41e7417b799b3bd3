"""Owned, poisoned surroundings for the memory-contract tests (tests/test_mem_contract_*.py).  A plain helper module.

Every buffer a call sees -- inputs, scale / zero arrays, masks, outputs, workspaces, prepared tables, status words -- is a
view into a uint8 tensor the test owns, with GUARD bytes of `fill` in front of it and GUARD bytes behind it.  A kernel that
reads past what it was given reads `fill`; one that writes past what it owns changes a guard byte, which Arena.check reads
back.  Nothing here can fault: the stray access lands in memory of the same allocation.

The two fills are chosen for what they mean in each type: 0x00 is 0.0 and code 0; 0xFF.. is a NaN in fp32 and bf16 and code
255 / -1 in the packed streams.  A ragged tile masked with a multiply instead of a select keeps 0 * NaN = NaN under the
second and passes under the first; a neighbour summed in through an off-by-one clamp shows under either, differently.
Outputs are pre-filled with `fill` too, so equal output bytes under both fills prove every byte was written: no sentinel
can collide with a legal value."""
import numpy as np
import torch

ALIGN = 256              # what a torch allocation's data_ptr() is a multiple of: the host plans see the same alignment
GUARD = 4096             # a condition, not a measurement: covers one full store row of the widest tile
SLACK = 2 * ALIGN        # room for the alignment pad (< ALIGN) and for off (< ALIGN)
FILLS = (0x00, 0xFF)

# one store row of the widest tile: 320 rows x 4 B of a column-major piece, or 256 lanes x 16 B of a row
assert GUARD % ALIGN == 0 and GUARD >= 4096 and GUARD >= 320 * 4 and GUARD >= 256 * 16


class ArenaError(AssertionError):
    pass


class _Buf:
    __slots__ = ("name", "raw", "start", "nbytes", "kept", "inplace", "zeroed")


class Arena:
    def __init__(self, device, fill):
        assert fill in FILLS, "fill must be 0x00 or 0xFF"
        self.device, self.fill = torch.device(device), fill
        self.bufs = []

    def _carve(self, name, nbytes, off):
        assert 0 <= off < ALIGN
        b = _Buf()
        b.raw = torch.full((GUARD + SLACK + nbytes + GUARD,), self.fill, dtype=torch.uint8, device=self.device)
        b.start = GUARD + (-(b.raw.data_ptr() + GUARD)) % ALIGN + off
        b.name, b.nbytes, b.kept, b.inplace, b.zeroed = name or "buffer %d" % len(self.bufs), nbytes, None, False, False
        assert b.start >= GUARD and b.raw.numel() - b.start - nbytes >= GUARD
        self.bufs.append(b)
        return b

    def place(self, t, off=0, name=None, inplace=False):
        """A view with t's dtype and shape whose bytes are t's, `off` bytes past a 256-byte boundary, inside guards.  An
        input: check() fails if the call changed it, unless inplace (the case writes it, as out=residual)."""
        t = t.contiguous()
        src = t.reshape(-1).view(torch.uint8)
        b = self._carve(name, src.numel(), off)
        assert off % t.element_size() == 0, "off must keep the element type's alignment"
        b.raw[b.start:b.start + b.nbytes].copy_(src)
        b.kept, b.inplace = src.clone(), inplace
        return b.raw[b.start:b.start + b.nbytes].view(t.dtype).view(t.shape)

    def blank(self, shape, dtype=torch.uint8, off=0, name=None, zero=False):
        """An output, workspace, table or status word: the payload holds `fill` too (zero=True: zeros -- a status word,
        whose contract is OR-accumulation into a zeroed flag)."""
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        esz = torch.empty((), dtype=dtype).element_size()
        b = self._carve(name, int(np.prod(shape, dtype=np.int64)) * esz, off)
        assert off % esz == 0, "off must keep the element type's alignment"
        v = b.raw[b.start:b.start + b.nbytes]
        if zero:
            v.zero_()
            b.zeroed = True
        return v.view(dtype).view(shape)

    def status(self, name="status"):
        return self.blank(1, torch.int32, name=name, zero=True)

    def check(self, what="", refused=False):
        """Read every guard back, and every input's payload.  Raises ArenaError naming the buffer and the first bad offset
        (relative to the payload's first byte: negative in the front guard, >= nbytes in the back guard).
        refused=True, after a call the library turned down: no blank buffer's payload may have changed either."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for b in self.bufs:
            if refused and b.kept is None:
                bad = (b.raw[b.start:b.start + b.nbytes] != (0 if b.zeroed else self.fill)).nonzero()
                if bad.numel():
                    raise ArenaError("%s: the refused call wrote %r: %d bytes changed, the first at payload offset %d"
                                     % (what, b.name, bad.numel(), int(bad[0])))
            end = b.start + b.nbytes
            for lo, hi, part in ((0, b.start, "front guard"), (end, b.raw.numel(), "back guard")):
                bad = (b.raw[lo:hi] != self.fill).nonzero()
                if bad.numel():
                    at = lo + int(bad[0])
                    raise ArenaError("%s: %s of %r written: %d bytes changed, the first at payload offset %d (0x%02x, fill 0x%02x)"
                                     % (what, part, b.name, bad.numel(), at - b.start, int(b.raw[at]), self.fill))
            if b.kept is not None and not b.inplace:
                bad = (b.raw[b.start:end] != b.kept).nonzero()
                if bad.numel():
                    raise ArenaError("%s: input %r modified: %d bytes changed, the first at payload offset %d"
                                     % (what, b.name, bad.numel(), int(bad[0])))


def same_bytes(a, b):
    """Two tensors hold the same bytes (NaN patterns count)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))
