"""Caller-owned buffers as a real caller keeps them: every buffer of a call
carved out of ONE allocation, at interior pointers, with guard bands around it
(tests/test_caller_buffers_gpu.py; the self-tests are in
tests/test_caller_buffers_cpu.py and run on the CPU).

Placement.  Every buffer starts at an address that is 16 mod 32, so it is 16-byte
aligned (what ``struct fe`` and the uint4 digest accesses need) and never 32-byte
aligned; the address mod 512 cycles through 16, 48, 112, 240 and 496 from buffer
to buffer, so the buffers of one call also differ in relative alignment.  No
buffer is less than 16-byte aligned.

Bands.  ``band`` bytes in front of and behind every buffer, and everything else
in the arena that is no buffer, hold the 32-bit word 5; a hole (an output that
is not filled beforehand) holds the word 7.  As field elements (5, 5, 5, 5) and
(7, 7, 7, 7) are canonical and nonzero, as indices or counts they are small: a
band value that reaches a computation gives a wrong answer, never a wild address
(the reasoning of the scratch poison word 3, from which both differ).

``verify()`` raises ArenaError when a byte that is no writable buffer and no
hole has changed (a band, or an input passed with ``writable=False``), and when
a hole still holds its fill from start to end.  The band size is a stated
condition, not a measurement: 64 KiB per side is more than any tile the tested
shapes move in one step, and since the arena is contiguous a write that jumps a
band lands in a neighbour's band or data and is still caught while it falls
inside the arena.  Out of reach: a write beyond the arena, and a read past the
end of a buffer whose value reaches no result."""
import numpy as np
import torch

BAND_WORD = 5
HOLE_WORD = 7
RESIDUES = (16, 48, 112, 240, 496)  # address mod 512; each is 16 mod 32


class ArenaError(AssertionError):
    pass


class _Buf:
    __slots__ = ("name", "start", "nbytes", "kind", "may_stay")

    def __init__(self, name, start, nbytes, kind, may_stay=False):
        self.name, self.start, self.nbytes, self.kind, self.may_stay = name, start, nbytes, kind, may_stay

    @property
    def end(self):
        return self.start + self.nbytes


def _words(nbytes, word, device):
    assert nbytes % 4 == 0
    return torch.full((nbytes // 4,), word, dtype=torch.int32, device=device).view(torch.uint8)


class Arena:
    """One ``torch.uint8`` allocation of ``capacity`` bytes on ``device``."""

    def __init__(self, device, band=65536, capacity=32 << 20):
        assert band >= 16 and band % 16 == 0 and capacity % 4 == 0
        self.device, self.band = torch.device(device), band
        self.mem = _words(capacity, BAND_WORD, self.device)
        # what every guarded byte must still hold at verify()
        self.shadow = self.mem.clone()
        self.base = self.mem.data_ptr()
        assert self.base % 16 == 0
        self.bufs = []
        self._cursor = 0

    # ---- placement -------------------------------------------------------------------
    def _place(self, name, nbytes, kind, may_stay=False):
        assert nbytes > 0 and all(b.name != name for b in self.bufs), name
        want = RESIDUES[len(self.bufs) % len(RESIDUES)]
        # the first buffer: one band in front; later ones: the previous buffer's
        # back band and this one's front band
        lo = self._cursor + (self.band if not self.bufs else 2 * self.band)
        start = lo + (want - (self.base + lo)) % 512
        if start + nbytes + self.band > self.mem.numel():
            raise ValueError("arena of %d bytes is full at buffer %r" % (self.mem.numel(), name))
        assert (self.base + start) % 32 == 16
        b = _Buf(name, start, nbytes, kind, may_stay)
        self.bufs.append(b)
        self._cursor = b.end
        return b

    def _view(self, b, like):
        raw = self.mem[b.start:b.end]
        if like == "limbs":
            assert b.nbytes % 16 == 0
            return raw.view(torch.int32).view(-1, 4)
        if like == "words":
            return raw.view(torch.int32)
        assert like == "bytes", like
        return raw

    def put(self, name, array, writable=False):
        """Copy a numpy array in -> a device view of the same bytes: an (n, 4)
        uint32 / int32 limb array comes back as int32 (n, 4), anything else as
        uint8.  writable=False: verify() checks that the call left it alone."""
        a = np.ascontiguousarray(array)
        limbs = a.ndim == 2 and a.shape[1] == 4 and a.dtype.itemsize == 4
        raw = torch.from_numpy(a.reshape(-1).view(np.uint8).copy())
        b = self._place(name, raw.numel(), "rw" if writable else "ro")
        self.mem[b.start:b.end] = raw.to(self.device)
        self.shadow[b.start:b.end] = self.mem[b.start:b.end]
        return self._view(b, "limbs" if limbs else "bytes")

    def hole(self, name, nbytes, like="limbs", may_stay=False):
        """Reserve an output of nbytes (a multiple of 4), filled with the word 7.
        like: "limbs" -> int32 (n, 4), "words" -> int32 (n,), "bytes" -> uint8.
        may_stay: the call may leave it unwritten."""
        b = self._place(name, nbytes, "hole", may_stay)
        self.mem[b.start:b.end] = _words(nbytes, HOLE_WORD, self.device)
        self.shadow[b.start:b.end] = self.mem[b.start:b.end]
        return self._view(b, like)

    def contains(self, address):
        return self.base <= address < self.base + self.mem.numel()

    # ---- the check ---------------------------------------------------------------------
    def _where(self, pos):
        """(buffer name, side, distance from the buffer's edge) of arena byte pos."""
        for b in self.bufs:
            if b.start <= pos < b.end:
                return b.name, "data", pos - b.start
        best = None
        for b in self.bufs:
            for side, dist in (("front", b.start - pos), ("back", pos - b.end + 1)):
                if dist > 0 and (best is None or dist < best[2]):
                    best = (b.name, side, dist)
        return best if best is not None else ("<empty arena>", "back", pos + 1)

    def verify(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        diff = self.mem != self.shadow
        for b in self.bufs:
            if b.kind != "ro":
                diff[b.start:b.end] = False
        if bool(diff.any()):
            pos = int(torch.nonzero(diff)[0, 0])
            name, side, dist = self._where(pos)
            got, was = int(self.mem[pos]), int(self.shadow[pos])
            if side == "data":
                raise ArenaError("read-only buffer %r: data byte %d from its start changed (0x%02x -> "
                                 "0x%02x)" % (name, dist, was, got))
            raise ArenaError("buffer %r: %s band changed %d byte%s from the buffer's edge (0x%02x -> "
                             "0x%02x)" % (name, side, dist, "" if dist == 1 else "s", was, got))
        for b in self.bufs:
            if b.kind == "hole" and not b.may_stay and \
                    torch.equal(self.mem[b.start:b.end], self.shadow[b.start:b.end]):
                raise ArenaError("hole %r: data still holds its fill from start to end (%d bytes "
                                 "never written)" % (b.name, b.nbytes))
