"""The checker of tests/test_caller_buffers_gpu.py can itself fail (the arena's
self-tests, on the CPU), and the GPU module names every device entry point of
include/mlhip.h: a new one fails here until it is placed in COVERED or, with a
reason of one of four kinds, in NOT_COVERED."""
import os
import re

import numpy as np
import pytest
import torch

import guard_arena as GA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 4096


def _arena():
    """An input, an in-place buffer and an output, as a call has them."""
    a = GA.Arena("cpu", band=BAND, capacity=1 << 20)
    rng = np.random.default_rng(1)
    x = a.put("in", rng.integers(0, 2 ** 32, size=(33, 4), dtype=np.uint64).astype(np.uint32))
    y = a.put("inout", rng.integers(0, 256, size=100, dtype=np.uint64).astype(np.uint8), writable=True)
    z = a.hole("out", 16 * 9)
    return a, x, y, z


def _buf(a, name):
    return next(b for b in a.bufs if b.name == name)


def test_placement_and_views():
    a, x, y, z = _arena()
    assert x.dtype == torch.int32 and tuple(x.shape) == (33, 4)
    assert y.dtype == torch.uint8 and tuple(y.shape) == (100,)
    assert z.dtype == torch.int32 and tuple(z.shape) == (9, 4)
    assert bool((z == GA.HOLE_WORD).all())
    for k in range(7):
        a.hole("h%d" % k, 64, like="bytes")
    prev_end = None
    for k, b in enumerate(a.bufs):
        addr = a.base + b.start
        assert addr % 32 == 16 and addr % 512 == GA.RESIDUES[k % 5]
        assert b.start >= (BAND if prev_end is None else prev_end + 2 * BAND)
        prev_end = b.end
    assert a.mem.numel() - prev_end >= BAND
    assert x.data_ptr() == a.base + _buf(a, "in").start and a.contains(x.data_ptr())
    assert not a.contains(a.base + a.mem.numel())
    # the views are the arena's bytes
    x[0, 0] += 0
    assert bool((a.mem[: _buf(a, "in").start].view(torch.int32) == GA.BAND_WORD).all())


def test_untouched_arena_passes_once_the_hole_is_written():
    a, x, y, z = _arena()
    z.fill_(1)
    y.fill_(9)  # a writable buffer may change
    a.verify()


def _flip(a, pos):
    a.mem[pos] = a.mem[pos] ^ 0x40  # a torch write, as a kernel's store would be


@pytest.mark.parametrize("name", ["in", "inout", "out"])
@pytest.mark.parametrize("where,side,dist", [
    ("just in front", "front", 1),
    ("just behind", "back", 1),
    ("first byte of the front band", "front", BAND),
    ("last byte of the back band", "back", BAND),
])
def test_band_byte_is_reported_with_name_side_and_distance(name, where, side, dist):
    a, x, y, z = _arena()
    z.fill_(1)
    b = _buf(a, name)
    _flip(a, b.start - dist if side == "front" else b.end + dist - 1)
    with pytest.raises(GA.ArenaError) as e:
        a.verify()
    msg = str(e.value)
    assert ("buffer %r" % name) in msg and (side + " band") in msg, msg
    assert ("changed %d byte" % dist) in msg, msg


def test_read_only_input_byte_is_reported():
    a, x, y, z = _arena()
    z.fill_(1)
    _flip(a, _buf(a, "in").start + 37)
    with pytest.raises(GA.ArenaError) as e:
        a.verify()
    msg = str(e.value)
    assert "read-only buffer 'in'" in msg and "data byte 37 " in msg, msg


def test_unwritten_hole_is_reported_unless_it_may_stay():
    a, x, y, z = _arena()
    with pytest.raises(GA.ArenaError) as e:
        a.verify()
    assert "hole 'out'" in str(e.value) and "data still holds its fill" in str(e.value)
    z[8, 3] = 0  # one word written: it no longer holds its fill from start to end
    a.verify()
    b = GA.Arena("cpu", band=BAND, capacity=1 << 18)
    b.hole("path", 32, like="bytes", may_stay=True)
    b.verify()


def test_full_arena_is_an_error_of_its_own():
    a = GA.Arena("cpu", band=BAND, capacity=1 << 16)
    with pytest.raises(ValueError):
        a.hole("big", 1 << 16, like="bytes")


# ---- the coverage condition -------------------------------------------------------------

def _device_entries():
    """Every exported function of include/mlhip.h with a parameter named dev_*
    or a ``void* dev``."""
    with open(os.path.join(ROOT, "include", "mlhip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set()
    for m in re.finditer(r"\b(mlh_\w+)\s*\(([^;{}()]*)\)\s*;", src):
        if re.search(r"\bdev_\w+|\bvoid\s*\*\s*dev\b", m.group(2)):
            names.add(m.group(1))
    return names


NOT_COVERED_KINDS = [
    r"mlh_sharded_\w+|mlh_comm_preflight",  # multi-GPU entries that need a transport
    r"mlh_bench_\w+",
    r"mlh_malloc|mlh_free|mlh_memcpy_\w+",
    r"mlh_\w+_launch_info",
]


def test_every_device_entry_point_is_covered_or_excused():
    import test_caller_buffers_gpu as TCB

    entries = _device_entries()
    assert len(entries) > 80 and "mlh_ntt" in entries and "mlh_free" in entries
    covered, excused = set(TCB.COVERED), set(TCB.NOT_COVERED)
    assert not covered & excused
    assert entries - (covered | excused) == set(), "device entry points in neither set"
    assert (covered | excused) - entries == set(), "names that are no device entry point"
    for name, reason in TCB.NOT_COVERED.items():
        assert reason and any(re.fullmatch(k, name) for k in NOT_COVERED_KINDS), name
