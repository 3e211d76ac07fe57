"""GPU: the NTT passes' two address forms.

A pass forms every global address as a wave-uniform base plus a per-lane byte
offset: 32 bits wide (narrow) while the tile and the tables span less than
2^32 bytes, 64 bits (wide) otherwise.  A context created under
MLH_NTT_WIDE_OFFSETS=1 takes the wide kernels at every size.

* narrow = wide = C oracle, bit for bit, at the smallest shape of every kernel
  kind, through forced plans: one table on pass 0 plus the last pass (TW 3 + 2:
  plans 6,6 and 4,9 -- 4,9's last pass loads straight from HBM, radix 2^4 and
  2^5 last passes load through the staged tile), a middle pass (TW 1: 4,4,4 and
  5,4,4), the inverse, Reed-Solomon with plain and bit-reversed input (ZT 1 and
  2), several vectors in one launch (mlh_ntt_batch: the vector strides enter
  the bases), and at 2^23 -- the smallest size at which pass 0 has two tables
  (R W > 2^22) -- the two-table pass 0 (TW 0: plan 9,7,7, since radix 2^7 / 2^8
  first passes with W <= 2^16 take the progression) and the progression pass 0
  (TW 5: the default plan 8,8,7), both against one oracle transform.
* 2^27 and 2^28, default plans: byte offsets with bit 31 set, and the largest
  size whose first and last passes are narrow.  No oracle answers there; the
  Horner kernel (mlh_poly_evaluate), which shares nothing with the passes,
  checks out[k] = x(w^k) -- every output depends on every input, so a wrong
  load anywhere shows -- and out(w^-m) = N x[m] -- a tile stored to the wrong
  place moves that sum.
"""
import ctypes
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import field as F  # noqa: E402

from multilinear_amd import _lib  # noqa: E402
from multilinear_amd import device as D  # noqa: E402

_ctxs = {}


def _c_oracle():
    from oracle import coracle

    coracle.lib()
    return coracle


def _context(wide):
    """A context of this module's own: narrow (the default) or created under
    MLH_NTT_WIDE_OFFSETS=1 (read once, at creation)."""
    import torch

    if wide not in _ctxs:
        old = os.environ.pop("MLH_NTT_WIDE_OFFSETS", None)
        if wide:
            os.environ["MLH_NTT_WIDE_OFFSETS"] = "1"
        try:
            h = ctypes.c_void_p()
            st = torch.cuda.current_stream(0).cuda_stream
            D.check(D.lib().mlh_context_create(0, ctypes.c_void_p(st), ctypes.byref(h)))
        finally:
            os.environ.pop("MLH_NTT_WIDE_OFFSETS", None)
            if old is not None:
                os.environ["MLH_NTT_WIDE_OFFSETS"] = old
        _ctxs[wide] = h.value
    return _ctxs[wide]


def _with_plan(ctx, plan, fn):
    digits = [int(v) for v in plan.split(",")] if plan else []
    arr = (ctypes.c_uint32 * len(digits))(*digits) if digits else None
    D.check(D.lib().mlh_set_ntt_plan(ctx, arr, len(digits)), ctx)
    try:
        return fn()
    finally:
        D.check(D.lib().mlh_set_ntt_plan(ctx, None, 0), ctx)


def _run(wide, plan, entry, x, n_out, *args):
    """entry(ctx, in, ..., out) on this module's narrow or wide context."""
    ctx = _context(wide)
    dx, out = D.to_device(x), D.empty(n_out)
    L = D.lib()

    def call():
        if entry == "ntt":
            D.check(L.mlh_ntt(ctx, D.ptr(dx), D.ptr(out), *args), ctx)
        elif entry == "intt":
            D.check(L.mlh_intt(ctx, D.ptr(dx), D.ptr(out), *args), ctx)
        elif entry == "ntt_batch":
            D.check(L.mlh_ntt_batch(ctx, D.ptr(dx), D.ptr(out), *args), ctx)
        elif entry == "rs":
            D.check(L.mlh_reed_solomon(ctx, D.ptr(dx), args[0], args[1], D.ptr(out)), ctx)
        else:
            D.check(L.mlh_reed_solomon_brev(ctx, D.ptr(dx), args[0], args[1], D.ptr(out)), ctx)

    _with_plan(ctx, plan, call)
    return D.from_device(out)


def _same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: first mismatches at %s of %d" % (what, bad[:8].tolist(), bad.size)


def _both(plan, entry, x, n_out, want, *args):
    narrow = _run(False, plan, entry, x, n_out, *args)
    wide = _run(True, plan, entry, x, n_out, *args)
    _same(narrow, want, "narrow vs oracle (%s %s)" % (entry, plan))
    _same(wide, want, "wide vs oracle (%s %s)" % (entry, plan))
    _same(narrow, wide, "narrow vs wide (%s %s)" % (entry, plan))


@pytest.mark.parametrize("plan", ["6,6", "4,9", "9,4", "4,4,4", "5,4,4"])
def test_small_plans_narrow_wide_oracle(plan):
    """Forward, inverse, RS (plain and bit-reversed input) and four vectors in
    one launch, per plan."""
    C = _c_oracle()
    log_n = sum(int(v) for v in plan.split(","))
    n = 1 << log_n
    g = F.pow_2_generator(log_n)
    gb = D.fe_bytes(g)
    x = D.random_limbs(4 * n, 4100 + log_n)
    fwd = [C.ntt_par(np.ascontiguousarray(x[i * n:(i + 1) * n]), log_n, g) for i in range(4)]
    _both(plan, "ntt", x[:n], n, fwd[0], log_n, gb)
    _both(plan, "intt", x[:n], n, C.ntt_par(np.ascontiguousarray(x[:n]), log_n, g, inverse=True), log_n, gb)
    _both(plan, "ntt_batch", x, 4 * n, np.concatenate(fwd), log_n, gb, 2)
    half = np.ascontiguousarray(x[:n // 2])
    code = C.reed_solomon_par(half, log_n - 1, g)
    _both(plan, "rs", half, n, code, log_n - 1, gb)
    perm = np.array([int(format(i, "0%db" % (log_n - 1))[::-1], 2) for i in range(n // 2)])
    _both(plan, "rs_brev", np.ascontiguousarray(half[perm]), n, code, log_n - 1, gb)


def test_two_table_and_progression_pass0_narrow_wide_oracle():
    """2^23: pass 0 as TA * TB (plan 9,7,7) and as a progression (default
    plan), one oracle transform for both."""
    C = _c_oracle()
    log_n = 23
    n = 1 << log_n
    g = F.pow_2_generator(log_n)
    x = D.random_limbs(n, 4123)
    want = C.ntt_par(x, log_n, g)
    for plan in ("9,7,7", ""):
        _both(plan, "ntt", x, n, want, log_n, D.fe_bytes(g))


def _poly_at(ctx, dev, n, point):
    out = (ctypes.c_uint8 * 16)()
    D.check(D.lib().mlh_poly_evaluate(ctx, D.ptr(dev), n, D.fe_bytes(point), out), ctx)
    return D.fe_from_bytes(out)


def _row(dev, i):
    return D.limbs_to_ints(D.from_device(dev[i:i + 1]))[0]


@pytest.mark.parametrize("log_n", [27, 28])
def test_large_transform_against_horner(log_n):
    import torch

    free = torch.cuda.mem_get_info(0)[0]
    if free < 16 << 30:
        pytest.skip("needs 16 GiB of free device memory (input, output and scratch of 2^28 elements); %d MiB free"
                    % (free >> 20))
    n = 1 << log_n
    ctx = D.context()
    w = F.pow_2_generator(log_n)
    x = D.random_device(n, 4200 + log_n)
    out = D.empty(n)
    D.check(D.lib().mlh_ntt(ctx, D.ptr(x), D.ptr(out), log_n, D.fe_bytes(w)), ctx)
    r = random.Random(4300 + log_n)
    for k in [0, 1, n // 2, n - 1] + [r.randrange(n) for _ in range(4)]:
        got, want = _row(out, k), _poly_at(ctx, x, n, pow(w, k, F.M))
        print("2^%d: out[%d] = %#x, x(w^k) = %#x" % (log_n, k, got, want))
        assert got == want, k
    winv = pow(w, F.M - 2, F.M)
    for m in [0, n - 1] + [r.randrange(n) for _ in range(4)]:
        got, want = _poly_at(ctx, out, n, pow(winv, m, F.M)), n * _row(x, m) % F.M
        print("2^%d: out(w^-%d) = %#x, N x[m] = %#x" % (log_n, m, got, want))
        assert got == want, m
    del x, out
    torch.cuda.empty_cache()
