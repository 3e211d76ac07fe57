"""Phase 2 of the two-phase system proof on the GPU: mlh_trace_fill against the
plain-Python model tests/fill_reference.py and the host interpreter, and
mlh_trace_column_sum, up to the lookup of test_phased_proof_gpu.py proved
through PhasedProver.fill with the column sum computed on the device.  Every
comparison is bit-exact."""
import ctypes
import random

import numpy as np
import pytest
import torch

import fill_reference as FR
import test_phased_proof_gpu as TP
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd.transcript import Transcript

pytestmark = pytest.mark.gpu

M = FR.M
INVALID = _lib.STATUS_CODES["MLH_ERR_INVALID"]

PROGRAMS = {"lookup": FR.LOOKUP, "product": FR.PRODUCT, "wide16": FR.WIDE16}


def _dev(values):
    return D.to_device(D.ints_to_limbs(values))


def _host(t):
    return D.limbs_to_ints(D.from_device(t))


def _random_matrix(h, W, seed):
    r = random.Random(seed)
    return [r.randrange(M) for _ in range(h * W)]


def _heights(prog):
    """The issue's heights around one chunk of the default launch: B and K from
    mlh_trace_fill_launch_info (K follows the height: one row per thread at
    these sizes)."""
    B, K, _ = prog.launch_info(0)
    top = (B * K).bit_length() - 1
    return sorted({min(L, 13) for L in (0, 1, 6, top - 1, top, top + 1)})


CASES = [(name, L, None) for name in sorted(PROGRAMS)
         for L in _heights(CS.FillProgram(PROGRAMS[name]))]
# the same around one chunk of B x K rows with K > 1, which the default rule
# takes only from 2^18 rows on: the launch shape given explicitly
for _name, _B, _K in (("lookup", 256, 8), ("lookup", 128, 16), ("lookup", 64, 2), ("wide16", 128, 4)):
    _top = (_B * _K).bit_length() - 1
    CASES += [(_name, L, (_B, _K)) for L in (_top - 1, _top, _top + 1)]


def test_launch_shapes():
    """The lookup at 2^20 rows: 256 threads, 8 rows per thread (512 chunks); 16
    from 2^21 rows on; a program without INV one row per thread; 66 slots of a
    width-32 program with 16 INVs fit 128 threads."""
    lookup = CS.FillProgram(FR.LOOKUP)
    assert lookup.launch_info(20) == (256, 8, 512)
    assert lookup.launch_info(22)[:2] == (256, 16)
    assert lookup.launch_info(12) == (256, 1, 16)
    assert CS.FillProgram(FR.PRODUCT).launch_info(20)[:2] == (256, 1)
    assert CS.FillProgram(FR.WIDE16).launch_info(20)[:2] == (128, 16)


@pytest.mark.parametrize("name,log_height,shape", CASES)
def test_fill_matches_model_and_host_interpreter(name, log_height, shape):
    w = PROGRAMS[name]
    prog = CS.FillProgram(w)
    W, h = prog.width, 1 << log_height
    B, K, blocks = prog.launch_info(log_height)
    assert blocks == -(-h // (B * K))  # none of these reaches the grid cap
    r = random.Random("%s %d" % (name, log_height))
    rnd = [r.randrange(M) for _ in range(prog.n_randoms)]
    matrix = _random_matrix(h, W, "m %s %d" % (name, log_height))
    for i in range(0, h, 5):  # zero denominators and zero inputs here and there
        matrix[i * W] = rnd[0] if prog.n_randoms else 0
    m = _dev(matrix)
    if shape is None:
        assert CS.Trace(m, W).fill(prog, rnd) is prog
    else:
        _fill_shaped(prog, m, log_height, rnd, *shape)
    got = _host(m)
    assert got == FR.fill_matrix(w, matrix, rnd)
    for j in range(W):  # a column that is no output is untouched
        if not (prog.output_mask >> j) & 1:
            assert got[j::W] == matrix[j::W]
    for i in range(h):
        assert got[i * W:(i + 1) * W] == prog.evaluate(matrix[i * W:(i + 1) * W], rnd), i


def _fill_shaped(prog, m, log_height, randoms, B, K):
    ctx = D.context()
    st = D.lib().mlh_trace_fill_shaped(ctx, prog.h, D.ptr(m), log_height, prog.width,
                                       CS._elems(randoms), B, K)
    assert st == 0, D.lib().mlh_last_error(ctx)


def _owned_rows(B, K, chunk, lane, ks):
    return [chunk * B * K + k * B + lane for k in ks]


@pytest.mark.parametrize("where", ["first", "last", "middle", "every_k", "whole_table"])
def test_zero_denominators_in_a_batch(where):
    """a = gamma (u's denominator) or t = gamma (v's) at chosen positions of a
    lane's K rows: the output is zero exactly there, and the lane's other rows,
    which share its inversion, are right."""
    prog = CS.FillProgram(FR.LOOKUP)
    B, K = 256, 8  # (the default rule's shape at 2^20 rows, here on two chunks)
    h, W = 2 * B * K, 5
    L = h.bit_length() - 1
    gamma = 0x1234567890ABCDEF1234567890ABCDEF % M
    matrix = _random_matrix(h, W, where)
    assert all((gamma - matrix[i * W]) % M and (gamma - matrix[i * W + 1]) % M for i in range(h))
    zu = {"first": _owned_rows(B, K, 0, 3, [0]),
          "last": _owned_rows(B, K, 1, 5, [K - 1]),
          "middle": _owned_rows(B, K, 0, 64, [K // 2]),
          "every_k": _owned_rows(B, K, 1, 7, range(K)),
          "whole_table": list(range(h))}[where]
    zv = {"first": _owned_rows(B, K, 1, B - 1, [0]),
          "last": _owned_rows(B, K, 0, 0, [K - 1]),
          "middle": _owned_rows(B, K, 1, 130, [K // 2, K // 2 + 1]),
          "every_k": _owned_rows(B, K, 0, 200, range(K)),
          "whole_table": []}[where]
    for i in zu:
        matrix[i * W] = gamma
    for i in zv:
        matrix[i * W + 1] = gamma
    m = _dev(matrix)
    _fill_shaped(prog, m, L, [gamma], B, K)
    got = _host(m)
    assert [i for i in range(h) if got[i * W + 3] == 0] == sorted(zu)
    assert [i for i in range(h) if got[i * W + 4] == 0] == sorted(zv)
    assert got == FR.fill_matrix(FR.LOOKUP, matrix, [gamma])


def test_self_reading_output_sees_the_old_value():
    prog = CS.FillProgram(FR.SELF)  # col1 <- col1 * col0 + rand0
    L, W = 9, 2
    h = 1 << L
    matrix = _random_matrix(h, W, "self")
    m = _dev(matrix)
    trace = CS.Trace(m, W)
    trace.fill(prog, [77])
    once = [v if k % 2 == 0 else (v * matrix[k - 1] + 77) % M for k, v in enumerate(matrix)]
    assert _host(m) == once
    trace.fill(prog, [5])  # applied again, to the new values
    twice = [v if k % 2 == 0 else (v * once[k - 1] + 5) % M for k, v in enumerate(once)]
    assert _host(m) == twice


def test_expression_assignments_through_trace_fill():
    """Trace.fill compiles {column: Expr} itself."""
    L, W = 7, 3
    matrix = _random_matrix(1 << L, W, "expr")
    m = _dev(matrix)
    prog = CS.Trace(m, W).fill({2: CS.var(0) * CS.inv(CS.var(1)) + 9}, [])
    assert prog.output_mask == 0b100 and prog.n_inverses == 1
    assert _host(m) == FR.fill_matrix(prog.wire, matrix, [])


def test_block_takes_a_second_chunk():
    """col1 <- 1 / (gamma - col0) at the smallest height where the grid is
    capped below the number of chunks, against mlh_field_sub + mlh_field_inv
    and torch's strided write-back, compared on the device."""
    prog = CS.FillProgram(FR.INV2)

    def chunks(L):
        B, K, _ = prog.launch_info(L)
        return -(-(1 << L) // (B * K))

    log_height = next(L for L in range(33) if prog.launch_info(L)[2] < chunks(L))
    B, K, blocks = prog.launch_info(log_height)
    print("fill 2^%d x 2: %d chunks of %d x %d rows on %d blocks"
          % (log_height, chunks(log_height), B, K, blocks))
    assert log_height <= 22
    h = 1 << log_height
    m = D.random_device(2 * h, seed=22)
    gamma = 0xFEDCBA9876543210FEDCBA9876543210 % M
    mv = m.view(h, 2, 4)
    mv[::4097, 0] = torch.from_numpy(D.ints_to_limbs([gamma]).view(np.int32)).to(m.device)  # zeros
    want = m.clone()
    g = _dev([gamma]).expand(h, 4).contiguous()
    want.view(h, 2, 4)[:, 1] = CS.field_inv(CS.field_sub(g, mv[:, 0].contiguous()))
    CS.Trace(m, 2).fill(prog, [gamma])
    assert torch.equal(m, want)
    assert not m.view(h, 2, 4)[::4097, 1].any()


# ---- mlh_trace_column_sum ---------------------------------------------------------------

@pytest.mark.parametrize("log_height,width,mask",
                         [(0, 1, 1), (1, 3, 0b101), (6, 5, 0b11000), (9, 32, 0xFFFFFFFF),
                          (13, 4, 0b1000), (6, 5, 0)])
def test_column_sum_matches_python(log_height, width, mask):
    h = 1 << log_height
    matrix = _random_matrix(h, width, "sum %d %d" % (log_height, width))
    cols = [j for j in range(width) if (mask >> j) & 1]
    want = sum(matrix[i * width + j] for i in range(h) for j in cols) % M
    m = _dev(matrix)
    assert CS.trace_column_sum(m, width, cols) == want
    if mask == 0:
        assert want == 0
    assert _host(m) == matrix


def _exact_sum(t):
    """Sum of (n, 4) int32 limbs as a field element: exact integer limb sums."""
    limbs = (t.to(torch.int64) & 0xFFFFFFFF).sum(dim=0).tolist()  # each < 2^32 n
    return sum(v << (32 * k) for k, v in enumerate(limbs)) % M


def test_column_sum_threads_take_many_elements():
    """2^18 x 12 = 3 * 2^20 elements: the grid is at its cap and a thread takes
    24 elements, its column advancing by (stride mod 12) = 8 with a carry."""
    L, W = 18, 12
    h = 1 << L
    m = D.random_device(h * W, seed=18)
    one = _exact_sum(CS.trace_columns(m, W, columns=(5, 1)))
    assert CS.trace_column_sum(m, W, [5]) == one
    two = (one + _exact_sum(CS.trace_columns(m, W, columns=(11, 1)))) % M
    assert CS.trace_column_sum(m, W, [11, 5]) == two
    assert CS.trace_column_sum(m, W, range(W)) == _exact_sum(m)


def test_column_sum_argument_errors():
    lib, ctx = D.lib(), D.context()
    m = _dev(list(range(24)))
    out = (ctypes.c_uint8 * 16)()
    f = lib.mlh_trace_column_sum
    assert f(ctx, D.ptr(m), 3, 3, 0b1000, out) == INVALID   # a mask bit at the width
    assert f(ctx, D.ptr(m), 3, 3, 0b1001, out) == INVALID
    assert f(ctx, None, 3, 3, 0b1, out) == INVALID
    assert f(ctx, D.ptr(m), 3, 3, 0b1, None) == INVALID
    assert f(ctx, D.ptr(m), 3, 0, 0, out) == INVALID
    assert f(ctx, D.ptr(m), 33, 3, 1, out) == INVALID
    assert f(ctx, D.ptr(m), 3, 3, 0b111, out) == 0
    assert D.fe_from_bytes(out) == sum(range(24))
    with pytest.raises(ValueError):
        CS.trace_column_sum(m, 3, [3])


# ---- argument errors of mlh_trace_fill ---------------------------------------------------

def test_fill_argument_errors_leave_the_matrix_unchanged():
    lib, ctx = D.lib(), D.context()
    prog = CS.FillProgram(FR.LOOKUP)
    matrix = _random_matrix(8, 5, "args")
    m = _dev(matrix)
    g = D.fe_bytes(3)
    f = lib.mlh_trace_fill
    assert f(ctx, prog.h, None, 3, 5, g) == INVALID            # null matrix
    assert f(ctx, prog.h, D.ptr(m), 3, 4, g) == INVALID        # not the program's width
    assert f(ctx, prog.h, D.ptr(m), 3, 5, None) == INVALID     # n_randoms = 1
    assert f(ctx, None, D.ptr(m), 3, 5, g) == INVALID
    assert f(ctx, prog.h, D.ptr(m), 33, 5, g) == INVALID
    assert f(ctx, prog.h, D.ptr(m), 3, 5, D.fe_bytes(M)) == INVALID  # non-canonical random
    s = lib.mlh_trace_fill_shaped
    wide = CS.FillProgram(FR.WIDE16)  # 66 slots x 256 threads: over the LDS
    assert s(ctx, wide.h, D.ptr(m), 0, 32, CS._elems([1, 2]), 256, 1) == INVALID
    assert s(ctx, prog.h, D.ptr(m), 3, 5, g, 192, 8) == INVALID
    assert s(ctx, prog.h, D.ptr(m), 3, 5, g, 128, 3) == INVALID
    assert _host(m) == matrix
    with pytest.raises(ValueError):
        CS.Trace(m, 5).fill(prog, [])
    # NULL randoms are fine for a program without any
    p0 = CS.FillProgram(FR.PRODUCT)
    m3 = _dev(list(range(1, 25)))
    assert f(ctx, p0.h, D.ptr(m3), 3, 3, None) == 0
    assert _host(m3) == FR.fill_matrix(FR.PRODUCT, list(range(1, 25)), [])


@pytest.mark.parametrize("threads,K", [(128, 16), (256, 4), (64, 1), (256, 1)])
def test_other_launch_shapes_give_the_same_bytes(threads, K):
    prog = CS.FillProgram(FR.LOOKUP)
    L, W = 12, 5
    gamma = 12345
    matrix = _random_matrix(1 << L, W, "shape")
    matrix[7 * W] = gamma
    a, b = _dev(matrix), _dev(matrix)
    CS.Trace(a, W).fill(prog, [gamma])
    ctx = D.context()
    assert D.lib().mlh_trace_fill_shaped(ctx, prog.h, D.ptr(b), L, W, D.fe_bytes(gamma), threads,
                                         K) == 0, D.lib().mlh_last_error(ctx)
    assert torch.equal(a, b)


# ---- the lookup, end to end ---------------------------------------------------------------

COL_A, COL_T, COL_M, COL_U, COL_V = range(5)


def _lookup_prove_filled(bump):
    """TP._lookup_prove with the helper columns filled by prover.fill and the
    column sum computed on the device."""
    h = 1 << TP.LOOKUP_L
    a, t, mult = TP._lookup_inputs(bump)
    matrix = _dev([v for i in range(h) for v in (a[i], t[i], mult[i], 0, 0)])
    cset, layout = TP._lookup_system()
    trace = CS.Trace(matrix, 5)
    tr = Transcript()
    tr.absorb(b"lookup")
    vt = tr.clone()
    prover = CS.System.phased_prover(tr, cset, layout, trace)
    with pytest.raises(ValueError):  # column 2 belongs to commitment 1
        prover.fill({COL_M: CS.var(COL_A) + 1})
    assert _host(matrix)[2::5] == mult
    prover.fill({COL_U: CS.inv(CS.rand(0) - CS.var(COL_A)),
                 COL_V: -CS.var(COL_M) * CS.inv(CS.rand(0) - CS.var(COL_T))})
    proof = prover.prove(tr, 0)
    return proof, vt, cset, layout, prover.column_sum, tr.random()


def test_lookup_through_fill_equals_the_vector_call_construction():
    proof, vt, cset, layout, colsum, digest = _lookup_prove_filled(bump=False)
    assert colsum == 0
    assert proof.verify(vt, cset, layout, 0, 0)
    assert vt.random() == digest
    old, ovt, _, _, old_colsum = TP._lookup_prove(bump=False)
    assert old_colsum == 0
    assert old.verify(ovt, cset, layout, 0, 0)
    assert proof.sumcheck_polynomials == old.sumcheck_polynomials
    assert proof.output == old.output
    assert proof.commitments == old.commitments
    assert digest == ovt.random()


def test_lookup_with_a_wrong_multiplicity_has_a_nonzero_column_sum():
    proof, vt, cset, layout, colsum, digest = _lookup_prove_filled(bump=True)
    _, _, _, _, want = TP._lookup_prove(bump=True)
    assert colsum == want != 0
    entry = vt.random()
    assert not proof.verify(vt, cset, layout, 0, 0)
    assert vt.random() == entry
    assert proof.verify(vt, cset, layout, 0, colsum)
    assert vt.random() == digest
