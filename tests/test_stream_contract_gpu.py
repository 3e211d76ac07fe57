"""The stream promise of include/mlhip.h ("All work is enqueued on the context's
HIP stream; functions that return host results synchronise that stream") under
the conditions a long-running caller meets and the rest of the suite does not:
a non-blocking side stream instead of the null stream, calls enqueued behind
pending work with inputs that are still being produced, and switches between
streams with work in flight (mlh_set_stream).

Every result is compared bit for bit with the oracle (oracle/, the C oracle,
tests/*_reference.py).  The inputs arrive late (tests/stream_harness.py): until
the stream reaches the copy that delivers them, the buffers hold other
canonical data, so work that runs out of stream order -- a launch or a copy on
stream 0, a missing dependency -- computes a wrong answer, never a fault.  A
run counts only if the stream was still busy when it mattered; each test prints
its arming line."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

import cs_reference as R
import fill_reference as FR
import lookup_reference as LR
import shifted_reference as SR
import stream_harness as H
import system_reference as SY
from multilinear_amd import _lib
from multilinear_amd import batched as MB
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd import fri as MF
from multilinear_amd import multilinear_pcs as MP
from multilinear_amd.transcript import Transcript
from oracle import batched as OB
from oracle import coracle as C
from oracle import field as F
from oracle import fri as OF
from oracle import pcs as OP
from oracle import polynomials as OPL
from oracle import sumcheck as OS
from oracle import transcript as OT

pytestmark = pytest.mark.gpu

M = F.M


@pytest.fixture(scope="module")
def S():
    return H.side_stream()


def _decoy(a):
    """Canonical elements of the same shape from another seed."""
    return D.random_limbs(a.shape[0], int(a[0, 0]) + 1000003)


def _ints(a):
    return D.limbs_to_ints(a)


def _limbs(values):
    return D.ints_to_limbs(values)


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _gen(log_n):
    return F.pow_2_generator(log_n)


def _bitrev(log_n):
    return np.array([int(format(i, "0%db" % log_n)[::-1], 2) for i in range(1 << log_n)])


def _enqueue(S, name, inputs, op):
    """A call that returns without synchronising: ``op(*buffers)`` -> the
    output tensors, consumed by a copy enqueued on the same stream with no
    host wait in between.  inputs: numpy limb arrays (device buffers of
    ``op``, each delivered late).  -> (idle outputs, armed outputs) as numpy."""
    def make():
        return [(D.to_device(a), D.to_device(_decoy(a))) for a in inputs]

    def call(*bufs):
        outs = op(*bufs)
        outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
        keep = [torch.empty_like(o) for o in outs]
        for k, o in zip(keep, outs):
            k.copy_(o, non_blocking=True)
        return lambda: [_np(k) for k in keep]

    return H.run_armed(S, name, make, call, syncs=False)


def _both(results, want):
    """The idle run and the armed run both equal the oracle."""
    want = list(want) if isinstance(want, (list, tuple)) else [want]
    for which, got in zip(("idle", "armed"), results):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), which


def _call(fn, *args):
    ctx = D.context()
    D.check(fn(ctx, *args), ctx)


# ---- A. calls that return without synchronising ------------------------------------

@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [10, 11, 19])  # the small kernel; one pass kernel; three passes
def test_ntt_behind_pending_work(S, log_n, inverse):
    lib, g = D.lib(), _gen(log_n)
    x = D.random_limbs(1 << log_n, 100 + log_n)

    def op(buf):
        out = torch.empty_like(buf)
        _call(lib.mlh_intt if inverse else lib.mlh_ntt, D.ptr(buf), D.ptr(out), log_n, D.fe_bytes(g))
        return out

    _both(_enqueue(S, "%s 2^%d" % ("intt" if inverse else "ntt", log_n), [x], op),
          C.ntt(x, log_n, g, inverse=inverse))


def test_ntt_batch_behind_pending_work(S):
    """mlh_ntt_batch takes a power-of-two batch (log_batch): 4 x 2^11, the
    smallest above one transform."""
    lib, log_n, log_batch = D.lib(), 11, 2
    g = _gen(log_n)
    x = D.random_limbs(1 << (log_n + log_batch), 111)

    def op(buf):
        out = torch.empty_like(buf)
        _call(lib.mlh_ntt_batch, D.ptr(buf), D.ptr(out), log_n, D.fe_bytes(g), log_batch)
        return out

    want = np.concatenate([C.ntt(x[j << log_n:(j + 1) << log_n], log_n, g)
                           for j in range(1 << log_batch)])
    _both(_enqueue(S, "ntt_batch 4 x 2^11", [x], op), want)


def test_ntt_host_on_a_busy_stream(S):
    """Host in, host out: the call synchronises, and there is no device input
    to deliver late -- the stream is busy when it is made."""
    lib, log_n = D.lib(), 11
    g = _gen(log_n)
    x = D.random_limbs(1 << log_n, 112)
    src = x.tobytes()

    def call():
        inb = (ctypes.c_uint8 * len(src)).from_buffer_copy(src)
        outb = (ctypes.c_uint8 * len(src))()
        _call(lib.mlh_ntt_host, inb, outb, log_n, D.fe_bytes(g), 0)
        return lambda: [np.frombuffer(bytes(outb), dtype=np.uint32).reshape(-1, 4)]

    _both(H.run_armed(S, "ntt_host 2^11", lambda: [], call, syncs=True), C.ntt(x, log_n, g))


@pytest.mark.parametrize("brev", [False, True])
def test_reed_solomon_behind_pending_work(S, brev):
    lib, log_n = D.lib(), 11
    g = _gen(log_n + 1)
    x = D.random_limbs(1 << log_n, 113)
    given = np.ascontiguousarray(x[_bitrev(log_n)]) if brev else x

    def op(buf):
        out = D.empty(2 << log_n)
        _call(lib.mlh_reed_solomon_brev if brev else lib.mlh_reed_solomon, D.ptr(buf), log_n,
              D.fe_bytes(g), D.ptr(out))
        return out

    _both(_enqueue(S, "reed_solomon%s 2^11" % ("_brev" if brev else ""), [given], op),
          C.reed_solomon(x, log_n, g))


def test_bit_reverse_behind_pending_work(S):
    lib, log_n = D.lib(), 11
    x = D.random_limbs(1 << log_n, 114)

    def op(buf):
        out = torch.empty_like(buf)
        _call(lib.mlh_bit_reverse_permutation, D.ptr(buf), D.ptr(out), log_n)
        return out

    _both(_enqueue(S, "bit_reverse 2^11", [x], op), np.ascontiguousarray(x[_bitrev(log_n)]))


@pytest.mark.parametrize("op_name", ["add", "mul", "scale", "inv"])
def test_field_ops_behind_pending_work(S, op_name):
    lib, n = D.lib(), 4097  # no multiple of any block
    a, b = D.random_limbs(n, 115), D.random_limbs(n, 116)
    a[7] = 0  # inv(0) = 0
    ai, bi = _ints(a), _ints(b)
    c = 0x0123456789ABCDEF0123456789ABCDEF % M
    want = {"add": lambda: [(u + v) % M for u, v in zip(ai, bi)],
            "mul": lambda: [u * v % M for u, v in zip(ai, bi)],
            "scale": lambda: [u * c % M for u in ai],
            "inv": lambda: [pow(u, M - 2, M) for u in ai]}[op_name]()

    def op(x, y=None):
        out = torch.empty_like(x)
        if op_name == "add":
            _call(lib.mlh_field_add, D.ptr(x), D.ptr(y), D.ptr(out), n)
        elif op_name == "mul":
            _call(lib.mlh_field_mul, D.ptr(x), D.ptr(y), D.ptr(out), n)
        elif op_name == "scale":
            _call(lib.mlh_field_scale, D.ptr(x), D.fe_bytes(c), D.ptr(out), n)
        else:
            _call(lib.mlh_field_inv, D.ptr(x), D.ptr(out), n)
        return out

    _both(_enqueue(S, "field_%s 4097" % op_name, [a, b] if op_name in ("add", "mul") else [a], op),
          _limbs(want))


def test_fri_fold_behind_pending_work(S):
    lib, log_domain, k = D.lib(), 12, 2
    n = 1 << (log_domain - k)
    layer = D.random_limbs(n, 117)
    r = 0x0FEDCBA9876543210FEDCBA987654321 % M
    li = _ints(layer)
    want = OF.fold_layer([(li[i], li[i + n // 2]) for i in range(n // 2)],
                         F.pow_2_generator_powers(log_domain), k, r)

    def op(buf):
        out = D.empty(n // 2)
        _call(lib.mlh_fri_fold, D.ptr(buf), log_domain - k, k, log_domain, D.fe_bytes(r), D.ptr(out))
        return out

    _both(_enqueue(S, "fri_fold (12, 2)", [layer], op), _limbs(want))


def _layers(leaves):
    return torch.empty((2 * leaves - 1, 32), dtype=torch.uint8, device="cuda")


def test_merkle_commit_pairs_root_left_on_the_device(S):
    lib, log_code = D.lib(), 11  # 2^10 pairs
    code = D.random_limbs(1 << log_code, 118)

    def op(buf):
        out = _layers(1 << (log_code - 1))
        _call(lib.mlh_merkle_commit_pairs, D.ptr(buf), log_code, D.ptr(out), None)
        return out

    _both(_enqueue(S, "merkle_commit_pairs 2^10, no root", [code], op),
          C.merkle_commit_pairs(code, log_code))


@pytest.mark.parametrize("which", ["to_coefficient", "to_evaluation"])
def test_mobius_behind_pending_work(S, which):
    lib, log_n = D.lib(), 13
    ev = D.random_limbs(1 << log_n, 119)
    co = C.to_coefficient(ev, log_n)
    given, want = (ev, co) if which == "to_coefficient" else (co, ev)

    def op(buf):  # in place
        _call(getattr(lib, "mlh_mle_" + which), D.ptr(buf), log_n)
        return buf

    _both(_enqueue(S, "mle_%s 2^13" % which, [given], op), want)


def test_eq_table_on_a_busy_stream(S):
    """The points are host memory: nothing to deliver late, the stream is busy."""
    lib, n = D.lib(), 13
    pts = _ints(D.random_limbs(n, 120))

    def call():
        out = D.empty(1 << n)
        _call(lib.mlh_eq_table, CS._elems(pts), n, D.ptr(out))
        keep = torch.empty_like(out)
        keep.copy_(out, non_blocking=True)
        return lambda: [_np(keep)]

    _both(H.run_armed(S, "eq_table 2^13", lambda: [], call, syncs=False), C.eq_table(pts))


def test_trace_columns_behind_pending_work(S):
    lib, L, W = D.lib(), 9, 7
    a = D.random_limbs(W << L, 121)

    def op(buf):
        out = torch.empty_like(buf)
        _call(lib.mlh_trace_columns, D.ptr(buf), L, W, D.ptr(out))
        return out

    _both(_enqueue(S, "trace_columns (9, 7)", [a], op),
          np.ascontiguousarray(a.reshape(1 << L, W, 4).transpose(1, 0, 2)).reshape(-1, 4))


def _fill_w7():
    """A fill program of the size of the deg5_w7 system: 2^5 rows of 7 columns,
    two outputs, one inversion, one random."""
    return CS.FillProgram(CS.compile_fill({5: CS.var(0) * CS.inv(CS.rand(0) - CS.var(1)) + 9,
                                           6: CS.var(2) * CS.var(3) - CS.var(4)}, 7, 1))


def test_trace_fill_behind_pending_work(S):
    lib, L, W = D.lib(), 5, 7
    prog = _fill_w7()
    a = D.random_limbs(W << L, 122)
    rnd = [0x1234567890ABCDEF1234567890ABCDEF % M]

    def op(buf):  # in place
        _call(lib.mlh_trace_fill, prog.h, D.ptr(buf), L, W, CS._elems(rnd))
        return buf

    _both(_enqueue(S, "trace_fill (5, 7)", [a], op), _limbs(FR.fill_matrix(prog.wire, _ints(a), rnd)))


def test_trace_fill_public_behind_pending_work(S):
    import public_reference as PUB
    import test_public_columns_gpu as TPUB

    lib, L, W, Fn = D.lib(), 5, 7, 3
    descs = TPUB._case(L, W, Fn)
    spec = PUB.builder(descs)
    a = D.random_limbs(W << L, 123)
    want = a.reshape(1 << L, W, 4).copy()
    want[:, W - Fn:] = _limbs(PUB.strip(descs, 1 << L)).reshape(1 << L, Fn, 4)

    def op(buf):  # in place
        _call(lib.mlh_trace_fill_public, spec.h, D.ptr(buf), L, W)
        return buf

    _both(_enqueue(S, "trace_fill_public (5, 7, 3)", [a], op), want.reshape(-1, 4))


def test_trace_extend_next_behind_pending_work(S):
    lib, L, W, K = D.lib(), 5, 7, 3
    cols = [6, 4, 2]
    a = D.random_limbs(W << L, 124)
    T = a.reshape(1 << L, W, 4)
    want = np.concatenate([T, np.roll(T, -1, axis=0)[:, cols]], axis=1)

    def op(buf):
        out = D.empty((W + K) << L)
        _call(lib.mlh_trace_extend_next, D.ptr(buf), L, W, (ctypes.c_uint32 * K)(*cols), K, D.ptr(out))
        return out

    _both(_enqueue(S, "trace_extend_next (5, 7, 3)", [a], op),
          np.ascontiguousarray(want).reshape(-1, 4))


def test_sumcheck_fold_behind_pending_work(S):
    lib, L = D.lib(), 10
    m, d = D.random_limbs(1 << L, 125), D.random_limbs(1 << L, 126)
    r = 0x00112233445566778899AABBCCDDEEFF % M
    tab = R.SumcheckTables(_ints(m), 1, 1 << L, _ints(d))
    tab.fold(r)
    half = 1 << (L - 1)

    def op(mb, db):  # in place; the folded halves
        _call(lib.mlh_sumcheck_fold, D.ptr(mb), D.ptr(db), L, D.fe_bytes(r))
        return mb[:half], db[:half]

    _both(_enqueue(S, "sumcheck_fold 2^10", [m, d], op), [_limbs(tab.matrix), _limbs(tab.delta)])


def test_cs_fold_behind_pending_work(S):
    lib, L, W = D.lib(), 10, 3
    m, d = D.random_limbs(W << L, 127), D.random_limbs(1 << L, 128)
    r = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % M
    tab = R.SumcheckTables(_ints(m), W, 1 << L, _ints(d))
    tab.fold(r)
    half = 1 << (L - 1)

    def op(mb, db):
        _call(lib.mlh_cs_fold, W, D.ptr(mb), D.ptr(db), L, D.fe_bytes(r))
        return mb[:half * W], db[:half]

    _both(_enqueue(S, "cs_fold 2^10 x 3", [m, d], op),
          [_limbs(tab.matrix[:half * W]), _limbs(tab.delta)])


def test_ntt_then_intt_back_to_back(S):
    """Two calls with no sync between them, the second reading the first's
    output: the round trip is the input."""
    lib, log_n = D.lib(), 11
    g = _gen(log_n)
    x = D.random_limbs(1 << log_n, 129)

    def op(buf):
        mid, out = torch.empty_like(buf), torch.empty_like(buf)
        _call(lib.mlh_ntt, D.ptr(buf), D.ptr(mid), log_n, D.fe_bytes(g))
        _call(lib.mlh_intt, D.ptr(mid), D.ptr(out), log_n, D.fe_bytes(g))
        return mid, out

    _both(_enqueue(S, "ntt, intt 2^11", [x], op), [C.ntt(x, log_n, g), x])


def test_reed_solomon_then_merkle_back_to_back(S):
    lib, log_n = D.lib(), 11
    g = _gen(log_n + 1)
    x = D.random_limbs(1 << log_n, 130)
    code = C.reed_solomon(x, log_n, g)

    def op(buf):
        mid, out = D.empty(2 << log_n), _layers(1 << log_n)
        _call(lib.mlh_reed_solomon, D.ptr(buf), log_n, D.fe_bytes(g), D.ptr(mid))
        _call(lib.mlh_merkle_commit_pairs, D.ptr(mid), log_n + 1, D.ptr(out), None)
        return mid, out

    _both(_enqueue(S, "reed_solomon, merkle_commit_pairs 2^11", [x], op),
          [code, C.merkle_commit_pairs(code, log_n + 1)])


# ---- B. calls that return host results ----------------------------------------------



def _returns(S, name, inputs, call):
    """A call that returns host results, so it waits for the stream itself:
    ``call(*buffers)`` -> host values.  inputs: numpy limb arrays, each
    delivered late; the stream is still busy right before the call.  ->
    (idle values, armed values)."""
    def make():
        return [(D.to_device(a), D.to_device(_decoy(a))) for a in inputs]

    def wrapped(*bufs):
        res = call(*bufs)
        return lambda: res

    return H.run_armed(S, name, make, wrapped, syncs=True)


def _same(results, want):
    for which, got in zip(("idle", "armed"), results):
        assert got == want, which


def _rand_ints(n, seed):
    return _ints(D.random_limbs(n, seed))


def test_merkle_commit_pairs_with_root(S):
    lib, log_code = D.lib(), 11
    code = D.random_limbs(1 << log_code, 201)
    want = C.merkle_commit_pairs(code, log_code)

    def call(buf):
        out, root = _layers(1 << (log_code - 1)), (ctypes.c_uint8 * 32)()
        _call(lib.mlh_merkle_commit_pairs, D.ptr(buf), log_code, D.ptr(out), root)
        return bytes(root), out.cpu().numpy().tobytes()

    _same(_returns(S, "merkle_commit_pairs 2^10, root", [code], call),
          (want[-1].tobytes(), want.tobytes()))


def test_mle_evaluate_with_late_evaluations(S):
    lib, n = D.lib(), 9
    ev = D.random_limbs(1 << n, 202)
    pts = _rand_ints(n, 203)

    def call(buf):
        out = (ctypes.c_uint8 * 16)()
        _call(lib.mlh_mle_evaluate, D.ptr(buf), n, CS._elems(pts), out)
        return D.fe_from_bytes(out)

    _same(_returns(S, "mle_evaluate 2^9", [ev], call), OPL.mle_evaluate(_ints(ev), pts))


def test_trace_evaluate_with_late_trace(S):
    lib, n, W = D.lib(), 9, 7
    mat = D.random_limbs(W << n, 204)
    pts = _rand_ints(n, 205)

    def call(buf):
        out = (ctypes.c_uint8 * (16 * W))()
        _call(lib.mlh_trace_evaluate, D.ptr(buf), n, W, CS._elems(pts), out)
        return CS._split(out, W)

    _same(_returns(S, "trace_evaluate (2^9, 7)", [mat], call), OS.trace_evaluate(_ints(mat), W, pts))


def test_sumcheck_partial_sums_with_late_tables(S):
    lib, L = D.lib(), 10
    m, d = D.random_limbs(1 << L, 206), D.random_limbs(1 << L, 207)

    def call(mb, db):
        out = (ctypes.c_uint8 * 32)()
        _call(lib.mlh_sumcheck_partial_sums, D.ptr(mb), D.ptr(db), L, out)
        return tuple(CS._split(out, 2))

    _same(_returns(S, "sumcheck_partial_sums 2^10", [m, d], call), C.partial_sums(m, d, L))


def test_trace_column_sum_with_late_trace(S):
    lib, L, W, mask = D.lib(), 9, 7, 0b1000101
    mat = D.random_limbs(W << L, 208)
    mi = _ints(mat)
    want = sum(mi[i * W + j] for i in range(1 << L) for j in range(W) if (mask >> j) & 1) % M

    def call(buf):
        out = (ctypes.c_uint8 * 16)()
        _call(lib.mlh_trace_column_sum, D.ptr(buf), L, W, mask, out)
        return D.fe_from_bytes(out)

    _same(_returns(S, "trace_column_sum (9, 7)", [mat], call), want)


def _cs_model(name):
    import test_cs_sumcheck_gpu as TCS

    return TCS.CASES[name], TCS.model(name)


def test_cs_partial_sums_with_late_tables(S):
    case, mo = _cs_model("quad3")
    lib, sysm, W, L, Dn = D.lib(), mo["sysm"], case.width, case.log_height, case.degree + 1
    prog = CS.Program(case.wire)
    tab = R.SumcheckTables(list(mo["matrix"]), W, 1 << L, list(mo["delta0"]))
    want = [tab.partial_sum(sysm.evaluate_composition, F.from_i64(x)) for x in range(1, Dn + 1)]

    def call(mb, db):
        out = (ctypes.c_uint8 * (16 * Dn))()
        _call(lib.mlh_cs_partial_sums, prog.h, W, D.ptr(mb), D.ptr(db), L,
              CS._elems(sysm.challenges.trace), CS._elems(sysm.constraint_mask), out)
        return CS._split(out, Dn)

    _same(_returns(S, "cs_partial_sums quad3", [_limbs(mo["matrix"]), _limbs(mo["delta0"])], call),
          want)


def _fri_view(p):
    """What a FriProof holds, in the oracle's shapes."""
    return dict(commitments=p.commitments, last_elem=p.last_elem, last_random=p.last_random,
                queries=[[(v, s) for v, s in p.query(q)] for q in range(_lib.NUM_QUERIES)])


def _fri_want(w):
    return dict(commitments=w.commitments, last_elem=w.last_elem, last_random=w.last_random,
                queries=[[(v, [s for s, _ in path]) for v, path in q] for q in w.queries])


@functools.lru_cache(maxsize=None)
def _fri_case(log_n, seed):
    gp = F.pow_2_generator_powers(log_n + 1)
    code = OF.reed_solomon(_rand_ints(1 << log_n, seed), gp[1])
    otr = OT.Transcript()
    otr.absorb(b"stream")
    want = OF.FriProof.prove(code, gp, otr)
    return _limbs(code), _fri_want(want), otr.random()


def _started():
    tr = Transcript()
    tr.absorb(b"stream")
    return tr


def _fri_prove_call(buf):
    tr = _started()
    p = MF.FriProof.prove(buf, tr)
    return _fri_view(p), tr.random()


def test_fri_prove_with_late_code(S):
    code, want, digest = _fri_case(9, 209)
    _same(_returns(S, "fri_prove 2^9", [code], _fri_prove_call), (want, digest))


@pytest.mark.parametrize("n", [13, 3])  # 13: one eq-factored head round
def test_sumcheck_prove_eq_with_late_evaluations(S, n):
    lib = D.lib()
    ev = D.random_limbs(1 << n, 210 + n)
    pts = _rand_ints(n, 211 + n)
    evi = _ints(ev)
    total = OPL.mle_evaluate(evi, pts)
    ot = OS.SumcheckTables.build_tables_for_pcs(pts, evi)
    otr = OT.Transcript()
    otr.absorb(b"stream")
    prev, want_polys, want_rs = total, [], []
    for _ in range(n):
        nz, r2, prev = ot.compute_sumcheck_polynomial(prev, otr)
        want_polys.append(tuple(nz))
        want_rs.append(r2)

    def call(buf):
        tr = _started()
        work = D.empty(1 << (n - 1))
        polys, rs, dl = (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * (16 * n))(), (ctypes.c_uint8 * 16)()
        _call(lib.mlh_sumcheck_prove_eq, D.ptr(buf), D.ptr(work), n, CS._elems(pts),
              D.fe_bytes(total), tr.h, polys, rs, dl)
        flat = CS._split(polys, 2 * n)
        return ([tuple(flat[2 * k:2 * k + 2]) for k in range(n)], CS._split(rs, n), tr.random(),
                _ints(_np(work[:1]))[0], D.fe_from_bytes(dl), _np(buf).tobytes())

    want = (want_polys, want_rs, otr.random(), ot.matrix[0], ot.delta[0], ev.tobytes())
    _same(_returns(S, "sumcheck_prove_eq n = %d" % n, [ev], call), want)


@functools.lru_cache(maxsize=None)
def _pcs_case(n, seed):
    ev = D.random_limbs(1 << n, seed)
    evi = _ints(ev)
    pts = _rand_ints(n, seed + 1)
    out = OPL.mle_evaluate(evi, pts)
    otr = OT.Transcript()
    otr.absorb(b"stream")
    w = OP.PCSProof.prove(pts, out, evi, otr)
    return ev, pts, out, ([tuple(p) for p in w.sumcheck_polynomials], _fri_want(w.fri_proof),
                          otr.random())


def _pcs_call(pts, out):
    def call(buf):
        tr = _started()
        p = MP.PCSProof.prove(pts, out, buf, tr)
        return p.sumcheck_polynomials, _fri_view(p.fri_proof), tr.random()
    return call


class _fused_max:
    """mlh_set_pcs_fused_max for the block, 24 (the default) restored after it."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        ctx = D.context()
        D.check(D.lib().mlh_set_pcs_fused_max(ctx, self.v), ctx)

    def __exit__(self, *exc):
        ctx = D.context()
        D.check(D.lib().mlh_set_pcs_fused_max(ctx, 24), ctx)
        return False


@pytest.mark.parametrize("rounds", ["fused", "cooperative"])
def test_pcs_prove_with_late_evaluations(S, rounds):
    n = 13
    ev, pts, out, want = _pcs_case(n, 220)
    with _fused_max(24 if rounds == "fused" else 0):  # 0: the cooperative round loop
        _same(_returns(S, "pcs_prove n = 13, %s rounds" % rounds, [ev], _pcs_call(pts, out)), want)


def _batched_view(fp):
    return dict(batch=fp.batch_commitment, commitments=fp.commitments, last_elem=fp.last_elem,
                last_random=fp.last_random, queries=bytes(fp._q))


def _batched_want(w):
    import test_gpu_parity as TG

    return dict(batch=w.batch_commitment, commitments=w.commitments, last_elem=w.last_elem,
                last_random=w.last_random, queries=TG._flat_batched_queries(w))


@functools.lru_cache(maxsize=None)
def _batched_fri_case(m, log_n, seed):
    gp = F.pow_2_generator_powers(log_n + 1)
    codes = [OF.reed_solomon(_rand_ints(1 << log_n, seed + j), gp[1]) for j in range(m)]
    otr = OT.Transcript()
    otr.absorb(b"stream")
    w = OB.BatchedFriProof.prove(codes, gp, otr)
    return _limbs([v for c in codes for v in c]), _batched_want(w), otr.random()


def _batched_fri_call(m):
    def call(buf):
        tr = _started()
        p = MB.BatchedFriProof.prove(buf, m, tr)
        return _batched_view(p), tr.random()
    return call


def test_batched_fri_prove_with_late_codes(S):
    m, log_n = 3, 9
    codes, want, digest = _batched_fri_case(m, log_n, 230)
    _same(_returns(S, "batched_fri_prove (3, 2^9)", [codes], _batched_fri_call(m)), (want, digest))


def test_batched_pcs_prove_with_late_evaluations(S):
    m, n = 2, 10
    polys = [_rand_ints(1 << n, 240 + j) for j in range(m)]
    pts = _rand_ints(n, 243)
    outs = [OPL.mle_evaluate(p, pts) for p in polys]
    otr = OT.Transcript()
    otr.absorb(b"stream")
    w = OB.BatchedPCSProof.prove(pts, outs, polys, otr)
    want = ([tuple(x) for x in w.sumcheck_polynomials], _batched_want(w.fri_proof), otr.random())

    def call(buf):
        tr = _started()
        p = MB.BatchedPCSProof.prove(pts, outs, buf, tr)
        return [tuple(x) for x in p.sumcheck_polynomials], _batched_view(p.fri_proof), tr.random()

    _same(_returns(S, "batched_pcs_prove (2, 10)", [_limbs([v for p in polys for v in p])], call), want)


def _cs_prove_case(name):
    """-> (inputs, call, want) of mlh_cs_sumcheck_prove on a case of cs_cases."""
    case, mo = _cs_model(name)
    lib, sysm, W, L, Dn = D.lib(), mo["sysm"], case.width, case.log_height, case.degree + 1
    prog = CS.Program(case.wire)

    def call(mb, db):
        tr = Transcript()
        tr.absorb(case.seed)
        polys, rs = (ctypes.c_uint8 * (16 * Dn * L))(), (ctypes.c_uint8 * (16 * L))()
        _call(lib.mlh_cs_sumcheck_prove, prog.h, W, D.ptr(mb), D.ptr(db), L,
              CS._elems(sysm.challenges.trace), CS._elems(sysm.constraint_mask),
              D.fe_bytes(mo["total"]), tr.h, polys, rs)
        flat = CS._split(polys, Dn * L)
        return ([flat[Dn * k:Dn * k + Dn] for k in range(L)], CS._split(rs, L), tr.random(),
                _ints(_np(mb[:W])), _ints(_np(db[:1]))[0])

    want = (mo["pols"], mo["rs"], mo["digest"], mo["final_row"], mo["final_delta"])
    return [_limbs(mo["matrix"]), _limbs(mo["delta0"])], call, want


@pytest.mark.parametrize("name", ["deg5_w7", "wide32"])
def test_cs_sumcheck_prove_with_late_tables(S, name):
    inputs, call, want = _cs_prove_case(name)
    _same(_returns(S, "cs_sumcheck_prove " + name, inputs, call), want)


def _pcs_views(pcs_list):
    return [dict(_batched_view(p.fri_proof), polys=p.sumcheck_polynomials,
                 indices=p.fri_proof.query_indices) for p in pcs_list]


def _pcs_wants(models):
    return [dict(batch=w["batch_commitment"], commitments=w["commitments"], last_elem=w["last_elem"],
                 last_random=w["last_random"], queries=w["queries"],
                 polys=[tuple(p) for p in w["polys"]], indices=w["indices"]) for w in models]


def _commit_range(m, L, W, col0, ncols):
    h = ctypes.c_void_p()
    _call(D.lib().mlh_trace_commit_range, D.ptr(m), L, W, col0, ncols, ctypes.byref(h))
    return h


@pytest.mark.parametrize("name", ["quad3", "deg5_w7"])
def test_system_prove_with_late_trace(S, name):
    """The commitment is made beforehand from the trace; the matrix the prover
    folds arrives late."""
    mo = SY.model(name)
    lib, L, W = D.lib(), mo["log_height"], mo["width"]
    prog = CS.Program(SY.program_wire(name))
    with torch.cuda.stream(S):
        committed = D.to_device(_limbs(mo["matrix"]))
        h = ctypes.c_void_p()
        _call(lib.mlh_trace_commit, D.ptr(committed), L, W, ctypes.byref(h))
    try:
        def call(work):
            tr = Transcript()
            tr.absorb(mo["seed"])
            p = CS.SystemProof(L, W, mo["degree"])
            _call(lib.mlh_system_prove, prog.h, h, D.ptr(work), D.fe_bytes(mo["total"]), tr.h,
                  ctypes.byref(p.c))
            p._sync()
            return (p.sumcheck_polynomials, p.output, _pcs_views([p.pcs]), tr.random(),
                    _ints(_np(work[:W])))

        want = (mo["pols"], mo["output"], _pcs_wants([mo["pcs"]]), mo["digest"], mo["output"])
        _same(_returns(S, "system_prove " + name, [_limbs(mo["matrix"])], call), want)
    finally:
        lib.mlh_trace_commitment_destroy(h)


def test_system_prove_shifted_with_late_trace(S):
    name = "mixed5"
    mo = SR.model(name)
    wire, shifts = SR.program(name)
    lib, L, W, P = D.lib(), mo["log_height"], mo["width"], mo["pre"]
    prog = CS.Program(wire)
    K = len(shifts)
    with torch.cuda.stream(S):
        committed = D.to_device(_limbs(mo["matrix"]))
        handles = [_commit_range(committed, L, W, 0, P)]
        if P < W:
            handles.append(_commit_range(committed, L, W, P, W - P))
    try:
        def call(work):
            tr = Transcript()
            tr.absorb(mo["seed"])
            p = CS.ShiftedSystemProof(L, W, mo["degree"], P, mo["mask"], shifts)
            _call(lib.mlh_system_prove_shifted, prog.h, handles[0],
                  handles[1] if len(handles) > 1 else None, mo["mask"],
                  (ctypes.c_uint32 * max(K, 1))(*shifts), K, D.ptr(work), D.fe_bytes(mo["total"]),
                  D.fe_bytes(mo["column_sum"]), tr.h, ctypes.byref(p.c))
            p._sync()
            return (p.sumcheck_polynomials, p.output, p.shift_polynomials, p.output2,
                    _pcs_views(p.pcs + p.pcs_shift), tr.random(), _np(work).tobytes())

        want = (mo["pols"], mo["output"], mo["pols2"], mo["output2"],
                _pcs_wants(mo["pcs"] + mo["pcs_shift"]), mo["digest"], _limbs(mo["matrix"]).tobytes())
        _same(_returns(S, "system_prove_shifted mixed5", [_limbs(mo["matrix"])], call), want)
    finally:
        for h in handles:
            lib.mlh_trace_commitment_destroy(h)


def _lookup_case():
    """The smallest height at which the lookup kernels run more than one block
    (the first layout of tests/test_trace_lookup_gpu.py, uniform values)."""
    import test_trace_lookup_gpu as TL

    W, values, T, Cc = TL.LAYOUTS[0]
    L = next(L for L in range(1, 17) if CS.lookup_counts_launch_info(L, len(values))[1] > 1)
    return L, W, values, T, Cc, TL._inputs(L, W, values, T, Cc, "uniform", "stream")


def test_trace_lookup_counts_with_late_trace(S):
    lib = D.lib()
    L, W, values, T, Cc, matrix = _lookup_case()
    out, n_missing, first = LR.lookup_counts(matrix, W, values, T, Cc)

    def call(buf):
        n, f = ctypes.c_uint64(), ctypes.c_uint64()
        _call(lib.mlh_trace_lookup_counts, D.ptr(buf), L, W, sum(1 << c for c in values), T, Cc,
              ctypes.byref(n), ctypes.byref(f))
        return n.value, (None if f.value == 2 ** 64 - 1 else f.value), _np(buf).tobytes()

    _same(_returns(S, "trace_lookup_counts 2^%d x %d" % (L, W), [_limbs(matrix)], call),
          (n_missing, first, _limbs(out).tobytes()))


def test_fri_step_api_back_to_back_on_a_busy_stream(S):
    """init, fold_step_gp for every k and open_queries, each behind a delay of
    its own on the same stream; the code arrives late for init."""
    log_n = 9
    L = log_n + 1
    gp = F.pow_2_generator_powers(L)
    code = OF.reed_solomon(_rand_ints(1 << log_n, 250), gp[1])
    otr = OT.Transcript()
    opd = OF.FriProverData.init(code, otr)
    steps = []
    for k in range(log_n):
        r = otr.next_challenge()
        opd.fold_step(gp, k, r, otr)
        steps.append((r, opd.fold_roots(), otr.random()))
    idx = [0, (1 << log_n) - 1, 137]
    want_q = [opd.open_query_at(i) for i in idx]
    true = D.to_device(_limbs(code))

    def run(ms):
        armed = []
        with torch.cuda.stream(S):
            if ms is None:
                buf = true.clone()
            else:
                buf, ready = H.late_input(S, true, D.to_device(_decoy(_limbs(code))), ms)
                armed.append(ready.query() is False)
            tr = Transcript()
            pd = MF.FriProverData.init(buf, tr)
            for k, (r, roots, digest) in enumerate(steps):
                if ms is not None:
                    armed.append(H.busy(S, ms).query() is False)
                assert tr.next_challenge() == r
                pd.fold_step(k, r, tr, gen_pows=(gp[1], L))
                assert pd.fold_roots() == roots and tr.random() == digest, k
            if ms is not None:
                armed.append(H.busy(S, ms).query() is False)
            got = pd.open_queries(idx, L)
            assert pd.last_element == opd.last_element
            for q, want in zip(got, want_q):
                assert [v for v, _ in q] == [v for v, _ in want]
                assert [s for _, s in q] == [[s for s, _ in path] for _, path in want]
        return armed

    with torch.cuda.stream(S):
        S.synchronize()
    t0 = time.perf_counter()
    run(None)
    idle_ms = (time.perf_counter() - t0) * 1e3
    ms = max(2.0, 4.0 * idle_ms / (len(steps) + 2))  # per call: the sequence has that many
    armed = run(ms)
    if not all(armed):
        ms *= 2.0
        armed = run(ms)
    print("stream fri step api 2^9: idle sequence %.3f ms, delay %.1f ms per call, %s"
          % (idle_ms, ms, "armed" if all(armed) else "not armed"))
    assert all(armed), "not armed: %r" % (armed,)


# ---- C. switching streams ------------------------------------------------------------
#
# mlh_set_stream (include/mlhip.h): work the context enqueued before a switch
# is ordered before work it enqueues after it, without the caller
# synchronising.  D.context() switches to torch's current stream.

@pytest.fixture(scope="module")
def S2():
    return H.side_stream()


def _armed_twice(name, scenario):
    """scenario(ms) -> armed (ms None: on idle streams, which also gives the
    time the delay is sized from).  Repeats once with twice the delay."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scenario(None)
    idle_ms = (time.perf_counter() - t0) * 1e3
    ms = max(2.0, 4.0 * idle_ms)
    armed = scenario(ms)
    if not armed:
        ms *= 2.0
        armed = scenario(ms)
    print("stream %s: idle run %.3f ms, delay %.1f ms, %s"
          % (name, idle_ms, ms, "armed" if armed else "not armed"))
    assert armed, "not armed: %s" % name


def _odd_generator(log_n, e):
    """A generator of order 2^log_n no other test uses: fresh table keys."""
    assert e & 1
    return pow(_gen(log_n), e, M)


def test_switch_with_tables_still_being_built(S, S2):
    """An NTT of a size, plan and generator this process has not used builds
    its tables on stream A behind a delay; the context then switches to B and
    runs the same transform on another vector.  B's transform reads the tables
    A is yet to build."""
    lib, log_n = D.lib(), 12
    x1, x2 = D.random_limbs(1 << log_n, 301), D.random_limbs(1 << log_n, 302)
    exps = iter([40961, 40963, 40965])

    def scenario(ms):
        g = _odd_generator(log_n, next(exps))
        with torch.cuda.stream(S2):
            in2, out2 = D.to_device(x2), D.empty(1 << log_n)
        with D.ntt_plan("4,4,4"):
            with torch.cuda.stream(S):
                true = D.to_device(x1)
                if ms is None:
                    in1, ready = true, None
                else:
                    in1, ready = H.late_input(S, true, D.to_device(_decoy(x1)), ms)
                out1 = D.empty(1 << log_n)
                _call(lib.mlh_ntt, D.ptr(in1), D.ptr(out1), log_n, D.fe_bytes(g))
            with torch.cuda.stream(S2):
                _call(lib.mlh_ntt, D.ptr(in2), D.ptr(out2), log_n, D.fe_bytes(g))
                armed = ready is not None and ready.query() is False
        S2.synchronize()
        S.synchronize()
        assert np.array_equal(_np(out2), C.ntt(x2, log_n, g)), "after the switch"
        assert np.array_equal(_np(out1), C.ntt(x1, log_n, g)), "before the switch"
        return armed

    _armed_twice("switch, unbuilt tables", scenario)


def test_switch_with_a_pool_block_in_flight(S, S2):
    """mlh_trace_fill on A behind a delay, then on B with other randoms: the
    pooled image of A's call must not be overwritten before A's kernel read it."""
    lib, L, W = D.lib(), 5, 7
    prog = _fill_w7()
    a1, a2 = D.random_limbs(W << L, 303), D.random_limbs(W << L, 304)
    r1, r2 = [0x1111111111111111AAAAAAAAAAAAAAAA % M], [0x2222222222222222BBBBBBBBBBBBBBBB % M]
    want1 = _limbs(FR.fill_matrix(prog.wire, _ints(a1), r1))
    want2 = _limbs(FR.fill_matrix(prog.wire, _ints(a2), r2))

    def scenario(ms):
        with torch.cuda.stream(S2):
            m2 = D.to_device(a2)
        with torch.cuda.stream(S):
            true = D.to_device(a1)
            if ms is None:
                m1, ready = true, None
            else:
                m1, ready = H.late_input(S, true, D.to_device(_decoy(a1)), ms)
            _call(lib.mlh_trace_fill, prog.h, D.ptr(m1), L, W, CS._elems(r1))
        with torch.cuda.stream(S2):
            _call(lib.mlh_trace_fill, prog.h, D.ptr(m2), L, W, CS._elems(r2))
            armed = ready is not None and ready.query() is False
        S2.synchronize()
        S.synchronize()
        assert np.array_equal(_np(m1), want1), "before the switch"
        assert np.array_equal(_np(m2), want2), "after the switch"
        return armed

    _armed_twice("switch, pool block in flight", scenario)


def test_switch_then_eviction(S, S2):
    """With a small table cache limit, an NTT waits on A behind a delay while
    transforms of other sizes on B evict its tables."""
    lib = D.lib()
    log_a = 14
    xa = D.random_limbs(1 << log_a, 305)
    xs = {ln: D.random_limbs(1 << ln, 306 + ln) for ln in (12, 16, 20)}
    exps = iter([40967, 40969, 40971])
    limit = 2 << 20
    runs = [(16, _gen(16)), (20, _gen(20))] + [(12, pow(_gen(12), e, M)) for e in range(41, 81, 2)]
    wants = [C.ntt_par(xs[ln], ln, g) for ln, g in runs]

    def scenario(ms):
        ga = _odd_generator(log_a, next(exps))
        ctx = D.context()
        D.check(lib.mlh_set_table_cache_limit(ctx, limit), ctx)
        try:
            with torch.cuda.stream(S2):
                ins = {ln: D.to_device(x) for ln, x in xs.items()}
            with torch.cuda.stream(S):
                true = D.to_device(xa)
                if ms is None:
                    ina, ready = true, None
                else:
                    ina, ready = H.late_input(S, true, D.to_device(_decoy(xa)), ms)
                outa = D.empty(1 << log_a)
                _call(lib.mlh_ntt, D.ptr(ina), D.ptr(outa), log_a, D.fe_bytes(ga))
            with torch.cuda.stream(S2):
                D.context()  # the switch
                # A is still busy at the switch (B's calls may wait: an eviction drains)
                armed = ready is not None and ready.query() is False
                for (ln, g), want in zip(runs, wants):
                    out = D.empty(1 << ln)
                    _call(lib.mlh_ntt, D.ptr(ins[ln]), D.ptr(out), ln, D.fe_bytes(g))
                    assert np.array_equal(_np(out), want), (ln, g)
                assert lib.mlh_table_cache_bytes(D.context()) <= limit  # A's tables, the oldest, went
            S.synchronize()
            assert np.array_equal(_np(outa), C.ntt(xa, log_a, ga)), "the transform enqueued on A"
        finally:
            ctx = D.context()
            D.check(lib.mlh_set_table_cache_limit(ctx, 1 << 30), ctx)
        return armed

    _armed_twice("switch, eviction", scenario)


def test_two_contexts_on_two_streams(S, S2):
    """Two contexts of one device, each on its own stream: NTTs and Merkle
    commits alternate between them with no synchronisation, each stream busy
    from the start.  No prover runs here, so no cooperative kernel shares the
    machine with the other stream's work."""
    lib, log_n, rounds = D.lib(), 11, 3
    g = _gen(log_n)
    xs = [[D.random_limbs(1 << log_n, 310 + 10 * c + i) for i in range(rounds)] for c in range(2)]
    streams = (S, S2)
    ctxs = []
    try:
        for st in streams:
            h = ctypes.c_void_p()
            assert lib.mlh_context_create(0, ctypes.c_void_p(st.cuda_stream), ctypes.byref(h)) == 0
            ctxs.append(h.value)

        def scenario(ms):
            ins, readies, pairs = [], [], []
            for c, st in enumerate(streams):
                with torch.cuda.stream(st):
                    pairs.append([(D.to_device(x), D.to_device(_decoy(x))) for x in xs[c]])
            for c, st in enumerate(streams):
                if ms is None:
                    ins.append([t for t, _ in pairs[c]])
                else:
                    bufs, ready = H.late_inputs(st, pairs[c], ms)
                    ins.append(bufs)
                    readies.append(ready)
            outs = [[], []]
            for i in range(rounds):
                for c, st in enumerate(streams):
                    with torch.cuda.stream(st):
                        ev, tree = D.empty(1 << log_n), _layers(1 << (log_n - 1))
                        D.check(lib.mlh_ntt(ctxs[c], D.ptr(ins[c][i]), D.ptr(ev), log_n, D.fe_bytes(g)),
                                ctxs[c])
                        D.check(lib.mlh_merkle_commit_pairs(ctxs[c], D.ptr(ev), log_n, D.ptr(tree), None),
                                ctxs[c])
                        outs[c].append((ev, tree))
            armed = bool(readies) and all(r.query() is False for r in readies)
            for st in streams:
                st.synchronize()
            for c in range(2):
                for i in range(rounds):
                    ev = C.ntt(xs[c][i], log_n, g)
                    assert np.array_equal(_np(outs[c][i][0]), ev), (c, i)
                    assert np.array_equal(_np(outs[c][i][1]), C.merkle_commit_pairs(ev, log_n)), (c, i)
            return armed

        _armed_twice("two contexts", scenario)
    finally:
        for h in ctxs:
            lib.mlh_context_destroy(h)


def test_set_stream_and_poison_reject_a_null_context():
    lib = D.lib()
    assert lib.mlh_set_stream(None, None) == _lib.MLH_ERR_INVALID
    assert lib.mlh_set_scratch_poison(None, 3) == _lib.MLH_ERR_INVALID
