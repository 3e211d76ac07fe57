"""Buffers the caller owns: every device entry point of the single-GPU C ABI
again, bit-exact against its oracle or model, with every device buffer of the
call carved out of ONE allocation at an interior pointer (tests/guard_arena.py).

The rest of the suite hands the library buffers that torch allocated one by
one: 512-byte aligned, each in its own rounded-up block, with allocator slack
behind it.  A kernel that writes a tile past the end of an output, lets a value
from beyond the end of an input reach a result, or assumes more than the
16-byte alignment that include/mlhip.h promises to need, passes there.  Here
every buffer starts at an address that is 16 mod 32 (never 32-byte aligned),
the buffers of one call differ in their alignment mod 512, 64 KiB of the word
5 stand in front of and behind each, outputs are pre-filled with the word 7,
and after the call and a mlh_synchronize

  * the outputs equal the oracle (oracle/, the C oracle, tests/*_reference.py),
  * no band byte and no byte of a read-only input has changed,
  * no output still holds its fill from start to end.

A band value that reaches a computation is a canonical, nonzero element or a
small index: a wrong answer, never a wild address.  No pointer is less than
16-byte aligned and nothing here aims at a fault.

Two ways to run a family.  Calls with device outputs are made on the raw C ABI
with inputs from ``put`` and outputs from ``hole``.  Calls whose only device
buffers are inputs (the provers, the in-place trace operations) run the
existing oracle comparison of their own module, with ``D.to_device`` placing
what it uploads in the arena for the duration.  A recorder in front of the
library notes every entry point that was called with a pointer into a live
arena; the last test compares that set with COVERED."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import cs_reference as R
import fill_reference as FR
import guard_arena as GA
import lookup_reference as LR
import public_reference as PUB
import test_cs_sumcheck_gpu as TCS
import test_gpu_parity as TG
import test_phased_proof_gpu as TP
import test_public_columns_gpu as TPUB
import test_shifted_proof_gpu as TSH
import test_stream_contract_gpu as TSC
import test_system_proof_gpu as TSY
import test_trace_check_gpu as TCHK
import test_trace_fill_gpu as TF
import test_trace_lookup_gpu as TL
import test_trace_lookup_tuple_gpu as TLT
import test_trace_scan_gpu as TSCAN
import test_trace_sort_gpu as TSORT
from multilinear_amd import _lib
from multilinear_amd import batched as MB
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from multilinear_amd import fri as MF
from multilinear_amd.transcript import Transcript
from oracle import coracle as C
from oracle import field as F
from oracle import fri as OF
from oracle import merkle as OM
from oracle import polynomials as OPL
from oracle import sumcheck as OS
from oracle import transcript as OT
from tests import dist_cpu_ops as DC
from tests import dist_spec as DS

pytestmark = pytest.mark.gpu

M = F.M

COVERED = {
    "mlh_pow_2_generator_powers",
    "mlh_field_add", "mlh_field_sub", "mlh_field_mul", "mlh_field_neg", "mlh_field_scale",
    "mlh_field_inv",
    "mlh_ntt", "mlh_intt", "mlh_ntt_batch", "mlh_bit_reverse_permutation",
    "mlh_reed_solomon", "mlh_reed_solomon_brev",
    "mlh_merkle_commit_pairs", "mlh_merkle_commit", "mlh_merkle_batch_commit",
    "mlh_merkle_open", "mlh_merkle_open_pairs", "mlh_merkle_top",
    "mlh_fri_fold", "mlh_fri_prove", "mlh_fri_prove_gp",
    "mlh_fri_prover_init", "mlh_fri_prover_init_gp", "mlh_fri_prover_fold",
    "mlh_fri_prover_fold_gp",
    "mlh_batched_fri_prove", "mlh_batched_fri_prover_init",
    "mlh_shard_ntt_cross", "mlh_shard_fri_fold", "mlh_shard_fri_fold_commit",
    "mlh_shard_fri_fold_dr", "mlh_shard_fri_fold_commit_dr",
    "mlh_transcript_to_device", "mlh_transcript_from_device", "mlh_device_transcript_absorb",
    "mlh_device_fri_last",
    "mlh_sumcheck_sums_dev", "mlh_sumcheck_fold_sums_dr", "mlh_sumcheck_fold_dr",
    "mlh_device_sumcheck_round",
    "mlh_mle_to_coefficient", "mlh_mle_to_evaluation", "mlh_eq_table", "mlh_eq_table_rotate",
    "mlh_mle_evaluate", "mlh_mle_coeffs_evaluate", "mlh_poly_evaluate", "mlh_trace_evaluate",
    "mlh_sumcheck_partial_sums", "mlh_sumcheck_fold", "mlh_sumcheck_fold_and_sums",
    "mlh_sumcheck_prove", "mlh_sumcheck_prove_eq", "mlh_pcs_prove", "mlh_batched_pcs_prove",
    "mlh_cs_partial_sums", "mlh_cs_fold", "mlh_cs_fold_and_sums", "mlh_cs_sumcheck_prove",
    "mlh_cs_sumcheck_prove_sums",
    "mlh_system_prove", "mlh_system_prove_phased", "mlh_system_prove_shifted",
    "mlh_system_prove_public",
    "mlh_trace_columns", "mlh_trace_columns_range", "mlh_trace_commit", "mlh_trace_commit_range",
    "mlh_trace_extend_next", "mlh_trace_fill", "mlh_trace_fill_shaped", "mlh_trace_fill_public",
    "mlh_trace_column_sum", "mlh_trace_scan", "mlh_trace_scan_shaped", "mlh_trace_sort",
    "mlh_trace_sort_shaped", "mlh_trace_check", "mlh_trace_check_shaped",
    "mlh_trace_check_public", "mlh_trace_lookup_counts", "mlh_trace_lookup_counts_shaped",
    "mlh_trace_lookup_tuple_counts", "mlh_trace_lookup_tuple_counts_shaped",
}

_TRANSPORT = "multi-GPU entry: needs a transport; tests/test_sharded_*_gpu.py"
_MEMORY = "allocates, frees or copies a caller's buffer; computes nothing"
NOT_COVERED = {
    "mlh_sharded_ntt": _TRANSPORT,
    "mlh_sharded_ntt_batch": _TRANSPORT,
    "mlh_sharded_ntt_fused_batch": _TRANSPORT,
    "mlh_sharded_reed_solomon": _TRANSPORT,
    "mlh_sharded_commit_rs_code": _TRANSPORT,
    "mlh_sharded_fri_prove": _TRANSPORT,
    "mlh_sharded_eq_table": _TRANSPORT,
    "mlh_sharded_sumcheck_prove": _TRANSPORT,
    "mlh_bench_ntt": "a timing helper: mlh_ntt in place in a loop, covered as mlh_ntt",
    "mlh_free": _MEMORY,
    "mlh_memcpy_h2d": _MEMORY,
    "mlh_memcpy_d2h": _MEMORY,
}


# ---- the recorder and the arenas of the running test --------------------------------------

_RECORDED = set()
_ARENAS = []


class _Recorder:
    """libmlhip with a note of every mlh_* entry point that is called with a
    pointer into a live arena (a ctypes.c_void_p, as D.ptr gives it)."""

    def __init__(self, real):
        self.__dict__["_real"] = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("mlh_"):
            return fn

        def call(*args):
            for a in args:
                if isinstance(a, ctypes.c_void_p) and a.value and \
                        any(ar.contains(a.value) for ar in _ARENAS):
                    _RECORDED.add(name)
                    break
            return fn(*args)

        return call


@pytest.fixture(scope="module", autouse=True)
def _recording():
    real = _lib.load()
    _lib._lib = _Recorder(real)
    yield
    _lib._lib = real


@pytest.fixture(autouse=True)
def _arenas_end_with_the_test():
    yield
    del _ARENAS[:]


class Bufs:
    """The buffers of one call (or of one sequence of calls on the same data)."""

    def __init__(self, capacity=32 << 20):
        self.a = GA.Arena("cuda", capacity=capacity)
        _ARENAS.append(self.a)
        self._n = itertools.count()

    def _name(self, kind, name):
        return name or "%s%d" % (kind, next(self._n))

    def ro(self, array, name=None):
        return self.a.put(self._name("in", name), array)

    def rw(self, array, name=None):
        return self.a.put(self._name("inout", name), array, writable=True)

    def out(self, n_elems, name=None, may_stay=False):
        return self.a.hole(self._name("out", name), 16 * n_elems, may_stay=may_stay)

    def outb(self, nbytes, name=None, like="bytes", may_stay=False):
        return self.a.hole(self._name("out", name), nbytes, like=like, may_stay=may_stay)

    def done(self):
        ctx = D.context()
        D.check(D.lib().mlh_synchronize(ctx), ctx)
        self.a.verify()


class uploads_into:
    """For the block, D.to_device (and with it every test module's _dev / dev)
    places what it uploads in ``bufs``, and D.empty (the delta table of
    polynomials.eq_table) reserves a hole there.  writable: one flag for all,
    or the flags of the uploads in call order (the last one repeats)."""

    def __init__(self, bufs, writable):
        self.bufs = bufs
        self.flags = [writable] if isinstance(writable, bool) else list(writable)
        self.k = 0

    def _put(self, limbs, device=0):
        a = np.ascontiguousarray(limbs, dtype=np.uint32).reshape(-1, 4)
        w = self.flags[min(self.k, len(self.flags) - 1)]
        self.k += 1
        return self.bufs.rw(a) if w else self.bufs.ro(a)

    def _empty(self, n, device=0):
        return self.bufs.out(n)

    def __enter__(self):
        self.saved = D.to_device, D.empty
        D.to_device, D.empty = self._put, self._empty
        return self

    def __exit__(self, *exc):
        D.to_device, D.empty = self.saved
        return False


def _existing(fn, *args, writable, capacity=32 << 20):
    """An oracle comparison of another module, its uploads in one arena."""
    b = Bufs(capacity)
    with uploads_into(b, writable) as up:
        fn(*args)
    assert up.k > 0
    b.done()


def _call(name, *args):
    ctx = D.context()
    D.check(getattr(D.lib(), name)(ctx, *args), ctx)


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _ints(a):
    return D.limbs_to_ints(a)


def _limbs(v):
    return D.ints_to_limbs(v)


def _same(got, want):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and np.array_equal(got, want)


def _cpu(limbs):
    return torch.from_numpy(np.ascontiguousarray(limbs, dtype=np.uint32).view(np.int32).copy())


def _first_multi_block(blocks_of):
    return next(L for L in range(1, 20) if blocks_of(L) > 1)


# ---- field ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 4097])
@pytest.mark.parametrize("op", ["add", "sub", "mul", "neg", "scale", "inv", "inv_in_place"])
def test_field_ops(op, n):
    a, b = D.random_limbs(n, 11 + n), D.random_limbs(n, 12 + n)
    a[n // 2] = 0  # inv(0) = 0
    ai, bi = _ints(a), _ints(b)
    c = 0x0123456789ABCDEF0123456789ABCDEF % M
    want = {"add": lambda: [(u + v) % M for u, v in zip(ai, bi)],
            "sub": lambda: [(u - v) % M for u, v in zip(ai, bi)],
            "mul": lambda: [u * v % M for u, v in zip(ai, bi)],
            "neg": lambda: [-u % M for u in ai],
            "scale": lambda: [u * c % M for u in ai],
            "inv": lambda: [pow(u, M - 2, M) for u in ai]}[op.split("_")[0]]()
    B = Bufs()
    if op == "inv_in_place":
        x = B.rw(a)
        _call("mlh_field_inv", D.ptr(x), D.ptr(x), n)
        out = x
    else:
        x = B.ro(a)
        if op in ("add", "sub", "mul"):
            y, out = B.ro(b), B.out(n)
            _call("mlh_field_" + op, D.ptr(x), D.ptr(y), D.ptr(out), n)
        elif op == "scale":
            out = B.out(n)
            _call("mlh_field_scale", D.ptr(x), D.fe_bytes(c), D.ptr(out), n)
        else:
            out = B.out(n)
            _call("mlh_field_" + op, D.ptr(x), D.ptr(out), n)
    B.done()
    _same(out, _limbs(want))


# ---- transforms -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ntt_case(log_n, inverse):
    x = D.random_limbs(1 << log_n, 100 + log_n)
    g = F.pow_2_generator(log_n)
    ref = C.ntt_par if log_n > 16 else C.ntt
    return x, g, ref(x, log_n, g, inverse=inverse)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [1, 10, 11, 19])  # the small kernel (two sizes); one pass; three passes
def test_ntt(log_n, inverse, in_place):
    x, g, want = _ntt_case(log_n, inverse)
    B = Bufs()
    if in_place:
        src = out = B.rw(x)
    else:
        src, out = B.ro(x), B.out(1 << log_n)
    _call("mlh_intt" if inverse else "mlh_ntt", D.ptr(src), D.ptr(out), log_n, D.fe_bytes(g))
    B.done()
    _same(out, want)


def test_ntt_batch():
    log_n, log_batch = 11, 2
    g = F.pow_2_generator(log_n)
    x = D.random_limbs(1 << (log_n + log_batch), 111)
    want = np.concatenate([C.ntt(x[j << log_n:(j + 1) << log_n], log_n, g)
                           for j in range(1 << log_batch)])
    B = Bufs()
    src, out = B.ro(x), B.out(x.shape[0])
    _call("mlh_ntt_batch", D.ptr(src), D.ptr(out), log_n, D.fe_bytes(g), log_batch)
    B.done()
    _same(out, want)


def _bitrev(log_n):
    return np.array([int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0
                     for i in range(1 << log_n)])


@pytest.mark.parametrize("brev", [False, True])
@pytest.mark.parametrize("log_n", [0, 1, 11])
def test_reed_solomon(log_n, brev):
    g = F.pow_2_generator(log_n + 1)
    x = D.random_limbs(1 << log_n, 113 + log_n)
    given = np.ascontiguousarray(x[_bitrev(log_n)]) if brev else x
    B = Bufs()
    src, out = B.ro(given), B.out(2 << log_n)
    _call("mlh_reed_solomon_brev" if brev else "mlh_reed_solomon", D.ptr(src), log_n, D.fe_bytes(g),
          D.ptr(out))
    B.done()
    _same(out, C.reed_solomon(x, log_n, g))


def test_bit_reverse_permutation():
    log_n = 11
    x = D.random_limbs(1 << log_n, 114)
    B = Bufs()
    src, out = B.ro(x), B.out(1 << log_n)
    _call("mlh_bit_reverse_permutation", D.ptr(src), D.ptr(out), log_n)
    B.done()
    _same(out, np.ascontiguousarray(x[_bitrev(log_n)]))


def test_pow_2_generator_powers():
    log_n = 11
    B = Bufs()
    out = B.out(1 << log_n)
    _call("mlh_pow_2_generator_powers", log_n, D.ptr(out))
    B.done()
    _same(out, _limbs(F.pow_2_generator_powers(log_n)))


# ---- Merkle ---------------------------------------------------------------------------------

def _layers(B, leaves, name=None):
    return B.outb(32 * (2 * leaves - 1), name)


@pytest.mark.parametrize("with_root", [False, True])
@pytest.mark.parametrize("log_code", [1, 2, 11])
def test_merkle_commit_pairs(log_code, with_root):
    code = D.random_limbs(1 << log_code, 118 + log_code)
    want = C.merkle_commit_pairs(code, log_code)
    B = Bufs()
    src, out = B.ro(code), _layers(B, 1 << (log_code - 1))
    root = (ctypes.c_uint8 * 32)() if with_root else None
    _call("mlh_merkle_commit_pairs", D.ptr(src), log_code, D.ptr(out), root)
    B.done()
    assert _np(out).tobytes() == want.tobytes()
    if with_root:
        assert bytes(root) == want[-1].tobytes()


def _oracle_layers(tree):
    return b"".join(d for layer in tree.layers for d in layer)


@pytest.mark.parametrize("item_len,count", [(1, 8), (100, 16)])  # no multiple of a SHA-256 block
def test_merkle_commit_generic_items(item_len, count):
    rng = np.random.default_rng(item_len)
    items = rng.integers(0, 256, size=(count, item_len), dtype=np.uint64).astype(np.uint8)
    want = OM.Merkle.commit([bytes(x) for x in items])
    B = Bufs()
    src, out = B.ro(items.reshape(-1)), _layers(B, count)
    root = (ctypes.c_uint8 * 32)()
    _call("mlh_merkle_commit", D.ptr(src), item_len, count, D.ptr(out), root)
    B.done()
    assert _np(out).tobytes() == _oracle_layers(want) and bytes(root) == want.root()


def test_merkle_batch_commit():
    m, count, item_len = 3, 16, 33
    rng = np.random.default_rng(7)
    items = rng.integers(0, 256, size=(m, count, item_len), dtype=np.uint64).astype(np.uint8)
    want = OM.Merkle.batch_commit([[bytes(x) for x in batch] for batch in items])
    B = Bufs()
    src, out = B.ro(items.reshape(-1)), _layers(B, count)
    root = (ctypes.c_uint8 * 32)()
    _call("mlh_merkle_batch_commit", D.ptr(src), item_len, m, count, D.ptr(out), root)
    B.done()
    assert _np(out).tobytes() == _oracle_layers(want) and bytes(root) == want.root()


def test_merkle_open_and_open_pairs_three_indices():
    """The tree and the code are read-only inputs of both calls."""
    log_code = 9
    code = TG.rand_vals(1 << log_code, 909)
    ot = OF.commit_rs_code(code)
    leaves, depth = 1 << (log_code - 1), log_code - 1
    idx = [0, leaves - 1, 77]
    ia = (ctypes.c_uint64 * 3)(*idx)
    B = Bufs()
    dcode = B.ro(_limbs(code), "code")
    tree = B.ro(C.merkle_commit_pairs(_limbs(code), log_code).reshape(-1), "layers")
    out = (ctypes.c_uint8 * (3 * 32 * depth))()
    _call("mlh_merkle_open", D.ptr(tree), leaves, ia, 3, out)
    out2 = (ctypes.c_uint8 * (3 * 32 * (1 + depth)))()
    _call("mlh_merkle_open_pairs", D.ptr(dcode), log_code, D.ptr(tree), depth, ia, 3, out2)
    B.done()
    assert bytes(out) == b"".join(bytes(s) for i in idx for s, _ in ot.open(i)[1])
    assert bytes(out2) == b"".join(OF.pair_bytes(code[i], code[i + leaves]) +
                                   b"".join(bytes(s) for s, _ in ot.open(i)[1]) for i in idx)


# ---- the rank-local steps of the sharded provers, on one device -------------------------------
#
# tests/dist_spec.HipOps makes each call; here its buffers come from the arena.
# tests/dist_cpu_ops.CpuOps is the same interface computed by the oracle.

class ArenaOps(DS.HipOps):
    def __init__(self, bufs):
        super().__init__(0)
        self.b = bufs

    def empty(self, n):
        return self.b.out(n)

    def empty_tree(self, leaves):
        return self.b.outb(int(D.lib().mlh_merkle_layers_bytes(leaves)))

    def dev_transcript(self, transcript):
        st = self.b.outb(int(D.lib().mlh_device_transcript_bytes()), "state")
        _call("mlh_transcript_to_device", transcript.h, D.ptr(st))
        return st

    def host_transcript(self, state):
        tr = Transcript()
        _call("mlh_transcript_from_device", D.ptr(state), tr.h)
        return tr


CPU = DC.CpuOps()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n,log_p,rank", [(12, 2, 3), (14, 1, 1)])  # world 4 and world 2
def test_shard_ntt_cross(log_n, log_p, rank, inverse):
    x = D.random_limbs(1 << (log_n - log_p), 400 + log_n)
    g = F.pow_2_generator(log_n)
    B = Bufs()
    got = ArenaOps(B).cross(B.ro(x), log_n, log_p, rank, g, inverse)
    B.done()
    _same(got, _np(CPU.cross(_cpu(x), log_n, log_p, rank, g, inverse)))


# (log_local, k, log_domain, log_s, log_p, rank): a layer of 2^(log_local + log_p) = 2^(log_domain - k)
SHARD_FOLDS = [(10, 1, 13, 8, 2, 3), (9, 0, 10, 7, 1, 1)]


@pytest.mark.parametrize("dr", [False, True])
@pytest.mark.parametrize("commit", [False, True])
@pytest.mark.parametrize("log_local,k,log_domain,log_s,log_p,rank", SHARD_FOLDS)
def test_shard_fri_fold(log_local, k, log_domain, log_s, log_p, rank, commit, dr):
    layer = D.random_limbs(1 << log_local, 410 + log_local)
    r = 0x0FEDCBA9876543210FEDCBA987654321 % M
    B = Bufs()
    ops = ArenaOps(B)
    src = B.ro(layer, "layer")
    rarg = B.ro(_limbs([r]), "r") if dr else r
    fn = getattr(ops, "fold" + ("_commit" if commit else "") + ("_dr" if dr else ""))
    got = fn(src, k, log_domain, rarg, log_s, log_p, rank)
    B.done()
    want = CPU.fold(_cpu(layer), k, log_domain, r, log_s, log_p, rank)
    if commit:
        _same(got[0], _np(want))
        assert _np(got[1]).tobytes() == CPU.commit_pairs(want).numpy().tobytes()
    else:
        _same(got, _np(want))


def test_merkle_top():
    P, per_rank = 4, 8
    rng = np.random.default_rng(3)
    gathered = rng.integers(0, 256, size=32 * P * per_rank, dtype=np.uint64).astype(np.uint8)
    B = Bufs()
    got = ArenaOps(B).merkle_top(B.ro(gathered), P, per_rank)
    B.done()
    assert _np(got).tobytes() == CPU.merkle_top(torch.from_numpy(gathered), P, per_rank).numpy().tobytes()


def _started():
    tr = Transcript()
    tr.absorb(b"caller buffers")
    return tr


@pytest.mark.parametrize("nbytes", [100, 32])  # the byte path and the word path
def test_device_transcript(nbytes):
    """to_device, absorb with a challenge written to HBM, from_device."""
    rng = np.random.default_rng(nbytes)
    src = rng.integers(0, 256, size=nbytes, dtype=np.uint64).astype(np.uint8)
    want = _started()
    want.absorb(src.tobytes())
    B = Bufs()
    ops = ArenaOps(B)
    state = ops.dev_transcript(_started())
    dsrc, ch = B.ro(src, "src"), B.out(1, "challenge")
    ops.absorb(state, dsrc, ch)
    got = ops.host_transcript(state)
    B.done()
    assert got.random() == want.random()
    assert _ints(_np(ch)) == [want.next_challenge()]


@pytest.mark.parametrize("equal", [True, False])
def test_device_fri_last(equal):
    v = D.random_limbs(2, 420)
    if equal:
        v[1] = v[0]
    want = _started()
    B = Bufs()
    ops = ArenaOps(B)
    state = ops.dev_transcript(_started())
    vals, flag, last = B.ro(v, "vals2"), B.outb(4, "flag", like="words"), B.out(1, "last")
    ops.fri_last(vals, state, flag, last)
    got = ops.host_transcript(state)
    B.done()
    want.absorb(v[0].tobytes())
    assert got.random() == want.random()
    assert int(_np(flag)[0]) == (0 if equal else 1)
    _same(last, v[:1])


def test_device_sumcheck_steps():
    """mlh_sumcheck_sums_dev, the device round, fold + sums with the challenge
    read from HBM, then the plain fold with it: one round and a half at 2^10,
    every buffer in one arena."""
    L = 10
    m0, d0 = D.random_limbs(1 << L, 430), D.random_limbs(1 << L, 431)
    claim = 0x00112233445566778899AABBCCDDEEFF % M
    # the oracle's run, on host tensors
    cm, cd = _cpu(m0), _cpu(d0)
    cs, cprev, cstate = CPU.empty(2), CPU.const(claim), _started()
    cpoly, cr, cs2 = CPU.empty(2), CPU.empty(1), CPU.empty(2)
    CPU.sc_sums_dev(cm, cd, L, cs)
    CPU.sc_round(cs, 1, cprev, cstate, cpoly, cr)
    CPU.sc_fold_sums_dr(cm, cd, L, cr, cs2)
    CPU.sc_fold_dr(cm, cd, L - 1, cr)
    B = Bufs()
    ops = ArenaOps(B)
    m, d = B.rw(m0, "matrix"), B.rw(d0, "delta")
    sums, prev = B.out(2, "sums"), B.rw(_limbs([claim]), "prev")
    state = ops.dev_transcript(_started())
    ops.sc_sums_dev(m, d, L, sums)
    B.done()  # the tables are inputs of this call: still what they were
    _same(m, m0)
    _same(d, d0)
    poly, r, sums2 = B.out(2, "poly"), B.out(1, "r"), B.out(2, "sums2")
    ops.sc_round(sums, 1, prev, state, poly, r)
    ops.sc_fold_sums_dr(m, d, L, r, sums2)
    ops.sc_fold_dr(m, d, L - 1, r)
    got_state = ops.host_transcript(state)
    B.done()
    for got, want in ((sums, cs), (poly, cpoly), (r, cr), (prev, cprev), (sums2, cs2),
                      (m[:1 << (L - 2)], cm[:1 << (L - 2)]), (d[:1 << (L - 2)], cd[:1 << (L - 2)])):
        _same(got, _np(want))
    assert got_state.random() == cstate.random()


# ---- FRI ------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_domain,k", [(12, 2), (11, 0)])
def test_fri_fold(log_domain, k):
    n = 1 << (log_domain - k)
    layer = D.random_limbs(n, 117 + k)
    r = 0x0FEDCBA9876543210FEDCBA987654321 % M
    li = _ints(layer)
    want = OF.fold_layer([(li[i], li[i + n // 2]) for i in range(n // 2)],
                         F.pow_2_generator_powers(log_domain), k, r)
    B = Bufs()
    src, out = B.ro(layer), B.out(n // 2)
    _call("mlh_fri_fold", D.ptr(src), log_domain - k, k, log_domain, D.fe_bytes(r), D.ptr(out))
    B.done()
    _same(out, _limbs(want))


def _fri_prove(buf, gp):
    tr = TSC._started()
    p = MF.FriProof.prove(buf, tr, gen_pows=gp)
    return TSC._fri_view(p), tr.random()


@pytest.mark.parametrize("gp", [False, True])
@pytest.mark.parametrize("log_code", [2, 9])
def test_fri_prove(log_code, gp):
    """The code is not modified; the proof goes to host buffers."""
    code, want, digest = TSC._fri_case(log_code - 1, 209)
    B = Bufs()
    got = _fri_prove(B.ro(code, "code"), (F.pow_2_generator(log_code), log_code) if gp else None)
    B.done()
    assert got == (want, digest)


@pytest.mark.parametrize("gp", [False, True])
def test_fri_prove_two_elements_is_refused_and_touches_nothing(gp):
    """log_code = 1: the reference's fold leaves no last element and panics
    (fri/mod.rs:136-145); here MLH_ERR_INVALID, and nothing is written."""
    B = Bufs()
    buf = B.ro(D.random_limbs(2, 5), "code")
    with pytest.raises(_lib.MlhError) as e:
        _fri_prove(buf, (F.pow_2_generator(1), 1) if gp else None)
    assert e.value.status == _lib.MLH_ERR_INVALID
    B.done()


def test_fri_prover_step_api():
    """init, fold_step for every k, open_query at 2^9."""
    _existing(TG.test_fri_prover_step_api, writable=False)


def test_fri_prover_fold_step_gp():
    """init and fold_step_gp with the caller's table, steps that are refused included."""
    _existing(TG.test_fri_prover_fold_step_gp_reference_signature, 8, writable=False)


def test_fri_prover_fold_and_open_queries_129():
    """fold, then 129 indices: they travel through device memory."""
    _existing(TG.test_fri_prover_open_queries_many, 129, writable=False)


def test_fri_prover_init_gp_and_fold_gp():
    log_n = 8
    L = log_n + 1
    gp = F.pow_2_generator_powers(L)
    code = OF.reed_solomon(TG.rand_vals(1 << log_n, 3), gp[1])
    otr = OT.Transcript()
    opd = OF.FriProverData.fold(gp, code, otr)
    B = Bufs()
    buf = B.ro(_limbs(code), "code")
    tr = Transcript()
    pd = MF.FriProverData.fold(buf, tr, gen_pows=(gp[1], L))
    assert pd.fold_roots() == opd.fold_roots() and pd.last_element == opd.last_element
    assert tr.random() == otr.random()
    tr2 = Transcript()
    pd2 = MF.FriProverData.init(buf, tr2, gen_pows=(gp[1], L))
    for k in range(log_n):
        pd2.fold_step(k, tr2.next_challenge(), tr2)  # folds with the table given at init
    assert pd2.fold_roots() == opd.fold_roots() and tr2.random() == otr.random()
    q, wq = pd2.open_query_at(37, L), opd.open_query_at(37)
    assert [v for v, _ in q] == [v for v, _ in wq]
    assert [s for _, s in q] == [[s for s, _ in path] for _, path in wq]
    B.done()


@pytest.mark.parametrize("m,log_n", [(3, 9), (5, 2)])
def test_batched_fri_prove(m, log_n):
    codes, want, digest = TSC._batched_fri_case(m, log_n, 230)
    B = Bufs()
    got = TSC._batched_fri_call(m)(B.ro(codes, "codes"))
    B.done()
    assert got == (want, digest)


@pytest.mark.parametrize("m,log_n", [(3, 9), (5, 2)])
def test_batched_fri_prover_step_api(m, log_n):
    _existing(TG.test_batched_fri_prover_step_api_reference_shape, m, log_n, writable=False)


# ---- polynomials ----------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["to_coefficient", "to_evaluation"])
@pytest.mark.parametrize("log_n", [1, 13])
def test_mobius(log_n, which):
    ev = D.random_limbs(1 << log_n, 119 + log_n)
    co = C.to_coefficient(ev.copy(), log_n)
    given, want = (ev, co) if which == "to_coefficient" else (co, ev)
    B = Bufs()
    buf = B.rw(given)
    _call("mlh_mle_" + which, D.ptr(buf), log_n)
    B.done()
    _same(buf, want)


@pytest.mark.parametrize("n", [1, 13])
def test_eq_table(n):
    pts = _ints(D.random_limbs(n, 120 + n))
    B = Bufs()
    out = B.out(1 << n)
    _call("mlh_eq_table", CS._elems(pts), n, D.ptr(out))
    B.done()
    _same(out, C.eq_table(pts))


def test_eq_table_rotate():
    log_n = 5
    src = D.random_limbs(1 << log_n, 95)
    B = Bufs()
    a, out = B.ro(src), B.out(1 << log_n)
    _call("mlh_eq_table_rotate", D.ptr(a), log_n, D.ptr(out))
    B.done()
    _same(out, np.roll(np.ascontiguousarray(src), 1, axis=0))


@pytest.mark.parametrize("m,n", [(1, 0), (6, 3), (1000, 10)])
def test_mle_evaluations(m, n):
    """A table shorter than 2^n is zero padded by the caller, as
    multilinear_amd.polynomials does: the padded table is the device input."""
    v = TG.rand_vals(m, 90 + m)
    args = TG.rand_vals(n, 91 + n)
    padded = _limbs(v + [0] * ((1 << n) - m))
    for name, want in (("mlh_mle_evaluate", OPL.mle_evaluate(v, args)),
                       ("mlh_mle_coeffs_evaluate", OPL.mle_coeffs_evaluate(v, args))):
        B = Bufs()
        out = (ctypes.c_uint8 * 16)()
        _call(name, D.ptr(B.ro(padded)), n, CS._elems(args) if n else (ctypes.c_uint8 * 1)(), out)
        B.done()
        assert D.fe_from_bytes(out) == want, name


@pytest.mark.parametrize("n", [1, 5, 4097])
def test_poly_evaluate(n):
    c = TG.rand_vals(n, 80 + n % 97)
    x = TG.rand_vals(1, 81)[0]
    B = Bufs()
    out = (ctypes.c_uint8 * 16)()
    _call("mlh_poly_evaluate", D.ptr(B.ro(_limbs(c))), n, D.fe_bytes(x), out)
    B.done()
    assert D.fe_from_bytes(out) == OPL.uni_evaluate(c, x)


@pytest.mark.parametrize("n,w", [(0, 5), (5, 3), (4, 513)])
def test_trace_evaluate(n, w):
    mat = TG.rand_vals(w << n, 40 + w)
    pts = TG.rand_vals(n, 41)
    B = Bufs()
    out = (ctypes.c_uint8 * (16 * w))()
    _call("mlh_trace_evaluate", D.ptr(B.ro(_limbs(mat))), n, w,
          CS._elems(pts) if n else (ctypes.c_uint8 * 1)(), out)
    B.done()
    assert CS._split(out, w) == OS.trace_evaluate(mat, w, pts)


# ---- sumcheck and PCS -------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 10])
def test_sumcheck_steps(L):
    """Partial sums (tables read only), fold, fold_and_sums."""
    m0, d0 = D.random_limbs(1 << L, 125 + L), D.random_limbs(1 << L, 126 + L)
    r = 0x00112233445566778899AABBCCDDEEFF % M
    half = 1 << (L - 1)
    tab = R.SumcheckTables(_ints(m0), 1, 1 << L, _ints(d0))
    B = Bufs()
    m, d = B.ro(m0, "matrix"), B.ro(d0, "delta")
    out = (ctypes.c_uint8 * 32)()
    _call("mlh_sumcheck_partial_sums", D.ptr(m), D.ptr(d), L, out)
    B.done()
    assert tuple(CS._split(out, 2)) == C.partial_sums(m0, d0, L)
    tab.fold(r)
    B = Bufs()
    m, d = B.rw(m0, "matrix"), B.rw(d0, "delta")
    _call("mlh_sumcheck_fold", D.ptr(m), D.ptr(d), L, D.fe_bytes(r))
    B.done()
    _same(m[:half], _limbs(tab.matrix))
    _same(d[:half], _limbs(tab.delta))
    if L >= 2:
        B = Bufs()
        m, d = B.rw(m0, "matrix"), B.rw(d0, "delta")
        _call("mlh_sumcheck_fold_and_sums", D.ptr(m), D.ptr(d), L, D.fe_bytes(r), out)
        B.done()
        _same(m[:half], _limbs(tab.matrix))
        _same(d[:half], _limbs(tab.delta))
        assert tuple(CS._split(out, 2)) == C.partial_sums(_limbs(tab.matrix), _limbs(tab.delta), L - 1)


def _pcs_rounds(n, seed):
    """The oracle's sumcheck rounds of build_tables_for_pcs tables."""
    ev = D.random_limbs(1 << n, seed)
    pts = _ints(D.random_limbs(n, seed + 1))
    evi = _ints(ev)
    total = OPL.mle_evaluate(evi, pts)
    ot = OS.SumcheckTables.build_tables_for_pcs(pts, evi)
    otr = OT.Transcript()
    otr.absorb(b"stream")
    prev, polys, rs = total, [], []
    for _ in range(n):
        nz, r2, prev = ot.compute_sumcheck_polynomial(prev, otr)
        polys.append(tuple(nz))
        rs.append(r2)
    return ev, pts, total, polys, rs, otr.random(), ot.matrix[0], ot.delta[0]


def _round_outputs(n, polys, rs):
    flat = CS._split(polys, 2 * n)
    return [tuple(flat[2 * k:2 * k + 2]) for k in range(n)], CS._split(rs, n)


@pytest.mark.parametrize("n", [1, 2, 13])
def test_sumcheck_prove(n):
    ev, pts, total, want_polys, want_rs, digest, m_last, d_last = _pcs_rounds(n, 140 + n)
    B = Bufs()
    m, d = B.rw(ev, "matrix"), B.rw(C.eq_table(pts), "delta")
    tr = TSC._started()
    polys, rs = (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * (16 * n))()
    _call("mlh_sumcheck_prove", D.ptr(m), D.ptr(d), n, D.fe_bytes(total), tr.h, polys, rs)
    B.done()
    assert _round_outputs(n, polys, rs) == (want_polys, want_rs) and tr.random() == digest
    assert _ints(_np(m[:1])) == [m_last] and _ints(_np(d[:1])) == [d_last]


@pytest.mark.parametrize("n", [3, 13])  # 13: one eq-factored head round
def test_sumcheck_prove_eq(n):
    """dev_evals is read only; dev_work, from the arena, receives the folds."""
    ev, pts, total, want_polys, want_rs, digest, m_last, d_last = _pcs_rounds(n, 210 + n)
    B = Bufs()
    buf, work = B.ro(ev, "evals"), B.out(1 << (n - 1), "work")
    tr = TSC._started()
    polys, rs, dl = (ctypes.c_uint8 * (32 * n))(), (ctypes.c_uint8 * (16 * n))(), (ctypes.c_uint8 * 16)()
    _call("mlh_sumcheck_prove_eq", D.ptr(buf), D.ptr(work), n, CS._elems(pts), D.fe_bytes(total), tr.h,
          polys, rs, dl)
    B.done()
    assert _round_outputs(n, polys, rs) == (want_polys, want_rs) and tr.random() == digest
    assert _ints(_np(work[:1])) == [m_last] and D.fe_from_bytes(dl) == d_last


@pytest.mark.parametrize("rounds", ["fused", "cooperative"])
@pytest.mark.parametrize("n", [1, 2, 13])
def test_pcs_prove(n, rounds):
    ev, pts, out, want = TSC._pcs_case(n, 220)
    B = Bufs()
    buf = B.ro(ev, "evals")
    with TSC._fused_max(24 if rounds == "fused" else 0):
        got = TSC._pcs_call(pts, out)(buf)
    B.done()
    assert got == want


@pytest.mark.parametrize("m,n", [(2, 10), (3, 5)])
def test_batched_pcs_prove(m, n):
    from oracle import batched as OB

    polys = [_ints(D.random_limbs(1 << n, 240 + 10 * n + j)) for j in range(m)]
    pts = _ints(D.random_limbs(n, 243 + n))
    outs = [OPL.mle_evaluate(p, pts) for p in polys]
    otr = OT.Transcript()
    otr.absorb(b"stream")
    w = OB.BatchedPCSProof.prove(pts, outs, polys, otr)
    B = Bufs()
    buf = B.ro(_limbs([v for p in polys for v in p]), "evals")
    tr = TSC._started()
    p = MB.BatchedPCSProof.prove(pts, outs, buf, tr)
    B.done()
    assert [tuple(x) for x in p.sumcheck_polynomials] == [tuple(x) for x in w.sumcheck_polynomials]
    assert TSC._batched_view(p.fri_proof) == TSC._batched_want(w.fri_proof)
    assert tr.random() == otr.random()


# ---- constraint systems -------------------------------------------------------------------------

def test_cs_step_api():
    """mlh_cs_partial_sums (tables read only: the module compares them), mlh_cs_fold
    and mlh_cs_fold_and_sums on quad3."""
    _existing(TCS.test_step_api_matches_model, "quad3", writable=True)


@pytest.mark.parametrize("name", ["deg5_w7", "wide32"])
def test_cs_sumcheck_prove(name):
    inputs, call, want = TSC._cs_prove_case(name)
    B = Bufs()
    got = call(B.rw(inputs[0], "matrix"), B.rw(inputs[1], "delta"))
    B.done()
    assert got == want


@pytest.mark.parametrize("name", ["deg5_w7", "wide32"])
def test_cs_sumcheck_prove_sums(name):
    """The claim with sum columns, against the phased model's rounds."""
    _existing(TP.test_prove_sums_matches_model, name, writable=True)


@pytest.mark.parametrize("name", ["quad3", "deg5_w7"])
def test_system_prove(name):
    """mlh_trace_commit reads the first upload; mlh_system_prove folds the second."""
    _existing(TSY.test_prove_matches_model_and_verifies, name, writable=[False, True])


def test_system_prove_phased():
    _existing(TP.test_prove_matches_model_and_verifies, "deg5_w7", writable=True)


def test_system_prove_shifted():
    """dev_matrix is not modified."""
    _existing(TSH.test_prove_matches_model_and_verifies, "mixed5", writable=False)


def test_system_prove_public():
    """The first upload takes the strip (mlh_trace_fill_public); the second is
    the trace the prover reads and does not modify."""
    _existing(TPUB.test_prove_matches_model_and_verifies, "pmixed5", writable=[True, False])


# ---- trace operations ------------------------------------------------------------------------------
#
# Each at the first height whose launch has more than one block; widths 7 and 5.

def _columns_info(L, W, col0=None, ncols=None):
    rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
    if col0 is None:
        st = D.lib().mlh_trace_columns_launch_info(L, W, ctypes.byref(rows), ctypes.byref(blocks))
    else:
        st = D.lib().mlh_trace_columns_range_launch_info(L, W, col0, ncols, ctypes.byref(rows),
                                                         ctypes.byref(blocks))
    assert st == 0
    return rows.value, blocks.value


def test_trace_columns():
    W = 7
    L = _first_multi_block(lambda L: _columns_info(L, W)[1])
    a = D.random_limbs(W << L, 121)
    B = Bufs()
    src, out = B.ro(a), B.out(W << L)
    _call("mlh_trace_columns", D.ptr(src), L, W, D.ptr(out))
    B.done()
    _same(out, np.ascontiguousarray(a.reshape(1 << L, W, 4).transpose(1, 0, 2)).reshape(-1, 4))


def test_trace_columns_range():
    W, col0, ncols = 7, 2, 3
    L = _first_multi_block(lambda L: _columns_info(L, W, col0, ncols)[1])
    a = D.random_limbs(W << L, 122)
    B = Bufs()
    src, out = B.ro(a), B.out(ncols << L)
    _call("mlh_trace_columns_range", D.ptr(src), L, W, col0, ncols, D.ptr(out))
    B.done()
    want = a.reshape(1 << L, W, 4)[:, col0:col0 + ncols].transpose(1, 0, 2)
    _same(out, np.ascontiguousarray(want).reshape(-1, 4))


def test_trace_commit_and_commit_range_roots():
    """The trace is read only; the roots are the models'."""
    _existing(TSY.test_commit_root, "deg5_w7", writable=False)
    mo = TP.PR.model("deg5_w7")
    L, W, P = mo["log_height"], mo["width"], mo["pre"]
    assert 0 < P < W
    B = Bufs()
    m = B.ro(_limbs(mo["matrix"]), "trace")
    roots = []
    for col0, ncols in ((0, P), (P, W - P)):
        st, h = TP._commit(m, L, W, col0, ncols)
        assert st == 0, D.lib().mlh_last_error(D.context())
        roots.append(TP._root(h))
        D.lib().mlh_trace_commitment_destroy(h)
    B.done()
    assert roots == [mo["root1"], mo["root2"]]


def test_trace_commit_range_at_several_blocks():
    """No model at this height: the root over columns [2, 5) of a 7-wide trace
    equals the root over the same three columns as a trace of their own."""
    W, col0, ncols = 7, 2, 3
    L = _first_multi_block(lambda L: _columns_info(L, W, col0, ncols)[1])
    a = D.random_limbs(W << L, 123)
    own = np.ascontiguousarray(a.reshape(1 << L, W, 4)[:, col0:col0 + ncols]).reshape(-1, 4)
    B = Bufs()
    wide, narrow = B.ro(a, "trace"), B.ro(own, "columns")
    roots = []
    for args in ((wide, W, col0, ncols), (narrow, ncols, 0, ncols)):
        h = ctypes.c_void_p()
        _call("mlh_trace_commit_range", D.ptr(args[0]), L, args[1], args[2], args[3], ctypes.byref(h))
        roots.append(TP._root(h))
        D.lib().mlh_trace_commitment_destroy(h)
    h = ctypes.c_void_p()
    _call("mlh_trace_commit", D.ptr(narrow), L, ncols, ctypes.byref(h))
    roots.append(TP._root(h))
    D.lib().mlh_trace_commitment_destroy(h)
    B.done()
    assert roots[0] == roots[1] == roots[2]


def test_trace_extend_next():
    W, cols = 7, [6, 4, 2]
    K = len(cols)
    L = _first_multi_block(lambda L: TSH._extend_info(L, W, K)[1])
    a = D.random_limbs(W << L, 124)
    T = a.reshape(1 << L, W, 4)
    want = np.concatenate([T, np.roll(T, -1, axis=0)[:, cols]], axis=1)
    B = Bufs()
    src, out = B.ro(a), B.out((W + K) << L)
    _call("mlh_trace_extend_next", D.ptr(src), L, W, (ctypes.c_uint32 * K)(*cols), K, D.ptr(out))
    B.done()
    _same(out, np.ascontiguousarray(want).reshape(-1, 4))


def _fill(shape):
    """The whole matrix against the model: the columns that are no output too."""
    W, prog = 7, TSC._fill_w7()
    L = _first_multi_block(lambda L: prog.launch_info(L)[2]) if shape is None else 8
    a = D.random_limbs(W << L, 125)
    a[5 * W + 1] = _limbs([0x1234567890ABCDEF1234567890ABCDEF % M])[0]  # a zero denominator
    rnd = [0x1234567890ABCDEF1234567890ABCDEF % M]
    B = Bufs()
    buf = B.rw(a)
    if shape is None:
        _call("mlh_trace_fill", prog.h, D.ptr(buf), L, W, CS._elems(rnd))
    else:
        _call("mlh_trace_fill_shaped", prog.h, D.ptr(buf), L, W, CS._elems(rnd), *shape)
    B.done()
    _same(buf, _limbs(FR.fill_matrix(prog.wire, _ints(a), rnd)))


def test_trace_fill():
    _fill(None)


def test_trace_fill_shaped():
    _fill((64, 2))  # 2^8 rows: two chunks of 128 rows


def test_trace_fill_public():
    W, Fn = 7, 3
    L = _first_multi_block(lambda L: CS.public_fill_launch_info(L, W, Fn)[1])
    descs = TPUB._case(L, W, Fn)
    spec = PUB.builder(descs)
    a = D.random_limbs(W << L, 126)
    want = a.reshape(1 << L, W, 4).copy()
    want[:, W - Fn:] = TPUB.np_strip(descs, 1 << L)
    B = Bufs()
    buf = B.rw(a)
    _call("mlh_trace_fill_public", spec.h, D.ptr(buf), L, W)
    B.done()
    _same(buf, want.reshape(-1, 4))


def test_trace_column_sum():
    L, W, mask = 11, 7, 0b1000101
    a = D.random_limbs(W << L, 127)
    ai = _ints(a)
    want = sum(ai[i * W + j] for i in range(1 << L) for j in range(W) if (mask >> j) & 1) % M
    B = Bufs()
    out = (ctypes.c_uint8 * 16)()
    _call("mlh_trace_column_sum", D.ptr(B.ro(a)), L, W, mask, out)
    B.done()
    assert D.fe_from_bytes(out) == want


# (threads, rows per thread, max blocks): four tiles of 128 rows on three blocks at 2^9, the last block empty
EMPTY_LAST_BLOCK = (64, 2, 3)


def test_trace_scan_and_scan_shaped():
    W = 7
    scans = [("add", 2, 0, 5), ("mul", 6, 6, 3), ("add", 0, 4, 7)]
    L = _first_multi_block(lambda L: CS.trace_scan_launch_info(L, W, len(scans))[2])
    _existing(TSCAN._check, D.random_limbs(W << L, 128), W, scans, [None], writable=True)
    _existing(TSCAN._check, D.random_limbs(W << 9, 129), W, scans, [EMPTY_LAST_BLOCK], writable=True)


def test_trace_sort_and_sort_shaped():
    W = 5
    L = _first_multi_block(lambda L: CS.trace_sort_launch_info(L, W, 2)[2])
    _existing(TSORT._check, D.random_limbs(W << L, 130), W, [4, 2], [(2, 0), (4, 1)], 3, [None],
              writable=True)
    rows = 1 << 9
    rng = np.random.default_rng(131)
    mat = TSORT._with_keys(W, rows, 132, {4: [int(v) for v in rng.integers(0, 1 << 16, size=rows)]})
    _existing(TSORT._check, mat, W, [4, 2], [(2, 0), (4, 1)], 3, [EMPTY_LAST_BLOCK], writable=True)


def test_trace_check_and_check_shaped():
    """The trace is read only (the module compares it too)."""
    name = "mixed5"
    prog, shifts, fns, W, rnd = TCHK._system(name)
    L = _first_multi_block(lambda L: CS.trace_check_launch_info(prog, L)[1])
    for LL, shapes in ((L, [None]), (8, [(64, 3)])):  # four chunks of 64 rows on three blocks
        vals = TCHK._matrix(name, LL)
        want = TCHK.CR.check(fns, vals, W, shifts, LL, rnd)
        _existing(TCHK._all_shapes, vals, W, prog, shifts, rnd, want, shapes, writable=False)


def test_trace_check_public():
    W, C_, L = 7, 4, 9
    descs = TPUB._case(L, W, W - C_)
    spec = PUB.builder(descs)
    committed = TCHK.PF.matrix("caller strip", 1 << L, C_)
    good = PUB.with_strip(committed, C_, descs, 1 << L)
    bad = list(good)
    row = (1 << L) - 1
    bad[row * W + C_ + 1] = (bad[row * W + C_ + 1] + 1) % M
    for vals in (good, bad):
        B = Bufs()
        got = TCHK._public(B.ro(_limbs(vals)), W, spec)
        B.done()
        assert got == TCHK.CR.check_public(vals, W, descs, L)


def test_trace_lookup_counts_and_shaped():
    W, values, T, Cc = TL.LAYOUTS[2]  # width 5, three value columns
    L = _first_multi_block(lambda L: CS.lookup_counts_launch_info(L, len(values))[1])
    matrix = TL._inputs(L, W, values, T, Cc, "uniform", "caller")
    _existing(TL._check, matrix, L, W, values, T, Cc,
              [dict(log_slots=L + 1, hash_bits=3, max_blocks=2, flags=1)], writable=True)


def test_trace_lookup_tuple_counts_and_shaped():
    arity, n_tuples = 2, 1
    W, tuples, table, Cc = TLT._layout(arity, n_tuples, spare=2)
    assert W == 7
    L = _first_multi_block(lambda L: CS.lookup_tuple_counts_launch_info(L, n_tuples)[1])
    matrix = TLT._inputs(L, W, tuples, table, "uniform", "caller")
    _existing(TLT._check, matrix, L, W, tuples, table, Cc, None,
              [dict(log_slots=L + 1, hash_bits=3, max_blocks=2, flags=1)], writable=True)


# ---- last: every entry point of COVERED was called with a pointer into an arena ---------------------

def test_every_covered_entry_point_was_called_on_arena_buffers():
    assert COVERED - _RECORDED == set()
