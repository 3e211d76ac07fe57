"""Scratch independence: every family of the single-GPU C ABI again, bit-exact
against the oracle, with mlh_set_scratch_poison on.

Pool blocks, the context's fixed scratch (reduction partials, the 64-element
scratch, the NTT ping-pong buffer, the pinned staging) and new cache tables
come from hipMalloc or hold what an earlier, usually identical, call left: a
kernel that reads a scratch word it never wrote gets a plausible value and the
other tests pass.  With the poison every such buffer holds the word 3 before
it is used: as a field element (3, 3, 3, 3) is canonical and nonzero, so a
stale element changes a sum or a digest; as a count or an index 3 is small, so
a stale index reads a wrong entry of the same buffer.  A stale read is a
mismatch with the oracle, never a fault.

The cases are the existing oracle comparisons of the other GPU modules, run
here under the poison (set again before each), and "history" pairs: the pool
hands a request a block of up to 1.25 x its size, so a smaller call inherits a
larger call's bytes."""
import ctypes

import pytest

import test_cs_sumcheck_gpu as TCS
import test_gpu_parity as TG
import test_phased_proof_gpu as TP
import test_public_columns_gpu as TPUB
import test_shifted_proof_gpu as TSH
import test_stream_contract_gpu as TSC
import test_system_proof_gpu as TSY
import test_trace_fill_gpu as TF
import test_trace_lookup_gpu as TL
import test_trace_lookup_tuple_gpu as TLT
from multilinear_amd import _lib
from multilinear_amd import constraint_system as CS
from multilinear_amd import device as D
from oracle import fri as OF
from oracle import merkle as OM

pytestmark = pytest.mark.gpu

WORD = 3


class poison:
    """mlh_set_scratch_poison(WORD) for the block; off after it."""

    def __enter__(self):
        again()
        return self

    def __exit__(self, *exc):
        ctx = D.context()
        D.check(D.lib().mlh_set_scratch_poison(ctx, 0), ctx)
        return False


def again():
    """Before each operation under test: the fixed scratch is filled anew."""
    ctx = D.context()
    D.check(D.lib().mlh_set_scratch_poison(ctx, WORD), ctx)


def _first_multi_block(info, *args):
    return next(L for L in range(1, 17) if info(L, *args)[1] > 1)


# (test function of another module, its arguments): each compares with the oracle
CASES = [
    # the families of test_stream_contract_gpu.py, section B, at its shapes
    (TG.test_merkle_commit_pairs_matches_oracle, (11,)),
    (TG.test_mle_evaluations_any_length, (1 << 9, 9)),
    (TG.test_trace_evaluate_matches_oracle, (9, 7)),
    (TG.test_sumcheck_rounds_match_oracle, ()),  # partial sums, fold, prove at 2^10
    (TF.test_column_sum_matches_python, (9, 32, 0xFFFFFFFF)),
    (TCS.test_step_api_matches_model, ("quad3",)),  # mlh_cs_partial_sums, mlh_cs_fold
    (TG.test_fri_prove_matches_oracle, (9,)),
    (TG.test_sumcheck_prove_matches_oracle, (13, True)),
    (TG.test_sumcheck_prove_matches_oracle, (3, True)),
    (TG.test_pcs_prove_matches_oracle, (13,)),
    (TG.test_batched_fri_prove_matches_oracle, (3, 9)),
    (TG.test_batched_pcs_prove_matches_oracle, (2, 10)),
    (TCS.test_prove_matches_model, ("deg5_w7",)),
    (TCS.test_prove_matches_model, ("wide32",)),
    (TSY.test_prove_matches_model_and_verifies, ("quad3",)),
    (TSY.test_prove_matches_model_and_verifies, ("deg5_w7",)),
    (TSH.test_prove_matches_model_and_verifies, ("mixed5",)),
    (TG.test_fri_prover_step_api, ()),
    (TG.test_fri_prover_open_queries_many, (3,)),
    # beyond them
    (TG.test_ntt_matches_oracle, (11,)),
    (TG.test_ntt_vs_c_oracle, (19,)),
    (TG.test_intt_vs_c_oracle, (18,)),
    (TG.test_ntt_intt_any_generator_match_oracle, (1,)),   # its smallest size
    (TG.test_ntt_intt_any_generator_match_oracle, (12,)),  # in place: through the NTT scratch
    (TG.test_reed_solomon_brev_vs_c_oracle, (11,)),
    (TG.test_fri_fold_matches_oracle, (13, 0)),
    (TG.test_merkle_commit_generic_items, ()),  # 1-byte and 100-byte items: no multiple of 64
    (TG.test_merkle_batch_commit, ()),
    (TG.test_poly_evaluate_matches_horner, (4097,)),
    (TF.test_fill_matches_model_and_host_interpreter, ("wide16", 6, None)),
    (TP.test_prove_matches_model_and_verifies, ("deg5_w7",)),
    (TPUB.test_prove_matches_model_and_verifies, ("pmixed5",)),
]


def _case_id(case):
    fn, args = case
    return "%s.%s%s" % (fn.__module__, fn.__name__, list(args))


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_oracle_comparison_under_poison(case):
    fn, args = case
    with poison():
        fn(*args)


def test_pcs_cooperative_rounds_under_poison():
    with TSC._fused_max(0), poison():
        TG.test_pcs_prove_matches_oracle(13)


def test_lookup_counts_under_poison():
    W, values, T, Cc = TL.LAYOUTS[0]
    L = _first_multi_block(CS.lookup_counts_launch_info, len(values))
    with poison():
        TL.test_counts_match_the_model(L, W, values, T, Cc, "uniform")
        again()
        TL.test_counts_match_the_model(L, W, values, T, Cc, "hot")


def test_lookup_tuple_counts_under_poison():
    arity, n_tuples = 2, 3
    L = _first_multi_block(CS.lookup_tuple_counts_launch_info, n_tuples)
    with poison():
        TLT.test_counts_match_the_model(L, arity, n_tuples, "uniform")
        again()
        TLT.test_counts_match_the_model(L, arity, n_tuples, "hot")


def test_merkle_open_three_indices_under_poison():
    """mlh_merkle_open and mlh_merkle_open_pairs, three indices in one call."""
    lib, log_code = D.lib(), 9
    code = TG.rand_vals(1 << log_code, 909)
    ot = OF.commit_rs_code(code)
    leaves, depth = 1 << (log_code - 1), log_code - 1
    idx = [0, leaves - 1, 77]
    ia = (ctypes.c_uint64 * 3)(*idx)
    with poison():
        dcode = TG.dev(code)
        layers = TSC._layers(leaves)
        ctx = D.context()
        D.check(lib.mlh_merkle_commit_pairs(ctx, D.ptr(dcode), log_code, D.ptr(layers), None), ctx)
        again()
        out = (ctypes.c_uint8 * (3 * 32 * depth))()
        D.check(lib.mlh_merkle_open(ctx, D.ptr(layers), leaves, ia, 3, out), ctx)
        want = b"".join(bytes(s) for i in idx for s, _ in ot.open(i)[1])
        assert bytes(out) == want
        again()
        out2 = (ctypes.c_uint8 * (3 * 32 * (1 + depth)))()
        D.check(lib.mlh_merkle_open_pairs(ctx, D.ptr(dcode), log_code, D.ptr(layers), depth, ia, 3,
                                          out2), ctx)
        want2 = b"".join(OF.pair_bytes(code[i], code[i + leaves]) +
                         b"".join(bytes(s) for s, _ in ot.open(i)[1]) for i in idx)
        assert bytes(out2) == want2
    assert OM.verify(OF.pair_bytes(code[77], code[77 + leaves]), ot.open(77)[1], ot.root(), 77)


# ---- history: a smaller call inherits a larger call's pool blocks ---------------------

def _run(inputs, call):
    return call(*[D.to_device(a) for a in inputs])


def _history(larger, smaller, want):
    """smaller() with the poison off (a reference run of its own), then, under
    the poison, larger() and smaller(): the second equals the oracle and the
    run with the poison off."""
    clean = smaller()
    with poison():
        larger()
        again()
        dirty = smaller()
    assert dirty == want
    assert dirty == clean


def test_history_batched_fri_five_then_four_codes():
    big, _, _ = TSC._batched_fri_case(5, 9, 930)
    codes, want, digest = TSC._batched_fri_case(4, 9, 940)
    _history(lambda: _run([big], TSC._batched_fri_call(5)),
             lambda: _run([codes], TSC._batched_fri_call(4)), (want, digest))


def test_history_pcs_14_then_13():
    ev14, pts14, out14, _ = TSC._pcs_case(14, 950)
    ev13, pts13, out13, want = TSC._pcs_case(13, 220)
    _history(lambda: _run([ev14], TSC._pcs_call(pts14, out14)),
             lambda: _run([ev13], TSC._pcs_call(pts13, out13)), want)


def test_history_fri_rejected_code_then_a_codeword():
    code, want, digest = TSC._fri_case(9, 209)

    def rejected():
        with pytest.raises(_lib.MlhError) as e:  # random elements are no codeword
            _run([D.random_limbs(code.shape[0], 960)], TSC._fri_prove_call)
        assert e.value.status == _lib.MLH_ERR_NOT_RS_CODE

    _history(rejected, lambda: _run([code], TSC._fri_prove_call), (want, digest))


def test_history_cs_sumcheck_wide32_then_deg5_w7():
    big_inputs, big_call, _ = TSC._cs_prove_case("wide32")
    inputs, call, want = TSC._cs_prove_case("deg5_w7")
    _history(lambda: _run(big_inputs, big_call), lambda: _run(inputs, call), want)


def test_poison_off_is_the_default_and_zero_turns_it_off():
    """The hook's own contract: set and cleared through the API."""
    lib, ctx = D.lib(), D.context()
    assert lib.mlh_set_scratch_poison(ctx, WORD) == 0
    assert lib.mlh_set_scratch_poison(ctx, 0) == 0
    assert lib.mlh_set_scratch_poison(None, WORD) == _lib.MLH_ERR_INVALID
    TG.test_ntt_matches_oracle(11)
