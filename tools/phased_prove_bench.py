#!/usr/bin/env python3
"""Times the pieces of the two-phase system proof on the reference's
sumcheck_high_bench shape (sumcheck.rs:367-398): the 16-row Pythagorean trace
doubled up to 2^20 rows x 4 columns, degree 2, sum 0, a clean transcript.

Median of --iters after --warmup, HIP events on the context stream, for
  mlh_cs_sumcheck_prove_sums with sum column {3} beside mask 0 (the cost of the
      sum term);
  mlh_trace_columns_range over [0, 2) + [2, 4) of 2^20 x 4, over [0, 16) +
      [16, 32) and over [31, 32) alone of 2^18 x 32, each beside the one full
      mlh_trace_columns call and a mlh_memcpy_d2d of the bytes it moves;
  mlh_field_inv at 2^20 and 2^24 elements beside mlh_field_mul at the same n;
  mlh_system_prove_phased with P = 2, S = {3} beside mlh_system_prove of the
      same trace, each split into sumcheck and openings by mlh_profile_get of
      one further profiled prove.
Prints one JSON line; nothing asserts on the numbers.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-height", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    from multilinear_amd import constraint_system as CS
    from multilinear_amd import device as D
    from multilinear_amd.polynomials import eq_table
    from multilinear_amd.transcript import Transcript

    L, W = args.log_height, 4
    rows, m = [], 2
    while len(rows) < 16:  # Euclid's formula, as the tests
        for n in range(1, m):
            if len(rows) < 16:
                a, b, c = m * m - n * n, 2 * m * n, m * m + n * n
                rows.append([a, b, c, a + b])
        m += 1
    base = D.to_device(D.ints_to_limbs([v for r in rows for v in r]))
    matrix = base.repeat(1 << (L - 4), 1).contiguous()
    exprs = [CS.var(0) * CS.var(0) + CS.var(1) * CS.var(1) - CS.var(2) * CS.var(2),
             CS.var(0) + CS.var(1) - CS.var(3)]
    cset = CS.ConstraintSet(exprs, 2)
    trace = CS.Trace(matrix, W)
    lib, ctx = D.lib(), D.context()
    column_sum = sum(r[3] for r in rows) * (1 << (L - 4)) % D.M

    def timed(fn, setup=None):
        ts = []
        for i in range(args.warmup + args.iters):
            arg = setup() if setup else None
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(arg)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ts.append(a.elapsed_time(b))
        return round(statistics.median(ts), 4)

    # ---- the sum term ---------------------------------------------------------
    prover = CS.System.prover(Transcript(), cset, CS.WitnessLayout(columns=W), trace)
    row = prover.challenges().row()
    cmask = CS._elems(prover.constraint_mask())
    polys = (ctypes.c_uint8 * (16 * 3 * L))()
    rs = (ctypes.c_uint8 * (16 * L))()
    beta = 0x1234567890ABCDEF

    def sums_setup():
        return matrix.clone(), eq_table(row), Transcript()

    def sums(mask):
        claim = D.fe_bytes(beta * column_sum % D.M if mask else 0)

        def run(arg):
            work, delta, tr = arg
            D.check(lib.mlh_cs_sumcheck_prove_sums(ctx, prover.program.h, W, D.ptr(work), D.ptr(delta),
                                                   L, None, cmask, mask, D.fe_bytes(beta), claim, tr.h,
                                                   polys, rs), ctx)
        return run

    sum_term = {"mask_0_ms": timed(sums(0), sums_setup), "mask_col3_ms": timed(sums(8), sums_setup)}

    # ---- the range transpose --------------------------------------------------
    def transposes(log_h, width, ranges):
        n = width << log_h
        src, dst = D.random_device(n, seed=log_h), D.empty(n)
        out = {}

        def run_ranges(_):
            off = 0
            for col0, ncols in ranges:
                D.check(lib.mlh_trace_columns_range(
                    ctx, D.ptr(src), log_h, width, col0, ncols,
                    ctypes.c_void_p(dst.data_ptr() + 16 * (off << log_h))), ctx)
                off += ncols

        moved = sum(nc for _, nc in ranges) << log_h
        out["ranges"] = ["[%d, %d)" % (c, c + nc) for c, nc in ranges]
        out["range_ms"] = timed(run_ranges)
        out["full_trace_columns_ms"] = timed(
            lambda _: D.check(lib.mlh_trace_columns(ctx, D.ptr(src), log_h, width, D.ptr(dst)), ctx))
        out["memcpy_d2d_same_bytes_ms"] = timed(
            lambda _: D.check(lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(src), 16 * moved), ctx))
        out["range_over_full"] = round(out["range_ms"] / out["full_trace_columns_ms"], 3)
        out["range_over_copy"] = round(out["range_ms"] / out["memcpy_d2d_same_bytes_ms"], 3)
        out["range_gbps"] = round(32 * moved / out["range_ms"] / 1e6, 1)
        return out

    transpose = {"2^%d x 4 halves" % L: transposes(L, 4, [(0, 2), (2, 2)]),
                 "2^18 x 32 halves": transposes(18, 32, [(0, 16), (16, 16)]),
                 "2^18 x 32 last column": transposes(18, 32, [(31, 1)])}

    # ---- mlh_field_inv --------------------------------------------------------
    inv = {}
    for log_n in (20, 24):
        n = 1 << log_n
        a, b, out = D.random_device(n, seed=log_n), D.random_device(n, seed=log_n + 1), D.empty(n)
        t_inv = timed(lambda _: D.check(lib.mlh_field_inv(ctx, D.ptr(a), D.ptr(out), n), ctx))
        t_mul = timed(lambda _: D.check(lib.mlh_field_mul(ctx, D.ptr(a), D.ptr(b), D.ptr(out), n), ctx))
        inv["2^%d" % log_n] = {"field_inv_ms": t_inv, "field_mul_ms": t_mul,
                               "inv_over_mul": round(t_inv / t_mul, 2)}
        del a, b, out

    # ---- the composed proof ---------------------------------------------------
    def profile(fn, labels):
        D.check(lib.mlh_profile_enable(ctx, 1), ctx)
        D.check(lib.mlh_profile_reset(ctx), ctx)
        fn()
        split = {}
        for label in labels:
            cnt, ms = ctypes.c_uint64(), ctypes.c_double()
            D.check(lib.mlh_profile_get(ctx, label.encode(), ctypes.byref(cnt), ctypes.byref(ms)), ctx)
            split[label + "_ms"] = round(ms.value, 4)
        D.check(lib.mlh_profile_enable(ctx, 0), ctx)
        return split

    layout1 = CS.WitnessLayout(columns=W, randoms=0)
    one = CS.System.committed_prover(Transcript(), cset, layout1, trace)

    def one_setup():
        return matrix.clone(), CS.SystemProof(L, W, 2), Transcript()

    def one_prove(arg):
        work, p, tr = arg
        D.check(lib.mlh_system_prove(ctx, one.program.h, one.commitment().h, D.ptr(work), D.fe_bytes(0),
                                     tr.h, ctypes.byref(p.c)), ctx)

    system_ms = timed(one_prove, one_setup)
    system_split = profile(lambda: one.prove(Transcript(), 0), ("system_sumcheck", "system_open"))

    P, mask = 2, 8
    layout2 = CS.WitnessLayout(columns=W, randoms=0, pre_random_columns=P, sum_columns=(3,))
    com1 = CS.Commitment.new(trace, columns=(0, P))
    com2 = CS.Commitment.new(trace, columns=(P, W - P))

    def two_setup():
        return matrix.clone(), CS.PhasedSystemProof(L, W, 2, P, mask), Transcript()

    def two_prove(arg):
        work, p, tr = arg
        D.check(lib.mlh_system_prove_phased(ctx, one.program.h, com1.h, com2.h, mask, D.ptr(work),
                                            D.fe_bytes(0), D.fe_bytes(column_sum), tr.h,
                                            ctypes.byref(p.c)), ctx)
        return p

    phased_ms = timed(two_prove, two_setup)
    phased_split = profile(lambda: two_prove(two_setup()),
                           ("system_sumcheck", "system_open", "system_open2"))
    proof = two_prove(two_setup())
    proof._sync()
    assert proof.verify(Transcript(), cset, layout2, 0, column_sum), "the proof it timed does not verify"
    commits = []

    def commit2(_):
        commits[:] = [CS.Commitment.new(trace, columns=(P, W - P))]

    commit2_ms = timed(commit2)
    del commits[:]

    print(json.dumps({
        "shape": "2^%d x %d, pythagorean, degree 2" % (L, W), "iters": args.iters,
        "warmup": args.warmup, "sum_term": sum_term, "transpose": transpose, "field_inv": inv,
        "system_prove_ms": system_ms, "system_prove_split_profiled_run": system_split,
        "phased_prove_P2_S3_ms": phased_ms, "phased_prove_split_profiled_run": phased_split,
        "commit_columns_2_4_ms": commit2_ms,
    }))


if __name__ == "__main__":
    main()
