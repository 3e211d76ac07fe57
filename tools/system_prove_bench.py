#!/usr/bin/env python3
"""Times the system proof on the reference's sumcheck_high_bench shape
(sumcheck.rs:367-398): the 16-row Pythagorean trace doubled up to 2^20 rows x
4 columns, degree 2, sum 0, a clean transcript.

Median of --iters after --warmup, HIP events on the context stream, for
  mlh_trace_columns (also at 2^18 x 32), beside a mlh_memcpy_d2d of the same
      byte count in the same process (the yardstick: it moves the same bytes);
  mlh_trace_commit;
  mlh_system_prove, split into sumcheck and opening by mlh_profile_get of one
      further profiled prove;
  the same run's mlh_cs_sumcheck_prove + mlh_batched_pcs_prove called
      separately on the same data (the composed call saves the codes and the
      batch tree, and pays one synchronisation for the output);
and the wall time of mlh_system_verify on the host.  Prints one JSON line;
nothing asserts on the numbers.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

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
    from multilinear_amd.batched import BatchedPCSProof
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
    cset = CS.ConstraintSet([CS.var(0) * CS.var(0) + CS.var(1) * CS.var(1) - CS.var(2) * CS.var(2),
                             CS.var(0) + CS.var(1) - CS.var(3)], 2)
    layout = CS.WitnessLayout(columns=W, randoms=0)
    trace = CS.Trace(matrix, W)
    lib, ctx = D.lib(), D.context()

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

    def transpose_vs_copy(log_h, width):
        n = width << log_h
        src, dst = D.random_device(n, seed=log_h), D.empty(n)
        t = timed(lambda _: D.check(lib.mlh_trace_columns(ctx, D.ptr(src), log_h, width, D.ptr(dst)), ctx))
        c = timed(lambda _: D.check(lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(src), 16 * n), ctx))
        return {"trace_columns_ms": t, "memcpy_d2d_ms": c, "copy_over_transpose": round(c / t, 3),
                "transpose_gbps": round(32 * n / t / 1e6, 1)}

    shapes = {"2^%d x %d" % (L, W): transpose_vs_copy(L, W), "2^18 x 32": transpose_vs_copy(18, 32)}

    commits = []

    def commit(_):
        commits[:] = [CS.Commitment.new(trace)]  # (the one before it is destroyed here)

    commit_ms = timed(commit)
    del commits[:]

    prover = CS.System.committed_prover(Transcript(), cset, layout, trace)

    def prove_setup():  # the matrix clone and the proof buffers stay outside the timed region
        return matrix.clone(), CS.SystemProof(L, W, 2), Transcript()

    def prove(arg):
        work, p, tr = arg
        D.check(lib.mlh_system_prove(ctx, prover.program.h, prover.commitment().h, D.ptr(work),
                                     D.fe_bytes(0), tr.h, ctypes.byref(p.c)), ctx)

    prove_ms = timed(prove, prove_setup)
    proof = prover.prove(Transcript(), 0)
    t0 = time.perf_counter()
    ok = proof.verify(Transcript(), cset, layout, 0)
    verify_ms = round(1e3 * (time.perf_counter() - t0), 3)
    assert ok, "the proof it timed does not verify"

    D.check(lib.mlh_profile_enable(ctx, 1), ctx)
    D.check(lib.mlh_profile_reset(ctx), ctx)
    prover.prove(Transcript(), 0)
    split = {}
    for label in ("system_sumcheck", "system_open"):
        cnt, ms = ctypes.c_uint64(), ctypes.c_double()
        D.check(lib.mlh_profile_get(ctx, label.encode(), ctypes.byref(cnt), ctypes.byref(ms)), ctx)
        split[label + "_ms"] = round(ms.value, 4)
    D.check(lib.mlh_profile_enable(ctx, 0), ctx)

    # the two calls on their own: same trace, challenges, point and claim
    cols = CS.trace_columns(matrix, W)
    root = prover.commitment().root()

    def sep_setup():
        tr = Transcript()
        tr.absorb(root)
        return tr, CS.SumcheckTables(matrix.clone(), W, 1 << L, eq_table(prover.challenges().row()))

    sc_out = {}

    def sumcheck(arg):
        tr, tables = arg
        sc_out["rs"] = prover.compute_sumcheck_polynomials(tr, tables, 0)[1]
        sc_out["tr"] = tr

    sumcheck_ms = timed(sumcheck, sep_setup)
    pcs_ms = timed(lambda _: BatchedPCSProof.prove(sc_out["rs"], proof.output, cols, sc_out["tr"].clone()))

    print(json.dumps({
        "shape": "2^%d x %d, pythagorean, degree 2" % (L, W), "iters": args.iters,
        "warmup": args.warmup, "transpose": shapes, "commit_ms": commit_ms, "prove_ms": prove_ms,
        "prove_split_profiled_run": split, "verify_host_ms": verify_ms,
        "separate_cs_sumcheck_prove_ms": sumcheck_ms, "separate_batched_pcs_prove_ms": pcs_ms,
        "separate_sum_ms": round(sumcheck_ms + pcs_ms, 4),
    }))


if __name__ == "__main__":
    main()
