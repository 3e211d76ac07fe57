#!/usr/bin/env python3
"""Times the pieces of the shifted system proof (next-row constraints).

Median of --iters after --warmup, HIP events on the context stream, for
  mlh_trace_extend_next at 2^20 x 4 with K = 2 and at 2^18 x 16 with K = 16,
      each beside a mlh_memcpy_d2d of the output's byte count in the same
      process (ratio = copy time / extension time, 1 = as fast as the copy);
  mlh_system_prove_shifted of the Fibonacci system (a, b, last; next(a) = b,
      next(b) = a + b off the last row) at 2^--log-height rows, one commitment,
      beside mlh_system_prove_phased of the same trace and layout with a
      row-local program of the same degree and number of constraints, split
      into the extension, the main sumcheck, the shift sumcheck, the first and
      the second openings by mlh_profile_get of one further profiled prove.
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
    from multilinear_amd.transcript import Transcript

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

    # ---- the extension ----------------------------------------------------------
    def extension(log_h, width, cols):
        K = len(cols)
        src, dst = D.random_device(width << log_h, seed=log_h), D.empty((width + K) << log_h)
        spare = D.empty((width + K) << log_h)
        arr = (ctypes.c_uint32 * K)(*cols)
        t = timed(lambda _: D.check(lib.mlh_trace_extend_next(ctx, D.ptr(src), log_h, width, arr, K,
                                                              D.ptr(dst)), ctx))
        nbytes = 16 * ((width + K) << log_h)
        c = timed(lambda _: D.check(lib.mlh_memcpy_d2d(ctx, D.ptr(spare), D.ptr(dst), nbytes), ctx))
        rows, blocks = ctypes.c_uint32(), ctypes.c_uint32()
        D.check(lib.mlh_trace_extend_next_launch_info(log_h, width, K, ctypes.byref(rows),
                                                      ctypes.byref(blocks)))
        return {"extend_next_ms": t, "memcpy_d2d_output_bytes_ms": c, "copy_over_extend": round(c / t, 3),
                "output_gbps": round(nbytes / t / 1e6, 1), "tile_rows": rows.value,
                "blocks": blocks.value}

    ext = {"2^20 x 4, K = 2": extension(20, 4, [0, 1]),
           "2^18 x 16, K = 16": extension(18, 16, list(range(16)))}

    # ---- the composed proof -----------------------------------------------------
    L, W, M = args.log_height, 3, D.M
    H = 1 << L
    vals, a, b = [], 1, 1
    for i in range(H):
        vals += [a, b, 1 if i == H - 1 else 0]
        a, b = b, (a + b) % M
    matrix = D.to_device(D.ints_to_limbs(vals))
    del vals
    trace = CS.Trace(matrix, W)
    gate = 1 - CS.var(2)
    shifted = CS.ConstraintSet([gate * (CS.nxt(0) - CS.var(1)),
                                gate * (CS.nxt(1) - CS.var(0) - CS.var(1))], 2)
    local = CS.ConstraintSet([gate * (CS.var(0) - CS.var(1)),
                              gate * (CS.var(1) - CS.var(0) - CS.var(1))], 2)
    layout = CS.WitnessLayout(columns=W, randoms=0, pre_random_columns=W)
    wire, shifts = CS.compile_shifted(shifted.constraints(), W, 0, 2)
    sprog = CS.Program(wire)
    lprog = CS.Program(CS.compile_program(local.constraints(), W, 0, 2))
    com = CS.Commitment.new(trace, columns=(0, W))
    K = len(shifts)
    arr = (ctypes.c_uint32 * K)(*shifts)

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

    def shifted_setup():
        return CS.ShiftedSystemProof(L, W, 2, W, 0, shifts), Transcript()

    def shifted_prove(arg):
        p, tr = arg
        D.check(lib.mlh_system_prove_shifted(ctx, sprog.h, com.h, None, 0, arr, K, D.ptr(matrix),
                                             D.fe_bytes(0), D.fe_bytes(0), tr.h, ctypes.byref(p.c)), ctx)
        return p

    def phased_setup():
        return matrix.clone(), CS.PhasedSystemProof(L, W, 2, W, 0), Transcript()

    def phased_prove(arg):
        work, p, tr = arg
        D.check(lib.mlh_system_prove_phased(ctx, lprog.h, com.h, None, 0, D.ptr(work), D.fe_bytes(0),
                                            D.fe_bytes(0), tr.h, ctypes.byref(p.c)), ctx)

    shifted_ms = timed(shifted_prove, shifted_setup)
    phased_ms = timed(phased_prove, phased_setup)
    shifted_split = profile(lambda: shifted_prove(shifted_setup()),
                            ("trace_extend_next", "system_sumcheck", "system_shift_sumcheck",
                             "system_open", "system_open_shift"))
    phased_split = profile(lambda: phased_prove(phased_setup()), ("system_sumcheck", "system_open"))
    proof = shifted_prove(shifted_setup())
    proof._sync()
    assert proof.verify(Transcript(), shifted, layout, 0, 0), "the proof it timed does not verify"

    print(json.dumps({
        "iters": args.iters, "warmup": args.warmup, "extend_next": ext,
        "shape": "2^%d x %d Fibonacci, K = %d, degree 2, one commitment" % (L, W, K),
        "shifted_prove_ms": shifted_ms, "shifted_prove_split_profiled_run": shifted_split,
        "phased_prove_row_local_ms": phased_ms, "phased_prove_split_profiled_run": phased_split,
        "shifted_over_phased": round(shifted_ms / phased_ms, 3),
    }))


if __name__ == "__main__":
    main()
