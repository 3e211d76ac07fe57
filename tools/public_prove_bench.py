#!/usr/bin/env python3
"""Times the pieces of the system proof with public columns.

Median of --iters after --warmup, HIP events on the context stream, for
  mlh_trace_fill_public at 2^20 x 5 with F = 3 (first, last, a sparse column:
      48-byte runs) and at 2^18 x 32 with F = 16 (every kind), each beside a
      mlh_memcpy_d2d of the strip's byte count in the same process (ratio =
      copy time / fill time, 1 = as fast as the copy), and the kernels alone
      (without the upload of the spec) from the profile scope of one call;
  mlh_system_prove_public of Fibonacci with a statement (a, b committed; first,
      last, io public) at 2^--log-height rows against mlh_system_prove_shifted
      of the (a, b, last) Fibonacci system with its committed selector, same
      build, alternating, --runs runs each, each split into the extension, the
      main sumcheck, the shift sumcheck, the first and the second openings by
      mlh_profile_get of one further profiled prove.
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
    ap.add_argument("--runs", type=int, default=3)
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

    # ---- the fill ---------------------------------------------------------------
    def fill(log_h, width, spec):
        F = len(spec)
        m = D.random_device(width << log_h, seed=log_h)
        t = timed(lambda _: D.check(lib.mlh_trace_fill_public(ctx, spec.h, D.ptr(m), log_h, width), ctx))
        nbytes = 16 * (F << log_h)
        src, dst = D.empty(F << log_h), D.empty(F << log_h)
        c = timed(lambda _: D.check(lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(src), nbytes), ctx))
        rows, blocks = CS.public_fill_launch_info(log_h, width, F)
        # the kernels alone, without the upload of the spec's image: the profile scope of one call
        D.check(lib.mlh_profile_enable(ctx, 1), ctx)
        D.check(lib.mlh_profile_reset(ctx), ctx)
        D.check(lib.mlh_trace_fill_public(ctx, spec.h, D.ptr(m), log_h, width), ctx)
        cnt, ms = ctypes.c_uint64(), ctypes.c_double()
        D.check(lib.mlh_profile_get(ctx, b"trace_fill_public", ctypes.byref(cnt), ctypes.byref(ms)), ctx)
        D.check(lib.mlh_profile_enable(ctx, 0), ctx)
        return {"fill_public_ms": t, "memcpy_d2d_strip_bytes_ms": c, "copy_over_fill": round(c / t, 3),
                "strip_gbps": round(nbytes / t / 1e6, 1), "kernels_profiled_run_ms": round(ms.value, 4),
                "spec_wire_bytes": len(spec.wire), "run_bytes": 16 * F, "stride_bytes": 16 * width,
                "tile_rows": rows, "blocks": blocks}

    H18 = 1 << 18
    every = CS.PublicColumns()
    for k in range(2):
        every.const(7 + k).first().last().row_index().periodic(range(1, 5)).periodic(range(1 << 10))
        every.sparse({0: 1, H18 // 2: 2, H18 - 1: 3}).sparse({r: r + 1 for r in range(0, H18, 64)})
    fills = {"2^20 x 5, F = 3": fill(20, 5, CS.PublicColumns().first().last().sparse({0: 1, (1 << 20) - 1: 2})),
             "2^18 x 32, F = 16": fill(18, 32, every)}

    # ---- the composed proofs ----------------------------------------------------
    L, M = args.log_height, D.M
    H = 1 << L
    ab, a, b, result = [], 1, 1, 1
    for i in range(H):
        ab.append((a, b))
        result = b
        a, b = b, (a + b) % M
    spec = CS.PublicColumns().first().last().sparse({0: 1, H - 1: result})
    pub_matrix = D.to_device(D.ints_to_limbs([x for a, b in ab for x in (a, b, 0, 0, 0)]))
    old_matrix = D.to_device(D.ints_to_limbs([x for i, (a, b) in enumerate(ab)
                                              for x in (a, b, 1 if i == H - 1 else 0)]))
    del ab
    pub_trace, old_trace = CS.Trace(pub_matrix, 5), CS.Trace(old_matrix, 3)
    pub_trace.fill_public(spec)
    gate = 1 - CS.var(3)
    pub_set = CS.ConstraintSet([gate * (CS.nxt(0) - CS.var(1)), gate * (CS.nxt(1) - CS.var(0) - CS.var(1)),
                                CS.var(2) * (CS.var(0) - CS.var(4)), CS.var(3) * (CS.var(1) - CS.var(4))], 2)
    gate = 1 - CS.var(2)
    old_set = CS.ConstraintSet([gate * (CS.nxt(0) - CS.var(1)),
                                gate * (CS.nxt(1) - CS.var(0) - CS.var(1))], 2)
    pub_layout = CS.WitnessLayout(columns=5, pre_random_columns=2, public_columns=spec)
    old_layout = CS.WitnessLayout(columns=3, pre_random_columns=3)
    pub_wire, pub_shifts = CS.compile_shifted(pub_set.constraints(), 5, 0, 2)
    old_wire, old_shifts = CS.compile_shifted(old_set.constraints(), 3, 0, 2)
    pub_prog, old_prog = CS.Program(pub_wire), CS.Program(old_wire)
    pub_com = CS.Commitment.new(pub_trace, columns=(0, 2))
    old_com = CS.Commitment.new(old_trace, columns=(0, 3))
    pub_arr = (ctypes.c_uint32 * len(pub_shifts))(*pub_shifts)
    old_arr = (ctypes.c_uint32 * len(old_shifts))(*old_shifts)
    labels = ("trace_extend_next", "system_sumcheck", "system_shift_sumcheck", "system_open",
              "system_open_shift")

    def profile(fn):
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

    def pub_setup():
        return CS.ShiftedSystemProof(L, 5, 2, 2, 0, pub_shifts, 3), Transcript()

    def pub_prove(arg):
        p, tr = arg
        D.check(lib.mlh_system_prove_public(ctx, pub_prog.h, pub_com.h, None, 0, pub_arr, len(pub_shifts),
                                            spec.h, D.ptr(pub_matrix), D.fe_bytes(0), D.fe_bytes(0),
                                            tr.h, ctypes.byref(p.c)), ctx)
        return p

    def old_setup():
        return CS.ShiftedSystemProof(L, 3, 2, 3, 0, old_shifts), Transcript()

    def old_prove(arg):
        p, tr = arg
        D.check(lib.mlh_system_prove_shifted(ctx, old_prog.h, old_com.h, None, 0, old_arr,
                                             len(old_shifts), D.ptr(old_matrix), D.fe_bytes(0),
                                             D.fe_bytes(0), tr.h, ctypes.byref(p.c)), ctx)
        return p

    pub_ms, old_ms = [], []
    for _ in range(args.runs):  # alternating
        old_ms.append(timed(old_prove, old_setup))
        pub_ms.append(timed(pub_prove, pub_setup))
    pub_split = profile(lambda: pub_prove(pub_setup()))
    old_split = profile(lambda: old_prove(old_setup()))
    proof = pub_prove(pub_setup())
    proof._sync()
    assert proof.verify(Transcript(), pub_set, pub_layout, 0, 0), "the proof it timed does not verify"
    proof = old_prove(old_setup())
    proof._sync()
    assert proof.verify(Transcript(), old_set, old_layout, 0, 0), "the shifted proof does not verify"

    pm, om = statistics.median(pub_ms), statistics.median(old_ms)
    print(json.dumps({
        "iters": args.iters, "warmup": args.warmup, "runs": args.runs, "fill_public": fills,
        "public_shape": "2^%d x 5 Fibonacci with a statement: 2 committed, 3 public, K = 2, degree 2" % L,
        "shifted_shape": "2^%d x 3 Fibonacci, committed selector, K = 2, degree 2" % L,
        "public_prove_ms": pub_ms, "shifted_prove_ms": old_ms,
        "public_minus_shifted_ms": round(pm - om, 4),
        "public_max_minus_min_ms": round(max(pub_ms) - min(pub_ms), 4),
        "shifted_max_minus_min_ms": round(max(old_ms) - min(old_ms), 4),
        "public_prove_split_profiled_run": pub_split, "shifted_prove_split_profiled_run": old_split,
    }))


if __name__ == "__main__":
    main()
