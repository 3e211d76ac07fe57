#!/usr/bin/env python3
"""Times mlh_trace_scan (running sums and products down columns of a device
trace) on 2^20 x 4 and 2^22 x 8 by default: one product scan, one sum scan and
four product scans in one call, totals_out NULL (no wait inside the call).

HIP events on the context stream, the median of --iters after --warmup, all in
one process; the variants of one comparison alternate inside each iteration.
Beside each scan, from the same run:
  - mlh_trace_column_sum over the scan's source columns (one strided read pass,
    with its synchronising read-back);
  - mlh_memcpy_d2d of the matrix's bytes;
  - mlh_trace_fill of a program without INV that writes one product column
    (one read-and-write pass over the rows);
  - four one-scan calls beside the four-scan call;
  - the product scan under other launch shapes (mlh_trace_scan_shaped).
The values are checked in tests/test_trace_scan_gpu.py; here the shaped
launches are compared with the default launch before timing.
Prints one JSON line; nothing asserts on the numbers.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(256, 1), (256, 2), (256, 4), (256, 8), (256, 16), (128, 4), (64, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, nargs="+", default=["20x4", "22x8"],
                    help="log_height x width")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-shapes", action="store_true", help="the default launch only")
    args = ap.parse_args()

    import torch

    from multilinear_amd import constraint_system as CS
    from multilinear_amd import device as D

    lib, ctx = D.lib(), D.context()

    def timed_group(fns):
        """{name: fn} -> {name: median ms}; the fns alternate inside each iteration."""
        ts = {k: [] for k in fns}
        for i in range(args.warmup + args.iters):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    ts[k].append(a.elapsed_time(b))
        return {k: round(statistics.median(v), 4) for k, v in ts.items()}

    def u8(v):
        return (ctypes.c_uint8 * len(v))(*v)

    result = {"iters": args.iters, "warmup": args.warmup}
    for case in args.cases:
        L, W = (int(x) for x in case.split("x"))
        h = 1 << L
        matrix = D.random_device(W * h, seed=L)
        one = CS._elems([1] * 4)

        def scan(ops, cols, shape=None, m=None):
            n = len(cols)
            a = (ctx, D.ptr(matrix if m is None else m), L, W, n, u8(ops), u8(cols), u8(cols), one,
                 None)
            if shape is None:
                return lambda: D.check(lib.mlh_trace_scan(*a), ctx)
            return lambda: D.check(lib.mlh_trace_scan_shaped(*a, shape[0], shape[1], 1024), ctx)

        if not args.no_shapes:  # the same bytes under every shape
            want = matrix.clone()
            scan([1], [0], m=want)()
            for s in SHAPES:
                got = matrix.clone()
                scan([1], [0], s, m=got)()
                assert torch.equal(got, want), s
            del want, got

        cols4 = list(range(min(4, W)))
        fns = {"mul1_ms": scan([1], [0]), "add1_ms": scan([0], [0]),
               "mul4_ms": scan([1] * len(cols4), cols4)}

        def four_calls():
            for c in cols4:
                scan([1], [c])()

        fns["mul1_x4_calls_ms"] = four_calls
        prog = CS.FillProgram(CS.compile_fill({W - 1: CS.var(0) * CS.var(W - 1)}, W, 0))
        fns["fill_one_product_ms"] = lambda: D.check(
            lib.mlh_trace_fill(ctx, prog.h, D.ptr(matrix), L, W, None), ctx)
        dst = D.empty(W * h)
        fns["memcpy_d2d_same_bytes_ms"] = lambda: D.check(
            lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(matrix), 16 * W * h), ctx)
        fns["column_sum_1_ms"] = lambda: CS.trace_column_sum(matrix, W, (0,))
        fns["column_sum_4_ms"] = lambda: CS.trace_column_sum(matrix, W, cols4)
        r = timed_group(fns)
        if not args.no_shapes:
            sh = timed_group({"mul1_B%d_R%d_ms" % s: scan([1], [0], s) for s in SHAPES})
            r.update(sh)
            r["fastest_shape"] = list(min(SHAPES, key=lambda s: sh["mul1_B%d_R%d_ms" % s]))
        r["launch_rule"] = list(CS.trace_scan_launch_info(L, W, 1))
        for k in ("mul1", "add1"):
            r[k + "_over_column_sum_1"] = round(r[k + "_ms"] / r["column_sum_1_ms"], 2)
            r[k + "_over_copy"] = round(r[k + "_ms"] / r["memcpy_d2d_same_bytes_ms"], 2)
            r[k + "_over_fill"] = round(r[k + "_ms"] / r["fill_one_product_ms"], 2)
        r["mul4_over_column_sum_4"] = round(r["mul4_ms"] / r["column_sum_4_ms"], 2)
        r["mul4_over_copy"] = round(r["mul4_ms"] / r["memcpy_d2d_same_bytes_ms"], 2)
        r["mul4_over_fill"] = round(r["mul4_ms"] / r["fill_one_product_ms"], 2)
        r["four_calls_over_mul4"] = round(r["mul1_x4_calls_ms"] / r["mul4_ms"], 2)
        result["2^%d x %d" % (L, W)] = r
        del matrix, dst

    print(json.dumps(result))


if __name__ == "__main__":
    main()
