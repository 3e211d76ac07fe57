#!/usr/bin/env python3
"""Times phase 2 of the two-phase proof on the lookup shape: 2^L x 5 rows
(a, t, m, u, v) with u = 1 / (gamma - a) and v = -m / (gamma - t), L = 20 and
22 by default.

HIP events on the context stream, the median of --iters after --warmup, all in
one process; the variants of one comparison alternate inside each iteration.
  1. mlh_trace_fill under its own launch rule (mlh_trace_fill_launch_info) and,
     through mlh_trace_fill_shaped, under B = 256 with K = 16 / 8 / 4, B = 128
     with K = 16 / 8 and B = 64 with K = 16;
  2. the composed path of tests/test_phased_proof_gpu.py: three strided column
     copies, mlh_field_sub / _inv / _scale / _sub / _inv / _mul and two strided
     copies back (gamma's broadcast vector is made outside the timed region);
  3. mlh_field_inv of 2 * 2^L contiguous elements: the multiplier-bound floor
     of two inverses per row;
  4. mlh_trace_column_sum over {u, v} (with its synchronising read-back) beside
     mlh_memcpy_d2d of the matrix's bytes.
The fill's matrix is compared with the composed path's before timing.  Prints
one JSON line; nothing asserts on the numbers.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(256, 16), (256, 8), (256, 4), (128, 16), (128, 8), (64, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-heights", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    from multilinear_amd import constraint_system as CS
    from multilinear_amd import device as D

    lib, ctx = D.lib(), D.context()
    M = D.M
    gamma = 0x0123456789ABCDEF0123456789ABCDEF % M
    prog = CS.FillProgram(CS.compile_fill(
        {3: CS.inv(CS.rand(0) - CS.var(0)), 4: -CS.var(2) * CS.inv(CS.rand(0) - CS.var(1))}, 5, 1))
    gb = D.fe_bytes(gamma)

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

    result = {"shape": "lookup, 2^L x 5, u = 1/(g - a), v = -m/(g - t)", "iters": args.iters,
              "warmup": args.warmup}
    for L in args.log_heights:
        h = 1 << L
        matrix = D.random_device(5 * h, seed=L)
        mv = matrix.view(h, 5, 4)
        g = D.to_device(D.ints_to_limbs([gamma])).expand(h, 4).contiguous()

        def composed():
            col = lambda j: mv[:, j].contiguous()
            u = CS.field_inv(CS.field_sub(g, col(0)))
            v = CS.field_mul(CS.field_scale(col(2), M - 1), CS.field_inv(CS.field_sub(g, col(1))))
            mv[:, 3] = u
            mv[:, 4] = v

        def fill(B, K):
            return lambda: D.check(lib.mlh_trace_fill_shaped(ctx, prog.h, D.ptr(matrix), L, 5, gb, B,
                                                             K), ctx)

        composed()
        want = matrix.clone()
        mv[:, 3:] = 0
        D.check(lib.mlh_trace_fill(ctx, prog.h, D.ptr(matrix), L, 5, gb), ctx)
        assert torch.equal(matrix, want), "the fill and the composed path disagree"

        fns = {"fill_ms": lambda: D.check(lib.mlh_trace_fill(ctx, prog.h, D.ptr(matrix), L, 5, gb),
                                          ctx)}
        fns.update({"fill_B%d_K%d_ms" % s: fill(*s) for s in SHAPES})
        fns["composed_ms"] = composed
        vec = D.random_device(2 * h, seed=L + 100)
        out = D.empty(2 * h)
        fns["field_inv_2x_ms"] = lambda: D.check(lib.mlh_field_inv(ctx, D.ptr(vec), D.ptr(out), 2 * h),
                                                 ctx)
        r = timed_group(fns)
        assert torch.equal(matrix, want)
        dst = D.empty(5 * h)
        r.update(timed_group({
            "column_sum_ms": lambda: CS.trace_column_sum(matrix, 5, (3, 4)),
            "memcpy_d2d_same_bytes_ms": lambda: D.check(
                lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(matrix), 80 * h), ctx)}))
        best = min(SHAPES, key=lambda s: r["fill_B%d_K%d_ms" % s])
        r["fastest_shape"] = list(best)
        r["launch_rule"] = list(prog.launch_info(L))
        r["composed_over_fill"] = round(r["composed_ms"] / r["fill_ms"], 2)
        r["fill_over_field_inv_2x"] = round(r["fill_ms"] / r["field_inv_2x_ms"], 2)
        r["column_sum_over_copy"] = round(r["column_sum_ms"] / r["memcpy_d2d_same_bytes_ms"], 2)
        r["column_sum_gbps"] = round(80 * h / r["column_sum_ms"] / 1e6, 1)
        result["2^%d" % L] = r
        del matrix, mv, g, want, vec, out, dst

    print(json.dumps(result))


if __name__ == "__main__":
    main()
