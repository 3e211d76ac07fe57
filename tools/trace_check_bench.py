#!/usr/bin/env python3
"""Times mlh_trace_check (the constraints once per row of a device trace, the
next row read by address) at 2^20 and 2^22 rows by default, for the fib, mixed
and wide systems of tests/shifted_reference.py, on a random trace (every row
fails) and on an all-zero one (every constraint holds, nothing is flushed).

HIP events on the context stream, the median of --iters after --warmup, all in
one process; the calls of one comparison alternate inside each iteration.
Beside each check, from the same run, on the same program and height:
  - mlh_cs_partial_sums on the extended trace: the first sumcheck pass, which
    interprets D = degree + 1 points per row pair where the check interprets
    one point per row (both calls synchronise once for their result);
  - mlh_trace_extend_next, the W + K wide copy the check does without;
  - mlh_memcpy_d2d of the trace's bytes;
  - the check under other block sizes (mlh_trace_check_shaped).
With public columns: mlh_trace_check_public beside mlh_trace_fill_public on a
16-column strip.  The values are checked in tests/test_trace_check_gpu.py; here
the shaped launches are compared with the default launch before timing.
Prints one JSON line; nothing asserts on the numbers.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SYSTEMS = {"fib": "fib4", "mixed": "mixed5", "wide": "wide9"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-heights", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--systems", type=str, nargs="+", default=list(SYSTEMS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-shapes", action="store_true", help="the default launch only")
    args = ap.parse_args()

    import torch

    import shifted_reference as SR
    from multilinear_amd import _lib
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

    result = {"iters": args.iters, "warmup": args.warmup}
    for name in args.systems:
        wire, shifts = SR.program(SYSTEMS[name])
        _, _, degree, W, n_rand = SR._system(SYSTEMS[name])[:5]
        prog = CS.Program(wire)
        K, NC = len(shifts), prog.n_constraints
        rnd = CS._elems([12345 + i for i in range(n_rand)])
        mask = CS._elems([7 + c for c in range(NC)])
        cols = (ctypes.c_uint32 * max(K, 1))(*shifts)
        for L in args.log_heights:
            h = 1 << L
            matrix = D.random_device(W * h, seed=L)
            zeros = torch.zeros_like(matrix)
            ext = D.empty((W + K) * h)
            delta = D.random_device(h, seed=L + 100)
            dst = D.empty(W * h)
            counts, firsts = (ctypes.c_uint64 * NC)(), (ctypes.c_uint64 * NC)()
            rep = _lib.TraceCheckReportC()
            sums = (ctypes.c_uint8 * (16 * (degree + 1)))()

            def check(m, shape=None):
                a = (ctx, prog.h, D.ptr(m), L, W, cols, K, rnd, counts, firsts, ctypes.byref(rep))
                if shape is None:
                    return lambda: D.check(lib.mlh_trace_check(*a), ctx)
                return lambda: D.check(lib.mlh_trace_check_shaped(*a, *shape), ctx)

            def extend():
                D.check(lib.mlh_trace_extend_next(ctx, D.ptr(matrix), L, W, cols, K, D.ptr(ext)), ctx)

            extend()
            threads, blocks = CS.trace_check_launch_info(prog, L)
            shapes = [(t, 1024) for t in (64, 128, 256)]
            check(matrix)()
            want = (bytes(counts), bytes(firsts), bytes(rep))
            for s in ([] if args.no_shapes else shapes):
                check(matrix, s)()
                assert (bytes(counts), bytes(firsts), bytes(rep)) == want, s
            r = {"failing_rows_random": rep.n_bad_rows}
            check(zeros)()
            r["failing_rows_zero"] = rep.n_bad_rows
            fns = {"check_random_ms": check(matrix), "check_zero_ms": check(zeros),
                   "cs_partial_sums_ms": lambda: D.check(lib.mlh_cs_partial_sums(
                       ctx, prog.h, W + K, D.ptr(ext), D.ptr(delta), L, rnd, mask, sums), ctx),
                   "extend_next_ms": extend,
                   "memcpy_d2d_same_bytes_ms": lambda: D.check(
                       lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(matrix), 16 * W * h), ctx)}
            r.update(timed_group(fns))
            if not args.no_shapes:
                r.update(timed_group({"check_B%d_ms" % s[0]: check(matrix, s) for s in shapes}))
            r["launch_rule"] = [threads, blocks]
            r["first_pass_launch"] = list(prog.launch_info(L))
            r["points_per_row_pair_first_pass"] = degree + 1
            r["check_over_first_pass"] = round(r["check_random_ms"] / r["cs_partial_sums_ms"], 3)
            r["check_over_extend_next"] = round(r["check_random_ms"] / r["extend_next_ms"], 3)
            r["check_over_copy"] = round(r["check_random_ms"] / r["memcpy_d2d_same_bytes_ms"], 3)
            result["%s W=%d K=%d 2^%d" % (name, W, K, L)] = r
            del matrix, zeros, ext, delta, dst

    # the public strip: 16 columns of 18
    import public_reference as PUB

    for L in args.log_heights:
        W, h = 18, 1 << L
        descs = PUB.pwide_descs(12)  # (periods up to 2^12, sparse rows below 2^12)
        spec = PUB.builder(descs)
        t = CS.Trace(D.random_device(W * h, seed=L + 7), W)
        t.fill_public(spec)
        res = t.check_public(spec)
        assert res.ok
        r = timed_group({"check_public_ms": lambda: t.check_public(spec),
                         "fill_public_ms": lambda: t.fill_public(spec)})
        r["check_public_over_fill_public"] = round(r["check_public_ms"] / r["fill_public_ms"], 3)
        result["public F=16 W=18 2^%d" % L] = r
        del t

    print(json.dumps(result))


if __name__ == "__main__":
    main()
