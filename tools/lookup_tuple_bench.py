#!/usr/bin/env python3
"""Times a tuple lookup's multiplicities on the XOR-lookup layout: 2^L x 9 rows
(a, b, c, ta, tb, tc, m, u, v), one value tuple, the table distinct random
tuples, L = 20 and 22 by default, arity 1, 2 and 3 (the first `arity`
components of each side) under three value distributions: uniform over the
table, 16 hot keys, one key.

HIP events on the context stream, the median of --iters after --warmup, all in
one process; the variants of one comparison alternate inside each iteration.
  1. mlh_trace_lookup_tuple_counts under its own rule;
  2. the composed path, what a caller had without it: mlh_trace_fill
     compresses the value tuple and the table tuple with a constant into the
     spare columns u and v (which phase 2 overwrites later), and
     mlh_trace_lookup_counts joins those two columns; fill and join are timed
     together (two calls, three launches, two borrowed columns, and right only
     as long as the compression does not collide);
  3. at arity 1, mlh_trace_lookup_counts on the same matrix;
  4. mlh_memcpy_d2d of the matrix's bytes: the floor of one pass over it.
The count column of every variant is compared with the tuple call's before
timing.  Prints one JSON line; nothing asserts on the numbers.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W = 9
VALUES, TABLE, COL_M, COL_U, COL_V = (0, 1, 2), (3, 4, 5), 6, 7, 8
COMPRESS = 0x9E3779B97F4A7C15F39CC0605CEDC834  # the composed path's constant


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

    result = {"shape": "XOR-lookup layout, 2^L x 9, one value tuple, distinct random table",
              "iters": args.iters, "warmup": args.warmup}
    for L in args.log_heights:
        h = 1 << L
        matrix = D.random_device(W * h, seed=L)
        mv = matrix.view(h, W, 4)
        trace = CS.Trace(matrix, W)
        gen = torch.Generator(device=matrix.device)
        gen.manual_seed(L)
        per_l = {"launch_rule": list(CS.lookup_tuple_counts_launch_info(L, 1))}
        for arity in (1, 2, 3):
            values, table = VALUES[:arity], TABLE[:arity]
            fill = CS.FillProgram(CS.compile_fill({COL_U: CS.tuple_key(values, COMPRESS),
                                                   COL_V: CS.tuple_key(table, COMPRESS)}, W, 0))

            def tuple_call():
                return trace.lookup_tuple_counts([values], table, COL_M)

            def composed():
                trace.fill(fill, [])
                return trace.lookup_counts([COL_U], COL_V, COL_M)

            def existing():
                return trace.lookup_counts([values[0]], table[0], COL_M)

            per_a = {}
            for dist, hot in (("uniform", h), ("hot16", 16), ("one_key", 1)):
                idx = torch.randint(0, hot, (h,), generator=gen, device=matrix.device)
                mv[:, :arity] = mv[idx, 3:3 + arity]
                mv[:, COL_M] = 7  # garbage: every call overwrites it
                assert tuple_call() == (0, None)
                want = mv[:, COL_M].clone()
                assert int(want[:, 0].sum()) == h and not bool(want[:, 1:].any())
                fns = {"tuple_ms": tuple_call, "composed_ms": composed}
                if arity == 1:
                    fns["existing_ms"] = existing
                for name, fn in fns.items():
                    mv[:, COL_M] = 7
                    assert fn() == (0, None), name
                    assert torch.equal(mv[:, COL_M], want), "%s disagrees with the tuple call" % name
                r = timed_group(fns)
                r["composed_over_tuple"] = round(r["composed_ms"] / r["tuple_ms"], 2)
                if arity == 1:
                    r["tuple_arity1_over_existing"] = round(r["tuple_ms"] / r["existing_ms"], 3)
                per_a[dist] = r
                print("2^%d arity %d %s: %s" % (L, arity, dist, json.dumps(r)), file=sys.stderr,
                      flush=True)
            per_l["arity_%d" % arity] = per_a
        dst = D.empty(W * h)
        per_l.update(timed_group({"memcpy_d2d_same_bytes_ms": lambda: D.check(
            lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(matrix), 16 * W * h), ctx)}))
        result["2^%d" % L] = per_l
        del matrix, mv, trace, dst, want

    print(json.dumps(result))


if __name__ == "__main__":
    main()
