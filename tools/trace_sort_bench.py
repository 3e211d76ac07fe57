#!/usr/bin/env python3
"""Times mlh_trace_sort (sorted copies of columns of a device trace) on 2^20 x 8
and 2^22 x 8 by default: one key column of values below 2^32, that column and
one more copied in key order.

Wall time around each call with the device idle before and after (the call
synchronises once itself, and the host path is host work), the median of
--iters after --warmup, all in one process; the variants alternate inside each
iteration:
  - sort_ms: mlh_trace_sort (the digit passes that the census leaves);
  - sort_all_passes_ms: the same with flags bit 0 (all 16 passes);
  - host_path_ms: what the call replaces: the key and source columns copied to
    the host, numpy.lexsort there, the sorted columns copied back;
  - memcpy_d2d_16B_per_row_ms: mlh_memcpy_d2d of 16 bytes per row, what one
    digit pass reads and writes in its scatter (8 B + 8 B per row);
  - the sort under other launch shapes (mlh_trace_sort_shaped).
The values are checked in tests/test_trace_sort_gpu.py; here the shaped launches
and the host path are compared with the default launch before timing.
Prints one JSON line; nothing asserts on the numbers.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(256, 4, 1024), (256, 8, 1024), (256, 16, 1024), (256, 8, 512), (256, 8, 256),
          (256, 16, 256), (128, 8, 1024), (128, 16, 1024)]
KEY, SRC, DST_KEY, DST_SRC = 0, 1, 2, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, nargs="+", default=["20x8", "22x8"],
                    help="log_height x width")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-shapes", action="store_true", help="the default launch only")
    args = ap.parse_args()

    import numpy as np
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
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        return {k: round(statistics.median(v), 4) for k, v in ts.items()}

    result = {"iters": args.iters, "warmup": args.warmup}
    for case in args.cases:
        L, W = (int(x) for x in case.split("x"))
        assert W >= 4
        h = 1 << L
        matrix = D.random_device(W * h, seed=L)
        matrix.view(h, W, 4)[:, KEY, 1:] = 0  # keys below 2^32
        copies = [(KEY, DST_KEY), (SRC, DST_SRC)]
        passes = {}

        def sort(shape=None, m=None, name=None):
            t = CS.Trace(matrix if m is None else m, W)

            def run():
                passes[name] = t.sort([KEY], copies, shape=shape)
            return run

        def host_path(m=None):
            v = (matrix if m is None else m).view(h, W, 4)
            key = v[:, KEY, :].cpu().numpy().view(np.uint32)
            src = v[:, SRC, :].cpu().numpy()
            order = np.lexsort((key[:, 0], key[:, 1], key[:, 2], key[:, 3]))  # stable, last key first
            v[:, DST_KEY, :] = torch.from_numpy(key.view(np.int32)[order]).to(v.device)
            v[:, DST_SRC, :] = torch.from_numpy(src[order]).to(v.device)

        want = matrix.clone()
        sort(m=want)()
        got = matrix.clone()
        host_path(got)
        assert torch.equal(got, want), "host path"
        if not args.no_shapes:  # the same bytes under every shape
            for s in SHAPES:
                got = matrix.clone()
                sort(s, m=got)()
                assert torch.equal(got, want), s
        del want, got

        dst = torch.empty((h, 4), dtype=torch.int32, device=matrix.device)
        src = torch.empty((h, 4), dtype=torch.int32, device=matrix.device)
        fns = {"sort_ms": sort(name="sort"),
               "sort_all_passes_ms": sort((256, 8, 1024, 1), name="all"),
               "host_path_ms": host_path,
               "memcpy_d2d_16B_per_row_ms": lambda: D.check(
                   lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(src), 16 * h), ctx)}
        r = timed_group(fns)
        r["passes"], r["passes_all"] = passes["sort"], passes["all"]
        r["per_pass_ms"] = round((r["sort_all_passes_ms"] - r["sort_ms"])
                                 / max(passes["all"] - passes["sort"], 1), 4)
        r["host_path_over_sort"] = round(r["host_path_ms"] / r["sort_ms"], 2)
        if not args.no_shapes:
            sh = timed_group({"sort_B%d_R%d_G%d_ms" % s: sort(s) for s in SHAPES})
            r.update(sh)
            r["fastest_shape"] = list(min(SHAPES, key=lambda s: sh["sort_B%d_R%d_G%d_ms" % s]))
        r["launch_rule"] = list(CS.trace_sort_launch_info(L, W, 1))
        result["2^%d x %d" % (L, W)] = r
        del matrix, dst, src

    print(json.dumps(result))


if __name__ == "__main__":
    main()
