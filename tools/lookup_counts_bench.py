#!/usr/bin/env python3
"""Times a lookup's multiplicities on the lookup shape: 2^L x 5 rows (a, t, m,
u, v), one value column a, the table t of distinct random elements, L = 20 and
22 by default, under three value distributions: uniform over the table, 16 hot
keys, one key.

HIP events on the context stream, the median of --iters after --warmup, all in
one process; the variants of one comparison alternate inside each iteration.
  1. mlh_trace_lookup_counts under its own rule (mlh_trace_lookup_counts_
     launch_info) and, through mlh_trace_lookup_counts_shaped, with log_slots =
     L + 1, L + 2 and L + 3, with the wave-level aggregation off, and under
     grid caps of 256 to 4096 blocks;
  2. what a caller without it does: the two columns copied to the host, counted
     there (a numpy sort-unique and a Python dict are each run, the faster one
     is reported; --host-iters runs, they take seconds, 0 leaves them out),
     the count column copied back;
  3. torch.unique(dim=0, return_inverse=True) + bincount on the device, when
     this torch build runs it;
  4. mlh_memcpy_d2d of the matrix's bytes: the floor of one pass over it.
The counted column is compared with the host's before timing.  Prints one JSON
line; nothing asserts on the numbers.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CAPS = [256, 512, 1024, 2048, 4096]
COL_A, COL_T, COL_M = 0, 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-heights", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3)
    args = ap.parse_args()

    import ctypes

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
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    ts[k].append(a.elapsed_time(b))
        return {k: round(statistics.median(v), 4) for k, v in ts.items()}

    def host_count(t, a, how):
        """Counts per table row on the host (the table's entries are distinct)."""
        h = len(t)
        if how == "dict":
            owner = {}
            for j, k in enumerate(t.view("V16").ravel().tolist()):
                owner.setdefault(k, j)
            idx = np.fromiter((owner.get(v, -1) for v in a.view("V16").ravel().tolist()),
                              dtype=np.int64, count=h)
            return np.bincount(idx[idx >= 0], minlength=h)
        u, inv = np.unique(np.concatenate([t, a]).view("V16").ravel(), return_inverse=True)
        inv = inv.ravel()
        return np.bincount(inv[h:], minlength=len(u))[inv[:h]]

    result = {"shape": "lookup, 2^L x 5, one value column, distinct random table",
              "iters": args.iters, "warmup": args.warmup, "host_iters": args.host_iters}
    n, first = ctypes.c_uint64(), ctypes.c_uint64()
    for L in args.log_heights:
        h = 1 << L
        matrix = D.random_device(5 * h, seed=L)
        mv = matrix.view(h, 5, 4)
        table = mv[:, COL_T].contiguous()
        gen = torch.Generator(device=matrix.device)
        gen.manual_seed(L)
        per_l = {"launch_rule": list(CS.lookup_counts_launch_info(L, 1))}
        slots = per_l["launch_rule"][2]

        def shaped(log_slots, max_blocks=0, flags=0):
            def run():
                D.check(lib.mlh_trace_lookup_counts_shaped(
                    ctx, D.ptr(matrix), L, 5, 1 << COL_A, COL_T, COL_M, ctypes.byref(n),
                    ctypes.byref(first), log_slots, log_slots, max_blocks, flags), ctx)
            return run

        def default():
            D.check(lib.mlh_trace_lookup_counts(ctx, D.ptr(matrix), L, 5, 1 << COL_A, COL_T, COL_M,
                                                ctypes.byref(n), ctypes.byref(first)), ctx)

        def host_path(how):
            def run():
                t = mv[:, COL_T].contiguous().cpu().numpy()
                a = mv[:, COL_A].contiguous().cpu().numpy()
                c = host_count(t, a, how)
                limbs = np.zeros((h, 4), dtype=np.int32)
                limbs[:, 0] = c.astype(np.uint32).view(np.int32)
                mv[:, COL_M] = torch.from_numpy(limbs).to(matrix.device)
                torch.cuda.synchronize()
            return run

        def torch_path():
            both = torch.cat([mv[:, COL_T], mv[:, COL_A]])
            u, inv = torch.unique(both, dim=0, return_inverse=True)
            c = torch.bincount(inv[h:], minlength=u.shape[0])[inv[:h]]
            mv[:, COL_M] = 0
            mv[:, COL_M, 0] = c.to(torch.int32)

        for dist, hot in (("uniform", h), ("hot16", 16), ("one_key", 1)):
            idx = torch.randint(0, hot, (h,), generator=gen, device=matrix.device)
            mv[:, COL_A] = table[idx]
            mv[:, COL_M] = 7  # garbage: the call overwrites it
            host_path("numpy")()
            want = matrix.clone()
            mv[:, COL_M] = 7
            default()
            assert (n.value, first.value) == (0, 2 ** 64 - 1)
            assert torch.equal(matrix, want), "the device's and the host's counts disagree"

            fns = {"default_ms": default, "no_aggregation_ms": shaped(slots, flags=1)}
            fns.update({"slots_L+%d_ms" % d: shaped(L + d) for d in (1, 2, 3)})
            fns.update({"cap_%d_ms" % c: shaped(slots, max_blocks=c) for c in CAPS})
            r = timed_group(fns)
            assert torch.equal(matrix, want)
            try:
                torch_path()
                assert torch.equal(matrix, want), "torch.unique + bincount disagrees"
                r.update(timed_group({"torch_unique_bincount_ms": torch_path}))
            except RuntimeError as e:  # this torch build does not run it
                r["torch_unique_bincount_ms"] = None
                r["torch_unique_bincount_error"] = str(e).splitlines()[0][:120]
            for how in ("numpy", "dict") if args.host_iters else ():
                ts = []
                for _ in range(args.host_iters):
                    t0 = time.perf_counter()
                    host_path(how)()
                    ts.append(1e3 * (time.perf_counter() - t0))
                r["host_%s_ms" % how] = round(statistics.median(ts), 1)
                assert torch.equal(matrix, want)
            if args.host_iters:  # (0: the device variants only)
                r["host_baseline_ms"] = min(r["host_numpy_ms"], r["host_dict_ms"])
                r["host_over_default"] = round(r["host_baseline_ms"] / r["default_ms"], 1)
            per_l[dist] = r
            print("2^%d %s: %s" % (L, dist, json.dumps(r)), file=sys.stderr, flush=True)
        dst = D.empty(5 * h)
        copy = timed_group({"memcpy_d2d_same_bytes_ms": lambda: D.check(
            lib.mlh_memcpy_d2d(ctx, D.ptr(dst), D.ptr(matrix), 80 * h), ctx)})
        per_l.update(copy)
        for dist in ("uniform", "hot16", "one_key"):
            per_l[dist]["default_over_copy"] = round(
                per_l[dist]["default_ms"] / copy["memcpy_d2d_same_bytes_ms"], 2)
        per_l["one_key_over_uniform"] = round(
            per_l["one_key"]["default_ms"] / per_l["uniform"]["default_ms"], 2)
        result["2^%d" % L] = per_l
        del matrix, mv, table, want, dst

    print(json.dumps(result))


if __name__ == "__main__":
    main()
