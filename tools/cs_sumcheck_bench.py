#!/usr/bin/env python3
"""Times mlh_cs_sumcheck_prove on the reference's sumcheck_high_bench shape
(sumcheck.rs:367-398): the 16-row Pythagorean trace doubled up to 2^20 rows x
4 columns, constraints x0^2 + x1^2 - x2^2 and x0 + x1 - x3 (degree 2), sum 0,
a clean transcript.

HIP events around the call (tables rebuilt outside the timed region), median
of --iters after --warmup; then one profiled prove for the per-kernel split
(mlh_profile_get) and the fraction of the HBM byte model reached:
  first pass   reads (W+1) * 16 * 2^L bytes
  fused pass   at height S reads (W+1) * 16 * S and writes half of it
  last fold    reads 2 rows, writes 1
Prints one JSON line.
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
    ap.add_argument("--peak-tbps", type=float, default=8.0, help="HBM peak the fraction is taken of")
    args = ap.parse_args()

    import torch

    from multilinear_amd import constraint_system as CS
    from multilinear_amd import device as D
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
    prover = CS.System.prover(Transcript(), cset, layout, CS.Trace(matrix, W))
    lib, ctx = D.lib(), D.context()

    def once(timed=True):
        tables = prover.build_tables()
        tr = Transcript()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pols, _ = prover.compute_sumcheck_polynomials(tr, tables, 0)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), pols, tr

    for _ in range(args.warmup):
        once()
    times = [once()[0] for _ in range(args.iters)]
    _, pols, tr = once()
    prover.verify_sumcheck_debug(Transcript(), pols, 0)  # the proof it timed verifies

    D.check(lib.mlh_profile_enable(ctx, 1), ctx)
    D.check(lib.mlh_profile_reset(ctx), ctx)
    once()
    split = {}
    for label in ("cs_sums", "cs_round", "cs_fold_sums", "cs_fold"):
        cnt, ms = ctypes.c_uint64(), ctypes.c_double()
        D.check(lib.mlh_profile_get(ctx, label.encode(), ctypes.byref(cnt), ctypes.byref(ms)), ctx)
        split[label] = {"launches": cnt.value, "ms": round(ms.value, 4)}
    D.check(lib.mlh_profile_enable(ctx, 0), ctx)

    row = (W + 1) * 16
    model = row * (1 << L) + sum(row * (1 << (L - k)) * 3 // 2 for k in range(L - 1)) + row * 3
    med = statistics.median(times)
    threads, blocks = prover.program.launch_info(L)
    print(json.dumps({
        "shape": "2^%d x %d, pythagorean, degree 2" % (L, W),
        "prove_ms_median": round(med, 4), "prove_ms_min": round(min(times), 4),
        "prove_ms_max": round(max(times), 4), "iters": args.iters, "warmup": args.warmup,
        "kernels_profiled_run": split, "first_pass_launch": {"threads": threads, "blocks": blocks},
        "hbm_model_bytes": model,
        "hbm_model_ms_at_peak": round(model / (args.peak_tbps * 1e9), 4),
        "fraction_of_hbm_model": round(model / (args.peak_tbps * 1e9) / med, 4),
    }))


if __name__ == "__main__":
    main()
