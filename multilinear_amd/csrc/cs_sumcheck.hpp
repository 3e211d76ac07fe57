// Constraint-system sumcheck launch interface (internal to libmlhip):
// SumcheckTables::{partial_sum, fold, compute_sumcheck_polynomial} for
// width > 1 and a programmable composition (constraint_system/sumcheck.rs:
// 147-247), kernels in cs_sumcheck.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"
#include "transcript_dev.hpp"

namespace mlh {

// A program's device image (cs_program.hpp cs_build_image), by value.
struct CsDev {
  const fe* uni;         // uniform pool: randoms | consts | mask
  const uint32_t* code;  // 2 words per instruction
  const uint32_t* outs;  // 1 word per constraint
  uint32_t width, n_temps, n_instr, n_constraints, D;
};

// partials[t * nb + block], t < D: the block's share of partial_sum(X = t + 1)
// over the h row pairs (i, i + h) of a height-2h table; *nb = blocks launched,
// *threads (optional) = the block size.
// smask != 0 (the sum columns, bit j = column j): also lin[block] = the
// block's sum over its rows and the mask's columns of hi, lin[nb + block] =
// that of hi - lo (lin: 2 * kCsMaxBlocks elements).
hipError_t launch_cs_sums(const CsDev& P, uint32_t threads, const fe* m, const fe* d, uint64_t h,
                          fe* partials, hipStream_t st, uint32_t* nb, uint32_t smask = 0,
                          fe* lin = nullptr);
// fold the height-S tables with r (r_dev non-null: read from the device) in
// place, then the sums of the folded height-S/2 tables as above (S >= 4).
hipError_t launch_cs_fold_sums(const CsDev& P, uint32_t threads, fe* m, fe* d, uint64_t S, fe r,
                               const fe* r_dev, fe* partials, hipStream_t st, uint32_t* nb,
                               uint32_t smask = 0, fe* lin = nullptr);
// fold only (all `width` columns and delta), S >= 2
hipError_t launch_cs_fold(uint32_t width, fe* m, fe* d, uint64_t S, fe r, const fe* r_dev,
                          hipStream_t st);
// one round on the device: reduce the partials, e0 = claim - e1, coefficients
// through the inverse Vandermonde matrix vinv ((D+1)^2), absorb c1..cD, draw
// r, claim = pol(r); coefficients c1..cD to poly_out, r to r_out.  lin
// non-null: evals[t] += beta * (A + (t - 1) B), A and B the sums of lin's two
// rows of nb partials (the sum columns' linear part).
hipError_t launch_cs_round(const fe* partials, uint32_t nb, uint32_t D, const fe* vinv, fe* prev,
                           DevSha* t, fe* poly_out, fe* r_out, hipStream_t st,
                           const fe* lin = nullptr, fe beta = fe{});
// out[t] = sum_b partials[t * nb + b] (the step API's reduction)
hipError_t launch_cs_reduce(const fe* partials, uint32_t nb, uint32_t D, fe* out, hipStream_t st);

}  // namespace mlh
