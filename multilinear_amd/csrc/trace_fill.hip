// Phase 2 of the two-phase system proof on gfx950 (WitnessLayout, system.rs:
// 23-29): fill the columns that depend on the trace randoms in place
// (trace_fill_kernel, a fill program of cs_program.hpp per row), and the sum of
// the sum columns (trace_column_sum_kernel).
//
// trace_fill_kernel.  Every lane interprets the program on its own rows, its
// register file in LDS as [slot][lane] 16-byte elements like cs_sumcheck.hip's
// (runtime-indexed per-thread arrays would go to scratch):
//   slots [0, W)                 the row's columns as they stood at entry
//   slots [W, W + T)             the program's temps
//   slots [W + T, .. + n_inv)    per INV v: the running prefix product, then inv_v
// The cost of a fill is the inverse: 138 products (fe_inv.hpp), and one lane
// running the chain costs its SIMD what 64 lanes do.  So a lane inverts once
// per INV for K of its rows (Montgomery's trick per lane, as field_inv_kernel).
// The prefix products p[v][k], k < K - 1, go to a global scratch buffer
// ([block][v][k][lane]: coalesced, each element written and read back by one
// lane only, L2-resident); in LDS they would take n_inv K slots per lane and
// leave one wave per SIMD, with every load and LDS latency of the staging and
// of the interpreter exposed (measured: DESIGN.md 6f).
// A block of B threads takes chunks of B K consecutive rows; lane tid owns the
// rows base + k B + tid, k < K.  For a fixed k the B rows are W B contiguous
// elements: loaded coalesced and scattered into the [column][row] slots as
// cs_sums_body does.  INV operands never depend on an INV (fill_decode), so:
//   sweep 1, k = 0 .. K-1: stage row batch k, run the instructions up to the
//     last INV whose values do not depend on an INV; at INV v its operand is
//     the denominator d; d' = d, or one for a zero or a lane without a row;
//     p[v][k] = p[v][k-1] d'.
//   inv_v = p[v][K-1]^(M-2), once per lane and INV, kept in INV v's slot.
//   sweep 2, k = K-1 .. 0: stage row batch k again (from L2 / HBM: cheap
//     beside 20+ products), run the whole program; INV v gives zero for d = 0,
//     else inv_v p[v][k-1] (inv_v at k = 0), then inv_v *= d'; the lane that
//     owns the row stores the outputs.
// 3 + 138 / K products per row and inverse; only the prefixes are kept, the
// denominators are recomputed.  Without an INV: K = 1 and sweep 2 alone.
// Column operands read the staged copy and only outputs are stored, so an
// output column reads its old value and the other columns are not written.
//
// LDS banking of the scatter (ds_write_b128: 8 groups of 8 lanes, bank =
// 16-byte unit mod 8): lanes e .. e+7 write rows e / W of columns e mod W, unit
// = column B + row, so the lanes of a group that share a row collide: up to
// min(W, 8)-way on W stores per row and sweep, beside 20+ products of ~70 VALU
// instructions each -- an estimated 2 % of the kernel; cs_sums_body's layout kept.
// The interpreter's own accesses are lane-contiguous: conflict free.
#include "bfly_asm.hpp"
#include "cs_program.hpp"
#include "cs_sumcheck.hpp"
#include "fe_inv.hpp"
#include "field.hpp"
#include "sc_dev.hpp"
#include "trace_fill.hpp"

namespace mlh {

__device__ __forceinline__ fe fill_fetch(uint32_t o, const fe* __restrict__ uni, const fe* lane_lds,
                                         uint32_t B) {
  if (o & kCsUniform) return fe_vgpr(uni[o & 0x7FFFu]);
  return lane_lds[o * B];
}

// Rows [row0, row0 + nrows) of the matrix into the column slots (nrows <= B).
__device__ __forceinline__ void fill_stage(fe* lds, const fe* m, uint64_t row0,
                                           uint32_t nrows, uint32_t B, uint32_t W) {
  const fe* src = m + row0 * W;
  uint32_t row = threadIdx.x / W, col = threadIdx.x % W;  // (the CsWalk of cs_sumcheck.hip)
  const uint32_t srow = B / W, scol = B % W;
  for (uint32_t e = threadIdx.x; e < nrows * W; e += B) {
    lds[col * B + row] = fe_load(src + e);
    row += srow;
    col += scol;
    if (col >= W) {
      col -= W;
      ++row;
    }
  }
}

// One pass of the interpreter over this lane's staged row.  FULL = false:
// sweep 1 (instructions [0, n_pre) that are not tainted; INV v extends the
// prefix).  FULL = true: sweep 2 (everything; INV v takes its result from
// inv_v and the prefix).  valid = the lane has a row in this batch.
template <bool FULL>
__device__ __forceinline__ void fill_run(const FillDev& P, fe* lane_lds, uint32_t B, uint32_t k,
                                         bool valid) {
  const uint32_t K = P.K, acc0 = P.width + P.n_temps;
  const uint32_t n = FULL ? P.n_instr : P.n_pre;
  for (uint32_t pc = 0; pc < n; ++pc) {
    const uint32_t w0 = P.code[2 * pc], w1 = P.code[2 * pc + 1];
    const uint32_t op = w0 & 0xFFu;
    if (!FULL && (w0 & kFillTainted) && op != kCsInv) continue;  // (wave-uniform)
    const fe a = fill_fetch(w1 & 0xFFFFu, P.uni, lane_lds, B);
    if (op == kCsInv) {
      const uint32_t v = w1 >> 16;
      fe* acc = lane_lds + (acc0 + v) * B;  // sweep 1: p[v][k]; sweep 2: inv_v
      // p[v][k], k < K - 1, of this block and lane (written and read by this lane only)
      fe* pv = P.prefix + ((uint64_t)blockIdx.x * P.n_inv + v) * (K - 1) * B + threadIdx.x;
      const bool z = !valid || fe_is_zero(a);
      if (!FULL) {
        const fe d = z ? fe_one() : a;
        const fe p = k ? fe_mul_s(*acc, d) : d;
        *acc = p;
        if (k + 1 < K) fe_store(pv + (uint64_t)k * B, p);
      } else {
        const fe inv = *acc;
        const fe r = k ? fe_mul_s(inv, fe_load(pv + (uint64_t)(k - 1) * B)) : inv;
        lane_lds[((w0 >> 8) & 0xFFu) * B] = z ? fe_zero() : r;
        if (k && !z) *acc = fe_mul_s(inv, a);
      }
      continue;
    }
    fe r;
    if (op == kCsNeg) {
      r = fe_neg(a);
    } else {
      const fe b = fill_fetch(w1 >> 16, P.uni, lane_lds, B);
      if (op == kCsMul)
        r = fe_mul_s(a, b);
      else if (op == kCsAdd)
        r = fe_add(a, b);
      else
        r = fe_sub(a, b);
    }
    lane_lds[((w0 >> 8) & 0xFFu) * B] = r;
  }
}

__global__ void __launch_bounds__(256)
trace_fill_kernel(const FillDev P, fe* m, uint64_t h, uint64_t chunks) {
  extern __shared__ fe fill_lds[];
  const uint32_t B = blockDim.x, tid = threadIdx.x, W = P.width, K = P.K;
  const uint32_t acc0 = W + P.n_temps;
  fe* lane_lds = fill_lds + tid;
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const uint64_t base = c * ((uint64_t)B * K);
    if (P.n_inv) {
      for (uint32_t k = 0; k < K; ++k) {
        const uint64_t row0 = base + (uint64_t)k * B;
        const uint32_t nrows = row0 >= h ? 0u : (h - row0 < B ? (uint32_t)(h - row0) : B);
        fill_stage(fill_lds, m, row0, nrows, B, W);
        __syncthreads();
        fill_run<false>(P, lane_lds, B, k, tid < nrows);
        __syncthreads();  // the next batch's loads overwrite other lanes' slots
      }
      for (uint32_t v = 0; v < P.n_inv; ++v) {  // p[v][K-1] -> inv_v
        fe* s = lane_lds + (acc0 + v) * B;
        *s = fe_inv_chain(*s);
      }
    }
    for (uint32_t k = K; k-- > 0;) {
      const uint64_t row0 = base + (uint64_t)k * B;
      const uint32_t nrows = row0 >= h ? 0u : (h - row0 < B ? (uint32_t)(h - row0) : B);
      if (!P.n_inv || k != K - 1) {  // (sweep 1 ended on batch K - 1: still staged)
        fill_stage(fill_lds, m, row0, nrows, B, W);
        __syncthreads();
      }
      const bool valid = tid < nrows;
      fill_run<true>(P, lane_lds, B, k, valid);
      if (valid) {
        fe* row = m + (row0 + tid) * W;
        for (uint32_t o = 0; o < P.n_outputs; ++o) {
          const uint32_t w = P.outs[o];
          fe_store(row + (w >> 16), fill_fetch(w & 0xFFFFu, P.uni, lane_lds, B));
        }
      }
      __syncthreads();
    }
  }
}

hipError_t launch_trace_fill(const FillDev& P, uint32_t threads, uint32_t blocks, fe* m,
                             uint64_t height, hipStream_t st) {
  const uint64_t lds = (uint64_t)(P.width + P.n_temps + P.n_inv) * threads * sizeof(fe);
  if (height == 0 || (threads != 64 && threads != 128 && threads != 256) || P.K < 1 ||
      lds > kCsLdsBytes || P.width < 1 || P.n_pre > P.n_instr || blocks < 1 ||
      (P.n_inv && P.K > 1 && !P.prefix))
    return hipErrorInvalidValue;
  const uint64_t chunks = fill_chunks(height, threads, P.K);
  if (blocks > chunks) blocks = (uint32_t)chunks;
  hipLaunchKernelGGL(trace_fill_kernel, dim3(blocks), dim3(threads), (size_t)lds, st, P, m, height,
                     chunks);
  return hipGetLastError();
}

// partials[block] = the block's share of sum_i sum_{j in mask} m[i W + j]: one
// streaming pass over the n = height * W elements, 16 bytes per lane and step,
// a lane's column advancing by (grid size mod W) with a carry.
__global__ void __launch_bounds__(kSumThreads)
trace_column_sum_kernel(const fe* __restrict__ m, uint64_t n, uint32_t W, uint32_t mask,
                        fe* __restrict__ partials) {
  __shared__ fe red[4];
  const uint64_t stride = (uint64_t)gridDim.x * kSumThreads;
  uint64_t e = (uint64_t)blockIdx.x * kSumThreads + threadIdx.x;
  uint32_t col = (uint32_t)(e % W);
  const uint32_t scol = (uint32_t)(stride % W);
  fe acc = fe_zero();
  for (; e < n; e += stride) {
    if ((mask >> col) & 1u) acc = fe_add(acc, fe_load(m + e));
    col += scol;
    if (col >= W) col -= W;
  }
  cs_block_sum(acc, kSumThreads, red, partials + blockIdx.x);
}

hipError_t launch_trace_column_sum(const fe* m, uint64_t height, uint32_t width, uint32_t mask,
                                   fe* partials, fe* out, hipStream_t st) {
  if (height == 0 || width < 1 || width > kCsMaxWidth) return hipErrorInvalidValue;
  const uint64_t n = height * width;
  const uint32_t nb = sum_blocks(n);
  hipLaunchKernelGGL(trace_column_sum_kernel, dim3(nb), dim3(kSumThreads), 0, st, m, n, width, mask,
                     partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_cs_reduce(partials, nb, 1, out, st);
}

}  // namespace mlh
