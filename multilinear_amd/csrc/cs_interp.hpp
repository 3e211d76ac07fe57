// The device interpreter of constraint programs (internal to libmlhip): what
// cs_sumcheck.hip (the sumcheck's composition at D points per row pair) and
// trace_check.hip (the constraints once per row) share.  A lane's register
// file lives in LDS as [slot][lane] (cs_sumcheck.hip's header comment): slots
// [0, width) the row's columns, [width, width + n_temps) the temps.  Decode is
// wave-uniform: the instruction words and the uniform pool are read through
// uniform addresses.
#pragma once
#include "cs_program.hpp"
#include "cs_sumcheck.hpp"
#include "field.hpp"
#include "sc_dev.hpp"

namespace mlh {

// (row, column) of the elements tid, tid + B, tid + 2B, ... of a chunk
struct CsWalk {
  uint32_t row, col, srow, scol, W;
  __device__ __forceinline__ CsWalk(uint32_t tid, uint32_t B, uint32_t W_)
      : row(tid / W_), col(tid % W_), srow(B / W_), scol(B % W_), W(W_) {}
  __device__ __forceinline__ void next() {
    row += srow;
    col += scol;
    if (col >= W) {
      col -= W;
      ++row;
    }
  }
};

__device__ __forceinline__ fe cs_fetch(uint32_t o, const fe* __restrict__ uni, const fe* lane_lds,
                                       uint32_t B) {
  if (o & kCsUniform) return fe_vgpr(uni[o & 0x7FFFu]);
  return lane_lds[o * B];
}

// Instruction pc of the program on this lane's slots (lane_lds = the lane's
// column of the LDS slots, B lanes per slot); a caller runs pc = 0 .. n_instr -
// 1 in order.  (The `for` stays with the callers: with the loop inside this
// function the sumcheck kernels came out with one scalar compare and branch of
// the other polarity, and their bytes are to stay what they were.)  Every
// result is canonical: fe_add, fe_sub, fe_neg and fe_mul_s return the
// representative below M.
__device__ __forceinline__ void cs_step(const CsDev& P, fe* lane_lds, uint32_t B, uint32_t pc) {
  const uint32_t w0 = P.code[2 * pc], w1 = P.code[2 * pc + 1];
  const uint32_t op = w0 & 0xFFu;
  const fe a = cs_fetch(w1 & 0xFFFFu, P.uni, lane_lds, B);
  fe r;
  if (op == kCsNeg) {
    r = fe_neg(a);
  } else {
    const fe b = cs_fetch(w1 >> 16, P.uni, lane_lds, B);
    if (op == kCsMul)
      r = fe_mul_s(a, b);
    else if (op == kCsAdd)
      r = fe_add(a, b);
    else
      r = fe_sub(a, b);
  }
  lane_lds[(w0 >> 8) * B] = r;
}

}  // namespace mlh
