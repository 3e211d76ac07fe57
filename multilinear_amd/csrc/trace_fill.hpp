// Launch interface of trace_fill.hip (internal to libmlhip): the in-place fill
// of a row-major trace by a fill program (cs_program.hpp) and the sum of a set
// of its columns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

namespace mlh {

// A fill program's device image (cs_program.hpp fill_build_image), by value.
struct FillDev {
  const fe* uni;         // uniform pool: randoms | consts
  const uint32_t* code;  // 2 words per instruction
  const uint32_t* outs;  // 1 word per output
  uint32_t width, n_temps, n_instr, n_pre, n_inv, n_outputs;
  uint32_t K;   // rows per thread and inversion
  fe* prefix;   // scratch: n_inv * (K - 1) * threads elements per block
};

// The program on every row of the height x width matrix m, in place: one
// launch of at most `blocks` blocks of `threads` (64, 128, 256); (width +
// n_temps + n_inv) 16-byte LDS slots per thread, within kCsLdsBytes.
hipError_t launch_trace_fill(const FillDev& P, uint32_t threads, uint32_t blocks, fe* m,
                             uint64_t height, hipStream_t st);
// out[0] = sum_i sum_{j in mask} m[i * width + j] (partials: kCsMaxBlocks elements)
hipError_t launch_trace_column_sum(const fe* m, uint64_t height, uint32_t width, uint32_t mask,
                                   fe* partials, fe* out, hipStream_t st);

}  // namespace mlh
