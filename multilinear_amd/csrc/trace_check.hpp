// Launch interface of trace_check.hip (internal to libmlhip): the witness
// check behind mlh_trace_check -- a constraint program run once per row of the
// row-major trace, next-row operands read by address, and integer verdicts
// reduced into a pooled counter array.  include/mlhip.h gives the semantics,
// DESIGN 6l the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cs_program.hpp"
#include "cs_sumcheck.hpp"
#include "field.hpp"
#include "trace_shift.hpp"

namespace mlh {

constexpr uint32_t kTkMaxBlocks = 1024;  // 4 per CU; a block loops over the chunks beyond that

// LDS slots per lane: the W + K columns of the extended row (the program's
// width) and the temps.  No step slots and no sums (cs_slots has both).
static inline uint32_t tk_slots(const CsProgram& p) { return p.width + p.n_temps; }
static inline bool tk_shape_ok(uint32_t slots, uint32_t threads, uint32_t max_blocks) {
  return (threads == 64 || threads == 128 || threads == 256) && max_blocks >= 1 &&
         max_blocks <= kTkMaxBlocks && (uint64_t)slots * 16 * threads <= kCsLdsBytes;
}
// The default grid: a block takes at least kCsRowsPerThread chunks of `threads`
// rows before the grid grows.
static inline uint32_t tk_blocks(uint64_t height, uint32_t threads) {
  const uint64_t per = (uint64_t)threads * kCsRowsPerThread, b = (height + per - 1) / per;
  return (uint32_t)(b < kTkMaxBlocks ? b : kTkMaxBlocks);
}
// The grid of an explicit shape: one block per chunk up to max_blocks.
static inline uint32_t tk_blocks_shaped(uint64_t height, uint32_t threads, uint32_t max_blocks) {
  const uint64_t chunks = (height + threads - 1) / threads;
  return (uint32_t)(chunks < max_blocks ? chunks : max_blocks);
}

// The counters of one call, 64-bit words: [0, NC) the failing rows per
// constraint, [NC] the rows with any failing constraint, [NC + 1, 2 NC + 1)
// the lowest failing row per constraint (all ones: none).  The caller zeroes
// the first NC + 1 and sets the rest to all ones on the stream before the
// launch.
static inline size_t tk_counter_words(uint32_t n_constraints) { return 2 * (size_t)n_constraints + 1; }

// P: the program's device image, P.width = width + n_shifts; m: 2^log_height x
// width, row-major; cols[k] < width.  The caller has checked tk_shape_ok.
hipError_t launch_trace_check(const CsDev& P, const fe* m, uint32_t log_height, uint32_t width,
                              const uint32_t* cols, uint32_t n_shifts, uint64_t* counters,
                              uint32_t threads, uint32_t blocks, hipStream_t st);

}  // namespace mlh
