// Public columns on the device (internal to libmlhip): the kernels that write
// the strip [width - F, width) of a row-major trace from a spec's device image
// (public_columns.hpp), in trace_public.hip.  include/mlhip.h and DESIGN 6j
// give the format and the protocol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"
#include "public_columns.hpp"

namespace mlh {

constexpr uint32_t kTpThreads = 256;
constexpr uint32_t kTpTileElems = 2048;  // 16-byte strip elements a block writes per tile
constexpr uint32_t kTpMaxBlocks = 1024;  // 4 per CU; a block loops over the tiles beyond that
constexpr uint32_t kTpMaxWidth = 32;

// Rows per tile for a strip of F columns: the power of two with rows * F <=
// kTpTileElems (F <= 16, so at least 128), at most the height.
inline uint32_t tp_log_rows(uint32_t log_height, uint32_t F) {
  uint32_t lr = 0;
  while ((2u << lr) * F <= kTpTileElems) ++lr;
  return lr < log_height ? lr : log_height;
}
inline uint32_t tp_blocks(uint32_t log_height, uint32_t F) {
  const uint64_t tiles = (1ull << log_height) >> tp_log_rows(log_height, F);
  return (uint32_t)(tiles < kTpMaxBlocks ? tiles : kTpMaxBlocks);
}

// matrix (row-major 2^log_height x width): columns [width - F, width) = the
// spec's columns; image: the spec's device image (pc_build_image) on the
// device, n_sparse entries at word sparse_off.  1 <= F <= min(width, 16), width
// <= 32, log_height <= 32, every period <= 2^log_height and every sparse row <
// 2^log_height (the caller checks).  The strip kernel, then the scatter.
hipError_t launch_trace_fill_public(fe* matrix, const void* image, uint32_t F, uint32_t sparse_off,
                                    uint32_t n_sparse, uint32_t log_height, uint32_t width,
                                    hipStream_t st);

// The strip of the matrix against the spec's image, nothing written: counters
// (2 F + 1 64-bit words: [0, F) the differing rows per column, [F] the rows
// with any difference, [F + 1, 2 F + 1) the lowest differing row per column,
// all ones when none; the caller zeroes the first F + 1 and sets the rest to
// all ones on the stream before the launch).  The limits of
// launch_trace_fill_public.
hipError_t launch_trace_check_public(const fe* matrix, const void* image, uint32_t F,
                                     uint32_t sparse_off, uint32_t log_height, uint32_t width,
                                     uint64_t* counters, hipStream_t st);

}  // namespace mlh
