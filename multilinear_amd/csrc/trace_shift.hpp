// Shifted columns (internal to libmlhip): the row-rotated extension of a trace
// and the eq table rotated by one row, kernels in trace_shift.hip.  The
// next-row constraints of the shifted system proof (include/mlhip.h, DESIGN
// 6i) run the ordinary constraint sumcheck on the extension.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

namespace mlh {

constexpr uint32_t kTsThreads = 256;
constexpr uint32_t kTsTileElems = 2048;  // 16-byte output elements a block writes per tile (32 KiB)
constexpr uint32_t kTsMinRows = 64;
constexpr uint32_t kTsMaxBlocks = 1024;  // 4 per CU; a block loops over the tiles beyond that
constexpr uint32_t kTsMaxWidth = 32;     // of the extension, W + K

// The source columns c_0 .. c_{K-1}, one byte each, as a kernel argument.
struct ShiftCols {
  uint64_t w[4];
};

// Rows per tile for an extension of `wext` columns: the power of two with
// rows * wext <= kTsTileElems (wext <= 32, so at least kTsMinRows), at most
// the height.
inline uint32_t ts_log_rows(uint32_t log_height, uint32_t wext) {
  uint32_t lr = 6;
  while ((2u << lr) * wext <= kTsTileElems) ++lr;
  return lr < log_height ? lr : log_height;
}
inline uint32_t ts_blocks(uint32_t log_height, uint32_t wext) {
  const uint64_t tiles = (1ull << log_height) >> ts_log_rows(log_height, wext);
  return (uint32_t)(tiles < kTsMaxBlocks ? tiles : kTsMaxBlocks);
}

// out (row-major 2^log_height x (width + n_shifts)):
//   out[i][j] = in[i][j], j < width;
//   out[i][width + k] = in[(i + 1) mod 2^log_height][cols[k]].
// cols[k] < width, width + n_shifts <= 32 (the caller checks); in and out must
// not overlap.  n_shifts = 0 is a copy.
hipError_t launch_trace_extend_next(const fe* in, fe* out, uint32_t log_height, uint32_t width,
                                    const uint32_t* cols, uint32_t n_shifts, hipStream_t st);

// out[j] = in[(j - 1) mod 2^log_n], out of place.
hipError_t launch_eq_rotate(const fe* in, fe* out, uint32_t log_n, hipStream_t st);

}  // namespace mlh
