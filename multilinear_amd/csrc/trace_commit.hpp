// Trace commitment launch interface (internal to libmlhip): the row-major
// trace as its column MLEs (Commitment::new's input, constraint_system/
// trace.rs:40-48), kernel in trace_commit.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

namespace mlh {

constexpr uint32_t kTcThreads = 256;
constexpr uint32_t kTcTileElems = 2048;  // 16-byte elements a block stages per tile (32 KiB)
constexpr uint32_t kTcMinRows = 64;      // a column's run per tile: at least 1 KiB contiguous
constexpr uint32_t kTcMaxBlocks = 1024;  // 4 per CU; a block loops over the tiles beyond that

// Rows per tile for a trace of `width` columns: the power of two with
// rows * width <= kTcTileElems (width <= 32, so at least kTcMinRows).
inline uint32_t tc_tile_rows(uint32_t width) {
  uint32_t r = kTcMinRows;
  while (2 * r * width <= kTcTileElems) r *= 2;
  return r;
}
// LDS pitch (in 16-byte elements) of one column's rows.  The staging stores
// are ds_write_b128: 8 consecutive lanes per LDS cycle, bank = (addr / 4) mod
// 32, so the 8 lanes' element slots must differ mod 8.  Lane e holds element
// (i, j) = (e / W, e mod W) and stores to slot j * pitch + i:
//   W odd:      pitch = W (mod 8) gives slot = pitch * e (mod 8), a bijection
//               on 8 consecutive e (W * W = 1 mod 8);
//   W = 2, 4:   pitch = 8 / W (mod 8): the 8 lanes are 8 / W rows x W columns;
//   W >= 8 or W = 6: pitch odd: the lanes of one row hit 8 different slots
//               (W = 6, 10, 12, ...: the lanes that wrap into the next row
//               collide 2-way, one extra LDS cycle under the store's 13).
// The column reads are ds_read_b128 of consecutive slots: conflict-free in
// its four 16-lane groups whatever the pitch.
inline uint32_t tc_pitch(uint32_t width, uint32_t rows) {
  uint32_t t = 1;
  if (width & 1)
    t = width & 7;
  else if (width == 2)
    t = 4;
  else if (width == 4)
    t = 2;
  return rows + t;  // rows is a multiple of 8
}
inline uint32_t tc_blocks(uint64_t height, uint32_t width) {
  const uint32_t rows = tc_tile_rows(width);
  const uint64_t tiles = (height + rows - 1) / rows;
  return (uint32_t)(tiles < kTcMaxBlocks ? tiles : kTcMaxBlocks);
}

// out[j * height + i] = in[i * width + col0 + j], i < height = 2^log_height,
// j < ncols (col0 + ncols <= width, width 1..32); in and out must not overlap.
// The tile, the pitch and the grid are those of an ncols-wide trace --
// tc_tile_rows(ncols), tc_pitch(ncols, R), tc_blocks(height, ncols).  The pitch
// rule above is a statement about the lane -> (i, j) map and the LDS slot
// j * pitch + i alone; in the range kernel that map is (e / ncols, e mod ncols),
// so the rule holds with ncols for W.  What changes with a range narrower than
// the width is the global side only (runs of ncols * 16 bytes at a stride of
// width * 16; the range kernel); the whole width runs trace_columns_kernel on
// contiguous tiles.  Reads nothing outside the range.
hipError_t launch_trace_columns(const fe* in, fe* out, uint32_t log_height, uint32_t width,
                                uint32_t col0, uint32_t ncols, hipStream_t st);

}  // namespace mlh
