// Launch interface of trace_scan.hip (internal to libmlhip): exclusive prefix
// scans (running sums and running products) down columns of a row-major trace,
// in place, as three stream-ordered launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

namespace mlh {

constexpr uint32_t kScanAdd = 0, kScanMul = 1;
constexpr uint32_t kScanMaxScans = 8, kScanMaxBlocks = 1024, kScanMaxRowsPerThread = 16;
// Default launch rule: 256 threads, 4 consecutive rows per thread, and
// min(ceil(height / 1024), 1024) blocks.
constexpr uint32_t kScanThreads = 256, kScanRowsPerThread = 4;

static inline bool scan_shape_ok(uint32_t threads, uint32_t rows_per_thread, uint32_t max_blocks) {
  return (threads == 64 || threads == 128 || threads == 256) && rows_per_thread >= 1 &&
         rows_per_thread <= kScanMaxRowsPerThread && !(rows_per_thread & (rows_per_thread - 1)) &&
         max_blocks >= 1 && max_blocks <= kScanMaxBlocks;
}
// Tiles of threads * rows_per_thread rows, and the blocks that share them.
static inline uint64_t scan_tiles(uint64_t height, uint32_t threads, uint32_t rows_per_thread) {
  const uint64_t t = (uint64_t)threads * rows_per_thread;
  return (height + t - 1) / t;
}
static inline uint32_t scan_blocks(uint64_t tiles, uint32_t max_blocks) {
  return tiles < max_blocks ? (uint32_t)tiles : max_blocks;
}
// Both, and the tiles each block owns, where asked for.  -> the blocks
static inline uint32_t scan_tiling(uint64_t height, uint32_t threads, uint32_t rows_per_thread,
                                   uint32_t max_blocks, uint64_t* tiles = nullptr,
                                   uint64_t* tiles_per_block = nullptr) {
  const uint64_t t = scan_tiles(height, threads, rows_per_thread);
  const uint32_t blocks = scan_blocks(t, max_blocks);
  if (tiles) *tiles = t;
  if (tiles_per_block) *tiles_per_block = (t + blocks - 1) / blocks;
  return blocks;
}

// One call's scans, by value (every index into the arrays is a compile-time
// constant in the kernels: no private segment).
struct ScanArgs {
  fe* m;            // height x width, row-major
  uint64_t height;
  uint64_t tiles, tiles_per_block;  // block b owns tiles [b tpb, min((b + 1) tpb, tiles))
  uint32_t width, n_scans, rows_per_thread, blocks;
  // scratch of this call: aggregates[s * blocks + b], offsets[s * blocks + b], totals[s]
  fe* aggregates;
  fe* offsets;
  fe* totals;
  uint8_t op[kScanMaxScans], src[kScanMaxScans], dst[kScanMaxScans];
  fe init[kScanMaxScans];
};
static inline size_t scan_scratch_elems(uint32_t n_scans, uint32_t blocks) {
  return (size_t)n_scans * (2 * (size_t)blocks + 1);
}

// The scans of `a` on st: with a.blocks > 1 the reduce, the offsets and the
// apply launch; with one block the apply launch alone (offset = init).
// a.totals holds the n_scans totals behind them on the stream.
hipError_t launch_trace_scan(const ScanArgs& a, uint32_t threads, hipStream_t st);

}  // namespace mlh
