// Launch interface of trace_sort.hip (internal to libmlhip): the stable
// ascending sort of the rows of a row-major trace by up to 4 key columns, as an
// LSD radix sort with 8-bit digits over (key limb, row index) pairs, and the
// gather that writes the sorted copies and the index column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"
#include "trace_scan.hpp"  // the tile and block rule: scan_shape_ok, scan_tiles, scan_blocks

namespace mlh {

constexpr uint32_t kSortMaxKeys = 4, kSortMaxCopies = 16, kSortNoColumn = 0xFFFFFFFFu;
constexpr uint32_t kSortMaxLogHeight = 28;  // row indices and counters are 32-bit
constexpr uint32_t kSortBins = 256, kSortDigitsPerKey = 16;
constexpr uint32_t kSortRunAll = 1u;  // flags bit 0: no digit pass is skipped
// Default launch rule: 256 threads, 8 rows per thread, and
// min(ceil(height / 2048), 1024) blocks.
constexpr uint32_t kSortThreads = 256, kSortRowsPerThread = 8;
// The census runs on at most this many blocks (a block flushes up to 4096 bins
// per key with one global atomic each).
constexpr uint32_t kSortCensusBlocks = 256;
constexpr uint32_t kSortOffsetThreads = 1024;

// One call, by value.
struct SortArgs {
  fe* m;  // height x width, row-major
  uint64_t height;
  uint64_t tiles, tiles_per_block;  // block b owns tiles [b tpb, min((b + 1) tpb, tiles))
  uint32_t width, n_keys, n_copies, perm_column;
  uint32_t threads, rows_per_thread, blocks;
  // scratch of this call
  uint2* items[2];   // (key limb, row) pairs, ping-pong: height each
  uint32_t* census;  // [16 n_keys][256]: rows whose digit g has the value v
  uint32_t* same;    // [16 n_keys]: nonzero when all rows agree in digit g
  uint32_t* hist;    // [256][sort_stride(blocks)], digit-major: the blocks' counts of one pass
  uint32_t* offsets; // [256][sort_stride(blocks)]: where block b's first row of value v goes
  uint8_t key[kSortMaxKeys], src[kSortMaxCopies], dst[kSortMaxCopies];
};

static inline size_t sort_align(size_t b) { return (b + 255) & ~(size_t)255; }
// The length of a row of hist and offsets: 16-byte loads and stores in the scan.
__host__ __device__ static inline uint32_t sort_stride(uint32_t blocks) {
  return (blocks + 3u) & ~3u;
}
// items[0], items[1], census, same, hist, offsets, each 256-byte aligned:
// 16 bytes per row, 16 KiB per key and 2 KiB per block (in fours), plus 256 bytes.
static inline size_t sort_scratch_bytes(uint64_t height, uint32_t n_keys, uint32_t blocks) {
  return 2 * sort_align(height * sizeof(uint2)) +
         sort_align((size_t)n_keys * kSortDigitsPerKey * kSortBins * 4) +
         sort_align((size_t)kSortMaxKeys * kSortDigitsPerKey * 4) +
         2 * sort_align((size_t)kSortBins * sort_stride(blocks) * 4);
}
static inline void sort_carve(SortArgs& a, void* scratch) {
  uint8_t* p = reinterpret_cast<uint8_t*>(scratch);
  a.items[0] = reinterpret_cast<uint2*>(p);
  p += sort_align(a.height * sizeof(uint2));
  a.items[1] = reinterpret_cast<uint2*>(p);
  p += sort_align(a.height * sizeof(uint2));
  a.census = reinterpret_cast<uint32_t*>(p);
  p += sort_align((size_t)a.n_keys * kSortDigitsPerKey * kSortBins * 4);
  a.same = reinterpret_cast<uint32_t*>(p);
  p += sort_align((size_t)kSortMaxKeys * kSortDigitsPerKey * 4);
  a.hist = reinterpret_cast<uint32_t*>(p);
  p += sort_align((size_t)kSortBins * sort_stride(a.blocks) * 4);
  a.offsets = reinterpret_cast<uint32_t*>(p);
}

// The digit census of the key columns on st: a.census zeroed and counted, and
// a.same[g] for every digit g = 16 k + byte (byte 0 the least significant of
// key k).
hipError_t launch_sort_census(const SortArgs& a, hipStream_t st);
// The digit passes in `run` (bit g: digit g runs), least significant first and
// the last key first, then the gather.  With run == 0 the gather alone (the
// identity permutation).
hipError_t launch_sort_passes(const SortArgs& a, uint64_t run, hipStream_t st);

}  // namespace mlh
