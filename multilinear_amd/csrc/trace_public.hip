// Public columns: the kernels behind mlh_trace_fill_public.
//
// trace_fill_public_kernel writes the strip [W - F, W) of the row-major H x W
// matrix in the form of trace_extend_next_kernel (trace_shift.hip).  Threads
// are indexed by element of the H x F strip: a block takes tiles of R
// consecutive rows (R a power of two, R * F <= 2048 elements) and lane e
// stores element e of the tile -- row e / F, column e mod F -- 16 bytes each
// (global_store_dwordx4), the lanes of a row one contiguous run of 16 F bytes
// at row * W + (W - F), the runs 16 W bytes apart.  (row, column) is carried
// from element to element (one divide per lane, outside the loops).  The
// per-column descriptors of the spec's image -- kind, period mask, table
// offset; the constant is the image word behind them -- go to LDS once per
// block; no kernel argument is indexed.  Every element is one 16-byte load
// from the image at off + (row & mask), unguarded and in bounds whatever the
// row: a periodic column's table entry, and for the other kinds (mask 0, off
// the column's own constant word) the constant, which is zero unless CONST.
// On top of it come selects on the kind: a compare of the row for FIRST and
// LAST, the row as limbs 0 and 1 for ROW; SPARSE stays zero.  All of a lane's
// loads are issued before its first store.  A block loops over tiles t =
// block, block + grid, ...
//
// trace_scatter_public_kernel, behind it on the stream, writes the sparse
// entries, one thread per entry.
#include "trace_public.hpp"

namespace mlh {

constexpr uint32_t kTpPerLane = kTpTileElems / kTpThreads;  // 8

// Element (row, column with descriptor d) of the strip, a sparse column's
// entries apart (zero here): what trace_fill_public_kernel stores and
// trace_check_public_kernel compares.  i: the row within the tile.
__device__ __forceinline__ uint4 tp_element(const uint4 d, const uint4* __restrict__ img, uint64_t row,
                                            uint32_t i, uint32_t i_first, uint32_t i_last) {
  const uint4 p = img[d.z + ((uint32_t)row & d.y)];
  const uint32_t flag = (uint32_t)((d.x == kPcFirst && i == i_first) | (d.x == kPcLast && i == i_last));
  const bool is_row = d.x == kPcRow;
  return uint4{is_row ? (uint32_t)row : (p.x | flag), is_row ? (uint32_t)(row >> 32) : p.y, p.z, p.w};
}

__global__ __launch_bounds__(kTpThreads) void trace_fill_public_kernel(
    uint4* __restrict__ m, const uint4* __restrict__ img, uint32_t width, uint32_t F,
    uint32_t log_rows, uint64_t tiles) {
  __shared__ uint4 desc[kPcMaxColumns];
  const uint32_t lane = threadIdx.x;
  if (lane < F) desc[lane] = img[2 * lane];
  __syncthreads();
  const uint32_t n = F << log_rows;  // <= kTpTileElems
  // (row, column) of element `lane`, advanced by kTpThreads elements per step
  const uint32_t i0 = lane / F, j0 = lane - i0 * F;
  const uint32_t di = kTpThreads / F, dj = kTpThreads - di * F;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t row0 = t << log_rows;
    // the tile's row that is the matrix's first / last (none: no row of a tile)
    const uint32_t i_first = t == 0 ? 0u : ~0u;
    const uint32_t i_last = t == tiles - 1 ? (1u << log_rows) - 1 : ~0u;
    uint4* dst = m + row0 * width + (width - F);
    uint4 v[kTpPerLane];
    uint32_t at[kTpPerLane];
    uint32_t i = i0, j = j0;
#pragma unroll
    for (uint32_t k = 0; k < kTpPerLane; ++k) {
      const uint4 d = desc[j];  // kind, mask, off
      v[k] = tp_element(d, img, row0 + i, i, i_first, i_last);
      at[k] = i * width + j;
      i += di;
      j += dj;
      if (j >= F) {
        j -= F;
        ++i;
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < kTpPerLane; ++k) {
      const uint32_t e = lane + k * kTpThreads;
      if (e < n) dst[at[k]] = v[k];
    }
  }
}

__global__ __launch_bounds__(kTpThreads) void trace_scatter_public_kernel(
    uint4* __restrict__ m, const uint4* __restrict__ entries, uint32_t n_sparse, uint32_t width,
    uint32_t F) {
  const uint32_t e = blockIdx.x * kTpThreads + threadIdx.x;
  if (e >= n_sparse) return;
  const uint4 d = entries[2 * e];
  const uint64_t row = (uint64_t)d.x | ((uint64_t)d.y << 32);
  m[row * width + (width - F) + d.z] = entries[2 * e + 1];
}

// trace_check_public_kernel (mlh_trace_check_public): the sibling
// of trace_fill_public_kernel that loads and compares where that one stores --
// the same tiling, the same element (tp_element).  The expected value of an
// element of a SPARSE column comes from a binary search over that column's
// entries of the image (sorted by row; the descriptor's fourth word is the
// column's first entry | count << 16): at most 12 halvings for 4096 entries,
// taken by the elements of SPARSE columns only.
// The verdict of an element is "its 16 bytes differ".  Per step of the tile a
// wave takes one ballot; only when it is not zero does it go through the
// columns, one ballot each, and the lowest lane of a column's ballot -- rows
// ascend with the lane -- adds the popcount to the block's count of that
// column and takes the min of its row into the column's first row (LDS).  A
// failing element also sets its row's bit in a bitmap of the tile's rows, which
// 64 threads count and clear behind the tile's barrier: the rows with any
// mismatch.  At its end the block flushes the counters that are not zero with
// 64-bit atomicAdd / atomicMin: counters[j] the count of column j, counters[F]
// the rows, counters[F + 1 + j] the first row of column j.  Integer adds and
// mins only: a pure function of the matrix and the spec.
__global__ __launch_bounds__(kTpThreads) void trace_check_public_kernel(
    const uint4* __restrict__ m, const uint4* __restrict__ img, uint32_t width, uint32_t F,
    uint32_t log_rows, uint64_t tiles, uint32_t sparse_off, unsigned long long* __restrict__ counters) {
  using u64 = unsigned long long;
  __shared__ uint4 desc[kPcMaxColumns];
  __shared__ u64 count[kPcMaxColumns + 1], first[kPcMaxColumns];
  __shared__ uint32_t row_bits[kTpTileElems / 32];  // (a tile has at most kTpTileElems rows)
  const uint32_t lane = threadIdx.x;
  if (lane < F) {
    desc[lane] = img[2 * lane];
    first[lane] = ~0ull;
  }
  if (lane <= F) count[lane] = 0;
  if (lane < kTpTileElems / 32) row_bits[lane] = 0;
  __syncthreads();
  const uint32_t n = F << log_rows;  // <= kTpTileElems
  const uint32_t i0 = lane / F, j0 = lane - i0 * F;
  const uint32_t di = kTpThreads / F, dj = kTpThreads - di * F;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t row0 = t << log_rows;
    const uint32_t i_first = t == 0 ? 0u : ~0u;
    const uint32_t i_last = t == tiles - 1 ? (1u << log_rows) - 1 : ~0u;
    const uint4* strip = m + row0 * width + (width - F);
    // all of a lane's loads of the strip are issued before its first compare
    uint4 got[kTpPerLane];
    uint32_t i = i0, j = j0;
#pragma unroll
    for (uint32_t k = 0; k < kTpPerLane; ++k) {
      got[k] = lane + k * kTpThreads < n ? strip[i * width + j] : uint4{0, 0, 0, 0};
      i += di;
      j += dj;
      if (j >= F) {
        j -= F;
        ++i;
      }
    }
    i = i0;
    j = j0;
#pragma unroll
    for (uint32_t k = 0; k < kTpPerLane; ++k) {
      const uint32_t e = lane + k * kTpThreads;
      const uint4 d = desc[j];
      const uint64_t row = row0 + i;
      uint4 want = tp_element(d, img, row, i, i_first, i_last);
      if (d.x == kPcSparse) {  // the entry of this row, if the column has one
        const uint4* ent = img + sparse_off + 2 * (d.w & 0xFFFFu);
        uint32_t lo = 0, cnt = d.w >> 16;
        for (uint32_t s = 0; s < 12 && cnt > 1; ++s) {
          const uint32_t half = cnt >> 1;
          const uint4 r = ent[2 * (lo + half)];
          const bool le = (((uint64_t)r.y << 32) | r.x) <= row;
          lo = le ? lo + half : lo;
          cnt = le ? cnt - half : half;
        }
        const uint4 r = ent[2 * lo];
        if ((((uint64_t)r.y << 32) | r.x) == row) want = ent[2 * lo + 1];
      }
      const uint4 g = got[k];
      const bool bad = e < n && ((g.x ^ want.x) | (g.y ^ want.y) | (g.z ^ want.z) | (g.w ^ want.w)) != 0u;
      if (__builtin_amdgcn_ballot_w64(bad)) {
        if (bad) atomicOr(&row_bits[i >> 5], 1u << (i & 31u));
        for (uint32_t c = 0; c < F; ++c) {
          const uint64_t b = __builtin_amdgcn_ballot_w64(bad && j == c);
          if (b && (lane & 63u) == (uint32_t)__builtin_ctzll(b)) {
            atomicAdd(&count[c], (u64)__popcll(b));
            atomicMin(&first[c], (u64)row);
          }
        }
      }
      i += di;
      j += dj;
      if (j >= F) {
        j -= F;
        ++i;
      }
    }
    __syncthreads();
    if (lane < kTpTileElems / 32 && row_bits[lane]) {
      atomicAdd(&count[F], (u64)__popc(row_bits[lane]));
      row_bits[lane] = 0;
    }
    __syncthreads();  // the next tile sets bits again
  }
  if (lane <= F && count[lane]) atomicAdd(counters + lane, count[lane]);
  if (lane < F && first[lane] != ~0ull) atomicMin(counters + F + 1 + lane, first[lane]);
}

hipError_t launch_trace_check_public(const fe* matrix, const void* image, uint32_t F,
                                     uint32_t sparse_off, uint32_t log_height, uint32_t width,
                                     uint64_t* counters, hipStream_t st) {
  if (!matrix || !image || !counters || F < 1 || F > kPcMaxColumns || F > width ||
      width > kTpMaxWidth || log_height > 32)
    return hipErrorInvalidValue;
  const uint32_t log_rows = tp_log_rows(log_height, F);
  const uint64_t height = 1ull << log_height, tiles = height >> log_rows;
  hipLaunchKernelGGL(trace_check_public_kernel, dim3(tp_blocks(log_height, F)), dim3(kTpThreads), 0, st,
                     reinterpret_cast<const uint4*>(matrix), reinterpret_cast<const uint4*>(image), width,
                     F, log_rows, tiles, sparse_off, reinterpret_cast<unsigned long long*>(counters));
  return hipGetLastError();
}

hipError_t launch_trace_fill_public(fe* matrix, const void* image, uint32_t F, uint32_t sparse_off,
                                    uint32_t n_sparse, uint32_t log_height, uint32_t width,
                                    hipStream_t st) {
  if (!matrix || !image || F < 1 || F > kPcMaxColumns || F > width || width > kTpMaxWidth ||
      log_height > 32)
    return hipErrorInvalidValue;
  const uint32_t log_rows = tp_log_rows(log_height, F);
  const uint64_t height = 1ull << log_height, tiles = height >> log_rows;
  const uint4* img = reinterpret_cast<const uint4*>(image);
  hipLaunchKernelGGL(trace_fill_public_kernel, dim3(tp_blocks(log_height, F)), dim3(kTpThreads), 0, st,
                     reinterpret_cast<uint4*>(matrix), img, width, F, log_rows, tiles);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || !n_sparse) return err;
  hipLaunchKernelGGL(trace_scatter_public_kernel, dim3((n_sparse + kTpThreads - 1) / kTpThreads),
                     dim3(kTpThreads), 0, st, reinterpret_cast<uint4*>(matrix), img + sparse_off,
                     n_sparse, width, F);
  return hipGetLastError();
}

}  // namespace mlh
