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
      const uint64_t row = row0 + i;
      const uint4 p = img[d.z + ((uint32_t)row & d.y)];
      const uint32_t flag = (uint32_t)((d.x == kPcFirst && i == i_first) | (d.x == kPcLast && i == i_last));
      const bool is_row = d.x == kPcRow;
      v[k] = uint4{is_row ? (uint32_t)row : (p.x | flag), is_row ? (uint32_t)(row >> 32) : p.y, p.z,
                   p.w};
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
