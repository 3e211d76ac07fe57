// Shifted columns: the kernels behind next-row constraints.
//
// trace_extend_next_kernel: T (row-major H x W) -> E (row-major H x W', W' = W
// + K) with E[i][j] = T[i][j] for j < W and E[i][W + k] = T[(i + 1) mod H][c_k].
// Threads are indexed by output element: a block takes tiles of R consecutive
// rows (R a power of two, R * W' <= 2048 elements, so a tile of E is one
// contiguous run) and lane e stores element e of the tile, lane after lane 16
// bytes on (global_store_dwordx4, coalesced).  Its source is a gather: element
// (i, j) of the tile reads T at row0 * W + i * W + off[j], off[j] = j for a
// copied column and W + c_k for a shifted one -- the same row or the one below
// -- so a tile of R rows reads R + 1 source rows, each element 1 + (uses as a
// source column) times, the repeats from L2.  The one index past the end of T,
// the row after the last tile's last row, wraps to row 0 by subtracting H * W
// (off[j] < 2 W, so one subtraction is the whole modulus).  off[] is 32 words
// of LDS written once per block; (i, j) is carried from element to element
// (one divide per lane, outside the loops); all of a lane's loads are issued
// before its first store.  A block loops over tiles t = block, block + grid,
// ...
//
// eq_rotate_kernel: out[j] = in[(j - 1) mod n], n a power of two: the delta
// table of the shift reduction, succ_rs[j] = eq_rs[j - 1].
#include "trace_shift.hpp"

namespace mlh {

constexpr uint32_t kTsPerLane = kTsTileElems / kTsThreads;  // 8

__global__ __launch_bounds__(kTsThreads) void trace_extend_next_kernel(
    const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t total_in, uint32_t width,
    uint32_t wext, ShiftCols cols, uint32_t log_rows, uint64_t tiles) {
  __shared__ uint32_t off[kTsMaxWidth];
  const uint32_t lane = threadIdx.x;
  if (lane < wext) {
    uint32_t o = lane;
    if (lane >= width) {
      const uint32_t k = lane - width, q = k >> 3;
      const uint64_t w = q == 0 ? cols.w[0] : (q == 1 ? cols.w[1] : (q == 2 ? cols.w[2] : cols.w[3]));
      o = width + (uint32_t)((w >> ((k & 7u) * 8u)) & 0xffu);
    }
    off[lane] = o;
  }
  __syncthreads();
  const uint32_t n = wext << log_rows;  // <= kTsTileElems
  // (row, column) of element `lane`, advanced by kTsThreads elements per step
  const uint32_t i0 = lane / wext, j0 = lane - i0 * wext;
  const uint32_t di = kTsThreads / wext, dj = kTsThreads - di * wext;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t row0 = t << log_rows;
    const uint64_t base = row0 * width;
    uint4* dst = out + row0 * wext;
    uint4 v[kTsPerLane];
    uint32_t i = i0, j = j0;
#pragma unroll
    for (uint32_t k = 0; k < kTsPerLane; ++k) {
      const uint32_t e = lane + k * kTsThreads;
      uint64_t s = base + (uint64_t)i * width + off[j];
      if (s >= total_in) s -= total_in;  // the row after the last one is row 0
      v[k] = e < n ? in[s] : uint4{0, 0, 0, 0};
      i += di;
      j += dj;
      if (j >= wext) {
        j -= wext;
        ++i;
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < kTsPerLane; ++k) {
      const uint32_t e = lane + k * kTsThreads;
      if (e < n) dst[e] = v[k];
    }
  }
}

__global__ __launch_bounds__(kTsThreads) void eq_rotate_kernel(const uint4* __restrict__ in,
                                                               uint4* __restrict__ out, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * kTsThreads;
  for (uint64_t j = (uint64_t)blockIdx.x * kTsThreads + threadIdx.x; j < n; j += stride)
    out[j] = in[(j + n - 1) & (n - 1)];
}

hipError_t launch_trace_extend_next(const fe* in, fe* out, uint32_t log_height, uint32_t width,
                                    const uint32_t* cols, uint32_t n_shifts, hipStream_t st) {
  const uint32_t wext = width + n_shifts;
  if (width < 1 || wext > kTsMaxWidth || log_height > 32 || (n_shifts && !cols))
    return hipErrorInvalidValue;
  ShiftCols sc = {{0, 0, 0, 0}};
  for (uint32_t k = 0; k < n_shifts; ++k) {
    if (cols[k] >= width) return hipErrorInvalidValue;
    sc.w[k >> 3] |= (uint64_t)cols[k] << ((k & 7u) * 8u);
  }
  const uint32_t log_rows = ts_log_rows(log_height, wext);
  const uint64_t height = 1ull << log_height, tiles = height >> log_rows;
  const dim3 grid(ts_blocks(log_height, wext)), block(kTsThreads);
  hipLaunchKernelGGL(trace_extend_next_kernel, grid, block, 0, st,
                     reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out),
                     height * width, width, wext, sc, log_rows, tiles);
  return hipGetLastError();
}

hipError_t launch_eq_rotate(const fe* in, fe* out, uint32_t log_n, hipStream_t st) {
  if (log_n > 32) return hipErrorInvalidValue;
  const uint64_t n = 1ull << log_n;
  uint64_t blocks = (n + kTsThreads - 1) / kTsThreads;
  if (blocks > kTsMaxBlocks) blocks = kTsMaxBlocks;
  hipLaunchKernelGGL(eq_rotate_kernel, dim3((uint32_t)blocks), dim3(kTsThreads), 0, st,
                     reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out), n);
  return hipGetLastError();
}

}  // namespace mlh
