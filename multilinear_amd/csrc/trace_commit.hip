// Trace commitment kernel: the row-major 2^L x W trace as W column MLEs
// (column-major), the input of the batched PCS commit that stands for
// Commitment::new (constraint_system/trace.rs:40-48).
//
// trace_columns_kernel: a block takes tiles of R consecutive rows (R a power
// of two, R * W <= 2048 elements; a table shorter than R is one short tile).
// A tile's rows * W elements are contiguous in the trace: lane e loads element
// e of the tile (global_load_dwordx4, coalesced), at most 8 loads per lane all
// issued before the first use, and stores it to the LDS slot j * pitch + i of
// its (row i, column j) (ds_write_b128; pitch: trace_commit.hpp).  After a
// barrier lane e reads slot (e / rows) * pitch + (e mod rows) -- consecutive
// lanes read consecutive slots of one column -- and stores it to
// out[j * H + row0 + i]: every column's run of `rows` elements is written as
// contiguous 16-byte stores.  A block loops over tiles t = block, block +
// grid, ...
#include "trace_commit.hpp"

namespace mlh {

constexpr uint32_t kTcPerLane = kTcTileElems / kTcThreads;  // 8

// One body for both kernels.  RANGE = false: the tile is contiguous, ncols =
// width and lane e loads src[e].  RANGE = true: the range kernel's strided load
// (below).  From the LDS store on the two are the same code.
template <bool RANGE>
__device__ __forceinline__ void trace_columns_body(const uint4* __restrict__ in,
                                                   uint4* __restrict__ out, uint64_t height,
                                                   uint32_t width, uint32_t col0, uint32_t ncols,
                                                   uint32_t log_rows, uint32_t pitch,
                                                   uint64_t tiles) {
  extern __shared__ uint4 tc_lds[];
  const uint32_t rows = 1u << log_rows, n = rows * ncols;  // n <= kTcTileElems
  const uint32_t lane = threadIdx.x;
  // (row, column) of element `lane`, advanced by kTcThreads elements per step
  const uint32_t i0 = lane / ncols, j0 = lane - i0 * ncols;
  const uint32_t di = kTcThreads / ncols, dj = kTcThreads - di * ncols;
  const auto step = [&](uint32_t& i, uint32_t& j) {
    i += di;
    j += dj;
    if (j >= ncols) {
      j -= ncols;
      ++i;
    }
  };
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t row0 = t << log_rows;
    const uint4* src = in + row0 * width + col0;
    uint4 v[kTcPerLane];
    uint32_t i = i0, j = j0;
#pragma unroll
    for (uint32_t k = 0; k < kTcPerLane; ++k) {
      const uint32_t e = lane + k * kTcThreads;
      v[k] = e < n ? src[RANGE ? (uint64_t)i * width + j : e] : uint4{0, 0, 0, 0};
      if (RANGE) step(i, j);
    }
    i = i0;
    j = j0;
#pragma unroll
    for (uint32_t k = 0; k < kTcPerLane; ++k) {
      const uint32_t e = lane + k * kTcThreads;
      if (e < n) tc_lds[j * pitch + i] = v[k];
      step(i, j);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kTcPerLane; ++k) {
      const uint32_t e = lane + k * kTcThreads;
      if (e < n) {
        const uint32_t c = e >> log_rows, r = e & (rows - 1);
        out[(uint64_t)c * height + row0 + r] = tc_lds[c * pitch + r];
      }
    }
    __syncthreads();  // the next tile's stores reuse the slots
  }
}

__global__ __launch_bounds__(kTcThreads) void trace_columns_kernel(
    const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t height, uint32_t width,
    uint32_t log_rows, uint32_t pitch, uint64_t tiles) {
  trace_columns_body<false>(in, out, height, width, 0, width, log_rows, pitch, tiles);
}

// trace_columns_range_kernel: the same for columns [col0, col0 + ncols) only.
// A tile is rows x ncols; its elements are no longer contiguous but ncols * 16
// byte runs at a stride of width * 16 bytes.  Lane e still takes element e of
// the tile in (row, column) order, (i, j) = (e / ncols, e mod ncols), now at
// in[(row0 + i) * width + col0 + j]: consecutive lanes read consecutive 16
// bytes within a run and step to the next row's run after ncols lanes.  (i, j)
// is carried from load to load (one divide per lane, outside the loops); all
// of a lane's loads are issued before the first LDS store.  From the LDS store
// on, the kernel sees a rows x ncols tile and nothing of `width`: slots, pitch
// (tc_pitch(ncols, R)) and the column read-out are trace_columns_kernel's with
// ncols for the width.  No element outside the range is read.
__global__ __launch_bounds__(kTcThreads) void trace_columns_range_kernel(
    const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t height, uint32_t width,
    uint32_t col0, uint32_t ncols, uint32_t log_rows, uint32_t pitch, uint64_t tiles) {
  trace_columns_body<true>(in, out, height, width, col0, ncols, log_rows, pitch, tiles);
}

// Columns [col0, col0 + ncols): the whole width is one contiguous tile per
// block (trace_columns_kernel), anything less the strided range kernel.
hipError_t launch_trace_columns(const fe* in, fe* out, uint32_t log_height, uint32_t width,
                                uint32_t col0, uint32_t ncols, hipStream_t st) {
  if (ncols == 0 || col0 >= width || ncols > width - col0) return hipErrorInvalidValue;
  const uint64_t height = 1ull << log_height;
  const uint32_t R = tc_tile_rows(ncols);
  uint32_t log_rows = 0;
  while ((2ull << log_rows) <= (height < R ? height : R)) ++log_rows;  // rows = min(R, height)
  const uint64_t tiles = height >> log_rows;
  const uint32_t pitch = tc_pitch(ncols, R);
  const dim3 grid(tc_blocks(height, ncols)), block(kTcThreads);
  const size_t lds = (size_t)ncols * pitch * sizeof(uint4);
  const uint4* src = reinterpret_cast<const uint4*>(in);
  uint4* dst = reinterpret_cast<uint4*>(out);
  if (ncols == width)
    hipLaunchKernelGGL(trace_columns_kernel, grid, block, lds, st, src, dst, height, width, log_rows,
                       pitch, tiles);
  else
    hipLaunchKernelGGL(trace_columns_range_kernel, grid, block, lds, st, src, dst, height, width,
                       col0, ncols, log_rows, pitch, tiles);
  return hipGetLastError();
}

}  // namespace mlh
