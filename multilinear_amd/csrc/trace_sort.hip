// Sorted columns on gfx950 (mlh_trace_sort): with key(i) the tuple of the
// 128-bit integers m[i][key columns] as the matrix stood at entry and pi the
// stable ascending sort permutation of the rows by key,
//   m[r][dst_s] = m[pi(r)][src_s],  m[r][perm_column] = pi(r).
//
// An LSD radix sort with 8-bit digits over (key limb, row) pairs of 8 bytes in
// two ping-pong arrays; the matrix is only read until the gather.  Every step
// is a stream-ordered launch and no workgroup waits for another one.  Digit g =
// 16 k + 4 l + b is byte b of the 32-bit limb l of key k (b and l counted from
// the least significant end).
//   0. trace_sort_census_kernel: one pass over the key columns counts every
//      digit of every key into LDS tables and adds the non-empty bins to
//      census[g][256] (zeroed on the stream before).  These counts do not depend
//      on the order of the rows, so this one pass serves every digit pass.
//      trace_sort_same_kernel: same[g] = some bin of census[g] holds all H rows;
//      the host reads same[] and drops those digits.
//   For every limb with a digit left, the last key first and limb 0 first:
//   1. trace_sort_limb_kernel: items[i] = (limb l of m[row_i][key k], row_i),
//      row_i = i before the first pass.  Then per digit b of it that is left:
//   2a. trace_sort_hist_kernel: hist[v][blk] = rows of block blk's range whose
//       digit is v (a row of the table: blocks rounded up to a multiple of 4).
//       A tile is B R consecutive rows and block blk owns the tiles [blk tpb,
//       min((blk + 1) tpb, tiles)), tpb = ceil(tiles / blocks): the range rule
//       of trace_scan.hip.
//   2b. trace_sort_offsets_kernel: one block; offsets[v][blk] = census[g][< v]
//       + hist[v][< blk]: the exclusive scan of the table in digit-major order
//       (a lane sums 4 consecutive blocks, the wave scans the lane sums).
//   2c. trace_sort_scatter_kernel: a block walks its tiles in order with its
//       256 running offsets in LDS.  In a tile wave w owns the 64 R consecutive
//       rows behind the tile's first + 64 R w and lane j takes the rows j + 64 q,
//       q < R, in order: every load of the wave is 512 contiguous bytes.  Step
//       q ranks its 64 rows: 8 ballots (one per digit bit) give a lane the set
//       of lanes with its digit; its rank among equal digits of the wave is the
//       wave's count so far (LDS, wcount[w][v]) plus the lanes below it in that
//       set, and the lowest lane of the set adds the set's size to the count.
//       After a barrier wcount[w][v] becomes the running offset plus the counts
//       of the waves before w, the running offset moves on by the tile's count,
//       and after another barrier a row goes to wcount[w][v] + rank.
//      The rank order is the row order inside a wave, between the waves of a
//      tile, between a block's tiles and between blocks: the pass is stable
//      whatever the shape, so the output is a function of the input alone.
//   3. trace_sort_gather_kernel: row r copies 16 bytes per (src, dst) pair from
//      row pi(r) = items[r].row and stores {pi(r), 0, 0, 0} in perm_column.
//      Destinations are no key and no source, so nothing it reads is written.
// All counters are 32-bit: H <= 2^28.
#include "field.hpp"
#include "trace_sort.hpp"

namespace mlh {

// bins[d] += 1 for every valid lane; one add per wave when the valid lanes
// agree (a digit that is constant over long runs: the high bytes of small
// keys).  Every branch but the last is uniform.
__device__ __forceinline__ void sort_count(uint32_t* bins, uint32_t d, bool valid) {
  const uint64_t act = __ballot(valid);
  if (!act) return;
  const uint32_t first = (uint32_t)__builtin_ctzll(act);
  const uint32_t d0 = (uint32_t)__shfl((int)d, (int)first, 64);
  const uint64_t eq = __ballot(valid && d == d0);
  if (eq == act) {
    if ((threadIdx.x & 63u) == first) atomicAdd(&bins[d0], (uint32_t)__popcll(act));
  } else if (valid) {
    atomicAdd(&bins[d], 1u);
  }
}

__global__ void __launch_bounds__(256) trace_sort_census_kernel(const SortArgs a) {
  extern __shared__ uint32_t census_bins[];  // [16 n_keys][256]
  const uint32_t B = blockDim.x, tid = threadIdx.x, W = a.width;
  const uint32_t n = a.n_keys * kSortDigitsPerKey * kSortBins;
  for (uint32_t i = tid; i < n; i += B) census_bins[i] = 0;
  __syncthreads();
  for (uint64_t r0 = (uint64_t)blockIdx.x * B; r0 < a.height; r0 += (uint64_t)gridDim.x * B) {
    const uint64_t row = r0 + tid;
    const bool valid = row < a.height;
#pragma unroll
    for (uint32_t k = 0; k < kSortMaxKeys; ++k) {
      if (k < a.n_keys) {
        fe v = fe{{0u, 0u, 0u, 0u}};
        if (valid) v = fe_load(a.m + row * W + a.key[k]);
#pragma unroll
        for (uint32_t j = 0; j < kSortDigitsPerKey; ++j)
          sort_count(census_bins + (k * kSortDigitsPerKey + j) * kSortBins,
                     (v.w[j >> 2] >> (8u * (j & 3u))) & 255u, valid);
      }
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += B) {
    const uint32_t c = census_bins[i];
    if (c) atomicAdd(a.census + i, c);
  }
}

// One block of 256 per digit.
__global__ void __launch_bounds__(256) trace_sort_same_kernel(const SortArgs a) {
  const uint32_t g = blockIdx.x;
  const int any = __syncthreads_or(a.census[g * kSortBins + threadIdx.x] == (uint32_t)a.height);
  if (threadIdx.x == 0) a.same[g] = any ? 1u : 0u;
}

__global__ void __launch_bounds__(256) trace_sort_limb_kernel(const SortArgs a, uint2* items,
                                                              uint32_t column, uint32_t limb,
                                                              uint32_t identity) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.height) return;
  const uint32_t row = identity ? (uint32_t)i : items[i].y;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a.m + (uint64_t)row * a.width + column);
  items[i] = make_uint2(p[limb], row);
}

// The rows of block b: [*begin, *end), empty for a block behind the last tile.
__device__ __forceinline__ void sort_block_range(const SortArgs& a, uint64_t* t0, uint64_t* t1) {
  *t0 = (uint64_t)blockIdx.x * a.tiles_per_block;
  *t1 = *t0 + a.tiles_per_block;
  if (*t1 > a.tiles) *t1 = a.tiles;
}

__global__ void __launch_bounds__(256) trace_sort_hist_kernel(const SortArgs a, const uint2* in,
                                                              uint32_t shift) {
  __shared__ uint32_t bins[kSortBins];
  const uint32_t B = blockDim.x, tid = threadIdx.x;
  const uint64_t T = (uint64_t)B * a.rows_per_thread;
  uint64_t t0, t1;
  sort_block_range(a, &t0, &t1);
  uint64_t end = t1 * T;
  if (end > a.height) end = a.height;
  for (uint32_t v = tid; v < kSortBins; v += B) bins[v] = 0;
  __syncthreads();
  for (uint64_t r0 = t0 * T; r0 < end; r0 += B) {  // (t1 <= t0: the first row is at or past end)
    const uint64_t i = r0 + tid;
    const bool valid = i < end;
    const uint32_t d = valid ? (in[i].x >> shift) & 255u : 0u;
    sort_count(bins, d, valid);
  }
  __syncthreads();
  for (uint32_t v = tid; v < kSortBins; v += B)
    a.hist[(uint64_t)v * sort_stride(a.blocks) + blockIdx.x] = bins[v];
}

// Inclusive sum across the wave.
__device__ __forceinline__ uint32_t sort_wave_scan(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// One block of 1024: the 256 digit starts from the census (threads 0..255),
// then wave w scans the rows v = 16 w .. 16 w + 15 of the table.  A row is
// sort_stride(blocks) counters long, a multiple of 4: a lane takes 4 consecutive
// blocks of a row with one 16-byte load (the wave 1 KiB contiguous) and one
// wave scan covers 256 blocks; the rows go kOffRows at a time with their loads
// in flight together and their scans interleaved (a wave scan is 6 dependent
// cross-lane steps: they are what this launch costs).  The counters behind
// `blocks` in a row are never written: they are loaded and not looked at.
constexpr uint32_t kOffRows = 8;

__global__ void __launch_bounds__(kSortOffsetThreads)
trace_sort_offsets_kernel(const SortArgs a, const uint32_t* __restrict__ census) {
  __shared__ uint32_t start[kSortBins];
  __shared__ uint32_t wsum[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nb = a.blocks;
  const uint32_t stride = sort_stride(nb);
  uint32_t c = 0, incl = 0;
  if (tid < kSortBins) {
    c = census[tid];
    incl = sort_wave_scan(c);
    if (lane == 63u) wsum[wave] = incl;
  }
  __syncthreads();
  if (tid < kSortBins) {
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    start[tid] = before + incl - c;
  }
  __syncthreads();
  constexpr uint32_t kWaveRows = kSortBins / (kSortOffsetThreads / 64);  // 16
  const uint32_t* __restrict__ hist = a.hist;
  uint32_t* __restrict__ offsets = a.offsets;
  for (uint32_t g = 0; g < kWaveRows; g += kOffRows) {
    const uint32_t v0 = wave * kWaveRows + g;
    uint32_t run[kOffRows];
#pragma unroll
    for (uint32_t j = 0; j < kOffRows; ++j) run[j] = start[v0 + j];
    for (uint32_t b0 = 0; b0 < nb; b0 += 256u) {
      const uint32_t b = b0 + 4u * lane;
      uint4 h[kOffRows];
      uint32_t sum[kOffRows], scan[kOffRows];
#pragma unroll
      for (uint32_t j = 0; j < kOffRows; ++j) {
        h[j] = make_uint4(0u, 0u, 0u, 0u);
        if (b < nb) h[j] = *reinterpret_cast<const uint4*>(hist + (uint64_t)(v0 + j) * stride + b);
      }
#pragma unroll
      for (uint32_t j = 0; j < kOffRows; ++j) {
        if (b + 1 >= nb) h[j].y = 0;
        if (b + 2 >= nb) h[j].z = 0;
        if (b + 3 >= nb) h[j].w = 0;
        sum[j] = scan[j] = h[j].x + h[j].y + h[j].z + h[j].w;
      }
      for (uint32_t d = 1; d < 64; d <<= 1) {  // kOffRows inclusive wave scans, step by step
#pragma unroll
        for (uint32_t j = 0; j < kOffRows; ++j) {
          const uint32_t u = (uint32_t)__shfl_up((int)scan[j], d, 64);
          if (lane >= d) scan[j] += u;
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < kOffRows; ++j) {
        const uint32_t at = run[j] + scan[j] - sum[j];
        if (b < nb)
          *reinterpret_cast<uint4*>(offsets + (uint64_t)(v0 + j) * stride + b) =
              make_uint4(at, at + h[j].x, at + h[j].x + h[j].y, at + h[j].x + h[j].y + h[j].z);
        run[j] += (uint32_t)__shfl((int)scan[j], 63, 64);
      }
    }
  }
}

template <uint32_t R>
__global__ void __launch_bounds__(256) trace_sort_scatter_kernel(const SortArgs a, const uint2* in,
                                                                 uint2* out, uint32_t shift) {
  __shared__ uint32_t wcount[4][kSortBins];
  __shared__ uint32_t running[kSortBins];
  const uint32_t B = blockDim.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t nw = B >> 6;
  const uint64_t T = (uint64_t)B * R, h = a.height;
  const uint64_t below_me = (1ull << lane) - 1ull;
  uint64_t t0, t1;
  sort_block_range(a, &t0, &t1);
  for (uint32_t v = tid; v < kSortBins; v += B)
    running[v] = a.offsets[(uint64_t)v * sort_stride(a.blocks) + blockIdx.x];
  for (uint64_t tile = t0; tile < t1; ++tile) {
    for (uint32_t i = tid; i < nw * kSortBins; i += B) (&wcount[0][0])[i] = 0;
    __syncthreads();
    const uint64_t first = tile * T + (uint64_t)wave * 64u * R + lane;
    uint2 item[R];
    uint32_t rank[R];
#pragma unroll
    for (uint32_t q = 0; q < R; ++q) {
      const uint64_t i = first + 64u * q;
      const bool valid = i < h;
      item[q] = valid ? in[i] : make_uint2(0u, 0u);
      const uint32_t d = (item[q].x >> shift) & 255u;
      uint64_t peers = __ballot(valid);
#pragma unroll
      for (uint32_t bit = 0; bit < 8; ++bit) {
        const bool set = (d >> bit) & 1u;
        const uint64_t m = __ballot(set);
        peers &= set ? m : ~m;
      }
      const uint32_t below = (uint32_t)__popcll(peers & below_me);
      const uint32_t prior = wcount[wave][d];  // every peer reads before the lowest one adds
      __builtin_amdgcn_wave_barrier();
      if (valid && below == 0) wcount[wave][d] = prior + (uint32_t)__popcll(peers);
      __builtin_amdgcn_wave_barrier();
      rank[q] = prior + below;
    }
    __syncthreads();
    for (uint32_t v = tid; v < kSortBins; v += B) {
      uint32_t run = running[v];
      for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t c = wcount[w][v];
        wcount[w][v] = run;
        run += c;
      }
      running[v] = run;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < R; ++q) {
      if (first + 64u * q < h) {
        const uint32_t d = (item[q].x >> shift) & 255u;
        out[wcount[wave][d] + rank[q]] = item[q];
      }
    }
    __syncthreads();  // the next tile zeroes wcount
  }
}

__global__ void __launch_bounds__(256) trace_sort_gather_kernel(const SortArgs a,
                                                                const uint2* items) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.height) return;
  const uint32_t W = a.width, n = a.n_copies;
  const uint32_t from = items ? items[r].y : (uint32_t)r;
  const fe* s = a.m + (uint64_t)from * W;
  fe* d = a.m + r * W;
  fe v[kSortMaxCopies];
#pragma unroll
  for (uint32_t c = 0; c < kSortMaxCopies; ++c)
    if (c < n) v[c] = fe_load(s + a.src[c]);
#pragma unroll
  for (uint32_t c = 0; c < kSortMaxCopies; ++c)
    if (c < n) fe_store(d + a.dst[c], v[c]);
  if (a.perm_column != kSortNoColumn) fe_store(d + a.perm_column, fe{{from, 0u, 0u, 0u}});
}

static bool sort_args_ok(const SortArgs& a) {
  return a.m && a.height && a.height <= (1ull << kSortMaxLogHeight) && a.width >= 1 &&
         a.n_keys >= 1 && a.n_keys <= kSortMaxKeys && a.n_copies <= kSortMaxCopies &&
         scan_shape_ok(a.threads, a.rows_per_thread, a.blocks) &&
         a.tiles == scan_tiles(a.height, a.threads, a.rows_per_thread) && a.blocks <= a.tiles &&
         a.tiles_per_block == (a.tiles + a.blocks - 1) / a.blocks && a.items[0] && a.items[1] &&
         a.census && a.same && a.hist && a.offsets;
}

hipError_t launch_sort_census(const SortArgs& a, hipStream_t st) {
  if (!sort_args_ok(a)) return hipErrorInvalidValue;
  const uint32_t digits = a.n_keys * kSortDigitsPerKey;
  const size_t bytes = (size_t)digits * kSortBins * 4;
  hipError_t e = hipMemsetAsync(a.census, 0, bytes, st);
  if (e != hipSuccess) return e;
  const uint64_t chunks = (a.height + 255) / 256;
  const uint32_t blocks = chunks < kSortCensusBlocks ? (uint32_t)chunks : kSortCensusBlocks;
  hipLaunchKernelGGL(trace_sort_census_kernel, dim3(blocks), dim3(256), bytes, st, a);
  hipLaunchKernelGGL(trace_sort_same_kernel, dim3(digits), dim3(256), 0, st, a);
  return hipGetLastError();
}

static void sort_scatter(const SortArgs& a, const uint2* in, uint2* out, uint32_t shift,
                         hipStream_t st) {
  const dim3 g(a.blocks), b(a.threads);
  switch (a.rows_per_thread) {
    case 1: hipLaunchKernelGGL(trace_sort_scatter_kernel<1>, g, b, 0, st, a, in, out, shift); break;
    case 2: hipLaunchKernelGGL(trace_sort_scatter_kernel<2>, g, b, 0, st, a, in, out, shift); break;
    case 4: hipLaunchKernelGGL(trace_sort_scatter_kernel<4>, g, b, 0, st, a, in, out, shift); break;
    case 8: hipLaunchKernelGGL(trace_sort_scatter_kernel<8>, g, b, 0, st, a, in, out, shift); break;
    default:
      hipLaunchKernelGGL(trace_sort_scatter_kernel<16>, g, b, 0, st, a, in, out, shift);
      break;
  }
}

hipError_t launch_sort_passes(const SortArgs& a, uint64_t run, hipStream_t st) {
  if (!sort_args_ok(a) || (a.n_keys < kSortMaxKeys && (run >> (kSortDigitsPerKey * a.n_keys))))
    return hipErrorInvalidValue;
  const uint32_t row_blocks = (uint32_t)((a.height + 255) / 256);
  uint32_t cur = 0;
  bool identity = true;
  for (uint32_t k = a.n_keys; k-- > 0;) {
    for (uint32_t l = 0; l < 4; ++l) {
      const uint32_t left = (uint32_t)(run >> (kSortDigitsPerKey * k + 4 * l)) & 15u;
      if (!left) continue;
      hipLaunchKernelGGL(trace_sort_limb_kernel, dim3(row_blocks), dim3(256), 0, st, a,
                         a.items[cur], (uint32_t)a.key[k], l, identity ? 1u : 0u);
      identity = false;
      for (uint32_t b = 0; b < 4; ++b) {
        if (!((left >> b) & 1u)) continue;
        const uint32_t g = kSortDigitsPerKey * k + 4 * l + b;
        hipLaunchKernelGGL(trace_sort_hist_kernel, dim3(a.blocks), dim3(a.threads), 0, st, a,
                           a.items[cur], 8u * b);
        hipLaunchKernelGGL(trace_sort_offsets_kernel, dim3(1), dim3(kSortOffsetThreads), 0, st, a,
                           a.census + (size_t)g * kSortBins);
        sort_scatter(a, a.items[cur], a.items[cur ^ 1u], 8u * b, st);
        cur ^= 1u;
      }
    }
  }
  hipLaunchKernelGGL(trace_sort_gather_kernel, dim3(row_blocks), dim3(256), 0, st, a,
                     identity ? (const uint2*)nullptr : a.items[cur]);
  return hipGetLastError();
}

}  // namespace mlh
