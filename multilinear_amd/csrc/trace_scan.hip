// Running-sum and running-product columns on gfx950 (mlh_trace_scan): for scan
// s with t[i] = m[i][src_s] as the matrix stood at entry and o = + or * in the
// field,
//   z[0] = init_s,  z[i + 1] = z[i] o t[i],  m[i][dst_s] = z[i],  total_s = z[H]:
// the exclusive scan, the column that first (z - init) and next(z) - z o t
// constrain.
//
// Reduce-then-scan in three stream-ordered launches; no workgroup waits for
// another one.  A tile is B R consecutive rows (B threads, R rows per thread);
// block b owns the tiles [b tpb, min((b + 1) tpb, tiles)), tpb = ceil(tiles /
// blocks): the last blocks own fewer tiles or none.
//   1. trace_scan_reduce_kernel: aggregates[s][b] = the o-aggregate of t over
//      block b's rows (the identity for an empty range).  Both operations are
//      commutative, so the lanes take the rows striped (row = first + k B +
//      tid: for a fixed k the B elements are W * 16 bytes apart).
//   2. trace_scan_offsets_kernel: one block; per scan the exclusive scan of the
//      at most 1024 aggregates seeded with init_s -> offsets[s][b], totals[s].
//   3. trace_scan_apply_kernel: per tile, thread tid owns the rows first + tid R
//      + r, r < R.  Pass 1 loads every scan's source in those rows and folds
//      them into the lane totals; these are scanned across the wave
//      (__shfl_up), the wave totals across the block through LDS, behind the
//      carry of the block's earlier tiles (LDS, seeded with offsets[s][b]).
//      Pass 2 walks the rows again: a row's sources of all scans are loaded
//      (from L2: pass 1 just read them) before its destinations are stored and
//      the running values move on.
// With one block, launch 3 runs alone: the carry starts at init_s and the block
// writes totals[s] (`single`).
//
// Snapshot semantics (a destination may be any scan's source): launch 1 ends
// before launch 3 begins, a row is read and written in launch 3 by one thread
// only, that thread has finished pass 1 over the tile before it stores, and in
// pass 2 it loads a row's sources before it stores that row's destinations.
// So the whole tile's sources are loaded before any of its destinations is
// stored, and pass 2's second look sees the values of entry.
//
// Every index into the per-scan arrays (ScanArgs and the lanes' own) is a
// compile-time constant: launches 1 and 3 are built for up to N = 1, 2, 4 and 8
// scans (the least N that holds n_scans runs), their scan loops unrolled N
// times under a uniform s < n_scans; the row loops stay rolled.  A lane of
// launch 3 holds N running values and N sources of a row, 8 N registers, beside
// a product's temporaries: one kernel for 8 scans would run every call at the
// 2 waves per SIMD of the widest (registers: DESIGN.md 6k).  Launch 2 takes a
// scan after the other.  The operation of a scan is uniform: a scalar branch
// between fe_add and fe_mul.
#include "field.hpp"
#include "trace_scan.hpp"

namespace mlh {

constexpr uint32_t kScanOffsetThreads = 256, kScanOffsetElems = kScanMaxBlocks / kScanOffsetThreads;

__device__ __forceinline__ fe scan_identity(uint32_t op) { return fe{{op, 0u, 0u, 0u}}; }
__device__ __forceinline__ fe scan_combine(uint32_t op, const fe& a, const fe& b) {
  return op == kScanMul ? fe_mul(a, b) : fe_add(a, b);
}
__device__ __forceinline__ fe scan_shfl_up(const fe& x, uint32_t d) {
  fe r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.w[i] = __shfl_up(x.w[i], d, 64);
  return r;
}

// Inclusive scan of v across the wave; lane 63 holds the wave's aggregate.
__device__ __forceinline__ fe scan_wave(uint32_t op, fe v) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const fe u = scan_shfl_up(v, d);
    v = scan_combine(op, lane >= d ? u : scan_identity(op), v);
  }
  return v;
}

// Block scan, first half: the aggregate of the earlier lanes of this wave;
// lane 63 leaves the wave's aggregate in waves[wave].
__device__ __forceinline__ fe scan_lanes_before(uint32_t op, const fe& v, fe* waves) {
  const uint32_t lane = threadIdx.x & 63u;
  const fe incl = scan_wave(op, v);
  if (lane == 63u) waves[threadIdx.x >> 6] = incl;
  const fe up = scan_shfl_up(incl, 1);
  return lane ? up : scan_identity(op);
}
// Second half, behind a barrier: carry o the earlier waves' aggregates;
// *all = carry o every wave's aggregate (the same in every thread).
__device__ __forceinline__ fe scan_waves_before(uint32_t op, const fe& carry, const fe* waves,
                                                fe* all) {
  const uint32_t wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  fe run = carry, mine = carry;
  for (uint32_t w = 0; w < nw; ++w) {
    if (w == wave) mine = run;
    run = scan_combine(op, run, waves[w]);
  }
  *all = run;
  return mine;
}

// The per-scan loops of the kernels built for up to N scans: unrolled, so that
// s is a constant in every index.
#define SCAN_FOR_EACH(s) _Pragma("unroll") for (uint32_t s = 0; s < N; ++s)

template <uint32_t N>
__global__ void __launch_bounds__(256) trace_scan_reduce_kernel(const ScanArgs a) {
  __shared__ fe waves[N][4];
  const uint32_t B = blockDim.x, tid = threadIdx.x, W = a.width, n = a.n_scans;
  const uint64_t T = (uint64_t)B * a.rows_per_thread;
  const uint64_t t0 = (uint64_t)blockIdx.x * a.tiles_per_block;
  uint64_t t1 = t0 + a.tiles_per_block;
  if (t1 > a.tiles) t1 = a.tiles;
  uint64_t end = t1 * T;  // (t1 <= t0, an empty range: the first row is at or past end)
  if (end > a.height) end = a.height;
  fe acc[N];
  SCAN_FOR_EACH(s) acc[s] = scan_identity(a.op[s]);
  for (uint64_t row = t0 * T + tid; row < end; row += B) {
    const fe* p = a.m + row * W;
    fe t[N];
    SCAN_FOR_EACH(s) if (s < n) t[s] = fe_load(p + a.src[s]);
    SCAN_FOR_EACH(s) if (s < n) acc[s] = scan_combine(a.op[s], acc[s], t[s]);
  }
  SCAN_FOR_EACH(s) if (s < n) {
    const fe incl = scan_wave(a.op[s], acc[s]);
    if ((tid & 63u) == 63u) waves[s][tid >> 6] = incl;
  }
  __syncthreads();
  if (tid == 0) {
    SCAN_FOR_EACH(s) if (s < n) {
      fe all;
      (void)scan_waves_before(a.op[s], scan_identity(a.op[s]), waves[s], &all);
      fe_store(a.aggregates + (uint64_t)s * a.blocks + blockIdx.x, all);
    }
  }
}

// One block of kScanOffsetThreads, a scan after the other; thread t takes the
// aggregates 4 t .. 4 t + 3 (the wave aggregates by the scan's parity: one
// barrier per scan).
__global__ void __launch_bounds__(kScanOffsetThreads) trace_scan_offsets_kernel(const ScanArgs a) {
  __shared__ fe waves[2][4];
  const uint32_t tid = threadIdx.x, nb = a.blocks;
  const uint32_t i0 = tid * kScanOffsetElems;
  for (uint32_t s = 0; s < a.n_scans; ++s) {
    const uint32_t op = a.op[s];
    const fe* agg = a.aggregates + (uint64_t)s * nb;
    fe t[kScanOffsetElems], acc = scan_identity(op);
#pragma unroll
    for (uint32_t j = 0; j < kScanOffsetElems; ++j) {
      t[j] = i0 + j < nb ? fe_load(agg + i0 + j) : scan_identity(op);
      acc = scan_combine(op, acc, t[j]);
    }
    const fe before = scan_lanes_before(op, acc, waves[s & 1u]);
    __syncthreads();
    fe all;
    fe z = scan_combine(op, scan_waves_before(op, a.init[s], waves[s & 1u], &all), before);
#pragma unroll
    for (uint32_t j = 0; j < kScanOffsetElems; ++j) {
      if (i0 + j < nb) fe_store(a.offsets + (uint64_t)s * nb + i0 + j, z);
      z = scan_combine(op, z, t[j]);
    }
    if (tid == 0) fe_store(a.totals + s, all);
  }
}

template <uint32_t N>
__global__ void __launch_bounds__(256) trace_scan_apply_kernel(const ScanArgs a, uint32_t single) {
  // both by the tile's parity: a tile's one barrier orders them against the
  // tile before and the tile after
  __shared__ fe waves[2][N][4];
  __shared__ fe carry[2][N];
  const uint32_t B = blockDim.x, tid = threadIdx.x, W = a.width, n = a.n_scans;
  const uint32_t R = a.rows_per_thread;
  const uint64_t T = (uint64_t)B * R, h = a.height;
  const uint64_t t0 = (uint64_t)blockIdx.x * a.tiles_per_block;
  uint64_t t1 = t0 + a.tiles_per_block;
  if (t1 > a.tiles) t1 = a.tiles;
  if (tid == 0) {
    SCAN_FOR_EACH(s) if (s < n)
      carry[0][s] = single ? a.init[s] : fe_load(a.offsets + (uint64_t)s * a.blocks + blockIdx.x);
  }
  uint32_t par = 0;
  for (uint64_t tile = t0; tile < t1; ++tile, par ^= 1u) {
    const uint64_t row0 = tile * T + (uint64_t)tid * R;
    fe z[N];
    SCAN_FOR_EACH(s) z[s] = scan_identity(a.op[s]);
    for (uint32_t r = 0; r < R; ++r) {  // pass 1: the lane's aggregates
      if (row0 + r >= h) break;
      const fe* p = a.m + (row0 + r) * W;
      fe t[N];
      SCAN_FOR_EACH(s) if (s < n) t[s] = fe_load(p + a.src[s]);
      SCAN_FOR_EACH(s) if (s < n) z[s] = scan_combine(a.op[s], z[s], t[s]);
    }
    SCAN_FOR_EACH(s) if (s < n) z[s] = scan_lanes_before(a.op[s], z[s], waves[par][s]);
    __syncthreads();
    SCAN_FOR_EACH(s) if (s < n) {  // z[s]: the scan's value at this lane's first row
      fe all;
      const fe w = scan_waves_before(a.op[s], carry[par][s], waves[par][s], &all);
      z[s] = scan_combine(a.op[s], w, z[s]);
      if (tid == 0) carry[par ^ 1u][s] = all;
    }
    for (uint32_t r = 0; r < R; ++r) {  // pass 2: a row's sources, then its destinations
      if (row0 + r >= h) break;
      fe* p = a.m + (row0 + r) * W;
      fe t[N];
      SCAN_FOR_EACH(s) if (s < n) t[s] = fe_load(p + a.src[s]);
      SCAN_FOR_EACH(s) if (s < n) {
        fe_store(p + a.dst[s], z[s]);
        z[s] = scan_combine(a.op[s], z[s], t[s]);
      }
    }
  }
  if (single && tid == 0) {  // (thread 0 wrote the last tile's carry itself)
    SCAN_FOR_EACH(s) if (s < n) fe_store(a.totals + s, carry[par][s]);
  }
}

template <uint32_t N>
static void scan_launch(const ScanArgs& a, uint32_t threads, uint32_t single, hipStream_t st) {
  if (!single) {
    hipLaunchKernelGGL(trace_scan_reduce_kernel<N>, dim3(a.blocks), dim3(threads), 0, st, a);
    hipLaunchKernelGGL(trace_scan_offsets_kernel, dim3(1), dim3(kScanOffsetThreads), 0, st, a);
  }
  hipLaunchKernelGGL(trace_scan_apply_kernel<N>, dim3(a.blocks), dim3(threads), 0, st, a, single);
}

hipError_t launch_trace_scan(const ScanArgs& a, uint32_t threads, hipStream_t st) {
  if (!a.m || !a.height || a.width < 1 || a.n_scans < 1 || a.n_scans > kScanMaxScans ||
      !scan_shape_ok(threads, a.rows_per_thread, a.blocks) ||
      a.tiles != scan_tiles(a.height, threads, a.rows_per_thread) || a.blocks > a.tiles ||
      a.tiles_per_block != (a.tiles + a.blocks - 1) / a.blocks || !a.aggregates || !a.offsets ||
      !a.totals)
    return hipErrorInvalidValue;
  const uint32_t single = a.blocks == 1;
  // the kernels built for the least of 1, 2, 4, 8 scans that holds n_scans
  if (a.n_scans == 1)
    scan_launch<1>(a, threads, single, st);
  else if (a.n_scans == 2)
    scan_launch<2>(a, threads, single, st);
  else if (a.n_scans <= 4)
    scan_launch<4>(a, threads, single, st);
  else
    scan_launch<8>(a, threads, single, st);
  return hipGetLastError();
}

}  // namespace mlh
