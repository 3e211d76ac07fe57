// Witness check on gfx950 (mlh_trace_check): the constraints of a
// program on every row of the row-major trace T (H x W), with the next-row
// operands of a shifted system read by address (constraints.rs:3-10: an Expr
// is a function of the row; evaluation.rs:21-29 without the mask).
//
// The program is W + K wide.  On row i its column operand j < W is T[i][j] and
// operand W + k is T[(i + 1) mod H][c_k]; no extension is materialised.  The
// interpreter is the sumcheck's (cs_interp.hpp): decode is wave-uniform, a
// lane's register file lives in LDS as [slot][lane],
//   slots [0, W)              the row's columns
//   slots [W, W + K)          the next row's source columns
//   slots [W + K, W + K + T)  the program's temps
// and there are no step slots and no sums.
//
// A block works on chunks of B = blockDim.x consecutive rows.  The chunk's
// nrows * W elements are contiguous in T, so the block loads them coalesced
// (thread e mod B takes element e, CsWalk) and scatters them into slots [0,
// W).  After the barrier lane r fills slot W + k from lane r + 1's slot c_k --
// the slots below W are not written again until the next chunk, so this
// needs no second barrier -- and the chunk's last valid lane reads its K
// elements of row (base + nrows) mod H from global memory: that one read is
// where the cyclic wrap and the chunk and block seams live.  Then the program
// runs once on the lane's row.
//
// Verdicts are integers: for constraint c the lane's bit is valid && out_c !=
// 0 (the interpreter's results are canonical, so zero is the four zero limbs).
// A wave reduces it with a 64-bit ballot and a popcount, and its lane 0
// updates the block's LDS counters: a 32-bit count per chunk, widened into a
// 64-bit block total after the chunk's second barrier by the thread that owns
// the constraint, and the lowest failing row.  At its end the block flushes
// the counters that are not zero with 64-bit atomicAdd / atomicMin.  Only
// integer adds and mins cross lanes, so the result does not depend on the
// launch shape or the order of the atomics.  No workgroup waits for another
// and every loop is bounded.
#include "trace_check.hpp"

#include "cs_interp.hpp"

namespace mlh {

using u64 = unsigned long long;

__global__ void __launch_bounds__(256)
trace_check_kernel(const CsDev P, const fe* __restrict__ m, uint64_t H, uint32_t W, uint32_t K,
                   ShiftCols cols, u64* __restrict__ counters) {
  extern __shared__ fe tk_lds[];
  __shared__ uint32_t src[kCsMaxWidth];
  __shared__ uint32_t chunk_count[kCsMaxConstraints + 1];  // [NC]: rows with any failure
  __shared__ u64 total[kCsMaxConstraints + 1], first[kCsMaxConstraints];
  const uint32_t B = blockDim.x, tid = threadIdx.x, NC = P.n_constraints;
  if (tid < K) {
    const uint32_t q = tid >> 3;
    const uint64_t w = q == 0 ? cols.w[0] : (q == 1 ? cols.w[1] : (q == 2 ? cols.w[2] : cols.w[3]));
    src[tid] = (uint32_t)((w >> ((tid & 7u) * 8u)) & 0xffu);
  }
  for (uint32_t c = tid; c <= NC; c += B) {
    chunk_count[c] = 0;
    total[c] = 0;
    if (c < NC) first[c] = ~0ull;
  }
  // (the first chunk's barrier publishes them: the grid has no more blocks than chunks)
  fe* lane_lds = tk_lds + tid;
  const uint32_t wave_row = tid & ~63u;
  const bool leader = (tid & 63u) == 0;
  for (uint64_t base = (uint64_t)blockIdx.x * B; base < H; base += (uint64_t)gridDim.x * B) {
    const uint32_t nrows = H - base < B ? (uint32_t)(H - base) : B;
    const fe* row0 = m + base * W;
    CsWalk w(tid, B, W);
    for (uint32_t e = tid; e < nrows * W; e += B, w.next()) tk_lds[w.col * B + w.row] = fe_load(row0 + e);
    __syncthreads();
    const bool valid = tid < nrows;
    if (valid) {
      if (tid + 1 < nrows) {
        for (uint32_t k = 0; k < K; ++k) lane_lds[(W + k) * B] = tk_lds[src[k] * B + tid + 1];
      } else {  // the seam: the row behind the chunk, row 0 behind the last one
        uint64_t nx = base + nrows;
        if (nx >= H) nx -= H;
        for (uint32_t k = 0; k < K; ++k) lane_lds[(W + k) * B] = fe_load(m + nx * W + src[k]);
      }
    }
    for (uint32_t pc = 0; pc < P.n_instr; ++pc) cs_step(P, lane_lds, B, pc);
    bool any = false;
    for (uint32_t c = 0; c < NC; ++c) {
      const fe out = cs_fetch(P.outs[c] & 0xFFFFu, P.uni, lane_lds, B);
      const bool bad = valid && !fe_eq(out, fe_zero());
      any |= bad;
      const uint64_t b = __builtin_amdgcn_ballot_w64(bad);
      if (b && leader) {
        atomicAdd(&chunk_count[c], (uint32_t)__popcll(b));
        atomicMin(&first[c], (u64)(base + wave_row + (uint32_t)__builtin_ctzll(b)));
      }
    }
    const uint64_t ba = __builtin_amdgcn_ballot_w64(any);
    if (ba && leader) atomicAdd(&chunk_count[NC], (uint32_t)__popcll(ba));
    __syncthreads();  // the next chunk's loads overwrite other lanes' slots
    for (uint32_t c = tid; c <= NC; c += B) {  // (read again only behind the next chunk's barrier)
      total[c] += chunk_count[c];
      chunk_count[c] = 0;
    }
  }
  // total[c] is this thread's own; first[c] was last written before the barrier above
  for (uint32_t c = tid; c <= NC; c += B) {
    if (total[c]) atomicAdd(counters + c, total[c]);
    if (c < NC && first[c] != ~0ull) atomicMin(counters + NC + 1 + c, first[c]);
  }
}

hipError_t launch_trace_check(const CsDev& P, const fe* m, uint32_t log_height, uint32_t width,
                              const uint32_t* cols, uint32_t n_shifts, uint64_t* counters,
                              uint32_t threads, uint32_t blocks, hipStream_t st) {
  const uint32_t slots = P.width + P.n_temps;
  if (!m || !counters || width < 1 || width + n_shifts != P.width || P.width > kCsMaxWidth ||
      P.n_constraints < 1 || P.n_constraints > kCsMaxConstraints || log_height > kCsMaxLogHeight ||
      !tk_shape_ok(slots, threads, kTkMaxBlocks) || blocks < 1 || blocks > kTkMaxBlocks ||
      (n_shifts && !cols))
    return hipErrorInvalidValue;
  const uint64_t H = 1ull << log_height;
  if (blocks > (H + threads - 1) / threads) return hipErrorInvalidValue;
  ShiftCols sc = {{0, 0, 0, 0}};
  for (uint32_t k = 0; k < n_shifts; ++k) {
    if (cols[k] >= width) return hipErrorInvalidValue;
    sc.w[k >> 3] |= (uint64_t)cols[k] << ((k & 7u) * 8u);
  }
  hipLaunchKernelGGL(trace_check_kernel, dim3(blocks), dim3(threads), (size_t)slots * threads * sizeof(fe),
                     st, P, m, H, width, n_shifts, sc, reinterpret_cast<u64*>(counters));
  return hipGetLastError();
}

}  // namespace mlh
