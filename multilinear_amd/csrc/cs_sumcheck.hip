// Constraint-system sumcheck on gfx950: width-W traces and a programmable
// composition (constraint_system/sumcheck.rs:147-247, evaluation.rs:21-29).
//
// The composition is a straight-line program (cs_program.hpp) that every lane
// interprets on its own row: decode is wave-uniform (the instruction words and
// the uniform pool are read through uniform addresses), the operands are
// per-lane.  Runtime-indexed per-thread arrays would go to scratch, so a lane's
// whole register file of the interpreter lives in LDS as [slot][lane] (16-byte
// elements, lane-contiguous: one ds_read_b128 / ds_write_b128 per access):
//   slots [0, W)            column values at the current X
//   slots [W, W + T)        the program's temps
//   slots [W + T, 2W + T)   the per-column step hi - lo
//   slots [2W + T, .. + D)  the D running sums
// For the row pair (i, i + h) the values at X = t are lo + t (hi - lo), formed
// incrementally from X = 1 (= hi) by adding the step once per point: the same
// field values as the reference's (1 - X) lo + X hi (partial_sum, :204-232;
// its X == 1 shortcut included), hence the same canonical outputs.
//
// A block works on chunks of blockDim.x consecutive row pairs.  The chunk's
// W * blockDim.x matrix elements are contiguous in the row-major trace, so the
// block loads them coalesced (thread e mod blockDim.x takes element e) and
// scatters them into the [column][row] LDS slots; after a barrier lane r
// interprets row r.  cs_fold_sums does the same from the four quarter rows of
// a height-4q table: it folds them with r, writes the folded half back in
// place (each element is read and written by one thread only) and leaves the
// folded pair (new[i], new[i + q]) in LDS for the next round's sums.
//
// Sum columns (template flag SUMS; the claim sum_i [delta_i composition(row_i)
// + beta sum_{j in S} row_i[j]]): the linear part of the round polynomial at
// X = t is A + (t - 1) B with A = sum_rows sum_{j in S} hi and B = sum_rows
// sum_{j in S} (hi - lo), both read from the slots the chunk's loads filled
// (values at X = 1 and steps) before the interpreter advances them.  A lane
// keeps its A and B in registers; the block reduces them into lin[block] and
// lin[gridDim.x + block], and cs_round_lin_kernel adds beta (A + (t - 1) B)
// to evals[t].  SUMS = false is the code without any of it.
#include "bfly_asm.hpp"
#include "cs_interp.hpp"
#include "cs_program.hpp"
#include "cs_sumcheck.hpp"
#include "field.hpp"
#include "sc_dev.hpp"
#include "transcript_dev.hpp"

namespace mlh {

constexpr uint32_t kCsMaxD = kCsMaxDegree + 1;

// (CsWalk, cs_fetch and the interpreter's step cs_step: cs_interp.hpp, shared with
// trace_check.hip)

// The D sums of one chunk: lane_lds = this lane's column of the LDS slots
// (filled with the values at X = 1 and the steps), dc / dd = delta at X = 1
// and its step (zero on a lane without a row).
__device__ __forceinline__ void cs_accumulate(const CsDev& P, fe* lane_lds, uint32_t B, bool valid,
                                              fe dc, const fe& dd) {
  const uint32_t W = P.width, step0 = W + P.n_temps, acc0 = step0 + W;
  for (uint32_t t = 0; t < P.D; ++t) {
    for (uint32_t pc = 0; pc < P.n_instr; ++pc) cs_step(P, lane_lds, B, pc);
    fe c = fe_zero();  // sum_c mask[c] * out_c (evaluation.rs:21-29)
    for (uint32_t k = 0; k < P.n_constraints; ++k) {
      const uint32_t o = P.outs[k];
      c = fe_add(c, fe_mul_s(cs_fetch(o & 0xFFFFu, P.uni, lane_lds, B), fe_vgpr(P.uni[o >> 16])));
    }
    if (valid) {
      fe* acc = lane_lds + (acc0 + t) * B;
      *acc = fe_add(*acc, fe_mul_s(c, dc));
    }
    if (t + 1 < P.D) {  // X -> X + 1
      for (uint32_t j = 0; j < W; ++j) lane_lds[j * B] = fe_add(lane_lds[j * B], lane_lds[(step0 + j) * B]);
      dc = fe_add(dc, dd);
    }
  }
}

// This lane's row of the sum columns (smask: bit j = column j), before
// cs_accumulate advances the slots: la += sum hi, lb += sum (hi - lo).
__device__ __forceinline__ void cs_linear(const CsDev& P, const fe* lane_lds, uint32_t B,
                                          uint32_t smask, fe& la, fe& lb) {
  const uint32_t step0 = P.width + P.n_temps;
  for (uint32_t j = 0; j < P.width; ++j)
    if ((smask >> j) & 1u) {
      la = fe_add(la, lane_lds[j * B]);
      lb = fe_add(lb, lane_lds[(step0 + j) * B]);
    }
}

// (cs_block_sum: sc_dev.hpp)

__device__ __forceinline__ void cs_zero_sums(const CsDev& P, fe* lane_lds, uint32_t B) {
  const uint32_t acc0 = 2 * P.width + P.n_temps;
  for (uint32_t t = 0; t < P.D; ++t) lane_lds[(acc0 + t) * B] = fe_zero();
}

// The end of both bodies: partials[t * gridDim.x + block] = the block's sum t; SUMS: its A and
// B into lin[block] and lin[gridDim.x + block], reduced in the caller's lred (4 elements of LDS).
template <bool SUMS>
__device__ __forceinline__ void cs_write_sums(const CsDev& P, const fe* lane_lds, uint32_t B,
                                              fe* __restrict__ partials, const fe& la, const fe& lb,
                                              fe* lred, fe* __restrict__ lin) {
  __shared__ fe red[4];
  const uint32_t acc0 = 2 * P.width + P.n_temps;
  for (uint32_t t = 0; t < P.D; ++t)
    cs_block_sum(lane_lds[(acc0 + t) * B], B, red, partials + (uint64_t)t * gridDim.x + blockIdx.x);
  if (SUMS) {
    cs_block_sum(la, B, lred, lin + blockIdx.x);
    cs_block_sum(lb, B, lred, lin + gridDim.x + blockIdx.x);
  }
}

template <bool SUMS>
__device__ __forceinline__ void cs_sums_body(const CsDev& P, const fe* __restrict__ m,
                                             const fe* __restrict__ d, uint64_t h,
                                             fe* __restrict__ partials, uint32_t smask,
                                             fe* __restrict__ lin) {
  extern __shared__ fe cs_lds[];
  const uint32_t B = blockDim.x, tid = threadIdx.x, W = P.width, step0 = W + P.n_temps;
  fe* lane_lds = cs_lds + tid;
  fe la = fe_zero(), lb = fe_zero();
  cs_zero_sums(P, lane_lds, B);
  for (uint64_t base = (uint64_t)blockIdx.x * B; base < h; base += (uint64_t)gridDim.x * B) {
    const uint32_t nrows = h - base < B ? (uint32_t)(h - base) : B;
    const fe* lo = m + base * W;
    const fe* hi = lo + h * W;
    CsWalk w(tid, B, W);
    for (uint32_t e = tid; e < nrows * W; e += B, w.next()) {
      const fe x1 = fe_load(hi + e), x0 = fe_load(lo + e);
      cs_lds[w.col * B + w.row] = x1;
      cs_lds[(step0 + w.col) * B + w.row] = fe_sub(x1, x0);
    }
    const bool valid = tid < nrows;
    fe dc = fe_zero(), dd = fe_zero();
    if (valid) {
      dc = fe_load(d + base + tid + h);
      dd = fe_sub(dc, fe_load(d + base + tid));
    }
    __syncthreads();
    if (SUMS && valid) cs_linear(P, lane_lds, B, smask, la, lb);
    cs_accumulate(P, lane_lds, B, valid, dc, dd);
    __syncthreads();  // the next chunk's loads overwrite other lanes' slots
  }
  __shared__ fe lred[4];
  cs_write_sums<SUMS>(P, lane_lds, B, partials, la, lb, lred, lin);
}

// (the kernels without sum columns keep their argument lists)
__global__ void __launch_bounds__(256)
cs_sums_kernel(const CsDev P, const fe* __restrict__ m, const fe* __restrict__ d, uint64_t h,
               fe* __restrict__ partials) {
  cs_sums_body<false>(P, m, d, h, partials, 0u, nullptr);
}
__global__ void __launch_bounds__(256)
cs_sums_lin_kernel(const CsDev P, const fe* __restrict__ m, const fe* __restrict__ d, uint64_t h,
                   fe* __restrict__ partials, uint32_t smask, fe* __restrict__ lin) {
  cs_sums_body<true>(P, m, d, h, partials, smask, lin);
}

template <bool SUMS>
__device__ __forceinline__ void cs_fold_sums_body(const CsDev& P, fe* m, fe* d, uint64_t S, fe r,
                                                  const fe* __restrict__ rp,
                                                  fe* __restrict__ partials, uint32_t smask,
                                                  fe* __restrict__ lin) {
  extern __shared__ fe cs_lds[];
  if (rp) r = fe_load(rp);
  r = fe_vgpr(r);
  const uint32_t B = blockDim.x, tid = threadIdx.x, W = P.width, step0 = W + P.n_temps;
  const uint64_t q = S / 4, qW = q * W;
  fe* lane_lds = cs_lds + tid;
  fe la = fe_zero(), lb = fe_zero();
  cs_zero_sums(P, lane_lds, B);
  for (uint64_t base = (uint64_t)blockIdx.x * B; base < q; base += (uint64_t)gridDim.x * B) {
    const uint32_t nrows = q - base < B ? (uint32_t)(q - base) : B;
    fe* t0 = m + base * W;
    CsWalk w(tid, B, W);
    for (uint32_t e = tid; e < nrows * W; e += B, w.next()) {
      const fe a = fe_load(t0 + e), b = fe_load(t0 + e + qW);
      const fe c = fe_load(t0 + e + 2 * qW), dq = fe_load(t0 + e + 3 * qW);
      const fe n0 = lerp_s(a, c, r), n1 = lerp_s(b, dq, r);  // sumcheck.rs:234-247
      fe_store(t0 + e, n0);
      fe_store(t0 + e + qW, n1);
      cs_lds[w.col * B + w.row] = n1;
      cs_lds[(step0 + w.col) * B + w.row] = fe_sub(n1, n0);
    }
    const bool valid = tid < nrows;
    fe dc = fe_zero(), dd = fe_zero();
    if (valid) {
      fe* dp = d + base + tid;
      const fe n0 = lerp_s(fe_load(dp), fe_load(dp + 2 * q), r);
      const fe n1 = lerp_s(fe_load(dp + q), fe_load(dp + 3 * q), r);
      fe_store(dp, n0);
      fe_store(dp + q, n1);
      dc = n1;
      dd = fe_sub(n1, n0);
    }
    __syncthreads();
    if (SUMS && valid) cs_linear(P, lane_lds, B, smask, la, lb);
    cs_accumulate(P, lane_lds, B, valid, dc, dd);
    __syncthreads();
  }
  __shared__ fe lred[4];
  cs_write_sums<SUMS>(P, lane_lds, B, partials, la, lb, lred, lin);
}

__global__ void __launch_bounds__(256)
cs_fold_sums_kernel(const CsDev P, fe* m, fe* d, uint64_t S, fe r, const fe* __restrict__ rp,
                    fe* __restrict__ partials) {
  cs_fold_sums_body<false>(P, m, d, S, r, rp, partials, 0u, nullptr);
}
__global__ void __launch_bounds__(256)
cs_fold_sums_lin_kernel(const CsDev P, fe* m, fe* d, uint64_t S, fe r, const fe* __restrict__ rp,
                        fe* __restrict__ partials, uint32_t smask, fe* __restrict__ lin) {
  cs_fold_sums_body<true>(P, m, d, S, r, rp, partials, smask, lin);
}

// SumcheckTables::fold (sumcheck.rs:234-247): elements [0, hW) of the matrix
// and [0, h) of delta, one per thread.
__global__ void __launch_bounds__(256)
cs_fold_kernel(fe* m, fe* d, uint64_t hW, uint64_t h, fe r, const fe* __restrict__ rp) {
  if (rp) r = fe_load(rp);
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < hW)
    fe_store(m + i, lerp_s(fe_load(m + i), fe_load(m + i + hW), r));
  else if (i - hW < h)
    fe_store(d + (i - hW), lerp_s(fe_load(d + (i - hW)), fe_load(d + (i - hW) + h), r));
}

// Reduce partials[t * nb + b] over b; thread 0 of the block ends with out_t in
// ev[t + 1] (LDS).
__device__ __forceinline__ void cs_reduce_partials(const fe* __restrict__ partials, uint32_t nb,
                                                   uint32_t D, fe* ev) {
  __shared__ fe red[4];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (uint32_t t = 0; t < D; ++t) {
    fe v = fe_zero();
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) v = fe_add(v, fe_load(partials + (uint64_t)t * nb + i));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fe_add(v, shfl_xor_fe(v, m));
    if (lane == 0) red[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (uint32_t w = 1; w < (blockDim.x >> 6); ++w) v = fe_add(v, red[w]);
      ev[t + 1] = v;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kRedThreads)
cs_reduce_kernel(const fe* __restrict__ partials, uint32_t nb, uint32_t D, fe* __restrict__ out) {
  __shared__ fe ev[kCsMaxD + 1];
  cs_reduce_partials(partials, nb, D, ev);
  if (threadIdx.x < D) fe_store(out + threadIdx.x, ev[threadIdx.x + 1]);
}

// next_challenge() (transcript.rs:35-38) of the LDS-resident state s0, as
// dsha_challenge, but with the scratch of the byte path (a state whose length
// is not a multiple of 4: bytes absorbed on the host) in LDS -- `c` and the
// 72-byte `pad` -- so that the kernel has no private segment.
// (dsha_update's byte loop, inlined: a call to the out-of-line function costs
// the kernel a stack frame)
__device__ __forceinline__ void cs_update_bytes(DevSha& s, const uint8_t* p, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    s.buf[s.len % 64] = p[i];
    s.len += 1;
    if (s.len % 64 == 0) dsha_compress_buf(s);
  }
}
// (forced inline: with two round kernels it has two call sites, and a call
// left out of line costs each of them a stack frame)
__device__ __forceinline__ fe cs_challenge(const DevSha& s0, DevSha& c, uint8_t* pad) {
  const uint64_t bits = s0.len * 8;
  const uint32_t fill = (uint32_t)(s0.len % 64);
  uint32_t h[8];
  if ((s0.len & 3) == 0) {  // the padded block(s) straight from the buffer words (dsha_final)
    const uint32_t* bw = reinterpret_cast<const uint32_t*>(s0.buf);
    const uint32_t pos = fill / 4;
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t b = bw[i];
      w[i] = (uint32_t)i < pos ? bswap32(b) : ((uint32_t)i == pos ? 0x80000000u : 0u);
    }
    Sha256State st;
#pragma unroll
    for (int i = 0; i < 8; ++i) st.h[i] = s0.h[i];
    if (pos >= 14) {
      sha256_compress_valu(st, w);
#pragma unroll
      for (int i = 0; i < 14; ++i) w[i] = 0;
    }
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
    sha256_compress_valu(st, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = st.h[i];
  } else {
    c = s0;
    const uint32_t nz = fill < 56 ? 55 - fill : 119 - fill;  // zeros up to length 56 mod 64
    pad[0] = 0x80;
    for (uint32_t i = 1; i <= nz; ++i) pad[i] = 0;
    for (uint32_t i = 0; i < 8; ++i) pad[1 + nz + i] = (uint8_t)(bits >> (56 - 8 * i));
    cs_update_bytes(c, pad, 1 + nz + 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = c.h[i];
  }
  fe v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v.w[i] = bswap32(h[i]);
  return canon_with_carry(v, 0u);
}

// One round (compute_sumcheck_polynomial, sumcheck.rs:174-202) after its sums:
// evals[1..D] from the partials, evals[0] = claim - evals[1] (:188), the
// coefficients as vinv * evals (lane k: coefficient k; the exact interpolation
// of polynomials.rs:51-87), absorb LE16(c1) .. LE16(cD) (:194-197), r =
// next_challenge(), claim = pol(r) by Horner (polynomials.rs:9-14).
// SUMS: evals[t] += beta (A + (t - 1) B), A and B reduced from lin (the sum
// columns' linear part; the header comment).
template <bool SUMS>
__device__ __forceinline__ void cs_round_body(const fe* __restrict__ partials, uint32_t nb, uint32_t D,
                                              const fe* __restrict__ vinv, fe* prev, DevSha* t,
                                              fe* __restrict__ poly_out, fe* __restrict__ r_out,
                                              const fe* __restrict__ lin, const fe& beta) {
  __shared__ DevSha s, sc;
  __shared__ uint32_t stage[4];
  __shared__ uint8_t pad[72];
  __shared__ fe ev[kCsMaxD + 1], coef[kCsMaxD + 1];
  if (threadIdx.x < sizeof(DevSha) / 4)
    reinterpret_cast<uint32_t*>(&s)[threadIdx.x] = reinterpret_cast<const uint32_t*>(t)[threadIdx.x];
  cs_reduce_partials(partials, nb, D, ev);  // (its barriers also publish the staged state)
  if (SUMS) {
    __shared__ fe lv[3];  // lv[1] = A, lv[2] = B
    cs_reduce_partials(lin, nb, 2, lv);
    if (threadIdx.x >= 1 && threadIdx.x <= D) {
      fe l = lv[1];
      for (uint32_t i = 1; i < threadIdx.x; ++i) l = fe_add(l, lv[2]);
      ev[threadIdx.x] = fe_add(ev[threadIdx.x], fe_mul(fe_vgpr(beta), l));
    }
    __syncthreads();
  }
  const uint32_t N = D + 1;
  const fe claim = fe_load(prev);
  if (threadIdx.x < N) {
    const uint32_t k = threadIdx.x;
    fe c = fe_mul(fe_load(vinv + k * N), fe_sub(claim, ev[1]));
    for (uint32_t j = 1; j < N; ++j) c = fe_add(c, fe_mul(fe_load(vinv + k * N + j), ev[j]));
    coef[k] = c;
    if (k) fe_store(poly_out + (k - 1), c);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (uint32_t k = 1; k < N; ++k) {
    const fe c = coef[k];
    const uint32_t w[4] = {c.w[0], c.w[1], c.w[2], c.w[3]};
    if ((s.len & 3) == 0) {
      dsha_absorb_words<4>(s, w);
    } else {
      for (int i = 0; i < 4; ++i) stage[i] = w[i];
      cs_update_bytes(s, reinterpret_cast<const uint8_t*>(stage), 16);
    }
  }
  const fe r = cs_challenge(s, sc, pad);
  fe_store(r_out, r);
  fe p = coef[D];
  for (uint32_t k = D; k-- > 0;) p = fe_add(fe_mul(p, r), coef[k]);
  fe_store(prev, p);
  *t = s;
}
__global__ void __launch_bounds__(kRedThreads)
cs_round_kernel(const fe* __restrict__ partials, uint32_t nb, uint32_t D,
                const fe* __restrict__ vinv, fe* prev, DevSha* t, fe* __restrict__ poly_out,
                fe* __restrict__ r_out) {
  cs_round_body<false>(partials, nb, D, vinv, prev, t, poly_out, r_out, nullptr, fe_zero());
}
__global__ void __launch_bounds__(kRedThreads)
cs_round_lin_kernel(const fe* __restrict__ partials, uint32_t nb, uint32_t D,
                    const fe* __restrict__ vinv, fe* prev, DevSha* t, fe* __restrict__ poly_out,
                    fe* __restrict__ r_out, const fe* __restrict__ lin, fe beta) {
  cs_round_body<true>(partials, nb, D, vinv, prev, t, poly_out, r_out, lin, beta);
}

// ---- launchers -------------------------------------------------------------

static inline size_t cs_lds_bytes(const CsDev& P, uint32_t threads) {
  return (size_t)(2 * P.width + P.n_temps + P.D) * threads * sizeof(fe);
}
// what the sums and the fold + sums launches both need
static inline bool cs_launch_ok(const CsDev& P, uint32_t threads, uint32_t smask, const fe* lin) {
  return threads >= 64 && threads <= 256 && !(threads & 63) && P.D <= kCsMaxD && (!smask || lin) &&
         cs_lds_bytes(P, threads) <= kCsLdsBytes;
}

hipError_t launch_cs_sums(const CsDev& P, uint32_t threads, const fe* m, const fe* d, uint64_t h,
                          fe* partials, hipStream_t st, uint32_t* nb, uint32_t smask, fe* lin) {
  if (!cs_launch_ok(P, threads, smask, lin) || h == 0) return hipErrorInvalidValue;
  const size_t lds = cs_lds_bytes(P, threads);
  const uint32_t n = cs_blocks(h, threads);
  if (smask)
    hipLaunchKernelGGL(cs_sums_lin_kernel, dim3(n), dim3(threads), lds, st, P, m, d, h, partials,
                       smask, lin);
  else
    hipLaunchKernelGGL(cs_sums_kernel, dim3(n), dim3(threads), lds, st, P, m, d, h, partials);
  *nb = n;
  return hipGetLastError();
}

hipError_t launch_cs_fold_sums(const CsDev& P, uint32_t threads, fe* m, fe* d, uint64_t S, fe r,
                               const fe* r_dev, fe* partials, hipStream_t st, uint32_t* nb,
                               uint32_t smask, fe* lin) {
  if (!cs_launch_ok(P, threads, smask, lin) || S < 4) return hipErrorInvalidValue;
  const size_t lds = cs_lds_bytes(P, threads);
  const uint32_t n = cs_blocks(S / 4, threads);
  if (smask)
    hipLaunchKernelGGL(cs_fold_sums_lin_kernel, dim3(n), dim3(threads), lds, st, P, m, d, S, r, r_dev,
                       partials, smask, lin);
  else
    hipLaunchKernelGGL(cs_fold_sums_kernel, dim3(n), dim3(threads), lds, st, P, m, d, S, r, r_dev,
                       partials);
  *nb = n;
  return hipGetLastError();
}

hipError_t launch_cs_fold(uint32_t width, fe* m, fe* d, uint64_t S, fe r, const fe* r_dev,
                          hipStream_t st) {
  if (S < 2 || width == 0) return hipErrorInvalidValue;
  const uint64_t h = S / 2, hW = h * width, n = hW + h;
  hipLaunchKernelGGL(cs_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m, d, hW, h,
                     r, r_dev);
  return hipGetLastError();
}

hipError_t launch_cs_round(const fe* partials, uint32_t nb, uint32_t D, const fe* vinv, fe* prev,
                           DevSha* t, fe* poly_out, fe* r_out, hipStream_t st, const fe* lin,
                           fe beta) {
  if (D < 2 || D > kCsMaxD) return hipErrorInvalidValue;
  if (lin)
    hipLaunchKernelGGL(cs_round_lin_kernel, dim3(1), dim3(kRedThreads), 0, st, partials, nb, D, vinv,
                       prev, t, poly_out, r_out, lin, beta);
  else
    hipLaunchKernelGGL(cs_round_kernel, dim3(1), dim3(kRedThreads), 0, st, partials, nb, D, vinv, prev,
                       t, poly_out, r_out);
  return hipGetLastError();
}

hipError_t launch_cs_reduce(const fe* partials, uint32_t nb, uint32_t D, fe* out, hipStream_t st) {
  if (D < 1 || D > kCsMaxD) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cs_reduce_kernel, dim3(1), dim3(kRedThreads), 0, st, partials, nb, D, out);
  return hipGetLastError();
}

}  // namespace mlh
