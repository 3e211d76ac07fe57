// Radix-2 NTT over F_M for gfx950.
//
// Reference semantics: src/ntt/mod.rs:69-110 (Polynomial::ntt) and :132-173
// (LagrangePolynomial::intt): natural-order coefficients in, natural-order
// evaluations out, evals[i] = sum_j c_j * gen^(i*j); the inverse uses gen^-1
// and scales by n^-1.  The reference's bit-reverse + serial-twiddle DIT is an
// implementation detail; any exact algorithm gives identical field values.
//
// MI355X design (DESIGN.md "NTT"): N = R_1 * ... * R_P with R_p = 2^6..2^9.
// Pass p transforms digit p of the index in place (a generalised four-step):
//   * a workgroup owns C = 8 adjacent "columns" x R rows, so every global
//     access is 8 elements x 16 B = 128 contiguous bytes (dwordx4 per lane);
//   * each thread holds 8 elements in VGPRs and runs radix-2 DIT stages in
//     register phases of <= 3 stages; phases exchange through LDS
//     (C*R*16 B, 32 KiB at R = 256);
//   * the sub-transform input is read in bit-reversed row order straight from
//     HBM (the permutation is on the per-lane global address, free), so the
//     DIT output is in natural order;
//   * passes p < P multiply by the inter-pass twiddle w^(j_rest*k*S_p), read
//     from one table TA[k][j_rest] or, when that would exceed 2^22 entries,
//     TA[k][j_lo] * TB[k][j_hi] (TB expanded, staged through LDS: one j_hi
//     per tile);
//     for the inverse, pass 0's TA carries the n^-1 scale (no extra pass);
//   * stage twiddles: expanded tables (fe_mul_pre), the lane-dependent ones
//     read from a per-workgroup LDS copy;
//   * the last pass tiles 8 consecutive k_1 values so its scattered natural-
//     order stores are still 128-byte runs.
//   * every global address is a wave-uniform base (SGPR pair) plus one 32-bit
//     per-lane byte offset per buffer; a thread's 8 rows differ by compile-time
//     constants that go to the base (64-bit offsets, ntt_pass_wide_kernel,
//     where a tile spans 2^32 bytes).
// Sizes N <= 2^10 use one LDS-resident workgroup (ntt_small).
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "bfly_asm.hpp"
#include "field.hpp"
#include "ntt.hpp"

namespace mlh {

constexpr int kCols = 8;  // columns per tile (8 x 16 B = 128 B runs)
constexpr int kLogCols = 3;
constexpr int kEPT = 8;   // elements per thread

__device__ __forceinline__ uint32_t bitrev(uint32_t x, int bits) {
  return __builtin_bitreverse32(x) >> (32 - bits);
}

// Global accesses of the pass kernels: a wave-uniform pointer (SGPR pair) plus
// a per-lane byte offset.  With a 32-bit offset the compiler selects the
// "global_load v, v_off32, s[base:base+1]" form, so the per-lane part of an
// address is one VGPR formed once and every further term (the element's
// compile-time row, the tile, the vector) is added to the base on the SALU.
// Off = uint32_t is valid while every byte offset from the uniform base is
// below 2^32 (the host decides per launch: pass_wide()); Off = uint64_t is
// the same arithmetic in 64 bits.
// The narrow form passes the base through readfirstlane (a scalar move for a
// value that is uniform already): otherwise the optimiser reassociates
// (base + constant row) + lane into (base + lane) + constant row, a 64-bit
// VGPR address plus one v_lshl_add_u64 per access.
// (the rebuilt pointer is typed as global memory, which an integer round trip
// would otherwise forget)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 global_u32x4;
template <typename Off>
__device__ __forceinline__ global_u32x4* pass_addr(const void* ubase, Off lane_bytes) {
  uint64_t v = reinterpret_cast<uint64_t>(ubase);
  if constexpr (sizeof(Off) == 4) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    v = ((uint64_t)hi << 32) | lo;
  }
  return (global_u32x4*)(v + lane_bytes);
}
template <typename Off>
__device__ __forceinline__ fe fe_load_at(const fe* ubase, Off lane_bytes) {
  const u32x4 v = *pass_addr<Off>(ubase, lane_bytes);
  return fe{{v.x, v.y, v.z, v.w}};
}
template <typename Off>
__device__ __forceinline__ void fe_store_at(fe* ubase, Off lane_bytes, const fe& x) {
  *pass_addr<Off>(ubase, lane_bytes) = u32x4{x.w[0], x.w[1], x.w[2], x.w[3]};
}
// Instruction selection sees one basic block at a time, and takes the
// SGPR-base form only where the 32-bit lane offset's zero extension is in the
// access's own block; the butterflies' rare-case branches split the epilogue
// into many blocks, and the optimiser keeps one shared (hoisted) extension.
// An empty statement that redefines the offset in place (same register, no
// instruction) before a block's accesses keeps each extension local.
__device__ __forceinline__ void pin_lane_offset(uint32_t& v) { asm("" : "+v"(v)); }
__device__ __forceinline__ void pin_lane_offset(uint64_t&) {}
// The constant of the butterflies' wrap correction (bfly_asm.hpp: a "v"
// operand of every statement).  Passed as a literal, each statement gets a
// v_mov_b32 of its own; redefined in place once, it is a value the optimiser
// cannot see through, held in one VGPR for the whole kernel.
__device__ __forceinline__ uint32_t pin_constant(uint32_t v) {
  asm("" : "+v"(v));
  return v;
}
constexpr uint32_t bitrev_c(uint32_t x, int bits) {
  uint32_t r = 0;
  for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
}
// Position of a thread's elements in register phase (s0, q): the group index
// gamma = t * G + gi keeps its low s0 bits and moves the rest up by q;
// element i of the group adds i << s0.  A bit placement, so it splits into a
// per-lane part (of t * G) and a compile-time part (of gi and i) on disjoint
// bits: pos = pos_lane + pos_c, and every address linear in pos is one lane
// term plus a constant.
constexpr uint32_t phase_bpos(uint32_t gamma, int s0, int q) {
  return (gamma & ((1u << s0) - 1u)) | ((gamma >> s0) << (s0 + q));
}
constexpr uint32_t phase_pos_c(int s0, int q, int e) {
  return phase_bpos((uint32_t)(e >> q), s0, q) + ((uint32_t)(e & ((1 << q) - 1)) << s0);
}

struct PassGeom {
  uint32_t log_n;
  uint32_t nradix;      // P
  uint32_t p;           // 0-based pass index
  uint32_t logr[kMaxPasses];
  // every stride and count is a power of two: log2 of each, so that the
  // kernels index by shifts (no 64-bit multiplies or divisions per address)
  uint32_t lstride;     // W_p = 2^lstride (elements between consecutive rows of this digit)
  uint32_t loga;        // inter-pass twiddle split jrest = jh * 2^loga + jl
  uint32_t ltpv;        // tiles per vector (batched transforms: blockIdx.x = b*2^ltpv + tile)
  uint32_t lin_v;       // elements between consecutive input vectors
  uint32_t lout_v;      // elements between consecutive output vectors
  // TW 4 (the sharded NTT's fused last pass, mlh_sharded_ntt_fused_batch):
  // log2 P, this rank, log2 of the per-source chunk of the receive buffer
  uint32_t sh_p = 0, sh_rank = 0, sh_lchunk = 0;
};

// Last pass: natural output index is K = k_1 + R_1*rev(mid) + (N/R_P)*k_P,
// where mid holds digits 2..P-1 in storage order (digit 2 most significant)
// and rev() re-weights them in natural order (digit 2 least significant).
__device__ __forceinline__ uint64_t reverse_mid_digits(const PassGeom& g, uint64_t mid) {
  uint64_t rev = 0;
  // storage: lowest digit of mid is digit P-1 (0-based index nradix-2)
  for (int q = (int)g.nradix - 2; q >= 1; --q) {
    uint32_t shift = 0;  // natural weight of digit q: R_2*...*R_{q}
    for (int i = 1; i < q; ++i) shift += g.logr[i];
    rev += (mid & ((1ull << g.logr[q]) - 1)) << shift;
    mid >>= g.logr[q];
  }
  return rev;
}

// TW: 0 = two-table twiddle (TA * TB), 1 = one table (TA), 2 = none (last pass),
// 5 = pass 0's twiddle as a progression (ta = P[k0][j] = w_S^(k0 j), k0 < 64;
// tb = C[j] = w_S^(64 j), expanded): a thread's rows after its last register
// phase are k0 + 64 i, so w_S^(j (k0 + 64 i)) = P[k0][j] C[j]^i -- one product
// per step instead of TA * TB per element, no TB staging through LDS, 2 + 4
// twiddle loads per thread instead of 8 + TB's (LOGR 7 and 8);
// 3 = one table on pass 0 (same code as 1; its own kernel so that rocprof and
// the kernel timer tell the first pass from the middle ones), 4 = the last
// pass of a sharded transform (as 2, over this rank's share of the global
// tiles, reading the all-to-all's receive buffer: global storage index V lives
// at ((V mod P) << sh_lchunk) | ((V >> p) mod 2^sh_lchunk); writing the
// block-cyclic local output, K with bits [logr0 - p, logr0) removed)
// waves per SIMD the LDS tile allows (160 KiB/CU): caps VGPRs to match
#ifndef MLH_WPS8
#define MLH_WPS8 4  // R = 2^8: 32 KiB tile + 8 KiB twiddle copy -> 4 workgroups per CU
#endif
#ifndef MLH_LAST_STAGED
#define MLH_LAST_STAGED 1  // last pass loads through LDS (coalesced runs): pass -3..6 %
#endif
#ifndef MLH_LAST_DIRECT
// last pass (not sharded, full input): phase 1 runs with the lanes of a
// column on consecutive rows (coalesced 16 B x TPC runs straight from HBM),
// the first exchange switches to the 8-columns-per-row lane map the later
// phases and the natural-order stores use: no staged tile, one LDS round trip
// and one barrier fewer
#define MLH_LAST_DIRECT 1
#endif
#ifndef MLH_LDS_PAD
#define MLH_LDS_PAD 0  // extra dynamic LDS per pass workgroup (occupancy experiments)
#endif
#ifndef MLH_DIAG_TW  // diagnostics only (WRONG results): 1 = no TB, 2 = no TB and no TA loads
#define MLH_DIAG_TW 0
#endif
#ifndef MLH_LDS_TW
#define MLH_LDS_TW 1  // stage twiddles of the lane-dependent phases read from an LDS copy
#endif
constexpr int pass_waves_per_simd(int logr, int ept) {
  return ept == 16 ? 2 : (logr == 8 ? MLH_WPS8 : (logr == 9 ? 4 : (logr == 7 ? 4 : 2)));
}

// ZT: 0 = full input; 1 = input has N/2 elements, upper half implicit zeros
// (Reed-Solomon); 2 = as 1, with the N/2 inputs stored bit-reversed, i.e.
// coefficient j is in[bitrev_{log_n - 1}(j)] (the PCS's bit_reverse_permutation
// folded into pass 0's loads; pass 0 only, never the last pass).
// EPT: elements per thread (8: register phases of 3 stages; 16: of 4 stages,
// one LDS exchange fewer at R = 2^8, twice the VGPRs).
// WIDE: 64-bit per-lane offsets (a tile or table that spans 2^32 bytes or more).
// (the body of both kernels below: ntt_pass_kernel is the narrow form,
// ntt_pass_wide_kernel the wide one)
template <int LOGR, int TW, int ZT, int EPT, bool WIDE>
__device__ __forceinline__ void ntt_pass_body(const fe* in, fe* out, const fe* __restrict__ tw,
                                              const fe* __restrict__ ta, const fe* __restrict__ tb,
                                              const PassGeom& g) {
  constexpr int R = 1 << LOGR;
  constexpr int LQ = EPT == 16 ? 4 : 3;  // stages per register phase
  constexpr int TPC = R / EPT;  // threads per column
  constexpr bool LAST = TW == 2 || TW == 4;
  constexpr bool SH = TW == 4;
  using Off = std::conditional_t<WIDE, uint64_t, uint32_t>;
  // sharded last pass: global storage index -> receive-buffer position
  auto phys = [&](uint64_t v) -> uint64_t {
    if constexpr (SH)
      return ((v & ((1ull << g.sh_p) - 1)) << g.sh_lchunk) |
             ((v >> g.sh_p) & ((1ull << g.sh_lchunk) - 1));
    else
      return v;
  };
  __shared__ fe lds[R * kCols];
#if MLH_LDS_TW
  // The expanded stage twiddles (R/2 entries x 4 limb-shifted multiples, 2R
  // fe).  Phase 1 indexes them by compile-time j (scalar loads); the later
  // phases by a lane-dependent j, where 4 global dwordx4 loads per twiddle per
  // lane were 3/4 of the pass's vector loads: those read this broadcast copy.
  // Written here; read only after the first exchange's barriers.
  __shared__ fe lds_tw[LOGR > LQ ? 2 * R : 1];
  if constexpr (LOGR > LQ) {
    constexpr int NT = kCols * R / EPT;  // threads per workgroup
    static_assert((2 * R) % NT == 0, "twiddle copy: whole rounds");
#pragma unroll
    for (int e = 0; e < 2 * R / NT; ++e)
      lds_tw[e * NT + threadIdx.x] = fe_load(tw + e * NT + threadIdx.x);
  }
#endif

  const int tid = threadIdx.x;
  // - 0x2D00, limb 1 of the butterflies' wrap correction
  const uint32_t kneg = pin_constant(0xFFFFD300u);
  // kDirect: phase 1 with column cA = tid / TPC and t = bitrev(tid mod TPC),
  // so lane l of a column loads row rev(8t + e) = rev3(e) TPC + l (consecutive
  // across lanes); the first exchange switches to c = tid mod 8, t = tid / 8
  constexpr bool kDirect = MLH_LAST_DIRECT && LAST && !SH && ZT == 0 && EPT == 8 && LOGR >= 6;
  constexpr int kLTPC = LOGR - 3;  // log2 threads per column (EPT = 8)
  const int cB = tid % kCols;
  int c = cB;
  int t = tid / kCols;
  if constexpr (kDirect) {
    c = tid >> kLTPC;
    t = (int)bitrev((uint32_t)tid & ((1u << kLTPC) - 1), kLTPC);
  }
  const uint64_t vec = (uint64_t)blockIdx.x >> g.ltpv;
  uint64_t tile = blockIdx.x & ((1ull << g.ltpv) - 1);
  if constexpr (SH) {  // this rank's tiles: first-digit columns whose top p bits are the rank
    const uint32_t lmid = g.log_n - g.logr[0] - LOGR;
    const uint32_t ld1 = g.logr[0] - kLogCols - g.sh_p;  // local first-digit column groups
    tile = ((((uint64_t)g.sh_rank << ld1) | (tile >> lmid)) << lmid) | (tile & ((1ull << lmid) - 1));
  }
  in += vec << g.lin_v;
  out += vec << g.lout_v;

  // ---- tile geometry -----------------------------------------------------
  // (base, jcol0, k1u, mid are wave-uniform; the lane's column cB is added
  // where an address or index needs it)
  uint64_t base, jcol0 = 0, jrest = 0, k1u = 0, mid = 0;
  uint32_t rshift;  // log2 element stride between rows of this digit
  uint32_t cshift;  // log2 element stride between the 8 columns
  if (!LAST) {
    const uint32_t lw = g.lstride;  // W >= kCols
    const uint64_t hi = tile >> (lw - kLogCols), lo = tile & ((1ull << (lw - kLogCols)) - 1);
    base = (hi << (LOGR + lw)) + (lo << kLogCols);
    jcol0 = lo << kLogCols;
    jrest = jcol0 + cB;
    rshift = lw;
    cshift = 0;
  } else {
    const uint32_t lw1 = g.log_n - g.logr[0];  // W1 = N / R1
    const uint32_t lmid = lw1 - LOGR;          // MID = N / (R1 R_P)
    const uint64_t d1hi = tile >> lmid;
    mid = tile & ((1ull << lmid) - 1);
    base = (d1hi << (kLogCols + lw1)) + (mid << LOGR);
    k1u = d1hi << kLogCols;
    rshift = 0;
    cshift = lw1;
  }
  const fe* tile_in = in + base;
  fe* tile_out = out + base;
  // phase 1's rows are bitrev(t EPT + e) = bitrev(t EPT) + bitrev(e): the lane's
  // byte offset into the tile, and a compile-time row added to the base
  const Off ld_lane = ((((Off)bitrev((uint32_t)t * EPT, LOGR)) << rshift) + ((Off)c << cshift)) << 4;


  // ---- phase 1: load bit-reversed rows, stages 0..2 in registers ---------
  fe x[EPT];
#if MLH_LAST_STAGED
  // last pass: its rows are consecutive elements, so a lane's bit-reversed
  // rows scatter one wave's loads over 64 separate 16-B pieces.  Load the tile
  // as 8 x 128-B runs per wave instruction (8 consecutive rows x 8 columns)
  // into LDS, then read the bit-reversed rows from there.
  if constexpr (LAST && ZT == 0 && !kDirect) {
    constexpr int NT = kCols * R / EPT;
    // (the staged tile's columns are XOR-swizzled by row: lanes 0..7 write 8
    // consecutive rows of one column, which unswizzled sit 128 B apart on the
    // same LDS banks; the reads take one row's 8 columns, a permutation either way)
    // SH: a row's low p bits are its source rank, so the 8 lanes of a column
    // take rows P apart (consecutive in that source's chunk), and the swizzle
    // mixes in the bits above the rank bits.
    auto swz = [&](uint32_t row) -> uint32_t {
      if constexpr (SH) return (row ^ (row >> g.sh_p)) & (kCols - 1);
      else return row & (kCols - 1);
    };
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const uint32_t idx = (uint32_t)(e * NT + tid);
      const uint32_t l = idx & 63, grp = idx >> 6;
      uint32_t row = grp * 8 + (l & 7);
      if constexpr (SH) {
        const uint32_t lq = LOGR - g.sh_p - 3;  // groups of 8 rows per source rank: 2^lq
        const uint32_t src = grp >> lq, q0 = grp & ((1u << lq) - 1);
        row = ((((q0 << 3) + (l & 7)) << g.sh_p)) | src;
      }
      const uint32_t col = l >> 3;
      if constexpr (SH) {
        lds[row * kCols + (col ^ swz(row))] = fe_load(in + phys(base + ((uint64_t)col << cshift) + row));
      } else {
        // idx = e NT + tid on disjoint bits, and (col << cshift) + row places
        // idx's bits: the element offset of idx is that of e NT (uniform)
        // plus that of tid (lane)
        auto tile_at = [&](uint32_t i) -> Off {
          return ((Off)((i & 63) >> 3) << cshift) + (Off)((i >> 6) * 8 + (i & 7));
        };
        lds[row * kCols + (col ^ swz(row))] =
            fe_load_at<Off>(tile_in + (uint64_t)tile_at((uint32_t)(e * NT)), tile_at((uint32_t)tid) << 4);
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const uint32_t row = bitrev((uint32_t)(t * EPT + e), LOGR);
      x[e] = lds[row * kCols + (c ^ swz(row))];
    }
  } else
#endif
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const uint32_t row = bitrev((uint32_t)(t * EPT + e), LOGR);
    // rows >= R/2 are the implicit zero half; bitrev puts them exactly at odd e
    if (ZT != 0 && (e & 1)) {
      x[e] = fe_zero();
    } else if (ZT == 2) {
      // coefficient row*W + col, row < R/2, lives at bitrev(col)*(R/2) +
      // bitrev_{LOGR-1}(row) = bitrev(col)*(R/2) + (t*EPT + e)/2: each lane
      // reads 4 consecutive elements
      // (bitrev(col) = bitrev(jcol0) + bitrev_3(cB) << (logw - 3): uniform + lane)
      const uint32_t logw = g.log_n - LOGR;
      const uint64_t colr_u = __builtin_bitreverse64(jcol0) >> (64 - logw);
      const Off colr_l = (Off)bitrev((uint32_t)cB, kLogCols) << (logw - kLogCols);
      x[e] = fe_load_at<Off>(in + (colr_u << (LOGR - 1)) + (e >> 1),
                             ((colr_l << (LOGR - 1)) + (Off)(t * (EPT / 2))) << 4);
    } else if constexpr (SH) {
      x[e] = fe_load(in + phys(base + ((uint64_t)c << cshift) + ((uint64_t)row << rshift)));
    } else {
      x[e] = fe_load_at<Off>(tile_in + ((uint64_t)bitrev_c((uint32_t)e, LOGR) << rshift), ld_lane);
    }
  }

  // Generic register phase: stages [s0, s0+q) on groups of 2^q elements.
  // Butterflies run two at a time through the generated asm (bfly_asm.hpp) in
  // the relaxed representation; phase 1's twiddles are wave-uniform (SGPR
  // operands), the later phases' come from the LDS copy (VGPR operands).
  auto run_phase = [&](auto S0_, auto Q_) {
    constexpr int s0 = decltype(S0_)::value;
    constexpr int q = decltype(Q_)::value;
    constexpr int G = EPT >> q;
    constexpr int NB = EPT / 2;            // butterflies per stage
    constexpr int BPG = 1 << (q - 1);      // per group
#pragma unroll
    for (int s = s0; s < s0 + q; ++s) {
      const int d = 1 << (s - s0);  // element distance inside a group
      int be0[NB], be1[NB];
      uint32_t bj[NB];
      bool btriv[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int gi = b / BPG, m = b % BPG;
        const int i = ((m >> (s - s0)) << (s - s0 + 1)) | (m & (d - 1));
        be0[b] = gi * (1 << q) + i;
        be1[b] = be0[b] + d;
        // (lane part + compile-time part of the position, as pos_lane below)
        bj[b] = (phase_bpos((uint32_t)(t * G), s0, q) & ((1u << s) - 1u)) +
                (phase_pos_c(s0, q, gi * (1 << q) + i) & ((1u << s) - 1u));
        // phase 1: j is a compile-time function of i (s == 0 or j == 0: w = 1)
        btriv[b] = s0 == 0 && (s == 0 || (i & ((1 << s) - 1)) == 0);
      }
      if (ZT != 0 && s0 == 0 && s == 0) {  // (u, 0) -> (u, u)
#pragma unroll
        for (int b = 0; b < NB; ++b) x[be1[b]] = x[be0[b]];
        continue;
      }
      uint64_t rare;
#pragma unroll
      for (int b = 0; b < NB; b += 2) {
        fe& u0 = x[be0[b]];
        fe& v0 = x[be1[b]];
        fe& u1 = x[be0[b + 1]];
        fe& v1 = x[be1[b + 1]];
        if (s0 == 0) {
          const fe* w0 = tw + 4 * (bj[b] << (LOGR - 1 - s));
          const fe* w1 = tw + 4 * (bj[b + 1] << (LOGR - 1 - s));
          if (!btriv[b] && !btriv[b + 1])
            bfly_mm_s(u0, v0, w0[0], w0[1], w0[2], w0[3], u1, v1, w1[0], w1[1], w1[2], w1[3], kneg, rare);
          else if (!btriv[b])
            bfly_mt_s(u0, v0, w0[0], w0[1], w0[2], w0[3], u1, v1, kneg, rare);
          else if (!btriv[b + 1])
            bfly_mt_s(u1, v1, w1[0], w1[1], w1[2], w1[3], u0, v0, kneg, rare);
          else
            bfly_tt_v(u0, v0, u1, v1, kneg, rare);
        } else {
#if MLH_LDS_TW
          const fe* w0 = lds_tw + 4 * (bj[b] << (LOGR - 1 - s));
          const fe* w1 = lds_tw + 4 * (bj[b + 1] << (LOGR - 1 - s));
#else
          const fe* w0 = tw + 4 * (bj[b] << (LOGR - 1 - s));
          const fe* w1 = tw + 4 * (bj[b + 1] << (LOGR - 1 - s));
#endif
          bfly_mm_v(u0, v0, w0[0], w0[1], w0[2], w0[3], u1, v1, w1[0], w1[1], w1[2], w1[3], kneg, rare);
        }
      }
    }
  };
  // the lane part of the phase's positions: element e is at pos_lane + pos_c(e)
  auto pos_lane = [&](auto S0_, auto Q_) -> uint32_t {
    constexpr int s0 = decltype(S0_)::value;
    constexpr int q = decltype(Q_)::value;
    return phase_bpos((uint32_t)(t * (EPT >> q)), s0, q);
  };

  using I0 = std::integral_constant<int, 0>;
  constexpr int Q1 = LOGR < LQ ? LOGR : LQ;
  run_phase(I0{}, std::integral_constant<int, Q1>{});
  uint32_t pos0 = pos_lane(I0{}, std::integral_constant<int, Q1>{});
  // the last register phase: its positions are the rows of the epilogue
  constexpr int kS0F = LOGR > 2 * LQ ? 2 * LQ : (LOGR > LQ ? LQ : 0);
  constexpr int kQF = LOGR - kS0F;
  auto pos_c = [](int e) -> uint32_t { return phase_pos_c(kS0F, kQF, e); };

  // ---- remaining phases through LDS -------------------------------------
  // One address VGPR per direction: element e is pos_c(e) * kCols * 16 bytes
  // from the lane's slot, an immediate of the ds instruction.
  auto exchange_and_run = [&](auto PS0_, auto PQ_, auto S0_, auto Q_) {
    constexpr int ps0 = decltype(PS0_)::value, pq = decltype(PQ_)::value;
    constexpr int s0 = decltype(S0_)::value, q = decltype(Q_)::value;
    __syncthreads();  // previous phase's reads of lds are done
    fe* wr = &lds[pos0 * kCols + c];
#pragma unroll
    for (int e = 0; e < EPT; ++e) fe_store(wr + phase_pos_c(ps0, pq, e) * kCols, x[e]);
    __syncthreads();
    pos0 = pos_lane(S0_, Q_);
    const fe* rd = &lds[pos0 * kCols + c];
#pragma unroll
    for (int e = 0; e < EPT; ++e) x[e] = fe_load(rd + phase_pos_c(s0, q, e) * kCols);
    run_phase(S0_, Q_);
  };
  // Two-table twiddle: TB[k][jh] has one jh for the tile's 8 columns (loga >=
  // 3), so the 8 lanes of a row read the same entry: one row per thread is
  // loaded and shared through the idle exchange tile.  TB is stored EXPANDED
  // (the 4 limb-shifted multiples, as the stage twiddles), so its product is
  // the 41-VALU expanded one (bfly_pp_v) instead of the 60-VALU full product.
  // MLH_P0_EARLY_TB: its loads (and the first TA pair's) are issued before the
  // last register phase, whose butterflies cover their latency; otherwise
  // just before the epilogue's barriers.
  constexpr int NTt = kCols * R / EPT;
  constexpr int kTbPerThread = TW == 0 ? R / NTt : 1;
  fe tbv[kTbPerThread][4];
  // TA[k][jl], jl = jrest mod 2^loga = (jcol0 mod 2^loga) + cB (loga >= 3): row
  // pos_c(e) and the tile's first jl go to the base, the lane keeps
  // ((pos0 << loga) + cB) * 16
  const fe* ta_tile = ta + (jcol0 & ((1ull << g.loga) - 1));
  auto ta_lane_of = [&](uint32_t p0) -> Off { return (((Off)p0 << g.loga) + (Off)cB) << 4; };
  auto ta_at = [&](int e, Off lane) -> fe {
    return fe_load_at<Off>(ta_tile + ((uint64_t)pos_c(e) << g.loga), lane);
  };
  Off ta_lane = 0;
  fe ta_c0, ta_c1;
  // MLH_TB_COALESCED: the 4R dwordx4 pieces of the tile's TB column are dealt
  // to the threads in order (piece i = part i mod 4 of row i / 4), so 4
  // adjacent lanes read one row's 64-B entry and a wave instruction touches 16
  // entries instead of 64 (each row's entry sits 2^ltcols x 64 B from the
  // next).  Round 5 counters (profiles/r05_ntt_pass_attrib.json): the
  // one-row-per-lane form made 256 of pass 0's 672 L1 requests per wave and
  // kept TA 62 % busy against 27 % in pass 1.  The LDS image is the same.
#ifndef MLH_TB_COALESCED
#define MLH_TB_COALESCED 1
#endif
  auto load_tb = [&]() {
    if constexpr (TW == 0 && MLH_DIAG_TW == 0) {
      const uint64_t jh = jcol0 >> g.loga;  // the same for the whole tile (loga >= 3)
      const uint32_t ltcols = g.lstride - g.loga;
      const fe* tb_tile = tb + (jh << 2);
#if MLH_TB_COALESCED
      static_assert(NTt % 4 == 0, "a round of pieces is whole rows");
      const Off tb_lane = ((((Off)(tid >> 2) << ltcols) << 2) + (Off)(tid & 3)) << 4;
#else
      const Off tb_lane = (((Off)tid << ltcols) << 2) << 4;
#endif
#pragma unroll
      for (int e = 0; e < kTbPerThread; ++e) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#if MLH_TB_COALESCED
          // piece i = (e 4 + k) NTt + tid: row i / 4 = (e 4 + k) NTt / 4 + tid / 4
          tbv[e][k] = fe_load_at<Off>(tb_tile + (((uint64_t)((e * 4 + k) * (NTt / 4)) << ltcols) << 2), tb_lane);
#else
          tbv[e][k] = fe_load_at<Off>(tb_tile + (((uint64_t)(e * NTt) << ltcols) << 2) + k, tb_lane);
#endif
        }
      }
    }
  };
  // the first pair's inter-pass twiddles (the asm products below keep later
  // loads from being hoisted, so each pair's are issued one pair ahead);
  // p0: the lane part of the last phase's positions
  auto load_ta0 = [&](uint32_t p0) {
    if constexpr (TW == 5) {
      (void)p0;
    } else if constexpr (!LAST && MLH_DIAG_TW == 2) {
      ta_c0 = fe{{(uint32_t)jrest | 1u, 7u, 9u, 3u}};
      ta_c1 = fe{{(uint32_t)p0 | 1u, 5u, 9u, 3u}};
    } else if constexpr (!LAST) {
      ta_lane = ta_lane_of(p0);
      ta_c0 = ta_at(0, ta_lane);
      ta_c1 = ta_at(1, ta_lane);
    }
  };
#ifndef MLH_P0_EARLY_TB
#define MLH_P0_EARLY_TB 0
#endif

  constexpr bool kEarly = MLH_P0_EARLY_TB && TW == 0 && LOGR > 2 * LQ;
  if constexpr (LOGR > LQ) {
    constexpr int Q2 = (LOGR - LQ) < LQ ? (LOGR - LQ) : LQ;
    using IQ1 = std::integral_constant<int, Q1>;
    using ILQ = std::integral_constant<int, LQ>;
    using IQ2 = std::integral_constant<int, Q2>;
    if constexpr (kDirect) {
      // written in the phase-1 map, read in the 8-columns-per-row map; the
      // column slot is XORed with the row's top 3 bits, so the 8 lanes of a
      // write group (consecutive l: distinct top bits of t) and of a read
      // group (8 columns of one row) each hit 8 distinct 16-B slots.
      // row = pos0 + pos_c on disjoint bits, so the XOR term is (lane part) ^
      // (constant part sc).  The writes have sc = 0 (phase 1's pos_c < 8): one
      // address VGPR plus immediates.  The reads are additive only among the
      // elements with the same sc (R = 2^9: all; 2^8: two values; 2^7: four;
      // 2^6: eight, i.e. not at all): one address VGPR per distinct sc.
      auto slot0 = [&](uint32_t p0, int col) -> uint32_t {
        return p0 * kCols + ((uint32_t)col ^ ((p0 >> (LOGR - 3)) & (kCols - 1)));
      };
      __syncthreads();  // (the twiddle copy's writes, before the phase-2 reads of lds_tw)
      static_assert((phase_pos_c(0, Q1, EPT - 1) >> (LOGR - 3)) == 0, "phase 1: constant rows below the swizzle bits");
      fe* wr = &lds[slot0(pos0, c)];
#pragma unroll
      for (int e = 0; e < EPT; ++e) fe_store(wr + phase_pos_c(0, Q1, e) * kCols, x[e]);
      __syncthreads();
      c = cB;
      t = tid / kCols;
      pos0 = pos_lane(ILQ{}, IQ2{});
      const uint32_t rd0 = slot0(pos0, c);
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        const uint32_t pc = phase_pos_c(LQ, Q2, e);
        const uint32_t sc = (pc >> (LOGR - 3)) & (kCols - 1);
        x[e] = fe_load(&lds[(rd0 ^ sc) + pc * kCols]);
      }
      run_phase(ILQ{}, IQ2{});
    } else {
      exchange_and_run(I0{}, IQ1{}, ILQ{}, IQ2{});
    }
    if constexpr (LOGR > 2 * LQ) {
      constexpr int Q3 = LOGR - 2 * LQ;
      static_assert(Q3 <= LQ, "LOGR <= 3 * LQ");
      using I2LQ = std::integral_constant<int, 2 * LQ>;
      using IQ3 = std::integral_constant<int, Q3>;
      if constexpr (kEarly) {
        load_tb();
        if (MLH_P0_EARLY_TB == 1) load_ta0(pos_lane(I2LQ{}, IQ3{}));  // 2: TB only
      }
      exchange_and_run(ILQ{}, IQ2{}, I2LQ{}, IQ3{});
    }
  }

  // ---- epilogue: inter-pass twiddle, store --------------------------------
  if constexpr (!kEarly) {
    load_ta0(pos0);
    load_tb();
  } else if (MLH_P0_EARLY_TB == 2) {
    load_ta0(pos0);
  }
  if constexpr (TW == 0) {
    static_assert(4 * R <= R * kCols, "the expanded TB column fits the exchange tile");
    constexpr int NT = NTt;
    __syncthreads();  // every lane's reads of the exchange tile are done
#pragma unroll
    for (int e = 0; e < kTbPerThread; ++e)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        lds[MLH_TB_COALESCED ? (e * 4 + k) * NT + tid : 4 * (e * NT + tid) + k] = tbv[e][k];
    __syncthreads();
  }
  // the lane's byte offset into the output tile (rows rshift apart, the 8
  // columns cshift apart); row pos_c(e) goes to the base
  Off st_lane = (((Off)pos0 << rshift) + ((Off)cB << cshift)) << 4;
  auto store_row = [&](int e) {
    fe_store_at<Off>(tile_out + ((uint64_t)pos_c(e) << rshift), st_lane, x[e]);
  };
  if constexpr (TW == 5) {
    constexpr int Q3 = LOGR - 2 * LQ, NI = 1 << Q3, G = EPT / NI;
    static_assert(LOGR > 2 * LQ && G % 2 == 0, "progression twiddle: groups in pairs");
    // (loaded here: issued before the last register phase instead -- P alone,
    // or P and C with 6 spilled registers -- measured no faster / 8 % slower)
    // P[k0][j] of each group (k0 = pos0 + pos_c(g NI): the group's first row);
    // P has the tile's row stride, so the lane's offset is the store's
    fe tv[G];
#pragma unroll
    for (int gq = 0; gq < G; ++gq)
      tv[gq] = fe_load_at<Off>(ta + jcol0 + ((uint64_t)pos_c(gq * NI) << g.lstride), st_lane);
    const fe* cp = tb + 4 * jcol0;
    const Off c_lane = (Off)cB << 6;
    const fe c0 = fe_load_at<Off>(cp, c_lane), c1 = fe_load_at<Off>(cp + 1, c_lane),
             c2 = fe_load_at<Off>(cp + 2, c_lane), c3 = fe_load_at<Off>(cp + 3, c_lane);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      uint64_t rare;
#pragma unroll
      for (int gq = 0; gq < G; gq += 2) {
        const int e0 = gq * NI + i, e1 = (gq + 1) * NI + i;
        bfly_ff_v(x[e0], tv[gq], x[e1], tv[gq + 1], rare);
        pin_lane_offset(st_lane);
        store_row(e0);
        store_row(e1);
      }
      if (i + 1 < NI) {
#pragma unroll
        for (int gq = 0; gq < G; gq += 2) bfly_pp_v(tv[gq], c0, c1, c2, c3, tv[gq + 1], c0, c1, c2, c3, rare);
      }
    }
  } else if constexpr (!LAST) {
    // w_S^(jrest k) = TA[k][jl] * TB[k][jh]: the 8 columns of a tile are 8
    // consecutive jl, so a wave's lanes read 8 runs of 128 B per table.  The
    // products run two elements per generated asm statement (relaxed result;
    // bfly_asm.hpp), and the next pass takes relaxed input.
    const fe* tb_rows = lds + 4 * pos0;  // the staged TB column: entry of row pos0 + pos_c(e)
#pragma unroll
    for (int e = 0; e < EPT; e += 2) {
      uint64_t rare;
      const fe a0 = ta_c0, a1 = ta_c1;
      if (e + 2 < EPT && MLH_DIAG_TW < 2) {  // the next pair's, in flight during this pair's products
        pin_lane_offset(ta_lane);
        ta_c0 = ta_at(e + 2, ta_lane);
        ta_c1 = ta_at(e + 3, ta_lane);
      }
      bfly_ff_v(x[e], a0, x[e + 1], a1, rare);
      if constexpr (TW == 0 && MLH_DIAG_TW == 0) {
        const fe* b0 = tb_rows + 4 * pos_c(e);
        const fe* b1 = tb_rows + 4 * pos_c(e + 1);
        bfly_pp_v(x[e], b0[0], b0[1], b0[2], b0[3], x[e + 1], b1[0], b1[1], b1[2], b1[3], rare);
      }
      pin_lane_offset(st_lane);
      store_row(e);
      store_row(e + 1);
    }
    (void)tb_rows;
  } else {
    // canonical output, four elements per asm statement
    static_assert(EPT % 4 == 0, "canonicalisation in fours");
#pragma unroll
    for (int e = 0; e < EPT; e += 4) bfly_cccc_v(x[e], x[e + 1], x[e + 2], x[e + 3]);
    // natural index K = k1 + R_1 rev(mid) + (pos << kshift), k1 = k1u + cB:
    // all but (pos0 << kshift) + cB is wave-uniform
    const uint32_t kshift = g.log_n - LOGR;
    const uint64_t kbase_u = k1u + (reverse_mid_digits(g, mid) << g.logr[0]);
    if constexpr (SH) {
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        uint64_t K = kbase_u + cB + ((uint64_t)(pos0 + pos_c(e)) << kshift);
        // drop the rank bits [logr0 - p, logr0) of K
        const uint32_t lo = g.logr[0] - g.sh_p;
        K = ((K >> g.logr[0]) << lo) | (K & ((1ull << lo) - 1));
        fe_store(out + K, x[e]);
      }
    } else {
      const Off k_lane = (((Off)pos0 << kshift) + (Off)cB) << 4;
#pragma unroll
      for (int e = 0; e < EPT; ++e)
        fe_store_at<Off>(out + kbase_u + ((uint64_t)pos_c(e) << kshift), k_lane, x[e]);
    }
  }
  (void)store_row;
  (void)st_lane;
  (void)ld_lane;
  (void)jrest;
  (void)TPC;
}

template <int LOGR, int TW, int ZT, int EPT = kEPT>
__global__ void __launch_bounds__(kCols * (1 << LOGR) / EPT,
                                  (TW == 2 || TW == 4) ? 1 : pass_waves_per_simd(LOGR, EPT))
ntt_pass_kernel(const fe* in, fe* out, const fe* __restrict__ tw,
                const fe* __restrict__ ta, const fe* __restrict__ tb, PassGeom g) {
  ntt_pass_body<LOGR, TW, ZT, EPT, false>(in, out, tw, ta, tb, g);
}

template <int LOGR, int TW, int ZT, int EPT = kEPT>
__global__ void __launch_bounds__(kCols * (1 << LOGR) / EPT,
                                  (TW == 2 || TW == 4) ? 1 : pass_waves_per_simd(LOGR, EPT))
ntt_pass_wide_kernel(const fe* in, fe* out, const fe* __restrict__ tw,
                     const fe* __restrict__ ta, const fe* __restrict__ tb, PassGeom g) {
  ntt_pass_body<LOGR, TW, ZT, EPT, true>(in, out, tw, ta, tb, g);
}

// Single-workgroup NTT for N <= 2^10: LDS-resident radix-2 DIT.
__global__ void __launch_bounds__(512)
ntt_small_kernel(const fe* __restrict__ in, fe* __restrict__ out, const fe* __restrict__ tw,
                 uint32_t log_n, uint32_t in_len, fe scale, int apply_scale, int brev_in) {
  __shared__ fe lds[1024];
  const uint32_t N = 1u << log_n;
  in += (uint64_t)blockIdx.x * in_len;
  out += (uint64_t)blockIdx.x * N;
  for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) {
    const uint32_t src = bitrev(i, (int)log_n);
    // brev_in: coefficient src is stored at bitrev_{log2 in_len}(src) (ZT == 2)
    const uint32_t at = (brev_in && in_len > 1) ? bitrev(src, 31 - __builtin_clz(in_len)) : src;
    lds[i] = src < in_len ? fe_load(in + at) : fe_zero();
  }
  __syncthreads();
  for (uint32_t s = 0; s < log_n; ++s) {
    const uint32_t h = 1u << s;
    for (uint32_t b = threadIdx.x; b < N / 2; b += blockDim.x) {
      const uint32_t j = b & (h - 1);
      const uint32_t p0 = j + ((b >> s) << (s + 1));
      const fe u = lds[p0];
      fe v = lds[p0 + h];
      if (j) v = fe_mul(v, tw[j << (log_n - 1 - s)]);
      lds[p0] = fe_add(u, v);
      lds[p0 + h] = fe_sub(u, v);
    }
    __syncthreads();
  }
  for (uint32_t i = threadIdx.x; i < N; i += blockDim.x) {
    fe v = lds[i];
    if (apply_scale) v = fe_mul(v, scale);
    fe_store(out + i, v);
  }
}

// table[t] = base^t * scale, t < count (twiddle tables; one-time per context).
// expand: entry t is the 4 limb-shifted multiples v * 2^(32k) (fe_mul_pre).
__global__ void pow_table_kernel(fe* __restrict__ out, fe base, fe scale, uint64_t count,
                                 int expand) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  fe v = fe_pow(base, t);
  v = fe_mul(v, scale);
  if (!expand) {
    fe_store(out + t, v);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    fe_store(out + 4 * t + k, v);
    v = fe_mul(v, fe{{0u, 1u, 0u, 0u}});  // * 2^32
  }
}

// 2D table out[k * cols + j] = base^(k * j * mult) * scale (inter-pass twiddles).
// expand: entry t is the 4 limb-shifted multiples (fe_mul_pre), as pow_table.
__global__ void pow_table2d_kernel(fe* __restrict__ out, fe base, fe scale, uint64_t rows,
                                   uint64_t cols, uint64_t mult, int expand) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * cols) return;
  const uint64_t k = t / cols, j = t % cols;
  fe v = fe_mul(fe_pow(base, k * j * mult), scale);
  if (!expand) {
    fe_store(out + t, v);
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    fe_store(out + 4 * t + q, v);
    v = fe_mul(v, fe{{0u, 1u, 0u, 0u}});  // * 2^32
  }
}

hipError_t launch_pow_table2d(fe* out, fe base, fe scale, uint64_t rows, uint64_t cols,
                              uint64_t mult, hipStream_t st, bool expand) {
  const uint64_t n = rows * cols;
  hipLaunchKernelGGL(pow_table2d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out,
                     base, scale, rows, cols, mult, expand ? 1 : 0);
  return hipGetLastError();
}

// gen_pows[i] = g^i for i < count (NttField::pow_2_generator_powers,
// src/ntt/mod.rs:18-28): block-base x in-block power, no serial chain.
__global__ void pow_series_kernel(fe* __restrict__ out, const fe* __restrict__ tlo,
                                  const fe* __restrict__ thi, uint64_t count) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  fe_store(out + t, fe_mul(tlo[t & 4095], thi[t >> 12]));
}

// mlh_gen_pows_verify: gp[t] (t < count, table index base + t) against
// g^(base + t); the smallest mismatching index to *bad (initialised ~0).
__global__ void pow_series_check_kernel(const fe* __restrict__ gp, uint64_t base, uint64_t count,
                                        const fe* __restrict__ tlo, const fe* __restrict__ thi,
                                        unsigned long long* bad) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint64_t i = base + t;
  const fe want = fe_mul(tlo[i & 4095], thi[i >> 12]);
  const fe got = fe_load(gp + t);
  if ((want.w[0] ^ got.w[0]) | (want.w[1] ^ got.w[1]) | (want.w[2] ^ got.w[2]) | (want.w[3] ^ got.w[3]))
    atomicMin(bad, (unsigned long long)i);
}

// ---- general-generator network --------------------------------------------
// Polynomial::ntt / LagrangePolynomial::intt (src/ntt/mod.rs:69-110, :132-173)
// for a generator whose order is not exactly N.  The reference's loop --
// bit-reverse, then stage len = 4..N with butterflies u +- v * g_len^j,
// g_len = gen^(N/len) -- is then a well-defined linear map but no DFT: with
// gen^(N/2) != -1, "u - w v" is not "u + w' v" for any power w', so the
// four-step passes above (which rely on that) cannot reproduce it.  These
// kernels run the same butterfly network stage by stage: the first kNetLB
// stages per LDS-resident block of 2^kNetLB positions, the rest up to 4 per
// launch in registers.  w^t (t < N/2) = tlo[t mod 2^12] * thi[t >> 12] (two
// small tables instead of one of N/2 entries, which would be 32 GiB at 2^32);
// stage s (len = 2^(s+1)) uses w^(j << (log_n - 1 - s)) = g_len^j, the
// reference's gen_pows[j] (exact: the field is exact, however the power is
// formed).  Correctness path, not tuned.
constexpr uint32_t kNetLB = 11;  // 2^11 entries = 32 KiB of LDS

__device__ __forceinline__ fe net_tw(const fe* __restrict__ tlo, const fe* __restrict__ thi,
                                     uint64_t t) {
  const uint64_t lo = t & 4095, hi = t >> 12;
  if (!hi) return fe_load(tlo + lo);
  if (!lo) return fe_load(thi + hi);
  return fe_mul(fe_load(tlo + lo), fe_load(thi + hi));
}

__device__ __forceinline__ uint64_t bitrev64(uint64_t x, uint32_t bits) {
  return bits ? __builtin_bitreverse64(x) >> (64 - bits) : 0;
}

// zero_top: 0 = N inputs; 1 = N/2 inputs, the rest zero (reed_solomon's
// resize, fri/mod.rs:19-28); 2 = as 1, coefficient c stored at
// in[bitrev_{log_n - 1}(c)].
__global__ void __launch_bounds__(1024)
ntt_net_block_kernel(const fe* __restrict__ in, fe* __restrict__ out, const fe* __restrict__ tlo,
                     const fe* __restrict__ thi, uint32_t log_n, uint32_t lb, int zero_top, fe scale, int apply_scale) {
  __shared__ fe lds[1u << kNetLB];
  const uint32_t B = 1u << lb;
  const uint64_t N = 1ull << log_n, base = (uint64_t)blockIdx.x << lb;
  for (uint32_t i = threadIdx.x; i < B; i += blockDim.x) {
    const uint64_t src = bitrev64(base + i, log_n);  // bit_reverse_permutation (ntt/mod.rs:113-123)
    fe v;
    if (zero_top == 0) v = fe_load(in + src);
    else if (src >= N / 2) v = fe_zero();
    else v = fe_load(in + (zero_top == 2 ? bitrev64(src, log_n - 1) : src));
    lds[i] = v;
  }
  __syncthreads();
  for (uint32_t s = 0; s < lb; ++s) {
    const uint32_t h = 1u << s;
    for (uint32_t b = threadIdx.x; b < B / 2; b += blockDim.x) {
      const uint32_t j = b & (h - 1);
      const uint32_t p0 = j + ((b >> s) << (s + 1));
      const fe u = lds[p0];
      fe v = lds[p0 + h];
      if (j) v = fe_mul(v, net_tw(tlo, thi, (uint64_t)j << (log_n - 1 - s)));  // gen_pows[0] = 1
      lds[p0] = fe_add(u, v);
      lds[p0 + h] = fe_sub(u, v);
    }
    __syncthreads();
  }
  for (uint32_t i = threadIdx.x; i < B; i += blockDim.x) {
    fe v = lds[i];
    if (apply_scale) v = fe_mul(v, scale);
    fe_store(out + base + i, v);
  }
}

// Stages s0 .. s0 + Q - 1 (s0 >= kNetLB): each thread owns the 2^Q positions
// base + m 2^s0 (m < 2^Q) that these stages couple; consecutive threads take
// consecutive low bits, so every load and store is a contiguous wave run.
// Runs in place (in == out) or out of place.
template <int Q>
__global__ void __launch_bounds__(256)
ntt_net_stage_kernel(const fe* in, fe* out, const fe* __restrict__ tlo, const fe* __restrict__ thi,
                     uint32_t log_n,
                     uint32_t s0, fe scale, int apply_scale) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (1ull << (log_n - Q))) return;
  const uint64_t low = g & ((1ull << s0) - 1);
  const uint64_t base = ((g >> s0) << (s0 + Q)) | low;
  fe x[1 << Q];
#pragma unroll
  for (int m = 0; m < (1 << Q); ++m) x[m] = fe_load(in + base + ((uint64_t)m << s0));
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const uint32_t s = s0 + q;
    const int d = 1 << q;
#pragma unroll
    for (int b = 0; b < (1 << (Q - 1)); ++b) {
      const int m = ((b >> q) << (q + 1)) | (b & (d - 1));  // pairs (m, m + d)
      const uint64_t j = (base + ((uint64_t)m << s0)) & ((1ull << s) - 1);
      const fe v = j ? fe_mul(x[m + d], net_tw(tlo, thi, j << (log_n - 1 - s))) : x[m + d];
      const fe u = x[m];
      x[m] = fe_add(u, v);
      x[m + d] = fe_sub(u, v);
    }
  }
#pragma unroll
  for (int m = 0; m < (1 << Q); ++m) {
    fe v = x[m];
    if (apply_scale) v = fe_mul(v, scale);
    fe_store(out + base + ((uint64_t)m << s0), v);
  }
}

hipError_t launch_ntt_network(const fe* in, fe* out, fe* scratch, const fe* tlo, const fe* thi,
                              uint32_t log_n,
                              int zero_top, fe scale, bool apply_scale, hipStream_t st) {
  if (log_n < 1 || log_n > 40 || (zero_top && in == out)) return hipErrorInvalidValue;
  const uint32_t lb = log_n < kNetLB ? log_n : kNetLB;
  const uint64_t blocks = 1ull << (log_n - lb);
  // the block pass gathers bit-reversed positions from all of `in`: out of
  // place whenever it has more than one block
  fe* first = (in == out && blocks > 1) ? scratch : out;
  const bool only = lb == log_n;
  const uint32_t threads = lb >= 11 ? 1024 : (1u << lb) / 2 < 64 ? 64 : (1u << lb) / 2;
  hipLaunchKernelGGL(ntt_net_block_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, in, first,
                     tlo, thi, log_n, lb, zero_top, scale, (only && apply_scale) ? 1 : 0);
  hipError_t e = hipGetLastError();
  for (uint32_t s0 = lb; e == hipSuccess && s0 < log_n;) {
    const uint32_t q = log_n - s0 < 4 ? log_n - s0 : 4;
    const bool last = s0 + q == log_n;
    fe* dst = last ? out : first;
    const int sc = (last && apply_scale) ? 1 : 0;
    const dim3 grid((unsigned)(((1ull << (log_n - q)) + 255) / 256)), blk(256);
    switch (q) {
      case 1: hipLaunchKernelGGL(ntt_net_stage_kernel<1>, grid, blk, 0, st, first, dst, tlo, thi, log_n, s0, scale, sc); break;
      case 2: hipLaunchKernelGGL(ntt_net_stage_kernel<2>, grid, blk, 0, st, first, dst, tlo, thi, log_n, s0, scale, sc); break;
      case 3: hipLaunchKernelGGL(ntt_net_stage_kernel<3>, grid, blk, 0, st, first, dst, tlo, thi, log_n, s0, scale, sc); break;
      default: hipLaunchKernelGGL(ntt_net_stage_kernel<4>, grid, blk, 0, st, first, dst, tlo, thi, log_n, s0, scale, sc); break;
    }
    e = hipGetLastError();
    s0 += q;
  }
  return e;
}

// ---- host-side launchers ---------------------------------------------------

template <int LOGR, int EPT>
static hipError_t launch_pass_ept(bool last, int zero_top, const fe* in, fe* out, const fe* tw,
                                  const fe* ta, const fe* tb, const PassGeom& g, uint64_t tiles,
                                  hipStream_t st, bool geo, bool wide) {
  constexpr int threads = kCols * (1 << LOGR) / EPT;
  const dim3 grid((unsigned)tiles), blk(threads);
#define MLH_PASS(TWV, ZTV)                                                                        \
  do {                                                                                            \
    if (wide)                                                                                     \
      hipLaunchKernelGGL((ntt_pass_wide_kernel<LOGR, TWV, ZTV, EPT>), grid, blk, MLH_LDS_PAD, st, \
                         in, out, tw, ta, tb, g);                                                 \
    else                                                                                          \
      hipLaunchKernelGGL((ntt_pass_kernel<LOGR, TWV, ZTV, EPT>), grid, blk, MLH_LDS_PAD,          \
                         st, in, out, tw, ta, tb, g);                                             \
  } while (0)
  if (last) {
    if (zero_top) return hipErrorInvalidValue;  // pass 0 is never the last pass here
    MLH_PASS(2, 0);
  } else if (geo) {  // TW 5 (pass 0, LOGR 7 / 8; ta = P, tb = C)
    if constexpr ((LOGR == 7 || LOGR == 8) && EPT == 8) {
      if (zero_top == 2) MLH_PASS(5, 2);
      else if (zero_top == 1) MLH_PASS(5, 1);
      else MLH_PASS(5, 0);
    } else {
      return hipErrorInvalidValue;
    }
  } else if (!tb && g.p == 0) {  // TW 3: as 1, a distinct kernel for the first pass
    if (zero_top == 2) MLH_PASS(3, 2);
    else if (zero_top == 1) MLH_PASS(3, 1);
    else MLH_PASS(3, 0);
  } else if (!tb) {
    if (zero_top) return hipErrorInvalidValue;  // only pass 0 has an implicit zero half
    MLH_PASS(1, 0);
  } else {
    if (zero_top == 2) MLH_PASS(0, 2);
    else if (zero_top == 1) MLH_PASS(0, 1);
    else MLH_PASS(0, 0);
  }
#undef MLH_PASS
  return hipGetLastError();
}

// EPT = 8 throughout: 16 elements per thread (4-stage register phases, one
// LDS exchange fewer at R = 2^8) measured 23 % slower for a 2^24 NTT -- 190
// VGPRs leave 2 waves per SIMD against 5, and the extra ILP does not cover it.
template <int LOGR>
static hipError_t launch_pass(bool last, int zero_top, const fe* in, fe* out, const fe* tw,
                              const fe* ta, const fe* tb, const PassGeom& g, uint64_t tiles,
                              hipStream_t st, bool geo, bool wide) {
  return launch_pass_ept<LOGR, kEPT>(last, zero_top, in, out, tw, ta, tb, g, tiles, st, geo, wide);
}

// Whether a pass needs 64-bit per-lane offsets: its largest byte offset from a
// wave-uniform base reaches 2^32.  A pass before the last spans its tile, R
// rows 2^lstride elements apart (its tables are smaller: TA at most
// 2^kFullTwLog entries, TB R * W / 2^loga expanded ones, the progression 64 W);
// the last pass's natural-order stores span the vector.  So 2^28 is the
// largest transform whose first and last passes take the narrow form.
static bool pass_wide(const NttTables& tb, uint32_t log_n, uint32_t lr, uint32_t lstride, bool last) {
  if (tb.wide_offsets) return true;
  return (last ? log_n : lr + lstride) + 4 > 32;
}

void ntt_plan_radices(uint32_t log_n, uint32_t* nradix, uint32_t* logr, const uint32_t* forced,
                      uint32_t nforced) {
  // A forced plan (mlh_set_ntt_plan: digits 4..9 summing to log_n) lets the
  // tests check every pass shape at oracle-sized N; otherwise the default.
  if (forced && nforced >= 2 && nforced <= (uint32_t)kMaxPasses) {
    uint32_t sum = 0;
    bool ok = true;
    for (uint32_t i = 0; i < nforced; ++i) {
      ok = ok && forced[i] >= 4 && forced[i] <= 9;
      sum += forced[i];
    }
    if (ok && sum == log_n) {
      *nradix = nforced;
      for (uint32_t i = 0; i < nforced; ++i) logr[i] = forced[i];
      return;
    }
  }
  const uint32_t P = (log_n + 8) / 9;  // ceil(log_n / 9)
  *nradix = P;
  uint32_t rem = log_n;
  for (uint32_t p = 0; p < P; ++p) {
    const uint32_t left = P - p;
    const uint32_t r = (rem + left - 1) / left;  // larger digits first
    logr[p] = r;
    rem -= r;
  }
}

hipError_t launch_ntt_small(const fe* in, fe* out, const fe* tw, uint32_t log_n, uint64_t in_len,
                            fe scale, bool apply_scale, hipStream_t st, uint64_t batch,
                            bool brev_in) {
  const uint32_t N = 1u << log_n;
  const uint32_t threads = N / 2 < 64 ? 64 : (N / 2 > 512 ? 512 : N / 2);
  hipLaunchKernelGGL(ntt_small_kernel, dim3((unsigned)batch), dim3(threads), 0, st, in, out, tw, log_n,
                     (uint32_t)in_len, scale, apply_scale ? 1 : 0, brev_in ? 1 : 0);
  return hipGetLastError();
}

void ntt_pass_label(const NttTables& tb, uint32_t p, int zero_top, char* buf, size_t n) {
  const bool last = p + 1 == tb.nradix;
  const int tw = last ? 2 : (tb.gp[p] ? 5 : (tb.tb[p] ? 0 : (p == 0 ? 3 : 1)));
  snprintf(buf, n, "ntt_pass<%u,%d,%d>", tb.logr[p], tw, p == 0 ? zero_top : 0);
}

hipError_t launch_ntt_passes(const fe* in, fe* out, fe* scratch, const NttTables& tb,
                             uint32_t log_n, int zero_top, hipStream_t st, hipEvent_t* ev,
                             uint64_t batch) {
  PassGeom g;
  g.log_n = log_n;
  g.nradix = tb.nradix;
  for (uint32_t p = 0; p < tb.nradix; ++p) g.logr[p] = tb.logr[p];
  const uint64_t N = 1ull << log_n;
  uint64_t W = N;
  for (uint32_t p = 0; p < tb.nradix; ++p) {
    const uint32_t lr = tb.logr[p];
    W >>= lr;
    g.p = p;
    g.lstride = (uint32_t)__builtin_ctzll(W);
    g.loga = tb.loga[p];
    const bool last = (p + 1 == tb.nradix);
    g.ltpv = log_n - kLogCols - lr;
    const uint64_t tiles = (N >> (kLogCols + lr)) * batch;
    g.lin_v = (p == 0 && zero_top) ? log_n - 1 : log_n;
    g.lout_v = log_n;
    // pass 0: in -> scratch; middle passes in place on scratch; the last pass
    // (a digit-reversal permutation of its tiles) scratch -> out.  The last
    // pass can never run in place: a block would overwrite tiles that other,
    // not yet resident, blocks still have to read.
    const fe* src = (p == 0) ? in : scratch;
    fe* dst = last ? out : scratch;
    const int zt = p == 0 ? zero_top : 0;
    if (ev) (void)hipEventRecord(ev[p], st);
    hipError_t e;
    const bool geo = tb.gp[p] != nullptr;  // TW 5: the progression tables instead of TA, TB
    const fe* ta = geo ? tb.gp[p] : tb.ta[p];
    const fe* tbb = geo ? tb.gc[p] : tb.tb[p];
    const bool wide = pass_wide(tb, log_n, lr, g.lstride, last);
    switch (lr) {
      case 4: e = launch_pass<4>(last, zt, src, dst, tb.tw[p], ta, tbb, g, tiles, st, geo, wide); break;
      case 5: e = launch_pass<5>(last, zt, src, dst, tb.tw[p], ta, tbb, g, tiles, st, geo, wide); break;
      case 6: e = launch_pass<6>(last, zt, src, dst, tb.tw[p], ta, tbb, g, tiles, st, geo, wide); break;
      case 7: e = launch_pass<7>(last, zt, src, dst, tb.tw[p], ta, tbb, g, tiles, st, geo, wide); break;
      case 8: e = launch_pass<8>(last, zt, src, dst, tb.tw[p], ta, tbb, g, tiles, st, geo, wide); break;
      case 9: e = launch_pass<9>(last, zt, src, dst, tb.tw[p], ta, tbb, g, tiles, st, geo, wide); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    if (tb.debug_sync) {
      e = hipStreamSynchronize(st);
      if (e != hipSuccess) return e;
    }
  }
  if (ev) (void)hipEventRecord(ev[tb.nradix], st);
  return hipSuccess;
}

// out[k][j] = in[k][j] * rowbase^k (k < rows, j < 2^lcols): an inter-pass
// twiddle table with a per-row factor (the sharded fused NTT's rank twist)
__global__ void __launch_bounds__(256)
scale_rows_kernel(const fe* __restrict__ in, fe* __restrict__ out, uint64_t n, uint32_t lcols, fe rowbase) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t k = i >> lcols;
  fe f = fe_one(), b = rowbase;
  while (k) {
    if (k & 1) f = fe_mul(f, b);
    b = fe_mul(b, b);
    k >>= 1;
  }
  fe_store(out + i, fe_mul(fe_load(in + i), f));
}

hipError_t launch_scale_rows(const fe* in, fe* out, uint64_t rows, uint32_t lcols, fe rowbase,
                             hipStream_t st) {
  const uint64_t n = rows << lcols;
  hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, n,
                     lcols, rowbase);
  return hipGetLastError();
}

hipError_t launch_ntt_passes_pre(const fe* in, fe* out, const NttTables& tb, uint32_t log_n,
                                 uint32_t npasses, hipStream_t st) {
  if (npasses == 0 || npasses >= tb.nradix) return hipErrorInvalidValue;
  PassGeom g;
  g.log_n = log_n;
  g.nradix = tb.nradix;
  for (uint32_t p = 0; p < tb.nradix; ++p) g.logr[p] = tb.logr[p];
  const uint64_t N = 1ull << log_n;
  uint64_t W = N;
  for (uint32_t p = 0; p < npasses; ++p) {
    const uint32_t lr = tb.logr[p];
    W >>= lr;
    g.p = p;
    g.lstride = (uint32_t)__builtin_ctzll(W);
    g.loga = tb.loga[p];
    g.ltpv = log_n - kLogCols - lr;
    g.lin_v = g.lout_v = log_n;
    const uint64_t tiles = N >> (kLogCols + lr);
    const fe* src = p == 0 ? in : out;  // pass 0: in -> out; then in place on out
    const bool wide = pass_wide(tb, log_n, lr, g.lstride, false);
    hipError_t e;
    switch (lr) {
      case 4: e = launch_pass<4>(false, 0, src, out, tb.tw[p], tb.ta[p], tb.tb[p], g, tiles, st, false, wide); break;
      case 5: e = launch_pass<5>(false, 0, src, out, tb.tw[p], tb.ta[p], tb.tb[p], g, tiles, st, false, wide); break;
      case 6: e = launch_pass<6>(false, 0, src, out, tb.tw[p], tb.ta[p], tb.tb[p], g, tiles, st, false, wide); break;
      case 7: e = launch_pass<7>(false, 0, src, out, tb.tw[p], tb.ta[p], tb.tb[p], g, tiles, st, false, wide); break;
      case 8: e = launch_pass<8>(false, 0, src, out, tb.tw[p], tb.ta[p], tb.tb[p], g, tiles, st, false, wide); break;
      case 9: e = launch_pass<9>(false, 0, src, out, tb.tw[p], tb.ta[p], tb.tb[p], g, tiles, st, false, wide); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_ntt_shard_last(const fe* recv, fe* out, const fe* tw, const uint32_t* logr,
                                 uint32_t nradix, uint32_t log_n, uint32_t log_p, uint32_t rank,
                                 hipStream_t st) {
  if (nradix < 2 || nradix > (uint32_t)kMaxPasses) return hipErrorInvalidValue;
  const uint32_t lr = logr[nradix - 1];
  if (lr < log_p + 3 || logr[0] < kLogCols + log_p) return hipErrorInvalidValue;
  PassGeom g;
  g.log_n = log_n;
  g.nradix = nradix;
  for (uint32_t p = 0; p < nradix; ++p) g.logr[p] = logr[p];
  g.p = nradix - 1;
  g.lstride = 0;
  g.loga = 0;
  g.ltpv = log_n - kLogCols - lr - log_p;  // this rank's tiles
  g.lin_v = g.lout_v = log_n;
  g.sh_p = log_p;
  g.sh_rank = rank;
  g.sh_lchunk = log_n - 2 * log_p;
  const dim3 grid((unsigned)(1ull << g.ltpv));
#define MLH_SHL(LR)                                                                                 \
  hipLaunchKernelGGL((ntt_pass_kernel<LR, 4, 0, kEPT>), grid, dim3(kCols * (1 << LR) / kEPT), MLH_LDS_PAD, \
                     st, recv, out, tw, nullptr, nullptr, g)
  switch (lr) {
    case 6: MLH_SHL(6); break;
    case 7: MLH_SHL(7); break;
    case 8: MLH_SHL(8); break;
    case 9: MLH_SHL(9); break;
    default: return hipErrorInvalidValue;
  }
#undef MLH_SHL
  return hipGetLastError();
}

hipError_t launch_pow_table(fe* out, fe base, fe scale, uint64_t count, hipStream_t st,
                            bool expand) {
  const unsigned blocks = (unsigned)((count + 255) / 256);
  hipLaunchKernelGGL(pow_table_kernel, dim3(blocks), dim3(256), 0, st, out, base, scale, count,
                     expand ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_pow_series(fe* out, const fe* tlo, const fe* thi, uint64_t count,
                             hipStream_t st) {
  const unsigned blocks = (unsigned)((count + 255) / 256);
  hipLaunchKernelGGL(pow_series_kernel, dim3(blocks), dim3(256), 0, st, out, tlo, thi, count);
  return hipGetLastError();
}

hipError_t launch_pow_series_check(const fe* gp, uint64_t base, uint64_t count, const fe* tlo,
                                   const fe* thi, unsigned long long* bad, hipStream_t st) {
  if (count == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((count + 255) / 256);
  hipLaunchKernelGGL(pow_series_check_kernel, dim3(blocks), dim3(256), 0, st, gp, base, count, tlo,
                     thi, bad);
  return hipGetLastError();
}

}  // namespace mlh
