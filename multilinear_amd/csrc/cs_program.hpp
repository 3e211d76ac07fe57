// Constraint programs: the straight-line form of the reference's
// Expr<F>(fn(&[F], &[F]) -> F) (constraint_system/constraints.rs:3-10) and
// ConstraintSet::evaluate (evaluation.rs:21-29).  One decoder (cs_decode) for
// the wire format of include/mlhip.h, one decoded form (CsProgram) and its
// device image (CsImage: the words cs_sumcheck.hip's interpreter reads), and
// the host interpreter (cs_host_eval) the verifier uses.  Plain C++: no HIP
// dependency, so verify.cpp keeps building for the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "host_field.hpp"

namespace mlh {

// wire / decoded opcodes and operand kinds (include/mlhip.h)
enum : uint8_t { kCsAdd = 0, kCsSub = 1, kCsMul = 2, kCsNeg = 3, kCsInv = 4 /* fill programs only */ };
enum : uint8_t { kCsCol = 0, kCsRand = 1, kCsConst = 2, kCsTemp = 3 };

constexpr uint32_t kCsMaxWidth = 32, kCsMaxTemps = 32, kCsMaxConsts = 64, kCsMaxRandoms = 64;
constexpr uint32_t kCsMaxConstraints = 256, kCsMaxInstr = 4096, kCsMaxDegree = 7;
constexpr uint32_t kCsHeaderBytes = 28, kCsInstrBytes = 8, kCsOperandBytes = 2;
constexpr uint32_t kCsMaxLogHeight = 32;

// Device operand: bit 15 set = a wave-uniform value, index into the uniform
// pool [randoms | consts | mask]; clear = a per-lane LDS slot, columns first
// (slot j = column j's value at the current X), then temps (width + t).
constexpr uint32_t kCsUniform = 0x8000u;

struct CsOperand {
  uint8_t kind, index;
};
struct CsInstr {
  uint8_t op, dst;
  CsOperand a, b;
};

struct CsProgram {
  uint32_t width = 0, n_randoms = 0, n_consts = 0, n_temps = 0, n_instr = 0, n_constraints = 0;
  uint32_t degree = 0;
  std::vector<u128> consts;
  std::vector<CsInstr> instr;
  std::vector<CsOperand> outs;
  // inverse Vandermonde matrix of the points 0..degree+1 (row k = coefficient
  // k's weights on the evaluations): the exact interpolation of
  // PolynomialEvals::interpolate (polynomials.rs:51-87) as one product
  std::vector<u128> vinv;
  uint32_t points() const { return degree + 1; }  // D: X = 1..D (sumcheck.rs:159,185)
};

static inline uint32_t cs_rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// (n+1) x (n+1) inverse Vandermonde of the points 0..n: column j holds the
// coefficients of the Lagrange basis polynomial L_j.
static inline std::vector<u128> cs_inverse_vandermonde(uint32_t n) {
  const uint32_t N = n + 1;
  std::vector<u128> out((size_t)N * N, 0);
  for (uint32_t j = 0; j < N; ++j) {
    std::vector<u128> lj(1, 1);
    u128 denom = 1;
    for (uint32_t m = 0; m < N; ++m) {
      if (m == j) continue;
      std::vector<u128> nx(lj.size() + 1, 0);  // lj *= (x - m)
      for (size_t i = 0; i < lj.size(); ++i) {
        nx[i] = h_sub(nx[i], h_mul(lj[i], (u128)m));
        nx[i + 1] = h_add(nx[i + 1], lj[i]);
      }
      lj.swap(nx);
      denom = h_mul(denom, h_sub((u128)j, (u128)m));
    }
    const u128 s = h_inv(denom);
    for (uint32_t k = 0; k < N; ++k) out[(size_t)k * N + j] = h_mul(lj[k], s);
  }
  return out;
}

// The constant pool of a wire-format program (constraint or fill): canonical
// elements; q ends behind it.
static inline bool cs_read_consts(const uint8_t*& q, uint32_t n, std::vector<u128>& out) {
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i, q += 16)
    if ((out[i] = h_load(q)) >= kModulus) return false;
  return true;
}

// Operand and instruction validation of both program kinds: index ranges, a
// temp read before it is written, reserved bytes, the formal degree of every
// temp (column 1, random / const 0, add / sub / neg / inv max, mul sum) and
// whether its value depends on the result of an INV (`tainted`: a property of
// the value a slot holds, updated at every write, since temps are reused).
struct CsCodeCheck {
  uint32_t width, n_randoms, n_consts, n_temps;
  uint32_t tdeg[kCsMaxTemps];
  bool twritten[kCsMaxTemps] = {}, ttaint[kCsMaxTemps] = {};
  bool ok = true;
  bool last_tainted = false;  // of the instruction instr() saw last
  CsCodeCheck(uint32_t w, uint32_t r, uint32_t c, uint32_t t)
      : width(w), n_randoms(r), n_consts(c), n_temps(t) {}
  uint32_t opdeg(const CsOperand& o) {
    switch (o.kind) {
      case kCsCol: ok = ok && o.index < width; return 1;
      case kCsRand: ok = ok && o.index < n_randoms; return 0;
      case kCsConst: ok = ok && o.index < n_consts; return 0;
      case kCsTemp:
        ok = ok && o.index < n_temps && twritten[o.index];  // read before written
        return ok ? tdeg[o.index] : 0;
      default: ok = false; return 0;
    }
  }
  bool tainted(const CsOperand& o) const { return o.kind == kCsTemp && ok && ttaint[o.index]; }
  // One 8-byte instruction; an op above max_op is rejected.
  bool instr(const uint8_t* q, uint8_t max_op, CsInstr& out) {
    const CsInstr in{q[0], q[1], {q[2], q[3]}, {q[4], q[5]}};
    if (in.op > max_op || in.dst >= n_temps || q[6] || q[7]) return false;
    const uint32_t da = opdeg(in.a);
    uint32_t d = da;
    bool t = tainted(in.a);
    if (in.op == kCsNeg || in.op == kCsInv) {
      if (in.b.kind || in.b.index) return false;  // NEG, INV: b is (0, 0)
      if (in.op == kCsInv) {
        if (t) return false;  // inverse depth 1
        t = true;
      }
    } else {
      const uint32_t db = opdeg(in.b);
      d = in.op == kCsMul ? da + db : (da > db ? da : db);
      t = t || tainted(in.b);
    }
    if (!ok) return false;
    tdeg[in.dst] = d > 0xFFFFu ? 0xFFFFu : d;  // (saturating: any such value exceeds degree)
    twritten[in.dst] = true;
    ttaint[in.dst] = last_tainted = t;
    out = in;
    return true;
  }
};

// Decode and validate a wire-format program; false = MLH_ERR_INVALID.
static inline bool cs_decode(const uint8_t* b, uint64_t len, CsProgram& p) {
  if (!b || len < kCsHeaderBytes) return false;
  p.width = cs_rd32(b);
  p.n_randoms = cs_rd32(b + 4);
  p.n_consts = cs_rd32(b + 8);
  p.n_temps = cs_rd32(b + 12);
  p.n_instr = cs_rd32(b + 16);
  p.n_constraints = cs_rd32(b + 20);
  p.degree = cs_rd32(b + 24);
  if (p.width < 1 || p.width > kCsMaxWidth || p.n_randoms > kCsMaxRandoms ||
      p.n_consts > kCsMaxConsts || p.n_temps > kCsMaxTemps || p.n_instr > kCsMaxInstr ||
      p.n_constraints < 1 || p.n_constraints > kCsMaxConstraints || p.degree < 1 ||
      p.degree > kCsMaxDegree)
    return false;
  const uint64_t want = (uint64_t)kCsHeaderBytes + 16ull * p.n_consts +
                        (uint64_t)kCsInstrBytes * p.n_instr +
                        (uint64_t)kCsOperandBytes * p.n_constraints;
  if (len != want) return false;  // truncated, or trailing bytes
  const uint8_t* q = b + kCsHeaderBytes;
  if (!cs_read_consts(q, p.n_consts, p.consts)) return false;
  CsCodeCheck chk(p.width, p.n_randoms, p.n_consts, p.n_temps);
  p.instr.resize(p.n_instr);
  for (uint32_t i = 0; i < p.n_instr; ++i, q += kCsInstrBytes)
    if (!chk.instr(q, kCsNeg, p.instr[i])) return false;
  p.outs.resize(p.n_constraints);
  for (uint32_t c = 0; c < p.n_constraints; ++c, q += kCsOperandBytes) {
    p.outs[c] = CsOperand{q[0], q[1]};
    const uint32_t d = chk.opdeg(p.outs[c]);
    if (!chk.ok || d > p.degree) return false;
  }
  p.vinv = cs_inverse_vandermonde(p.degree + 1);
  return true;
}

// The program of the shift reduction (mlhip.h, shifted proof, step 7): the one
// constraint sum_k rand(k) * var(cols[k]) over a width-wide row, declared
// degree 1, written in the wire format and decoded like a caller's program.
// n_shifts 1..width, cols[k] < width; false otherwise.
static inline bool cs_shift_program(uint32_t width, const uint32_t* cols, uint32_t n_shifts,
                                    CsProgram& p) {
  if (!cols || n_shifts < 1 || n_shifts > kCsMaxWidth) return false;
  const uint32_t K = n_shifts, n_instr = 2 * K - 1;
  const uint32_t hdr[7] = {width, K, 0, K > 1 ? 2u : 1u, n_instr, 1, 1};
  std::vector<uint8_t> b;
  for (uint32_t w : hdr)
    for (uint32_t s = 0; s < 32; s += 8) b.push_back((uint8_t)(w >> s));
  for (uint32_t k = 0; k < K; ++k) {
    if (cols[k] >= width) return false;
    const uint8_t mul[8] = {kCsMul, (uint8_t)(k ? 1 : 0), kCsRand, (uint8_t)k, kCsCol, (uint8_t)cols[k], 0, 0};
    b.insert(b.end(), mul, mul + 8);
    if (k) {
      const uint8_t add[8] = {kCsAdd, 0, kCsTemp, 0, kCsTemp, 1, 0, 0};
      b.insert(b.end(), add, add + 8);
    }
  }
  b.push_back(kCsTemp);
  b.push_back(0);
  return cs_decode(b.data(), b.size(), p);
}

// ConstraintSet::evaluate (evaluation.rs:21-29): sum_c mask[c] * out_c(values, randoms).
static inline u128 cs_host_eval(const CsProgram& p, const u128* values, const u128* randoms,
                                const u128* mask) {
  u128 temps[kCsMaxTemps] = {};
  auto get = [&](const CsOperand& o) -> u128 {
    switch (o.kind) {
      case kCsCol: return values[o.index];
      case kCsRand: return randoms[o.index];
      case kCsConst: return p.consts[o.index];
      default: return temps[o.index];
    }
  };
  for (const CsInstr& in : p.instr) {
    const u128 a = get(in.a);
    u128 r;
    switch (in.op) {
      case kCsAdd: r = h_add(a, get(in.b)); break;
      case kCsSub: r = h_sub(a, get(in.b)); break;
      case kCsMul: r = h_mul(a, get(in.b)); break;
      default: r = h_sub(0, a); break;
    }
    temps[in.dst] = r;
  }
  u128 acc = 0;
  for (uint32_t c = 0; c < p.n_constraints; ++c) acc = h_add(acc, h_mul(mask[c], get(p.outs[c])));
  return acc;
}

// ---- device image ------------------------------------------------------------
// 16-byte elements first: uniform pool [randoms | consts | mask], then the
// inverse Vandermonde matrix ((D+1)^2); then 32-bit words: per instruction
// (op | dst slot << 8, a | b << 16), per constraint (out | mask index << 16).
struct CsImageLayout {
  uint32_t n_uni, vinv_off /* elements */, code_off /* bytes */, outs_off /* bytes */, bytes;
};
static inline CsImageLayout cs_image_layout(const CsProgram& p) {
  CsImageLayout l;
  l.n_uni = p.n_randoms + p.n_consts + p.n_constraints;
  l.vinv_off = l.n_uni;
  const uint32_t N = p.degree + 2;
  l.code_off = 16 * (l.n_uni + N * N);
  l.outs_off = l.code_off + 8 * p.n_instr;
  l.bytes = (l.outs_off + 4 * p.n_constraints + 15) & ~15u;
  return l;
}
// (P: CsProgram or FillProgram)
template <class P>
static inline uint32_t cs_dev_operand(const P& p, const CsOperand& o) {
  switch (o.kind) {
    case kCsCol: return o.index;
    case kCsTemp: return p.width + o.index;
    case kCsRand: return kCsUniform | o.index;
    default: return kCsUniform | (p.n_randoms + o.index);
  }
}
static inline std::vector<uint8_t> cs_build_image(const CsProgram& p, const u128* randoms,
                                                  const u128* mask) {
  const CsImageLayout l = cs_image_layout(p);
  std::vector<uint8_t> img(l.bytes, 0);
  uint8_t* q = img.data();
  for (uint32_t i = 0; i < p.n_randoms; ++i, q += 16) h_store(q, randoms[i]);
  for (uint32_t i = 0; i < p.n_consts; ++i, q += 16) h_store(q, p.consts[i]);
  for (uint32_t i = 0; i < p.n_constraints; ++i, q += 16) h_store(q, mask[i]);
  for (u128 v : p.vinv) {
    h_store(q, v);
    q += 16;
  }
  uint32_t* w = reinterpret_cast<uint32_t*>(img.data() + l.code_off);
  for (const CsInstr& in : p.instr) {
    *w++ = (uint32_t)in.op | ((p.width + in.dst) << 8);
    *w++ = cs_dev_operand(p, in.a) | ((in.op == kCsNeg ? 0u : cs_dev_operand(p, in.b)) << 16);
  }
  for (uint32_t c = 0; c < p.n_constraints; ++c)
    *w++ = cs_dev_operand(p, p.outs[c]) | ((p.n_randoms + p.n_consts + c) << 16);
  return img;
}

// Launch shape of the streaming kernels: LDS slots per lane = width (values at
// X) + width (their step hi - lo) + temps + D (running sums); the block is the
// largest of 256 / 128 / 64 threads whose slots fit kCsLdsBytes; a block takes
// at least kCsRowsPerThread row pairs per thread before the grid grows, up to
// kCsMaxBlocks blocks (the partials buffer holds D * kCsMaxBlocks sums).
constexpr uint32_t kCsLdsBytes = 152 * 1024;  // of the CU's 160 KiB (the rest: reduction scratch)
constexpr uint32_t kCsRowsPerThread = 4, kCsMaxBlocks = 512;
static inline uint32_t cs_slots(const CsProgram& p) { return 2 * p.width + p.n_temps + p.points(); }
static inline uint32_t cs_threads(uint32_t slots) {
  uint32_t t = 256;
  while (t > 64 && slots * 16 * t > kCsLdsBytes) t >>= 1;
  return t;
}
static inline uint32_t cs_blocks(uint64_t pairs, uint32_t threads) {
  const uint64_t per = (uint64_t)threads * kCsRowsPerThread;
  uint64_t b = (pairs + per - 1) / per;
  if (b > kCsMaxBlocks) b = kCsMaxBlocks;
  return b ? (uint32_t)b : 1;
}

// ---- fill programs -------------------------------------------------------------
// A per-row program whose outputs go to columns of the same row (include/
// mlhip.h): the constraint-program format with op 4 = INV, outputs (column,
// operand) and no degree.  fill_decode shares cs_decode's validation
// (CsCodeCheck); fill_host_eval is the specification of trace_fill.hip.
constexpr uint32_t kFillMaxInv = 16, kFillOutBytes = 4;
constexpr uint32_t kFillTainted = 1u << 24;  // device code word 0: the value depends on an INV

struct FillOut {
  uint8_t column;
  CsOperand src;
};
struct FillProgram {
  uint32_t width = 0, n_randoms = 0, n_consts = 0, n_temps = 0, n_instr = 0, n_outputs = 0;
  uint32_t n_inv = 0, n_pre = 0 /* instructions up to and including the last INV */, out_mask = 0;
  std::vector<u128> consts;
  std::vector<CsInstr> instr;
  std::vector<uint8_t> tainted;  // per instruction: INV, or an operand depends on one
  std::vector<FillOut> outs;
};

static inline bool fill_decode(const uint8_t* b, uint64_t len, FillProgram& p) {
  if (!b || len < kCsHeaderBytes) return false;
  p.width = cs_rd32(b);
  p.n_randoms = cs_rd32(b + 4);
  p.n_consts = cs_rd32(b + 8);
  p.n_temps = cs_rd32(b + 12);
  p.n_instr = cs_rd32(b + 16);
  p.n_outputs = cs_rd32(b + 20);
  if (p.width < 1 || p.width > kCsMaxWidth || p.n_randoms > kCsMaxRandoms ||
      p.n_consts > kCsMaxConsts || p.n_temps > kCsMaxTemps || p.n_instr > kCsMaxInstr ||
      p.n_outputs < 1 || p.n_outputs > p.width || cs_rd32(b + 24) != 0)
    return false;
  const uint64_t want = (uint64_t)kCsHeaderBytes + 16ull * p.n_consts +
                        (uint64_t)kCsInstrBytes * p.n_instr + (uint64_t)kFillOutBytes * p.n_outputs;
  if (len != want) return false;  // truncated, or trailing bytes
  const uint8_t* q = b + kCsHeaderBytes;
  if (!cs_read_consts(q, p.n_consts, p.consts)) return false;
  CsCodeCheck chk(p.width, p.n_randoms, p.n_consts, p.n_temps);
  p.instr.resize(p.n_instr);
  p.tainted.resize(p.n_instr);
  p.n_inv = p.n_pre = 0;
  for (uint32_t i = 0; i < p.n_instr; ++i, q += kCsInstrBytes) {
    if (!chk.instr(q, kCsInv, p.instr[i])) return false;
    p.tainted[i] = chk.last_tainted;
    if (p.instr[i].op == kCsInv) {
      if (++p.n_inv > kFillMaxInv) return false;
      p.n_pre = i + 1;
    }
  }
  p.outs.resize(p.n_outputs);
  p.out_mask = 0;
  for (uint32_t c = 0; c < p.n_outputs; ++c, q += kFillOutBytes) {
    p.outs[c] = FillOut{q[0], CsOperand{q[1], q[2]}};
    chk.opdeg(p.outs[c].src);
    if (!chk.ok || q[3] || q[0] >= p.width || ((p.out_mask >> q[0]) & 1u)) return false;
    p.out_mask |= 1u << q[0];
  }
  return true;
}

// The row after the fill: every column operand reads `row`, the outputs go to
// `out` (which starts as a copy of row).
static inline void fill_host_eval(const FillProgram& p, const u128* row, const u128* randoms,
                                  u128* out) {
  u128 temps[kCsMaxTemps] = {};
  auto get = [&](const CsOperand& o) -> u128 {
    switch (o.kind) {
      case kCsCol: return row[o.index];
      case kCsRand: return randoms[o.index];
      case kCsConst: return p.consts[o.index];
      default: return temps[o.index];
    }
  };
  for (const CsInstr& in : p.instr) {
    const u128 a = get(in.a);
    u128 r;
    switch (in.op) {
      case kCsAdd: r = h_add(a, get(in.b)); break;
      case kCsSub: r = h_sub(a, get(in.b)); break;
      case kCsMul: r = h_mul(a, get(in.b)); break;
      case kCsNeg: r = h_sub(0, a); break;
      default: r = h_inv(a); break;  // zero -> zero (field.rs:113-118)
    }
    temps[in.dst] = r;
  }
  u128 res[kCsMaxWidth];
  for (uint32_t c = 0; c < p.n_outputs; ++c) res[c] = get(p.outs[c].src);
  for (uint32_t j = 0; j < p.width; ++j) out[j] = row[j];
  for (uint32_t c = 0; c < p.n_outputs; ++c) out[p.outs[c].column] = res[c];
}

// Device image: the uniform pool [randoms | consts] (16-byte elements), then
// 32-bit words: per instruction (op | dst slot << 8 | kFillTainted, a | b <<
// 16; INV: a | inverse index << 16), per output (operand | column << 16).
// Operands as in CsImage (cs_dev_operand).
struct FillImageLayout {
  uint32_t code_off, outs_off, bytes;
};
static inline FillImageLayout fill_image_layout(const FillProgram& p) {
  FillImageLayout l;
  l.code_off = 16 * (p.n_randoms + p.n_consts);
  l.outs_off = l.code_off + 8 * p.n_instr;
  l.bytes = (l.outs_off + 4 * p.n_outputs + 15) & ~15u;
  return l;
}
static inline std::vector<uint8_t> fill_build_image(const FillProgram& p, const u128* randoms) {
  const FillImageLayout l = fill_image_layout(p);
  std::vector<uint8_t> img(l.bytes, 0);
  uint8_t* q = img.data();
  for (uint32_t i = 0; i < p.n_randoms; ++i, q += 16) h_store(q, randoms[i]);
  for (uint32_t i = 0; i < p.n_consts; ++i, q += 16) h_store(q, p.consts[i]);
  uint32_t* w = reinterpret_cast<uint32_t*>(img.data() + l.code_off);
  uint32_t v = 0;
  for (uint32_t i = 0; i < p.n_instr; ++i) {
    const CsInstr& in = p.instr[i];
    *w++ = (uint32_t)in.op | ((p.width + in.dst) << 8) | (p.tainted[i] ? kFillTainted : 0u);
    const uint32_t hi = in.op == kCsInv ? v++ : (in.op == kCsNeg ? 0u : cs_dev_operand(p, in.b));
    *w++ = cs_dev_operand(p, in.a) | (hi << 16);
  }
  for (const FillOut& o : p.outs) *w++ = cs_dev_operand(p, o.src) | ((uint32_t)o.column << 16);
  return img;
}

// Launch shape of the fill kernel (trace_fill.hip): B threads, K rows per
// thread and inversion.  LDS slots per lane = width + temps + n_inv; the K - 1
// prefix products per lane and INV live in a global scratch buffer, n_inv *
// (K - 1) * B elements per block.  B = the largest of 256, 128, 64 whose slots
// fit kCsLdsBytes.  K = the largest of 16, 8, 4, 2, 1 that still leaves
// kFillMinChunks chunks of B * K rows (a wave's K rows are one serial task:
// 2^20 rows at K = 16 are one wave per SIMD of a 256-CU part, with nothing to
// hide its load and LDS latencies behind; two or more per SIMD do), K = 1
// without an INV.  A block loops over chunks once there are more than
// kFillMaxBlocks, or than the blocks whose prefixes fit kFillScratchBytes.
constexpr uint32_t kFillMaxBlocks = 512, kFillMinChunks = 512;
constexpr uint64_t kFillScratchBytes = 64ull << 20;
static inline uint32_t fill_slots(const FillProgram& p) { return p.width + p.n_temps + p.n_inv; }
static inline bool fill_shape_ok(const FillProgram& p, uint32_t B, uint32_t K) {
  return (B == 64 || B == 128 || B == 256) && K >= 1 && K <= 16 && !(K & (K - 1)) &&
         (p.n_inv || K == 1) && (uint64_t)fill_slots(p) * 16 * B <= kCsLdsBytes;
}
static inline uint64_t fill_chunks(uint64_t height, uint32_t B, uint32_t K) {
  const uint64_t per = (uint64_t)B * K;
  return (height + per - 1) / per;
}
static inline void fill_shape(const FillProgram& p, uint64_t height, uint32_t* B, uint32_t* K) {
  uint32_t b = 256, k = p.n_inv ? 16 : 1;
  while (b > 64 && !fill_shape_ok(p, b, 1)) b >>= 1;
  while (k > 1 && fill_chunks(height, b, k) < kFillMinChunks) k >>= 1;
  *B = b;
  *K = k;
}
// elements of prefix scratch per block
static inline uint64_t fill_prefix_elems(const FillProgram& p, uint32_t B, uint32_t K) {
  return (uint64_t)p.n_inv * (K - 1) * B;
}
static inline uint32_t fill_blocks(const FillProgram& p, uint64_t chunks, uint32_t B, uint32_t K) {
  uint64_t cap = kFillMaxBlocks;
  const uint64_t per = 16 * fill_prefix_elems(p, B, K);
  if (per && kFillScratchBytes / per < cap) cap = kFillScratchBytes / per;
  if (cap < 1) cap = 1;
  return chunks < cap ? (uint32_t)chunks : (uint32_t)cap;
}

// Blocks of the column-sum kernel (trace_fill.hip): 256 threads take 16-byte
// elements of whole rows, kSumElemsPerThread each before the grid grows, up to
// kCsMaxBlocks blocks (the partials the one-block reduction reads).
constexpr uint32_t kSumThreads = 256, kSumElemsPerThread = 16;
static inline uint32_t sum_blocks(uint64_t elems) {
  const uint64_t per = (uint64_t)kSumThreads * kSumElemsPerThread;
  const uint64_t b = (elems + per - 1) / per;
  return b > kCsMaxBlocks ? kCsMaxBlocks : (b ? (uint32_t)b : 1);
}

}  // namespace mlh

struct mlh_cs_program {
  mlh::CsProgram p;
};
struct mlh_fill_program {
  mlh::FillProgram p;
};
