// Public columns: the columns of a trace that have a short description, which
// the prover neither commits nor opens and whose multilinear extensions the
// verifier evaluates itself (include/mlhip.h).  One decoder
// (pc_decode) for the wire format of include/mlhip.h, the decoded form
// (PublicColumns), the closed-form evaluator (pc_evaluate) the verifier uses
// and the device image (pc_build_image: the words trace_public.hip reads).
// Plain C++: no HIP dependency, so verify.cpp keeps building for the host
// sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "host_field.hpp"
#include "host_sha256.hpp"

namespace mlh {

enum : uint32_t { kPcConst = 0, kPcFirst = 1, kPcLast = 2, kPcRow = 3, kPcPeriodic = 4, kPcSparse = 5 };

constexpr uint32_t kPcMaxColumns = 16, kPcMaxLogPeriod = 16, kPcMaxSparse = 4096;
constexpr uint32_t kPcMaxLogHeight = 32;
// The device image, in 16-byte words: two per column slot -- {kind, period
// mask, table offset, sparse range} and the constant (zero unless CONST) --
// for all kPcMaxColumns slots, then the periodic tables, then two per sparse
// entry -- {row low, row high, column of the strip, 0} and the value, column
// after column and by ascending row within one.  The sparse range of a SPARSE
// column is the index of its first entry | its count << 16 (zero otherwise).  A column that
// is not periodic has mask 0 and its own constant word as its table, so that
// word (off + (row & mask)) is the element's base value for every kind.
constexpr uint32_t kPcDescWords = 2 * kPcMaxColumns;

struct PublicColumn {
  uint32_t kind = 0, arg = 0;
  std::vector<u128> values;    // CONST: 1; PERIODIC: 2^arg; SPARSE: arg
  std::vector<uint64_t> rows;  // SPARSE: arg, strictly increasing
};

struct PublicColumns {
  std::vector<PublicColumn> cols;
  uint8_t digest[32] = {0};  // SHA-256 of the wire bytes
  uint32_t max_log_period = 0;
  uint64_t max_row = 0;  // the largest sparse row
  std::vector<uint8_t> image;
  uint32_t sparse_off = 0, n_sparse = 0;  // of the image, in 16-byte words / entries
  uint32_t count() const { return (uint32_t)cols.size(); }
  // The conditions that depend on the height: every period at most 2^L rows,
  // every sparse row below 2^L.
  bool fits(uint32_t log_height) const {
    return log_height <= kPcMaxLogHeight && max_log_period <= log_height &&
           (max_row >> log_height) == 0;
  }
};

static inline uint32_t pc_rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static inline uint64_t pc_rd64(const uint8_t* p) {
  return (uint64_t)pc_rd32(p) | ((uint64_t)pc_rd32(p + 4) << 32);
}
static inline void pc_wr32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  p[3] = (uint8_t)(v >> 24);
}

static inline void pc_build_image(PublicColumns& s) {
  uint64_t words = kPcDescWords, sparse = 0;
  for (const PublicColumn& c : s.cols) {
    if (c.kind == kPcPeriodic) words += c.values.size();
    if (c.kind == kPcSparse) sparse += c.rows.size();
  }
  s.sparse_off = (uint32_t)words;
  s.n_sparse = (uint32_t)sparse;
  s.image.assign(16 * (words + 2 * sparse), 0);
  uint8_t* img = s.image.data();
  uint32_t table = kPcDescWords, entry = s.sparse_off;
  for (uint32_t j = 0; j < s.count(); ++j) {
    const PublicColumn& c = s.cols[j];
    uint8_t* d = img + 32ull * j;
    pc_wr32(d, c.kind);
    pc_wr32(d + 8, 2 * j + 1);  // mask 0 and the constant's own word: one load path for every kind
    if (c.kind == kPcConst) h_store(d + 16, c.values[0]);
    if (c.kind == kPcPeriodic) {
      pc_wr32(d + 4, (uint32_t)c.values.size() - 1);
      pc_wr32(d + 8, table);
      for (const u128 v : c.values) h_store(img + 16ull * table++, v);
    }
    if (c.kind == kPcSparse) {
      // (the check's search: this column's first entry | count << 16; at most 16 * 4096 entries)
      pc_wr32(d + 12, ((entry - s.sparse_off) / 2) | ((uint32_t)c.rows.size() << 16));
      for (size_t m = 0; m < c.rows.size(); ++m, entry += 2) {
        uint8_t* e = img + 16ull * entry;
        pc_wr32(e, (uint32_t)c.rows[m]);
        pc_wr32(e + 4, (uint32_t)(c.rows[m] >> 32));
        pc_wr32(e + 8, j);
        h_store(e + 16, c.values[m]);
      }
    }
  }
}

// The wire format of include/mlhip.h: exactly one byte string per spec.  False
// for an unknown kind, a nonzero reserved word or arg, a non-canonical
// element, unsorted or repeated sparse rows, a short buffer, trailing bytes.
static inline bool pc_decode(const uint8_t* b, uint64_t len, PublicColumns& s) {
  uint64_t at = 0;
  const auto have = [&](uint64_t n) { return n <= len - at; };
  if (len < 8) return false;
  const uint32_t F = pc_rd32(b);
  if (F < 1 || F > kPcMaxColumns || pc_rd32(b + 4) != 0) return false;
  at = 8;
  s.cols.assign(F, PublicColumn());
  for (PublicColumn& c : s.cols) {
    if (!have(8)) return false;
    c.kind = pc_rd32(b + at);
    c.arg = pc_rd32(b + at + 4);
    at += 8;
    uint64_t n_values = 0;
    switch (c.kind) {
      case kPcConst: n_values = 1; break;
      case kPcFirst:
      case kPcLast:
      case kPcRow: break;
      case kPcPeriodic:
        if (c.arg > kPcMaxLogPeriod) return false;
        n_values = 1ull << c.arg;
        if (c.arg > s.max_log_period) s.max_log_period = c.arg;
        break;
      case kPcSparse:
        if (c.arg < 1 || c.arg > kPcMaxSparse) return false;
        n_values = c.arg;
        break;
      default: return false;
    }
    if (c.kind < kPcPeriodic && c.arg != 0) return false;
    const uint64_t stride = c.kind == kPcSparse ? 24 : 16;
    if (!have(stride * n_values)) return false;
    c.values.resize(n_values);
    if (c.kind == kPcSparse) c.rows.resize(n_values);
    for (uint64_t m = 0; m < n_values; ++m, at += stride) {
      if (c.kind == kPcSparse) {
        c.rows[m] = pc_rd64(b + at);
        if (m && c.rows[m] <= c.rows[m - 1]) return false;
      }
      c.values[m] = h_load(b + at + (stride - 16));
      if (c.values[m] >= kModulus) return false;
    }
    if (c.kind == kPcSparse && c.rows.back() > s.max_row) s.max_row = c.rows.back();
  }
  if (at != len) return false;
  HostSha256 sha;
  sha.update(b, (size_t)len);
  sha.digest(s.digest);
  pc_build_image(s);
  return true;
}

// The multilinear extensions of the columns over 2^L rows at `point` (L
// canonical elements), in closed form; bit b of the row index belongs to x_b =
// point[L - 1 - b] (Mask::evaluate's order, evaluation.rs:56-73):
//   CONST c; FIRST prod_b (1 - x_b); LAST prod_b x_b; ROW sum_b 2^b x_b;
//   PERIODIC(k, v): the extension of v at point[L - k : L], the 2^k-entry table
//   folded from its top bit down; SPARSE: sum_m v_m eq(point, row_m).
// The caller has checked s.fits(L).  out: count() elements.
static inline void pc_evaluate(const PublicColumns& s, uint32_t L, const u128* point, u128* out) {
  const auto x = [&](uint32_t b) { return point[L - 1 - b]; };
  for (uint32_t j = 0; j < s.count(); ++j) {
    const PublicColumn& c = s.cols[j];
    u128 acc = 0;
    switch (c.kind) {
      case kPcConst: acc = c.values[0]; break;
      case kPcFirst:
        acc = 1;
        for (uint32_t b = 0; b < L; ++b) acc = h_mul(acc, h_sub(1, x(b)));
        break;
      case kPcLast:
        acc = 1;
        for (uint32_t b = 0; b < L; ++b) acc = h_mul(acc, x(b));
        break;
      case kPcRow:
        for (uint32_t b = 0; b < L; ++b) acc = h_add(acc, h_mul((u128)1 << b, x(b)));
        break;
      case kPcPeriodic: {
        std::vector<u128> t = c.values;
        for (uint32_t b = c.arg; b-- > 0;) {  // bit b of the index, the table's top bit first
          const size_t half = (size_t)1 << b;
          for (size_t i = 0; i < half; ++i)
            t[i] = h_add(t[i], h_mul(x(b), h_sub(t[i + half], t[i])));
        }
        acc = t[0];
        break;
      }
      default:  // kPcSparse
        for (size_t m = 0; m < c.rows.size(); ++m) {
          u128 eq = c.values[m];
          for (uint32_t b = 0; b < L; ++b)
            eq = h_mul(eq, ((c.rows[m] >> b) & 1) ? x(b) : h_sub(1, x(b)));
          acc = h_add(acc, eq);
        }
        break;
    }
    out[j] = acc;
  }
}

}  // namespace mlh

struct mlh_public_columns {
  mlh::PublicColumns p;
};
