// Host memory-safety driver for the program decoders of csrc/cs_program.hpp
// (header only): cs_decode and fill_decode, the host interpreters cs_host_eval
// and fill_host_eval, and the device images cs_build_image / fill_build_image.
// Built with -fsanitize=address,undefined by tests/test_program_fuzz_cpu.py and
// run on the CPU.  Input: valid wire programs of tests/program_fuzz.py,
//   u32 count; per program u8 kind (0 constraint, 1 fill), u32 len, bytes.
// Every program must decode as its kind.  Then seeded mutants -- byte flips,
// small values, truncations, extensions, forged header words, header counts
// changed together with the length, forged instruction fields -- go to both
// decoders.  An accepted mutant is interpreted on random elements and built
// into its device image, whose words are checked against what the kernels
// index with them: LDS slots below the lane's slot count, uniform indices
// inside the pool, inverse indices below n_inv.  Any out-of-bounds access or UB
// aborts through the sanitizers; a word out of range fails the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../multilinear_amd/csrc/cs_program.hpp"

using namespace mlh;

static uint64_t rng_state = 0x5EEDull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static u128 rnd_elem() {
  switch (rnd() % 8) {
    case 0: return 0;
    case 1: return kModulus - 1;
    default: return h_reduce_once((((u128)rnd()) << 64 | rnd()) % kModulus);
  }
}

static void fail(const char* what) {
  printf("FAIL: %s\n", what);
  exit(1);
}

static bool operand_ok(uint32_t o, uint32_t lane_slots, uint32_t n_uni) {
  return (o & kCsUniform) ? (o & 0x7FFFu) < n_uni : o < lane_slots;
}

static void exercise_cs(const CsProgram& p) {
  std::vector<u128> values(p.width), randoms(p.n_randoms + 1), mask(p.n_constraints);
  for (u128& v : values) v = rnd_elem();
  for (u128& v : randoms) v = rnd_elem();
  for (u128& v : mask) v = rnd_elem();
  if (cs_host_eval(p, values.data(), randoms.data(), mask.data()) >= kModulus) fail("cs value");
  const std::vector<uint8_t> img = cs_build_image(p, randoms.data(), mask.data());
  const CsImageLayout l = cs_image_layout(p);
  if (img.size() != l.bytes || l.outs_off + 4 * p.n_constraints > l.bytes) fail("cs image size");
  if (p.vinv.size() != (size_t)(p.degree + 2) * (p.degree + 2)) fail("vinv size");
  const uint32_t* w = reinterpret_cast<const uint32_t*>(img.data() + l.code_off);
  const uint32_t temps = p.width + p.n_temps, pool = p.n_randoms + p.n_consts;
  for (uint32_t i = 0; i < p.n_instr; ++i, w += 2) {
    const uint32_t dst = w[0] >> 8;
    if ((w[0] & 0xFFu) > kCsNeg || dst < p.width || dst >= temps) fail("cs code word 0");
    if (!operand_ok(w[1] & 0xFFFFu, temps, pool) || !operand_ok(w[1] >> 16, temps, pool))
      fail("cs operand");
  }
  for (uint32_t c = 0; c < p.n_constraints; ++c, ++w)
    if (!operand_ok(*w & 0xFFFFu, temps, pool) || (*w >> 16) < pool || (*w >> 16) >= l.n_uni)
      fail("cs output word");
  const uint32_t t = cs_threads(cs_slots(p));
  if ((uint64_t)cs_slots(p) * 16 * t > kCsLdsBytes) fail("cs slots over the LDS");
}

static void exercise_fill(const FillProgram& p) {
  std::vector<u128> row(p.width), randoms(p.n_randoms + 1), out(p.width);
  for (u128& v : row) v = rnd() % 4 ? rnd_elem() : 0;
  for (u128& v : randoms) v = rnd_elem();
  fill_host_eval(p, row.data(), randoms.data(), out.data());
  for (uint32_t j = 0; j < p.width; ++j)
    if (out[j] >= kModulus || (!((p.out_mask >> j) & 1u) && out[j] != row[j])) fail("fill value");
  const std::vector<uint8_t> img = fill_build_image(p, randoms.data());
  const FillImageLayout l = fill_image_layout(p);
  if (img.size() != l.bytes || l.outs_off + 4 * p.n_outputs > l.bytes) fail("fill image size");
  if (p.n_pre > p.n_instr || p.n_inv > kFillMaxInv) fail("fill counts");
  const uint32_t* w = reinterpret_cast<const uint32_t*>(img.data() + l.code_off);
  const uint32_t temps = p.width + p.n_temps, pool = p.n_randoms + p.n_consts;
  uint32_t last_inv = 0, n_inv = 0;
  for (uint32_t i = 0; i < p.n_instr; ++i, w += 2) {
    const uint32_t op = w[0] & 0xFFu, dst = (w[0] >> 8) & 0xFFu;
    if (op > kCsInv || dst < p.width || dst >= temps || (w[0] >> 8 & 0xFFFFu) != dst)
      fail("fill code word 0");
    if (!operand_ok(w[1] & 0xFFFFu, temps, pool)) fail("fill operand a");
    if (op == kCsInv) {
      if ((w[1] >> 16) != n_inv++ || !(w[0] & kFillTainted)) fail("fill inverse index");
      last_inv = i + 1;
    } else if (!operand_ok(w[1] >> 16, temps, pool)) {
      fail("fill operand b");
    }
  }
  if (n_inv != p.n_inv || last_inv != p.n_pre) fail("fill n_inv / n_pre");
  for (uint32_t c = 0; c < p.n_outputs; ++c, ++w)
    if (!operand_ok(*w & 0xFFFFu, temps, pool) || (*w >> 16) >= p.width) fail("fill output word");
  for (uint32_t L = 0; L <= 32; L += 4) {
    uint32_t B, K;
    fill_shape(p, 1ull << L, &B, &K);
    if (!fill_shape_ok(p, B, K) && (uint64_t)fill_slots(p) * 16 * 64 <= kCsLdsBytes) fail("fill shape");
    if (fill_blocks(p, fill_chunks(1ull << L, B, K), B, K) < 1) fail("fill blocks");
  }
}

struct Seed {
  uint8_t kind;
  std::vector<uint8_t> b;
};

static void put32(std::vector<uint8_t>& b, size_t at, uint32_t v) {
  if (at + 4 <= b.size()) memcpy(b.data() + at, &v, 4);
}

static void mutate(std::vector<uint8_t>& b, uint8_t kind) {
  static const uint32_t forged[] = {0, 1, 2, 7, 8, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257,
                                    4095, 4096, 4097, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
  const uint32_t hdr = cs_rd32(b.data() + 8);  // n_consts
  const size_t code = kCsHeaderBytes + 16 * (size_t)hdr;
  switch (rnd() % 8) {
    case 0:  // byte flips
      for (uint32_t k = 1 + rnd() % 3; k--;) b[rnd() % b.size()] ^= (uint8_t)(1u << (rnd() % 8));
      break;
    case 1:  // a small value somewhere: an opcode, a kind, an index
      b[rnd() % b.size()] = (uint8_t)(rnd() % 6);
      break;
    case 2:
      b.resize(rnd() % b.size());
      break;
    case 3:
      for (uint32_t k = 1 + rnd() % 24; k--;) b.push_back((uint8_t)rnd());
      break;
    case 4:  // a forged header word
      put32(b, 4 * (rnd() % 7), forged[rnd() % (sizeof(forged) / sizeof(forged[0]))]);
      break;
    case 5: {  // fewer outputs, the length adjusted: still well-formed
      const uint32_t n = cs_rd32(b.data() + 20), per = kind ? kFillOutBytes : kCsOperandBytes;
      const uint32_t cut = n > 1 ? 1 + rnd() % (n - 1) : 0;
      if ((size_t)cut * per > b.size() - kCsHeaderBytes) break;
      put32(b, 20, n - cut);
      b.resize(b.size() - (size_t)cut * per);
      break;
    }
    case 6: {  // one more temp, or another declared degree
      if (rnd() % 2)
        put32(b, 12, cs_rd32(b.data() + 12) + 1);
      else if (!kind)
        put32(b, 24, 1 + rnd() % 8);
      break;
    }
    default: {  // a forged field of one instruction
      const uint32_t n = cs_rd32(b.data() + 16);
      if (n && code + 8 * (size_t)n <= b.size())
        b[code + 8 * (rnd() % n) + rnd() % 6] = (uint8_t)(rnd() % 40);
      break;
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> d;
  uint8_t buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
  fclose(f);
  const long rounds = atol(argv[2]);
  std::vector<Seed> seeds;
  size_t at = 4;
  if (d.size() < 4) return 2;
  for (uint32_t i = 0, n = cs_rd32(d.data()); i < n; ++i) {
    if (at + 5 > d.size()) return 2;
    Seed s;
    s.kind = d[at];
    const uint32_t len = cs_rd32(d.data() + at + 1);
    at += 5;
    if (len < kCsHeaderBytes || at + len > d.size()) return 2;
    s.b.assign(d.begin() + at, d.begin() + at + len);
    at += len;
    seeds.push_back(s);
  }
  if (seeds.empty()) return 2;
  for (const Seed& s : seeds) {  // the table's programs themselves
    if (s.kind) {
      FillProgram p;
      if (!fill_decode(s.b.data(), s.b.size(), p)) fail("a valid fill program was rejected");
      exercise_fill(p);
    } else {
      CsProgram p;
      if (!cs_decode(s.b.data(), s.b.size(), p)) fail("a valid constraint program was rejected");
      exercise_cs(p);
    }
  }
  {
    CsProgram cp;
    FillProgram fp;
    if (cs_decode(nullptr, 0, cp) || fill_decode(nullptr, 64, fp)) fail("a null buffer was accepted");
  }
  unsigned long accepted = 0, rejected = 0;
  for (long i = 0; i < rounds; ++i) {
    const Seed& s = seeds[rnd() % seeds.size()];
    std::vector<uint8_t> b = s.b;
    for (uint32_t k = 1 + (rnd() % 4 == 0); k--;)
      if (b.size() >= kCsHeaderBytes) mutate(b, s.kind);
    // an exact-size heap copy, so that a read past the end is seen
    std::vector<uint8_t> exact(b.begin(), b.end());
    const uint8_t* q = exact.empty() ? nullptr : exact.data();
    CsProgram cp;
    const bool c_ok = cs_decode(q, exact.size(), cp);
    if (c_ok) exercise_cs(cp);
    FillProgram fp;
    const bool f_ok = fill_decode(q, exact.size(), fp);
    if (f_ok) exercise_fill(fp);
    if (c_ok || f_ok)
      ++accepted;
    else
      ++rejected;
  }
  printf("program decode ok: accepted %lu rejected %lu\n", accepted, rejected);
  return 0;
}
