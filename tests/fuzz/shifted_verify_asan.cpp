// Host memory-safety driver for the shifted system proof's host-only code:
// mlh_shift_succ_evaluate and mlh_system_verify_shifted (verify.cpp).  Built
// with -fsanitize=address,undefined by tests/test_shifted_host_sanitized.py and
// run on the CPU.  Input: a valid proof of the plain-Python model
// (tests/shifted_reference.py) in the dump format of that test:
//   u32 L, W, degree, P, mask, K, cols[32], n_pcs; u32 len + seed; u32 len +
//   program wire; sum[16]; column_sum[16]; sumcheck_polys; output; shift_polys;
//   output2; n_pcs openings at rs, then n_pcs at rs' -- each u32 num_codes,
//   num_trees, root[32], commitments, last_elem[16], last_random[32], u64 len +
//   queries, polys [L][2][16]; digest[32].
// It checks that the proof verifies into the model's digest, that succ on 0/1
// points is the successor relation, and then verifies thousands of mutants:
// byte flips in every buffer, forged headers and shift lists (duplicates,
// columns out of range, K up to 40).  Any out-of-bounds access or UB aborts
// through the sanitizers; a rejected proof must leave the transcript as it
// was; a mutant of the shift part (output[W:], output2, shift_polys, the shift
// list) that verifies fails the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/mlhip.h"

static uint64_t rng_state = 0x5EEDull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Reader {
  std::vector<uint8_t> d;
  size_t at = 0;
  bool ok = true;
  std::vector<uint8_t> take(uint64_t n) {
    if (!ok || n > d.size() - at) {
      ok = false;
      return {};
    }
    std::vector<uint8_t> r(d.begin() + at, d.begin() + at + n);
    at += n;
    return r;
  }
  uint32_t u32() {
    const std::vector<uint8_t> b = take(4);
    uint32_t v = 0;
    if (ok) memcpy(&v, b.data(), 4);
    return v;
  }
  uint64_t u64() {
    const std::vector<uint8_t> b = take(8);
    uint64_t v = 0;
    if (ok) memcpy(&v, b.data(), 8);
    return v;
  }
};

struct Opening {
  uint32_t num_codes = 0, num_trees = 0;
  std::vector<uint8_t> root, commits, last_elem, last_random, queries, polys;
};

struct Proof {
  uint32_t L = 0, W = 0, degree = 0, P = 0, mask = 0, K = 0, cols[32] = {}, n_pcs = 0;
  std::vector<uint8_t> polys, output, shift_polys, output2;
  Opening open[4];
  // the C struct over these buffers
  void fill(mlh_shifted_proof* c) {
    memset(c, 0, sizeof(*c));
    c->log_height = L;
    c->width = W;
    c->degree = degree;
    c->pre_random_columns = P;
    c->sum_column_mask = mask;
    c->n_shifts = K;
    memcpy(c->shift_columns, cols, sizeof(cols));
    c->sumcheck_polys = polys.data();
    c->output = output.data();
    c->shift_polys = shift_polys.data();
    c->output2 = output2.data();
    for (uint32_t i = 0; i < 2 * n_pcs; ++i) {
      Opening& o = open[i];
      mlh_batched_pcs_proof* p = i < n_pcs ? &c->pcs[i] : &c->pcs_shift[i - n_pcs];
      p->fri.log_code = L + 1;
      p->fri.num_codes = o.num_codes;
      p->fri.num_trees = o.num_trees;
      p->fri.num_queries = MLH_NUM_QUERIES;
      memcpy(p->fri.batch_commitment, o.root.data(), 32);
      p->fri.commitments = o.commits.data();
      memcpy(p->fri.last_elem, o.last_elem.data(), 16);
      memcpy(p->fri.last_random, o.last_random.data(), 32);
      p->fri.queries = o.queries.data();
      p->sumcheck_polys = o.polys.data();
    }
  }
};

static int fails = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");      \
      ++fails;                    \
    }                             \
  } while (0)

static void put(uint8_t* p, uint64_t v) {
  memset(p, 0, 16);
  memcpy(p, &v, 8);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int iters = atoi(argv[2]);
  Reader r;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) r.d.insert(r.d.end(), buf, buf + n);
    fclose(f);
  }
  Proof pf;
  pf.L = r.u32();
  pf.W = r.u32();
  pf.degree = r.u32();
  pf.P = r.u32();
  pf.mask = r.u32();
  pf.K = r.u32();
  for (uint32_t& c : pf.cols) c = r.u32();
  pf.n_pcs = r.u32();
  if (!r.ok || pf.L < 1 || pf.L > 16 || pf.W < 1 || pf.W + pf.K > 32 || pf.K < 1 || pf.degree > 7 ||
      pf.n_pcs < 1 || pf.n_pcs > 2)
    return 2;
  const std::vector<uint8_t> seed = r.take(r.u32()), wire = r.take(r.u32());
  const std::vector<uint8_t> sum = r.take(16), column_sum = r.take(16);
  pf.polys = r.take(16ull * (pf.degree + 1) * pf.L);
  pf.output = r.take(16ull * (pf.W + pf.K));
  pf.shift_polys = r.take(32ull * pf.L);
  pf.output2 = r.take(16ull * pf.W);
  for (uint32_t i = 0; i < 2 * pf.n_pcs; ++i) {
    Opening& o = pf.open[i];
    o.num_codes = r.u32();
    o.num_trees = r.u32();
    if (o.num_trees > 64) return 2;
    o.root = r.take(32);
    o.commits = r.take(32ull * o.num_trees);
    o.last_elem = r.take(16);
    o.last_random = r.take(32);
    o.queries = r.take(r.u64());
    o.polys = r.take(32ull * pf.L);
  }
  const std::vector<uint8_t> digest = r.take(32);
  if (!r.ok || r.at != r.d.size()) return 2;

  // ---- mlh_shift_succ_evaluate ------------------------------------------------
  {
    uint8_t x[64 * 16], y[64 * 16], out[16];
    for (uint32_t n = 0; n <= 64; ++n) {
      for (uint32_t i = 0; i < n; ++i) {
        put(x + 16 * i, rnd());
        put(y + 16 * i, rnd());
      }
      CHECK(mlh_shift_succ_evaluate(x, y, n, out) == MLH_OK, "succ n=%u", n);
    }
    CHECK(mlh_shift_succ_evaluate(x, y, 65, out) == MLH_ERR_INVALID, "succ n=65");
    CHECK(mlh_shift_succ_evaluate(nullptr, y, 3, out) == MLH_ERR_INVALID, "succ null");
    memset(x, 0xff, 16);
    CHECK(mlh_shift_succ_evaluate(x, y, 1, out) == MLH_ERR_INVALID, "succ non-canonical");
    const uint32_t n = 3;
    for (uint32_t i = 0; i < 8; ++i)
      for (uint32_t j = 0; j < 8; ++j) {
        for (uint32_t t = 0; t < n; ++t) {
          put(x + 16 * t, (i >> (n - 1 - t)) & 1);
          put(y + 16 * t, (j >> (n - 1 - t)) & 1);
        }
        uint8_t want[16];
        put(want, j == ((i + 1) & 7) ? 1 : 0);
        CHECK(mlh_shift_succ_evaluate(x, y, n, out) == MLH_OK && !memcmp(out, want, 16),
              "succ bits %u %u", i, j);
      }
  }

  // ---- mlh_system_verify_shifted ----------------------------------------------
  mlh_cs_program* prog = nullptr;
  if (mlh_cs_program_create(wire.data(), wire.size(), &prog) != MLH_OK) return 2;
  mlh_transcript *base = nullptr, *tr = nullptr;
  mlh_transcript_create(&base);
  mlh_transcript_absorb(base, seed.data(), seed.size());
  uint8_t entry[32], got[32];
  mlh_transcript_random(base, entry);
  const auto run = [&](Proof& p, uint32_t L, uint32_t P, uint32_t mask, const uint32_t* cols,
                       uint32_t K) {
    mlh_shifted_proof c;
    p.fill(&c);
    if (tr) mlh_transcript_destroy(tr);
    mlh_transcript_clone(base, &tr);
    const mlh_status st = mlh_system_verify_shifted(prog, L, P, mask, cols, K, sum.data(),
                                                    column_sum.data(), &c, tr);
    mlh_transcript_random(tr, got);
    return st;
  };
  {
    Proof p = pf;
    CHECK(run(p, pf.L, pf.P, pf.mask, pf.cols, pf.K) == MLH_OK, "the seed proof does not verify");
    CHECK(!memcmp(got, digest.data(), 32), "the seed proof ends in another transcript state");
  }
  int accepted_other = 0;
  for (int it = 0; it < iters; ++it) {
    Proof p = pf;
    uint32_t cols[40];
    memset(cols, 0, sizeof(cols));
    memcpy(cols, pf.cols, sizeof(pf.cols));
    uint32_t L = pf.L, P = pf.P, mask = pf.mask, K = pf.K;
    bool shift_part = false;
    std::vector<uint8_t>* bufs[] = {&p.output, &p.output2, &p.shift_polys, &p.polys};
    const uint32_t kind = rnd() % 12;
    if (kind < 3) {  // a bit of the shift part
      std::vector<uint8_t>& b = *bufs[kind];
      const size_t lo = kind == 0 ? 16ull * pf.W : 0;
      b[lo + rnd() % (b.size() - lo)] ^= (uint8_t)(1u << (rnd() % 8));
      shift_part = true;
    } else if (kind == 3) {
      std::vector<uint8_t>& b = *bufs[rnd() % 4];
      memset(b.data() + 16 * (rnd() % (b.size() / 16)), 0xff, 16);  // non-canonical
      shift_part = true;
    } else if (kind == 4) {  // the verifier's shift list
      K = rnd() % 41;
      for (uint32_t k = 0; k < 40; ++k) cols[k] = rnd() % 4 ? rnd() % (pf.W + 2) : (uint32_t)rnd();
      shift_part = K != pf.K || memcmp(cols, pf.cols, 4 * pf.K) != 0;
    } else if (kind == 5) {  // the proof's shift list
      p.K = rnd() % 3 ? pf.K : (uint32_t)(rnd() % 41);
      p.cols[rnd() % 32] = rnd() % 2 ? (uint32_t)(rnd() % pf.W) : (uint32_t)rnd();
      shift_part = p.K != pf.K || memcmp(p.cols, pf.cols, sizeof(pf.cols)) != 0;
    } else if (kind == 6) {  // headers and public inputs
      switch (rnd() % 6) {
        case 0: p.L = (uint32_t)(rnd() % 40); break;
        case 1: p.W = (uint32_t)(rnd() % 40); break;
        case 2: p.P = (uint32_t)(rnd() % 40); break;
        case 3: L = (uint32_t)(rnd() % 40); break;
        case 4: P = (uint32_t)(rnd() % 40); break;
        default: mask = (uint32_t)rnd(); break;
      }
    } else if (kind == 7) {
      Opening& o = p.open[rnd() % (2 * pf.n_pcs)];
      o.num_codes = (uint32_t)(rnd() % 40);
    } else {  // a bit of an opening
      Opening& o = p.open[rnd() % (2 * pf.n_pcs)];
      std::vector<uint8_t>* ob[] = {&o.root, &o.commits, &o.last_elem, &o.queries, &o.polys};
      std::vector<uint8_t>& b = *ob[rnd() % 5];
      if (!b.empty()) b[rnd() % b.size()] ^= (uint8_t)(1u << (rnd() % 8));
    }
    const mlh_status st = run(p, L, P, mask, cols, K);
    if (st == MLH_OK) {
      CHECK(!shift_part, "iteration %d: a mutant of the shift part verifies (kind %u)", it, kind);
      ++accepted_other;
    } else {
      CHECK(!memcmp(got, entry, 32), "iteration %d: rejected, but the transcript moved", it);
    }
  }
  if (tr) mlh_transcript_destroy(tr);
  mlh_transcript_destroy(base);
  mlh_cs_program_destroy(prog);
  if (fails) return 1;
  printf("shifted verify ok: %d mutants, %d unchanged in effect\n", iters, accepted_other);
  return 0;
}
