// Host memory-safety driver for the public columns' host-only code: the spec
// decoder and evaluator (mlh_public_columns_create / _evaluate / _digest,
// csrc/public_columns.hpp) and mlh_system_verify_public (verify.cpp).  Built
// with -fsanitize=address,undefined by tests/test_public_host_sanitized.py and
// run on the CPU.  Input: a valid proof of the plain-Python model
// (tests/public_reference.py) in the dump format of that test:
//   u32 L, W, degree, P, mask, K, cols[32], n_pcs, F; u32 len + seed; u32 len +
//   program wire; u32 len + spec wire; sum[16]; column_sum[16]; sumcheck_polys;
//   output; shift_polys; output2; n_pcs openings at rs, then n_pcs at rs' --
//   each u32 num_codes, num_trees, root[32], commitments, last_elem[16],
//   last_random[32], u64 len + queries, polys [L][2][16]; digest[32].
// It checks that the proof verifies into the model's digest, then runs create /
// count / digest / evaluate / destroy over byte mutants of the spec wire
// (flips, truncations, extensions, forged words; evaluation at the proof's
// height and at heights 0..40), and verifies thousands of mutants of the proof
// and of the spec.  Any out-of-bounds access or UB aborts through the
// sanitizers; a rejected proof must leave the transcript as it was; a mutant
// of the public part (output[W-F:W], output2[W-F:W], a spec that decodes to
// other bytes, no spec) that verifies fails the run.
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

// One mutant of a spec's wire bytes.
static std::vector<uint8_t> mutate_wire(const std::vector<uint8_t>& wire) {
  std::vector<uint8_t> w = wire;
  switch (rnd() % 6) {
    case 0: w[rnd() % w.size()] ^= (uint8_t)(1u << (rnd() % 8)); break;
    case 1: w.resize(rnd() % (w.size() + 1)); break;
    case 2: w.resize(w.size() + 1 + rnd() % 40, (uint8_t)rnd()); break;
    case 3: {  // a forged word: a count, a kind, an arg
      const size_t at = 4 * (rnd() % (w.size() / 4));
      const uint32_t v = rnd() % 2 ? (uint32_t)(rnd() % 20) : (uint32_t)rnd();
      memcpy(w.data() + at, &v, 4);
      break;
    }
    case 4: memset(w.data() + rnd() % w.size(), 0xff, 1); break;
    default:  // a large arg in the first column header
      if (w.size() >= 16) {
        const uint32_t v = (uint32_t)(rnd() % 5000);
        memcpy(w.data() + 12, &v, 4);
      }
      break;
  }
  return w;
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
  const uint32_t F = r.u32();
  if (!r.ok || pf.L < 1 || pf.L > 16 || pf.W < 2 || pf.W + pf.K > 32 || pf.K < 1 || pf.degree > 7 ||
      pf.n_pcs < 1 || pf.n_pcs > 2 || F < 1 || F > 16 || F >= pf.W)
    return 2;
  const std::vector<uint8_t> seed = r.take(r.u32()), wire = r.take(r.u32());
  const std::vector<uint8_t> spec_wire = r.take(r.u32());
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
  if (!r.ok || r.at != r.d.size() || spec_wire.size() < 16) return 2;

  // ---- the spec: create / count / digest / evaluate / destroy -----------------
  mlh_public_columns* spec = nullptr;
  if (mlh_public_columns_create(spec_wire.data(), spec_wire.size(), &spec) != MLH_OK) return 2;
  CHECK(mlh_public_columns_count(spec) == F, "the seed spec has another column count");
  uint8_t spec_digest[32];
  CHECK(mlh_public_columns_digest(spec, spec_digest) == MLH_OK, "digest");
  int decoded = 0;
  {
    uint8_t point[40 * 16], out[16 * 16], d2[32];
    for (int it = 0; it < iters; ++it) {
      const std::vector<uint8_t> w = mutate_wire(spec_wire);
      // an exact-size copy on the heap: a read past the end is seen
      std::vector<uint8_t> exact(w.begin(), w.end());
      mlh_public_columns* s = nullptr;
      const mlh_status st = mlh_public_columns_create(exact.data(), exact.size(), &s);
      if (st != MLH_OK) {
        CHECK(st == MLH_ERR_INVALID && !s, "iteration %d: create returned %d", it, (int)st);
        continue;
      }
      ++decoded;
      const uint32_t n = mlh_public_columns_count(s);
      CHECK(n >= 1 && n <= 16, "iteration %d: %u columns", it, n);
      CHECK(mlh_public_columns_digest(s, d2) == MLH_OK, "iteration %d: digest", it);
      CHECK((w == spec_wire) == !memcmp(d2, spec_digest, 32), "iteration %d: digest of other bytes", it);
      for (uint32_t i = 0; i < 40; ++i) put(point + 16 * i, rnd());
      const mlh_status a = mlh_public_columns_evaluate(s, pf.L, point, out);
      CHECK(a == MLH_OK || a == MLH_ERR_INVALID, "iteration %d: evaluate returned %d", it, (int)a);
      const uint32_t h = (uint32_t)(rnd() % 41);
      const mlh_status b = mlh_public_columns_evaluate(s, h, point, out);
      CHECK(b == MLH_ERR_INVALID || (b == MLH_OK && h <= 32), "iteration %d: height %u gave %d", it,
            h, (int)b);
      memset(point, 0xff, 16);  // a non-canonical point
      if (pf.L) CHECK(mlh_public_columns_evaluate(s, pf.L, point, out) == MLH_ERR_INVALID, "point");
      mlh_public_columns_destroy(s);
    }
    CHECK(mlh_public_columns_create(nullptr, 8, &spec) == MLH_ERR_INVALID, "create null");
    CHECK(mlh_public_columns_evaluate(nullptr, 1, point, out) == MLH_ERR_INVALID, "evaluate null");
    mlh_public_columns_destroy(nullptr);
  }

  // ---- mlh_system_verify_public -------------------------------------------------
  mlh_cs_program* prog = nullptr;
  if (mlh_cs_program_create(wire.data(), wire.size(), &prog) != MLH_OK) return 2;
  mlh_transcript *base = nullptr, *tr = nullptr;
  mlh_transcript_create(&base);
  mlh_transcript_absorb(base, seed.data(), seed.size());
  uint8_t entry[32], got[32];
  mlh_transcript_random(base, entry);
  const auto run = [&](Proof& p, uint32_t L, uint32_t P, uint32_t mask, const uint32_t* cols,
                       uint32_t K, const mlh_public_columns* s) {
    mlh_shifted_proof c;
    p.fill(&c);
    if (tr) mlh_transcript_destroy(tr);
    mlh_transcript_clone(base, &tr);
    const mlh_status st = mlh_system_verify_public(prog, L, P, mask, cols, K, s, sum.data(),
                                                   column_sum.data(), &c, tr);
    mlh_transcript_random(tr, got);
    return st;
  };
  {
    Proof p = pf;
    CHECK(run(p, pf.L, pf.P, pf.mask, pf.cols, pf.K, spec) == MLH_OK, "the seed proof does not verify");
    CHECK(!memcmp(got, digest.data(), 32), "the seed proof ends in another transcript state");
    CHECK(run(p, pf.L, pf.P, pf.mask, pf.cols, pf.K, nullptr) == MLH_ERR_VERIFY, "verifies without a spec");
    CHECK(!memcmp(got, entry, 32), "no spec: the transcript moved");
  }
  int accepted_other = 0;
  for (int it = 0; it < iters; ++it) {
    Proof p = pf;
    uint32_t cols[40];
    memset(cols, 0, sizeof(cols));
    memcpy(cols, pf.cols, sizeof(pf.cols));
    uint32_t L = pf.L, P = pf.P, mask = pf.mask, K = pf.K;
    bool public_part = false;
    mlh_public_columns* other = nullptr;
    const uint32_t kind = rnd() % 12;
    if (kind < 2) {  // a bit of a public element of output / output2
      std::vector<uint8_t>& b = kind == 0 ? p.output : p.output2;
      b[16ull * (pf.W - F) + rnd() % (16ull * F)] ^= (uint8_t)(1u << (rnd() % 8));
      public_part = true;
    } else if (kind == 2) {  // a non-canonical element anywhere
      std::vector<uint8_t>* bufs[] = {&p.output, &p.output2, &p.shift_polys, &p.polys};
      std::vector<uint8_t>& b = *bufs[rnd() % 4];
      memset(b.data() + 16 * (rnd() % (b.size() / 16)), 0xff, 16);
      public_part = true;
    } else if (kind < 6) {  // another spec
      const std::vector<uint8_t> w = mutate_wire(spec_wire);
      if (mlh_public_columns_create(w.data(), w.size(), &other) != MLH_OK) other = nullptr;
      public_part = other != nullptr && w != spec_wire;
      if (!other) continue;
    } else if (kind == 6) {  // the verifier's shift list
      K = rnd() % 41;
      for (uint32_t k = 0; k < 40; ++k) cols[k] = rnd() % 4 ? rnd() % (pf.W + 2) : (uint32_t)rnd();
    } else if (kind == 7) {  // headers and public inputs
      switch (rnd() % 6) {
        case 0: p.L = (uint32_t)(rnd() % 40); break;
        case 1: p.W = (uint32_t)(rnd() % 40); break;
        case 2: p.P = (uint32_t)(rnd() % 40); break;
        case 3: L = (uint32_t)(rnd() % 40); break;
        case 4: P = (uint32_t)(rnd() % 40); break;
        default: mask = (uint32_t)rnd(); break;
      }
    } else if (kind == 8) {
      Opening& o = p.open[rnd() % (2 * pf.n_pcs)];
      o.num_codes = (uint32_t)(rnd() % 40);
    } else if (kind == 9) {  // a bit of a committed element or a coefficient
      std::vector<uint8_t>* bufs[] = {&p.output, &p.output2, &p.shift_polys, &p.polys};
      std::vector<uint8_t>& b = *bufs[rnd() % 4];
      b[rnd() % b.size()] ^= (uint8_t)(1u << (rnd() % 8));
    } else {  // a bit of an opening
      Opening& o = p.open[rnd() % (2 * pf.n_pcs)];
      std::vector<uint8_t>* ob[] = {&o.root, &o.commits, &o.last_elem, &o.queries, &o.polys};
      std::vector<uint8_t>& b = *ob[rnd() % 5];
      if (!b.empty()) b[rnd() % b.size()] ^= (uint8_t)(1u << (rnd() % 8));
    }
    const mlh_status st = run(p, L, P, mask, cols, K, other ? other : spec);
    if (st == MLH_OK) {
      CHECK(!public_part, "iteration %d: a mutant of the public part verifies (kind %u)", it, kind);
      ++accepted_other;
    } else {
      CHECK(!memcmp(got, entry, 32), "iteration %d: rejected, but the transcript moved", it);
    }
    mlh_public_columns_destroy(other);
  }
  if (tr) mlh_transcript_destroy(tr);
  mlh_transcript_destroy(base);
  mlh_cs_program_destroy(prog);
  mlh_public_columns_destroy(spec);
  if (fails) return 1;
  printf("public verify ok: %d mutants, %d specs decoded, %d unchanged in effect\n", iters, decoded,
         accepted_other);
  return 0;
}
