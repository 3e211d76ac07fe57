// Host-only half of the C ABI: the Fiat-Shamir transcript, Merkle path
// verification and the FRI / PCS / batched verifiers (fri/mod.rs:184-340,
// multilinear_pcs.rs:138-190, batched_fri.rs:226-388, batched_pcs.rs:186-250,
// merkle_tree/mod.rs:216-293, transcript.rs).  Plain C++ with no HIP
// dependency, so the untrusted-input paths (these verifiers and the wire
// decoder, wire.hip) also build with host ASan/UBSan for the fuzz tests
// (tests/test_host_sanitized.py).
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/mlhip.h"
#include "cs_program.hpp"
#include "host_field.hpp"
#include "host_sha256.hpp"
#include "host_transcript.hpp"
#include "system_head.hpp"

using namespace mlh;

extern "C" {

mlh_status mlh_transcript_create(mlh_transcript** out) {
  if (!out) return MLH_ERR_INVALID;
  *out = new mlh_transcript();
  return MLH_OK;
}
mlh_status mlh_transcript_clone(const mlh_transcript* t, mlh_transcript** out) {
  if (!t || !out) return MLH_ERR_INVALID;
  *out = new mlh_transcript(*t);
  return MLH_OK;
}
void mlh_transcript_destroy(mlh_transcript* t) { delete t; }
mlh_status mlh_transcript_absorb(mlh_transcript* t, const uint8_t* bytes, uint64_t len) {
  if (!t || (!bytes && len)) return MLH_ERR_INVALID;
  t->sha.update(bytes, (size_t)len);
  return MLH_OK;
}
mlh_status mlh_transcript_random(const mlh_transcript* t, uint8_t out[32]) {
  if (!t || !out) return MLH_ERR_INVALID;
  t->sha.digest(out);
  return MLH_OK;
}
mlh_status mlh_transcript_next_challenge(mlh_transcript* t, uint8_t out[16]) {
  if (!t || !out) return MLH_ERR_INVALID;
  uint8_t d[32];
  t->sha.digest(d);
  h_store(out, h_reduce_once(h_load(d)));  // Field128::from(u128), field.rs:138-142
  return MLH_OK;
}

uint64_t mlh_fri_query_bytes(uint32_t log_code) {
  if (log_code < 2) return 0;
  uint64_t items = 0;
  for (uint32_t t = 0; t + 1 < log_code; ++t) items += 1 + (log_code - 1 - t);
  return items * 32;
}


uint64_t mlh_batched_fri_query_bytes(uint32_t log_code, uint32_t num_codes) {
  if (log_code < 2 || num_codes == 0) return 0;
  uint64_t b = 32ull * num_codes + 32ull * (log_code - 1);
  for (uint32_t t = 0; t + 2 < log_code; ++t) b += 32ull * (1 + (log_code - 2 - t));
  return b;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// host verifiers (fri/mod.rs:184-340, multilinear_pcs.rs:138-190)
// ---------------------------------------------------------------------------
static void sha_pair(const uint8_t* a, const uint8_t* b, uint8_t out[32]) {
  HostSha256 s;
  s.update(a, 32);
  s.update(b, 32);
  s.digest(out);
}

// MerkleInclusionPath::verify (merkle_tree/mod.rs:216-253); directions from index bits.
static bool verify_path_len(const uint8_t* value, uint64_t len, const uint8_t* sibs,
                            uint32_t depth, const uint8_t root[32], uint64_t index) {
  uint8_t h[32];
  HostSha256 s;
  s.update(value, len);
  s.digest(h);
  for (uint32_t l = 0; l < depth; ++l) {
    uint8_t nh[32];
    if ((index >> l) & 1)
      sha_pair(sibs + 32 * l, h, nh);  // Direction::Left
    else
      sha_pair(h, sibs + 32 * l, nh);  // Direction::Right
    memcpy(h, nh, 32);
  }
  return memcmp(h, root, 32) == 0;
}

static bool verify_path(const uint8_t* value32, const uint8_t* sibs, uint32_t depth,
                        const uint8_t root[32], uint64_t index) {
  return verify_path_len(value32, 32, sibs, depth, root, index);
}

// Proof elements are canonical: the reference's proofs hold typed field
// elements (ReedSolomonPair<F>, fri/mod.rs:177-236) and hash their canonical
// bytes, so 16 bytes that spell a value >= M cannot occur there.  Over raw
// bytes that is a rejection (as cs_sumcheck_verify_rs's load_canonical).
static bool all_canonical(const uint8_t* src, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (h_load(src + 16 * i) >= kModulus) return false;
  return true;
}

extern "C" {

mlh_status mlh_merkle_verify(const uint8_t* value, uint64_t value_len, const uint8_t* sibs,
                             uint32_t depth, uint64_t dirs, const uint8_t root[32],
                             uint64_t index) {
  if ((value_len && !value) || (depth && !sibs) || !root || depth > 63) return MLH_ERR_INVALID;
  uint8_t h[32];
  HostSha256 s;
  s.update(value, value_len);
  s.digest(h);
  uint64_t computed = 0;
  for (uint32_t l = 0; l < depth; ++l) {
    uint8_t nh[32];
    if ((dirs >> l) & 1) {  // Direction::Left
      computed += 1ull << l;
      sha_pair(sibs + 32 * l, h, nh);
    } else {
      sha_pair(h, sibs + 32 * l, nh);
    }
    memcpy(h, nh, 32);
  }
  if (memcmp(h, root, 32) != 0) return MLH_ERR_VERIFY;
  if (computed != index) return MLH_ERR_VERIFY_INDEX;
  return MLH_OK;
}

}  // extern "C"

// QueryProof::verify (fri/mod.rs:184-236) over flat records: ntrees paths,
// tree t has leaves n/2^t (depth log2(n) - t), gen of order 2n.
static bool query_chain(const uint8_t* rec, const uint8_t* commitments, uint32_t ntrees,
                        uint64_t n, uint64_t index, u128 gen, const u128* rs, u128 last) {
  const u128 inv2 = h_inv(2);
  uint64_t cur_n = n, cur_idx = index, off = 0;
  u128 cur_gen = gen;
  const uint32_t depth0 = 63 - __builtin_clzll(n);
  for (uint32_t t = 0; t < ntrees; ++t) {
    const uint32_t depth = depth0 - t;
    const uint8_t* val = rec + off;
    if (!verify_path(val, val + 32, depth, commitments + 32 * t, cur_idx)) return false;
    if (!all_canonical(val, 2)) return false;
    const u128 v = h_load(val), mv = h_load(val + 16);
    const u128 gp = h_pow(cur_gen, cur_idx);
    const u128 even = h_mul(h_add(v, mv), inv2);
    const u128 odd = h_mul(h_sub(v, mv), h_inv(h_mul(2, gp)));
    const u128 folded = h_add(even, h_mul(rs[t], odd));
    if (t + 1 == ntrees) return folded == last;
    const uint64_t nidx = cur_idx % (cur_n / 2);
    const uint8_t* nval = rec + off + 32ull * (1 + depth);
    const u128 nv = nidx == cur_idx ? h_load(nval) : h_load(nval + 16);
    if (nv != folded) return false;
    cur_gen = h_mul(cur_gen, cur_gen);
    cur_n /= 2;
    cur_idx = nidx;
    off += 32ull * (1 + depth);
  }
  return true;
}

static mlh_status fri_verify_queries(const mlh_fri_proof* pf, mlh_transcript* tr,
                                     const std::vector<u128>& rs) {
  const uint32_t L = pf->log_code;
  const uint64_t domain = 1ull << L;
  const u128 gen = h_pow2_generator(L);
  const uint64_t qbytes = mlh_fri_query_bytes(L);
  const u128 last = h_load(pf->last_elem);
  if (!all_canonical(pf->last_elem, 1)) return MLH_ERR_VERIFY;
  for (uint32_t q = 0; q < pf->num_queries; ++q) {
    uint64_t index;
    transcript_draw_indices(tr, domain / 2, 1, &index);
    if (pf->query_indices && pf->query_indices[q] != index) return MLH_ERR_VERIFY;
    if (!query_chain(pf->queries + q * qbytes, pf->commitments, pf->num_trees, domain / 2, index,
                     gen, rs.data(), last))
      return MLH_ERR_VERIFY;
  }
  uint8_t lr[32];
  mlh_transcript_random(tr, lr);
  return memcmp(lr, pf->last_random, 32) == 0 ? MLH_OK : MLH_ERR_VERIFY;
}

// BatchedFriProof::verify_queries (batched_fri.rs:226-278, 345-388).
static mlh_status batched_verify_queries(const mlh_batched_fri_proof* pf, mlh_transcript* tr,
                                         const std::vector<u128>& rs, u128 fr) {
  const uint32_t L = pf->log_code, m = pf->num_codes;
  const uint64_t domain = 1ull << L, n = domain / 2;
  const u128 gen = h_pow2_generator(L);
  const uint64_t qbytes = mlh_batched_fri_query_bytes(L, m);
  const u128 inv2 = h_inv(2), last = h_load(pf->last_elem);
  if (!all_canonical(pf->last_elem, 1)) return MLH_ERR_VERIFY;
  for (uint32_t q = 0; q < pf->num_queries; ++q) {
    uint64_t index;  // (drawn and absorbed; nothing below reads the transcript)
    transcript_draw_indices(tr, n, 1, &index);
    if (pf->query_indices && pf->query_indices[q] != index) return MLH_ERR_VERIFY;
    const uint8_t* rec = pf->queries + q * qbytes;
    if (!verify_path_len(rec, 32ull * m, rec + 32ull * m, L - 1, pf->batch_commitment, index))
      return MLH_ERR_VERIFY;
    if (!all_canonical(rec, 2ull * m)) return MLH_ERR_VERIFY;
    u128 v = 0, mv = 0;  // fingerprints (Horner over the codes)
    for (uint32_t j = 0; j < m; ++j) {
      v = h_add(h_mul(v, fr), h_load(rec + 32ull * j));
      mv = h_add(h_mul(mv, fr), h_load(rec + 32ull * j + 16));
    }
    const u128 gp = h_pow(gen, index);
    const u128 even = h_mul(h_add(v, mv), inv2);
    const u128 odd = h_mul(h_sub(v, mv), h_inv(h_mul(2, gp)));
    const u128 folded = h_add(even, h_mul(rs[0], odd));
    const uint8_t* inner = rec + 32ull * m + 32ull * (L - 1);
    if (pf->num_trees == 0) {
      if (folded != last) return MLH_ERR_VERIFY;
    } else {
      const uint64_t nidx = index % (n / 2);
      const u128 nv = nidx == index ? h_load(inner) : h_load(inner + 16);
      if (nv != folded) return MLH_ERR_VERIFY;
      if (!query_chain(inner, pf->commitments, pf->num_trees, n / 2, nidx, h_mul(gen, gen),
                       rs.data() + 1, last))
        return MLH_ERR_VERIFY;
    }
  }
  uint8_t lr[32];
  mlh_transcript_random(tr, lr);
  return memcmp(lr, pf->last_random, 32) == 0 ? MLH_OK : MLH_ERR_VERIFY;
}

extern "C" {

// Header checks of an untrusted proof before any shift or index is derived
// from it: the reference's verifiers index Vecs whose lengths the proof
// fixes and panic on an inconsistent proof; here that is MLH_ERR_VERIFY.
static bool fri_header_ok(uint32_t log_code, uint32_t num_trees, uint32_t want_trees) {
  return log_code >= 2 && log_code <= 41 && num_trees == want_trees;
}

mlh_status mlh_fri_verify(const mlh_fri_proof* pf) {
  if (!pf || !pf->commitments || !pf->queries) return MLH_ERR_INVALID;
  if (pf->num_queries != MLH_NUM_QUERIES) return MLH_ERR_VERIFY;
  if (pf->log_code < 2 || pf->log_code > 41) return MLH_ERR_VERIFY;
  if (pf->num_trees + MLH_LOG_BLOWUP != pf->log_code) return MLH_ERR_VERIFY;
  mlh_transcript tr;
  std::vector<u128> rs;
  for (uint32_t t = 0; t < pf->num_trees; ++t) {
    mlh_transcript_absorb(&tr, pf->commitments + 32 * t, 32);
    uint8_t r[16];
    mlh_transcript_next_challenge(&tr, r);
    rs.push_back(h_load(r));
  }
  mlh_transcript_absorb(&tr, pf->last_elem, 16);
  return fri_verify_queries(pf, &tr, rs);
}

mlh_status mlh_pcs_verify(const mlh_pcs_proof* pf, uint32_t n_vars, const uint8_t* inputs,
                          const uint8_t output[16], mlh_transcript* tr) {
  if (!pf || !tr || !output || !pf->sumcheck_polys || (n_vars && !inputs)) return MLH_ERR_INVALID;
  const mlh_fri_proof* fp = &pf->fri;
  if (fp->num_queries != MLH_NUM_QUERIES) return MLH_ERR_VERIFY;
  // n_vars >= 1: rs[n_vars - 1] below; the code of an n-variate MLE has
  // 2^(n + LOG_BLOWUP) elements (multilinear_pcs.rs:103-107)
  if (n_vars == 0 || !fri_header_ok(fp->log_code, fp->num_trees, n_vars) ||
      fp->log_code != n_vars + MLH_LOG_BLOWUP)
    return MLH_ERR_VERIFY;
  if (!all_canonical(pf->sumcheck_polys, 2ull * n_vars)) return MLH_ERR_VERIFY;
  std::vector<u128> rs;
  for (uint32_t k = 0; k < n_vars; ++k) {
    mlh_transcript_absorb(tr, fp->commitments + 32 * k, 32);
    mlh_transcript_absorb(tr, pf->sumcheck_polys + 32 * k, 32);
    uint8_t r[16];
    mlh_transcript_next_challenge(tr, r);
    rs.push_back(h_load(r));
  }
  mlh_transcript_absorb(tr, fp->last_elem, 16);
  // SumcheckPolynomial::to_polynomial chain (sumcheck.rs:269-276)
  const u128 inv2 = h_inv(2);
  auto to_poly = [&](uint32_t k, u128 s, u128 c[3]) {
    c[1] = h_load(pf->sumcheck_polys + 32 * k);
    c[2] = h_load(pf->sumcheck_polys + 32 * k + 16);
    c[0] = h_mul(h_sub(s, h_add(c[1], c[2])), inv2);
  };
  auto eval = [&](const u128 c[3], u128 x) { return h_add(c[0], h_mul(x, h_add(c[1], h_mul(c[2], x)))); };
  u128 c[3];
  to_poly(0, h_load(output), c);
  for (uint32_t k = 1; k < n_vars; ++k) {
    const u128 v = eval(c, rs[k - 1]);
    to_poly(k, v, c);
  }
  const u128 r = rs[n_vars - 1];
  // Delta::evaluate (evaluation.rs:75-91)
  u128 delta = 1;
  for (uint32_t i = 0; i < n_vars; ++i) {
    const u128 a = h_load(inputs + 16 * i), b = rs[i];
    delta = h_mul(delta, h_add(h_mul(a, b), h_mul(h_sub(1, a), h_sub(1, b))));
  }
  if (h_mul(delta, h_load(fp->last_elem)) != eval(c, r)) return MLH_ERR_VERIFY;
  return fri_verify_queries(fp, tr, rs);
}

mlh_status mlh_batched_fri_verify(const mlh_batched_fri_proof* pf) {
  if (!pf || !pf->queries || (pf->num_trees && !pf->commitments) || pf->num_codes == 0)
    return MLH_ERR_INVALID;
  if (pf->num_queries != MLH_NUM_QUERIES) return MLH_ERR_VERIFY;
  if (pf->log_code < 2 || pf->log_code > 41) return MLH_ERR_VERIFY;
  if (pf->num_trees + 1 + MLH_LOG_BLOWUP != pf->log_code) return MLH_ERR_VERIFY;
  mlh_transcript tr;
  mlh_transcript_absorb(&tr, pf->batch_commitment, 32);
  uint8_t frb[16];
  mlh_transcript_next_challenge(&tr, frb);
  mlh_transcript_absorb(&tr, frb, 16);
  std::vector<u128> rs;
  uint8_t r[16];
  mlh_transcript_next_challenge(&tr, r);
  rs.push_back(h_load(r));
  for (uint32_t t = 0; t < pf->num_trees; ++t) {
    mlh_transcript_absorb(&tr, pf->commitments + 32 * t, 32);
    mlh_transcript_next_challenge(&tr, r);
    rs.push_back(h_load(r));
  }
  mlh_transcript_absorb(&tr, pf->last_elem, 16);
  return batched_verify_queries(pf, &tr, rs, h_load(frb));
}

mlh_status mlh_batched_pcs_verify(const mlh_batched_pcs_proof* pf, uint32_t n_vars,
                                  const uint8_t* inputs, const uint8_t* outputs,
                                  mlh_transcript* tr) {
  if (!pf || !tr || !inputs || !outputs || !pf->sumcheck_polys) return MLH_ERR_INVALID;
  const mlh_batched_fri_proof* fp = &pf->fri;
  if (fp->num_queries != MLH_NUM_QUERIES) return MLH_ERR_VERIFY;
  // n_vars >= 1 (the first round is the batch layer), num_trees = n_vars - 1,
  // code length 2^(n_vars + LOG_BLOWUP) (batched_pcs.rs:137-147, 186-250)
  if (n_vars == 0 || fp->num_codes == 0 || !fri_header_ok(fp->log_code, fp->num_trees, n_vars - 1) ||
      fp->log_code != n_vars + MLH_LOG_BLOWUP)
    return MLH_ERR_VERIFY;
  if (!all_canonical(pf->sumcheck_polys, 2ull * n_vars)) return MLH_ERR_VERIFY;
  const uint32_t m = fp->num_codes;
  for (uint32_t i = 0; i < n_vars; ++i) mlh_transcript_absorb(tr, inputs + 16 * i, 16);
  for (uint32_t j = 0; j < m; ++j) mlh_transcript_absorb(tr, outputs + 16 * j, 16);
  std::vector<u128> rs;
  u128 fr = 0;
  for (uint32_t i = 0; i < n_vars; ++i) {
    if (i == 0) {
      mlh_transcript_absorb(tr, fp->batch_commitment, 32);
      uint8_t b[16];
      mlh_transcript_next_challenge(tr, b);
      fr = h_load(b);
      mlh_transcript_absorb(tr, b, 16);
    } else {
      mlh_transcript_absorb(tr, fp->commitments + 32 * (i - 1), 32);
    }
    mlh_transcript_absorb(tr, pf->sumcheck_polys + 32 * i, 32);
    uint8_t r[16];
    mlh_transcript_next_challenge(tr, r);
    rs.push_back(h_load(r));
  }
  mlh_transcript_absorb(tr, fp->last_elem, 16);
  // sumcheck chain from fingerprint(fr, outputs) (batched_pcs.rs:221-240)
  u128 sum = 0;
  for (uint32_t j = 0; j < m; ++j) sum = h_add(h_mul(sum, fr), h_load(outputs + 16 * j));
  const u128 inv2 = h_inv(2);
  u128 cur = sum, val = 0;
  for (uint32_t k = 0; k < n_vars; ++k) {
    const u128 c1 = h_load(pf->sumcheck_polys + 32 * k), c2 = h_load(pf->sumcheck_polys + 32 * k + 16);
    const u128 c0 = h_mul(h_sub(cur, h_add(c1, c2)), inv2);
    val = h_add(c0, h_mul(rs[k], h_add(c1, h_mul(c2, rs[k]))));
    cur = val;
  }
  // Delta::evaluate(inputs, rs) (evaluation.rs:75-91)
  u128 delta = 1;
  for (uint32_t i = 0; i < n_vars; ++i) {
    const u128 a = h_load(inputs + 16 * i), b = rs[i];
    delta = h_mul(delta, h_add(h_mul(a, b), h_mul(h_sub(1, a), h_sub(1, b))));
  }
  if (h_mul(delta, h_load(fp->last_elem)) != val) return MLH_ERR_VERIFY;
  return batched_verify_queries(fp, tr, rs, fr);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// constraint system: programs, challenges, the sumcheck verifier
// (constraint_system/{constraints,system,evaluation,sumcheck}.rs)
// ---------------------------------------------------------------------------
static bool load_canonical(const uint8_t* src, uint32_t n, std::vector<u128>& out) {
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    out[i] = h_load(src + 16ull * i);
    if (out[i] >= kModulus) return false;
  }
  return true;
}

// Mask::evaluate (evaluation.rs:56-73)
static u128 mask_evaluate(uint64_t index, uint32_t n_vars, const u128* points) {
  u128 acc = 1;
  for (uint32_t i = 0; i < n_vars; ++i) {
    const u128 p = points[n_vars - 1 - i];
    acc = h_mul(acc, ((index >> i) & 1) ? p : h_sub(1, p));
  }
  return acc;
}

// Polynomial::evaluate (polynomials.rs:9-14)
static u128 horner(const std::vector<u128>& c, u128 x) {
  u128 acc = 0;
  for (size_t i = c.size(); i-- > 0;) acc = h_add(h_mul(acc, x), c[i]);
  return acc;
}

// The number of constraint challenges: next_power_of_two().trailing_zeros() (system.rs:83-87)
static uint32_t cs_log_nc(uint32_t n_constraints) {
  uint32_t log_nc = 0;
  while ((1ull << log_nc) < n_constraints) ++log_nc;
  return log_nc;
}

extern "C" {

mlh_status mlh_cs_program_create(const uint8_t* bytes, uint64_t len, mlh_cs_program** out) {
  if (!bytes || !out) return MLH_ERR_INVALID;
  std::unique_ptr<mlh_cs_program> p(new mlh_cs_program());
  if (!cs_decode(bytes, len, p->p)) return MLH_ERR_INVALID;
  *out = p.release();
  return MLH_OK;
}
void mlh_cs_program_destroy(mlh_cs_program* prog) { delete prog; }
uint32_t mlh_cs_program_width(const mlh_cs_program* prog) { return prog ? prog->p.width : 0; }
uint32_t mlh_cs_program_degree(const mlh_cs_program* prog) { return prog ? prog->p.degree : 0; }
uint32_t mlh_cs_program_n_constraints(const mlh_cs_program* prog) {
  return prog ? prog->p.n_constraints : 0;
}
uint32_t mlh_cs_program_n_randoms(const mlh_cs_program* prog) {
  return prog ? prog->p.n_randoms : 0;
}

mlh_status mlh_cs_program_evaluate(const mlh_cs_program* prog, const uint8_t* host_values,
                                   const uint8_t* host_randoms, const uint8_t* host_mask,
                                   uint8_t out[16]) {
  if (!prog || !host_values || !host_mask || !out || (prog->p.n_randoms && !host_randoms))
    return MLH_ERR_INVALID;
  std::vector<u128> v, r, m;
  if (!load_canonical(host_values, prog->p.width, v) ||
      !load_canonical(host_randoms, prog->p.n_randoms, r) ||
      !load_canonical(host_mask, prog->p.n_constraints, m))
    return MLH_ERR_INVALID;
  h_store(out, cs_host_eval(prog->p, v.data(), r.data(), m.data()));
  return MLH_OK;
}

mlh_status mlh_cs_launch_info(const mlh_cs_program* prog, uint32_t log_height, uint32_t* threads,
                              uint32_t* blocks) {
  if (!prog || !threads || !blocks || log_height < 1 || log_height > kCsMaxLogHeight)
    return MLH_ERR_INVALID;
  *threads = cs_threads(cs_slots(prog->p));
  *blocks = cs_blocks(1ull << (log_height - 1), *threads);
  return MLH_OK;
}

// ---- fill programs (cs_program.hpp): decoder, accessors, host interpreter ----

mlh_status mlh_fill_program_create(const uint8_t* bytes, uint64_t len, mlh_fill_program** out) {
  if (!bytes || !out) return MLH_ERR_INVALID;
  std::unique_ptr<mlh_fill_program> p(new mlh_fill_program());
  if (!fill_decode(bytes, len, p->p)) return MLH_ERR_INVALID;
  *out = p.release();
  return MLH_OK;
}
void mlh_fill_program_destroy(mlh_fill_program* prog) { delete prog; }
uint32_t mlh_fill_program_width(const mlh_fill_program* prog) { return prog ? prog->p.width : 0; }
uint32_t mlh_fill_program_n_randoms(const mlh_fill_program* prog) {
  return prog ? prog->p.n_randoms : 0;
}
uint32_t mlh_fill_program_n_outputs(const mlh_fill_program* prog) {
  return prog ? prog->p.n_outputs : 0;
}
uint32_t mlh_fill_program_n_inverses(const mlh_fill_program* prog) {
  return prog ? prog->p.n_inv : 0;
}
uint32_t mlh_fill_program_output_mask(const mlh_fill_program* prog) {
  return prog ? prog->p.out_mask : 0;
}

mlh_status mlh_fill_program_evaluate(const mlh_fill_program* prog, const uint8_t* host_row,
                                     const uint8_t* host_randoms, uint8_t* out_row) {
  if (!prog || !host_row || !out_row || (prog->p.n_randoms && !host_randoms)) return MLH_ERR_INVALID;
  std::vector<u128> v, r;
  if (!load_canonical(host_row, prog->p.width, v) ||
      !load_canonical(host_randoms, prog->p.n_randoms, r))
    return MLH_ERR_INVALID;
  u128 res[kCsMaxWidth];
  fill_host_eval(prog->p, v.data(), r.data(), res);
  for (uint32_t j = 0; j < prog->p.width; ++j) h_store(out_row + 16ull * j, res[j]);
  return MLH_OK;
}

mlh_status mlh_trace_fill_launch_info(const mlh_fill_program* prog, uint32_t log_height,
                                      uint32_t* threads, uint32_t* rows_per_thread,
                                      uint32_t* blocks) {
  if (!prog || !threads || !rows_per_thread || !blocks || log_height > kCsMaxLogHeight)
    return MLH_ERR_INVALID;
  fill_shape(prog->p, 1ull << log_height, threads, rows_per_thread);
  *blocks = fill_blocks(prog->p, fill_chunks(1ull << log_height, *threads, *rows_per_thread),
                        *threads, *rows_per_thread);
  return MLH_OK;
}

mlh_status mlh_system_challenges(mlh_transcript* tr, uint32_t log_rows, uint32_t n_randoms,
                                 uint32_t n_constraints, uint8_t* row_out, uint8_t* trace_out,
                                 uint8_t* constraint_out, uint8_t* mask_out) {
  const uint32_t log_nc = cs_log_nc(n_constraints);
  if (!tr || log_rows > 64 || (log_rows && !row_out) || (n_randoms && !trace_out) ||
      (log_nc && !constraint_out) || (n_constraints && !mask_out))
    return MLH_ERR_INVALID;
  // vec![transcript.next_challenge(); n] evaluates the call once and clones it,
  // and next_challenge() leaves the state as it was (transcript.rs:35-38): one
  // value fills all three vectors (system.rs:138-140)
  uint8_t c[16];
  mlh_transcript_next_challenge(tr, c);
  for (uint32_t i = 0; i < log_rows; ++i) memcpy(row_out + 16ull * i, c, 16);
  for (uint32_t i = 0; i < n_randoms; ++i) memcpy(trace_out + 16ull * i, c, 16);
  for (uint32_t i = 0; i < log_nc; ++i) memcpy(constraint_out + 16ull * i, c, 16);
  const std::vector<u128> pts(log_nc, h_load(c));
  for (uint32_t k = 0; k < n_constraints; ++k)  // system.rs:93-95
    h_store(mask_out + 16ull * k, mask_evaluate(k, log_nc, pts.data()));
  return MLH_OK;
}

mlh_status mlh_system_trace_randoms(const mlh_transcript* tr, const uint8_t root1[32],
                                    uint32_t n_randoms, uint8_t* out) {
  if (!tr || !root1 || (n_randoms && !out)) return MLH_ERR_INVALID;
  mlh_transcript t = *tr;  // the caller's state stays as it is
  mlh_transcript_absorb(&t, root1, 32);
  uint8_t c[16];
  mlh_transcript_next_challenge(&t, c);  // vec![next_challenge(); n] (system.rs:139)
  for (uint32_t i = 0; i < n_randoms; ++i) memcpy(out + 16ull * i, c, 16);
  return MLH_OK;
}

}  // extern "C"

// The transcript head of every system proof (system_head.hpp; the order is
// mlhip.h's): the one place where the provers and the verifiers derive it.
mlh_status mlh::system_head(mlh_transcript* tr, const CsProgram& P, uint32_t log_height,
                            const uint8_t* public_digest, const uint8_t root1[32],
                            const uint8_t* root2, uint32_t sum_column_mask, const uint8_t sum[16], const uint8_t* column_sum, SystemHead* out) {
  if (!tr || !root1 || !sum || !out || (sum_column_mask && !column_sum)) return MLH_ERR_INVALID;
  std::vector<uint8_t> cons(16ull * cs_log_nc(P.n_constraints));
  if (public_digest) mlh_transcript_absorb(tr, public_digest, 32);  // 0.
  mlh_transcript_absorb(tr, root1, 32);                             // 1.
  uint8_t c[16];
  mlh_transcript_next_challenge(tr, c);  // 2. vec![next_challenge(); n] (system.rs:139)
  for (uint32_t i = 0; i < P.n_randoms; ++i) memcpy(out->randoms.data() + 16ull * i, c, 16);
  if (root2) mlh_transcript_absorb(tr, root2, 32);  // 3.
  const mlh_status st = mlh_system_challenges(tr, log_height, 0, P.n_constraints, out->row.data(),
                                              nullptr, cons.data(), out->mask.data());  // 4.
  if (st != MLH_OK) return st;
  memcpy(out->claim, sum, 16);
  if (sum_column_mask) {  // 5.
    mlh_transcript_absorb(tr, column_sum, 16);
    mlh_transcript_next_challenge(tr, out->beta);
    h_store(out->claim, h_add(h_load(sum), h_mul(h_load(out->beta), h_load(column_sum))));
  }
  return MLH_OK;
}

// System::verify_with_evaluations (sumcheck.rs:91-124); rs_out (optional)
// receives the challenges it derives.
// smask / beta: the sum columns' term (mlh_cs_sumcheck_verify_sums); sum is
// then the combined claim.
// delta_at (optional): the delta table's evaluation at the challenges, handed
// in by a caller whose table is not eq(row points) -- the shift reduction's
// succ(rs, .); host_row_points is then not read.  Null: Delta::evaluate of the
// row points.
typedef u128 (*DeltaAtFn)(const void* user, const std::vector<u128>& rs);
static mlh_status cs_sumcheck_verify_rs(const mlh_cs_program* prog, uint32_t log_height,
                                        const uint8_t* host_row_points, const uint8_t* host_randoms,
                                        const uint8_t* host_mask, uint32_t smask, const uint8_t* beta,
                                        const uint8_t sum[16], const uint8_t* polys,
                                        const uint8_t* host_output, mlh_transcript* tr,
                                        std::vector<u128>* rs_out, DeltaAtFn delta_at = nullptr,
                                        const void* delta_user = nullptr) {
  if (!prog || (!host_row_points && !delta_at) || !host_mask || !sum || !polys || !host_output ||
      !tr || log_height < 1 || log_height > kCsMaxLogHeight || (prog->p.n_randoms && !host_randoms))
    return MLH_ERR_INVALID;
  const CsProgram& P = prog->p;
  if (smask && (!beta || h_load(beta) >= kModulus || (P.width < 32 && (smask >> P.width))))
    return MLH_ERR_INVALID;
  const uint32_t L = log_height, D = P.points();
  std::vector<u128> row, rnd, mask, output, co;
  if ((!delta_at && !load_canonical(host_row_points, L, row)) ||
      !load_canonical(host_randoms, P.n_randoms, rnd) ||
      !load_canonical(host_mask, P.n_constraints, mask) || h_load(sum) >= kModulus)
    return MLH_ERR_INVALID;
  if (!load_canonical(host_output, P.width, output) || !load_canonical(polys, L * D, co))
    return MLH_ERR_VERIFY;
  TranscriptGuard guard(tr);
  const u128 inv2 = h_inv(2);
  std::vector<u128> rs, pol(D + 1);
  u128 claim = h_load(sum), r = 0;
  for (uint32_t k = 0; k < L; ++k) {  // sumcheck.rs:98-116
    u128 sc = 0;
    for (uint32_t j = 0; j < D; ++j) {
      mlh_transcript_absorb(tr, polys + 16ull * (k * D + j), 16);
      pol[j + 1] = co[k * D + j];
      sc = h_add(sc, pol[j + 1]);
    }
    pol[0] = h_mul(h_sub(claim, sc), inv2);  // to_polynomial (:269-276)
    uint8_t c[16];
    mlh_transcript_next_challenge(tr, c);
    r = h_load(c);
    rs.push_back(r);
    claim = horner(pol, r);
  }
  u128 delta = 1;  // Delta::evaluate (evaluation.rs:80-90)
  if (delta_at)
    delta = delta_at(delta_user, rs);
  else
    for (uint32_t i = 0; i < L; ++i)
      delta = h_mul(delta, h_add(h_mul(row[i], rs[i]), h_mul(h_sub(1, row[i]), h_sub(1, rs[i]))));
  const u128 comp = cs_host_eval(P, output.data(), rnd.data(), mask.data());
  u128 lin = 0;  // beta * sum_{j in S} output[j]
  if (smask) {
    for (uint32_t j = 0; j < P.width; ++j)
      if ((smask >> j) & 1u) lin = h_add(lin, output[j]);
    lin = h_mul(lin, h_load(beta));
  }
  if (h_add(h_mul(delta, comp), lin) != claim) return MLH_ERR_VERIFY;  // :119-123
  guard.keep();
  if (rs_out) *rs_out = rs;
  return MLH_OK;
}

// succ(x, y) = sum_i eq(x, i) eq(y, (i + 1) mod 2^n) in closed form (mlhip.h):
// bit b of the row index <-> point[n - 1 - b].  One pass from the top bit down
// for the suffix products of (x_b y_b + (1 - x_b)(1 - y_b)), one from bit 0 up
// with the running product of x_b (1 - y_b).
static u128 succ_evaluate(const u128* x, const u128* y, uint32_t n) {
  std::vector<u128> hi(n + 1, 1);  // hi[k] = prod_{b >= k} eq1(x_b, y_b)
  for (uint32_t k = n; k-- > 0;) {
    const u128 xb = x[n - 1 - k], yb = y[n - 1 - k];
    hi[k] = h_mul(hi[k + 1], h_add(h_mul(xb, yb), h_mul(h_sub(1, xb), h_sub(1, yb))));
  }
  u128 low = 1, acc = 0;  // low = prod_{b < k} x_b (1 - y_b)
  for (uint32_t k = 0; k < n; ++k) {
    const u128 xb = x[n - 1 - k], yb = y[n - 1 - k];
    acc = h_add(acc, h_mul(h_mul(low, h_mul(h_sub(1, xb), yb)), hi[k + 1]));
    low = h_mul(low, h_mul(xb, h_sub(1, yb)));
  }
  return h_add(acc, low);  // the wrap: all ones -> all zeros
}
static u128 succ_at(const void* user, const std::vector<u128>& rs2) {
  const std::vector<u128>& rs = *static_cast<const std::vector<u128>*>(user);
  return succ_evaluate(rs.data(), rs2.data(), (uint32_t)rs.size());
}

// The shift part of a shifted proof as the verifier core sees it (null: none,
// or K = 0).
struct ShiftVerify {
  const uint32_t* cols;
  uint32_t K;
  const uint8_t* polys;    // [L][2][16]
  const uint8_t* output2;  // [W][16]
  const mlh_batched_pcs_proof* pcs1;
  const mlh_batched_pcs_proof* pcs2;  // null: one phase
};

// What follows the header checks of the system verifiers: the head, the
// sumcheck against the claimed output, the shift reduction (sh; mlhip.h, step
// 7), then the opening(s) at its rs -- pcs1 for the first pcs1->fri.num_codes
// columns, pcs2 (null: one phase) for the rest -- and, with sh, those of the
// same columns at rs'.  Every rejection is MLH_ERR_VERIFY with the transcript
// as at entry.
// pub (null: none; the caller has checked that it fits L and the width): the
// last pub->p.count() of the W real columns are public -- its digest is
// absorbed first, the openings cover the columns below them, and output (and,
// with sh, output2) must hold the spec's own evaluations there (mlhip.h,
// public columns).
static mlh_status system_verify_core(const mlh_cs_program* prog, uint32_t L, uint32_t sum_column_mask,
                                     const uint8_t sum[16], const uint8_t* column_sum,
                                     const uint8_t* polys, const uint8_t* output,
                                     const mlh_batched_pcs_proof* pcs1,
                                     const mlh_batched_pcs_proof* pcs2, mlh_transcript* tr,
                                     const ShiftVerify* sh = nullptr,
                                     const mlh_public_columns* pub = nullptr) {
  TranscriptGuard guard(tr);
  SystemHead h(prog->p, L);
  std::vector<u128> rs, rs2;
  mlh_status st = system_head(tr, prog->p, L, pub ? pub->p.digest : nullptr,
                              pcs1->fri.batch_commitment,
                              pcs2 ? pcs2->fri.batch_commitment : nullptr, sum_column_mask, sum,
                              column_sum, &h);
  if (st == MLH_OK)
    st = cs_sumcheck_verify_rs(prog, L, h.row.data(), h.randoms.data(), h.mask.data(),
                               sum_column_mask, h.beta, h.claim, polys, output, tr, &rs);
  const uint32_t P1 = pcs1->fri.num_codes;
  // the public columns' evaluations at `at` against the proof's, element for element
  const auto public_ok = [&](const std::vector<u128>& at, const uint8_t* out) {
    const uint32_t F = pub->p.count(), W = prog->p.width - (sh ? sh->K : 0);
    std::vector<u128> want(F);
    pc_evaluate(pub->p, L, at.data(), want.data());
    for (uint32_t j = 0; j < F; ++j)
      if (h_load(out + 16ull * (W - F + j)) != want[j]) return false;
    return true;
  };
  if (st == MLH_OK && pub && !public_ok(rs, output)) st = MLH_ERR_VERIFY;
  if (st == MLH_OK && sh) {
    const uint32_t W = prog->p.width - sh->K;
    mlh_cs_program sp;
    std::vector<uint8_t> lambdas;
    uint8_t claim2[16], one[16];
    h_store(one, 1);
    if (!cs_shift_program(W, sh->cols, sh->K, sp.p)) return MLH_ERR_VERIFY;
    shift_challenge(tr, output, W, sh->K, &lambdas, claim2);
    st = cs_sumcheck_verify_rs(&sp, L, nullptr, lambdas.data(), one, 0, nullptr, claim2, sh->polys,
                               sh->output2, tr, &rs2, succ_at, &rs);
    if (st == MLH_OK && pub && !public_ok(rs2, sh->output2)) st = MLH_ERR_VERIFY;
  }
  std::vector<uint8_t> in(16ull * L);
  const auto open = [&](const std::vector<u128>& at, const uint8_t* out,
                        const mlh_batched_pcs_proof* a, const mlh_batched_pcs_proof* b) {
    for (uint32_t i = 0; i < L; ++i) h_store(in.data() + 16ull * i, at[i]);
    mlh_status s = mlh_batched_pcs_verify(a, L, in.data(), out, tr);
    if (s == MLH_OK && b) s = mlh_batched_pcs_verify(b, L, in.data(), out + 16ull * P1, tr);
    return s;
  };
  if (st == MLH_OK) st = open(rs, output, pcs1, pcs2);
  if (st == MLH_OK && sh) st = open(rs2, sh->output2, sh->pcs1, sh->pcs2);
  if (st != MLH_OK) return MLH_ERR_VERIFY;
  guard.keep();
  return MLH_OK;
}

extern "C" {

mlh_status mlh_cs_sumcheck_verify(const mlh_cs_program* prog, uint32_t log_height,
                                  const uint8_t* host_row_points, const uint8_t* host_randoms,
                                  const uint8_t* host_mask, const uint8_t sum[16],
                                  const uint8_t* polys, const uint8_t* host_output,
                                  mlh_transcript* tr) {
  return cs_sumcheck_verify_rs(prog, log_height, host_row_points, host_randoms, host_mask, 0, nullptr,
                               sum, polys, host_output, tr, nullptr);
}

mlh_status mlh_cs_sumcheck_verify_sums(const mlh_cs_program* prog, uint32_t log_height,
                                       const uint8_t* host_row_points, const uint8_t* host_randoms,
                                       const uint8_t* host_mask, uint32_t sum_column_mask,
                                       const uint8_t* beta, const uint8_t claim[16],
                                       const uint8_t* polys, const uint8_t* host_output,
                                       mlh_transcript* tr) {
  return cs_sumcheck_verify_rs(prog, log_height, host_row_points, host_randoms, host_mask,
                               sum_column_mask, beta, claim, polys, host_output, tr, nullptr);
}

mlh_status mlh_system_verify(const mlh_cs_program* prog, uint32_t log_height, const uint8_t sum[16],
                             const mlh_system_proof* proof, mlh_transcript* tr) {
  if (!prog || !sum || !proof || !tr || !proof->sumcheck_polys || !proof->output ||
      !proof->pcs.sumcheck_polys)
    return MLH_ERR_INVALID;
  const CsProgram& P = prog->p;
  if (log_height < 1 || log_height > kCsMaxLogHeight || proof->log_height != log_height ||
      proof->width != P.width || proof->degree != P.degree || proof->pcs.fri.num_codes != P.width ||
      h_load(sum) >= kModulus)
    return MLH_ERR_VERIFY;
  return system_verify_core(prog, log_height, 0, sum, nullptr, proof->sumcheck_polys, proof->output,
                            &proof->pcs, nullptr, tr);
}

mlh_status mlh_system_verify_phased(const mlh_cs_program* prog, uint32_t log_height,
                                    uint32_t pre_random_columns, uint32_t sum_column_mask,
                                    const uint8_t sum[16], const uint8_t column_sum[16],
                                    const mlh_phased_proof* proof, mlh_transcript* tr) {
  if (!prog || !sum || !column_sum || !proof || !tr || !proof->sumcheck_polys || !proof->output ||
      !proof->pcs[0].sumcheck_polys)
    return MLH_ERR_INVALID;
  const CsProgram& P = prog->p;
  const uint32_t L = log_height, W = P.width, P1 = pre_random_columns;
  if (L < 1 || L > kCsMaxLogHeight || P1 < 1 || P1 > W || (W < 32 && (sum_column_mask >> W)) ||
      proof->log_height != L || proof->width != W || proof->degree != P.degree ||
      proof->pre_random_columns != P1 || proof->sum_column_mask != sum_column_mask ||
      proof->pcs[0].fri.num_codes != P1 ||
      (P1 < W && (!proof->pcs[1].sumcheck_polys || proof->pcs[1].fri.num_codes != W - P1)) ||
      h_load(sum) >= kModulus || h_load(column_sum) >= kModulus)
    return MLH_ERR_VERIFY;
  return system_verify_core(prog, L, sum_column_mask, sum, column_sum, proof->sumcheck_polys,
                            proof->output, &proof->pcs[0], P1 < W ? &proof->pcs[1] : nullptr, tr);
}

mlh_status mlh_shift_succ_evaluate(const uint8_t* x, const uint8_t* y, uint32_t n, uint8_t out[16]) {
  if (!out || n > 64 || (n && (!x || !y))) return MLH_ERR_INVALID;
  std::vector<u128> xv, yv;
  if (!load_canonical(x, n, xv) || !load_canonical(y, n, yv)) return MLH_ERR_INVALID;
  h_store(out, succ_evaluate(xv.data(), yv.data(), n));
  return MLH_OK;
}

// ---- public columns (public_columns.hpp; mlhip.h gives the format and the protocol) ----
mlh_status mlh_public_columns_create(const uint8_t* wire, uint64_t len, mlh_public_columns** out) {
  if (!wire || !out) return MLH_ERR_INVALID;
  std::unique_ptr<mlh_public_columns> s(new mlh_public_columns());
  if (!pc_decode(wire, len, s->p)) return MLH_ERR_INVALID;
  *out = s.release();
  return MLH_OK;
}
void mlh_public_columns_destroy(mlh_public_columns* spec) { delete spec; }
uint32_t mlh_public_columns_count(const mlh_public_columns* spec) {
  return spec ? spec->p.count() : 0;
}
mlh_status mlh_public_columns_digest(const mlh_public_columns* spec, uint8_t out[32]) {
  if (!spec || !out) return MLH_ERR_INVALID;
  memcpy(out, spec->p.digest, 32);
  return MLH_OK;
}
mlh_status mlh_public_columns_evaluate(const mlh_public_columns* spec, uint32_t log_height,
                                       const uint8_t* point, uint8_t* out) {
  if (!spec || !out || (log_height && !point) || !spec->p.fits(log_height)) return MLH_ERR_INVALID;
  std::vector<u128> x, v(spec->p.count());
  if (!load_canonical(point, log_height, x)) return MLH_ERR_INVALID;
  pc_evaluate(spec->p, log_height, x.data(), v.data());
  for (uint32_t j = 0; j < spec->p.count(); ++j) h_store(out + 16ull * j, v[j]);
  return MLH_OK;
}

mlh_status mlh_system_verify_public(const mlh_cs_program* prog, uint32_t log_height,
                                    uint32_t pre_random_columns, uint32_t sum_column_mask,
                                    const uint32_t* shift_columns, uint32_t n_shifts,
                                    const mlh_public_columns* spec, const uint8_t sum[16],
                                    const uint8_t column_sum[16], const mlh_shifted_proof* proof,
                                    mlh_transcript* tr) {
  const uint32_t K = n_shifts, F = spec ? spec->p.count() : 0;
  if (!prog || !sum || !column_sum || !proof || !tr || !proof->sumcheck_polys || !proof->output ||
      !proof->pcs[0].sumcheck_polys || (K && !shift_columns) ||
      !shift_list_ok(prog->p.width, shift_columns, K) || F >= prog->p.width - K ||
      (spec && !spec->p.fits(log_height)))
    return MLH_ERR_INVALID;
  const CsProgram& P = prog->p;
  const uint32_t L = log_height, W = P.width - K, C = W - F, P1 = pre_random_columns;
  const bool two = P1 < C;  // C: the committed columns
  if (L < 1 || L > kCsMaxLogHeight || P1 < 1 || P1 > C || (W < 32 && (sum_column_mask >> W)) ||
      proof->log_height != L || proof->width != W || proof->degree != P.degree ||
      proof->pre_random_columns != P1 || proof->sum_column_mask != sum_column_mask ||
      proof->n_shifts != K || proof->pcs[0].fri.num_codes != P1 ||
      (two && (!proof->pcs[1].sumcheck_polys || proof->pcs[1].fri.num_codes != C - P1)) ||
      h_load(sum) >= kModulus || h_load(column_sum) >= kModulus)
    return MLH_ERR_VERIFY;
  for (uint32_t k = 0; k < 32; ++k)
    if (proof->shift_columns[k] != (k < K ? shift_columns[k] : 0u)) return MLH_ERR_VERIFY;
  if (!K)
    return system_verify_core(prog, L, sum_column_mask, sum, column_sum, proof->sumcheck_polys,
                              proof->output, &proof->pcs[0], two ? &proof->pcs[1] : nullptr, tr,
                              nullptr, spec);
  if (!proof->shift_polys || !proof->output2 || !proof->pcs_shift[0].sumcheck_polys ||
      proof->pcs_shift[0].fri.num_codes != P1 ||
      (two && (!proof->pcs_shift[1].sumcheck_polys || proof->pcs_shift[1].fri.num_codes != C - P1)))
    return MLH_ERR_VERIFY;
  const ShiftVerify sh = {shift_columns, K, proof->shift_polys, proof->output2, &proof->pcs_shift[0],
                          two ? &proof->pcs_shift[1] : nullptr};
  return system_verify_core(prog, L, sum_column_mask, sum, column_sum, proof->sumcheck_polys,
                            proof->output, &proof->pcs[0], two ? &proof->pcs[1] : nullptr, tr, &sh,
                            spec);
}

mlh_status mlh_system_verify_shifted(const mlh_cs_program* prog, uint32_t log_height,
                                     uint32_t pre_random_columns, uint32_t sum_column_mask,
                                     const uint32_t* shift_columns, uint32_t n_shifts,
                                     const uint8_t sum[16], const uint8_t column_sum[16],
                                     const mlh_shifted_proof* proof, mlh_transcript* tr) {
  return mlh_system_verify_public(prog, log_height, pre_random_columns, sum_column_mask,
                                  shift_columns, n_shifts, nullptr, sum, column_sum, proof, tr);
}

}  // extern "C"
