// What the system provers (capi.hip) and verifiers (verify.cpp) share
// (internal to libmlhip): the transcript head of the system proof -- steps 1-5
// of the order in mlhip.h, derived in one place for all four entry points --
// and the guard that leaves a caller's transcript untouched on failure.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/mlhip.h"
#include "cs_program.hpp"
#include "host_transcript.hpp"
#include "public_columns.hpp"

// Restores the caller's transcript to its state at construction unless keep()
// was called: a failed prove or verify leaves it untouched (mlhip.h), the root
// absorbed first included.
struct TranscriptGuard {
  mlh_transcript* tr;
  mlh::HostSha256 saved;
  bool kept = false;
  explicit TranscriptGuard(mlh_transcript* t) : tr(t), saved(t->sha) {}
  TranscriptGuard(const TranscriptGuard&) = delete;
  TranscriptGuard& operator=(const TranscriptGuard&) = delete;
  ~TranscriptGuard() {
    if (!kept) tr->sha = saved;
  }
  void keep() { kept = true; }
};

namespace mlh {

// The challenges of one system proof, LE16 each.
struct SystemHead {
  std::vector<uint8_t> row;      // log_height row points
  std::vector<uint8_t> randoms;  // n_randoms trace randoms
  std::vector<uint8_t> mask;     // n_constraints mask values
  uint8_t beta[16] = {0};        // zero without sum columns
  uint8_t claim[16] = {0};       // sum + beta * column_sum
  SystemHead(const CsProgram& P, uint32_t log_height)
      : row(16ull * log_height), randoms(16ull * P.n_randoms), mask(16ull * P.n_constraints) {}
};

// 0. with public columns (public_digest non-null), absorb the spec's 32-byte
// digest; 1. absorb root1; 2. the trace randoms; 3. absorb root2 (null: one phase);
// 4. the row and constraint challenges and the mask (mlh_system_challenges);
// 5. with sum columns (sum_column_mask != 0; column_sum required), absorb
// LE16(column_sum) and draw beta; claim = sum + beta * column_sum, else sum.
// With no public columns, root2 null and no sum columns this is the one-phase order byte for
// byte: next_challenge() leaves the state as it was, so step 2's value is the
// one step 4 draws.  out: a SystemHead(P, log_height).  The caller guards the
// transcript.
mlh_status system_head(mlh_transcript* tr, const CsProgram& P, uint32_t log_height,
                       const uint8_t* public_digest, const uint8_t root1[32], const uint8_t* root2,
                       uint32_t sum_column_mask, const uint8_t sum[16], const uint8_t* column_sum, SystemHead* out);

// The shift list of a shifted system over a program of width wext = W + K: K
// distinct source columns below W (K = 0: no list).  Prover and verifier refuse
// the same lists.
inline bool shift_list_ok(uint32_t wext, const uint32_t* cols, uint32_t n_shifts) {
  if (n_shifts >= wext || wext > kCsMaxWidth || (n_shifts && !cols)) return false;
  const uint32_t W = wext - n_shifts;
  uint32_t seen = 0;
  for (uint32_t k = 0; k < n_shifts; ++k) {
    if (cols[k] >= W || ((seen >> cols[k]) & 1u)) return false;
    seen |= 1u << cols[k];
  }
  return true;
}

// Step 7's challenge and what both sides derive from it (mlhip.h, shifted
// proof): absorb the W' elements of `output`, draw lambda, then the randoms
// lambda^0 .. lambda^(K-1) (LE16 each) and the claim sum_k lambda^k output[W + k].
// output: canonical elements.
inline void shift_challenge(mlh_transcript* tr, const uint8_t* output, uint32_t W, uint32_t K,
                            std::vector<uint8_t>* randoms, uint8_t claim[16]) {
  mlh_transcript_absorb(tr, output, 16ull * (W + K));
  uint8_t c[16];
  mlh_transcript_next_challenge(tr, c);
  const u128 lambda = h_load(c);
  randoms->resize(16ull * K);
  u128 pw = 1, acc = 0;
  for (uint32_t k = 0; k < K; ++k) {
    h_store(randoms->data() + 16ull * k, pw);
    acc = h_add(acc, h_mul(pw, h_load(output + 16ull * (W + k))));
    pw = h_mul(pw, lambda);
  }
  h_store(claim, acc);
}

}  // namespace mlh
