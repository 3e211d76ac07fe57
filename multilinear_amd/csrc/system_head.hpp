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

// 1. absorb root1; 2. the trace randoms; 3. absorb root2 (null: one phase);
// 4. the row and constraint challenges and the mask (mlh_system_challenges);
// 5. with sum columns (sum_column_mask != 0; column_sum required), absorb
// LE16(column_sum) and draw beta; claim = sum + beta * column_sum, else sum.
// With root2 null and no sum columns this is the one-phase order byte for
// byte: next_challenge() leaves the state as it was, so step 2's value is the
// one step 4 draws.  out: a SystemHead(P, log_height).  The caller guards the
// transcript.
mlh_status system_head(mlh_transcript* tr, const CsProgram& P, uint32_t log_height,
                       const uint8_t root1[32], const uint8_t* root2, uint32_t sum_column_mask,
                       const uint8_t sum[16], const uint8_t* column_sum, SystemHead* out);

}  // namespace mlh
