// The FRI prover's host side (fri_prover.hip) as the PCS provers, the batched
// PCS opening and the trace commitment (capi.hip) use it: the layers, the
// device-transcript commit loop, the query tails.  Not part of the public C ABI.
#pragma once
#include "batched.hpp"
#include "context.hpp"
#include "merkle.hpp"
#include "sumcheck.hpp"
#include "transcript_dev.hpp"

struct FriLayer {
  const fe* values = nullptr;  // 2^log_n values (pairs i, i + n/2)
  void* owned_values = nullptr;
  uint8_t* tree = nullptr;  // 2L-1 digests, L = n/2
  uint32_t log_n = 0;
  uint8_t root[32];
};

struct mlh_fri_prover {
  mlh_ctx* ctx;
  uint32_t log_code;
  // gen_pows of the reference's FriProverData calls (fri/mod.rs:58,79,136,261):
  // a geometric table of 2^log_gp powers of gp_gen; fold twiddle
  // gen_pows[len - i 2^k] = gp_gen^(-i 2^k).  Default: the code's domain.
  u128 gp_gen;
  uint32_t log_gp;
  std::vector<FriLayer> layers;
  bool has_last = false;
  uint8_t last[16];
  mlh_fri_prover(mlh_ctx* c, uint32_t lc)
      : ctx(c), log_code(lc), gp_gen(mlh::h_pow2_generator(lc)), log_gp(lc) {}
  ~mlh_fri_prover() {
    for (auto& l : layers) {
      pool_free(ctx, l.owned_values);
      pool_free(ctx, l.tree);
    }
  }
};

// The batch layer of BatchedFriProverData::init (batched_fri.rs:41-81): the tree over the
// m codes' ([m][N]) RS pairs, N/2 leaves; ra (optional) absorbs its root on the device.
mlh_status batch_layer_commit(mlh_ctx* ctx, const fe* codes, uint32_t m, uint64_t N, uint8_t* tree,
                              mlh::RootAbsorb ra = mlh::RootAbsorb());

// Device-side commit loop state: [transcript | r_0..r_steps | last (16) |
// flag (16) | batch root (32) | fingerprint r (16) | roots 32 x (steps + 1) |
// polys 32 x steps | prev (16) | extra (16 x n_extra)].
struct FriDevLoop {
  mlh_ctx* ctx;
  mlh_fri_prover* p;
  const fe *tlo = nullptr, *thi = nullptr;
  const fe* twt = nullptr;  // every fold layer's twiddles (fold_layer_table), or nullptr
  PoolBuf scratch;
  size_t off_r = 128, off_last = 0, off_flag = 0, off_broot = 0, off_fr = 0, off_roots = 0,
         off_polys = 0, off_prev = 0, off_extra = 0;
  bool done = false;
  // batched mode: the m codes ([m][N]) and the batch-layer tree
  const fe* codes = nullptr;
  uint32_t m = 0;
  PoolBuf btree;
  const uint8_t* bt = nullptr;  // the batch-layer tree: btree, or the caller's built one
  explicit FriDevLoop(mlh_ctx* c, mlh_fri_prover* pr) : ctx(c), p(pr), scratch(c), btree(c) {}
  uint8_t* sb() const { return scratch.as<uint8_t>(); }
  mlh::DevSha* dt() const { return reinterpret_cast<mlh::DevSha*>(sb()); }
  fe* r(uint32_t k) const { return reinterpret_cast<fe*>(sb() + off_r) + k; }
  uint8_t* root(uint32_t t) const { return sb() + off_roots + 32 * t; }
  fe* poly(uint32_t k) const { return reinterpret_cast<fe*>(sb() + off_polys) + 2 * k; }
  fe* prev() const { return reinterpret_cast<fe*>(sb() + off_prev); }
  fe* fr() const { return reinterpret_cast<fe*>(sb() + off_fr); }
  fe* extra() const { return reinterpret_cast<fe*>(sb() + off_extra); }

  // first: the scratch (n_extra 16-byte slots at extra()), the fold tables, the transcript
  mlh_status layout(uint32_t log_code, const mlh_transcript* tr, size_t n_extra = 0);

  // BatchedFriProverData::init (batched_fri.rs:41-98): batch layer over the
  // m codes' RS pairs, absorb its root, fingerprint_r = next_challenge(),
  // absorb LE16(fingerprint_r); r_0 = next_challenge() if challenge_r0.
  // built_tree (optional): the batch layer's tree over these codes, already
  // built (a trace commitment's); only its root is absorbed then.
  mlh_status init_batched(const fe* dev_codes, uint32_t num_codes, uint32_t log_code,
                          const mlh_transcript* tr, bool challenge_r0, size_t n_extra = 0,
                          const uint8_t* built_tree = nullptr);

  // FriProverData::init after layout() (whose extra() slots the caller may
  // fill first): the commit of layer 0.  poly0 (optional): 32 bytes absorbed
  // after root 0, before its challenge
  mlh_status init(const void* dev_code, uint32_t log_code, bool challenge_after_root0,
                  const fe* poly0 = nullptr);

  // fold_step k with the challenge at rp (device); absorbs the new root (or
  // the last element) and (poly_next) 32 more bytes; writes next_challenge()
  // to r(k + 1) if challenge_next.
  // job (optional): a PCS round run by an extra workgroup of the fold launch
  mlh_status step(uint32_t k, const fe* rp, bool challenge_next, const fe* poly_next = nullptr,
                  const mlh::PcsJob* job = nullptr);
  // batched_fold_step (batched_fri.rs:100-176), fold 0: the fingerprinted pairs
  // of the codes into the inner prover's first layer (or the last element).
  mlh_status step_batched(const fe* rp, bool challenge_next, const fe* poly_next = nullptr);

  // one sync: challenges, last element, RS flag, roots (+ polys_bytes of
  // sumcheck polys); then the cooperative kernels' failure word
  mlh_status finish(size_t polys_bytes);
  // the device's challenge slot k, as copied back by finish()
  const uint8_t* host_r(uint32_t k) const { return ctx->pinned + 16 * k; }
  const uint8_t* host_polys() const { return ctx->pinned + (off_polys - off_r); }
  const uint8_t* host_broot() const { return ctx->pinned + (off_broot - off_r); }
  const uint8_t* host_fr() const { return ctx->pinned + (off_fr - off_r); }
};

// FriProof::prove tail (fri/mod.rs:266-284) and its batched form (batched_fri.rs:287-300; lp
// committed the batch layer): query indices from the transcript, openings, last_random.
mlh_status fri_queries(mlh_ctx* ctx, mlh_fri_prover* p, mlh_transcript* tr, mlh_fri_proof* proof);
mlh_status batched_queries(mlh_ctx* ctx, FriDevLoop& lp, mlh_transcript* tr,
                           mlh_batched_fri_proof* pf);
