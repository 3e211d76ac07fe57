// The sumcheck and PCS provers' host side (pcs_prover.hip) as the trace
// commitment, the constraint-system prove and the system proof (capi.hip) use
// it: the round buffer of a sumcheck prove with the transcript on the device
// and the batched PCS's two halves.  Not part of the public C ABI.
#pragma once
#include "context.hpp"
#include "transcript_dev.hpp"

// [DevSha 128 | claim 16 | polys 16 D x L | rs 16 x L | extra]: D field
// elements per round polynomial, L rounds.  One copy of polys | rs (| extra)
// to ctx->pinned ends the prove; `host` keeps it for the replay and the caller.
struct RoundBuf {
  mlh_ctx* ctx;
  uint32_t D, L;
  PoolBuf buf;
  std::vector<uint8_t> host;
  RoundBuf(mlh_ctx* c, uint32_t D_, uint32_t L_) : ctx(c), D(D_), L(L_), buf(c) {}
  size_t out_bytes() const { return 16ull * (D + 1) * L; }
  mlh_status alloc(size_t extra_bytes = 0) { return buf.alloc(144 + out_bytes() + extra_bytes); }
  mlh::DevSha* dt() const { return buf.as<mlh::DevSha>(); }
  fe* prev() const { return reinterpret_cast<fe*>(buf.as<uint8_t>() + 128); }
  fe* poly(uint32_t k) const { return reinterpret_cast<fe*>(buf.as<uint8_t>() + 144) + (uint64_t)D * k; }
  fe* r(uint32_t k) const { return poly(L) + k; }
  fe* extra() const { return r(L); }
  // the transcript's state and the claim, from the host
  mlh_status seed(const mlh_transcript* tr, const uint8_t claim[16]) {
    static_assert(sizeof(mlh::DevSha) <= 128, "DevSha slot");
    memcpy(ctx->pinned, &tr->sha, sizeof(mlh::DevSha));
    memcpy(ctx->pinned + 128, claim, 16);
    HIP_TRY(ctx, hipMemcpyAsync(buf.p, ctx->pinned, 144, hipMemcpyHostToDevice, ctx->stream));
    return MLH_OK;
  }
  // polys | rs to the host: the prove's one sync
  mlh_status read_back() {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned, poly(0), out_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    from_pinned();
    return MLH_OK;
  }
  // the same from ctx->pinned, where the prove's last kernel left them (HostOut)
  void from_pinned(size_t extra = 0) { host.assign(ctx->pinned, ctx->pinned + out_bytes() + extra); }
  // host transcript replay (sumcheck.rs:188-199): per round absorb the D
  // elements, expect r_k; tr advances only if every challenge agrees
  mlh_status replay(mlh_transcript* tr) const {
    ReplayCheck rc(ctx, tr);
    for (uint32_t k = 0; k < L; ++k) {
      rc.absorb(host.data() + 16ull * D * k, 16ull * D);
      rc.expect(host.data() + 16ull * D * L + 16ull * k);
    }
    return rc.status();
  }
  void copy_out(uint8_t* polys_out, uint8_t* rs_out) const {
    if (polys_out) memcpy(polys_out, host.data(), 16ull * D * L);
    if (rs_out) memcpy(rs_out, host.data() + 16ull * D * L, 16ull * L);
  }
};

// The transcript-independent front of BatchedPCSProof::prove
// (batched_pcs.rs:135-149): per polynomial to_coefficient, bit reverse and
// reed_solomon at blow-up 2, into dev_codes ([num_polys][2^(n_vars+1)]).
mlh_status batched_pcs_codes(mlh_ctx* ctx, const void* dev_evals, uint32_t num_polys,
                             uint32_t n_vars, fe* dev_codes);

// BatchedPCSProof::prove from the point where the codes exist
// (batched_pcs.rs:150-180): dev_codes as batched_pcs_codes leaves them,
// dev_evals the MLEs; built_tree (optional) the batch layer's tree over those
// codes (FriDevLoop::init_batched).
mlh_status batched_pcs_open(mlh_ctx* ctx, const fe* dev_codes, const void* dev_evals,
                            const uint8_t* built_tree, uint32_t num_polys, uint32_t n_vars,
                            const uint8_t* inputs, const uint8_t* outputs, mlh_transcript* tr,
                            mlh_batched_pcs_proof* proof);
