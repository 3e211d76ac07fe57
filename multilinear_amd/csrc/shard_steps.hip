// The rank-local steps of the multi-GPU schedules behind the C ABI: what one
// rank runs between two collectives.  Kernels: dist.hip, fri.hip, merkle.hip,
// sumcheck.hip, transcript_dev.hpp; the orchestration that calls these steps
// is sharded.hip (tests/dist_spec.py restates it in Python as the spec the CPU
// tests run).  Host code only.
#include "context.hpp"
#include "dist.hpp"
#include "host_sha256.hpp"
#include "host_transcript.hpp"
#include "merkle.hpp"
#include "sumcheck.hpp"
#include "tables.hpp"
#include "transcript_dev.hpp"

using namespace mlh;

namespace {

// One fold of a block-layout FRI layer (mlh_shard_fri_fold and its three
// variants).  The challenge is r (16 host bytes) or, where r is null, read by
// the kernel from dev_r; with_tree: the folded layer's tree is built into
// dev_tree by the same launch.
mlh_status shard_fold(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local, uint32_t k,
                      uint32_t log_domain, const uint8_t* r, const void* dev_r, void* dev_next,
                      bool with_tree, void* dev_tree, uint32_t log_s, uint32_t log_p,
                      uint32_t rank) {
  const bool dr = r == nullptr;  // challenge on the device: dev_r is checked after the sizes
  if (!ctx || !dev_layer || !dev_next) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_domain > 40 || log_p > 4 || (rank >> log_p) || log_local < 1 ||
      log_local + log_p + k != log_domain)
    return fail(ctx, MLH_ERR_INVALID, "local layer must be 2^(log_domain - k - log_p)");
  if (log_s + 1 > log_local && log_p > 0)
    return fail(ctx, MLH_ERR_INVALID, "pairs not local: layer spans < 2 blocks per rank");
  if ((with_tree && !dev_tree) || (dr && !dev_r)) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (with_tree && (log_local < 2 || (log_p && log_s + 2 > log_local)))
    return fail(ctx, MLH_ERR_INVALID, "folded layer's pairs are not local");
  ShardMap m;
  m.log_s = log_p ? log_s : 40;
  m.log_p = log_p;
  m.rank = rank;
  const fe *tlo, *thi;
  MLH_TRY(fold_tables(ctx, log_domain, &tlo, &thi));
  const fe* layer = reinterpret_cast<const fe*>(dev_layer);
  fe* next = reinterpret_cast<fe*>(dev_next);
  const fe rv = dr ? fe{} : to_fe(h_load(r));
  const fe* rd = dr ? reinterpret_cast<const fe*>(dev_r) : nullptr;
  if (with_tree)
    HIP_TRY(ctx, launch_fri_fold_commit(layer, 1ull << log_local, next,
                                        reinterpret_cast<uint8_t*>(dev_tree), rv, tlo, thi, k,
                                        1ull << log_domain, ctx->stream, m, rd));
  else
    HIP_TRY(ctx, launch_fri_fold(layer, 1ull << log_local, next, rv, tlo, thi, k,
                                 1ull << log_domain, ctx->stream, m, rd));
  return MLH_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// NTT: the cross-shard DFT; FRI: fold (and commit) of a block-layout layer,
// the owner's opening of its local subtree, the top levels over all ranks
// ---------------------------------------------------------------------------
mlh_status mlh_shard_ntt_cross(mlh_ctx* ctx, const void* dev_in, void* dev_out, uint32_t log_n,
                               uint32_t log_p, uint32_t rank, const uint8_t gen[16], int inverse) {
  if (!ctx || !dev_in || !dev_out || !gen) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_p < 1 || log_p > 4 || log_n < 2 * log_p || log_n > 40)
    return fail(ctx, MLH_ERR_INVALID, "need 1 <= log_p <= 4 and log_n >= 2 log_p");
  if (rank >> log_p) return fail(ctx, MLH_ERR_INVALID, "rank out of range");
  if (dev_in == dev_out) return fail(ctx, MLH_ERR_INVALID, "shard_ntt_cross is out of place");
  const u128 g = h_load(gen);
  if (!check_generator(g, log_n)) return fail(ctx, MLH_ERR_BAD_GENERATOR, "generator order != n");
  const uint64_t P = 1ull << log_p, S = 1ull << (log_n - 2 * log_p);
  const u128 w = inverse ? h_inv(g) : g;
  const fe *tlo, *thi, *wp;
  MLH_TRY(get_table(ctx, w, 4096, 1, &tlo));
  MLH_TRY(get_table(ctx, h_pow(w, 4096), hi_count(log_n - log_p), 1, &thi));
  MLH_TRY(get_table(ctx, h_pow(w, 1ull << (log_n - log_p)), P / 2, 1, &wp));
  const u128 scale = inverse ? h_inv((u128)P) : (u128)1;
  static const char* labs[2][5] = {{"", "shard_dft<1,0>", "shard_dft<2,0>", "shard_dft<3,0>", "shard_dft<4,0>"},
                                   {"", "shard_dft<1,1>", "shard_dft<2,1>", "shard_dft<3,1>", "shard_dft<4,1>"}};
  ProfScope ps(ctx, labs[inverse ? 1 : 0][log_p]);
  HIP_TRY(ctx, launch_shard_dft(reinterpret_cast<const fe*>(dev_in), reinterpret_cast<fe*>(dev_out),
                                S, (uint64_t)rank * S, log_p, inverse != 0, tlo, thi, wp,
                                to_fe(scale), ctx->stream));
  ps.end();
  return MLH_OK;
}

mlh_status mlh_shard_fri_fold(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local, uint32_t k,
                              uint32_t log_domain, const uint8_t r[16], void* dev_next,
                              uint32_t log_s, uint32_t log_p, uint32_t rank) {
  if (!r) return fail(ctx, MLH_ERR_INVALID, "null argument");
  return shard_fold(ctx, dev_layer, log_local, k, log_domain, r, nullptr, dev_next, false, nullptr,
                    log_s, log_p, rank);
}

mlh_status mlh_shard_fri_fold_commit(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local,
                                     uint32_t k, uint32_t log_domain, const uint8_t r[16],
                                     void* dev_next, void* dev_tree, uint32_t log_s,
                                     uint32_t log_p, uint32_t rank) {
  if (!r) return fail(ctx, MLH_ERR_INVALID, "null argument");
  return shard_fold(ctx, dev_layer, log_local, k, log_domain, r, nullptr, dev_next, true, dev_tree,
                    log_s, log_p, rank);
}

mlh_status mlh_shard_fri_fold_dr(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local,
                                 uint32_t k, uint32_t log_domain, const void* dev_r,
                                 void* dev_next, uint32_t log_s, uint32_t log_p, uint32_t rank) {
  return shard_fold(ctx, dev_layer, log_local, k, log_domain, nullptr, dev_r, dev_next, false,
                    nullptr, log_s, log_p, rank);
}

mlh_status mlh_shard_fri_fold_commit_dr(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local,
                                        uint32_t k, uint32_t log_domain, const void* dev_r,
                                        void* dev_next, void* dev_tree, uint32_t log_s,
                                        uint32_t log_p, uint32_t rank) {
  return shard_fold(ctx, dev_layer, log_local, k, log_domain, nullptr, dev_r, dev_next, true,
                    dev_tree, log_s, log_p, rank);
}

mlh_status mlh_merkle_open_pairs(mlh_ctx* ctx, const void* dev_values, uint32_t log_n,
                                 const void* dev_tree, uint32_t levels, const uint64_t* idx,
                                 uint32_t nq, uint8_t* out) {
  if (!ctx || !dev_values || !dev_tree || (nq && (!idx || !out)))
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_n < 1 || log_n > 40 || levels > log_n - 1)
    return fail(ctx, MLH_ERR_INVALID, "levels must be <= log_n - 1");
  const uint64_t half = 1ull << (log_n - 1);
  for (uint32_t q = 0; q < nq; ++q)
    if (idx[q] >= half) return fail(ctx, MLH_ERR_INVALID, "index out of bounds");
  if (nq == 0) return MLH_OK;
  const uint64_t rec = 32ull * (1 + levels);
  PoolBuf didx(ctx), dout(ctx);
  MLH_TRY(didx.alloc(nq * sizeof(uint64_t)));
  MLH_TRY(dout.alloc(nq * rec));
  HIP_TRY(ctx, hipMemcpyAsync(didx.p, idx, nq * sizeof(uint64_t), hipMemcpyHostToDevice,
                              ctx->stream));
  HIP_TRY(ctx, launch_open_pairs(reinterpret_cast<const fe*>(dev_values), half,
                                 reinterpret_cast<const uint8_t*>(dev_tree), levels,
                                 didx.as<uint64_t>(), nq, dout.as<uint8_t>(), ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(out, dout.p, nq * rec, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLH_OK;
}

mlh_status mlh_merkle_top(mlh_ctx* ctx, const void* dev_gathered, uint32_t P, uint64_t per_rank,
                          void* dev_levels) {
  if (!ctx || !dev_gathered || !dev_levels) return fail(ctx, MLH_ERR_INVALID, "null argument");
  const uint64_t n = (uint64_t)P * per_rank;
  if (!n || (n & (n - 1))) return fail(ctx, MLH_ERR_NOT_POW2, "top tree size must be a power of two");
  uint8_t* lv = reinterpret_cast<uint8_t*>(dev_levels);
  HIP_TRY(ctx, launch_top_reorder(reinterpret_cast<const uint8_t*>(dev_gathered), P, per_rank, lv,
                                  ctx->stream));
  HIP_TRY(ctx, launch_merkle_levels(lv, n, ctx->stream));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// The transcript in HBM: the kernel that absorbs a root or a round's sums draws
// the challenge, and the next step reads it there (no host round trip inside
// the fold loop or the round loop)
// ---------------------------------------------------------------------------
uint64_t mlh_device_transcript_bytes(void) { return 128; }

mlh_status mlh_transcript_to_device(mlh_ctx* ctx, const mlh_transcript* tr, void* dev_state) {
  if (!ctx || !tr || !dev_state) return fail(ctx, MLH_ERR_INVALID, "null argument");
  std::vector<uint8_t> b(sizeof(DevSha));
  memcpy(b.data(), &tr->sha, sizeof(DevSha));
  HIP_TRY(ctx, hipMemcpyAsync(dev_state, b.data(), sizeof(DevSha), hipMemcpyHostToDevice,
                              ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLH_OK;
}

mlh_status mlh_transcript_from_device(mlh_ctx* ctx, const void* dev_state, mlh_transcript* tr) {
  if (!ctx || !tr || !dev_state) return fail(ctx, MLH_ERR_INVALID, "null argument");
  HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned, dev_state, sizeof(DevSha), hipMemcpyDeviceToHost,
                              ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(&tr->sha, ctx->pinned, sizeof(DevSha));
  return MLH_OK;
}

mlh_status mlh_device_transcript_absorb(mlh_ctx* ctx, void* dev_state, const void* dev_src,
                                        uint32_t n, void* dev_challenge) {
  if (!ctx || !dev_state || (n && !dev_src)) return fail(ctx, MLH_ERR_INVALID, "null argument");
  HIP_TRY(ctx, launch_transcript_absorb(reinterpret_cast<DevSha*>(dev_state),
                                        reinterpret_cast<const uint8_t*>(dev_src), n,
                                        reinterpret_cast<fe*>(dev_challenge), ctx->stream));
  return MLH_OK;
}

mlh_status mlh_device_fri_last(mlh_ctx* ctx, const void* dev_vals2, void* dev_state,
                               void* dev_flag, void* dev_last) {
  if (!ctx || !dev_vals2 || !dev_state || !dev_flag || !dev_last)
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  HIP_TRY(ctx, launch_fri_last(reinterpret_cast<const fe*>(dev_vals2),
                               reinterpret_cast<DevSha*>(dev_state),
                               reinterpret_cast<uint32_t*>(dev_flag),
                               reinterpret_cast<fe*>(dev_last), ctx->stream));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// Sumcheck steps with the sums and the challenge in HBM
// ---------------------------------------------------------------------------
mlh_status mlh_sumcheck_sums_dev(mlh_ctx* ctx, const void* dev_matrix, const void* dev_delta,
                                 uint32_t log_height, void* dev_sums) {
  if (!ctx || !dev_matrix || !dev_delta || !dev_sums || log_height < 1 || log_height > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_sums(reinterpret_cast<const fe*>(dev_matrix),
                           reinterpret_cast<const fe*>(dev_delta), 1ull << (log_height - 1),
                           ctx->partials, reinterpret_cast<fe*>(dev_sums), ctx->stream));
  return MLH_OK;
}

mlh_status mlh_sumcheck_fold_sums_dr(mlh_ctx* ctx, void* dev_matrix, void* dev_delta,
                                     uint32_t log_height, const void* dev_r, void* dev_sums) {
  if (!ctx || !dev_matrix || !dev_delta || !dev_r || !dev_sums || log_height < 2 ||
      log_height > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_fold_sums(reinterpret_cast<fe*>(dev_matrix), reinterpret_cast<fe*>(dev_delta),
                                1ull << log_height, fe{}, ctx->partials,
                                reinterpret_cast<fe*>(dev_sums), ctx->stream,
                                reinterpret_cast<const fe*>(dev_r)));
  return MLH_OK;
}

mlh_status mlh_sumcheck_fold_dr(mlh_ctx* ctx, void* dev_matrix, void* dev_delta,
                                uint32_t log_height, const void* dev_r) {
  if (!ctx || !dev_matrix || !dev_delta || !dev_r || log_height < 1 || log_height > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_fold(reinterpret_cast<fe*>(dev_matrix), reinterpret_cast<fe*>(dev_delta),
                           1ull << log_height, fe{}, ctx->stream,
                           reinterpret_cast<const fe*>(dev_r)));
  return MLH_OK;
}

mlh_status mlh_device_sumcheck_round(mlh_ctx* ctx, const void* dev_sum_pairs, uint32_t npairs,
                                     void* dev_prev, void* dev_state, void* dev_poly_out,
                                     void* dev_r_out) {
  if (!ctx || !dev_sum_pairs || !dev_prev || !dev_state || !dev_poly_out || !dev_r_out ||
      npairs == 0)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_sumcheck_round(reinterpret_cast<const fe*>(dev_sum_pairs), npairs,
                                     reinterpret_cast<fe*>(dev_prev),
                                     reinterpret_cast<DevSha*>(dev_state),
                                     reinterpret_cast<fe*>(dev_poly_out),
                                     reinterpret_cast<fe*>(dev_r_out), ctx->stream));
  return MLH_OK;
}

}  // extern "C"
