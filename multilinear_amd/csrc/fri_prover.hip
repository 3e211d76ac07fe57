// The FRI prover's host side: FriProverData::{init, fold_step, fold,
// open_query_at} (src/fri/mod.rs:57-175), FriProof::prove (:260-285) and their
// batched forms (batched_fri.rs), stepwise with the host transcript and as
// whole commit phases with the transcript on the device (FriDevLoop).  A layer
// is built in one place (PendingLayer) and folded in one (fold_step_core).
#include "fri_prover.hpp"

#include "tables.hpp"

using namespace mlh;

// A layer being built: its values (unless borrowed: layer 0 is the caller's code),
// then its tree, pool blocks that go back unless commit() hands them to the prover.
struct PendingLayer {
  PoolBuf vb, tb;
  FriLayer l;
  PendingLayer(mlh_ctx* c, uint32_t log_n, const fe* borrowed = nullptr) : vb(c), tb(c) {
    l.log_n = log_n;
    l.values = borrowed;
  }
  mlh_status alloc(bool tree = true) {
    if (!l.values) {
      MLH_TRY(vb.alloc(sizeof(fe) << l.log_n));
      l.values = vb.as<fe>();
    }
    if (tree) {
      MLH_TRY(tb.alloc(mlh_merkle_layers_bytes(1ull << (l.log_n - 1))));
      l.tree = tb.as<uint8_t>();
    }
    return MLH_OK;
  }
  const FriLayer& commit(mlh_fri_prover* p) {
    l.owned_values = vb.release();
    tb.release();
    p->layers.push_back(l);
    return p->layers.back();
  }
};

// gen_pows[1] of a caller's table gen_pows = [g^0 .. g^(2^log_gp - 1)]
// (NttField::pow_2_generator_powers, ntt/mod.rs:18-28, or any generator of
// order exactly 2^log_gp)
static mlh_status load_gen_pows_1(mlh_ctx* ctx, const uint8_t bytes[16], uint32_t log_gp, u128* g) {
  if (log_gp > 40) return fail(ctx, MLH_ERR_INVALID, "gen_pows length");
  *g = h_load(bytes);
  if (!check_generator(*g, log_gp))
    return fail(ctx, MLH_ERR_BAD_GENERATOR, "gen_pows[1] must have order exactly gen_pows.len()");
  return MLH_OK;
}

// The reference indexes gen_pows[len - i 2^k] with i 2^k < 2^(log_code - 1), so
// a table shorter than half the code underflows its index (a panic there).
// gen == nullptr: the prover's default, the code's domain.
static mlh_status set_gen_pows(mlh_ctx* ctx, mlh_fri_prover* p, const uint8_t* gen,
                               uint32_t log_gp) {
  if (!gen) return MLH_OK;
  if (log_gp > 40 || log_gp + 1 < p->log_code)
    return fail(ctx, MLH_ERR_INVALID, "gen_pows shorter than half the code");
  MLH_TRY(load_gen_pows_1(ctx, gen, log_gp, &p->gp_gen));
  p->log_gp = log_gp;
  return MLH_OK;
}

mlh_status batch_layer_commit(mlh_ctx* ctx, const fe* codes, uint32_t m, uint64_t N, uint8_t* tree,
                              RootAbsorb ra) {
  HIP_TRY(ctx, launch_batch_pairs_leaves(codes, m, N, tree, ctx->stream));
  HIP_TRY(ctx, launch_merkle_levels(tree, N / 2, ctx->stream, ra));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// the fold step (fri/mod.rs:79-134, batched_fri.rs:100-176)
// ---------------------------------------------------------------------------
// What a step folds.  Plain: the prover's last layer with fold index k and the
// table (gen, log_gp): twiddle gen_pows[len - i 2^k] = gen^(-(i 2^k) mod len);
// twl (optional) that layer's slice of the layer table.  Batch (codes set):
// the m codes of 2^log_n values, fingerprinted with *fr (device).
struct FoldSrc {
  u128 gen;
  uint32_t log_gp;
  const fe *tlo, *thi;  // fold_tables_g(gen, log_gp), fetched if null
  uint32_t k;
  const fe* twl = nullptr;
  const fe* codes = nullptr;
  uint32_t m = 0, log_n = 0;
  const fe* fr = nullptr;
};
// Where the challenge comes from and the new root (or the last element) goes.
// Host: the challenge r (the batch fold reads rp, its device copy) and the
// transcript tr.  Device (lp set): the challenge at rp; ra absorbs the root,
// then its poly_in, and draws the next one; job: a PCS round in the fold launch.
struct FoldSink {
  fe r;
  mlh_transcript* tr;
  const fe* rp = nullptr;
  FriDevLoop* lp = nullptr;
  RootAbsorb ra;
  const PcsJob* job = nullptr;
};

static mlh_status fold_step_core(mlh_ctx* ctx, mlh_fri_prover* p, const FoldSrc& s,
                                 const FoldSink& t) {
  // a batched prover's inner view has no tree before batched_fold_step, nor
  // after a step that produced the last element directly (log_code 2); the
  // reference panics on merkle_trees.last().unwrap() there
  if (!s.codes && p->layers.empty())
    return fail(ctx, MLH_ERR_INVALID, "fold_step before any tree (batched_fold_step not applied)");
  // (after the last element, the reference folds its last tree again and
  // re-absorbs the element: layers.back() is still that tree here, too)
  const fe* in = s.codes ? s.codes : p->layers.back().values;
  const uint32_t log_n = s.codes ? s.log_n : p->layers.back().log_n;  // n = 2 * pairs
  const uint64_t n = 1ull << log_n, half_n = n / 2, n0 = 1ull << s.log_gp;
  const uint64_t blowup = 1ull << MLH_LOG_BLOWUP;
  if (n <= blowup) return MLH_OK;  // fri/mod.rs:83-85, batched_fri.rs:104-106
  // The reference accepts any k whose indices stay in the table, (n/2 - 1) 2^k <=
  // len; else its usize index underflows (a panic).  (log space first: with
  // (log_n - 1) + k <= 62 the shift cannot wrap; beyond it no table is that long)
  if (!s.codes && (s.k > 40 || (log_n - 1) + s.k > 62 || ((half_n - 1) << s.k) > n0))
    return fail(ctx, MLH_ERR_INVALID, "gen_pows index len - i*2^k underflows (fri/mod.rs:106-110)");
  const bool last = half_n == blowup;  // fri/mod.rs:116-126, batched_fri.rs:152-162
  if (last && (t.job || t.ra.poly_in))
    return fail(ctx, MLH_ERR_INVALID, "no PCS round after the last FRI fold");
  const fe *tlo = s.tlo, *thi = s.thi;
  if (!tlo) MLH_TRY(fold_tables_g(ctx, s.gen, s.log_gp, &tlo, &thi));
  PendingLayer nx(ctx, log_n - 1);
  MLH_TRY(nx.alloc(!last));
  fe* vals = nx.vb.as<fe>();
  uint8_t* tree = nx.l.tree;  // null for the last fold: two values, no leaves
  if (s.codes) {
    HIP_TRY(ctx, launch_batched_fold_leaves(s.codes, s.m, n, s.fr, t.rp, tlo, thi, vals, tree,
                                            ctx->stream));
    if (!last) HIP_TRY(ctx, launch_merkle_levels(tree, half_n / 2, ctx->stream, t.ra));
  } else if (last) {
    HIP_TRY(ctx, launch_fri_fold(in, n, vals, t.r, tlo, thi, s.k, n0, ctx->stream, ShardMap(), t.rp));
  } else {
    HIP_TRY(ctx, launch_fri_fold_commit(in, n, vals, tree, t.r, tlo, thi, s.k, n0, ctx->stream,
                                        ShardMap(), t.rp, t.ra, t.job, s.twl));
  }
  if (last && t.lp) {  // the device checks the pair, absorbs the element; finish() reads both
    uint8_t* sb = t.lp->sb();
    HIP_TRY(ctx, launch_fri_last(vals, t.lp->dt(), reinterpret_cast<uint32_t*>(sb + t.lp->off_flag),
                                 reinterpret_cast<fe*>(sb + t.lp->off_last), ctx->stream));
    t.lp->done = true;
    return MLH_OK;
  }
  if (last) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned, vals, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (memcmp(ctx->pinned, ctx->pinned + 16, 16) != 0)
      return fail(ctx, MLH_ERR_NOT_RS_CODE, "not an RS code");
    memcpy(p->last, ctx->pinned, 16);
    p->has_last = true;
    mlh_transcript_absorb(t.tr, p->last, 16);
    return MLH_OK;
  }
  // (the layer joins the prover last: an error return above leaves no layer and no block)
  if (t.tr) MLH_TRY(read_root(ctx, tree, half_n / 2, nx.l.root));
  const FriLayer& l = nx.commit(p);
  if (t.tr) mlh_transcript_absorb(t.tr, l.root, 32);
  return MLH_OK;
}

extern "C" {

mlh_status mlh_fri_prover_init(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                               mlh_transcript* tr, mlh_fri_prover** out) {
  return mlh_fri_prover_init_gp(ctx, dev_code, log_code, nullptr, 0, tr, out);
}

mlh_status mlh_fri_prover_init_gp(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                                  const uint8_t gen_pows_1[16], uint32_t log_gen_pows,
                                  mlh_transcript* tr, mlh_fri_prover** out) {
  if (!ctx || !dev_code || !tr || !out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_code < 1 || log_code > 40)
    return fail(ctx, MLH_ERR_NOT_POW2, "Input size must be a power of two");
  std::unique_ptr<mlh_fri_prover> p(new mlh_fri_prover(ctx, log_code));
  MLH_TRY(set_gen_pows(ctx, p.get(), gen_pows_1, log_gen_pows));
  PendingLayer l0(ctx, log_code, reinterpret_cast<const fe*>(dev_code));
  MLH_TRY(l0.alloc());
  MLH_TRY(mlh_merkle_commit_pairs(ctx, dev_code, log_code, l0.l.tree, l0.l.root));
  mlh_transcript_absorb(tr, l0.commit(p.get()).root, 32);
  *out = p.release();
  return MLH_OK;
}

mlh_status mlh_fri_prover_fold_step(mlh_ctx* ctx, mlh_fri_prover* p, uint32_t k,
                                    const uint8_t r[16], mlh_transcript* tr) {
  if (!ctx || !p || !r || !tr) return fail(ctx, MLH_ERR_INVALID, "null argument");
  return fold_step_core(ctx, p, FoldSrc{p->gp_gen, p->log_gp, nullptr, nullptr, k},
                        FoldSink{to_fe(h_load(r)), tr});
}

mlh_status mlh_fri_prover_fold_step_gp(mlh_ctx* ctx, mlh_fri_prover* p, const uint8_t gen_pows_1[16],
                                       uint32_t log_gen_pows, uint32_t k, const uint8_t r[16],
                                       mlh_transcript* tr) {
  if (!ctx || !p || !gen_pows_1 || !r || !tr) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_gen_pows < 1) return fail(ctx, MLH_ERR_INVALID, "gen_pows length");
  u128 g;
  MLH_TRY(load_gen_pows_1(ctx, gen_pows_1, log_gen_pows, &g));
  return fold_step_core(ctx, p, FoldSrc{g, log_gen_pows, nullptr, nullptr, k},
                        FoldSink{to_fe(h_load(r)), tr});
}

}  // extern "C"

// ---------------------------------------------------------------------------
// the commit phase with the transcript on the device
// ---------------------------------------------------------------------------
static_assert(sizeof(DevSha) == sizeof(HostSha256), "transcript layouts differ");

mlh_status FriDevLoop::layout(uint32_t log_code, const mlh_transcript* tr, size_t n_extra) {
  const uint32_t steps = log_code - MLH_LOG_BLOWUP;
  off_last = off_r + 16 * (steps + 1);
  off_flag = off_last + 16;
  off_broot = off_flag + 16;
  off_fr = off_broot + 32;
  off_roots = off_fr + 16;
  off_polys = off_roots + 32 * (steps + 1);
  off_prev = off_polys + 32 * steps;
  off_extra = off_prev + 16;
  MLH_TRY(scratch.alloc(off_extra + 16 * (n_extra ? n_extra : 1)));
  if (p->log_gp == log_code) MLH_TRY(fold_layer_table(ctx, p->gp_gen, log_code, &twt));
  MLH_TRY(fold_tables_g(ctx, p->gp_gen, p->log_gp, &tlo, &thi));
  memcpy(ctx->pinned, &tr->sha, sizeof(DevSha));
  HIP_TRY(ctx, hipMemcpyAsync(dt(), ctx->pinned, sizeof(DevSha), hipMemcpyHostToDevice,
                              ctx->stream));
  return MLH_OK;
}

mlh_status FriDevLoop::init_batched(const fe* dev_codes, uint32_t num_codes, uint32_t log_code,
                                    const mlh_transcript* tr, bool challenge_r0, size_t n_extra,
                                    const uint8_t* built_tree) {
  MLH_TRY(layout(log_code, tr, n_extra));
  codes = dev_codes;
  m = num_codes;
  const uint64_t N = 1ull << log_code, L = N / 2;
  if (built_tree) {
    bt = built_tree;
    HIP_TRY(ctx, launch_transcript_absorb(dt(), bt + (2 * L - 2) * 32, 32, fr(), ctx->stream,
                                          sb() + off_broot));
  } else {
    MLH_TRY(btree.alloc(mlh_merkle_layers_bytes(L)));
    bt = btree.as<uint8_t>();
    MLH_TRY(batch_layer_commit(ctx, codes, m, N, btree.as<uint8_t>(),
                               RootAbsorb{dt(), fr(), sb() + off_broot}));
  }
  HIP_TRY(ctx, launch_transcript_absorb(dt(), reinterpret_cast<const uint8_t*>(fr()), 16,
                                        challenge_r0 ? r(0) : nullptr, ctx->stream));
  return MLH_OK;
}

mlh_status FriDevLoop::init(const void* dev_code, uint32_t log_code, bool challenge_after_root0,
                            const fe* poly0) {
  PendingLayer l0(ctx, log_code, reinterpret_cast<const fe*>(dev_code));
  MLH_TRY(l0.alloc());
  HIP_TRY(ctx, launch_commit_pairs(
                   l0.l.values, 1ull << (log_code - 1), l0.l.tree, ctx->stream,
                   RootAbsorb{dt(), challenge_after_root0 ? r(0) : nullptr, root(0), poly0}));
  l0.commit(p);
  return MLH_OK;
}

// fold k of the device loop: the new tree is the prover's next one, its root
// slot root(layers.size()); the challenge after it goes to r(k + 1)
static FoldSink dev_sink(FriDevLoop& lp, uint32_t k, const fe* rp, bool challenge_next,
                         const fe* poly_next, const PcsJob* job) {
  return FoldSink{fe{}, nullptr, rp, &lp,
                  RootAbsorb{lp.dt(), challenge_next ? lp.r(k + 1) : nullptr,
                             lp.root((uint32_t)lp.p->layers.size()), poly_next},
                  job};
}

mlh_status FriDevLoop::step(uint32_t k, const fe* rp, bool challenge_next, const fe* poly_next,
                            const PcsJob* job) {
  if (done) return MLH_OK;
  const uint32_t Lg = p->log_gp;  // the layer table's part for fold k (pairs of a 2^(Lg - k) layer)
  const fe* twl = twt && p->layers.back().log_n + k == Lg
                      ? twt + ((1ull << Lg) - (1ull << (Lg - k))) : nullptr;
  return fold_step_core(ctx, p, FoldSrc{p->gp_gen, Lg, tlo, thi, k, twl},
                        dev_sink(*this, k, rp, challenge_next, poly_next, job));
}

mlh_status FriDevLoop::step_batched(const fe* rp, bool challenge_next, const fe* poly_next) {
  return fold_step_core(
      ctx, p, FoldSrc{p->gp_gen, p->log_gp, tlo, thi, 0, nullptr, codes, m, p->log_code, fr()},
      dev_sink(*this, 0, rp, challenge_next, poly_next, nullptr));
}

mlh_status FriDevLoop::finish(size_t polys_bytes) {
  if (!done) return fail(ctx, MLH_ERR_INVALID, "fold produced no last element");
  const size_t nt = p->layers.size();
  const size_t bytes = off_polys - off_r + polys_bytes;
  if (bytes > kPinStage) return fail(ctx, MLH_ERR_INVALID, "proof staging too large");
  HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned, sb() + off_r, bytes, hipMemcpyDeviceToHost,
                              ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  MLH_TRY(device_check(ctx));
  const uint8_t* h = ctx->pinned;
  for (size_t t = 0; t < nt; ++t)
    memcpy(p->layers[t].root, h + (off_roots - off_r) + 32 * t, 32);
  uint32_t flag;
  memcpy(&flag, h + (off_flag - off_r), 4);
  if (flag) return fail(ctx, MLH_ERR_NOT_RS_CODE, "not an RS code");
  memcpy(p->last, h + (off_last - off_r), 16);
  p->has_last = true;
  return MLH_OK;
}

// FriProverData::fold (fri/mod.rs:136-145) with the transcript on the device:
// every round's challenge is derived on the GPU from the root just written,
// so the whole commit phase is one stream of kernels with a single sync at
// the end; the host transcript then replays the same absorbs (root_0,
// root_1, ..., last element) and ends in the identical state.
static mlh_status fri_fold_device(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                                  const uint8_t* gen, uint32_t log_gp, mlh_transcript* tr,
                                  mlh_fri_prover** out) {
  if (!ctx || !dev_code || !tr || !out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_code < 2 || log_code > 40)
    return fail(ctx, log_code < 2 ? MLH_ERR_INVALID : MLH_ERR_NOT_POW2,
                "fold needs 4 <= code length <= 2^40");
  std::unique_ptr<mlh_fri_prover> p(new mlh_fri_prover(ctx, log_code));
  MLH_TRY(set_gen_pows(ctx, p.get(), gen, log_gp));
  FriDevLoop lp(ctx, p.get());
  device_arm(ctx);
  MLH_TRY(lp.layout(log_code, tr));
  MLH_TRY(lp.init(dev_code, log_code, true));
  const uint32_t steps = log_code - MLH_LOG_BLOWUP;
  for (uint32_t k = 0; k < steps; ++k) MLH_TRY(lp.step(k, lp.r(k), true));
  MLH_TRY(lp.finish(0));
  // host replay: root_t, then the challenge r_t the device drew from it
  ReplayCheck rc(ctx, tr);
  for (size_t t = 0; t < p->layers.size(); ++t) {
    rc.absorb(p->layers[t].root, 32);
    rc.expect(lp.host_r((uint32_t)t));
  }
  rc.absorb(p->last, 16);
  MLH_TRY(rc.status());
  *out = p.release();
  return MLH_OK;
}

extern "C" {

mlh_status mlh_fri_prover_fold(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                               mlh_transcript* tr, mlh_fri_prover** out) {
  return fri_fold_device(ctx, dev_code, log_code, nullptr, 0, tr, out);
}

mlh_status mlh_fri_prover_fold_gp(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                                  const uint8_t gen_pows_1[16], uint32_t log_gen_pows,
                                  mlh_transcript* tr, mlh_fri_prover** out) {
  if (!gen_pows_1) return fail(ctx, MLH_ERR_INVALID, "null argument");
  return fri_fold_device(ctx, dev_code, log_code, gen_pows_1, log_gen_pows, tr, out);
}

uint32_t mlh_fri_prover_num_trees(const mlh_fri_prover* p) {
  return p ? (uint32_t)p->layers.size() : 0;
}

mlh_status mlh_fri_prover_roots(const mlh_fri_prover* p, uint8_t* roots_out) {
  if (!p || !roots_out) return MLH_ERR_INVALID;
  for (size_t i = 0; i < p->layers.size(); ++i) memcpy(roots_out + 32 * i, p->layers[i].root, 32);
  return MLH_OK;
}

mlh_status mlh_fri_prover_last_element(const mlh_fri_prover* p, uint8_t out[16]) {
  if (!p || !out || !p->has_last) return MLH_ERR_INVALID;
  memcpy(out, p->last, 16);
  return MLH_OK;
}

void mlh_fri_prover_destroy(mlh_fri_prover* p) { delete p; }

}  // extern "C"

// ---------------------------------------------------------------------------
// queries
// ---------------------------------------------------------------------------
// Gather opened query records from the device-resident layers/trees.
struct QueryTree {
  const fe* values;
  const uint8_t* tree;
  uint32_t log_n;  // layer values
};
// The layer table travels in the kernel arguments (up to 40 layers, ~1 KB)
// with, for a proof's 128 queries, the indices (1 KB): the query phase is then
// one launch and one D2H copy, no host-to-device copies.
constexpr uint32_t kMaxQueryTrees = 40;
struct QueryTrees {
  QueryTree t[kMaxQueryTrees];
  uint32_t n;
};
static_assert(MLH_NUM_QUERIES == 128, "QueryIdx holds 128 indices");
static_assert(sizeof(QueryTrees) + sizeof(mlh::QueryIdx) + 64 <= 4096, "kernel argument budget");

// d_idx: device indices (openings of more than 128 queries), else idx.v
__global__ void gather_queries_kernel(const QueryTrees trees, const mlh::QueryIdx idx,
                                      const uint64_t* __restrict__ d_idx, uint32_t nq,
                                      uint64_t qbytes, uint64_t base, uint8_t* __restrict__ out) {
  const uint32_t q = blockIdx.x;
  if (q >= nq) return;
  const uint64_t iq = d_idx ? d_idx[q] : idx.v[q];
  // record offsets per tree
  uint64_t off = base;
  for (uint32_t t = 0; t < trees.n; ++t) {
    const QueryTree T = trees.t[t];
    const uint64_t half = 1ull << (T.log_n - 1);  // leaves
    const uint64_t i = iq % half;                   // fri/mod.rs:169-170
    const uint32_t depth = T.log_n - 1;
    uint8_t* rec = out + q * qbytes + off;
    if (threadIdx.x == 0) {
      fe_store(reinterpret_cast<fe*>(rec), fe_load(T.values + i));
      fe_store(reinterpret_cast<fe*>(rec + 16), fe_load(T.values + i + half));
    }
    // siblings: level l node (i >> l) ^ 1, level l starts at sum_{j<l} half>>j
    for (uint32_t l = threadIdx.x; l < depth; l += blockDim.x) {
      const uint64_t lvl_off = 2 * half - (2 * half >> l);
      const uint64_t sib = ((i >> l) ^ 1ull);
      const uint4* src = reinterpret_cast<const uint4*>(T.tree + (lvl_off + sib) * 32);
      uint4* dst = reinterpret_cast<uint4*>(rec + 32 + (uint64_t)l * 32);
      dst[0] = src[0];
      dst[1] = src[1];
    }
    off += 32ull * (1 + depth);
  }
}

// Pinned host staging for a query phase: the gather kernels write the
// records straight into it (zero-copy over PCIe, ~1.3 MB for a 2^25 code: no
// device buffer, no copy launch), and it holds indices beyond 128.  Grow-only;
// a caller's stream sync ends every use before the next one.  Allocated
// non-coherent (explicitly; what flags 0 gives under the default
// HIP_HOST_COHERENT=0): the kernels' writes become visible to the host only
// at the end of the kernel, so EVERY host read of records a kernel wrote here
// must follow a sync of the stream that ran it (each caller syncs ctx->stream
// before copying records out).
static mlh_status query_stage(mlh_ctx* ctx, size_t bytes, uint8_t** out) {
  if (bytes > ctx->qstage_bytes) {
    if (ctx->qstage) HIP_TRY(ctx, hipHostFree(ctx->qstage));
    ctx->qstage = nullptr;
    ctx->qstage_bytes = 0;
    void* h = nullptr;
    HIP_TRY(ctx, hipHostMalloc(&h, bytes, hipHostMallocNonCoherent));
    ctx->qstage = reinterpret_cast<uint8_t*>(h);
    ctx->qstage_bytes = bytes;
  }
  *out = ctx->qstage;
  return MLH_OK;
}

// Launch the per-tree gathers of p's layers into records at d_out (qbytes
// each, this part starting at byte `base` of a record; device or pinned host
// memory); indices in idx.v, or at d_idx (device) when nq > 128.
static mlh_status gather_queries_dev(mlh_ctx* ctx, const mlh_fri_prover* p, const mlh::QueryIdx& idx,
                                     const uint64_t* d_idx, uint32_t nq, uint64_t qbytes,
                                     uint64_t base, uint8_t* d_out) {
  const uint32_t nt = (uint32_t)p->layers.size();
  if (nt == 0 || nq == 0) return MLH_OK;
  if (nt > kMaxQueryTrees) return fail(ctx, MLH_ERR_INVALID, "more than 40 FRI layers");
  if (nq > MLH_NUM_QUERIES && !d_idx) return fail(ctx, MLH_ERR_INVALID, "query indices not on the device");
  QueryTrees qt;
  qt.n = nt;
  for (uint32_t t = 0; t < nt; ++t)
    qt.t[t] = QueryTree{p->layers[t].values, p->layers[t].tree, p->layers[t].log_n};
  hipLaunchKernelGGL(gather_queries_kernel, dim3(nq), dim3(64), 0, ctx->stream, qt, idx,
                     nq > MLH_NUM_QUERIES ? d_idx : nullptr, nq, qbytes, base, d_out);
  HIP_TRY(ctx, hipGetLastError());
  return MLH_OK;
}

static mlh_status gather_queries(mlh_ctx* ctx, const mlh_fri_prover* p, const uint64_t* idx,
                                 uint32_t nq, uint8_t* host_out) {
  const uint64_t qbytes = mlh_fri_query_bytes(p->log_code);
  const size_t off_out = nq > MLH_NUM_QUERIES ? 8ull * nq : 0;
  uint8_t* h;
  MLH_TRY(query_stage(ctx, off_out + nq * qbytes, &h));
  mlh::QueryIdx qi;
  memset(&qi, 0, sizeof(qi));
  PoolBuf didx(ctx);
  if (nq > MLH_NUM_QUERIES) {
    memcpy(h, idx, 8ull * nq);
    MLH_TRY(didx.alloc(nq * sizeof(uint64_t)));
    HIP_TRY(ctx, hipMemcpyAsync(didx.p, h, nq * sizeof(uint64_t), hipMemcpyHostToDevice,
                                ctx->stream));
  } else {
    memcpy(qi.v, idx, 8ull * nq);
  }
  MLH_TRY(gather_queries_dev(ctx, p, qi, didx.as<uint64_t>(), nq, qbytes, 0, h + off_out));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(host_out, h + off_out, nq * qbytes);
  return MLH_OK;
}

// The tail both proofs share (fri/mod.rs:266-284): the indices drawn from the
// transcript (modulo half of p's code), p's roots and last element, last_random.
static void proof_tail(const mlh_fri_prover* p, mlh_transcript* tr, mlh::QueryIdx* qi,
                       uint64_t* indices_out, uint8_t* commitments, uint8_t last_elem[16],
                       uint8_t last_random[32]) {
  transcript_draw_indices(tr, 1ull << (p->log_code - 1), MLH_NUM_QUERIES, qi->v);
  if (indices_out) memcpy(indices_out, qi->v, sizeof qi->v);
  if (commitments) mlh_fri_prover_roots(p, commitments);
  memcpy(last_elem, p->last, 16);
  mlh_transcript_random(tr, last_random);
}

mlh_status fri_queries(mlh_ctx* ctx, mlh_fri_prover* p, mlh_transcript* tr, mlh_fri_proof* proof) {
  proof->log_code = p->log_code;
  proof->num_trees = (uint32_t)p->layers.size();
  proof->num_queries = MLH_NUM_QUERIES;
  mlh::QueryIdx qi;
  proof_tail(p, tr, &qi, proof->query_indices, proof->commitments, proof->last_elem,
             proof->last_random);
  if (proof->queries) MLH_TRY(gather_queries(ctx, p, qi.v, MLH_NUM_QUERIES, proof->queries));
  return MLH_OK;
}

// (the batch column + batch siblings and the inner paths share one staging buffer)
mlh_status batched_queries(mlh_ctx* ctx, FriDevLoop& lp, mlh_transcript* tr,
                           mlh_batched_fri_proof* pf) {
  const uint32_t L = lp.p->log_code, m = lp.m;
  pf->log_code = L;
  pf->num_codes = m;
  pf->num_trees = (uint32_t)lp.p->layers.size();
  pf->num_queries = MLH_NUM_QUERIES;
  mlh::QueryIdx qi;
  proof_tail(lp.p, tr, &qi, pf->query_indices, pf->commitments, pf->last_elem, pf->last_random);
  if (!pf->queries) return MLH_OK;
  const uint64_t qbytes = mlh_batched_fri_query_bytes(L, m);
  uint8_t* h;
  MLH_TRY(query_stage(ctx, MLH_NUM_QUERIES * qbytes, &h));
  HIP_TRY(ctx, launch_batch_queries(lp.codes, m, 1ull << L, lp.bt, qi, MLH_NUM_QUERIES, qbytes, h,
                                    ctx->stream));
  MLH_TRY(gather_queries_dev(ctx, lp.p, qi, nullptr, MLH_NUM_QUERIES, qbytes,
                             32ull * m + 32ull * (L - 1), h));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(pf->queries, h, MLH_NUM_QUERIES * qbytes);
  return MLH_OK;
}

static mlh_status fri_prove(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                            const uint8_t* gen, uint32_t log_gp, mlh_transcript* tr,
                            mlh_fri_proof* proof) {
  if (!ctx || !dev_code || !tr || !proof) return fail(ctx, MLH_ERR_INVALID, "null argument");
  mlh_fri_prover* p = nullptr;
  MLH_TRY(fri_fold_device(ctx, dev_code, log_code, gen, log_gp, tr, &p));
  mlh_status s = fri_queries(ctx, p, tr, proof);
  delete p;
  return s;
}

extern "C" {

mlh_status mlh_fri_prover_open_query(mlh_ctx* ctx, const mlh_fri_prover* p, uint64_t index,
                                     uint8_t* out) {
  return mlh_fri_prover_open_queries(ctx, p, &index, 1, out);
}

mlh_status mlh_fri_prover_open_queries(mlh_ctx* ctx, const mlh_fri_prover* p,
                                       const uint64_t* idx, uint32_t nq, uint8_t* out) {
  if (!ctx || !p || !idx || !out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  for (uint32_t q = 0; q < nq; ++q)
    if (idx[q] >= (1ull << (p->log_code - 1))) return fail(ctx, MLH_ERR_INVALID, "index out of bounds");
  if (nq == 0) return MLH_OK;
  return gather_queries(ctx, p, idx, nq, out);
}

mlh_status mlh_fri_prove(mlh_ctx* ctx, const void* dev_code, uint32_t log_code, mlh_transcript* tr,
                         mlh_fri_proof* proof) {
  return fri_prove(ctx, dev_code, log_code, nullptr, 0, tr, proof);
}

mlh_status mlh_fri_prove_gp(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                            const uint8_t gen_pows_1[16], uint32_t log_gen_pows, mlh_transcript* tr,
                            mlh_fri_proof* proof) {
  if (!gen_pows_1) return fail(ctx, MLH_ERR_INVALID, "null argument");
  return fri_prove(ctx, dev_code, log_code, gen_pows_1, log_gen_pows, tr, proof);
}

// BatchedFriProof::prove (batched_fri.rs:280-311)
mlh_status mlh_batched_fri_prove(mlh_ctx* ctx, const void* dev_codes, uint32_t num_codes,
                                 uint32_t log_code, mlh_transcript* tr,
                                 mlh_batched_fri_proof* proof) {
  if (!ctx || !dev_codes || !tr || !proof) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (num_codes == 0) return fail(ctx, MLH_ERR_INVALID, "Codes must not be empty");
  if (log_code < 2 || log_code > 40)
    return fail(ctx, MLH_ERR_NOT_POW2, "Code size must be a power of two (>= 4)");
  mlh_fri_prover p(ctx, log_code);
  FriDevLoop lp(ctx, &p);
  device_arm(ctx);
  MLH_TRY(lp.init_batched(reinterpret_cast<const fe*>(dev_codes), num_codes, log_code, tr, true));
  // fold (batched_fri.rs:178-205): the batched step, then ordinary steps
  MLH_TRY(lp.step_batched(lp.r(0), true));
  const uint32_t steps = log_code - MLH_LOG_BLOWUP;
  for (uint32_t k = 1; k < steps; ++k) MLH_TRY(lp.step(k, lp.r(k), true));
  MLH_TRY(lp.finish(0));
  // host transcript replay: batch root, fingerprint_r, inner roots, last
  ReplayCheck rc(ctx, tr);
  rc.absorb(lp.host_broot(), 32);
  rc.expect(lp.host_fr());
  rc.absorb(lp.host_fr(), 16);
  rc.expect(lp.host_r(0));
  for (size_t t = 0; t < p.layers.size(); ++t) {
    rc.absorb(p.layers[t].root, 32);
    rc.expect(lp.host_r((uint32_t)t + 1));
  }
  rc.absorb(p.last, 16);
  MLH_TRY(rc.status());
  memcpy(proof->batch_commitment, lp.host_broot(), 32);
  return batched_queries(ctx, lp, tr, proof);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// BatchedFriProverData step by step (batched_fri.rs:9-224), host transcript:
// init -> batched_fold_step(gen_pows, r, tr) -> the inner fri_data's
// fold_step(gen_pows, k, r, tr) for k >= 1 (mlh_fri_prover_fold_step(_gp) on
// the handle mlh_batched_fri_prover_inner returns) -> open_query_at.  The
// whole-proof path (mlh_batched_fri_prove) keeps the transcript on the device.
// ---------------------------------------------------------------------------
struct mlh_batched_fri_prover {
  mlh_ctx* ctx;
  const fe* codes = nullptr;  // caller's [m][N], must outlive the prover
  uint32_t m = 0, log_code = 0;
  PoolBuf btree;              // batch layer: N/2 leaves + levels
  PoolBuf scal;               // device [fingerprint_r | r]
  uint8_t broot[32];
  uint8_t fr[16];
  mlh_fri_prover inner;       // fri_data: merkle_trees start at the folded layer
  mlh_batched_fri_prover(mlh_ctx* c, uint32_t lc)
      : ctx(c), log_code(lc), btree(c), scal(c), inner(c, lc - 1) {}  // (inner: the folded layer's size)
};

extern "C" {

mlh_status mlh_batched_fri_prover_init(mlh_ctx* ctx, const void* dev_codes, uint32_t num_codes,
                                       uint32_t log_code, mlh_transcript* tr, mlh_batched_fri_prover** out) {
  if (!ctx || !dev_codes || !tr || !out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (num_codes == 0) return fail(ctx, MLH_ERR_INVALID, "Codes must not be empty");
  if (log_code < 2 || log_code > 40)
    return fail(ctx, MLH_ERR_NOT_POW2, "Code size must be a power of two (>= 4)");
  std::unique_ptr<mlh_batched_fri_prover> bp(new mlh_batched_fri_prover(ctx, log_code));
  bp->codes = reinterpret_cast<const fe*>(dev_codes);
  bp->m = num_codes;
  bp->inner.gp_gen = h_pow2_generator(log_code);  // the batched code's domain
  bp->inner.log_gp = log_code;
  const uint64_t N = 1ull << log_code;
  MLH_TRY(bp->btree.alloc(mlh_merkle_layers_bytes(N / 2)));
  MLH_TRY(bp->scal.alloc(32));
  uint8_t* bt = bp->btree.as<uint8_t>();
  MLH_TRY(batch_layer_commit(ctx, bp->codes, num_codes, N, bt));
  MLH_TRY(read_root(ctx, bt, N / 2, bp->broot));
  // batched_fri.rs:82-89: absorb the root, fingerprint_r = next_challenge(),
  // absorb LE16(fingerprint_r)
  mlh_transcript_absorb(tr, bp->broot, 32);
  mlh_transcript_next_challenge(tr, bp->fr);
  mlh_transcript_absorb(tr, bp->fr, 16);
  *out = bp.release();
  return MLH_OK;
}

mlh_status mlh_batched_fri_prover_fold_step_gp(mlh_ctx* ctx, mlh_batched_fri_prover* bp,
                                               const uint8_t gen_pows_1[16], uint32_t log_gen_pows,
                                               const uint8_t r[16], mlh_transcript* tr) {
  if (!ctx || !bp || !gen_pows_1 || !r || !tr) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_gen_pows < 1) return fail(ctx, MLH_ERR_INVALID, "gen_pows length");
  u128 g;
  MLH_TRY(load_gen_pows_1(ctx, gen_pows_1, log_gen_pows, &g));
  if ((1ull << (bp->log_code - 1)) - 1 > (1ull << log_gen_pows))
    return fail(ctx, MLH_ERR_INVALID, "gen_pows index len - i underflows (batched_fri.rs:131-136)");
  // (called again, the reference folds the batch layer again and pushes a
  // second tree onto fri_data; this binding folds it once)
  if (!bp->inner.layers.empty() || bp->inner.has_last)
    return fail(ctx, MLH_ERR_INVALID, "batched_fold_step already applied");
  memcpy(ctx->pinned, bp->fr, 16);
  memcpy(ctx->pinned + 16, r, 16);
  fe* sc = bp->scal.as<fe>();
  HIP_TRY(ctx, hipMemcpyAsync(sc, ctx->pinned, 32, hipMemcpyHostToDevice, ctx->stream));
  return fold_step_core(
      ctx, &bp->inner,
      FoldSrc{g, log_gen_pows, nullptr, nullptr, 0, nullptr, bp->codes, bp->m, bp->log_code, sc},
      FoldSink{fe{}, tr, sc + 1});
}

mlh_fri_prover* mlh_batched_fri_prover_inner(mlh_batched_fri_prover* bp) {
  return bp ? &bp->inner : nullptr;
}

mlh_status mlh_batched_fri_prover_batch_root(const mlh_batched_fri_prover* bp, uint8_t out[32]) {
  if (!bp || !out) return MLH_ERR_INVALID;
  memcpy(out, bp->broot, 32);
  return MLH_OK;
}

mlh_status mlh_batched_fri_prover_fingerprint_r(const mlh_batched_fri_prover* bp, uint8_t out[16]) {
  if (!bp || !out) return MLH_ERR_INVALID;
  memcpy(out, bp->fr, 16);
  return MLH_OK;
}

mlh_status mlh_batched_fri_prover_open_query(mlh_ctx* ctx, const mlh_batched_fri_prover* bp,
                                             uint64_t index, uint8_t* out) {
  if (!ctx || !bp || !out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  const uint32_t L = bp->log_code;
  if (index >= (1ull << (L - 1))) return fail(ctx, MLH_ERR_INVALID, "index out of bounds");
  const uint64_t qbytes = mlh_batched_fri_query_bytes(L, bp->m);
  uint8_t* h;
  MLH_TRY(query_stage(ctx, qbytes, &h));
  mlh::QueryIdx qi;
  memset(&qi, 0, sizeof(qi));
  qi.v[0] = index;
  HIP_TRY(ctx, launch_batch_queries(bp->codes, bp->m, 1ull << L, bp->btree.as<uint8_t>(), qi, 1,
                                    qbytes, h, ctx->stream));
  // the inner paths at index mod N/4 (batched_fri.rs:215-221; the gather
  // reduces the index per tree); zero where the inner prover has fewer trees
  const uint64_t base = 32ull * bp->m + 32ull * (L - 1);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memset(h + base, 0, qbytes - base);
  MLH_TRY(gather_queries_dev(ctx, &bp->inner, qi, nullptr, 1, qbytes, base, h));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(out, h, qbytes);
  return MLH_OK;
}

void mlh_batched_fri_prover_destroy(mlh_batched_fri_prover* bp) {
  if (bp) {
    (void)hipStreamSynchronize(bp->ctx->stream);
    delete bp;
  }
}

}  // extern "C"
