// C ABI (include/mlhip.h) and the C++ host layer above the gfx950 kernels:
// host orchestration only, no kernel lives here.
// Here: the context, the pool and the twiddle-table cache, the NTT /
// Reed-Solomon / Merkle / field entries, the stepwise sumcheck entries, the
// trace commitment, the constraint-system sumcheck and the system proofs.
// Elsewhere: what prepares or checks a trace before its commitment (fill, sum,
// scan, sort, lookup counts, shifted extension, public columns, witness check),
// trace_host.hip; the FRI prover, fri_prover.hip; the sumcheck, PCS and batched-
// PCS provers above it, pcs_prover.hip; the multi-GPU schedules, sharded.hip, and
// their rank-local steps, shard_steps.hip; verifiers and host transcript, verify.cpp.
// Every large vector is device resident; only roots, round sums (32 B each),
// the last element and the opened query paths cross PCIe.  The whole-proof
// entries run the Fiat-Shamir transcript on the device (FriDevLoop): the kernel
// that writes a root or a round's sums draws the challenge, one sync ends the
// commit phase, and the host transcript replays the absorbs and checks every
// challenge (ReplayCheck).  Only the stepwise entries, whose challenges come
// from the caller, run it on the host, one round trip per step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/mlhip.h"
#include "field.hpp"
#include "dist.hpp"
#include "fieldops.hpp"
#include "host_field.hpp"
#include "host_sha256.hpp"
#include "host_transcript.hpp"
#include "context.hpp"
#include "cs_call.hpp"
#include "cs_program.hpp"
#include "cs_sumcheck.hpp"
#include "fri_prover.hpp"
#include "fused_ntt.hpp"
#include "merkle.hpp"
#include "ntt.hpp"
#include "pcs_prover.hpp"
#include "sha256.hpp"
#include "sumcheck.hpp"
#include "system_head.hpp"
#include "tables.hpp"
#include "trace_commit.hpp"
#include "trace_shift.hpp"
#include "transcript_dev.hpp"

using namespace mlh;


// Table cache bound: when a new table would take the cache past its limit,
// least-recently-used tables are freed (after the stream drains, since queued
// kernels may still read them).  The tables one operation fetches are stamped
// consecutively and fewer than kTablePin.  An NTT of kMaxPasses = 6 passes: 6
// stage tables, 5 + 5 inter-pass tables (TA, TB) and pass 0's progression and
// step tables, 18 at the most (13 for the default plan of 2^40).  A PCS prove:
// those, the fold-layer table and the 2 fold tables, 21.  So the newest
// kTablePin stamps -- every table the running operation holds a pointer to --
// are never evicted.
constexpr uint64_t kTablePin = 24;

static mlh_status table_make_room(mlh_ctx* ctx, size_t need) {
  if (ctx->table_bytes + need <= ctx->table_limit) return MLH_OK;
  std::vector<std::pair<uint64_t, TableKey>> order;
  for (auto& kv : ctx->tables)
    if (kv.second.stamp + kTablePin <= ctx->table_stamp) order.push_back({kv.second.stamp, kv.first});
  std::sort(order.begin(), order.end(),
            [](const std::pair<uint64_t, TableKey>& a, const std::pair<uint64_t, TableKey>& b) {
              return a.first < b.first;
            });
  bool synced = false;
  for (auto& o : order) {
    if (ctx->table_bytes + need <= ctx->table_limit) break;
    if (!synced) {
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      synced = true;
    }
    auto it = ctx->tables.find(o.second);
    HIP_TRY(ctx, hipFree(it->second.d));
    ctx->table_bytes -= it->second.bytes;
    ctx->tables.erase(it);
  }
  return MLH_OK;
}

static bool table_hit(mlh_ctx* ctx, const TableKey& k, const fe** out) {
  auto it = ctx->tables.find(k);
  if (it == ctx->tables.end()) return false;
  it->second.stamp = ++ctx->table_stamp;
  *out = it->second.d;
  return true;
}

static mlh_status table_alloc(mlh_ctx* ctx, const TableKey& k, size_t bytes, fe** d) {
  MLH_TRY(table_make_room(ctx, bytes));
  HIP_TRY(ctx, hipMalloc(d, bytes));
  ctx->tables[k] = CachedTable{*d, bytes, ++ctx->table_stamp};
  ctx->table_bytes += bytes;
  return poison_fill(ctx, *d, bytes);  // before the build kernel the caller enqueues
}

// table[t] = base^t * scale, t < count, cached per context.  expand: 4 fe per
// entry (t * 2^(32k), k < 4) for fe_mul_pre.
mlh_status mlh::get_table(mlh_ctx* ctx, u128 base, uint64_t count, u128 scale, const fe** out,
                          bool expand) {
  TableKey k{base, count, scale, expand ? 1 : 0};
  if (table_hit(ctx, k, out)) return MLH_OK;
  fe* d = nullptr;
  MLH_TRY(table_alloc(ctx, k, count * sizeof(fe) * (expand ? 4 : 1), &d));
  HIP_TRY(ctx, launch_pow_table(d, to_fe(base), to_fe(scale), count, ctx->stream, expand));
  *out = d;
  return MLH_OK;
}

// 2D table[k * cols + j] = base^(k j mult) * scale, k < rows, cached per context
static mlh_status get_table2d(mlh_ctx* ctx, u128 base, uint64_t rows, uint64_t cols,
                              uint64_t mult, u128 scale, const fe** out, bool expand = false) {
  TableKey k{base, rows, scale, expand ? 1 : 0, cols, mult};
  if (table_hit(ctx, k, out)) return MLH_OK;
  fe* d = nullptr;
  MLH_TRY(table_alloc(ctx, k, rows * cols * sizeof(fe) * (expand ? 4 : 1), &d));
  HIP_TRY(ctx, launch_pow_table2d(d, to_fe(base), to_fe(scale), rows, cols, mult, ctx->stream,
                                  expand));
  *out = d;
  return MLH_OK;
}

uint64_t mlh::hi_count(uint32_t log_n) {
  const uint64_t N = 1ull << log_n;
  return N <= 4096 ? 1 : N / 4096;
}

#ifndef MLH_P0_GEO
#define MLH_P0_GEO 1  // 0: pass 0 always multiplies TA * TB
#endif
#ifndef MLH_P0_GEO_MAXLOGW
#define MLH_P0_GEO_MAXLOGW 16  // largest W (columns) of the progression table: 64 W entries
#endif
static mlh_status get_ntt_tables(mlh_ctx* ctx, u128 gen, uint32_t log_n, bool inverse,
                                 NttTables* tb, const uint32_t* plan = nullptr, uint32_t nplan = 0) {
  const uint64_t N = 1ull << log_n;
  const u128 w = inverse ? h_inv(gen) : gen;
  const u128 scale = inverse ? h_inv((u128)N) : (u128)1;
  tb->log_n = log_n;
  tb->inverse = inverse;
  tb->scale = to_fe(scale);
  if (log_n <= 10) {
    MLH_TRY(get_table(ctx, w, N / 2 ? N / 2 : 1, 1, &tb->tw_small));
    return MLH_OK;
  }
  tb->debug_sync = ctx->debug_sync;
  tb->wide_offsets = ctx->ntt_wide_offsets;
  if (plan)
    ntt_plan_radices(log_n, &tb->nradix, tb->logr, plan, nplan);
  else
    ntt_plan_radices(log_n, &tb->nradix, tb->logr, ctx->forced_plan, ctx->forced_plan_len);
  for (uint32_t p = 0; p < tb->nradix; ++p) {
    const uint64_t R = 1ull << tb->logr[p];
    MLH_TRY(get_table(ctx, h_pow(w, N / R), R / 2, 1, &tb->tw[p], true));
  }
  uint64_t S = 1;
  for (uint32_t p = 0; p + 1 < tb->nradix; ++p) {  // the last pass has no twiddle
    const uint64_t R = 1ull << tb->logr[p];
    const uint32_t logw = log_n - (uint32_t)__builtin_ctzll(S) - tb->logr[p];
    const uint32_t loga =
        tb->logr[p] + logw <= kFullTwLog ? logw : (logw < kTwLogA ? logw : kTwLogA);
    const u128 ws = h_pow(w, S);
    tb->loga[p] = loga;
    MLH_TRY(get_table2d(ctx, ws, R, 1ull << loga, 1, p == 0 ? scale : (u128)1, &tb->ta[p]));
    tb->tb[p] = nullptr;
    if (logw > loga)  // expanded: the kernel multiplies by it with the expanded product
      MLH_TRY(get_table2d(ctx, ws, R, 1ull << (logw - loga), 1ull << loga, 1, &tb->tb[p], true));
    // pass 0 with two tables, R = 2^7 / 2^8, W <= 2^16: the progression form
    // (64 W + 4 W entries: 68 MiB at 2^24)
    if (MLH_P0_GEO && p == 0 && logw > loga && (tb->logr[0] == 7 || tb->logr[0] == 8) &&
        logw <= MLH_P0_GEO_MAXLOGW) {
      MLH_TRY(get_table2d(ctx, ws, 64, 1ull << logw, 1, scale, &tb->gp[0]));
      MLH_TRY(get_table(ctx, h_pow(ws, 64), 1ull << logw, 1, &tb->gc[0], true));
    }
    S <<= tb->logr[p];
  }
  return MLH_OK;
}

// gen must have order exactly 2^log_n
bool mlh::check_generator(u128 gen, uint32_t log_n) {
  if (gen >= kModulus) return false;
  if (log_n == 0) return gen == 1;
  const u128 half = h_pow(gen, (u128)1 << (log_n - 1));
  return half == kModulus - 1;  // gen^(N/2) = -1  <=>  order exactly N
}

// the root of a tree of `leaves` leaves: one synchronising D2H copy (out may be null)
mlh_status mlh::read_root(mlh_ctx* ctx, const uint8_t* layers, uint64_t leaves, uint8_t out[32]) {
  if (!out) return MLH_OK;
  return read_back(ctx, layers + (2 * leaves - 2) * 32, 32, out);
}

// Fold twiddles gen_pows[len - e] = g^(-e), e < len = 2^log_len (fri/mod.rs:106-110),
// as T_lo[e mod 4096] * T_hi[e / 4096] of g^-1.
mlh_status mlh::fold_tables_g(mlh_ctx* ctx, u128 g, uint32_t log_len, const fe** tlo,
                              const fe** thi) {
  const u128 ginv = h_inv(g);
  MLH_TRY(get_table(ctx, ginv, 4096, 1, tlo));
  MLH_TRY(get_table(ctx, h_pow(ginv, 4096), hi_count(log_len), 1, thi));
  return MLH_OK;
}
mlh_status mlh::fold_tables(mlh_ctx* ctx, uint32_t log_domain, const fe** tlo, const fe** thi) {
  return fold_tables_g(ctx, h_pow2_generator(log_domain), log_domain, tlo, thi);
}

// Every fold layer's twiddles of the domain of g (order 2^L) in one cached
// table (fri.hip fold_layer_table): a pair's twiddle is one 16-B load instead
// of a product of two table entries.  Domains up to 2^25 (512 MiB, the size of
// the reference's own gen_pows table there); *out = nullptr above that.
#ifndef MLH_FOLD_TABLE_MAX_LOG
#define MLH_FOLD_TABLE_MAX_LOG 25
#endif
mlh_status mlh::fold_layer_table(mlh_ctx* ctx, u128 g, uint32_t L, const fe** out) {
  *out = nullptr;
  if (L < 2 || L > MLH_FOLD_TABLE_MAX_LOG) return MLH_OK;
  const TableKey key{h_inv(g), (1ull << L) - 1, 0, 2};
  if (table_hit(ctx, key, out)) return MLH_OK;
  fe* d = nullptr;
  MLH_TRY(table_alloc(ctx, key, ((1ull << L) - 1) * sizeof(fe), &d));
  const fe *tlo, *thi;  // (after the big allocation: it cannot evict these)
  MLH_TRY(fold_tables_g(ctx, g, L, &tlo, &thi));
  HIP_TRY(ctx, launch_fold_layer_table(d, tlo, thi, L, ctx->stream));
  *out = d;
  return MLH_OK;
}

static mlh_status ensure_ntt_scratch(mlh_ctx* ctx, uint32_t log_n) {
  const size_t need = (size_t)16 << log_n;
  if (ctx->ntt_scratch_bytes < need) {
    if (ctx->ntt_scratch) {
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      HIP_TRY(ctx, hipFree(ctx->ntt_scratch));
      ctx->ntt_scratch = nullptr;
      ctx->ntt_scratch_bytes = 0;
    }
    HIP_TRY(ctx, hipMalloc(&ctx->ntt_scratch, need));
    ctx->ntt_scratch_bytes = need;
    MLH_TRY(poison_fill(ctx, ctx->ntt_scratch, need));
  }
  return MLH_OK;
}

// Generator of any other order (gen < M; 0 included): the reference's radix-2
// network stage by stage (ntt.hip "general-generator network"), w = gen or,
// for the inverse, gen^-1 (winter-math inverts 0 to 0, as h_inv does).
static mlh_status ntt_network_core(mlh_ctx* ctx, const fe* in, fe* out, uint32_t log_n, u128 gen,
                                   bool inverse, int zero_top) {
  const u128 w = inverse ? h_inv(gen) : gen;
  const fe *tlo, *thi;  // w^t = tlo[t mod 4096] thi[t >> 12], t < N/2
  MLH_TRY(get_table(ctx, w, 4096, 1, &tlo));
  MLH_TRY(get_table(ctx, h_pow(w, 4096), hi_count(log_n - 1), 1, &thi));
  fe* scratch = nullptr;
  if (in == out && log_n > 11) {
    MLH_TRY(ensure_ntt_scratch(ctx, log_n));
    scratch = ctx->ntt_scratch;
  }
  const u128 scale = inverse ? h_inv((u128)1 << log_n) : (u128)1;
  HIP_TRY(ctx, launch_ntt_network(in, out, scratch, tlo, thi, log_n, zero_top, to_fe(scale), inverse,
                                  ctx->stream));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// Sharded NTT with the rank digit fused into the last pass (fused_ntt.hpp):
// the global 2^L transform runs the plan (local digits..., c + p) where the
// local 2^(L-p) array of rank g (cyclic: global index P m + g) takes the
// passes before the last one exactly as a local NTT with plan (local digits...,
// c) would, except that each inter-pass table row k carries the extra factor
// (w_N^S)^(k g) (the global column index is P j + g); the last pass transforms
// the low (c + p) bits of the global index -- c local bits and the p rank bits
// -- on the all-to-all's receive buffer.  Three HBM passes instead of the
// local NTT's three plus the cross-shard DFT's one.
FusedNtt::~FusedNtt() {
  for (void* q : scaled) pool_free(ctx, q);
}

mlh_status FusedNtt::prepare(mlh_ctx* c, u128 gen, uint32_t log_n, uint32_t log_p, uint32_t rank_) {
  ctx = c;
  L = log_n;
  p = log_p;
  rank = rank_;
  const uint32_t Lloc = L - p;
  const uint32_t cl = 9 - p;  // local bits of the last digit: the fused radix is 2^9
  if (p < 1 || p > 4 || cl < 4 || Lloc < cl + 4 || Lloc > 40) return fail(ctx, MLH_ERR_INVALID, "fused plan");
  uint32_t npre = 0, pre[kMaxPasses];
  ntt_plan_radices(Lloc - cl, &npre, pre);
  if (npre + 1 > (uint32_t)kMaxPasses || pre[0] < p + 3) return fail(ctx, MLH_ERR_INVALID, "fused plan");
  uint32_t plan[kMaxPasses];
  for (uint32_t i = 0; i < npre; ++i) plan[i] = pre[i];
  plan[npre] = cl;
  // the local plan as a forced plan needs digits 4..9 (ntt_plan_radices)
  for (uint32_t i = 0; i <= npre; ++i)
    if (plan[i] < 4 || plan[i] > 9) return fail(ctx, MLH_ERR_INVALID, "fused plan");
  const u128 gl = h_pow(gen, (u128)1 << p);  // the local generator w_N^P
  MLH_TRY(get_ntt_tables(ctx, gl, Lloc, false, &loc, plan, npre + 1));
  if (loc.nradix != npre + 1) return fail(ctx, MLH_ERR_INVALID, "fused plan");
  nglob = npre + 1;
  for (uint32_t i = 0; i < npre; ++i) logr[i] = plan[i];
  logr[npre] = cl + p;
  // rank twist of the pre-exchange passes' TA rows: (w_N^S)^(k rank)
  uint64_t S = 1;
  for (uint32_t i = 0; i < npre; ++i) {
    const uint64_t R = 1ull << plan[i];
    void* q;
    MLH_TRY(pool_alloc(ctx, (R << loc.loga[i]) * sizeof(fe), &q));
    scaled.push_back(q);
    const u128 rb = h_pow(gen, (u128)S * rank);
    HIP_TRY(ctx, launch_scale_rows(loc.ta[i], reinterpret_cast<fe*>(q), R, loc.loga[i], to_fe(rb), ctx->stream));
    loc.ta[i] = reinterpret_cast<const fe*>(q);
    S <<= plan[i];
  }
  // the fused last pass's stage twiddles: w_N^(N / 2^9), expanded
  const uint64_t Rl = 1ull << logr[npre];
  MLH_TRY(get_table(ctx, h_pow(gen, (u128)(1ull << (L - logr[npre]))), Rl / 2, 1, &tw_last, true));
  return MLH_OK;
}

mlh_status FusedNtt::run_pre(const void* in, void* out) {
  ProfScope ps(ctx, "ntt_fused_pre");
  HIP_TRY(ctx, launch_ntt_passes_pre(reinterpret_cast<const fe*>(in), reinterpret_cast<fe*>(out), loc, L - p,
                                     nglob - 1, ctx->stream));
  ps.end();
  return MLH_OK;
}

mlh_status FusedNtt::run_last(const void* recv, void* out) {
  ProfScope ps(ctx, "ntt_fused_last");
  HIP_TRY(ctx, launch_ntt_shard_last(reinterpret_cast<const fe*>(recv), reinterpret_cast<fe*>(out), tw_last,
                                     logr, nglob, L, p, rank, ctx->stream));
  ps.end();
  return MLH_OK;
}

// Core NTT on device (in may equal out; zero_top 1: input has N/2 elements,
// 2: N/2 elements stored bit-reversed -- then in must not equal out).
static mlh_status ntt_core(mlh_ctx* ctx, const fe* in, fe* out, uint32_t log_n, u128 gen,
                           bool inverse, int zero_top) {
  NttTables tb;
  MLH_TRY(get_ntt_tables(ctx, gen, log_n, inverse, &tb));
  if (log_n <= 10) {
    const uint64_t N = 1ull << log_n;
    // (in-place is safe: the small kernel reads everything into LDS before writing)
    HIP_TRY(ctx, launch_ntt_small(in, out, tb.tw_small, log_n, zero_top ? N / 2 : N, tb.scale,
                                  inverse, ctx->stream, 1, zero_top == 2));
    return MLH_OK;
  }
  MLH_TRY(ensure_ntt_scratch(ctx, log_n));
  char lab0[64];
  if (ctx->prof_on) ntt_pass_label(tb, 0, zero_top, lab0, sizeof lab0);
  if (ctx->prof_on && prof_sample(ctx, lab0)) {
    std::vector<hipEvent_t> ev(tb.nradix + 1);
    for (auto& e : ev) e = take_event(ctx);
    HIP_TRY(ctx, launch_ntt_passes(in, out, ctx->ntt_scratch, tb, log_n, zero_top, ctx->stream,
                                   ev.data()));
    for (uint32_t p = 0; p < tb.nradix; ++p) {
      char lab[64];
      ntt_pass_label(tb, p, zero_top, lab, sizeof lab);
      ctx->pending.push_back(mlh_ctx::Pending{lab, ev[p], ev[p + 1]});
    }
    return MLH_OK;
  }
  HIP_TRY(ctx, launch_ntt_passes(in, out, ctx->ntt_scratch, tb, log_n, zero_top, ctx->stream));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// context / memory API
// ---------------------------------------------------------------------------
extern "C" {

const char* mlh_version(void) { return "mlhip 0.1 (gfx950)"; }

// why the last mlh_context_create of this thread failed (no context to hold it):
// mlh_last_error(NULL) returns it
static thread_local char g_create_err[160] = "null context";

mlh_status mlh_context_create(int device, void* hip_stream, mlh_ctx** out) {
  if (!out) return MLH_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= device || device < 0) {
    snprintf(g_create_err, sizeof g_create_err, "mlh_context_create: hipGetDeviceCount -> %s, %d devices, device %d",
             hipGetErrorString(e), n, device);
    return MLH_ERR_HIP;
  }
  e = hipSetDevice(device);
  if (e != hipSuccess) {
    snprintf(g_create_err, sizeof g_create_err, "mlh_context_create: hipSetDevice(%d) -> %s", device,
             hipGetErrorString(e));
    return MLH_ERR_HIP;
  }
  std::unique_ptr<mlh_ctx> c(new mlh_ctx());
  c->device = device;
  c->stream = reinterpret_cast<hipStream_t>(hip_stream);
  const char* dbg = getenv("MLH_DEBUG_SYNC");
  c->debug_sync = dbg && *dbg && strcmp(dbg, "0") != 0;
  const char* wide = getenv("MLH_NTT_WIDE_OFFSETS");
  c->ntt_wide_offsets = wide && *wide && strcmp(wide, "0") != 0;
  void* st = nullptr;
  const bool ok = hipMalloc(&c->partials, 2 * kMaxRedBlocks * sizeof(fe)) == hipSuccess &&
                  hipMalloc(&c->small, 64 * sizeof(fe)) == hipSuccess &&
                  hipHostMalloc(&c->pinned, kPinnedBytes, 0) == hipSuccess &&
                  hipHostMalloc(&st, 64, hipHostMallocCoherent) == hipSuccess;
  if (!ok) {  // (hipFree / hipHostFree of a null pointer are no-ops)
    snprintf(g_create_err, sizeof g_create_err, "mlh_context_create: allocation failed (%s)",
             hipGetErrorString(hipGetLastError()));
    (void)hipFree(c->partials);
    (void)hipFree(c->small);
    (void)hipHostFree(c->pinned);
    (void)hipHostFree(st);
    return MLH_ERR_OOM;
  }
  c->dev_status = reinterpret_cast<volatile uint32_t*>(st);
  *c->dev_status = 0;
  // (created here, with the context's device current: mlh_set_stream may be
  // called with another device current)
  if (hipEventCreateWithFlags(&c->switch_ev, hipEventDisableTiming) != hipSuccess) {
    snprintf(g_create_err, sizeof g_create_err, "mlh_context_create: hipEventCreate failed (%s)",
             hipGetErrorString(hipGetLastError()));
    (void)hipFree(c->partials);
    (void)hipFree(c->small);
    (void)hipHostFree(c->pinned);
    (void)hipHostFree(st);
    return MLH_ERR_HIP;
  }
  *out = c.release();
  return MLH_OK;
}

void mlh_context_destroy(mlh_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->side) (void)hipStreamSynchronize(ctx->side);  // before anything it may use is freed
  if (ctx->side2) (void)hipStreamSynchronize(ctx->side2);
  resolve_profile(ctx);
  for (auto e : ctx->ev_free) (void)hipEventDestroy(e);
  if (ctx->switch_ev) (void)hipEventDestroy(ctx->switch_ev);
  for (auto& kv : ctx->tables) (void)hipFree(kv.second.d);
  for (auto& kv : ctx->pool) (void)hipFree(kv.second);
  for (auto& kv : ctx->live) (void)hipFree(kv.first);
  (void)hipFree(ctx->ntt_scratch);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->side2) (void)hipStreamDestroy(ctx->side2);
  (void)hipFree(ctx->partials);
  (void)hipFree(ctx->small);
  (void)hipHostFree(ctx->pinned);
  (void)hipHostFree(const_cast<uint32_t*>(ctx->dev_status));
  if (ctx->qstage) (void)hipHostFree(ctx->qstage);
  delete ctx;
}

mlh_status mlh_set_table_cache_limit(mlh_ctx* ctx, uint64_t bytes) {
  if (!ctx) return MLH_ERR_INVALID;
  ctx->table_limit = (size_t)bytes;
  return table_make_room(ctx, 0);
}

uint64_t mlh_table_cache_bytes(const mlh_ctx* ctx) { return ctx ? ctx->table_bytes : 0; }

mlh_status mlh_set_ntt_plan(mlh_ctx* ctx, const uint32_t* logr, uint32_t count) {
  if (!ctx || (count && !logr) || count > (uint32_t)kMaxPasses)
    return fail(ctx, MLH_ERR_INVALID, "plan: at most kMaxPasses digits");
  for (uint32_t i = 0; i < count; ++i)
    if (logr[i] < 4 || logr[i] > 9) return fail(ctx, MLH_ERR_INVALID, "plan digits must be 4..9");
  ctx->forced_plan_len = count;
  for (uint32_t i = 0; i < count; ++i) ctx->forced_plan[i] = logr[i];
  return MLH_OK;
}

mlh_status mlh_set_coop_spin_limit(mlh_ctx* ctx, uint32_t sleeps) {
  if (!ctx) return MLH_ERR_INVALID;
  ctx->coop_spin = sleeps;
  return MLH_OK;
}

mlh_status mlh_set_pcs_fused_max(mlh_ctx* ctx, uint32_t max_vars) {
  if (!ctx) return MLH_ERR_INVALID;
  ctx->pcs_fused_max = max_vars < 24 ? max_vars : 24;
  return MLH_OK;
}

mlh_status mlh_set_stream(mlh_ctx* ctx, void* hip_stream) {
  if (!ctx) return MLH_ERR_INVALID;
  hipStream_t next = reinterpret_cast<hipStream_t>(hip_stream);
  if (next == ctx->stream) return MLH_OK;
  // Order the new stream behind the old one on the device (no host wait):
  // pool blocks, cached tables still being built and an eviction's drain all
  // assume that later work of the context runs after its earlier work.
  hipStream_t prev = ctx->stream;
  ctx->stream = next;
  HIP_TRY(ctx, hipEventRecord(ctx->switch_ev, prev));
  HIP_TRY(ctx, hipStreamWaitEvent(next, ctx->switch_ev, 0));
  return MLH_OK;
}

mlh_status mlh_set_scratch_poison(mlh_ctx* ctx, uint32_t word) {
  if (!ctx) return MLH_ERR_INVALID;
  ctx->poison = word;
  if (!word) return MLH_OK;
  MLH_TRY(poison_fill(ctx, ctx->partials, 2 * kMaxRedBlocks * sizeof(fe)));
  MLH_TRY(poison_fill(ctx, ctx->small, 64 * sizeof(fe)));
  MLH_TRY(poison_fill(ctx, ctx->ntt_scratch, ctx->ntt_scratch_bytes));
  // the pinned staging is filled by the host: wait for copies that still use it
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint32_t* w = reinterpret_cast<uint32_t*>(ctx->pinned);
  for (size_t i = 0; i < kPinnedBytes / 4; ++i) w[i] = word;
  w = reinterpret_cast<uint32_t*>(ctx->qstage);
  for (size_t i = 0; i < ctx->qstage_bytes / 4; ++i) w[i] = word;
  return MLH_OK;
}

mlh_status mlh_synchronize(mlh_ctx* ctx) {
  if (!ctx) return MLH_ERR_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLH_OK;
}

const char* mlh_last_error(const mlh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err; }

mlh_status mlh_malloc(mlh_ctx* ctx, size_t bytes, void** dev) {
  if (!ctx || !dev) return MLH_ERR_INVALID;
  HIP_TRY(ctx, hipMalloc(dev, bytes ? bytes : 16));
  return MLH_OK;
}
mlh_status mlh_free(mlh_ctx* ctx, void* dev) {
  if (!ctx) return MLH_ERR_INVALID;
  HIP_TRY(ctx, hipFree(dev));
  return MLH_OK;
}
mlh_status mlh_memcpy_h2d(mlh_ctx* ctx, void* dev, const void* host, size_t bytes) {
  if (!ctx) return MLH_ERR_INVALID;
  HIP_TRY(ctx, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLH_OK;
}
mlh_status mlh_memcpy_d2h(mlh_ctx* ctx, void* host, const void* dev, size_t bytes) {
  if (!ctx) return MLH_ERR_INVALID;
  HIP_TRY(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLH_OK;
}
mlh_status mlh_memcpy_d2d(mlh_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return MLH_ERR_INVALID;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// field helpers / NTT
// ---------------------------------------------------------------------------
mlh_status mlh_pow_2_generator(uint32_t log_size, uint8_t gen_out[16]) {
  if (!gen_out || log_size > 40) return MLH_ERR_INVALID;
  h_store(gen_out, h_pow2_generator(log_size));
  return MLH_OK;
}

mlh_status mlh_gen_pows_params(const uint8_t* gen_pows, uint64_t len, uint8_t gen_out[16],
                               uint32_t* log_len_out) {
  if (!gen_pows || !gen_out || !log_len_out) return MLH_ERR_INVALID;
  if (len < 2 || (len & (len - 1)) || len > (1ull << 40)) return MLH_ERR_INVALID;
  const uint32_t lg = 63 - __builtin_clzll(len);
  auto at = [&](uint64_t i) { return h_load(gen_pows + 16 * i); };
  const u128 g = at(1);
  if (at(0) != 1 || !check_generator(g, lg)) return MLH_ERR_INVALID;  // order exactly len
  u128 p = g;
  for (uint32_t j = 0; j < lg; ++j, p = h_mul(p, p))
    if (at(1ull << j) != p) return MLH_ERR_INVALID;  // gen_pows[2^j] = g^(2^j)
  if (at(len / 2) != kModulus - 1 || h_mul(at(len - 1), g) != 1) return MLH_ERR_INVALID;
  // every index below 4096, and 16 pseudo-random ones (SplitMix64 of len)
  p = 1;
  for (uint64_t i = 0; i < len && i < 4096; ++i, p = h_mul(p, g))
    if (at(i) != p) return MLH_ERR_INVALID;
  uint64_t x = len ^ 0x9E3779B97F4A7C15ull;
  for (int q = 0; q < 16; ++q) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const uint64_t i = z & (len - 1);
    if (at(i) != h_pow(g, (u128)i)) return MLH_ERR_INVALID;
  }
  h_store(gen_out, g);
  *log_len_out = lg;
  return MLH_OK;
}

mlh_status mlh_gen_pows_verify(mlh_ctx* ctx, const uint8_t* gen_pows, uint64_t len,
                               uint8_t gen_out[16], uint32_t* log_len_out) {
  if (!ctx || !gen_pows) return fail(ctx, MLH_ERR_INVALID, "null argument");
  uint8_t gb[16];
  uint32_t lg = 0;
  if (mlh_gen_pows_params(gen_pows, len, gb, &lg) != MLH_OK)
    return fail(ctx, MLH_ERR_INVALID, "gen_pows is not the power series of an element of order len");
  const u128 g = h_load(gb);
  const fe *tlo, *thi;
  MLH_TRY(get_table(ctx, g, 4096, 1, &tlo));
  MLH_TRY(get_table(ctx, h_pow(g, 4096), hi_count(lg), 1, &thi));
  const uint64_t chunk = len < (1ull << 20) ? len : (1ull << 20);
  PoolBuf buf(ctx), badb(ctx);
  MLH_TRY(buf.alloc(chunk * 16));
  MLH_TRY(badb.alloc(8));
  unsigned long long* bad = badb.as<unsigned long long>();
  HIP_TRY(ctx, hipMemsetAsync(bad, 0xFF, 8, ctx->stream));
  for (uint64_t base = 0; base < len; base += chunk) {  // stream order keeps buf's reuse safe
    const uint64_t cnt = len - base < chunk ? len - base : chunk;
    HIP_TRY(ctx, hipMemcpyAsync(buf.p, gen_pows + 16 * base, cnt * 16, hipMemcpyHostToDevice,
                                ctx->stream));
    HIP_TRY(ctx, launch_pow_series_check(buf.as<fe>(), base, cnt, tlo, thi, bad, ctx->stream));
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->pinned + kPinSlotB, bad, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t first;
  memcpy(&first, ctx->pinned + kPinSlotB, 8);
  if (first != ~0ull)
    return fail(ctx, MLH_ERR_INVALID,
                "gen_pows[" + std::to_string(first) + "] is not gen_pows[1]^" + std::to_string(first));
  if (gen_out) memcpy(gen_out, gb, 16);
  if (log_len_out) *log_len_out = lg;
  return MLH_OK;
}

mlh_status mlh_pow_2_generator_powers(mlh_ctx* ctx, uint32_t log_size, void* dev_out) {
  if (!ctx || !dev_out || log_size > 40) return fail(ctx, MLH_ERR_INVALID, "bad argument");
  const u128 g = h_pow2_generator(log_size);
  const fe *tlo, *thi;
  MLH_TRY(get_table(ctx, g, 4096, 1, &tlo));
  MLH_TRY(get_table(ctx, h_pow(g, 4096), hi_count(log_size), 1, &thi));
  HIP_TRY(ctx, launch_pow_series(reinterpret_cast<fe*>(dev_out), tlo, thi, 1ull << log_size,
                                 ctx->stream));
  return MLH_OK;
}

static mlh_status ntt_entry(mlh_ctx* ctx, const void* in, void* out, uint32_t log_n,
                            const uint8_t gen[16], bool inverse) {
  if (!ctx || !in || !out || !gen) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_n < 1 || log_n > 32) return fail(ctx, MLH_ERR_NOT_POW2, "The number of coeffs must be a power of 2 (n >= 2)");
  const u128 g = h_load(gen);
  if (g >= kModulus) return fail(ctx, MLH_ERR_BAD_GENERATOR, "generator not canonical");
  if (!check_generator(g, log_n))  // not of order n: the reference's network, not a DFT
    return ntt_network_core(ctx, reinterpret_cast<const fe*>(in), reinterpret_cast<fe*>(out),
                            log_n, g, inverse, 0);
  return ntt_core(ctx, reinterpret_cast<const fe*>(in), reinterpret_cast<fe*>(out), log_n, g,
                  inverse, false);
}

mlh_status mlh_ntt(mlh_ctx* ctx, const void* dev_coeffs, void* dev_evals, uint32_t log_n,
                   const uint8_t gen[16]) {
  return ntt_entry(ctx, dev_coeffs, dev_evals, log_n, gen, false);
}

mlh_status mlh_intt(mlh_ctx* ctx, const void* dev_evals, void* dev_coeffs, uint32_t log_n,
                    const uint8_t gen[16]) {
  return ntt_entry(ctx, dev_evals, dev_coeffs, log_n, gen, true);
}

mlh_status mlh_ntt_batch(mlh_ctx* ctx, const void* dev_coeffs, void* dev_evals, uint32_t log_n,
                         const uint8_t gen[16], uint32_t log_batch) {
  if (!ctx || !dev_coeffs || !dev_evals || !gen) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_n < 1 || log_n > 32 || log_n + log_batch > 32)
    return fail(ctx, MLH_ERR_NOT_POW2, "The number of coeffs must be a power of 2 (n >= 2)");
  const u128 g = h_load(gen);
  if (g >= kModulus || !check_generator(g, log_n))
    return fail(ctx, MLH_ERR_BAD_GENERATOR, "generator not of order 2^log_n");
  const fe* in = reinterpret_cast<const fe*>(dev_coeffs);
  fe* out = reinterpret_cast<fe*>(dev_evals);
  NttTables tb;
  MLH_TRY(get_ntt_tables(ctx, g, log_n, false, &tb));
  const uint64_t batch = 1ull << log_batch;
  if (log_n <= 10) {
    HIP_TRY(ctx, launch_ntt_small(in, out, tb.tw_small, log_n, 1ull << log_n, tb.scale, false,
                                  ctx->stream, batch));
    return MLH_OK;
  }
  MLH_TRY(ensure_ntt_scratch(ctx, log_n + log_batch));
  HIP_TRY(ctx, launch_ntt_passes(in, out, ctx->ntt_scratch, tb, log_n, 0, ctx->stream, nullptr, batch));
  return MLH_OK;
}

static mlh_status vec_op(mlh_ctx* ctx, int op, const void* a, const void* b, void* out, uint64_t n) {
  if (!ctx || !a || !out || (op < 3 && !b)) return fail(ctx, MLH_ERR_INVALID, "null argument");
  HIP_TRY(ctx, launch_vec_op(op, reinterpret_cast<const fe*>(a), reinterpret_cast<const fe*>(b),
                             reinterpret_cast<fe*>(out), n, ctx->stream));
  return MLH_OK;
}
mlh_status mlh_field_add(mlh_ctx* ctx, const void* a, const void* b, void* out, uint64_t n) {
  return vec_op(ctx, 0, a, b, out, n);
}
mlh_status mlh_field_sub(mlh_ctx* ctx, const void* a, const void* b, void* out, uint64_t n) {
  return vec_op(ctx, 1, a, b, out, n);
}
mlh_status mlh_field_mul(mlh_ctx* ctx, const void* a, const void* b, void* out, uint64_t n) {
  return vec_op(ctx, 2, a, b, out, n);
}
mlh_status mlh_field_neg(mlh_ctx* ctx, const void* a, void* out, uint64_t n) {
  return vec_op(ctx, 3, a, nullptr, out, n);
}
mlh_status mlh_field_scale(mlh_ctx* ctx, const void* a, const uint8_t c[16], void* out,
                           uint64_t n) {
  if (!ctx || !a || !out || !c) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (h_load(c) >= kModulus) return fail(ctx, MLH_ERR_INVALID, "scalar not canonical");
  HIP_TRY(ctx, launch_vec_op(4, reinterpret_cast<const fe*>(a), nullptr, reinterpret_cast<fe*>(out),
                             n, ctx->stream, to_fe(h_load(c))));
  return MLH_OK;
}
mlh_status mlh_field_inv(mlh_ctx* ctx, const void* a, void* out, uint64_t n) {
  if (!ctx) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (n == 0) return MLH_OK;
  if (!a || !out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (a != out && ranges_overlap(a, out, n * 16))
    return fail(ctx, MLH_ERR_INVALID, "mlh_field_inv: in place or disjoint buffers only");
  ProfScope ps(ctx, "field_inv");
  HIP_TRY(ctx, launch_field_inv(reinterpret_cast<const fe*>(a), reinterpret_cast<fe*>(out), n,
                                ctx->stream));
  ps.end();
  return MLH_OK;
}

mlh_status mlh_bit_reverse_permutation(mlh_ctx* ctx, const void* dev_in, void* dev_out,
                                       uint32_t log_n) {
  if (!ctx || !dev_in || !dev_out || dev_in == dev_out)
    return fail(ctx, MLH_ERR_INVALID, "bit_reverse_permutation is out of place");
  if (log_n > 40) return fail(ctx, MLH_ERR_INVALID, "log_n too large");
  // n = 1 has no bit reversal in the reference (a usize shifted by 64: a
  // panic); n >= 2 as there
  if (log_n == 0) return fail(ctx, MLH_ERR_NOT_POW2, "bit_reverse_permutation needs n >= 2");
  HIP_TRY(ctx, launch_bitrev(reinterpret_cast<const fe*>(dev_in), reinterpret_cast<fe*>(dev_out),
                             log_n, ctx->stream));
  return MLH_OK;
}

mlh_status mlh_ntt_host(mlh_ctx* ctx, const uint8_t* host_in, uint8_t* host_out, uint32_t log_n,
                        const uint8_t gen[16], int inverse) {
  if (!ctx || !host_in || !host_out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  const size_t bytes = (size_t)16 << log_n;
  PoolBuf buf(ctx);
  MLH_TRY(buf.alloc(bytes));
  HIP_TRY(ctx, hipMemcpyAsync(buf.p, host_in, bytes, hipMemcpyHostToDevice, ctx->stream));
  MLH_TRY(ntt_entry(ctx, buf.p, buf.p, log_n, gen, inverse != 0));
  HIP_TRY(ctx, hipMemcpyAsync(host_out, buf.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// Reed-Solomon / Merkle / fold
// ---------------------------------------------------------------------------
mlh_status mlh_reed_solomon(mlh_ctx* ctx, const void* dev_coeffs, uint32_t log_n,
                            const uint8_t gen[16], void* dev_code) {
  if (!ctx || !dev_coeffs || !dev_code || !gen) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_n > 31) return fail(ctx, MLH_ERR_INVALID, "log_n too large");
  if (dev_coeffs == dev_code) return fail(ctx, MLH_ERR_INVALID, "reed_solomon is out of place");
  const uint32_t lc = log_n + MLH_LOG_BLOWUP;
  const u128 g = h_load(gen);
  if (g >= kModulus) return fail(ctx, MLH_ERR_BAD_GENERATOR, "generator not canonical");
  if (!check_generator(g, lc))  // not of order 2n: the reference's network, not a DFT
    return ntt_network_core(ctx, reinterpret_cast<const fe*>(dev_coeffs),
                            reinterpret_cast<fe*>(dev_code), lc, g, false, 1);
  return ntt_core(ctx, reinterpret_cast<const fe*>(dev_coeffs), reinterpret_cast<fe*>(dev_code),
                  lc, g, false, 1);
}

mlh_status mlh_reed_solomon_brev(mlh_ctx* ctx, const void* dev_coeffs, uint32_t log_n,
                                 const uint8_t gen[16], void* dev_code) {
  if (!ctx || !dev_coeffs || !dev_code || !gen) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_n > 31) return fail(ctx, MLH_ERR_INVALID, "log_n too large");
  if (dev_coeffs == dev_code) return fail(ctx, MLH_ERR_INVALID, "reed_solomon is out of place");
  const uint32_t lc = log_n + MLH_LOG_BLOWUP;
  const u128 g = h_load(gen);
  if (g >= kModulus) return fail(ctx, MLH_ERR_BAD_GENERATOR, "generator not canonical");
  if (!check_generator(g, lc))  // not of order 2n: the reference's network, not a DFT
    return ntt_network_core(ctx, reinterpret_cast<const fe*>(dev_coeffs),
                            reinterpret_cast<fe*>(dev_code), lc, g, false, 2);
  return ntt_core(ctx, reinterpret_cast<const fe*>(dev_coeffs), reinterpret_cast<fe*>(dev_code),
                  lc, g, false, 2);
}

uint64_t mlh_merkle_layers_bytes(uint64_t leaves) { return leaves ? (2 * leaves - 1) * 32 : 0; }

static bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }

mlh_status mlh_merkle_commit_pairs(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                                   void* dev_layers, uint8_t root_out[32]) {
  if (!ctx || !dev_code || !dev_layers) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_code < 1 || log_code > 40)
    return fail(ctx, MLH_ERR_NOT_POW2, "Data length must be a power of two");
  const uint64_t L = 1ull << (log_code - 1);
  uint8_t* layers = reinterpret_cast<uint8_t*>(dev_layers);
  HIP_TRY(ctx, launch_commit_pairs(reinterpret_cast<const fe*>(dev_code), L, layers, ctx->stream));
  return read_root(ctx, layers, L, root_out);
}

mlh_status mlh_merkle_commit(mlh_ctx* ctx, const void* dev_items, uint64_t item_len,
                             uint64_t count, void* dev_layers, uint8_t root_out[32]) {
  if (!ctx || !dev_items || !dev_layers) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (!is_pow2(count)) return fail(ctx, MLH_ERR_NOT_POW2, "Data length must be a power of two");
  uint8_t* layers = reinterpret_cast<uint8_t*>(dev_layers);
  HIP_TRY(ctx, launch_leaf_bytes(reinterpret_cast<const uint8_t*>(dev_items), item_len, count,
                                 layers, ctx->stream));
  HIP_TRY(ctx, launch_merkle_levels(layers, count, ctx->stream));
  return read_root(ctx, layers, count, root_out);
}

mlh_status mlh_merkle_batch_commit(mlh_ctx* ctx, const void* dev_items, uint64_t item_len,
                                   uint32_t m, uint64_t count, void* dev_layers,
                                   uint8_t root_out[32]) {
  if (!ctx || !dev_items || !dev_layers) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (m == 0) return fail(ctx, MLH_ERR_INVALID, "Data must not be empty");
  if (!is_pow2(count))
    return fail(ctx, MLH_ERR_NOT_POW2, "Each batch length must be a power of two");
  uint8_t* layers = reinterpret_cast<uint8_t*>(dev_layers);
  HIP_TRY(ctx, launch_leaf_batch(reinterpret_cast<const uint8_t*>(dev_items), item_len,
                                 item_len * count, m, count, layers, ctx->stream));
  HIP_TRY(ctx, launch_merkle_levels(layers, count, ctx->stream));
  return read_root(ctx, layers, count, root_out);
}

mlh_status mlh_fri_fold(mlh_ctx* ctx, const void* dev_layer, uint32_t log_layer, uint32_t k,
                        uint32_t log_domain, const uint8_t r[16], void* dev_next) {
  if (!ctx || !dev_layer || !dev_next || !r) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_layer < 1 || log_domain > 40 || log_layer + k != log_domain)
    return fail(ctx, MLH_ERR_INVALID, "layer size must be 2^(log_domain - k)");
  const fe *tlo, *thi;
  MLH_TRY(fold_tables(ctx, log_domain, &tlo, &thi));
  HIP_TRY(ctx, launch_fri_fold(reinterpret_cast<const fe*>(dev_layer), 1ull << log_layer,
                               reinterpret_cast<fe*>(dev_next), to_fe(h_load(r)), tlo, thi, k,
                               1ull << log_domain, ctx->stream));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// multilinear / sumcheck
// ---------------------------------------------------------------------------
mlh_status mlh_mle_to_coefficient(mlh_ctx* ctx, void* dev_evals, uint32_t log_n) {
  if (!ctx || !dev_evals || log_n > 40) return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_mobius(reinterpret_cast<fe*>(dev_evals), log_n, false, ctx->stream));
  return MLH_OK;
}

mlh_status mlh_mle_to_evaluation(mlh_ctx* ctx, void* dev_coeffs, uint32_t log_n) {
  if (!ctx || !dev_coeffs || log_n > 40) return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_mobius(reinterpret_cast<fe*>(dev_coeffs), log_n, true, ctx->stream));
  return MLH_OK;
}

static mlh_status eq_table_impl(mlh_ctx* ctx, const uint8_t* host_points, uint32_t n,
                                void* dev_out, bool mono);

mlh_status mlh_eq_table(mlh_ctx* ctx, const uint8_t* host_points, uint32_t n, void* dev_out) {
  return eq_table_impl(ctx, host_points, n, dev_out, false);
}

static mlh_status eq_table_impl(mlh_ctx* ctx, const uint8_t* host_points, uint32_t n,
                                void* dev_out, bool mono) {
  if (!ctx || !dev_out || (n && !host_points) || n > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  PoolBuf pts(ctx), scratch(ctx);
  MLH_TRY(pts.alloc((n ? n : 1) * sizeof(fe)));
  const uint32_t a = n / 2, b = n - a;
  MLH_TRY(scratch.alloc(((1ull << a) + (1ull << b)) * sizeof(fe)));
  if (n) HIP_TRY(ctx, hipMemcpyAsync(pts.p, host_points, n * 16ull, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_eq_table(pts.as<fe>(), n, scratch.as<fe>(), reinterpret_cast<fe*>(dev_out),
                               ctx->stream, mono));
  // pts/scratch go back to the pool now: a later user of those blocks is
  // ordered after these kernels on the same stream (and the pageable H2D
  // above has consumed host_points before returning)
  return MLH_OK;
}

// the first of the pair in ctx->small
static mlh_status read_small_first(mlh_ctx* ctx, uint8_t out[16]) {
  uint8_t pair[32];
  MLH_TRY(read_back(ctx, ctx->small, 32, pair));
  memcpy(out, pair, 16);
  return MLH_OK;
}

mlh_status mlh_mle_evaluate(mlh_ctx* ctx, const void* dev_evals, uint32_t n,
                            const uint8_t* host_args, uint8_t out[16]) {
  if (!ctx || !dev_evals || !out || n > 40) return fail(ctx, MLH_ERR_INVALID, "bad argument");
  PoolBuf eq(ctx);
  MLH_TRY(eq.alloc((16ull << n)));
  MLH_TRY(mlh_eq_table(ctx, host_args, n, eq.p));
  HIP_TRY(ctx, launch_dot(reinterpret_cast<const fe*>(dev_evals), eq.as<fe>(), 1ull << n,
                          ctx->partials, ctx->small, ctx->stream));
  return read_small_first(ctx, out);
}

mlh_status mlh_mle_coeffs_evaluate(mlh_ctx* ctx, const void* dev_coeffs, uint32_t n,
                                   const uint8_t* host_args, uint8_t out[16]) {
  if (!ctx || !dev_coeffs || !out || n > 40) return fail(ctx, MLH_ERR_INVALID, "bad argument");
  PoolBuf mono(ctx);
  MLH_TRY(mono.alloc((16ull << n)));
  MLH_TRY(eq_table_impl(ctx, host_args, n, mono.p, true));
  HIP_TRY(ctx, launch_dot(reinterpret_cast<const fe*>(dev_coeffs), mono.as<fe>(), 1ull << n,
                          ctx->partials, ctx->small, ctx->stream));
  return read_small_first(ctx, out);
}

mlh_status mlh_poly_evaluate(mlh_ctx* ctx, const void* dev_coeffs, uint64_t n, const uint8_t x[16],
                             uint8_t out[16]) {
  if (!ctx || (n && !dev_coeffs) || !x || !out || n > (1ull << 40))
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  if (n == 0) {  // fold over nothing: F::from(0)
    memset(out, 0, 16);
    return MLH_OK;
  }
  const u128 xv = h_load(x);
  if (xv >= kModulus) return fail(ctx, MLH_ERR_INVALID, "x not canonical");
  const uint64_t nlo = n < 4096 ? n : 4096, nhi = (n + 4095) / 4096;
  PoolBuf tlo(ctx), thi(ctx);
  MLH_TRY(tlo.alloc(16 * nlo));
  MLH_TRY(thi.alloc(16 * nhi));
  HIP_TRY(ctx, launch_pow_table(tlo.as<fe>(), to_fe(xv), to_fe(1), nlo, ctx->stream));
  HIP_TRY(ctx, launch_pow_table(thi.as<fe>(), to_fe(h_pow(xv, 4096)), to_fe(1), nhi, ctx->stream));
  HIP_TRY(ctx, launch_poly_eval(reinterpret_cast<const fe*>(dev_coeffs), n, tlo.as<fe>(),
                                thi.as<fe>(), ctx->partials, ctx->small, ctx->stream));
  return read_small_first(ctx, out);
}

mlh_status mlh_trace_evaluate(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                             uint32_t width, const uint8_t* host_points, uint8_t* out) {
  if (!ctx || !dev_matrix || !out || log_height > 40 || width == 0 || width > (1u << 20) ||
      (log_height && !host_points))
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  const uint64_t height = 1ull << log_height;
  const uint32_t nc = width < 256 ? width : 256;
  PoolBuf eq(ctx), partials(ctx), res(ctx);
  MLH_TRY(eq.alloc(16ull << log_height));
  MLH_TRY(partials.alloc(16ull * trace_eval_blocks(height, nc) * nc));
  MLH_TRY(res.alloc(16ull * width));
  MLH_TRY(mlh_eq_table(ctx, host_points, log_height, eq.p));
  HIP_TRY(ctx, launch_trace_eval(reinterpret_cast<const fe*>(dev_matrix), eq.as<fe>(), height, width,
                                 partials.as<fe>(), res.as<fe>(), ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(out, res.p, 16ull * width, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLH_OK;
}

mlh_status mlh_sumcheck_partial_sums(mlh_ctx* ctx, const void* dev_matrix, const void* dev_delta,
                                     uint32_t log_height, uint8_t out[32]) {
  if (!ctx || !dev_matrix || !dev_delta || !out || log_height < 1 || log_height > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_sums(reinterpret_cast<const fe*>(dev_matrix),
                           reinterpret_cast<const fe*>(dev_delta), 1ull << (log_height - 1),
                           ctx->partials, ctx->small, ctx->stream));
  return read_back(ctx, ctx->small, 32, out);
}

mlh_status mlh_sumcheck_fold(mlh_ctx* ctx, void* dev_matrix, void* dev_delta, uint32_t log_height,
                             const uint8_t r[16]) {
  if (!ctx || !dev_matrix || !dev_delta || !r || log_height < 1 || log_height > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_fold(reinterpret_cast<fe*>(dev_matrix), reinterpret_cast<fe*>(dev_delta),
                           1ull << log_height, to_fe(h_load(r)), ctx->stream));
  return MLH_OK;
}

mlh_status mlh_sumcheck_fold_and_sums(mlh_ctx* ctx, void* dev_matrix, void* dev_delta,
                                      uint32_t log_height, const uint8_t r[16], uint8_t out[32]) {
  if (!ctx || !dev_matrix || !dev_delta || !r || !out || log_height < 2 || log_height > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_fold_sums(reinterpret_cast<fe*>(dev_matrix), reinterpret_cast<fe*>(dev_delta),
                                1ull << log_height, to_fe(h_load(r)), ctx->partials, ctx->small,
                                ctx->stream));
  return read_back(ctx, ctx->small, 32, out);
}

mlh_status mlh_merkle_open(mlh_ctx* ctx, const void* dev_layers, uint64_t leaves,
                           const uint64_t* host_idx, uint32_t nq, uint8_t* out) {
  if (!ctx || !dev_layers || (nq && (!host_idx || !out)))
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (!is_pow2(leaves)) return fail(ctx, MLH_ERR_NOT_POW2, "Data length must be a power of two");
  for (uint32_t q = 0; q < nq; ++q)
    if (host_idx[q] >= leaves) return fail(ctx, MLH_ERR_INVALID, "index out of bounds");
  const uint32_t depth = 63 - __builtin_clzll(leaves);
  if (nq == 0 || depth == 0) return MLH_OK;
  const uint64_t rec = 32ull * depth;
  PoolBuf didx(ctx), dout(ctx);
  MLH_TRY(didx.alloc(nq * sizeof(uint64_t)));
  MLH_TRY(dout.alloc(nq * rec));
  HIP_TRY(ctx, hipMemcpyAsync(didx.p, host_idx, nq * sizeof(uint64_t), hipMemcpyHostToDevice,
                              ctx->stream));
  HIP_TRY(ctx, launch_merkle_paths(reinterpret_cast<const uint8_t*>(dev_layers), leaves,
                                   didx.as<uint64_t>(), nq, dout.as<uint8_t>(), ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(out, dout.p, nq * rec, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// kernel timer
// ---------------------------------------------------------------------------
mlh_status mlh_profile_enable(mlh_ctx* ctx, int on) {
  if (!ctx || on < 0) return MLH_ERR_INVALID;
  ctx->prof_on = on != 0;
  ctx->prof_every = on > 1 ? (uint32_t)on : 1u;
  ctx->prof_ticks.clear();
  return MLH_OK;
}

mlh_status mlh_profile_reset(mlh_ctx* ctx) {
  if (!ctx) return MLH_ERR_INVALID;
  resolve_profile(ctx);
  ctx->prof.clear();
  return MLH_OK;
}

mlh_status mlh_profile_get(mlh_ctx* ctx, const char* label, uint64_t* count, double* total_ms) {
  if (!ctx || !label || !count || !total_ms) return MLH_ERR_INVALID;
  resolve_profile(ctx);
  auto it = ctx->prof.find(label);
  *count = it == ctx->prof.end() ? 0 : it->second.first;
  *total_ms = it == ctx->prof.end() ? 0.0 : it->second.second;
  return MLH_OK;
}

// ---------------------------------------------------------------------------
// bench helper
// ---------------------------------------------------------------------------
mlh_status mlh_bench_ntt(mlh_ctx* ctx, void* dev_buf, uint32_t log_n, uint32_t iters,
                         float* ms_out) {
  if (!ctx || !dev_buf || !ms_out || iters == 0) return fail(ctx, MLH_ERR_INVALID, "bad argument");
  uint8_t gen[16];
  h_store(gen, h_pow2_generator(log_n));
  MLH_TRY(mlh_ntt(ctx, dev_buf, dev_buf, log_n, gen));  // warm the table cache
  hipEvent_t a, b;
  HIP_TRY(ctx, hipEventCreate(&a));
  HIP_TRY(ctx, hipEventCreate(&b));
  HIP_TRY(ctx, hipEventRecord(a, ctx->stream));
  for (uint32_t i = 0; i < iters; ++i) MLH_TRY(mlh_ntt(ctx, dev_buf, dev_buf, log_n, gen));
  HIP_TRY(ctx, hipEventRecord(b, ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(b));
  float ms = 0;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *ms_out = ms / iters;
  return MLH_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// trace commitment and the system proof (constraint_system/trace.rs:40-48,
// system.rs:56-72): Commitment::new as the commit phase of the batched PCS
// over the trace's column MLEs, opened at the sumcheck's point.
// ---------------------------------------------------------------------------
struct mlh_trace_commitment {
  mlh_ctx* ctx;
  uint32_t log_height = 0, width = 0;
  void* evals = nullptr;  // [width][2^log_height] column MLEs
  void* codes = nullptr;  // [width][2^(log_height+1)] RS codes
  void* tree = nullptr;   // batch layer: 2^log_height leaves + levels
  uint8_t root[32];
  ~mlh_trace_commitment() {
    pool_free(ctx, evals);
    pool_free(ctx, codes);
    pool_free(ctx, tree);
  }
};

static bool trace_range_ok(uint32_t log_height, uint32_t width, uint32_t col0, uint32_t ncols) {
  return width >= 1 && width <= kCsMaxWidth && log_height <= kCsMaxLogHeight && ncols >= 1 &&
         col0 < width && ncols <= width - col0;
}

// mlh_trace_columns (col0 = 0, ncols = width) and mlh_trace_columns_range.
// dev_out holds ncols columns and the trace is read over its whole extent; for
// the whole width that is the plain overlap rule.
static mlh_status trace_columns_impl(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                     uint32_t width, uint32_t col0, uint32_t ncols, void* dev_out) {
  if (!ctx || !dev_matrix || !dev_out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (!trace_range_ok(log_height, width, col0, ncols))
    return fail(ctx, MLH_ERR_INVALID,
                "width 1..32, log_height 0..32, a column range inside the trace");
  const uint64_t tb = ((uint64_t)width << log_height) * 16, ob = ((uint64_t)ncols << log_height) * 16;
  const uintptr_t x = (uintptr_t)dev_matrix, y = (uintptr_t)dev_out;
  if (x < y ? y - x < tb : x - y < ob)
    return fail(ctx, MLH_ERR_INVALID, "the trace transpose is out of place: the buffers overlap");
  ProfScope ps(ctx, ncols == width ? "trace_columns" : "trace_columns_range");
  HIP_TRY(ctx, launch_trace_columns(reinterpret_cast<const fe*>(dev_matrix),
                                    reinterpret_cast<fe*>(dev_out), log_height, width, col0, ncols,
                                    ctx->stream));
  ps.end();
  return MLH_OK;
}

static mlh_status trace_launch_info(uint32_t log_height, uint32_t width, uint32_t col0,
                                    uint32_t ncols, uint32_t* tile_rows, uint32_t* blocks) {
  if (!tile_rows || !blocks || !trace_range_ok(log_height, width, col0, ncols))
    return MLH_ERR_INVALID;
  *tile_rows = tc_tile_rows(ncols);
  *blocks = tc_blocks(1ull << log_height, ncols);
  return MLH_OK;
}

// Commitment::new over columns [col0, col0 + ncols)
static mlh_status trace_commit_impl(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                    uint32_t width, uint32_t col0, uint32_t ncols,
                                    mlh_trace_commitment** out) {
  if (!ctx || !dev_matrix || !out) return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (log_height < 1 || !trace_range_ok(log_height, width, col0, ncols))
    return fail(ctx, MLH_ERR_INVALID,
                "width 1..32, log_height 1..32, a column range inside the trace");
  std::unique_ptr<mlh_trace_commitment> c(new mlh_trace_commitment());
  c->ctx = ctx;
  c->log_height = log_height;
  c->width = ncols;
  const uint64_t n = 1ull << log_height;
  MLH_TRY(pool_alloc(ctx, ncols * n * 16, &c->evals));
  MLH_TRY(pool_alloc(ctx, ncols * n * 32, &c->codes));
  MLH_TRY(pool_alloc(ctx, mlh_merkle_layers_bytes(n), &c->tree));
  MLH_TRY(trace_columns_impl(ctx, dev_matrix, log_height, width, col0, ncols, c->evals));
  fe* codes = reinterpret_cast<fe*>(c->codes);
  MLH_TRY(batched_pcs_codes(ctx, c->evals, ncols, log_height, codes));
  // the batch layer of BatchedFriProverData::init (batched_fri.rs:41-81)
  uint8_t* bt = reinterpret_cast<uint8_t*>(c->tree);
  MLH_TRY(batch_layer_commit(ctx, codes, ncols, 2 * n, bt));
  MLH_TRY(read_root(ctx, bt, n, c->root));
  *out = c.release();
  return MLH_OK;
}

extern "C" {

mlh_status mlh_trace_columns(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                             uint32_t width, void* dev_out) {
  return trace_columns_impl(ctx, dev_matrix, log_height, width, 0, width, dev_out);
}

mlh_status mlh_trace_columns_launch_info(uint32_t log_height, uint32_t width, uint32_t* tile_rows,
                                         uint32_t* blocks) {
  return trace_launch_info(log_height, width, 0, width, tile_rows, blocks);
}

mlh_status mlh_trace_columns_range(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                   uint32_t width, uint32_t col0, uint32_t ncols, void* dev_out) {
  return trace_columns_impl(ctx, dev_matrix, log_height, width, col0, ncols, dev_out);
}

mlh_status mlh_trace_columns_range_launch_info(uint32_t log_height, uint32_t width, uint32_t col0,
                                               uint32_t ncols, uint32_t* tile_rows,
                                               uint32_t* blocks) {
  return trace_launch_info(log_height, width, col0, ncols, tile_rows, blocks);
}

mlh_status mlh_trace_commit(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                            uint32_t width, mlh_trace_commitment** out) {
  return trace_commit_impl(ctx, dev_matrix, log_height, width, 0, width, out);
}

mlh_status mlh_trace_commit_range(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                  uint32_t width, uint32_t col0, uint32_t ncols,
                                  mlh_trace_commitment** out) {
  return trace_commit_impl(ctx, dev_matrix, log_height, width, col0, ncols, out);
}

mlh_status mlh_trace_commitment_root(const mlh_trace_commitment* c, uint8_t out[32]) {
  if (!c || !out) return MLH_ERR_INVALID;
  memcpy(out, c->root, 32);
  return MLH_OK;
}

uint32_t mlh_trace_commitment_width(const mlh_trace_commitment* c) { return c ? c->width : 0; }

uint32_t mlh_trace_commitment_log_height(const mlh_trace_commitment* c) {
  return c ? c->log_height : 0;
}

void mlh_trace_commitment_destroy(mlh_trace_commitment* c) {
  if (c) {
    (void)hipStreamSynchronize(c->ctx->stream);
    delete c;
  }
}

}  // extern "C"

// ---------------------------------------------------------------------------
// constraint-system sumcheck (constraint_system/sumcheck.rs:40-53,147-247):
// width-W tables, the composition a constraint program (cs_program.hpp)
// ---------------------------------------------------------------------------
static bool cs_args_ok(const mlh_cs_program* prog, uint32_t width, const void* m, const void* d,
                       const uint8_t* randoms, const uint8_t* mask) {
  return prog && m && d && mask && width == prog->p.width && (!prog->p.n_randoms || randoms);
}

static mlh_status cs_read_sums(mlh_ctx* ctx, const CsCall& cc, uint32_t nb, uint8_t* out) {
  static_assert(16 * (kCsMaxDegree + 2) <= kPinnedBytes, "a round's sums fit the staging buffer");
  HIP_TRY(ctx, launch_cs_reduce(ctx->partials, nb, cc.dev.D, ctx->small, ctx->stream));
  return read_back(ctx, ctx->small, 16ull * cc.dev.D, out);
}

extern "C" {

mlh_status mlh_cs_partial_sums(mlh_ctx* ctx, const mlh_cs_program* prog, uint32_t width,
                               const void* dev_matrix, const void* dev_delta, uint32_t log_height,
                               const uint8_t* host_randoms, const uint8_t* host_mask,
                               uint8_t* out) {
  if (!ctx || !out || !cs_args_ok(prog, width, dev_matrix, dev_delta, host_randoms, host_mask) ||
      log_height < 1 || log_height > kCsMaxLogHeight)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  CsCall cc(ctx);
  MLH_TRY(cc.init(ctx, prog, host_randoms, host_mask));
  uint32_t nb = 0;
  HIP_TRY(ctx, launch_cs_sums(cc.dev, cc.threads, reinterpret_cast<const fe*>(dev_matrix),
                              reinterpret_cast<const fe*>(dev_delta), 1ull << (log_height - 1),
                              ctx->partials, ctx->stream, &nb));
  return cs_read_sums(ctx, cc, nb, out);
}

mlh_status mlh_cs_fold(mlh_ctx* ctx, uint32_t width, void* dev_matrix, void* dev_delta,
                       uint32_t log_height, const uint8_t r[16]) {
  if (!ctx || !dev_matrix || !dev_delta || !r || width < 1 || width > kCsMaxWidth ||
      log_height < 1 || log_height > kCsMaxLogHeight || h_load(r) >= kModulus)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  HIP_TRY(ctx, launch_cs_fold(width, reinterpret_cast<fe*>(dev_matrix),
                              reinterpret_cast<fe*>(dev_delta), 1ull << log_height,
                              to_fe(h_load(r)), nullptr, ctx->stream));
  return MLH_OK;
}

mlh_status mlh_cs_fold_and_sums(mlh_ctx* ctx, const mlh_cs_program* prog, uint32_t width,
                                void* dev_matrix, void* dev_delta, uint32_t log_height,
                                const uint8_t* host_randoms, const uint8_t* host_mask,
                                const uint8_t r[16], uint8_t* out) {
  if (!ctx || !out || !r || !cs_args_ok(prog, width, dev_matrix, dev_delta, host_randoms, host_mask) ||
      log_height < 2 || log_height > kCsMaxLogHeight || h_load(r) >= kModulus)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  CsCall cc(ctx);
  MLH_TRY(cc.init(ctx, prog, host_randoms, host_mask));
  uint32_t nb = 0;
  HIP_TRY(ctx, launch_cs_fold_sums(cc.dev, cc.threads, reinterpret_cast<fe*>(dev_matrix),
                                   reinterpret_cast<fe*>(dev_delta), 1ull << log_height,
                                   to_fe(h_load(r)), nullptr, ctx->partials, ctx->stream, &nb));
  return cs_read_sums(ctx, cc, nb, out);
}

mlh_status mlh_cs_sumcheck_prove(mlh_ctx* ctx, const mlh_cs_program* prog, uint32_t width,
                                 void* dev_matrix, void* dev_delta, uint32_t log_height,
                                 const uint8_t* host_randoms, const uint8_t* host_mask,
                                 const uint8_t sum[16], mlh_transcript* tr, uint8_t* polys_out,
                                 uint8_t* rs_out) {
  return mlh_cs_sumcheck_prove_sums(ctx, prog, width, dev_matrix, dev_delta, log_height, host_randoms,
                                    host_mask, 0, nullptr, sum, tr, polys_out, rs_out);
}

mlh_status mlh_cs_sumcheck_prove_sums(mlh_ctx* ctx, const mlh_cs_program* prog, uint32_t width,
                                      void* dev_matrix, void* dev_delta, uint32_t log_height,
                                      const uint8_t* host_randoms, const uint8_t* host_mask,
                                      uint32_t sum_column_mask, const uint8_t* beta,
                                      const uint8_t claim[16], mlh_transcript* tr,
                                      uint8_t* polys_out, uint8_t* rs_out) {
  if (!ctx || !claim || !tr || !cs_args_ok(prog, width, dev_matrix, dev_delta, host_randoms, host_mask) ||
      log_height > kCsMaxLogHeight || h_load(claim) >= kModulus)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  const uint32_t smask = sum_column_mask;
  if (smask && (!beta || h_load(beta) >= kModulus || (width < 32 && (smask >> width))))
    return fail(ctx, MLH_ERR_INVALID, "sum columns: beta missing or a mask bit at or above the width");
  const uint32_t L = log_height;
  if (L == 0) return MLH_OK;  // zero rounds (sumcheck.rs:160-161)
  CsCall cc(ctx);
  MLH_TRY(cc.init(ctx, prog, host_randoms, host_mask));
  const uint32_t D = cc.dev.D;
  // the round buffer, behind its challenges the sum columns' 2 x kCsMaxBlocks
  // partials; one sync, at the end
  RoundBuf rb(ctx, D, L);
  MLH_TRY(rb.alloc(smask ? 32ull * kCsMaxBlocks : 0));
  fe* lin = smask ? rb.extra() : nullptr;
  const fe fbeta = smask ? to_fe(h_load(beta)) : fe{};
  MLH_TRY(rb.seed(tr, claim));
  fe* m = reinterpret_cast<fe*>(dev_matrix);
  fe* d = reinterpret_cast<fe*>(dev_delta);
  uint32_t nb = 0;
  {
    ProfScope ps(ctx, "cs_sums");
    HIP_TRY(ctx, launch_cs_sums(cc.dev, cc.threads, m, d, 1ull << (L - 1), ctx->partials,
                                ctx->stream, &nb, smask, lin));
    ps.end();
  }
  for (uint32_t k = 0; k < L; ++k) {
    {
      ProfScope ps(ctx, "cs_round");
      HIP_TRY(ctx, launch_cs_round(ctx->partials, nb, D, cc.vinv, rb.prev(), rb.dt(), rb.poly(k),
                                   rb.r(k), ctx->stream, lin, fbeta));
      ps.end();
    }
    const uint64_t S = 1ull << (L - k);
    if (S >= 4) {  // fold with r_k + round k+1's sums, one pass
      ProfScope ps(ctx, "cs_fold_sums");
      HIP_TRY(ctx, launch_cs_fold_sums(cc.dev, cc.threads, m, d, S, fe{}, rb.r(k), ctx->partials,
                                       ctx->stream, &nb, smask, lin));
      ps.end();
    } else {
      ProfScope ps(ctx, "cs_fold");
      HIP_TRY(ctx, launch_cs_fold(width, m, d, S, fe{}, rb.r(k), ctx->stream));
      ps.end();
    }
  }
  static_assert(16ull * (kCsMaxDegree + 2) * kCsMaxLogHeight <= kPinStage, "prove staging");
  MLH_TRY(rb.read_back());
  MLH_TRY(rb.replay(tr));  // (sumcheck.rs:194-198)
  rb.copy_out(polys_out, rs_out);
  return MLH_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// System::prover + the composed proof (system.rs:56-72): commitment root ->
// ChallengeSet -> constraint sumcheck -> batched PCS opening of the committed
// columns at the sumcheck's point.
// ---------------------------------------------------------------------------
// Drains the stream when it leaves scope (null: nothing): declared behind the
// pooled buffers of a call, it runs before they go back to the pool, on every
// return path.
struct StreamDrain {
  mlh_ctx* ctx;
  explicit StreamDrain(mlh_ctx* c) : ctx(c) {}
  ~StreamDrain() {
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
  }
};
// The shift part of mlh_system_prove_shifted as the prover core sees it.
struct ShiftProve {
  const uint32_t* cols;
  uint32_t K;
  void* dev_copy;  // the W-wide trace, untouched; folded here
  void* dev_succ;  // 2^L elements of scratch: the rotated eq table
  uint8_t* polys_out;
  uint8_t* output2_out;
  mlh_batched_pcs_proof* pcs1;
  mlh_batched_pcs_proof* pcs2;
};
// What follows the argument checks of the system provers: the transcript
// head, delta = eq(row), the sumcheck rounds, output = row 0 of the folded
// matrix, then BatchedPCSProof::prove(inputs = rs, outputs = output) on each
// handle's codes, evaluations and batch tree -- com1 for its columns into pcs1,
// com2 (null: one phase) for the rest into pcs2.  A failure leaves the
// transcript as at entry, the root absorbed first included.
// sh (null: none; K = 0: none, but the stream is drained before the pooled
// delta table goes back): dev_matrix is then the extension, prog->p.width = W
// + K columns wide, and after the sumcheck comes the shift reduction on
// sh->dev_copy (mlhip.h, step 7) and, behind the openings at rs, those of the
// same handles at rs'.
// public_digest (null: none): the digest of the public columns' spec, absorbed
// first (step 0); the handles then cover the columns below the public ones, and
// the openings, which take the handles' widths, leave those out.
static mlh_status system_prove_core(mlh_ctx* ctx, const mlh_cs_program* prog,
                                    const mlh_trace_commitment* com1,
                                    const mlh_trace_commitment* com2, uint32_t sum_column_mask,
                                    void* dev_matrix, const uint8_t sum[16],
                                    const uint8_t* column_sum, mlh_transcript* tr,
                                    uint8_t* polys_out, uint8_t* output_out,
                                    mlh_batched_pcs_proof* pcs1, mlh_batched_pcs_proof* pcs2,
                                    const ShiftProve* sh = nullptr,
                                    const uint8_t* public_digest = nullptr) {
  const uint32_t L = com1->log_height, W = prog->p.width;
  TranscriptGuard guard(tr);
  SystemHead h(prog->p, L);
  if (system_head(tr, prog->p, L, public_digest, com1->root, com2 ? com2->root : nullptr,
                  sum_column_mask, sum, column_sum, &h) != MLH_OK)
    return fail(ctx, MLH_ERR_INVALID, "challenge set");
  PoolBuf delta(ctx);
  StreamDrain drain(sh ? ctx : nullptr);
  if (sh && !sh->K) sh = nullptr;  // no shifted column: the phased proof from here on
  MLH_TRY(delta.alloc(16ull << L));
  MLH_TRY(mlh_eq_table(ctx, h.row.data(), L, delta.p));
  std::vector<uint8_t> rs(16ull * L);
  {
    ProfScope ps(ctx, "system_sumcheck");
    MLH_TRY(mlh_cs_sumcheck_prove_sums(ctx, prog, W, dev_matrix, delta.p, L, h.randoms.data(),
                                       h.mask.data(), sum_column_mask, h.beta, h.claim, tr,
                                       polys_out, rs.data()));
    ps.end();
  }
  static_assert(16 * kCsMaxWidth <= kPinnedBytes, "a row of the trace fits the staging buffer");
  std::vector<uint8_t> output(16ull * W), rs2(16ull * L), output2;
  MLH_TRY(read_back(ctx, dev_matrix, output.size(), output.data()));
  if (sh) {  // step 7: sum_j succ_rs[j] sum_k lambda^k T_{c_k}[j] = sum_k lambda^k N_k
    ProfScope ps(ctx, "system_shift_sumcheck");
    const uint32_t Wt = W - sh->K;
    mlh_cs_program sp;
    if (!cs_shift_program(Wt, sh->cols, sh->K, sp.p)) return fail(ctx, MLH_ERR_INVALID, "shift list");
    std::vector<uint8_t> lambdas;
    uint8_t claim2[16], one[16];
    h_store(one, 1);
    shift_challenge(tr, output.data(), Wt, sh->K, &lambdas, claim2);
    // eq(rs) into the delta table the sumcheck has consumed, rotated by a row
    MLH_TRY(mlh_eq_table(ctx, rs.data(), L, delta.p));
    HIP_TRY(ctx, launch_eq_rotate(delta.as<const fe>(), reinterpret_cast<fe*>(sh->dev_succ), L,
                                  ctx->stream));
    MLH_TRY(mlh_cs_sumcheck_prove(ctx, &sp, Wt, sh->dev_copy, sh->dev_succ, L, lambdas.data(), one,
                                  claim2, tr, sh->polys_out, rs2.data()));
    output2.resize(16ull * Wt);
    MLH_TRY(read_back(ctx, sh->dev_copy, output2.size(), output2.data()));
    ps.end();
  }
  {
    ProfScope ps(ctx, "system_open");
    MLH_TRY(batched_pcs_open(ctx, reinterpret_cast<const fe*>(com1->codes), com1->evals,
                             reinterpret_cast<const uint8_t*>(com1->tree), com1->width, L, rs.data(),
                             output.data(), tr, pcs1));
    ps.end();
  }
  if (com2) {
    ProfScope ps(ctx, "system_open2");
    MLH_TRY(batched_pcs_open(ctx, reinterpret_cast<const fe*>(com2->codes), com2->evals,
                             reinterpret_cast<const uint8_t*>(com2->tree), com2->width, L, rs.data(),
                             output.data() + 16ull * com1->width, tr, pcs2));
    ps.end();
  }
  if (sh) {  // the same handles at (rs', output2)
    ProfScope ps(ctx, "system_open_shift");
    MLH_TRY(batched_pcs_open(ctx, reinterpret_cast<const fe*>(com1->codes), com1->evals,
                             reinterpret_cast<const uint8_t*>(com1->tree), com1->width, L, rs2.data(),
                             output2.data(), tr, sh->pcs1));
    if (com2)
      MLH_TRY(batched_pcs_open(ctx, reinterpret_cast<const fe*>(com2->codes), com2->evals,
                               reinterpret_cast<const uint8_t*>(com2->tree), com2->width, L,
                               rs2.data(), output2.data() + 16ull * com1->width, tr, sh->pcs2));
    ps.end();
    memcpy(sh->output2_out, output2.data(), output2.size());
  }
  memcpy(output_out, output.data(), output.size());
  guard.keep();
  return MLH_OK;
}

extern "C" {

mlh_status mlh_system_prove(mlh_ctx* ctx, const mlh_cs_program* prog,
                            const mlh_trace_commitment* com, void* dev_matrix,
                            const uint8_t sum[16], mlh_transcript* tr, mlh_system_proof* proof) {
  if (!ctx || !prog || !com || !dev_matrix || !sum || !tr || !proof || !proof->sumcheck_polys ||
      !proof->output)
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (com->ctx != ctx) return fail(ctx, MLH_ERR_INVALID, "commitment of another context");
  if (prog->p.width != com->width)
    return fail(ctx, MLH_ERR_INVALID, "program width differs from the commitment's");
  if (h_load(sum) >= kModulus) return fail(ctx, MLH_ERR_INVALID, "non-canonical sum");
  MLH_TRY(system_prove_core(ctx, prog, com, nullptr, 0, dev_matrix, sum, nullptr, tr,
                            proof->sumcheck_polys, proof->output, &proof->pcs, nullptr));
  proof->log_height = com->log_height;
  proof->width = com->width;
  proof->degree = prog->p.degree;
  return MLH_OK;
}

// The two-phase proof (WitnessLayout::pre_random_columns / sum_columns,
// system.rs:17-30): mlhip.h gives the transcript order.
mlh_status mlh_system_prove_phased(mlh_ctx* ctx, const mlh_cs_program* prog,
                                   const mlh_trace_commitment* com1,
                                   const mlh_trace_commitment* com2, uint32_t sum_column_mask,
                                   void* dev_matrix, const uint8_t sum[16],
                                   const uint8_t column_sum[16], mlh_transcript* tr,
                                   mlh_phased_proof* proof) {
  if (!ctx || !prog || !com1 || !dev_matrix || !sum || !column_sum || !tr || !proof ||
      !proof->sumcheck_polys || !proof->output)
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (com1->ctx != ctx || (com2 && com2->ctx != ctx))
    return fail(ctx, MLH_ERR_INVALID, "commitment of another context");
  const uint32_t W = prog->p.width, P1 = com1->width, P2 = com2 ? com2->width : 0;
  if (P1 < 1 || P1 + P2 != W || (com2 && com2->log_height != com1->log_height))
    return fail(ctx, MLH_ERR_INVALID,
                "the commitments' widths must add up to the program's (com2 null iff all columns "
                "are pre-random), over the same rows");
  if (W < 32 && (sum_column_mask >> W))
    return fail(ctx, MLH_ERR_INVALID, "sum column at or above the width");
  if (h_load(sum) >= kModulus || h_load(column_sum) >= kModulus)
    return fail(ctx, MLH_ERR_INVALID, "non-canonical sum");
  MLH_TRY(system_prove_core(ctx, prog, com1, com2, sum_column_mask, dev_matrix, sum, column_sum, tr,
                            proof->sumcheck_polys, proof->output, &proof->pcs[0], &proof->pcs[1]));
  proof->log_height = com1->log_height;
  proof->width = W;
  proof->degree = prog->p.degree;
  proof->pre_random_columns = P1;
  proof->sum_column_mask = sum_column_mask;
  return MLH_OK;
}

mlh_status mlh_system_prove_public(mlh_ctx* ctx, const mlh_cs_program* prog,
                                   const mlh_trace_commitment* com1,
                                   const mlh_trace_commitment* com2, uint32_t sum_column_mask,
                                   const uint32_t* shift_columns, uint32_t n_shifts,
                                   const mlh_public_columns* spec, const void* dev_matrix,
                                   const uint8_t sum[16], const uint8_t column_sum[16],
                                   mlh_transcript* tr, mlh_shifted_proof* proof) {
  const uint32_t K = n_shifts, F = spec ? spec->p.count() : 0;
  if (!ctx || !prog || !com1 || !dev_matrix || !sum || !column_sum || !tr || !proof ||
      !proof->sumcheck_polys || !proof->output ||
      (K && (!shift_columns || !proof->shift_polys || !proof->output2)))
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (com1->ctx != ctx || (com2 && com2->ctx != ctx))
    return fail(ctx, MLH_ERR_INVALID, "commitment of another context");
  const uint32_t Wx = prog->p.width, P1 = com1->width, P2 = com2 ? com2->width : 0;
  if (!shift_list_ok(Wx, shift_columns, K))
    return fail(ctx, MLH_ERR_INVALID,
                "shift list: distinct source columns below W, W + K the program's width, at most 32");
  const uint32_t W = Wx - K, L = com1->log_height;
  if (F >= W) return fail(ctx, MLH_ERR_INVALID, "as many public columns as the trace has columns");
  if (P1 < 1 || P1 + P2 + F != W || (com2 && com2->log_height != L))
    return fail(ctx, MLH_ERR_INVALID,
                "the commitments' widths, the public columns and n_shifts must add up to the "
                "program's width (com2 null iff all committed columns are pre-random), over the "
                "same rows");
  if (spec && !spec->p.fits(L))
    return fail(ctx, MLH_ERR_INVALID, "a period or a sparse row of the spec is beyond the height");
  if (W < 32 && (sum_column_mask >> W))
    return fail(ctx, MLH_ERR_INVALID, "sum column at or above the trace's width");
  if (h_load(sum) >= kModulus || h_load(column_sum) >= kModulus)
    return fail(ctx, MLH_ERR_INVALID, "non-canonical sum");
  // E, the copy of T for the shift reduction and its delta table: pooled, and
  // back in the pool only after the stream is drained
  PoolBuf ext(ctx), copy(ctx), succ(ctx);
  StreamDrain drain(ctx);
  MLH_TRY(ext.alloc((16ull * Wx) << L));
  MLH_TRY(mlh_trace_extend_next(ctx, dev_matrix, L, W, shift_columns, K, ext.p));
  ShiftProve sh = {shift_columns, K, nullptr, nullptr, proof->shift_polys, proof->output2,
                   &proof->pcs_shift[0], &proof->pcs_shift[1]};
  if (K) {
    MLH_TRY(copy.alloc((16ull * W) << L));
    MLH_TRY(succ.alloc(16ull << L));
    HIP_TRY(ctx, hipMemcpyAsync(copy.p, dev_matrix, (16ull * W) << L, hipMemcpyDeviceToDevice,
                                ctx->stream));
    sh.dev_copy = copy.p;
    sh.dev_succ = succ.p;
  }
  MLH_TRY(system_prove_core(ctx, prog, com1, com2, sum_column_mask, ext.p, sum, column_sum, tr,
                            proof->sumcheck_polys, proof->output, &proof->pcs[0], &proof->pcs[1],
                            &sh, spec ? spec->p.digest : nullptr));
  proof->log_height = L;
  proof->width = W;
  proof->degree = prog->p.degree;
  proof->pre_random_columns = P1;
  proof->sum_column_mask = sum_column_mask;
  proof->n_shifts = K;
  for (uint32_t k = 0; k < 32; ++k) proof->shift_columns[k] = k < K ? shift_columns[k] : 0u;
  return MLH_OK;
}

mlh_status mlh_system_prove_shifted(mlh_ctx* ctx, const mlh_cs_program* prog,
                                    const mlh_trace_commitment* com1,
                                    const mlh_trace_commitment* com2, uint32_t sum_column_mask,
                                    const uint32_t* shift_columns, uint32_t n_shifts,
                                    const void* dev_matrix, const uint8_t sum[16],
                                    const uint8_t column_sum[16], mlh_transcript* tr,
                                    mlh_shifted_proof* proof) {
  return mlh_system_prove_public(ctx, prog, com1, com2, sum_column_mask, shift_columns, n_shifts,
                                 nullptr, dev_matrix, sum, column_sum, tr, proof);
}

}  // extern "C"
