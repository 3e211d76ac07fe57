// The sumcheck and PCS provers' host side, the layer above the FRI prover
// (fri_prover.hip) --
//   SumcheckTables::compute_sumcheck_polynomial(s)   sumcheck.rs:77-202
//   PCSProof::prove                                  multilinear_pcs.rs:90-136
//   BatchedPCSProof::prove                           batched_pcs.rs:127-180
// -- with the transcript on the device: the launch order below is the proof's
// transcript order, so every step of it is written once.
#include "pcs_prover.hpp"

#include "fieldops.hpp"
#include "fri_prover.hpp"

using namespace mlh;

static CoopCtl coop_ctl(mlh_ctx* ctx) {
  return CoopCtl{const_cast<uint32_t*>(ctx->dev_status), ctx->coop_spin};
}

// The code front of both PCS provers: the copy and the permutation are folded
// into the Moebius and first NTT passes; gen_pows[1] (multilinear_pcs.rs:103-104)
mlh_status batched_pcs_codes(mlh_ctx* ctx, const void* dev_evals, uint32_t num_polys,
                             uint32_t n_vars, fe* dev_codes) {
  const uint64_t n = 1ull << n_vars, N = 2 * n;
  uint8_t genb[16];
  h_store(genb, h_pow2_generator(n_vars + MLH_LOG_BLOWUP));
  PoolBuf coeffs(ctx);
  MLH_TRY(coeffs.alloc(n * 16));
  const uint8_t* ev = reinterpret_cast<const uint8_t*>(dev_evals);
  for (uint32_t j = 0; j < num_polys; ++j) {
    HIP_TRY(ctx, launch_mobius(coeffs.as<fe>(), n_vars, false, ctx->stream,
                               reinterpret_cast<const fe*>(ev + (uint64_t)j * n * 16)));
    MLH_TRY(mlh_reed_solomon_brev(ctx, coeffs.p, n_vars, genb,
                                  reinterpret_cast<uint8_t*>(dev_codes) + (uint64_t)j * N * 16));
  }
  return MLH_OK;
}

extern "C" {

mlh_status mlh_sumcheck_prove(mlh_ctx* ctx, void* dev_matrix, void* dev_delta, uint32_t log_height,
                              const uint8_t sum[16], mlh_transcript* tr, uint8_t* polys_out,
                              uint8_t* rs_out) {
  if (!ctx || !dev_matrix || !dev_delta || !sum || !tr || log_height < 1 || log_height > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  // transcript on the device (one sync)
  const uint32_t L = log_height;
  RoundBuf rb(ctx, 2, L);
  MLH_TRY(rb.alloc());
  MLH_TRY(rb.seed(tr, sum));
  fe* m = reinterpret_cast<fe*>(dev_matrix);
  fe* d = reinterpret_cast<fe*>(dev_delta);
  // rounds on tables > 2^tail entries: partial-sum kernels over HBM + the
  // one-lane round kernel; the last `tail` rounds in one LDS-resident launch
  const uint32_t tail = sumcheck_tail_rounds(L);
  uint32_t np = 0;
  if (L > tail)
    HIP_TRY(ctx, launch_sums(m, d, 1ull << (L - 1), ctx->partials, ctx->small, ctx->stream, &np));
  for (uint32_t k = 0; k + tail < L; ++k) {
    HIP_TRY(ctx, launch_sumcheck_round(ctx->partials, np, rb.prev(), rb.dt(), rb.poly(k), rb.r(k),
                                       ctx->stream));
    const uint64_t S = 1ull << (L - k);
    if (k + 1 + tail < L)  // the next round is not a tail round: fold + its sums
      HIP_TRY(ctx, launch_fold_sums(m, d, S, fe{}, ctx->partials, ctx->small, ctx->stream, rb.r(k),
                                    &np));
    else
      HIP_TRY(ctx, launch_fold(m, d, S, fe{}, ctx->stream, rb.r(k)));
  }
  HIP_TRY(ctx, launch_sumcheck_tail(m, d, tail, rb.prev(), rb.dt(), rb.poly(L - tail),
                                    rb.r(L - tail), ctx->stream));
  MLH_TRY(rb.read_back());
  MLH_TRY(rb.replay(tr));
  rb.copy_out(polys_out, rs_out);
  return MLH_OK;
}

// Sumcheck over SumcheckTables::build_tables_for_pcs (sumcheck.rs:128-145:
// matrix, delta = eq(points)) with delta kept factored while the tables are
// larger than 2^a entries (sumcheck.hip, "eq-factored rounds"): rounds
// k < B = L - a stream only the matrix and carry delta as c_k * eq(p_k..);
// folding round B-1 writes delta_B = c_B * eq(p_B..p_{L-1}) (2^a entries) and
// the remaining rounds run the two-table kernels on it.  Round polynomials,
// challenges and the folded matrix equal those of the materialised tables.
#ifndef MLH_TAIL_XC
#define MLH_TAIL_XC 1  // 0: the tail launch sums its group-A corners itself
#endif
#ifndef MLH_TAIL_RSUF
#define MLH_TAIL_RSUF 1  // 0: the tail launch computes its suffix products itself
#endif
struct EqSumcheck {
  static constexpr uint32_t kEqLo = 12;  // = sumcheck_tail_rounds' LDS limit
  mlh_ctx* ctx;
  const fe* src = nullptr;  // round 0's matrix (read only)
  fe* m = nullptr;          // the folded matrix (== src: folded in place)
  uint32_t L = 0, a = 0, B = 0;
  PoolBuf buf;
  fe *pts = nullptr, *c = nullptr, *lo = nullptr, *d = nullptr, *H = nullptr;
  fe* Hs = nullptr;  // eq suffix tables of the last a points (sumcheck_eq_tail_kernel)
  uint32_t* kw = nullptr;  // padding-block K + W tables per round (init with a transcript)
  fe* wts = nullptr;       // eq weights of the last finished group's challenges (its fold)
  uint32_t tail_xc_nb = 0; // head_rounds: the tail's group-A corner sums are in ctx->partials
  bool tail_tables = false; // Hs filled (init's want_tail)
  fe* rsuf = nullptr;       // the tail's suffix products (want_tail; eq_setup_kernel)
  PoolBuf yb;
  fe* Y = nullptr;   // head table (corner_sums): src's 2^B corner sums, folded in place
  fe* wf = nullptr;  // the two fold_head passes' weights
  explicit EqSumcheck(mlh_ctx* c_) : ctx(c_), buf(c_), yb(c_) {}

  // matrix: round 0's table; work (2^(L-1) entries, optional) receives the
  // folded table -- the first fold reads `matrix` and writes `work`, so the
  // caller's evaluations are never copied (build_tables_for_pcs's clone)
  // sha / sum / dt_out / prev_out (optional): also place the transcript state
  // and the claimed sum on the device in the same launch
  mlh_status init(const fe* matrix, fe* work, uint32_t L_, const uint8_t* host_points,
                  bool want_tail = false, const void* sha = nullptr, const uint8_t* sum = nullptr,
                  DevSha* dt_out = nullptr, fe* prev_out = nullptr) {
    src = matrix;
    m = work ? work : const_cast<fe*>(matrix);
    L = L_;
    tail_tables = want_tail;
    a = L < kEqLo ? L : kEqLo;
    B = L - a;
    // c | lo[2^a] | d[2^a] | H[2^B - 1] | Hs[2^a - 1] | pts[L] | kw[64 L words] | wts[64] |
    // rsuf[2 kEqTailRsuf] (tail, head)
    MLH_TRY(buf.alloc(16 * (1 + 3 * (1ull << a) + (1ull << B) + L + 16ull * L + 64 + 2 * kEqTailRsuf)));
    c = buf.as<fe>();
    lo = c + 1;
    d = B ? lo + (1ull << a) : lo;  // B == 0: delta is the whole eq table
    H = lo + 2 * (1ull << a);
    Hs = H + (1ull << B);
    pts = Hs + (1ull << a);
    kw = sha ? reinterpret_cast<uint32_t*>(pts + L) : nullptr;
    wts = pts + L + 16ull * L;
    rsuf = MLH_TAIL_RSUF && want_tail ? wts + 64 : nullptr;
    EqSetupArgs args{};
    if (L) memcpy(args.pts, host_points, 16ull * L);
    if (sha) memcpy(&args.sha, sha, sizeof(DevSha));
    if (sum) memcpy(&args.sum, sum, 16);
    args.L = L;
    args.B = B;
    HIP_TRY(ctx, launch_eq_setup(args, pts, c, lo, H, want_tail ? Hs : nullptr, dt_out, prev_out,
                                 ctx->stream, kw, rsuf));
    return MLH_OK;
  }
  const fe* Hk(uint32_t k) const { return H + ((1ull << B) - (1ull << (B - k))); }
  // the eq suffix table of tail round j (init's want_tail): 2^(a-j-1) entries
  const fe* Hsj(uint32_t j) const { return Hs + ((1ull << a) - (1ull << (a - j))); }

  // B <= 12: the B-variable corner sums of the table, one pass
  mlh_status corner_sums() {
    MLH_TRY(yb.alloc(16 * ((1ull << B) + 128)));
    Y = yb.as<fe>();
    wf = Y + (1ull << B);
    HIP_TRY(ctx, launch_corner_sums_lo(src, B, a, lo, Y, ctx->stream));
    return MLH_OK;
  }
  // The fold of the table over all B <= 12 head variables as two eq-weighted
  // passes, src -> m then m in place: JA = min(B, 6) variables with the weights
  // wf, JB = B - JA with wf + 64; rs: the B challenges.  xc: the last pass also
  // sums the tail's group-A corners (JN = 6 over its 2^12 outputs, e = Hs_5,
  // H = H_{B-1} = [1]), *nb partials per corner in ctx->partials.
  mlh_status fold_head(const fe* rs, bool xc, uint32_t* nb) {
    const uint32_t JA = B < 6 ? B : 6, JB = B - JA;
    const bool xa = xc && !JB;
    HIP_TRY(ctx, launch_fold_group_eq(src, 1ull << L, JA, xa ? 6 : 0, rs, wf, m,
                                      xa ? Hk(B - 1) : nullptr, xa ? Hsj(5) : lo, xa ? 6 : a,
                                      ctx->partials, ctx->stream, nb));
    if (JB)
      HIP_TRY(ctx, launch_fold_group_eq(m, 1ull << (L - JA), JB, xc ? 6 : 0, rs + JA, wf + 64, m,
                                        xc ? Hk(B - 1) : nullptr, xc ? Hsj(5) : lo, xc ? 6 : a,
                                        ctx->partials, ctx->stream, nb));
    return MLH_OK;
  }

  // Head rounds k < B go in groups of up to kGroup (sumcheck.hip, "grouped
  // eq-factored rounds"): one HBM pass yields the corner sums of a whole
  // group, the group's rounds run from them, and one pass folds the group's
  // variables and yields the next group's corner sums.  gk / gJ / gnb: the
  // current group's first round, size and partial block count.
  static constexpr uint32_t kGroup = 3;
  uint32_t gk = 0, gJ = 0, gnb = 0;
  uint32_t group_len(uint32_t k) const { return B - k < kGroup ? B - k : kGroup; }

  // round 0's sums (B > 0: the first group's corner sums) into ctx->partials
  mlh_status first_sums(uint32_t* np) {
    if (B) {
      gk = 0;
      gJ = group_len(0);
      HIP_TRY(ctx, launch_group_sums_eq(src, 1ull << L, gJ, Hk(gJ - 1), lo, a, ctx->partials,
                                        ctx->stream, &gnb));
      *np = gnb;
    } else {
      HIP_TRY(ctx, launch_sums(src, d, 1ull << (L - 1), ctx->partials, ctx->small, ctx->stream, np));
    }
    return MLH_OK;
  }
  // round k (r: its challenge slot; the slots of one group are contiguous)
  mlh_status round(uint32_t k, uint32_t np, fe* prev, DevSha* dt, fe* poly, fe* r) {
    if (k < B) {
      const uint32_t t = k - gk;
      HIP_TRY(ctx, launch_sumcheck_group(ctx->partials, gnb, gJ, 0, t, t + 1, prev, dt, poly, r - t,
                                         pts + gk, c, ctx->stream, coop_ctl(ctx), nullptr, wts));
    } else {
      HIP_TRY(ctx, launch_sumcheck_round(ctx->partials, np, prev, dt, poly, r, ctx->stream));
    }
    return MLH_OK;
  }
  // The head of a prove with no work between rounds (mlh_sumcheck_prove_eq):
  // passes of up to 6 rounds (two chained groups of <= 3 from one set of
  // corner sums), each folded in one HBM pass that also sums the next; the
  // last pass's fold leaves T_B (2^a entries) in m for the tail.
  mlh_status head_rounds(fe* prev, DevSha* dt, fe* polys, fe* rs) {
    if (!B) return MLH_OK;
    if (B <= kEqLo && a == kEqLo && B >= 2) {
      // B <= 12: one pass for the B-variable corner sums Y, all B rounds in one
      // launch on Y (two corner groups), then the B-variable fold of the table
      // as two eq-weighted passes (sumcheck.hip "grouped eq-factored rounds")
      const uint32_t JA = B < 6 ? B : 6;
      MLH_TRY(corner_sums());
      HIP_TRY(ctx, launch_sumcheck_eq_head(Y, B, Hk(JA - 1), pts, c, prev, dt, polys, rs, wf,
                                           ctx->stream, coop_ctl(ctx), kw,
                                           rsuf ? rsuf + kEqTailRsuf : nullptr));
      // the last fold also sums the tail's group-A corners: the tail launch
      // then skips that phase of its prologue (tail_xc_nb partials per corner
      // in ctx->partials; tail launch 59.3 -> 56.5 us, the fold +1 us)
      const bool xc = MLH_TAIL_XC && tail_tables;
      uint32_t nb = 0;
      MLH_TRY(fold_head(rs, xc, &nb));
      tail_xc_nb = xc ? nb : 0;
      return MLH_OK;
    }
    uint32_t nb = 0, k = 0, JT = B < kMaxGroup ? B : kMaxGroup;
    HIP_TRY(ctx, launch_group_sums_eq(src, 1ull << L, JT, Hk(JT - 1), lo, a, ctx->partials,
                                      ctx->stream, &nb));
    for (;;) {
      const uint32_t J1 = JT < 3 ? JT : 3;
      HIP_TRY(ctx, launch_sumcheck_group(ctx->partials, nb, J1, JT - J1, 0, J1, prev, dt,
                                         polys + 2 * k, rs + k, pts + k, c, ctx->stream,
                                         coop_ctl(ctx), kw ? kw + 64 * k : nullptr, wts));
      const fe* in = k == 0 ? src : m;
      const uint64_t S = 1ull << (L - k);
      k += JT;
      const uint32_t JN = B - k < kMaxGroup ? B - k : kMaxGroup;
      HIP_TRY(ctx, launch_fold_group_eq(in, S, JT, JN, rs + k - JT, wts, m,
                                        JN ? Hk(k + JN - 1) : nullptr, lo, a, ctx->partials,
                                        ctx->stream, &nb));
      if (!JN) return MLH_OK;
      JT = JN;
    }
  }
  // after round k's challenge (r_dev): fold what is due (HBM) with round k+1's
  // sums.  A head group folds once, after its last round.  (The tail's fold on
  // a second stream beside the FRI fold_step, which needs the same r, measured
  // no faster: the tree tail it would fill is a handful of waves, and the
  // cross-stream events cost about what it saved.)
  mlh_status fold(uint32_t k, const fe* r_dev, uint32_t* np) {
    const uint64_t S = 1ull << (L - k);
    if (k < B) {
      if (k + 1 < gk + gJ) return MLH_OK;  // mid-group: nothing to fold yet
      const fe* in = gk == 0 ? src : m;
      const uint32_t JN = group_len(k + 1);
      HIP_TRY(ctx, launch_fold_group_eq(in, 1ull << (L - gk), gJ, JN, r_dev - (gJ - 1), wts, m,
                                        JN ? Hk(k + JN) : nullptr, lo, a, ctx->partials,
                                        ctx->stream, &gnb));
      if (JN) {
        gk = k + 1;
        gJ = JN;
        *np = gnb;
        return MLH_OK;
      }
      HIP_TRY(ctx, launch_scale_dev(lo, c, 1ull << a, d, ctx->stream));
      HIP_TRY(ctx, launch_sums(m, d, 1ull << (a - 1), ctx->partials, ctx->small, ctx->stream, np));
    } else if (S >= 4) {  // B == 0: the first fold reads src
      HIP_TRY(ctx, launch_fold_sums(m, d, S, fe{}, ctx->partials, ctx->small, ctx->stream, r_dev, np,
                                    k == 0 ? src : m));
    } else {
      HIP_TRY(ctx, launch_fold(m, d, S, fe{}, ctx->stream, r_dev, k == 0 ? src : m));
    }
    return MLH_OK;
  }
};

mlh_status mlh_sumcheck_prove_eq(mlh_ctx* ctx, const void* dev_evals, void* dev_work,
                                 uint32_t log_height, const uint8_t* host_points,
                                 const uint8_t sum[16], mlh_transcript* tr, uint8_t* polys_out,
                                 uint8_t* rs_out, uint8_t* delta_out) {
  if (!ctx || !dev_evals || !host_points || !sum || !tr || log_height < 1 || log_height > 40)
    return fail(ctx, MLH_ERR_INVALID, "bad argument");
  const uint32_t L = log_height;
  RoundBuf rb(ctx, 2, L);
  MLH_TRY(rb.alloc(16));
  fe* dfin = rb.extra();  // the final delta
  EqSumcheck es(ctx);  // its setup launch also places the transcript state and the claim
  device_arm(ctx);
  MLH_TRY(es.init(reinterpret_cast<const fe*>(dev_evals), reinterpret_cast<fe*>(dev_work), L,
                  host_points, true, &tr->sha, sum, rb.dt(), rb.prev()));
  // head rounds stream only the matrix (passes of up to 6 rounds); the last a
  // rounds run in the LDS-resident eq tail on the 2^a-entry folded table
  MLH_TRY(es.head_rounds(rb.prev(), rb.dt(), rb.poly(0), rb.r(0)));
  HIP_TRY(ctx, launch_sumcheck_eq_tail(es.B ? es.m : es.src, 0, nullptr, es.a, es.Hs,
                                       es.pts + es.B, es.c, rb.prev(), rb.dt(), rb.poly(es.B),
                                       rb.r(es.B), es.m, dfin, ctx->stream, coop_ctl(ctx),
                                       es.kw ? es.kw + 64 * es.B : nullptr,
                                       HostOut{reinterpret_cast<const uint8_t*>(rb.poly(0)), ctx->pinned,
                                               (uint32_t)(48ull * L + 16)},
                                       es.tail_xc_nb ? ctx->partials : nullptr, es.tail_xc_nb,
                                       es.rsuf));
  HIP_TRY(ctx, prove_wait(ctx));
  MLH_TRY(device_check(ctx));
  rb.from_pinned(16);  // the tail kernel copied polys | rs | final delta back
  MLH_TRY(rb.replay(tr));
  rb.copy_out(polys_out, rs_out);
  if (delta_out) memcpy(delta_out, rb.host.data() + rb.out_bytes(), 16);
  return MLH_OK;
}

// PCSProverData::fold (multilinear_pcs.rs:43-76) for n_vars <= 24, with the
// sumcheck off the transcript chain (sumcheck.hip "PCS rounds off the
// transcript kernel"): round k's (c1, c2) come from a one-workgroup job on
// the eq-factored table once r_{k-1} exists -- an extra workgroup of FRI step
// k-1's fold launch -- and the launch that writes FRI root k absorbs root k,
// then (c1, c2)_k, and draws r_k: the transcript order of the reference
// (root_k | c1_k | c2_k -> r_k), with no sumcheck launch between challenges.
// Head (the first B = n - 12 variables): the 2^B corner sums of the 2^n table
// in one pass; after r_{B-1} two fold_group_eq passes fold the table to the
// 2^12 entries the tail rounds use.  Shared by the PCS and the batched PCS.
struct PcsRounds {
  mlh_ctx* ctx;
  FriDevLoop& lp;
  EqSumcheck es;  // src: the evaluations; m: the folded table (may be the same buffer)
  PcsRoundState* st = nullptr;
  PcsRounds(mlh_ctx* c, FriDevLoop& l) : ctx(c), lp(l), es(c) {}

  // after lp.layout(.., >= 5 extra slots): tables, round state (claim =
  // claim_host, or claim_dev copied on the device), round 0's polynomial
  mlh_status init(const fe* evals, fe* work, uint32_t n, const uint8_t* host_inputs,
                  const uint8_t* claim_host, const fe* claim_dev) {
    MLH_TRY(es.init(evals, work, n, host_inputs, /*want_tail=*/true));
    const uint32_t B = es.B;
    uint8_t init_state[80] = {};  // (claim, c = 1, e0 = c1 = c2 = 0)
    if (claim_host) memcpy(init_state, claim_host, 16);
    init_state[16] = 1;
    memcpy(ctx->pinned + kPinSlotA, init_state, 80);
    st = reinterpret_cast<PcsRoundState*>(lp.extra());
    HIP_TRY(ctx, hipMemcpyAsync(st, ctx->pinned + kPinSlotA, 80, hipMemcpyHostToDevice, ctx->stream));
    if (claim_dev)
      HIP_TRY(ctx, hipMemcpyAsync(&st->claim, claim_dev, 16, hipMemcpyDeviceToDevice, ctx->stream));
    if (B) MLH_TRY(es.corner_sums());  // the head rounds run on Y
    HIP_TRY(ctx, launch_pcs_round(B ? es.Y : evals, B ? es.Y : work, B ? B : n, false, nullptr, nullptr,
                                  es.pts, e_of(0), st, lp.poly(0), ctx->stream));
    return MLH_OK;
  }
  // e of round k: H_k (head) or Hs_{k-B} (tail); 2^(h-1) entries for a table of 2^h
  const fe* e_of(uint32_t k) const { return k < es.B ? es.Hk(k) : es.Hsj(k - es.B); }
  // round kn (>= 1) as a job; at kn == B the table fold over the head
  // variables is enqueued first (it needs r_0..r_{B-1})
  mlh_status job(uint32_t kn, PcsJob* out) {
    const uint32_t k = kn - 1, B = es.B;
    PcsJob j{nullptr, es.m, 0, 1, lp.r(k), es.pts + k, es.pts + kn, e_of(kn), st, lp.poly(kn)};
    if (kn < B) {  // head: fold Y with r_k
      j.src = es.Y;
      j.dst = es.Y;
      j.log_h = B - kn;
    } else if (kn == B) {  // fold the table over the B head variables; round B on it
      const uint32_t JA = B < 6 ? B : 6;
      uint32_t nb = 0;
      HIP_TRY(ctx, launch_eq_weights(lp.r(0), JA, B - JA, es.wf, ctx->stream));
      MLH_TRY(es.fold_head(lp.r(0), /*xc=*/false, &nb));
      j.src = es.m;
      j.log_h = es.a;
      j.fold = 0;
    } else {  // tail: fold with r_k (the first tail fold of B = 0 reads the evaluations)
      j.src = (B == 0 && kn == 1) ? es.src : es.m;
      j.log_h = es.L - kn;
    }
    *out = j;
    return MLH_OK;
  }
  // The fused rounds, after round 0's polynomial and the absorb that draws r_0:
  // FRI step k carries round k + 1 as a job of its fold launch.  batched: step 0
  // is the batched fold, which takes no job -- round 1 is its own launch before it.
  mlh_status rounds(bool batched) {
    for (uint32_t k = 0; k < es.L; ++k) {
      const uint32_t kn = k + 1;  // the round whose polynomial follows r_k
      const bool more = kn < es.L;
      PcsJob job{};
      if (more) MLH_TRY(this->job(kn, &job));
      if (batched && k == 0) {
        if (more)
          HIP_TRY(ctx, launch_pcs_round(job.src, job.dst, job.log_h, job.fold != 0, job.r_prev, job.p_prev,
                                        job.p_k, job.e, job.st, job.poly_out, ctx->stream));
        MLH_TRY(lp.step_batched(lp.r(0), more, more ? lp.poly(1) : nullptr));
      } else {
        MLH_TRY(lp.step(k, lp.r(k), more, more ? lp.poly(kn) : nullptr, more ? &job : nullptr));
      }
    }
    return MLH_OK;
  }
};

// The cooperative rounds (n_vars above the context's pcs_fused_max), the claim
// at lp.prev(): round k's kernel absorbs (c1, c2) and draws r_k, which the
// sumcheck fold and FRI step k read from HBM.  batched: as above.
static mlh_status pcs_rounds_coop(EqSumcheck& es, FriDevLoop& lp, bool batched) {
  uint32_t np = 0;
  MLH_TRY(es.first_sums(&np));
  for (uint32_t k = 0; k < es.L; ++k) {
    MLH_TRY(es.round(k, np, lp.prev(), lp.dt(), lp.poly(k), lp.r(k)));
    MLH_TRY(es.fold(k, lp.r(k), &np));
    if (batched && k == 0)
      MLH_TRY(lp.step_batched(lp.r(0), false));
    else
      MLH_TRY(lp.step(k, lp.r(k), false));
  }
  return MLH_OK;
}

// Host replay of the rounds, after lp.finish: per round (c1, c2), expect r_k,
// then the root of layer layer0 + k, or the last element past the layers.
// polys_out (optional) receives the round polynomials.
static void pcs_replay_rounds(ReplayCheck& rc, const FriDevLoop& lp, uint32_t n_vars,
                              uint32_t layer0, void* polys_out) {
  const mlh_fri_prover& fp = *lp.p;
  if (polys_out) memcpy(polys_out, lp.host_polys(), 32ull * n_vars);
  for (uint32_t k = 0; k < n_vars; ++k) {
    rc.absorb(lp.host_polys() + 32 * k, 32);
    rc.expect(lp.host_r(k));
    if (layer0 + k < fp.layers.size())
      rc.absorb(fp.layers[layer0 + k].root, 32);
    else
      rc.absorb(fp.last, 16);
  }
}

mlh_status mlh_pcs_prove(mlh_ctx* ctx, const void* dev_evals, uint32_t n_vars,
                         const uint8_t* host_inputs, const uint8_t output[16], mlh_transcript* tr,
                         mlh_pcs_proof* proof) {
  if (!ctx || !dev_evals || !output || !tr || !proof || (n_vars && !host_inputs))
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (n_vars < 1 || n_vars > 36) return fail(ctx, MLH_ERR_INVALID, "n_vars out of range");
  const uint32_t log_domain = n_vars + MLH_LOG_BLOWUP;
  const uint64_t n = 1ull << n_vars;
  const fe* evals = reinterpret_cast<const fe*>(dev_evals);
  PoolBuf code(ctx), matrix(ctx);
  MLH_TRY(code.alloc(2 * n * 16));
  MLH_TRY(matrix.alloc(n / 2 * 16));  // the folded table (the first fold reads dev_evals)
  // to_coefficient (:102), bit reverse (:104), reed_solomon (:107)
  MLH_TRY(batched_pcs_codes(ctx, dev_evals, 1, n_vars, code.as<fe>()));
  // PCSProverData::init (:28-42) + fold loop (:57-75), transcript on the device
  mlh_fri_prover fp(ctx, log_domain);
  FriDevLoop lp(ctx, &fp);
  device_arm(ctx);
  if (n_vars <= ctx->pcs_fused_max) {
    MLH_TRY(lp.layout(log_domain, tr, 5));
    PcsRounds pr(ctx, lp);
    MLH_TRY(pr.init(evals, matrix.as<fe>(), n_vars, host_inputs, output, nullptr));
    // FRI init: root 0 | (c1, c2)_0 -> r_0
    MLH_TRY(lp.init(code.p, log_domain, true, lp.poly(0)));
    MLH_TRY(pr.rounds(false));
  } else {
    MLH_TRY(lp.layout(log_domain, tr));
    MLH_TRY(lp.init(code.p, log_domain, false));
    EqSumcheck es(ctx);  // delta = eq(inputs), factored (build_tables_for_pcs)
    MLH_TRY(es.init(evals, matrix.as<fe>(), n_vars, host_inputs));
    memcpy(ctx->pinned + kPinSlotA, output, 16);
    HIP_TRY(ctx, hipMemcpyAsync(lp.prev(), ctx->pinned + kPinSlotA, 16, hipMemcpyHostToDevice,
                                ctx->stream));
    MLH_TRY(pcs_rounds_coop(es, lp, false));
  }
  MLH_TRY(lp.finish(32ull * n_vars));
  // host transcript replay (armed only now: an error above leaves the transcript
  // untouched): root_0, then per round (c1, c2), root_{k+1} / last
  ReplayCheck rc(ctx, tr);
  rc.absorb(fp.layers[0].root, 32);
  pcs_replay_rounds(rc, lp, n_vars, 1, proof->sumcheck_polys);
  MLH_TRY(rc.status());
  return fri_queries(ctx, &fp, tr, &proof->fri);
}

mlh_status mlh_batched_pcs_prove(mlh_ctx* ctx, const void* dev_evals, uint32_t num_polys,
                                 uint32_t n_vars, const uint8_t* inputs, const uint8_t* outputs,
                                 mlh_transcript* tr, mlh_batched_pcs_proof* proof) {
  if (!ctx || !dev_evals || !inputs || !outputs || !tr || !proof)
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (num_polys == 0) return fail(ctx, MLH_ERR_INVALID, "no polynomials");
  if (n_vars < 1 || n_vars > 36) return fail(ctx, MLH_ERR_INVALID, "n_vars out of range");
  PoolBuf codes(ctx);
  MLH_TRY(codes.alloc(((uint64_t)num_polys << (n_vars + MLH_LOG_BLOWUP)) * 16));
  MLH_TRY(batched_pcs_codes(ctx, dev_evals, num_polys, n_vars, codes.as<fe>()));
  return batched_pcs_open(ctx, codes.as<fe>(), dev_evals, nullptr, num_polys, n_vars, inputs,
                          outputs, tr, proof);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// batched PCS (batched_pcs.rs; the batched FRI under it: fri_prover.hip)
// ---------------------------------------------------------------------------
mlh_status batched_pcs_open(mlh_ctx* ctx, const fe* dev_codes, const void* dev_evals,
                            const uint8_t* built_tree, uint32_t num_polys, uint32_t n_vars,
                            const uint8_t* inputs, const uint8_t* outputs, mlh_transcript* tr,
                            mlh_batched_pcs_proof* proof) {
  const uint32_t log_domain = n_vars + MLH_LOG_BLOWUP;
  const uint64_t n = 1ull << n_vars;
  PoolBuf matrix(ctx), outs(ctx);
  MLH_TRY(matrix.alloc(n * 16));
  MLH_TRY(outs.alloc(16ull * num_polys));
  // init (batched_pcs.rs:36-78): absorb the claim, batched FRI init.  The
  // replay check is armed first: any failure from here on restores the
  // caller's transcript to its state at entry.
  ReplayCheck rc(ctx, tr);
  for (uint32_t i = 0; i < n_vars; ++i) rc.absorb(inputs + 16 * i, 16);
  for (uint32_t j = 0; j < num_polys; ++j) rc.absorb(outputs + 16 * j, 16);
  mlh_fri_prover fp(ctx, log_domain);
  FriDevLoop lp(ctx, &fp);
  device_arm(ctx);
  const bool fused = n_vars <= ctx->pcs_fused_max;
  MLH_TRY(lp.init_batched(dev_codes, num_polys, log_domain, tr, false, fused ? 5 : 0, built_tree));
  // fingerprinted MLE + eq table; previous_sum = fingerprint(fr, outputs)
  fe* mt = matrix.as<fe>();
  HIP_TRY(ctx, launch_fingerprint(reinterpret_cast<const fe*>(dev_evals), num_polys, n, lp.fr(), mt,
                                  ctx->stream));
  {
    std::vector<uint8_t> ob(outputs, outputs + 16ull * num_polys);
    HIP_TRY(ctx, hipMemcpyAsync(outs.p, ob.data(), ob.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // ob is pageable and goes out of scope
  }
  HIP_TRY(ctx, launch_fingerprint_scalar(outs.as<fe>(), num_polys, lp.fr(), lp.prev(), ctx->stream));
  if (fused) {  // (batched_pcs.rs:80-125) the PCS rounds off the transcript chain (PcsRounds)
    PcsRounds pr(ctx, lp);  // the fingerprinted table is ours: its folds run in place
    MLH_TRY(pr.init(mt, mt, n_vars, inputs, nullptr, lp.prev()));
    HIP_TRY(ctx, launch_transcript_absorb(lp.dt(), reinterpret_cast<const uint8_t*>(lp.poly(0)), 32,
                                          lp.r(0), ctx->stream));  // (c1, c2)_0 -> r_0
    MLH_TRY(pr.rounds(true));
  } else {
    EqSumcheck es(ctx);  // delta = eq(inputs), factored
    MLH_TRY(es.init(mt, nullptr, n_vars, inputs));
    MLH_TRY(pcs_rounds_coop(es, lp, true));
  }
  MLH_TRY(lp.finish(32ull * n_vars));
  // host transcript replay
  rc.absorb(lp.host_broot(), 32);
  rc.expect(lp.host_fr());
  rc.absorb(lp.host_fr(), 16);
  pcs_replay_rounds(rc, lp, n_vars, 0, proof->sumcheck_polys);
  MLH_TRY(rc.status());
  memcpy(proof->fri.batch_commitment, lp.host_broot(), 32);
  return batched_queries(ctx, lp, tr, &proof->fri);
}
