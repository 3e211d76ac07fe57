/*
 * mlhip.h -- C ABI of the MI355X (gfx950) proving backend for the hot path of
 * fr34za/multilinear (reference @ 2025-06-20): radix-2 NTT, Reed-Solomon LDE,
 * SHA-256 Merkle level hashing, FRI layer folding, and MLE/sumcheck round
 * sums over the field.rs prime M = 2^128 - 45*2^40 + 1.
 *
 * Conventions (identical to the reference's in-memory forms):
 *   - a field element is 16 bytes: the canonical u128 (value < M), little
 *     endian -- Field128::as_ref (src/field.rs:33-38);
 *   - a digest is the 32 SHA-256 output bytes (HashDigest, merkle_tree/mod.rs:5);
 *   - a Merkle tree of L = 2^l leaves is one buffer of 2L-1 digests in level
 *     order (leaves first, root last) -- Merkle::layers flattened
 *     (merkle_tree/mod.rs:7-11);
 *   - "dev" pointers are device (HBM) pointers on the context's device, e.g.
 *     from mlh_malloc or any HIP allocator; "host" pointers are host memory.
 *   - Device pointers to field elements and digests must be 16-byte aligned;
 *     nothing more is assumed, so a caller may pass interior pointers of an
 *     arena of its own.  A call reads and writes only the byte ranges its
 *     comment gives.
 *   - All work is enqueued on the context's HIP stream; functions that return
 *     host results (roots, sums, proofs) synchronise that stream.
 *
 * Errors: the reference prover panics (assert!) on non-power-of-two sizes,
 * bad lengths and the "not an RS code" check; here every entry point returns
 * an mlh_status and mlh_last_error() gives the message.  Nothing falls back
 * to a CPU implementation: without a usable gfx950 device every compute call
 * returns MLH_ERR_HIP.
 */
#ifndef MLHIP_H
#define MLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mlh_status {
  MLH_OK = 0,
  MLH_ERR_INVALID = 1,       /* bad argument (null pointer, size out of range)   */
  MLH_ERR_NOT_POW2 = 2,      /* "must be a power of two" asserts                   */
  MLH_ERR_BAD_GENERATOR = 3, /* generator not canonical, or (FRI / sharded entry
                                points) not of order exactly 2^log_n              */
  MLH_ERR_HIP = 4,           /* HIP runtime error / no device                      */
  MLH_ERR_OOM = 5,           /* device allocation failed                           */
  MLH_ERR_NOT_RS_CODE = 6,   /* fri/mod.rs:119-122 "not an RS code"                */
  MLH_ERR_VERIFY = 7,        /* verifier rejected (Merkle: IncompatibleHash)       */
  MLH_ERR_VERIFY_INDEX = 8,  /* Merkle path directions != index (IncompatibleIndex) */
  MLH_ERR_COMM = 9,          /* a collective of the multi-GPU transport failed      */
  MLH_ERR_DEVICE = 10        /* device-side failure inside a prove: a cooperative
                                kernel's wait timed out, or a challenge the device
                                drew differs from the host transcript replay; the
                                outputs of that call are invalid and the caller's
                                transcript is left as it was at the call's entry */
} mlh_status;

typedef struct mlh_ctx mlh_ctx;               /* device + stream + twiddle caches */
typedef struct mlh_transcript mlh_transcript; /* transcript.rs Transcript         */
typedef struct mlh_fri_prover mlh_fri_prover; /* fri/mod.rs FriProverData         */

#define MLH_LOG_BLOWUP 1   /* fri/mod.rs:16 */
#define MLH_NUM_QUERIES 128 /* fri/mod.rs:17 */

/* ---- context and memory ------------------------------------------------- */
const char* mlh_version(void);
mlh_status mlh_context_create(int device, void* hip_stream, mlh_ctx** out);
void mlh_context_destroy(mlh_ctx* ctx);
/* Twiddle / fold tables are cached per context (built on the first use of a
 * size and generator) in a bounded LRU cache: default limit 1 GiB; tables the
 * running operation uses are never evicted, so the cache may exceed a very
 * small limit by that operation's tables.  limit 0 frees every table not in
 * use at the next opportunity.  The largest: an FRI prove of a codeword of
 * 2^L <= 2^25 elements caches every fold layer's twiddles in one table of
 * 2^L - 1 entries (512 MiB at 2^25); above 2^25 the folds form them from two
 * 4096-entry tables instead.  A 2^23 or 2^24 NTT's first pass adds a 64 x 2^16
 * progression table and its 2^16-entry step table (68 MiB at 2^24). */
mlh_status mlh_set_table_cache_limit(mlh_ctx* ctx, uint64_t bytes);
uint64_t mlh_table_cache_bytes(const mlh_ctx* ctx);
/* Test/tuning hook: force the NTT radix plan of this context (count digits
 * 4..9; a plan applies to the transforms whose log size equals its digit sum;
 * count = 0 restores the default plan). */
mlh_status mlh_set_ntt_plan(mlh_ctx* ctx, const uint32_t* logr, uint32_t count);
/* Test hook: the cooperative sumcheck kernels' wait limit, in s_sleep(1)
 * periods (0 restores the default 2^22).  A wait that exceeds it abandons the
 * kernel's rounds and the prove returns MLH_ERR_DEVICE. */
mlh_status mlh_set_coop_spin_limit(mlh_ctx* ctx, uint32_t sleeps);
/* Test hook: the PCS and batched PCS provers compute their sumcheck rounds
 * off the transcript chain for n_vars <= max_vars (default and cap 24) and
 * with one cooperative launch per round above it; both give the same proof. */
mlh_status mlh_set_pcs_fused_max(mlh_ctx* ctx, uint32_t max_vars);
/* Binds the context to another HIP stream.  Work the context enqueued before
 * the switch is ordered before work it enqueues after it, on the device and
 * without a host wait: the new stream waits for an event recorded on the old
 * one.  So the caller need not synchronise around a switch -- the context's
 * pooled scratch, its cached tables (which may still be being built) and a
 * cache eviction's drain stay correct across it.  Passing the stream the
 * context already has does nothing.  The stream being left must still exist
 * (MLH_ERR_HIP otherwise; the context is bound to the new stream even then,
 * but unordered).  Not promised: concurrent use of one
 * context from two streams (or two threads); work the caller itself enqueues
 * on either stream is ordered only by the caller.  Use one context per
 * stream for independent work. */
mlh_status mlh_set_stream(mlh_ctx* ctx, void* hip_stream);
/* Test hook: while word != 0, every scratch buffer the library hands to its
 * own kernels is first filled with `word` (as 32-bit words) on the context's
 * stream: each block of the device memory pool when it is given out, each new
 * cache table before its build kernel, the NTT ping-pong buffer when it is
 * (re)allocated.  The call itself fills the context's fixed scratch (reduction
 * partials, the 64-element scratch, the current NTT buffer) on the stream and,
 * after synchronising the stream, the pinned staging buffers on the host.  A
 * kernel that reads a scratch word it never wrote then computes with `word`
 * instead of a stale, plausible value.  0 (the default) turns it off; off, it
 * costs nothing. */
mlh_status mlh_set_scratch_poison(mlh_ctx* ctx, uint32_t word);
mlh_status mlh_synchronize(mlh_ctx* ctx);
/* The message of ctx's last failure; with ctx == NULL, why this thread's last
 * mlh_context_create failed. */
const char* mlh_last_error(const mlh_ctx* ctx);
mlh_status mlh_malloc(mlh_ctx* ctx, size_t bytes, void** dev);
mlh_status mlh_free(mlh_ctx* ctx, void* dev);
mlh_status mlh_memcpy_h2d(mlh_ctx* ctx, void* dev, const void* host, size_t bytes);
mlh_status mlh_memcpy_d2h(mlh_ctx* ctx, void* host, const void* dev, size_t bytes);
mlh_status mlh_memcpy_d2d(mlh_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ---- field helpers (host) ------------------------------------------------ */
/* NttField::pow_2_generator (src/ntt/mod.rs:42-54): 3^((M-1)/2^log_size). */
mlh_status mlh_pow_2_generator(uint32_t log_size, uint8_t gen_out[16]);
/* NttField::pow_2_generator_powers (src/ntt/mod.rs:18-28): out[i] = g^i,
 * i < 2^log_size, written to dev (no serial chain on the device). */
mlh_status mlh_pow_2_generator_powers(mlh_ctx* ctx, uint32_t log_size, void* dev_out);

/* Elementwise Field128 ops on device vectors of n elements (src/field.rs:66-111:
 * Add, Sub, Mul, Neg).  Inputs canonical; out may alias an input. */
mlh_status mlh_field_add(mlh_ctx* ctx, const void* dev_a, const void* dev_b, void* dev_out, uint64_t n);
mlh_status mlh_field_sub(mlh_ctx* ctx, const void* dev_a, const void* dev_b, void* dev_out, uint64_t n);
mlh_status mlh_field_mul(mlh_ctx* ctx, const void* dev_a, const void* dev_b, void* dev_out, uint64_t n);
mlh_status mlh_field_neg(mlh_ctx* ctx, const void* dev_a, void* dev_out, uint64_t n);
/* out[i] = a[i] * c (scalar Mul, field.rs:98-106); c canonical LE16. */
mlh_status mlh_field_scale(mlh_ctx* ctx, const void* dev_a, const uint8_t c[16], void* dev_out,
                           uint64_t n);
/* out[i] = a[i]^(M - 2): the inverse, zero -> zero, as Field128's Div through
 * winter-math's inv (field.rs:113-118).  n = 0 is MLH_OK and does nothing;
 * dev_out == dev_a (in place) is allowed, any other overlap is
 * MLH_ERR_INVALID.  One power per thread over several elements (Montgomery's
 * trick): about 3 + 138 / K products per element.  One launch. */
mlh_status mlh_field_inv(mlh_ctx* ctx, const void* dev_a, void* dev_out, uint64_t n);

/* ---- NTT (src/ntt/mod.rs) ------------------------------------------------ */
/* Polynomial::ntt (ntt/mod.rs:69-110): evals[i] = sum_j coeffs[j] gen^(ij),
 * natural order in and out, when gen has order exactly 2^log_n (the fast
 * passes).  Any other canonical gen (0 included) gets the reference's own
 * bit-reverse + radix-2 network output -- well defined but not a DFT -- from a
 * stage-by-stage path (log_n + 1 - 11 launches; a correctness path, not tuned).
 * In-place (dev_in == dev_out) is allowed. */
mlh_status mlh_ntt(mlh_ctx* ctx, const void* dev_coeffs, void* dev_evals, uint32_t log_n,
                   const uint8_t gen[16]);
/* LagrangePolynomial::intt (ntt/mod.rs:132-173): gen is the forward
 * generator (LagrangePolynomial::gen); uses gen^-1 (0 for gen = 0, as
 * winter-math's inverse) and scales by 1/n.  Generators as mlh_ntt. */
mlh_status mlh_intt(mlh_ctx* ctx, const void* dev_evals, void* dev_coeffs, uint32_t log_n,
                    const uint8_t gen[16]);
/* mlh_ntt on 2^log_batch vectors of 2^log_n elements each, stored one after
 * the other, in one launch per pass (gen of order exactly 2^log_n;
 * log_n + log_batch <= 32).  In-place is allowed. */
mlh_status mlh_ntt_batch(mlh_ctx* ctx, const void* dev_coeffs, void* dev_evals, uint32_t log_n,
                         const uint8_t gen[16], uint32_t log_batch);
/* bit_reverse_permutation (ntt/mod.rs:113-123), out of place (in != out);
 * log_n >= 1 (n = 1 panics in the reference: MLH_ERR_NOT_POW2). */
mlh_status mlh_bit_reverse_permutation(mlh_ctx* ctx, const void* dev_in, void* dev_out,
                                       uint32_t log_n);
/* Vec -> Vec convenience (host buffers, includes PCIe copies). */
mlh_status mlh_ntt_host(mlh_ctx* ctx, const uint8_t* host_in, uint8_t* host_out, uint32_t log_n,
                        const uint8_t gen[16], int inverse);

/* ---- Reed-Solomon, Merkle, FRI (src/fri, src/merkle_tree) -------------------- */
/* reed_solomon (fri/mod.rs:19-28): zero-pad 2^log_n coeffs to 2^(log_n+1) and
 * NTT with gen (order 2^(log_n+1); any other canonical gen as mlh_ntt).
 * dev_code holds 2^(log_n+1) elements. */
mlh_status mlh_reed_solomon(mlh_ctx* ctx, const void* dev_coeffs, uint32_t log_n,
                            const uint8_t gen[16], void* dev_code);
/* reed_solomon(bit_reverse_permutation(coeffs)) in one transform: the commit
 * step of multilinear_pcs.rs:104-107 / batched_pcs.rs:146-147 with the
 * permutation folded into the first pass's loads (out of place). */
mlh_status mlh_reed_solomon_brev(mlh_ctx* ctx, const void* dev_coeffs, uint32_t log_n,
                                 const uint8_t gen[16], void* dev_code);
/* Bytes of a flattened tree with `leaves` leaves: (2*leaves - 1) * 32. */
uint64_t mlh_merkle_layers_bytes(uint64_t leaves);
/* commit_rs_code (fri/mod.rs:45-55) + Merkle::commit (merkle_tree/mod.rs:65-85):
 * leaf i = SHA256(LE16(code[i]) ‖ LE16(code[i + n/2])), n = 2^log_code. */
mlh_status mlh_merkle_commit_pairs(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                                   void* dev_layers, uint8_t root_out[32]);
/* Merkle::commit over `count` (power of two) items of item_len bytes each. */
mlh_status mlh_merkle_commit(mlh_ctx* ctx, const void* dev_items, uint64_t item_len,
                             uint64_t count, void* dev_layers, uint8_t root_out[32]);
/* Merkle::batch_commit (merkle_tree/mod.rs:92-131): m batches of `count`
 * items, batch j at dev_items + j*count*item_len; leaf i hashes the m items i. */
mlh_status mlh_merkle_batch_commit(mlh_ctx* ctx, const void* dev_items, uint64_t item_len,
                                   uint32_t m, uint64_t count, void* dev_layers,
                                   uint8_t root_out[32]);
/* The fold loop of FriProverData::fold_step (fri/mod.rs:89-114): layer of
 * 2^log_layer values (pairs i, i + n/2) -> 2^(log_layer-1) values, fold index
 * k, original domain 2^log_domain (twiddle g^(-i 2^k)). */
mlh_status mlh_fri_fold(mlh_ctx* ctx, const void* dev_layer, uint32_t log_layer, uint32_t k,
                        uint32_t log_domain, const uint8_t r[16], void* dev_next);

/* FriProverData (fri/mod.rs:10-175), device resident.
 * gen_pows: the reference's FriProverData::{init,fold} and FriProof::prove
 * take the table gen_pows and fold with twiddle gen_pows[gen_pows.len() - i 2^k]
 * (fri/mod.rs:106-110).  The plain entry points assume the canonical table of
 * the code's own length (pow_2_generator_powers(log_code), what every reference
 * caller passes); the _gp variants take the table as (gen_pows[1],
 * log2(gen_pows.len())) for any geometric table of a generator of order exactly
 * gen_pows.len() (MLH_ERR_BAD_GENERATOR otherwise; MLH_ERR_INVALID when the
 * table is shorter than half the code, where the reference's index underflows). */
/* The shim from the reference's gen_pows: &[F] (fri/mod.rs:79, :136, :261) to
 * the _gp arguments: returns (g = gen_pows[1], log2(len)) after checking, on
 * the host, that len is a power of two >= 2, g has order exactly len, and the
 * table agrees with 1, g, g^2, ... at every index < min(len, 4096), at every
 * 2^j, at len/2 (= -1), at len-1 (= g^-1) and at 16 pseudo-random indices
 * (MLH_ERR_INVALID otherwise).  That is a spot check: a table altered only
 * elsewhere passes it, and the library would then fold with the true powers
 * where the reference folds with the altered entry (fri/mod.rs:110).  The full
 * check is mlh_gen_pows_verify. */
mlh_status mlh_gen_pows_params(const uint8_t* gen_pows, uint64_t len, uint8_t gen_out[16],
                               uint32_t* log_len_out);
/* Full check of a host gen_pows table: every entry against g^i on the device
 * (one pass of the table over PCIe, ~16 B per entry, plus one comparison
 * kernel), after mlh_gen_pows_params' checks.  MLH_OK iff the table IS the
 * power series of gen_pows[1] (of order len); otherwise MLH_ERR_INVALID with
 * the first differing index in mlh_last_error().  gen_out / log_len_out as
 * mlh_gen_pows_params (either may be null).  A caller that reuses one table for
 * many proofs verifies it once. */
mlh_status mlh_gen_pows_verify(mlh_ctx* ctx, const uint8_t* gen_pows, uint64_t len,
                               uint8_t gen_out[16], uint32_t* log_len_out);
mlh_status mlh_fri_prover_init(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                               mlh_transcript* tr, mlh_fri_prover** out); /* :58-76  */
mlh_status mlh_fri_prover_init_gp(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                                  const uint8_t gen_pows_1[16], uint32_t log_gen_pows,
                                  mlh_transcript* tr, mlh_fri_prover** out);
/* fold_step(&mut self, gen_pows, k, r, transcript) (fri/mod.rs:79-134).  The
 * plain form folds with the table the prover was created with (init: the
 * code's canonical table); _gp takes the caller's table for this step, as the
 * reference does at every call (multilinear_pcs.rs:72, batched_pcs.rs:121,
 * batched_fri.rs:200, fri/mod.rs:141): twiddle gen_pows[len - i 2^k] =
 * gen_pows_1^(-(i 2^k) mod len) for a table of 2^log_gen_pows powers of a
 * generator of that exact order (MLH_ERR_BAD_GENERATOR otherwise).  Any k is
 * accepted while (n/2 - 1) 2^k <= len (beyond it the reference's index
 * underflows: MLH_ERR_INVALID).  Like the reference, a step after the last
 * element folds the last tree again and re-absorbs the element. */
mlh_status mlh_fri_prover_fold_step(mlh_ctx* ctx, mlh_fri_prover* p, uint32_t k,
                                    const uint8_t r[16], mlh_transcript* tr); /* :79-134 */
mlh_status mlh_fri_prover_fold_step_gp(mlh_ctx* ctx, mlh_fri_prover* p, const uint8_t gen_pows_1[16],
                                       uint32_t log_gen_pows, uint32_t k, const uint8_t r[16],
                                       mlh_transcript* tr);
mlh_status mlh_fri_prover_fold(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                               mlh_transcript* tr, mlh_fri_prover** out); /* :136-145 */
mlh_status mlh_fri_prover_fold_gp(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                                  const uint8_t gen_pows_1[16], uint32_t log_gen_pows,
                                  mlh_transcript* tr, mlh_fri_prover** out);
uint32_t mlh_fri_prover_num_trees(const mlh_fri_prover* p);
mlh_status mlh_fri_prover_roots(const mlh_fri_prover* p, uint8_t* roots_out /* [T][32] */);
/* last_element (fri/mod.rs:13); MLH_ERR_INVALID while still None. */
mlh_status mlh_fri_prover_last_element(const mlh_fri_prover* p, uint8_t out[16]);
/* open_query_at (fri/mod.rs:154-175) -> one query record (layout below). */
mlh_status mlh_fri_prover_open_query(mlh_ctx* ctx, const mlh_fri_prover* p, uint64_t index,
                                     uint8_t* out);
void mlh_fri_prover_destroy(mlh_fri_prover* p);

/* FriProof (fri/mod.rs:239-249) as caller-allocated flat buffers.
 * Query record for a code of 2^L elements: for tree t = 0..L-2: the opened
 * ReedSolomonPair (32 B) then its L-1-t sibling digests leaf-to-root (32 B
 * each); the Direction of level i is Right iff bit i of the opened index is 0
 * (merkle_tree/mod.rs:43-47), so it is not stored. */
typedef struct mlh_fri_proof {
  uint32_t log_code;    /* L = log2(code length)                    */
  uint32_t num_trees;   /* commitments: L - MLH_LOG_BLOWUP          */
  uint32_t num_queries; /* MLH_NUM_QUERIES                          */
  uint8_t* commitments; /* [num_trees][32]                         */
  uint8_t last_elem[16];
  uint8_t last_random[32];
  uint64_t* query_indices; /* [num_queries]                         */
  uint8_t* queries;        /* [num_queries][mlh_fri_query_bytes(L)]  */
} mlh_fri_proof;
uint64_t mlh_fri_query_bytes(uint32_t log_code);
/* FriProof::prove (fri/mod.rs:261-285); _gp: with the caller's gen_pows (above). */
mlh_status mlh_fri_prove(mlh_ctx* ctx, const void* dev_code, uint32_t log_code, mlh_transcript* tr,
                         mlh_fri_proof* proof);
mlh_status mlh_fri_prove_gp(mlh_ctx* ctx, const void* dev_code, uint32_t log_code,
                            const uint8_t gen_pows_1[16], uint32_t log_gen_pows, mlh_transcript* tr,
                            mlh_fri_proof* proof);
/* Wire format: serde + bincode 2 standard / little-endian / fixed-int encoding
 * of FriProof<Field128> (fri/mod.rs:239-249, 367-397; field.rs:40-64) -- the
 * bytes the reference's bincode::serde::encode_to_vec produces.  encode needs
 * query_indices (the Direction of every path level is bit i of the index);
 * decode fills commitments, queries, last_elem, last_random and (if non-NULL)
 * query_indices recovered from the directions; MLH_ERR_VERIFY if a path's
 * directions disagree with its index (the reference verifier rejects those). */
uint64_t mlh_fri_proof_encoded_size(const mlh_fri_proof* proof);
mlh_status mlh_fri_proof_encode(const mlh_fri_proof* proof, uint8_t* out, uint64_t cap);
mlh_status mlh_fri_proof_decode_header(const uint8_t* in, uint64_t len, uint32_t* log_code,
                                       uint32_t* num_queries);
mlh_status mlh_fri_proof_decode(const uint8_t* in, uint64_t len, mlh_fri_proof* proof);
/* FriProof::verify (fri/mod.rs:287-340), host side; MLH_ERR_VERIFY if rejected.
 * Proof elements are canonical: last_elem or an opened leaf element that the
 * verifier reads whose 16 bytes spell a value >= M is MLH_ERR_VERIFY.  The
 * reference holds typed ReedSolomonPair<F> values (fri/mod.rs:177-236) and
 * hashes their canonical bytes, so it cannot accept such a leaf. */
mlh_status mlh_fri_verify(const mlh_fri_proof* proof);

/* Batched open_query_at: nq records (layout above) for host indices idx[nq]. */
mlh_status mlh_fri_prover_open_queries(mlh_ctx* ctx, const mlh_fri_prover* p,
                                       const uint64_t* idx, uint32_t nq, uint8_t* out);

/* ---- sharded building blocks (one process per GPU) ------------------------
 * The reference is single-node CPU code with no distributed API; these are
 * the rank-local steps multilinear_amd/dist.py drives between torch.distributed
 * (RCCL) collectives.  A sharded vector of 2^log_n elements over P = 2^log_p
 * ranks uses a block-cyclic layout with block 2^log_s: local index l of rank
 * r holds global ((l >> log_s) << (log_s + log_p)) | (r << log_s) | (l mod 2^log_s).
 * The distributed NTT (Polynomial::ntt / reed_solomon, ntt/mod.rs:69-108)
 * takes the cyclic layout (log_s = 0) and produces log_s = log_n - 2 log_p. */
/* Cross-shard stage: dev_in/dev_out are [P][S], S = 2^(log_n - 2 log_p).
 * Forward: row g of dev_in is the chunk received from rank g (its local
 * length-N/P NTT with generator gen^P, chunk `rank`); dev_out row t holds
 * X[t N/P + rank S + jl].  inverse != 0: the reverse (row t in, row g out,
 * scaled by 1/P; the local inverse NTT supplies 1/(N/P)).  gen has order 2^log_n. */
mlh_status mlh_shard_ntt_cross(mlh_ctx* ctx, const void* dev_in, void* dev_out, uint32_t log_n,
                               uint32_t log_p, uint32_t rank, const uint8_t gen[16], int inverse);
/* fold_step's fold (fri/mod.rs:89-114) on a sharded layer of 2^log_local local
 * values (pairs l, l + n_local/2 are global pairs i, i + n/2 while the layer
 * spans >= 2 blocks per rank); k and log_domain are global. */
mlh_status mlh_shard_fri_fold(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local, uint32_t k,
                              uint32_t log_domain, const uint8_t r[16], void* dev_next,
                              uint32_t log_s, uint32_t log_p, uint32_t rank);
/* Fold, then hash the folded layer's local leaves and build its local tree
 * (dev_tree: mlh_merkle_layers_bytes(2^(log_local-2)) bytes).  Levels below
 * log_s are the global tree's; the caller combines the level-log_s nodes of
 * all ranks. */
mlh_status mlh_shard_fri_fold_commit(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local,
                                     uint32_t k, uint32_t log_domain, const uint8_t r[16],
                                     void* dev_next, void* dev_tree, uint32_t log_s,
                                     uint32_t log_p, uint32_t rank);
/* Merkle::open / batch_open (merkle_tree/mod.rs:31-58, :134-175) on any device
 * tree of `leaves` leaves (mlh_merkle_commit*, level order): for each
 * host_idx[q] the log2(leaves) sibling digests, bottom-up, into host out
 * (nq * 32 * log2(leaves) bytes).  Direction of level i is Right iff bit i of
 * the index is 0.  MLH_ERR_INVALID for an index >= leaves (the reference
 * returns None).  The opened value is the caller's item (column) itself. */
mlh_status mlh_merkle_open(mlh_ctx* ctx, const void* dev_layers, uint64_t leaves,
                           const uint64_t* host_idx, uint32_t nq, uint8_t* out);
/* MerkleInclusionPath::verify / batch_verify (merkle_tree/mod.rs:216-293),
 * host side: value = the leaf bytes (batch_verify: the column items
 * concatenated), sibs = depth digests, dirs bit i = 1 for Direction::Left.
 * MLH_OK, MLH_ERR_VERIFY (IncompatibleHash) or MLH_ERR_VERIFY_INDEX
 * (IncompatibleIndex), checked in that order as the reference does. */
mlh_status mlh_merkle_verify(const uint8_t* value, uint64_t value_len, const uint8_t* sibs,
                             uint32_t depth, uint64_t dirs, const uint8_t root[32], uint64_t index);
/* Merkle::open (merkle_tree/mod.rs:31-58) on a local pair tree: for each
 * local leaf idx[q]: values[idx], values[idx + n/2], then the sibling digests
 * of levels 0..levels-1.  out: nq * 32 * (1 + levels) bytes (host). */
mlh_status mlh_merkle_open_pairs(mlh_ctx* ctx, const void* dev_values, uint32_t log_n,
                                 const void* dev_tree, uint32_t levels, const uint64_t* idx,
                                 uint32_t nq, uint8_t* out);

/* Device-resident Fiat-Shamir for sharded loops: the transcript state lives
 * in a mlh_device_transcript_bytes() device buffer (same bytes as the host
 * SHA-256 state); absorb reads from HBM and optionally writes
 * next_challenge() (16 B) to HBM, where the *_dr steps read it. */
uint64_t mlh_device_transcript_bytes(void);
mlh_status mlh_transcript_to_device(mlh_ctx* ctx, const mlh_transcript* tr, void* dev_state);
mlh_status mlh_transcript_from_device(mlh_ctx* ctx, const void* dev_state, mlh_transcript* tr);
mlh_status mlh_device_transcript_absorb(mlh_ctx* ctx, void* dev_state, const void* dev_src,
                                        uint32_t n, void* dev_challenge);
/* final fold's two values: flag (u32) = not an RS code, absorb LE16(v0), last = v0 */
mlh_status mlh_device_fri_last(mlh_ctx* ctx, const void* dev_vals2, void* dev_state,
                               void* dev_flag, void* dev_last);
/* mlh_shard_fri_fold(_commit) with the challenge read from HBM (dev_r, 16 B). */
mlh_status mlh_shard_fri_fold_dr(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local,
                                 uint32_t k, uint32_t log_domain, const void* dev_r,
                                 void* dev_next, uint32_t log_s, uint32_t log_p, uint32_t rank);
mlh_status mlh_shard_fri_fold_commit_dr(mlh_ctx* ctx, const void* dev_layer, uint32_t log_local,
                                        uint32_t k, uint32_t log_domain, const void* dev_r,
                                        void* dev_next, void* dev_tree, uint32_t log_s,
                                        uint32_t log_p, uint32_t rank);
/* Cross-rank top of a sharded tree: dev_gathered = [P][per_rank] subtree roots
 * (all-gathered); dev_levels receives the tree over the P*per_rank nodes in
 * global order (t*P + h), level 0 first, root last: (2*P*per_rank - 1) x 32 B. */
mlh_status mlh_merkle_top(mlh_ctx* ctx, const void* dev_gathered, uint32_t P, uint64_t per_rank,
                          void* dev_levels);

/* Device-resident sumcheck steps: round sums written to HBM (2 x 16 B), the
 * challenge read from HBM; mlh_device_sumcheck_round adds npairs (s1, s2)
 * pairs (e.g. one per rank, all-gathered), interpolates, absorbs (c1, c2)
 * into the device transcript, writes c1 c2 and r, and updates the claim. */
mlh_status mlh_sumcheck_sums_dev(mlh_ctx* ctx, const void* dev_matrix, const void* dev_delta,
                                 uint32_t log_height, void* dev_sums);
mlh_status mlh_sumcheck_fold_sums_dr(mlh_ctx* ctx, void* dev_matrix, void* dev_delta,
                                     uint32_t log_height, const void* dev_r, void* dev_sums);
mlh_status mlh_sumcheck_fold_dr(mlh_ctx* ctx, void* dev_matrix, void* dev_delta,
                                uint32_t log_height, const void* dev_r);
mlh_status mlh_device_sumcheck_round(mlh_ctx* ctx, const void* dev_sum_pairs, uint32_t npairs,
                                     void* dev_prev, void* dev_state, void* dev_poly_out,
                                     void* dev_r_out);

/* ---- batched FRI / batched PCS (src/fri/batched_fri.rs, batched_pcs.rs) ----
 * m codes (or MLEs) stored back to back on the device: item j at j * size.
 * fingerprint(r, c_0..c_{m-1}) = Horner = sum_j c_j r^(m-1-j) (batched_fri.rs:30-38). */
typedef struct mlh_batched_fri_proof {
  uint32_t log_code;    /* L = log2(code length)                            */
  uint32_t num_codes;   /* m                                               */
  uint32_t num_trees;   /* inner FRI commitments: L - 2                    */
  uint32_t num_queries; /* MLH_NUM_QUERIES                                 */
  uint8_t batch_commitment[32];
  uint8_t* commitments; /* [num_trees][32]                                 */
  uint8_t last_elem[16];
  uint8_t last_random[32];
  uint64_t* query_indices; /* [num_queries] (optional)                     */
  uint8_t* queries;        /* [num_queries][mlh_batched_fri_query_bytes]   */
} mlh_batched_fri_proof;
/* Query record: the opened batch column (m x 32 B RS pairs, code order) and
 * its L-1 batch-tree siblings, then the inner QueryProof: for inner tree
 * t = 0..L-3 the pair (32 B) and its L-2-t siblings (directions = index bits). */
uint64_t mlh_batched_fri_query_bytes(uint32_t log_code, uint32_t num_codes);
/* BatchedFriProof::prove (batched_fri.rs:280-311). */
mlh_status mlh_batched_fri_prove(mlh_ctx* ctx, const void* dev_codes, uint32_t num_codes,
                                 uint32_t log_code, mlh_transcript* tr,
                                 mlh_batched_fri_proof* proof);
/* BatchedFriProof::verify (batched_fri.rs:313-388), host side.  last_elem or
 * an opened element (batch column or inner leaf) >= M: MLH_ERR_VERIFY, as
 * mlh_fri_verify (typed ReedSolomonPair<F>, fri/mod.rs:177-236). */
mlh_status mlh_batched_fri_verify(const mlh_batched_fri_proof* proof);
/* BatchedFriProverData step by step (batched_fri.rs:9-224), the transcript on
 * the host: what BatchedFriProverData::fold (:178-205) and BatchedPCSProverData
 * (batched_pcs.rs:80-125) call.
 *  - init (:41-98): batch layer of the m codes' RS pairs (dev_codes = the codes
 *    back to back, 2^log_code each, kept by the caller while the prover lives),
 *    absorb its root, fingerprint_r = next_challenge(), absorb LE16 of it;
 *  - fold_step_gp = batched_fold_step(&mut self, gen_pows, r, transcript)
 *    (:100-176): fingerprinted pairs folded with k = 0 and twiddle
 *    gen_pows[len - i], then the folded layer's tree (or, at 4 elements, the
 *    last element) into fri_data, and its root (last element) absorbed; a
 *    second call is MLH_ERR_INVALID (the reference would fold the batch layer
 *    again);
 *  - inner = &mut self.fri_data: the FriProverData whose fold_step(gen_pows, k,
 *    r, tr) the reference calls for k >= 1 (:200) -- pass it to
 *    mlh_fri_prover_fold_step(_gp), _roots, _last_element, _open_query(ies);
 *    owned by the batched prover (do not destroy it);
 *  - open_query = open_query_at (:207-224): one record in the
 *    mlh_batched_fri_query_bytes layout (inner part zero where fri_data has
 *    no tree yet). */
typedef struct mlh_batched_fri_prover mlh_batched_fri_prover;
mlh_status mlh_batched_fri_prover_init(mlh_ctx* ctx, const void* dev_codes, uint32_t num_codes,
                                       uint32_t log_code, mlh_transcript* tr,
                                       mlh_batched_fri_prover** out);
mlh_status mlh_batched_fri_prover_fold_step_gp(mlh_ctx* ctx, mlh_batched_fri_prover* bp,
                                               const uint8_t gen_pows_1[16], uint32_t log_gen_pows,
                                               const uint8_t r[16], mlh_transcript* tr);
mlh_fri_prover* mlh_batched_fri_prover_inner(mlh_batched_fri_prover* bp);
mlh_status mlh_batched_fri_prover_batch_root(const mlh_batched_fri_prover* bp, uint8_t out[32]);
mlh_status mlh_batched_fri_prover_fingerprint_r(const mlh_batched_fri_prover* bp, uint8_t out[16]);
mlh_status mlh_batched_fri_prover_open_query(mlh_ctx* ctx, const mlh_batched_fri_prover* bp,
                                             uint64_t index, uint8_t* out);
void mlh_batched_fri_prover_destroy(mlh_batched_fri_prover* bp);
typedef struct mlh_batched_pcs_proof {
  mlh_batched_fri_proof fri;
  uint8_t* sumcheck_polys; /* [n_vars][2][16] */
} mlh_batched_pcs_proof;
/* BatchedPCSProof::prove (batched_pcs.rs:127-180): dev_evals = num_polys MLEs
 * of 2^n_vars evals; claim = (inputs[n_vars], outputs[num_polys]) LE16 each. */
mlh_status mlh_batched_pcs_prove(mlh_ctx* ctx, const void* dev_evals, uint32_t num_polys,
                                 uint32_t n_vars, const uint8_t* inputs, const uint8_t* outputs,
                                 mlh_transcript* tr, mlh_batched_pcs_proof* proof);
/* BatchedPCSProof::verify (batched_pcs.rs:182-250), host side.  A sumcheck
 * coefficient, last_elem or an opened element >= M: MLH_ERR_VERIFY, as
 * mlh_fri_verify (typed ReedSolomonPair<F>, fri/mod.rs:177-236).  inputs and
 * outputs are the caller's and are not range-checked here. */
mlh_status mlh_batched_pcs_verify(const mlh_batched_pcs_proof* proof, uint32_t n_vars,
                                  const uint8_t* inputs, const uint8_t* outputs,
                                  mlh_transcript* tr);

/* ---- transcript (src/transcript.rs), host side --------------------------- */
mlh_status mlh_transcript_create(mlh_transcript** out);
mlh_status mlh_transcript_clone(const mlh_transcript* t, mlh_transcript** out);
void mlh_transcript_destroy(mlh_transcript* t);
mlh_status mlh_transcript_absorb(mlh_transcript* t, const uint8_t* bytes, uint64_t len); /* :31 */
mlh_status mlh_transcript_random(const mlh_transcript* t, uint8_t out[32]);             /* :23 */
mlh_status mlh_transcript_next_challenge(mlh_transcript* t, uint8_t out[16]);          /* :35 */

/* ---- multilinear polynomials and sumcheck -------------------------------- */
/* MultilinearPolynomialEvals::to_coefficient (polynomials.rs:150-163), in place. */
mlh_status mlh_mle_to_coefficient(mlh_ctx* ctx, void* dev_evals, uint32_t log_n);
/* MultilinearPolynomial::to_evaluation (polynomials.rs:111-124), in place. */
mlh_status mlh_mle_to_evaluation(mlh_ctx* ctx, void* dev_coeffs, uint32_t log_n);
/* delta table of SumcheckTables::build_tables_for_pcs (sumcheck.rs:128-145,
 * Mask::evaluate evaluation.rs:51-73): out[idx] = prod_i (bit_i(idx) ?
 * p[n-1-i] : 1-p[n-1-i]); host_points: n elements. */
mlh_status mlh_eq_table(mlh_ctx* ctx, const uint8_t* host_points, uint32_t n, void* dev_out);
/* MultilinearPolynomialEvals::evaluate (polynomials.rs:165-187). */
mlh_status mlh_mle_evaluate(mlh_ctx* ctx, const void* dev_evals, uint32_t n,
                            const uint8_t* host_args, uint8_t out[16]);
/* MultilinearPolynomial::evaluate (polynomials.rs:126-146), coefficient form:
 * sum_pos coeffs[pos] * prod_{bit b of pos set} args[n-1-b]. */
mlh_status mlh_mle_coeffs_evaluate(mlh_ctx* ctx, const void* dev_coeffs, uint32_t n,
                                   const uint8_t* host_args, uint8_t out[16]);
/* Polynomial::evaluate (ntt/mod.rs:61-67, polynomials.rs:9-14): Horner's
 * value sum_i coeffs[i] x^i of n device coefficients at host x (canonical);
 * n = 0 gives 0. */
mlh_status mlh_poly_evaluate(mlh_ctx* ctx, const void* dev_coeffs, uint64_t n, const uint8_t x[16],
                             uint8_t out[16]);
/* Trace::evaluate (constraint_system/evaluation.rs:31-48): the row-major
 * 2^log_height x width trace (dev_matrix, element (i, j) at i*width + j) as
 * width MLEs evaluated at the log_height host points (big-endian, Mask order):
 * out[j] = sum_i Mask{i}(points) * matrix[i*width + j]; out: 16*width bytes. */
mlh_status mlh_trace_evaluate(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                              uint32_t width, const uint8_t* host_points, uint8_t* out);
/* SumcheckTables::partial_sum (sumcheck.rs:204-232), composition x[0]
 * (multilinear_pcs.rs:56), at X = 1 and X = 2: out = s1 ‖ s2.
 * Tables have 2^log_height elements. */
mlh_status mlh_sumcheck_partial_sums(mlh_ctx* ctx, const void* dev_matrix, const void* dev_delta,
                                     uint32_t log_height, uint8_t out[32]);
/* SumcheckTables::fold (sumcheck.rs:234-247), in place: height 2^log_height
 * -> 2^(log_height-1) (first half). */
mlh_status mlh_sumcheck_fold(mlh_ctx* ctx, void* dev_matrix, void* dev_delta, uint32_t log_height,
                             const uint8_t r[16]);
/* fold followed by the next round's partial sums, one HBM pass. */
mlh_status mlh_sumcheck_fold_and_sums(mlh_ctx* ctx, void* dev_matrix, void* dev_delta,
                                      uint32_t log_height, const uint8_t r[16], uint8_t out[32]);
/* SumcheckTables::compute_sumcheck_polynomials (sumcheck.rs:77-102) for the
 * PCS composition (x[0], total degree 2): log_height rounds; per round the
 * two nonzero coefficients (c1, c2) go to polys_out[round][2][16] and the
 * challenge to rs_out[round][16].  Tables are folded in place. */
mlh_status mlh_sumcheck_prove(mlh_ctx* ctx, void* dev_matrix, void* dev_delta, uint32_t log_height,
                              const uint8_t sum[16], mlh_transcript* tr, uint8_t* polys_out,
                              uint8_t* rs_out);
/* SumcheckTables::build_tables_for_pcs (sumcheck.rs:128-145) followed by
 * compute_sumcheck_polynomials (:77-102), with the delta table = eq(points)
 * never materialised at full size: it stays c_k * eq(p_k..p_{L-1}) (a running
 * scalar times a two-level factored table) until it has 2^12 entries.  Same
 * outputs as mlh_eq_table + mlh_sumcheck_prove; half the HBM traffic.
 * dev_evals: the MLE (2^log_height elements).  dev_work (2^(log_height-1)
 * elements) receives the folded matrix (the first half of the table as
 * SumcheckTables::fold leaves it) and dev_evals is not modified -- the
 * matrix clone of build_tables_for_pcs is never made; dev_work = NULL folds
 * dev_evals in place.  host_points: log_height elements; delta_out
 * (optional): the fully folded delta. */
mlh_status mlh_sumcheck_prove_eq(mlh_ctx* ctx, const void* dev_evals, void* dev_work,
                                 uint32_t log_height, const uint8_t* host_points,
                                 const uint8_t sum[16], mlh_transcript* tr, uint8_t* polys_out,
                                 uint8_t* rs_out, uint8_t* delta_out);

/* ---- constraint-system sumcheck (src/constraint_system) ------------------- *
 * The general prover of constraint_system/sumcheck.rs: a row-major
 * 2^log_height x width trace (element (i, j) at i*width + j), a delta table of
 * 2^log_height elements (System::build_tables, :22-38: mlh_eq_table of the row
 * challenges) and a composition sum_c mask[c] * constraint_c(row, randoms)
 * (ConstraintSet::evaluate, evaluation.rs:21-29) of degree `degree`.
 *
 * A constraint program replaces Expr<F>(fn(&[F], &[F]) -> F)
 * (constraints.rs:3-10): straight-line code over field elements, built on the
 * host and interpreted on the device.  Wire format, little-endian, no padding:
 *   header   7 x u32: width, n_randoms, n_consts, n_temps, n_instr,
 *            n_constraints, degree
 *   consts   n_consts x 16 bytes, canonical elements
 *   code     n_instr x 8 bytes: op, dst_temp, a.kind, a.index, b.kind,
 *            b.index, 0, 0   (op: 0 ADD, 1 SUB, 2 MUL, 3 NEG; temp[dst] =
 *            a op b; NEG: temp[dst] = -a and b = (0, 0))
 *   outputs  n_constraints x 2 bytes: kind, index (constraint c's value)
 * An operand is (kind, index): kind 0 column (the row's element `index`),
 * 1 random, 2 const, 3 temp.  Limits: width 1..32, n_temps <= 32,
 * n_consts <= 64, n_randoms <= 64, n_constraints 1..256, n_instr <= 4096,
 * degree 1..7.  mlh_cs_program_create returns MLH_ERR_INVALID for a buffer
 * that is truncated or has trailing bytes, an index out of range, a temp read
 * before it is written, a non-canonical constant, n_constraints == 0, a limit
 * exceeded, a nonzero reserved byte, or an output whose formal degree (column
 * 1, random / const 0, add / sub / neg max, mul sum) exceeds `degree`; a
 * declared degree above the formal one is allowed, as in the reference.
 * A program object is host memory only and may be used with any context. */
typedef struct mlh_cs_program mlh_cs_program;
#define MLH_CS_MAX_LOG_HEIGHT 32
mlh_status mlh_cs_program_create(const uint8_t* bytes, uint64_t len, mlh_cs_program** out);
void mlh_cs_program_destroy(mlh_cs_program* prog);
uint32_t mlh_cs_program_width(const mlh_cs_program* prog);         /* system.rs:106-108 */
uint32_t mlh_cs_program_degree(const mlh_cs_program* prog);        /* constraints.rs:31-33 */
uint32_t mlh_cs_program_n_constraints(const mlh_cs_program* prog); /* constraints.rs:27-29 */
uint32_t mlh_cs_program_n_randoms(const mlh_cs_program* prog);     /* system.rs:22 */
/* System::evaluate_composition (evaluation.rs:5-11) on the host: the program
 * on one row (width values), n_randoms randoms and n_constraints mask
 * elements; the interpreter mlh_cs_sumcheck_verify uses. */
mlh_status mlh_cs_program_evaluate(const mlh_cs_program* prog, const uint8_t* host_values,
                                   const uint8_t* host_randoms, const uint8_t* host_mask,
                                   uint8_t out[16]);
/* Launch shape of the first pass over tables of 2^log_height rows: the block
 * size (from the program's LDS slots) and the number of blocks; a thread
 * visits ceil(2^(log_height-1) / (threads * blocks)) row pairs. */
mlh_status mlh_cs_launch_info(const mlh_cs_program* prog, uint32_t log_height, uint32_t* threads,
                              uint32_t* blocks);
/* ChallengeSet::new (system.rs:131-146) and the constraint mask (:82-95), as
 * the reference computes them: `vec![transcript.next_challenge(); n]`
 * evaluates the call once and clones it, and next_challenge() does not change
 * the transcript (transcript.rs:35-38), so row_out (log_rows elements),
 * trace_out (n_randoms) and constraint_out (log2(next_pow2(n_constraints)))
 * are all filled with the same single challenge and the transcript is left
 * unchanged.  mask_out[c] = Mask{c, n_vars = log2(next_pow2(n_constraints))}
 * .evaluate(constraint), n_constraints elements (1 for a single constraint). */
mlh_status mlh_system_challenges(mlh_transcript* tr, uint32_t log_rows, uint32_t n_randoms,
                                 uint32_t n_constraints, uint8_t* row_out, uint8_t* trace_out,
                                 uint8_t* constraint_out, uint8_t* mask_out);
/* SumcheckTables::partial_sum (sumcheck.rs:204-232) at X = 1..D, D = degree+1
 * (:159,185): out = D x 16 bytes.  width must equal the program's
 * (MLH_ERR_INVALID otherwise, as for every call below that takes both);
 * host_randoms: n_randoms elements (may be NULL when 0), host_mask:
 * n_constraints elements. */
mlh_status mlh_cs_partial_sums(mlh_ctx* ctx, const mlh_cs_program* prog, uint32_t width,
                               const void* dev_matrix, const void* dev_delta, uint32_t log_height,
                               const uint8_t* host_randoms, const uint8_t* host_mask,
                               uint8_t* out);
/* SumcheckTables::fold (sumcheck.rs:234-247) of all columns and delta, in
 * place: height 2^log_height -> 2^(log_height-1) (the first half). */
mlh_status mlh_cs_fold(mlh_ctx* ctx, uint32_t width, void* dev_matrix, void* dev_delta,
                       uint32_t log_height, const uint8_t r[16]);
/* fold followed by the folded tables' partial sums, one HBM pass
 * (log_height >= 2). */
mlh_status mlh_cs_fold_and_sums(mlh_ctx* ctx, const mlh_cs_program* prog, uint32_t width,
                                void* dev_matrix, void* dev_delta, uint32_t log_height,
                                const uint8_t* host_randoms, const uint8_t* host_mask,
                                const uint8_t r[16], uint8_t* out);
/* System::compute_sumcheck_polynomials (sumcheck.rs:40-53) =
 * SumcheckTables::compute_sumcheck_polynomials (:147-202): log_height rounds
 * on the device with one synchronisation at the end; per round the D nonzero
 * coefficients c1..cD go to polys_out[round][D][16] and the challenge to
 * rs_out[round][16] (either may be NULL).  Tables are folded in place: on
 * return row 0 of dev_matrix is Trace::evaluate(rs) and dev_delta[0] is
 * Delta{row}.evaluate(rs).  The host replays the transcript from the returned
 * coefficients; if a challenge differs the call returns MLH_ERR_DEVICE and
 * leaves the transcript unchanged.  log_height == 0 is zero rounds: MLH_OK,
 * nothing written, transcript untouched.  log_height <=
 * MLH_CS_MAX_LOG_HEIGHT. */
mlh_status mlh_cs_sumcheck_prove(mlh_ctx* ctx, const mlh_cs_program* prog, uint32_t width,
                                 void* dev_matrix, void* dev_delta, uint32_t log_height,
                                 const uint8_t* host_randoms, const uint8_t* host_mask,
                                 const uint8_t sum[16], mlh_transcript* tr, uint8_t* polys_out,
                                 uint8_t* rs_out);
/* System::verify_with_evaluations (sumcheck.rs:91-124), host only, with
 * SumcheckPolynomial::to_polynomial's a0 = (sum - sum of coefficients) / 2
 * (:269-276): host_row_points = the row challenges (log_height elements),
 * polys = [log_height][D][16], host_output = width elements (Trace::evaluate
 * at the challenges).  MLH_ERR_VERIFY where the reference asserts (and for a
 * non-canonical element of polys or host_output); the transcript is then
 * left as it was.  On MLH_OK it has absorbed every coefficient. */
mlh_status mlh_cs_sumcheck_verify(const mlh_cs_program* prog, uint32_t log_height,
                                  const uint8_t* host_row_points, const uint8_t* host_randoms,
                                  const uint8_t* host_mask, const uint8_t sum[16],
                                  const uint8_t* polys, const uint8_t* host_output,
                                  mlh_transcript* tr);

/* The same with sum columns (WitnessLayout::sum_columns, system.rs:27-29: "the
 * sum of all sum columns is the main result of the trace"): the claim is
 *   sum_i [ delta[i] composition(row_i) + beta sum_{j in S} row_i[j] ]
 * with S = the set bits of sum_column_mask (bit j = column j; a bit at or
 * above the width is MLH_ERR_INVALID) and claim = sum + beta * column_sum, which
 * the caller forms.  The round polynomial keeps total degree d + 1 and its D
 * points; the final check is delta(rs) composition(output) + beta
 * sum_{j in S} output[j] = pol(r_last).  sum_column_mask = 0 (beta may be
 * NULL) is mlh_cs_sumcheck_prove / _verify themselves, which call these: the
 * same launches, the same bytes. */
mlh_status mlh_cs_sumcheck_prove_sums(mlh_ctx* ctx, const mlh_cs_program* prog, uint32_t width,
                                      void* dev_matrix, void* dev_delta, uint32_t log_height,
                                      const uint8_t* host_randoms, const uint8_t* host_mask,
                                      uint32_t sum_column_mask, const uint8_t* beta,
                                      const uint8_t claim[16], mlh_transcript* tr,
                                      uint8_t* polys_out, uint8_t* rs_out);
mlh_status mlh_cs_sumcheck_verify_sums(const mlh_cs_program* prog, uint32_t log_height,
                                       const uint8_t* host_row_points, const uint8_t* host_randoms,
                                       const uint8_t* host_mask, uint32_t sum_column_mask,
                                       const uint8_t* beta, const uint8_t claim[16],
                                       const uint8_t* polys, const uint8_t* host_output,
                                       mlh_transcript* tr);

/* ---- trace commitment and the system proof (src/constraint_system) -------- *
 * The reference calls Commitment::new(&trace) in System::prover before the
 * challenges are drawn (system.rs:62-63) and leaves its body a TODO
 * (trace.rs:40-48).  Here the commitment is the commit phase of the batched
 * PCS over the trace's width column MLEs, and the system proof opens it at
 * the sumcheck's point, so a verifier without the trace can check
 * sum_i delta[i] * composition(row_i) = sum.  Transcript order, prover and
 * verifier alike:
 *   1. absorb the 32-byte trace root;
 *   2. ChallengeSet::new and the constraint mask (mlh_system_challenges);
 *   3. the constraint sumcheck with delta = mlh_eq_table(row): per round
 *      absorb c1..cD, draw r; output = Trace::evaluate(rs);
 *   4. BatchedPCSProof::prove / verify with inputs = rs, outputs = output. */
/* Row-major 2^log_height x width trace -> width column MLEs, column-major:
 * out[j * 2^log_height + i] = matrix[i * width + j] (the columns
 * Trace::evaluate, evaluation.rs:31-48, treats as MLEs).  Out of place: width
 * 1..32, log_height 0..32; MLH_ERR_INVALID for a null pointer, a width out of
 * range or overlapping buffers.  One kernel launch on the context stream. */
mlh_status mlh_trace_columns(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                             uint32_t width, void* dev_out);
/* Launch shape of mlh_trace_columns: the rows a block stages per tile and the
 * number of blocks; a block visits ceil(tiles / blocks) tiles of
 * min(tile_rows, 2^log_height) rows. */
mlh_status mlh_trace_columns_launch_info(uint32_t log_height, uint32_t width, uint32_t* tile_rows,
                                         uint32_t* blocks);
/* Commitment::new (trace.rs:44-47): mlh_trace_columns, then the
 * transcript-independent front of BatchedPCSProof::prove -- per column
 * to_coefficient, bit reverse, reed_solomon at blow-up 2
 * (batched_pcs.rs:135-149) -- and the batch layer's Merkle tree over the width
 * codes (BatchedFriProverData::init, batched_fri.rs:41-81).  The handle owns
 * the column evaluations (width * 2^log_height * 16 B), the codes (twice
 * that) and the tree (mlh_merkle_layers_bytes(2^log_height)); dev_matrix is
 * not modified and not referenced after the call.  Its root equals the
 * batch_commitment of mlh_batched_pcs_prove over the same columns.  width
 * 1..32, log_height 1..32 (the batched PCS needs one variable).  Synchronises. */
typedef struct mlh_trace_commitment mlh_trace_commitment;
mlh_status mlh_trace_commit(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                            uint32_t width, mlh_trace_commitment** out);
/* The same over columns [col0, col0 + ncols) of the row-major trace only:
 * out[j * 2^log_height + i] = matrix[i * width + col0 + j], j < ncols.  No
 * element outside the range is read (in phase 1 of a two-phase proof the later
 * columns are not filled yet).  MLH_ERR_INVALID also for ncols = 0 or a range
 * that leaves the trace.  One kernel launch; its launch shape is that of an
 * ncols-wide trace. */
mlh_status mlh_trace_columns_range(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                   uint32_t width, uint32_t col0, uint32_t ncols, void* dev_out);
mlh_status mlh_trace_columns_range_launch_info(uint32_t log_height, uint32_t width, uint32_t col0,
                                               uint32_t ncols, uint32_t* tile_rows,
                                               uint32_t* blocks);
/* mlh_trace_commit over columns [col0, col0 + ncols) (Commitment::new,
 * trace.rs:44-47, of the columns a WitnessLayout phase holds, system.rs:23-26):
 * the handle's width is ncols and its root equals the batch_commitment of
 * mlh_batched_pcs_prove over those columns.  It depends on no element outside
 * the range. */
mlh_status mlh_trace_commit_range(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                  uint32_t width, uint32_t col0, uint32_t ncols,
                                  mlh_trace_commitment** out);
mlh_status mlh_trace_commitment_root(const mlh_trace_commitment* c, uint8_t out[32]);
uint32_t mlh_trace_commitment_width(const mlh_trace_commitment* c);
uint32_t mlh_trace_commitment_log_height(const mlh_trace_commitment* c);
/* Drains the context stream first. */
void mlh_trace_commitment_destroy(mlh_trace_commitment* c);
typedef struct mlh_system_proof {
  uint32_t log_height, width, degree;
  uint8_t* sumcheck_polys;   /* [log_height][degree+1][16], c1..cD per round  */
  uint8_t* output;           /* [width][16] = Trace::evaluate(rs)             */
  mlh_batched_pcs_proof pcs; /* caller-allocated as for mlh_batched_pcs_prove
                                (n_vars = log_height, num_polys = width);
                                pcs.fri.batch_commitment is the trace commitment */
} mlh_system_proof;
/* System::prover (system.rs:56-72) through to a proof, in the order above:
 * the rounds of mlh_cs_sumcheck_prove (sumcheck.rs:40-53) on dev_matrix --
 * the committed trace, folded in place -- then BatchedPCSProof::prove
 * (batched_pcs.rs:150-180) on the handle's codes, evaluations and batch tree
 * (no code or tree is computed a second time).  MLH_ERR_INVALID for a null
 * pointer (proof->sumcheck_polys and proof->output included), a program width
 * other than the commitment's, a handle of another context or a
 * non-canonical sum.  On any non-OK return the transcript is exactly as it
 * was at entry.  A dev_matrix that is not the committed trace cannot be
 * detected here: the call returns MLH_OK and mlh_system_verify rejects the
 * proof. */
mlh_status mlh_system_prove(mlh_ctx* ctx, const mlh_cs_program* prog,
                            const mlh_trace_commitment* commitment, void* dev_matrix,
                            const uint8_t sum[16], mlh_transcript* tr, mlh_system_proof* proof);
/* The verifier of that proof, host only: absorb pcs.fri.batch_commitment,
 * draw the challenges (system.rs:39-54), System::verify_with_evaluations
 * (sumcheck.rs:91-124) with host_output = proof->output, then
 * BatchedPCSProof::verify (batched_pcs.rs:182-250) at the rs the sumcheck
 * derived.  MLH_ERR_VERIFY where a component rejects, where
 * proof->{log_height, width, degree} disagree with log_height or the program,
 * and for a non-canonical element; the transcript is then exactly as it was
 * at entry.  On MLH_OK it ends in the prover's state. */
mlh_status mlh_system_verify(const mlh_cs_program* prog, uint32_t log_height, const uint8_t sum[16],
                             const mlh_system_proof* proof, mlh_transcript* tr);

/* ---- the system proof in two phases (WitnessLayout, system.rs:17-30) ------- *
 * pre_random_columns P (1 <= P <= width W): "the columns that you must fill
 * before knowing the value of the random challenges" (system.rs:23-26);
 * sum_columns S (a mask over the columns): "the sum of all sum columns is the
 * main result of the trace" (system.rs:27-29).  The verifier checks
 *   sum_i delta[i] composition(row_i) = sum  and  sum_i sum_{j in S} row_i[j]
 *   = column_sum
 * through one sumcheck over their random combination.  Transcript order:
 *   1. absorb root1, the commitment to columns [0, P);
 *   2. the trace randoms: n_randoms copies of one next_challenge()
 *      (ChallengeSet::new, system.rs:139);
 *   3. if P < W: absorb root2, the commitment to columns [P, W);
 *   4. the row and constraint challenges and the mask (mlh_system_challenges
 *      with n_randoms = 0);
 *   5. if S is not empty: absorb LE16(column_sum), beta = next_challenge();
 *   6. mlh_cs_sumcheck_prove_sums with claim = sum + beta * column_sum;
 *      output = row 0 of the folded matrix;
 *   7. BatchedPCSProof::prove (batched_pcs.rs:127-180) on commitment 1 with
 *      inputs rs, outputs output[0:P];  8. if P < W: the same on commitment 2
 *      with output[P:W].
 * With P = W and S empty this is mlh_system_prove's order, byte for byte. */
/* Steps 1-2 on a copy of tr, which is left as it is: what the prover calls
 * between the two commitments to fill the columns at and above P.  out:
 * n_randoms elements. */
mlh_status mlh_system_trace_randoms(const mlh_transcript* tr, const uint8_t root1[32],
                                    uint32_t n_randoms, uint8_t* out);
typedef struct mlh_phased_proof {
  uint32_t log_height, width, degree;
  uint32_t pre_random_columns; /* P */
  uint32_t sum_column_mask;    /* S, bit j = column j */
  uint8_t* sumcheck_polys;     /* [log_height][degree+1][16], c1..cD per round */
  uint8_t* output;             /* [width][16] = Trace::evaluate(rs)            */
  /* caller-allocated as for mlh_batched_pcs_prove with n_vars = log_height:
   * pcs[0] for P polynomials, pcs[1] for W - P (unused when P = W) */
  mlh_batched_pcs_proof pcs[2];
} mlh_phased_proof;
/* System::prover (system.rs:56-72) for a two-phase layout, steps 1-8.  P is
 * commitment1's width; commitment2 is NULL iff P = W, and the two widths add
 * up to the program's.  dev_matrix is the trace as commitment2 saw it, folded
 * in place.  Both openings run on the handles' codes, evaluations and batch
 * trees (nothing is computed a second time).  MLH_ERR_INVALID for a null
 * pointer, widths that do not add up, handles of different heights or of
 * another context, a mask bit at or above W, a non-canonical sum or
 * column_sum.  On any non-OK return the transcript is exactly as at entry. */
mlh_status mlh_system_prove_phased(mlh_ctx* ctx, const mlh_cs_program* prog,
                                   const mlh_trace_commitment* commitment1,
                                   const mlh_trace_commitment* commitment2,
                                   uint32_t sum_column_mask, void* dev_matrix,
                                   const uint8_t sum[16], const uint8_t column_sum[16],
                                   mlh_transcript* tr, mlh_phased_proof* proof);
/* The verifier (system.rs:39-54, sumcheck.rs:91-124, batched_pcs.rs:182-250),
 * host only, in the same order with root1 / root2 = pcs[0] / pcs[1]'s
 * batch_commitment.  MLH_ERR_VERIFY, with the transcript exactly as at entry,
 * for any rejection, any disagreement between the proof's header and
 * (log_height, the program, pre_random_columns, sum_column_mask) and any
 * non-canonical element.  On MLH_OK the transcript ends in the prover's state. */
mlh_status mlh_system_verify_phased(const mlh_cs_program* prog, uint32_t log_height,
                                    uint32_t pre_random_columns, uint32_t sum_column_mask,
                                    const uint8_t sum[16], const uint8_t column_sum[16],
                                    const mlh_phased_proof* proof, mlh_transcript* tr);

/* ---- next-row constraints: shifted columns in the system proof -------------- *
 * The rows are cyclic: next(c) at row i is column c of row (i + 1) mod
 * 2^log_height.  A shifted system is a trace of width W, a list of K distinct
 * source columns c_0 .. c_{K-1} (each < W, K >= 0, W + K <= 32) and an
 * ordinary constraint program of width W' = W + K in which column W + k stands
 * for next(c_k); the list travels beside the program, whose wire format is
 * unchanged.  A constraint that should not hold across the wrap from the last
 * row to row 0 is gated by a selector column of the caller's, e.g.
 * (1 - last) * (next(a) - a - b); such a selector belongs in a public column
 * (below), where the verifier derives it.  The sumcheck folds rows pairwise, so "the
 * next row" is a protocol step and no addressing mode.  Transcript order, on
 * top of the two-phase proof's:
 *   1-5. as mlh_system_prove_phased (the program's randoms and constraints);
 *   6. the constraint sumcheck (mlh_cs_sumcheck_prove_sums) on the extension E,
 *      2^log_height x W': E[i][j] = T[i][j], j < W, E[i][W + k] =
 *      T[(i + 1) mod 2^log_height][c_k]; the sum-column mask names real
 *      columns only; output = row 0 of the folded E: T_j(rs) for j < W and
 *      N_k = sum_i eq(rs, i) T_{c_k}(i + 1) for the rest;
 *   7. only if K > 0: absorb the W' elements of output (16 W' bytes, in
 *      order), lambda = next_challenge(), then mlh_cs_sumcheck_prove of
 *        sum_j succ_rs[j] sum_k lambda^k T_{c_k}[j] = sum_k lambda^k N_k
 *      on an untouched copy of T, with delta succ_rs[j] = eq_rs[(j - 1) mod
 *      2^log_height] (mlh_eq_table of rs rotated by one row), the one
 *      constraint sum_k rand(k) var(c_k) of declared degree 1 (two
 *      coefficients per round), randoms lambda^0 .. lambda^(K-1) and mask [1]:
 *      shift_polys, the point rs' and output2 = T_j(rs'), j < W.  The
 *      verifier's final check is
 *        succ(rs, rs') sum_k lambda^k output2[c_k] = pol_last(r_last)
 *      with succ in closed form (mlh_shift_succ_evaluate);
 *   8. BatchedPCSProof::prove on commitment 1 at (rs, output[0:P]), if P < W
 *      on commitment 2 at (rs, output[P:W]); then, only if K > 0, on the same
 *      commitments in the same order at (rs', output2[0:P]) and (rs',
 *      output2[P:W]).  Both commitments are opened at rs' whether or not they
 *      hold a source column: one rule, no evaluation in the proof unbound.
 * With K = 0 the proof bytes and the final transcript state are
 * mlh_system_prove_phased's. */
/* dev_out (row-major 2^log_height x (width + n_shifts)) = the extension E of
 * the row-major 2^log_height x width dev_matrix, which is not modified.  Out of
 * place; width >= 1, width + n_shifts <= 32, log_height 0..32 (one row is its
 * own next row); MLH_ERR_INVALID for a null pointer, a source column at or above
 * width, overlapping buffers.  Duplicates are allowed here (the proof's list
 * must be distinct).  One kernel launch on the context stream. */
mlh_status mlh_trace_extend_next(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                 uint32_t width, const uint32_t* shift_columns, uint32_t n_shifts,
                                 void* dev_out);
/* Its launch shape: the rows of E a block writes per tile and the number of
 * blocks; a block visits ceil(tiles / blocks) tiles of tile_rows rows and
 * reads tile_rows + 1 rows of the trace for each. */
mlh_status mlh_trace_extend_next_launch_info(uint32_t log_height, uint32_t width, uint32_t n_shifts,
                                             uint32_t* tile_rows, uint32_t* blocks);
/* dev_out[j] = dev_in[(j - 1) mod 2^log_n], 2^log_n elements, out of place
 * (log_n 0..32): mlh_eq_table(x) -> the table of y -> succ(x, y). */
mlh_status mlh_eq_table_rotate(mlh_ctx* ctx, const void* dev_in, uint32_t log_n, void* dev_out);
/* succ(x, y) = sum_i eq(x, i) eq(y, (i + 1) mod 2^n) in O(n) field operations,
 * host only; x, y: n canonical elements each (n 0..64; n = 0 gives 1).  With
 * x_b the coordinate of bit b of the row index, bit b <-> point[n - 1 - b]
 * (Mask::evaluate's order, evaluation.rs:56-73):
 *   succ(x, y) = sum_{k<n} prod_{b<k} x_b (1 - y_b) * (1 - x_k) y_k
 *                * prod_{b>k} (x_b y_b + (1 - x_b)(1 - y_b))  +  prod_b x_b (1 - y_b)
 * (the carry of i + 1 stops at bit k; the last term is the wrap 2^n - 1 -> 0).
 * MLH_ERR_INVALID for a null pointer or a non-canonical element. */
mlh_status mlh_shift_succ_evaluate(const uint8_t* x, const uint8_t* y, uint32_t n, uint8_t out[16]);
typedef struct mlh_shifted_proof {
  uint32_t log_height, width /* W */, degree;
  uint32_t pre_random_columns; /* P */
  uint32_t sum_column_mask;    /* S, bit j = column j < W */
  uint32_t n_shifts;           /* K */
  uint32_t shift_columns[32];  /* c_0 .. c_{K-1}; the rest zero */
  uint8_t* sumcheck_polys;     /* [log_height][degree+1][16]                     */
  uint8_t* output;             /* [W + K][16]: row 0 of the folded extension     */
  uint8_t* shift_polys;        /* [log_height][2][16]; unused when K = 0         */
  uint8_t* output2;            /* [W][16] = Trace::evaluate(rs'); unused, K = 0  */
  /* caller-allocated as for mlh_phased_proof: pcs at rs, pcs_shift at rs'
   * (unused when K = 0); [1] unused when P = W */
  mlh_batched_pcs_proof pcs[2];
  mlh_batched_pcs_proof pcs_shift[2];
} mlh_shifted_proof;
/* The prover, steps 1-8.  prog: the W'-wide program; commitment1 / 2 as for
 * mlh_system_prove_phased over the W real columns (W = their widths' sum).
 * dev_matrix, the 2^log_height x W trace, is NOT modified: the extension, the
 * copy of step 7 and the two delta tables come from the context pool, where
 * they return on every path once the stream is drained (peak: (2 W + K + 2)
 * 2^log_height elements beside the handles).  Nothing is committed or encoded
 * a second time.  MLH_ERR_INVALID for a duplicate or out-of-range source column,
 * W + K other than the program's width or above 32, a sum-mask bit at or above
 * W, K > 0 with shift_columns, proof->shift_polys or proof->output2 null, and
 * every argument error of the phased call.  On any non-OK return the
 * transcript is exactly as at entry.  A trace that breaks a constraint is not
 * detected here: MLH_OK, and the verifier rejects. */
mlh_status mlh_system_prove_shifted(mlh_ctx* ctx, const mlh_cs_program* prog,
                                    const mlh_trace_commitment* commitment1,
                                    const mlh_trace_commitment* commitment2,
                                    uint32_t sum_column_mask, const uint32_t* shift_columns,
                                    uint32_t n_shifts, const void* dev_matrix,
                                    const uint8_t sum[16], const uint8_t column_sum[16],
                                    mlh_transcript* tr, mlh_shifted_proof* proof);
/* The verifier, host only, in the same order.  MLH_ERR_INVALID for a null
 * pointer or a shift list the prover would refuse; MLH_ERR_VERIFY, with the
 * transcript exactly as at entry, for any rejection, any disagreement between
 * the proof's header or shift list and the arguments, and any non-canonical
 * element.  On MLH_OK the transcript ends in the prover's state. */
mlh_status mlh_system_verify_shifted(const mlh_cs_program* prog, uint32_t log_height,
                                     uint32_t pre_random_columns, uint32_t sum_column_mask,
                                     const uint32_t* shift_columns, uint32_t n_shifts,
                                     const uint8_t sum[16], const uint8_t column_sum[16],
                                     const mlh_shifted_proof* proof, mlh_transcript* tr);

/* ---- public columns: selectors, constants and inputs the verifier derives ---- *
 * The last F columns of a W-wide trace, [W - F, W), are public: they have a
 * short description (the spec), the prover neither commits nor opens them, and
 * the verifier evaluates their multilinear extensions itself, in closed form.
 * The committed phases are [0, P) and [P, W - F).  A selector such as the wrap
 * gate `last` of (1 - last) * (next(a) - a - b), a public input tied to a row,
 * a round constant or the row index belongs here: as a committed column it is
 * the prover's to choose.
 *
 * Wire format of a spec (all integers little-endian u32 unless stated; elements
 * LE16 and canonical; 1 <= F <= 16):
 *   header   2 x u32: F, 0 (reserved)
 *   per column, in order: u32 kind, u32 arg, payload
 *     0 CONST     arg 0           1 element c             row i holds c
 *     1 FIRST     arg 0           -                       1 at row 0, else 0
 *     2 LAST      arg 0           -                       1 at row H - 1, else 0
 *     3 ROW       arg 0           -                       row i holds i
 *     4 PERIODIC  arg k (0..16)   2^k elements v          row i holds v[i mod 2^k]
 *     5 SPARSE    arg m (1..4096) m x (u64 row, element)  rows strictly increasing;
 *                                                         0 elsewhere
 * Exactly one byte string per spec: MLH_ERR_INVALID for an unknown kind, a
 * nonzero reserved word or arg (kinds 0-3), a non-canonical element, unsorted
 * or repeated sparse rows, a short buffer, trailing bytes.  Where the height
 * 2^L is known a spec must fit it, else MLH_ERR_INVALID: every PERIODIC k <= L
 * and every SPARSE row < 2^L.  The handle belongs to no context and is host
 * only. */
typedef struct mlh_public_columns mlh_public_columns;
mlh_status mlh_public_columns_create(const uint8_t* wire, uint64_t len, mlh_public_columns** out);
void mlh_public_columns_destroy(mlh_public_columns* spec);
uint32_t mlh_public_columns_count(const mlh_public_columns* spec); /* F; 0 for null */
/* SHA-256 of the wire bytes, computed once at create. */
mlh_status mlh_public_columns_digest(const mlh_public_columns* spec, uint8_t out[32]);
/* out[j] = the multilinear extension of column j over 2^log_height rows at
 * point (log_height canonical elements; log_height 0..32), host only, in
 * O(log H) field operations per column (PERIODIC: O(2^k); SPARSE: O(m log H)).
 * With x_b = point[log_height - 1 - b] the coordinate of bit b of the row
 * index (Mask::evaluate's order, evaluation.rs:56-73):
 *   CONST     c
 *   FIRST     prod_b (1 - x_b)
 *   LAST      prod_b x_b
 *   ROW       sum_b 2^b x_b
 *   PERIODIC  the extension of v at point[L - k : L], the 2^k-entry table folded
 *             in the same bit order; v[0] for k = 0
 *   SPARSE    sum_m v_m eq(point, row_m)
 * MLH_ERR_INVALID for a null pointer, a spec that does not fit log_height or a
 * non-canonical point. */
mlh_status mlh_public_columns_evaluate(const mlh_public_columns* spec, uint32_t log_height,
                                       const uint8_t* point, uint8_t* out);
/* Writes columns [width - F, width) of the row-major 2^log_height x width
 * dev_matrix in place and touches no other byte: a strip kernel (256 threads,
 * at most 1024 blocks, a block loops over tiles of tile_rows rows, 16-byte
 * stores in runs of 16 F bytes per row) and, with SPARSE columns, a scatter
 * kernel behind it on the context stream.  The periodic tables and sparse
 * entries reach the device once per call, through the context pool.  width
 * 1..32, F <= width, log_height 0..32 (with one row, that row is both first
 * and last); MLH_ERR_INVALID for a null pointer, these limits or a spec that
 * does not fit log_height, with the matrix untouched. */
mlh_status mlh_trace_fill_public(mlh_ctx* ctx, const mlh_public_columns* spec, void* dev_matrix,
                                 uint32_t log_height, uint32_t width);
/* Its launch shape for n_public = F columns: the rows a block writes per tile
 * (a power of two with tile_rows * F <= 2048, at most the height) and the
 * number of blocks; a block visits ceil(tiles / blocks) tiles. */
mlh_status mlh_trace_fill_public_launch_info(uint32_t log_height, uint32_t width, uint32_t n_public,
                                             uint32_t* tile_rows, uint32_t* blocks);
/* mlh_system_prove_shifted with public columns.  mlh_shifted_proof is reused
 * unchanged: width = W with the public columns included, output is [W + K],
 * output2 is [W].  Transcript order:
 *   0. only if F > 0: absorb the 32-byte digest of the spec;
 *   1-5. as mlh_system_prove_shifted; commitment1 covers [0, P), commitment2
 *      [P, W - F) and is null iff P = W - F: P1 + P2 + F = W, W the program's
 *      width minus K;
 *   6-7. unchanged: the sumcheck and the shift reduction run on all W columns; a
 *      public column may be a shift source or a sum column;
 *   8. the openings cover the committed columns only: output[0:P] on commitment
 *      1 and output[P:W-F] on commitment 2 at rs, and with K > 0 the same of
 *      output2 at rs'.
 * The verifier, after each sumcheck and before the openings, computes
 * mlh_public_columns_evaluate(spec, L, rs) and rejects unless it equals
 * output[W-F:W] element for element, and with K > 0 the same at rs' against
 * output2[W-F:W]: all F columns at both points, whether or not a constraint
 * reads them -- nothing in the proof stays unbound.  With spec null (F = 0) the
 * proof bytes and the final transcript state are mlh_system_prove_shifted's.
 * A caller who needs the trace randoms before phase 2
 * (mlh_system_trace_randoms) absorbs the digest into a clone of the transcript
 * first: the randoms are drawn behind step 0.
 *
 * The prover does not check that the strip of dev_matrix (see
 * mlh_trace_fill_public) equals the spec: like a broken constraint, a wrong
 * strip returns MLH_OK and the verifier rejects (mlh_trace_check and
 * mlh_trace_check_public say beforehand which constraint, which column and
 * which row).  MLH_ERR_INVALID, with the
 * transcript as at entry, for every argument error of the shifted call and for
 * F >= W, widths that do not add up (a commitment2 given although P = W - F
 * included) and a spec that does not fit the height. */
mlh_status mlh_system_prove_public(mlh_ctx* ctx, const mlh_cs_program* prog,
                                   const mlh_trace_commitment* commitment1,
                                   const mlh_trace_commitment* commitment2,
                                   uint32_t sum_column_mask, const uint32_t* shift_columns,
                                   uint32_t n_shifts, const mlh_public_columns* spec,
                                   const void* dev_matrix, const uint8_t sum[16],
                                   const uint8_t column_sum[16], mlh_transcript* tr,
                                   mlh_shifted_proof* proof);
/* The verifier, host only and trace-less, in the same order.  MLH_ERR_INVALID
 * for a null pointer, a shift list the prover would refuse, F >= W or a spec
 * that does not fit log_height; MLH_ERR_VERIFY for every rejection of the
 * proof, as mlh_system_verify_shifted.  In both cases the transcript is as at
 * entry; on MLH_OK it ends in the prover's state. */
mlh_status mlh_system_verify_public(const mlh_cs_program* prog, uint32_t log_height,
                                    uint32_t pre_random_columns, uint32_t sum_column_mask,
                                    const uint32_t* shift_columns, uint32_t n_shifts,
                                    const mlh_public_columns* spec, const uint8_t sum[16],
                                    const uint8_t column_sum[16], const mlh_shifted_proof* proof,
                                    mlh_transcript* tr);

/* ---- phase 2 on the device: fill programs and the column sum --------------- *
 * Between mlh_system_trace_randoms and mlh_trace_commit_range of the columns
 * at and above P the prover fills "the columns that you must fill" after
 * "knowing the value of the random challenges" (system.rs:23-26), e.g. u =
 * 1 / (gamma - a) of a lookup, and then needs the sum of the sum columns
 * (system.rs:27-29) for mlh_system_prove_phased.  Both run on the row-major
 * matrix in place, with no transpose and no host copy of a column.
 *
 * A fill program is a per-row straight-line program whose outputs are written
 * to columns of the same row: the constraint-program wire format above with
 *   header   7 x u32: width, n_randoms, n_consts, n_temps, n_instr,
 *            n_outputs, 0 (reserved)
 *   consts   as above
 *   code     as above, plus op 4 INV: temp[dst] = a^(M - 2), the inverse, zero
 *            -> zero (field.rs:113-118), b = (0, 0)
 *   outputs  n_outputs x 4 bytes: column, kind, index, 0: column `column` of
 *            the row receives the operand (kind, index)
 * and no degree.  Limits: those of constraint programs, n_outputs 1..width,
 * output columns distinct and below width, at most 16 INV, and inverse depth
 * 1: the operand of an INV may not depend on the result of an INV (a property
 * of the value, tracked through every temp write).  mlh_fill_program_create
 * returns MLH_ERR_INVALID for everything mlh_cs_program_create rejects
 * (which still rejects op 4) and for a nonzero reserved header word, a
 * duplicate or out-of-range output column, an INV with b != (0, 0), a 17th
 * INV and an INV of a value that depends on an INV.
 * Semantics: for every row, all column operands read the row as it stood when
 * the call began, then the outputs are stored: an output column may be read
 * (its old value is seen) and the columns that are no output are not written.
 * A program object is host memory only and may be used with any context. */
typedef struct mlh_fill_program mlh_fill_program;
mlh_status mlh_fill_program_create(const uint8_t* bytes, uint64_t len, mlh_fill_program** out);
void mlh_fill_program_destroy(mlh_fill_program* prog);
uint32_t mlh_fill_program_width(const mlh_fill_program* prog);
uint32_t mlh_fill_program_n_randoms(const mlh_fill_program* prog);
uint32_t mlh_fill_program_n_outputs(const mlh_fill_program* prog);
uint32_t mlh_fill_program_n_inverses(const mlh_fill_program* prog);
uint32_t mlh_fill_program_output_mask(const mlh_fill_program* prog); /* bit j: column j is written */
/* The host interpreter, the specification of mlh_trace_fill: out_row (width
 * elements) = host_row (width canonical elements) after the fill.  Host only. */
mlh_status mlh_fill_program_evaluate(const mlh_fill_program* prog, const uint8_t* host_row,
                                     const uint8_t* host_randoms, uint8_t* out_row);
/* The program on every row of the 2^log_height x width device matrix, in
 * place (log_height 0..32).  width must equal the program's; host_randoms:
 * n_randoms canonical elements, NULL allowed when 0.  One kernel launch on the
 * context stream behind one copy of the randoms, constants and code; the call
 * does not wait for the kernel.  A lane inverts once per INV for
 * rows_per_thread of its rows (Montgomery's trick): 3 + 138 / rows_per_thread
 * products per row and INV, the prefix products in a pooled scratch buffer of
 * at most 64 MiB. */
mlh_status mlh_trace_fill(mlh_ctx* ctx, const mlh_fill_program* prog, void* dev_matrix,
                          uint32_t log_height, uint32_t width, const uint8_t* host_randoms);
/* Its launch shape: threads per block (the largest of 256, 128, 64 whose
 * width + n_temps + n_inverses LDS slots of 16 bytes fit 152 KiB), rows per
 * thread and inversion (the largest of 16, 8, 4, 2, 1 that leaves 512 chunks;
 * 1 without an INV) and blocks; a block visits ceil(ceil(2^log_height /
 * (threads * rows_per_thread)) / blocks) chunks of threads * rows_per_thread
 * rows. */
mlh_status mlh_trace_fill_launch_info(const mlh_fill_program* prog, uint32_t log_height,
                                      uint32_t* threads, uint32_t* rows_per_thread,
                                      uint32_t* blocks);
/* mlh_trace_fill under another launch shape, for measurements: threads 64, 128
 * or 256, rows_per_thread a power of two up to 16 (1 for a program without
 * INV); MLH_ERR_INVALID when (width + n_temps + n_inverses) * 16 * threads
 * exceeds 152 KiB of LDS.  The same bytes as mlh_trace_fill. */
mlh_status mlh_trace_fill_shaped(mlh_ctx* ctx, const mlh_fill_program* prog, void* dev_matrix,
                                 uint32_t log_height, uint32_t width, const uint8_t* host_randoms,
                                 uint32_t threads, uint32_t rows_per_thread);
/* out = sum_i sum_{j in column_mask} matrix[i * width + j]: the column_sum of
 * mlh_system_prove_phased ("the sum of all sum columns", system.rs:27-29).
 * width 1..32, log_height 0..32; a mask bit at or above width is
 * MLH_ERR_INVALID, mask 0 gives zero.  One streaming pass and a one-block
 * reduction; synchronises once to return the value. */
mlh_status mlh_trace_column_sum(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                uint32_t width, uint32_t column_mask, uint8_t out[16]);

/* ---- running sums and running products on the device ------------------------ *
 * The column that a next-row constraint next(z) = z * t or next(z) = z + t
 * holds (the grand product of a permutation or multiset argument, a memory
 * accumulator, the running sum of a log-derivative bus) is a prefix scan over
 * the 2^log_height rows.  This call writes up to 8 of them in place, with no
 * host copy of a column.
 * For scan s let t[i] = matrix[i][src_columns[s]] as the matrix stood when the
 * call began, o = + (MLH_SCAN_ADD) or * (MLH_SCAN_MUL) in the field and init_s =
 * host_inits[16 s ..].  After the call, with H = 2^log_height,
 *   z[0] = init_s,  z[i + 1] = z[i] o t[i],
 *   matrix[i][dst_columns[s]] = z[i] for every i < H,
 *   totals_out[16 s ..] = z[H - 1] o t[H - 1]:
 * the exclusive scan, the column that first * (z - init) and next(z) - z o t
 * constrain; the total is the value across the cyclic wrap, so next(z) = z o t
 * holds on the last row without a (1 - last) gate exactly when total_s ==
 * init_s (a grand product that closes to 1).  The inclusive form is one
 * row-local fill on top (z o t, mlh_trace_fill); there is no flag for it.
 * dst may equal src (in place), a destination may be the source of another
 * scan (which still sees the old values), two scans may share a source;
 * destination columns must be distinct, and the columns that are no
 * destination are not written.
 * width 1..32, log_height 0..32, n_scans 1..8, ops 0 or 1, columns below width,
 * inits canonical.  Anything else and a NULL pointer (totals_out excepted) is
 * MLH_ERR_INVALID before anything is enqueued: the matrix is untouched.
 * Three launches on the context stream, none of which waits for another
 * workgroup: the blocks' aggregates, their exclusive scan seeded with the
 * inits (one block), and the scan of each block's rows behind its offset; one
 * launch when there is one block.  The field operations are exact and
 * associative: the bytes do not depend on the launch shape.  With totals_out
 * == NULL the call does not wait for the device; otherwise it synchronises
 * once to return the totals, as mlh_trace_column_sum does. */
#define MLH_SCAN_ADD 0
#define MLH_SCAN_MUL 1
mlh_status mlh_trace_scan(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height, uint32_t width,
                          uint32_t n_scans, const uint8_t* ops, const uint8_t* src_columns,
                          const uint8_t* dst_columns, const uint8_t* host_inits /* n_scans x 16 */,
                          uint8_t* totals_out /* n_scans x 16, or NULL */);
/* Its launch shape: threads per block (256), consecutive rows per thread (4)
 * and blocks (min(ceil(2^log_height / (threads * rows_per_thread)), 1024)); a
 * block takes ceil(tiles / blocks) consecutive tiles of threads *
 * rows_per_thread rows, the last blocks fewer or none.  The limits of
 * mlh_trace_scan. */
mlh_status mlh_trace_scan_launch_info(uint32_t log_height, uint32_t width, uint32_t n_scans,
                                      uint32_t* threads, uint32_t* rows_per_thread,
                                      uint32_t* blocks);
/* The same kernels and the same bytes under another shape, for tests of the
 * seams at small heights and for measurements: threads 64, 128 or 256,
 * rows_per_thread a power of two up to 16, max_blocks 1..1024 (the grid is
 * min(tiles, max_blocks) blocks); MLH_ERR_INVALID otherwise. */
mlh_status mlh_trace_scan_shaped(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                 uint32_t width, uint32_t n_scans, const uint8_t* ops,
                                 const uint8_t* src_columns, const uint8_t* dst_columns,
                                 const uint8_t* host_inits, uint8_t* totals_out, uint32_t threads,
                                 uint32_t rows_per_thread, uint32_t max_blocks);

/* ---- sorted copies of columns on the device ---------------------------------- *
 * The log of a memory-consistency argument in address-then-timestamp order, the
 * sorted column of a range check by differences, the second side of a multiset
 * argument "the same rows, ordered": a sorted copy of columns, written in place
 * with no host copy of a column.
 * Let H = 2^log_height and key(i) the tuple of the 16-byte elements
 * matrix[i][key_columns[0 .. n_keys - 1]] as the matrix stood when the call
 * began, each read as an unsigned 128-bit little-endian integer (canonical
 * input is the caller's contract, as in the lookup calls; the order is that of
 * the 16 bytes as an integer).  pi is the one permutation of 0..H-1 with
 * key(pi(0)) <= key(pi(1)) <= ... lexicographically, key_columns[0] the most
 * significant, and pi(r) < pi(r + 1) wherever the keys are equal: the stable
 * ascending sort.  There is no descending flag.  After the call, for r < H,
 *   matrix[r][dst_columns[s]] = old matrix[pi(r)][src_columns[s]], s < n_copies;
 *   matrix[r][perm_column]    = pi(r) as a canonical element, when perm_column
 *                               is not MLH_SORT_NO_COLUMN: the index column that
 *                               a permutation argument over (value, row) pairs
 *                               needs;
 *   *passes_out               = the number of digit passes that ran (below);
 * and no other byte of the matrix is written.  A key column may also be a
 * source (the usual case) and a source may repeat.  Destination columns and
 * perm_column are pairwise distinct and disjoint from every key and source
 * column, so the gather is in place with no staging copy.  The result is a pure
 * function of the matrix and the column lists: it does not depend on the launch
 * shape.
 * width 1..32, log_height 0..28 (row indices are 32-bit, as in
 * mlh_trace_lookup_counts), n_keys 1..4, n_copies 0..16, and at least one
 * output: n_copies > 0 or a perm_column.  A column at or above width, an
 * overlap that the rules above forbid, a limit exceeded and a NULL ctx,
 * dev_matrix, key_columns, or src_columns / dst_columns with n_copies > 0, are
 * MLH_ERR_INVALID before anything is enqueued: the matrix is untouched.
 * passes_out may be NULL.
 * An LSD radix sort with 8-bit digits over (32-bit key limb, row index) pairs,
 * every step a launch on the context stream, none of which waits for another
 * workgroup.  A digit census (one pass over the key columns: LDS tables per
 * block, one 32-bit atomic add per non-empty bin) counts all 16 n_keys digits
 * at once; the call then synchronises once to learn which digits all H rows
 * agree in, and skips those (keys below 2^32 leave at most 4 of a key's 16
 * passes; H = 1 or all keys equal leave none, and the gather alone runs with
 * pi the identity).  A limb is gathered from the matrix once and serves its up
 * to four digit passes; a pass is a per-block histogram, a one-block exclusive
 * scan of the blocks x 256 table in digit-major order behind the census's digit
 * starts, and a stable scatter (a block walks its consecutive tiles in order,
 * ranks by wave ballots); one last launch gathers the copies with 16-byte loads
 * and stores.  Scratch, pooled: 16 bytes per row (two arrays of pairs), 16 KiB
 * per key (the census), 2 KiB per block and 256 bytes. */
#define MLH_SORT_MAX_KEYS   4
#define MLH_SORT_MAX_COPIES 16
#define MLH_SORT_NO_COLUMN  0xFFFFFFFFu
mlh_status mlh_trace_sort(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height, uint32_t width,
                          uint32_t n_keys, const uint32_t* key_columns /* most significant first */,
                          uint32_t n_copies, const uint32_t* src_columns,
                          const uint32_t* dst_columns,
                          uint32_t perm_column /* or MLH_SORT_NO_COLUMN */,
                          uint32_t* passes_out /* or NULL */);
/* Its launch shape: threads per block (256), rows per thread (8) and blocks
 * (min(ceil(2^log_height / (threads * rows_per_thread)), 1024)); a block takes
 * ceil(tiles / blocks) consecutive tiles of threads * rows_per_thread rows, the
 * last blocks fewer or none.  In a tile a wave owns 64 * rows_per_thread
 * consecutive rows and lane j of it the rows j, j + 64, ...  width 1..32,
 * log_height 0..28, n_keys 1..4. */
mlh_status mlh_trace_sort_launch_info(uint32_t log_height, uint32_t width, uint32_t n_keys,
                                      uint32_t* threads, uint32_t* rows_per_thread,
                                      uint32_t* blocks);
/* The same kernels and the same bytes under another shape, for tests of the
 * seams at small heights and for measurements: threads 64, 128 or 256,
 * rows_per_thread a power of two up to 16, max_blocks 1..1024 (the grid is
 * min(tiles, max_blocks) blocks).  flags bit 0: run every digit pass, skip
 * none (*passes_out = 16 n_keys; the call then does not wait for the device);
 * any other bit, and any other shape, is MLH_ERR_INVALID. */
mlh_status mlh_trace_sort_shaped(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                 uint32_t width, uint32_t n_keys, const uint32_t* key_columns,
                                 uint32_t n_copies, const uint32_t* src_columns,
                                 const uint32_t* dst_columns, uint32_t perm_column,
                                 uint32_t* passes_out, uint32_t threads, uint32_t rows_per_thread,
                                 uint32_t max_blocks, uint32_t flags);

/* ---- the witness check on the device ---------------------------------------- *
 * The provers do not detect a trace that breaks a constraint or a public strip
 * that differs from its spec: they return MLH_OK and the verifier rejects.
 * These calls tell the caller beforehand which constraint fails, on how many
 * rows and where first, with no host copy of the trace.
 *
 * mlh_trace_check runs every constraint of `prog` (constraints.rs:3-10: an
 * expression of the row and the randoms that must be zero) on every row, each
 * on its own and without the constraint mask of evaluation.rs:21-29.  With H =
 * 2^log_height, W = width and K = n_shifts source columns, as
 * mlh_system_prove_shifted takes them, the program is W + K wide; on row i its
 * column operand j < W is matrix[i][j] and column operand W + k is
 * matrix[(i + 1) mod H][shift_columns[k]].  No extension is materialised.
 * Constraint c fails on row i when its output there is not the field's zero.
 *   counts_out[c]     = the number of rows on which c fails;
 *   first_rows_out[c] = the lowest such row, UINT64_MAX when there is none;
 *   report            = as commented in the struct.
 * The constraint mask and the delta table play no part, so the check can run
 * before any commitment exists (the randoms are whatever the caller will
 * prove with).  The matrix is not written.  The result is a pure function of
 * the matrix, the program, the randoms and the shift list: it does not depend
 * on the launch shape or on the order of the atomics (only integer adds and
 * mins cross lanes).
 * width 1..32, width + n_shifts equal to the program's width and at most 32,
 * log_height 0..32 (one row is its own next row, as in mlh_trace_extend_next);
 * source columns below width, duplicates allowed here as in
 * mlh_trace_extend_next; randoms canonical, host_randoms may be NULL when the
 * program has none.  Anything else and a NULL ctx, prog, dev_matrix or report
 * is MLH_ERR_INVALID: nothing is enqueued and the outputs stay untouched.  A
 * failing trace is MLH_OK.
 * One launch: a block takes chunks of `threads` consecutive rows, loads them
 * coalesced into LDS (width + n_shifts + temps slots of 16 bytes per lane),
 * takes the next row's operands from the neighbouring lane -- the chunk's last
 * lane from global memory, across the cyclic wrap behind the last row --
 * interprets the program once per row and reduces the verdicts with wave
 * ballots, per-block LDS counters and 64-bit atomics into a pooled array that
 * the call zeroes on the stream first.  No workgroup waits for another.
 * Synchronises once to return the counters, as mlh_trace_lookup_counts does. */
typedef struct mlh_trace_check_report {
  uint64_t n_bad_rows;           /* rows on which at least one constraint is nonzero */
  uint64_t first_bad_row;        /* the lowest of them; UINT64_MAX when none         */
  uint32_t first_bad_constraint; /* the lowest constraint that is nonzero on that row;
                                    UINT32_MAX when none                             */
  uint32_t reserved;             /* 0 */
} mlh_trace_check_report;
mlh_status mlh_trace_check(mlh_ctx* ctx, const mlh_cs_program* prog, const void* dev_matrix,
                           uint32_t log_height, uint32_t width,
                           const uint32_t* shift_columns, uint32_t n_shifts,
                           const uint8_t* host_randoms,
                           uint64_t* counts_out /* [n_constraints] or NULL */,
                           uint64_t* first_rows_out /* [n_constraints] or NULL */,
                           mlh_trace_check_report* report);
/* Its launch shape: threads per block (the largest of 256, 128, 64 whose
 * program width + n_temps LDS slots of 16 bytes fit 152 KiB) and blocks
 * (min(ceil(2^log_height / (threads * 4)), 1024), each looping over chunks of
 * `threads` rows with the grid's stride).  log_height 0..32. */
mlh_status mlh_trace_check_launch_info(const mlh_cs_program* prog, uint32_t log_height,
                                       uint32_t* threads, uint32_t* blocks);
/* The same kernel and the same counters under another shape, for tests of the
 * seams at small heights and for measurements: threads 64, 128 or 256,
 * max_blocks 1..1024 (the grid is min(ceil(2^log_height / threads),
 * max_blocks) blocks); MLH_ERR_INVALID otherwise and when the slots do not fit
 * 152 KiB of LDS at that block size. */
mlh_status mlh_trace_check_shaped(mlh_ctx* ctx, const mlh_cs_program* prog, const void* dev_matrix,
                                  uint32_t log_height, uint32_t width,
                                  const uint32_t* shift_columns, uint32_t n_shifts,
                                  const uint8_t* host_randoms, uint64_t* counts_out,
                                  uint64_t* first_rows_out, mlh_trace_check_report* report,
                                  uint32_t threads, uint32_t max_blocks);
/* The public strip against its spec.  With F the spec's columns,
 *   counts_out[j]     = the number of rows i where matrix[i][width - F + j]
 *                       differs in its 16 bytes from what mlh_trace_fill_public
 *                       would write there;
 *   first_rows_out[j] = the lowest such row, UINT64_MAX when there is none;
 *   *n_bad_rows       = the rows with a difference in any of the F columns,
 *   *first_bad_row    = the lowest of them, UINT64_MAX when there is none.
 * counts_out and first_rows_out ([F]) may be NULL.  The limits and argument
 * errors of mlh_trace_fill_public, and MLH_ERR_INVALID for a NULL n_bad_rows
 * or first_bad_row; no byte of the matrix is written, and a committed column
 * is not looked at.  The tiling and the expected values of
 * mlh_trace_fill_public, loads and a compare where that call stores; the
 * expected value of a SPARSE column's element by a binary search over the
 * column's entries (at most 12 steps); the reduction of mlh_trace_check.  A
 * pure function of the matrix and the spec.  Synchronises once. */
mlh_status mlh_trace_check_public(mlh_ctx* ctx, const mlh_public_columns* spec,
                                  const void* dev_matrix, uint32_t log_height, uint32_t width,
                                  uint64_t* counts_out /* [F] or NULL */,
                                  uint64_t* first_rows_out /* [F] or NULL */,
                                  uint64_t* n_bad_rows, uint64_t* first_bad_row);

/* ---- a lookup's multiplicities on the device -------------------------------- *
 * The multiplicity column m of a log-derivative lookup (v = -m / (gamma - t))
 * is a pre-random column: it must stand in the matrix before
 * mlh_trace_commit_range of the first column range.  This call counts it in
 * place, with no host copy of a column.
 * Let key(j) = matrix[j][table_column] as 16 bytes; row j is the owner of its
 * key when no lower row has the same key.  After the call
 *   matrix[j][count_column] = the number of pairs (i, c), c in
 *     value_column_mask, with matrix[i][c] == key(j), as a canonical element,
 *     when j is an owner, and zero otherwise (a table padded by repeating an
 *     entry: the lowest row takes the whole count);
 *   *n_missing = the number of pairs (i, c) whose value equals no table entry;
 *   *first_missing_row = the lowest such i, UINT64_MAX when there is none;
 * and no other column is written.  A missing value is no error: MLH_OK, and
 * the counts of the values that were found are right.  Equality is equality of
 * the 16 bytes (canonical inputs are the caller's contract).  The result is a
 * pure function of the matrix: it does not depend on the launch shape, on where
 * the hash puts a key or on the order of the atomics.
 * width 1..32, log_height 0..28 (row indices are 32-bit with one value
 * reserved).  MLH_ERR_INVALID for an empty mask, a mask bit, table_column or
 * count_column at or above width, table_column == count_column, either of them
 * in the mask, and NULL pointers; the matrix is then untouched.
 * A hash join with open addressing over row indices in a pooled scratch array
 * of 2^log_slots 32-bit slots, log_slots = log_height + 2 (16 bytes per row):
 * one launch inserts the table rows (and zeroes the count column), a second
 * counts one (row, value column) pair per thread with a 64-bit atomic add into
 * the owner's count element, the lanes of a wave that found the same owner
 * combined and kept in a per-wave cache so that a few hot entries cost one add
 * per wave.  Every probe loop is bounded by the number of slots.  Both
 * launches: 256 threads, min(ceil(work / 256), 1024) blocks looping with the
 * grid's stride, work = 2^log_height rows, times the number of value columns
 * for the count.  Synchronises once to return the two counters. */
mlh_status mlh_trace_lookup_counts(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                   uint32_t width, uint32_t value_column_mask,
                                   uint32_t table_column, uint32_t count_column,
                                   uint64_t* n_missing, uint64_t* first_missing_row);
/* Its launch shape: threads per block (256), blocks of the count launch
 * (min(ceil(2^log_height * n_value_columns / 256), 1024)) and log_slots
 * (log_height + 2).  n_value_columns 1..30, log_height 0..28. */
mlh_status mlh_trace_lookup_counts_launch_info(uint32_t log_height, uint32_t n_value_columns,
                                               uint32_t* threads, uint32_t* blocks,
                                               uint32_t* log_slots);
/* The same bytes under another shape, for tests of the probe paths at small
 * heights and for measurements.  log_slots log_height..31; hash_bits 0..
 * log_slots keeps that many low bits of the slot hash (0: every key starts at
 * slot 0 and the table is one probe chain); max_blocks caps both grids (0: the
 * rule above); flags bit 0 turns the wave-level combining off (one atomic per
 * lane), every other bit is MLH_ERR_INVALID, as are log_slots and hash_bits
 * outside those ranges.  With log_slots == log_height and distinct keys the
 * slot array is full and a missing value ends at the probe bound. */
mlh_status mlh_trace_lookup_counts_shaped(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                          uint32_t width, uint32_t value_column_mask,
                                          uint32_t table_column, uint32_t count_column,
                                          uint64_t* n_missing, uint64_t* first_missing_row,
                                          uint32_t log_slots, uint32_t hash_bits,
                                          uint32_t max_blocks, uint32_t flags);

/* ---- tuple lookups: multi-column multiplicities on the device --------------- *
 * The lookups of a real trace have tuple keys: a 4-bit XOR table is the triple
 * (x, y, x ^ y), a tagged range table a pair.  Phase 2 compresses a tuple with
 * a trace random (a + alpha * b + alpha^2 * c) and inverts gamma - that; the
 * multiplicity column is pre-random and must count the tuples themselves
 * (counting per column is wrong: every component of (3, 5, 7) can occur in its
 * own table column while the triple occurs in no table row).  This is the
 * owner rule of mlh_trace_lookup_counts with a tuple in place of an element
 * (DESIGN.md 6h).
 * Let key(j) = the 16 * arity bytes matrix[j][table_columns[0]] || ... ||
 * matrix[j][table_columns[arity - 1]]; row j is the owner of its key when no
 * lower row has the same key.  Let value(i, l) = the same concatenation over
 * value_columns[l * arity + 0 .. arity - 1] of row i (value_columns is
 * [n_tuples][arity], tuple-major).  A pair (i, l) is enabled when
 * selector_columns is NULL, or selector_columns[l] is MLH_LOOKUP_NO_SELECTOR,
 * or the 16 bytes of matrix[i][selector_columns[l]] are not all zero.  After
 * the call
 *   matrix[j][count_column] = the number of enabled pairs (i, l) with
 *     value(i, l) == key(j), as a canonical element, when j is an owner, and
 *     zero otherwise (the lowest row of a repeated key takes the whole count);
 *   *n_missing = the number of enabled pairs whose value equals no key;
 *   *first_missing_row = the lowest such i, UINT64_MAX when there is none;
 * and no other column is written.  A missing tuple is no error: MLH_OK, and
 * the counts of the tuples that were found are right.  A disabled pair is
 * neither counted nor missing.  The order of the components matters: (x, y)
 * and (y, x) are different keys.  Equality is equality of the bytes.  The
 * result is a pure function of the matrix and the column lists: it does not
 * depend on the launch shape, on where the hash puts a key or on the order of
 * the atomics.
 * width 1..32, log_height 0..28, arity 1..MLH_LOOKUP_MAX_ARITY, n_tuples
 * 1..MLH_LOOKUP_MAX_TUPLES, arity * n_tuples <= 32.  MLH_ERR_INVALID, the
 * matrix untouched, for anything outside these, a NULL ctx, dev_matrix,
 * table_columns, value_columns, n_missing or first_missing_row, a column at
 * or above width (a selector other than MLH_LOOKUP_NO_SELECTOR included), two
 * equal table columns, a value column that is a table column, and
 * count_column among the table, value or selector columns.  A value column
 * may repeat within a tuple and across tuples ((x, y, z) and (y, x, z) of a
 * commutative table share all three), and a selector may be any column but
 * the count column.
 * The hash join of mlh_trace_lookup_counts: the slot array holds row indices,
 * the hash is MurmurHash3 x86_32 over the 4 * arity limbs in component order
 * with the length word 16 * arity (at arity 1 the one-column entry's hash),
 * and a visited slot's row is compared component by component, ending at the
 * first that differs.  One kernel instance per arity keeps the thread's tuple
 * in registers; the value and selector columns stand behind the counters in
 * the 256-byte header of the pooled scratch array, and a wave, whose 64 pairs
 * are always of one tuple, reads its tuple's with scalar loads.  Both
 * launches: 256 threads, min(ceil(work / 256), 1024) blocks looping with the
 * grid's stride, work = 2^log_height rows for the insert and n_tuples *
 * 2^log_height pairs for the count, log_slots = log_height + 2.  Synchronises
 * once to return the two counters. */
#define MLH_LOOKUP_MAX_ARITY 8
#define MLH_LOOKUP_MAX_TUPLES 16
#define MLH_LOOKUP_NO_SELECTOR 0xFFFFFFFFu
mlh_status mlh_trace_lookup_tuple_counts(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                         uint32_t width, uint32_t arity,
                                         const uint32_t* table_columns, uint32_t n_tuples,
                                         const uint32_t* value_columns,
                                         const uint32_t* selector_columns, uint32_t count_column,
                                         uint64_t* n_missing, uint64_t* first_missing_row);
/* Its launch shape: threads per block (256), blocks of the count launch
 * (min(ceil(2^log_height * n_tuples / 256), 1024)) and log_slots (log_height +
 * 2).  n_tuples 1..16, log_height 0..28. */
mlh_status mlh_trace_lookup_tuple_counts_launch_info(uint32_t log_height, uint32_t n_tuples,
                                                     uint32_t* threads, uint32_t* blocks,
                                                     uint32_t* log_slots);
/* The same bytes under another shape: log_slots, hash_bits, max_blocks and
 * flags as mlh_trace_lookup_counts_shaped takes them (flags bit 0 turns the
 * wave-level combining off, every other bit is MLH_ERR_INVALID). */
mlh_status mlh_trace_lookup_tuple_counts_shaped(mlh_ctx* ctx, void* dev_matrix,
                                                uint32_t log_height, uint32_t width,
                                                uint32_t arity, const uint32_t* table_columns,
                                                uint32_t n_tuples, const uint32_t* value_columns,
                                                const uint32_t* selector_columns,
                                                uint32_t count_column, uint64_t* n_missing,
                                                uint64_t* first_missing_row, uint32_t log_slots,
                                                uint32_t hash_bits, uint32_t max_blocks,
                                                uint32_t flags);

/* ---- multilinear PCS (src/fri/multilinear_pcs.rs) ------------------------ */
typedef struct mlh_pcs_proof {
  mlh_fri_proof fri;
  uint8_t* sumcheck_polys; /* [n_vars][2][16] nonzero coefficients c1, c2 */
} mlh_pcs_proof;
/* PCSProof::prove (multilinear_pcs.rs:90-136): dev_evals (2^n_vars elements)
 * is not modified; host_inputs: n_vars points; output: the claimed value. */
mlh_status mlh_pcs_prove(mlh_ctx* ctx, const void* dev_evals, uint32_t n_vars,
                         const uint8_t* host_inputs, const uint8_t output[16], mlh_transcript* tr,
                         mlh_pcs_proof* proof);
/* PCSProof::verify (multilinear_pcs.rs:138-190), host side.  A sumcheck
 * coefficient, last_elem or an opened leaf element >= M: MLH_ERR_VERIFY, as
 * mlh_fri_verify (typed ReedSolomonPair<F>, fri/mod.rs:177-236).  host_inputs
 * and output are the caller's and are not range-checked here. */
mlh_status mlh_pcs_verify(const mlh_pcs_proof* proof, uint32_t n_vars, const uint8_t* host_inputs,
                          const uint8_t output[16], mlh_transcript* tr);

/* ---- multi-GPU: one process per GPU -------
 * The reference has no distributed API; these run its NTT / reed_solomon /
 * FriProof::prove / sumcheck on P = 2^p ranks.  Exchanges go through a
 * transport: the built-in one is RCCL over xGMI (mlh_comm: rank 0 calls
 * mlh_comm_unique_id and sends the 128 bytes to the other ranks out of band,
 * every rank calls mlh_comm_create); a caller may supply its own (e.g. over
 * host memory; host_side = 1 makes the library drain its stream before each
 * call).  Every rank calls the same entry point with its shard; collectives
 * are enqueued on the context stream.
 * Layout of a sharded 2^log_n vector: block-cyclic with block 2^log_s, local
 * index l of rank r = global ((l >> log_s) << (log_s + p)) | (r << log_s) |
 * (l mod 2^log_s); "cyclic" = log_s 0. */
typedef int (*mlh_all_to_all_fn)(void* user, const void* dev_send, void* dev_recv,
                                 uint64_t bytes_per_rank, void* hip_stream);
typedef int (*mlh_all_gather_fn)(void* user, const void* dev_send, void* dev_recv, uint64_t bytes,
                                 void* hip_stream);
typedef struct mlh_transport {
  uint32_t world;     /* P, a power of two <= 16                                */
  uint32_t rank;      /* this process                                           */
  uint32_t host_side; /* 1: callbacks complete on the host (stream drained first) */
  void* user;
  /* chunk i (bytes_per_rank) of dev_send goes to rank i; chunk i of dev_recv came from rank i */
  mlh_all_to_all_fn all_to_all;
  /* dev_recv = every rank's dev_send (bytes each), in rank order */
  mlh_all_gather_fn all_gather;
} mlh_transport;
typedef struct mlh_comm mlh_comm;
mlh_status mlh_comm_unique_id(uint8_t out[128]);
mlh_status mlh_comm_create(mlh_ctx* ctx, uint32_t world, uint32_t rank, const uint8_t id[128],
                           mlh_comm** out);
void mlh_comm_destroy(mlh_comm* comm);
mlh_status mlh_comm_transport(mlh_comm* comm, mlh_transport* out);
/* What RCCL itself reports for the communicator (ncclCommCount,
 * ncclCommUserRank, ncclCommCuDevice): the ranks it connected, this rank, and
 * its device -- the self-check a multi-GPU run prints. */
mlh_status mlh_comm_info(mlh_comm* comm, uint32_t* count, uint32_t* rank, int* device);
/* Transport pre-flight (no reference counterpart): one all-to-all of
 * P x bytes_per_rank and one all-gather of bytes_per_rank through `tp`, each
 * word a function of (source rank, destination rank, position), checked on the
 * device.  *mismatches = the words this rank received wrong (0 on a sound
 * transport); *ms (optional) = the two collectives' duration on the context
 * stream.  Run it before the first data-path collective of a multi-GPU job. */
mlh_status mlh_comm_preflight(mlh_ctx* ctx, const mlh_transport* tp, uint64_t bytes_per_rank,
                              uint64_t* mismatches, float* ms);
/* Polynomial::ntt / LagrangePolynomial::intt (ntt/mod.rs:69-173) of a 2^log_n
 * vector: forward takes the cyclic layout (2^log_n / P local elements) and
 * returns block 2^log_n / P^2; inverse != 0 the reverse.  One all-to-all. */
mlh_status mlh_sharded_ntt(mlh_ctx* ctx, const mlh_transport* tp, const void* dev_in, void* dev_out,
                           uint32_t log_n, const uint8_t gen[16], int inverse);
/* count sharded NTTs (or INTTs) of 2^log_n vectors, dev_in[i] -> dev_out[i]
 * with mlh_sharded_ntt's layouts, pipelined on two streams: the all-to-all of
 * transform i (and the local step after it) runs on the context's second
 * stream while the first local step of transform i + 1 runs on the context
 * stream.  On return the context stream is ordered after all of them.  This is
 * Polynomial::ntt (ntt/mod.rs:69-110) called on count polynomials in turn. */
mlh_status mlh_sharded_ntt_batch(mlh_ctx* ctx, const mlh_transport* tp, const void* const* dev_in,
                                 void* const* dev_out, uint32_t count, uint32_t log_n,
                                 const uint8_t gen[16], int inverse);
/* The same forward transforms with the rank digit fused into the last pass:
 * the local passes but the last, ONE all-to-all, one pass over the received
 * chunks -- three HBM passes per element instead of the local NTT's three plus
 * the cross-shard DFT's.  Input cyclic (rank g holds x[g + P m]);
 * output block-cyclic with block 2^(*log_s_out) (the plan's first digit minus
 * log2 P: 6 at 2^27 over 8 ranks), i.e. local l of rank r is global
 * ((l >> s) << (s + p)) | (r << s) | (l mod 2^s).  2 <= P <= 8; local size
 * >= 2^(13 - log2 P).  Pipelined on three streams like mlh_sharded_ntt_batch. */
mlh_status mlh_sharded_ntt_fused_batch(mlh_ctx* ctx, const mlh_transport* tp, const void* const* dev_in,
                                       void* const* dev_out, uint32_t count, uint32_t log_n,
                                       const uint8_t gen[16], uint32_t* log_s_out);
/* reed_solomon (fri/mod.rs:19-28): 2^log_n coefficients in the cyclic layout,
 * gen of order 2^(log_n + 1) -> the codeword in block 2^(log_n + 1) / P^2. */
mlh_status mlh_sharded_reed_solomon(mlh_ctx* ctx, const mlh_transport* tp, const void* dev_coeffs,
                                    uint32_t log_n, const uint8_t gen[16], void* dev_code);
/* commit_rs_code (fri/mod.rs:45-55) + Merkle::commit (merkle_tree/mod.rs:65-85)
 * of a 2^log_code codeword in the block 2^log_code / P^2 layout: local leaves
 * and subtrees, one all-gather of the subtree roots, the top levels on every
 * rank; root_out (host) = the root of the natural-order codeword's tree. */
mlh_status mlh_sharded_commit_rs_code(mlh_ctx* ctx, const mlh_transport* tp, const void* dev_code,
                                      uint32_t log_code, uint8_t root_out[32]);
/* FriProof::prove (fri/mod.rs:261-285) of a 2^log_code codeword in the block
 * 2^log_code / P^2 layout (mlh_sharded_reed_solomon's output); layers below
 * 2^gather_log entries are gathered and finished replicated (16 is a good
 * value).  Every rank returns the same proof: byte-identical to mlh_fri_prove
 * of the natural-order codeword. */
mlh_status mlh_sharded_fri_prove(mlh_ctx* ctx, const mlh_transport* tp, const void* dev_code,
                                 uint32_t log_code, uint32_t gather_log, mlh_transcript* tr,
                                 mlh_fri_proof* proof);
/* build_tables_for_pcs's delta (sumcheck.rs:128-145) in the cyclic layout:
 * rank r gets delta[l P + r], l < 2^(n - p). */
mlh_status mlh_sharded_eq_table(mlh_ctx* ctx, const mlh_transport* tp, const uint8_t* points,
                                uint32_t n, void* dev_out);
/* compute_sumcheck_polynomials (sumcheck.rs:77-102), composition x[0], of
 * tables in the cyclic layout; polys_out [n][2][16], rs_out [n][16] as
 * mlh_sumcheck_prove.  The local tables are folded in place while they hold
 * >= 2 entries (the last log2 P rounds fold gathered copies); on return entry
 * 0 of every rank's dev_m / dev_d holds the fully folded m(r) / d(r), the
 * length-1 tables the reference ends with.  The RCCL transport (mlh_comm) at
 * P > 1 has run only on the driver's multi-GPU node; the tests drive these
 * entry points at P > 1 through a host-side transport. */
mlh_status mlh_sharded_sumcheck_prove(mlh_ctx* ctx, const mlh_transport* tp, void* dev_m, void* dev_d,
                                      uint32_t n, const uint8_t sum[16], mlh_transcript* tr,
                                      uint8_t* polys_out, uint8_t* rs_out);

/* ---- device timing helpers (bench / profiling) --------------------------- */
/* Kernel timer: while enabled, the NTT pass launches are bracketed by HIP
 * events on the context stream -- those of every transform for on = 1, of
 * every on-th transform for on > 1 (each timing event costs the stream a few
 * microseconds; sampling keeps that out of a throughput measurement);
 * mlh_profile_get (synchronising) returns the launch count and summed
 * milliseconds of the bracketed launches for a kernel label such as
 * "ntt_pass<8,0,0>" (radix log2, last pass, zero-padded input). */
mlh_status mlh_profile_enable(mlh_ctx* ctx, int on);
mlh_status mlh_profile_reset(mlh_ctx* ctx);
mlh_status mlh_profile_get(mlh_ctx* ctx, const char* label, uint64_t* count, double* total_ms);
/* Time `iters` forward NTTs of 2^log_n on the context stream with HIP events
 * (dev_buf is transformed in place); returns the mean ms per NTT. */
mlh_status mlh_bench_ntt(mlh_ctx* ctx, void* dev_buf, uint32_t log_n, uint32_t iters,
                         float* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* MLHIP_H */
