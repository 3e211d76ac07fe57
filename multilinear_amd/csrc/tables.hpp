// The table-cache helpers of capi.hip (where they are described and the cache
// lives) that fri_prover.hip, shard_steps.hip and sharded.hip share.  Not part
// of the public C ABI.
#pragma once
#include "context.hpp"

namespace mlh {
bool check_generator(u128 gen, uint32_t log_n);
mlh_status get_table(mlh_ctx* ctx, u128 base, uint64_t count, u128 scale, const fe** out,
                     bool expand = false);
uint64_t hi_count(uint32_t log_n);
mlh_status fold_tables(mlh_ctx* ctx, uint32_t log_domain, const fe** tlo, const fe** thi);
mlh_status read_root(mlh_ctx* ctx, const uint8_t* layers, uint64_t leaves, uint8_t out[32]);
mlh_status fold_tables_g(mlh_ctx* ctx, u128 g, uint32_t log_len, const fe** tlo, const fe** thi);
mlh_status fold_layer_table(mlh_ctx* ctx, u128 g, uint32_t L, const fe** out);
}  // namespace mlh
