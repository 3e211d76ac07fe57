// The C entries that prepare or check a trace before it is committed, with
// their _shaped and _launch_info forms (mlhip.h gives the semantics): host code
// only, the kernels are in trace_{fill,scan,sort,lookup,shift,public,check}.hip.
#include "cs_call.hpp"
#include "trace_check.hpp"
#include "trace_fill.hpp"
#include "trace_lookup.hpp"
#include "trace_public.hpp"
#include "trace_scan.hpp"
#include "trace_shift.hpp"
#include "trace_sort.hpp"

using namespace mlh;

static_assert(16 * kScanMaxScans <= kPinnedBytes && 4 * kSortDigitsPerKey * kSortMaxKeys <= kPinnedBytes &&
                  sizeof(LookupCounters) <= kPinnedBytes, "what read_back stages below fits the buffer");

extern "C" {

// ---- phase 2 of the two-phase proof: fill and column sum (trace_fill.hip) ----

// The fill with an explicit launch shape (mlh_trace_fill: the shape of
// fill_shape).  One pooled buffer holds this call's randoms beside the
// program's constants, instruction words and output words, filled by one copy.
mlh_status mlh_trace_fill_shaped(mlh_ctx* ctx, const mlh_fill_program* prog, void* dev_matrix,
                                 uint32_t log_height, uint32_t width, const uint8_t* host_randoms,
                                 uint32_t threads, uint32_t rows_per_thread) {
  if (!ctx || !prog || !dev_matrix || width != prog->p.width || log_height > kCsMaxLogHeight ||
      (prog->p.n_randoms && !host_randoms) || !fill_shape_ok(prog->p, threads, rows_per_thread))
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_fill: bad argument");
  const FillProgram& p = prog->p;
  std::vector<u128> rnd(p.n_randoms);
  if (load_canonical(host_randoms, p.n_randoms, rnd.data()) < p.n_randoms)
    return fail(ctx, MLH_ERR_INVALID, "non-canonical random");
  const std::vector<uint8_t> img = fill_build_image(p, rnd.data());
  PoolBuf buf(ctx);
  FillDev dev{};
  MLH_TRY(upload_program(ctx, buf, img, p, fill_image_layout(p), dev));
  dev.n_pre = p.n_pre;
  dev.n_inv = p.n_inv;
  dev.n_outputs = p.n_outputs;
  dev.K = rows_per_thread;
  const uint64_t height = 1ull << log_height;
  const uint32_t blocks = fill_blocks(p, fill_chunks(height, threads, dev.K), threads, dev.K);
  PoolBuf prefix(ctx);  // the lanes' prefix products (trace_fill.hip)
  if (const uint64_t elems = blocks * fill_prefix_elems(p, threads, dev.K)) {
    MLH_TRY(prefix.alloc(16 * elems));
    dev.prefix = prefix.as<fe>();
  }
  ProfScope ps(ctx, "trace_fill");
  HIP_TRY(ctx, launch_trace_fill(dev, threads, blocks, reinterpret_cast<fe*>(dev_matrix), height,
                                 ctx->stream));
  ps.end();
  return MLH_OK;  // (the buffer goes back to the pool: its next user is behind this launch on the stream)
}

mlh_status mlh_trace_fill(mlh_ctx* ctx, const mlh_fill_program* prog, void* dev_matrix,
                          uint32_t log_height, uint32_t width, const uint8_t* host_randoms) {
  uint32_t B = 0, K = 0;
  if (prog && log_height <= kCsMaxLogHeight) fill_shape(prog->p, 1ull << log_height, &B, &K);
  return mlh_trace_fill_shaped(ctx, prog, dev_matrix, log_height, width, host_randoms, B, K);
}

mlh_status mlh_trace_column_sum(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                uint32_t width, uint32_t column_mask, uint8_t out[16]) {
  if (!ctx || !dev_matrix || !out || width < 1 || width > kCsMaxWidth ||
      log_height > kCsMaxLogHeight || (width < 32 && (column_mask >> width)))
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_column_sum: bad argument");
  ProfScope ps(ctx, "trace_column_sum");
  HIP_TRY(ctx, launch_trace_column_sum(reinterpret_cast<const fe*>(dev_matrix), 1ull << log_height,
                                       width, column_mask, ctx->partials, ctx->small, ctx->stream));
  ps.end();
  return read_back(ctx, ctx->small, 16, out);
}

// ---- running sums and running products down columns (trace_scan.hip) ----

static_assert(MLH_SCAN_ADD == kScanAdd && MLH_SCAN_MUL == kScanMul, "mlhip.h and trace_scan.hpp agree");

static bool scan_dims_ok(uint32_t log_height, uint32_t width, uint32_t n_scans) {
  return log_height <= kCsMaxLogHeight && width >= 1 && width <= kCsMaxWidth && n_scans >= 1 &&
         n_scans <= kScanMaxScans;
}

mlh_status mlh_trace_scan_shaped(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                 uint32_t width, uint32_t n_scans, const uint8_t* ops,
                                 const uint8_t* src_columns, const uint8_t* dst_columns,
                                 const uint8_t* host_inits, uint8_t* totals_out, uint32_t threads,
                                 uint32_t rows_per_thread, uint32_t max_blocks) {
  if (!ctx || !dev_matrix || !ops || !src_columns || !dst_columns || !host_inits ||
      !scan_dims_ok(log_height, width, n_scans) ||
      !scan_shape_ok(threads, rows_per_thread, max_blocks))
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_scan: bad argument");
  ScanArgs a{};
  uint32_t written = 0;
  for (uint32_t s = 0; s < n_scans; ++s) {
    if (ops[s] > kScanMul || src_columns[s] >= width || dst_columns[s] >= width ||
        ((written >> dst_columns[s]) & 1u))
      return fail(ctx, MLH_ERR_INVALID, "mlh_trace_scan: bad op, column out of range or "
                                        "destination written twice");
    written |= 1u << dst_columns[s];
    u128 init;
    if (load_canonical(host_inits + 16ull * s, 1, &init) < 1)
      return fail(ctx, MLH_ERR_INVALID, "mlh_trace_scan: non-canonical init");
    a.op[s] = ops[s];
    a.src[s] = src_columns[s];
    a.dst[s] = dst_columns[s];
    a.init[s] = to_fe(init);
  }
  a.m = reinterpret_cast<fe*>(dev_matrix);
  a.height = 1ull << log_height;
  a.width = width;
  a.n_scans = n_scans;
  a.rows_per_thread = rows_per_thread;
  a.blocks = scan_tiling(a.height, threads, rows_per_thread, max_blocks, &a.tiles, &a.tiles_per_block);
  PoolBuf scratch(ctx);  // the blocks' aggregates and offsets, the totals
  MLH_TRY(scratch.alloc(scan_scratch_elems(n_scans, a.blocks) * sizeof(fe)));
  a.aggregates = scratch.as<fe>();
  a.offsets = a.aggregates + (size_t)n_scans * a.blocks;
  a.totals = a.offsets + (size_t)n_scans * a.blocks;
  ProfScope ps(ctx, "trace_scan");
  HIP_TRY(ctx, launch_trace_scan(a, threads, ctx->stream));
  ps.end();
  if (!totals_out) return MLH_OK;  // (the scratch's next user is behind these launches)
  return read_back(ctx, a.totals, 16ull * n_scans, totals_out);
}

mlh_status mlh_trace_scan(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height, uint32_t width,
                          uint32_t n_scans, const uint8_t* ops, const uint8_t* src_columns,
                          const uint8_t* dst_columns, const uint8_t* host_inits,
                          uint8_t* totals_out) {
  return mlh_trace_scan_shaped(ctx, dev_matrix, log_height, width, n_scans, ops, src_columns,
                               dst_columns, host_inits, totals_out, kScanThreads,
                               kScanRowsPerThread, kScanMaxBlocks);
}

mlh_status mlh_trace_scan_launch_info(uint32_t log_height, uint32_t width, uint32_t n_scans,
                                      uint32_t* threads, uint32_t* rows_per_thread,
                                      uint32_t* blocks) {
  if (!threads || !rows_per_thread || !blocks || !scan_dims_ok(log_height, width, n_scans))
    return MLH_ERR_INVALID;
  *threads = kScanThreads;
  *rows_per_thread = kScanRowsPerThread;
  *blocks = scan_tiling(1ull << log_height, kScanThreads, kScanRowsPerThread, kScanMaxBlocks);
  return MLH_OK;
}

// ---- sorted copies of columns (trace_sort.hip) ----

static_assert(MLH_SORT_MAX_KEYS == kSortMaxKeys && MLH_SORT_MAX_COPIES == kSortMaxCopies &&
                  MLH_SORT_NO_COLUMN == kSortNoColumn,
              "mlhip.h and trace_sort.hpp agree");

static bool sort_dims_ok(uint32_t log_height, uint32_t width, uint32_t n_keys) {
  return log_height <= kSortMaxLogHeight && width >= 1 && width <= kCsMaxWidth && n_keys >= 1 &&
         n_keys <= kSortMaxKeys;
}

mlh_status mlh_trace_sort_shaped(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                 uint32_t width, uint32_t n_keys, const uint32_t* key_columns,
                                 uint32_t n_copies, const uint32_t* src_columns,
                                 const uint32_t* dst_columns, uint32_t perm_column,
                                 uint32_t* passes_out, uint32_t threads, uint32_t rows_per_thread,
                                 uint32_t max_blocks, uint32_t flags) {
  if (!ctx || !dev_matrix || !key_columns || !sort_dims_ok(log_height, width, n_keys) ||
      n_copies > kSortMaxCopies || (n_copies && (!src_columns || !dst_columns)) ||
      (!n_copies && perm_column == kSortNoColumn) ||
      !scan_shape_ok(threads, rows_per_thread, max_blocks) || (flags & ~kSortRunAll))
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_sort: bad argument");
  SortArgs a{};
  uint32_t read = 0, written = 0;  // column masks
  for (uint32_t k = 0; k < n_keys; ++k) {
    if (key_columns[k] >= width)
      return fail(ctx, MLH_ERR_INVALID, "mlh_trace_sort: key column out of range");
    read |= 1u << key_columns[k];
    a.key[k] = (uint8_t)key_columns[k];
  }
  for (uint32_t s = 0; s < n_copies; ++s) {
    if (src_columns[s] >= width || dst_columns[s] >= width || ((written >> dst_columns[s]) & 1u))
      return fail(ctx, MLH_ERR_INVALID, "mlh_trace_sort: column out of range or destination "
                                        "written twice");
    read |= 1u << src_columns[s];
    written |= 1u << dst_columns[s];
    a.src[s] = (uint8_t)src_columns[s];
    a.dst[s] = (uint8_t)dst_columns[s];
  }
  if (perm_column != kSortNoColumn) {
    if (perm_column >= width || ((written >> perm_column) & 1u))
      return fail(ctx, MLH_ERR_INVALID, "mlh_trace_sort: perm_column out of range or a destination");
    written |= 1u << perm_column;
  }
  if (read & written)
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_sort: a destination is a key or a source");
  a.m = reinterpret_cast<fe*>(dev_matrix);
  a.height = 1ull << log_height;
  a.width = width;
  a.n_keys = n_keys;
  a.n_copies = n_copies;
  a.perm_column = perm_column;
  a.threads = threads;
  a.rows_per_thread = rows_per_thread;
  a.blocks = scan_tiling(a.height, threads, rows_per_thread, max_blocks, &a.tiles, &a.tiles_per_block);
  PoolBuf scratch(ctx);  // the pairs, the census and one pass's tables
  MLH_TRY(scratch.alloc(sort_scratch_bytes(a.height, n_keys, a.blocks)));
  sort_carve(a, scratch.p);
  const uint32_t digits = kSortDigitsPerKey * n_keys;
  ProfScope ps(ctx, "trace_sort");
  HIP_TRY(ctx, launch_sort_census(a, ctx->stream));
  uint64_t run = digits == 64 ? ~0ull : (1ull << digits) - 1;
  if (!(flags & kSortRunAll)) {  // drop the digits in which all rows agree
    uint32_t same[kSortDigitsPerKey * kSortMaxKeys];
    MLH_TRY(read_back(ctx, a.same, 4ull * digits, same));
    for (uint32_t g = 0; g < digits; ++g)
      if (same[g]) run &= ~(1ull << g);
  }
  HIP_TRY(ctx, launch_sort_passes(a, run, ctx->stream));
  ps.end();
  if (passes_out) *passes_out = (uint32_t)__builtin_popcountll(run);
  return MLH_OK;  // (the scratch's next user is behind these launches)
}

mlh_status mlh_trace_sort(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height, uint32_t width,
                          uint32_t n_keys, const uint32_t* key_columns, uint32_t n_copies,
                          const uint32_t* src_columns, const uint32_t* dst_columns,
                          uint32_t perm_column, uint32_t* passes_out) {
  return mlh_trace_sort_shaped(ctx, dev_matrix, log_height, width, n_keys, key_columns, n_copies,
                               src_columns, dst_columns, perm_column, passes_out, kSortThreads,
                               kSortRowsPerThread, kScanMaxBlocks, 0);
}

mlh_status mlh_trace_sort_launch_info(uint32_t log_height, uint32_t width, uint32_t n_keys,
                                      uint32_t* threads, uint32_t* rows_per_thread,
                                      uint32_t* blocks) {
  if (!threads || !rows_per_thread || !blocks || !sort_dims_ok(log_height, width, n_keys))
    return MLH_ERR_INVALID;
  *threads = kSortThreads;
  *rows_per_thread = kSortRowsPerThread;
  *blocks = scan_tiling(1ull << log_height, kSortThreads, kSortRowsPerThread, kScanMaxBlocks);
  return MLH_OK;
}

// ---- a lookup's multiplicities, before the first commitment (trace_lookup.hip) ----

static_assert(MLH_LOOKUP_MAX_ARITY == kLkMaxArity && MLH_LOOKUP_MAX_TUPLES == kLkMaxTuples &&
                  MLH_LOOKUP_NO_SELECTOR == kLkNoSelector,
              "mlhip.h and trace_lookup.hpp agree");

// Shared by the single-key and the tuple entries: the slot array's rule, the read-out, the launch rule
static bool lookup_shape_ok(uint32_t log_height, uint32_t log_slots, uint32_t hash_bits, uint32_t flags) {
  return log_height <= kLkMaxLogHeight && log_slots >= log_height && log_slots <= kLkMaxLogSlots &&
         hash_bits <= log_slots && !(flags & ~kLkNoAggregate);
}
static mlh_status lookup_read(mlh_ctx* ctx, const LookupCounters* dev_counters, uint64_t* n_missing,
                              uint64_t* first_missing_row) {
  LookupCounters c;
  MLH_TRY(read_back(ctx, dev_counters, sizeof(c), &c));
  *n_missing = c.n_missing;
  *first_missing_row = c.first_missing_row == kLkEmpty ? UINT64_MAX : c.first_missing_row;
  return MLH_OK;
}
// n: the value columns or the tuples, 1..n_max, each a unit of work per row
static mlh_status lookup_launch_info(uint32_t log_height, uint32_t n, uint32_t n_max,
                                     uint32_t* threads, uint32_t* blocks, uint32_t* log_slots) {
  if (!threads || !blocks || !log_slots || log_height > kLkMaxLogHeight || n < 1 || n > n_max)
    return MLH_ERR_INVALID;
  *threads = kLkThreads;
  *blocks = lk_blocks((uint64_t)n << log_height, 0);
  *log_slots = lk_default_log_slots(log_height);
  return MLH_OK;
}

static bool lookup_columns_ok(uint32_t width, uint32_t value_mask, uint32_t T, uint32_t C) {
  return width >= 1 && width <= kCsMaxWidth && value_mask && (width == 32 || !(value_mask >> width)) &&
         T < width && C < width && T != C && !((value_mask >> T) & 1u) && !((value_mask >> C) & 1u);
}

mlh_status mlh_trace_lookup_counts_shaped(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                          uint32_t width, uint32_t value_column_mask,
                                          uint32_t table_column, uint32_t count_column,
                                          uint64_t* n_missing, uint64_t* first_missing_row,
                                          uint32_t log_slots, uint32_t hash_bits,
                                          uint32_t max_blocks, uint32_t flags) {
  if (!ctx || !dev_matrix || !n_missing || !first_missing_row ||
      !lookup_columns_ok(width, value_column_mask, table_column, count_column) ||
      !lookup_shape_ok(log_height, log_slots, hash_bits, flags))
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_lookup_counts: bad argument");
  PoolBuf scratch(ctx);  // the counters and the slot array
  MLH_TRY(scratch.alloc(lk_scratch_bytes(log_slots)));
  LookupArgs a{};
  a.m = reinterpret_cast<fe*>(dev_matrix);
  a.log_height = log_height;
  a.width = width;
  a.value_mask = value_column_mask;
  a.table_column = table_column;
  a.count_column = count_column;
  a.log_slots = log_slots;
  a.hash_bits = hash_bits;
  a.max_blocks = max_blocks;
  a.flags = flags;
  ProfScope ps(ctx, "trace_lookup_counts");
  HIP_TRY(ctx, launch_lookup_insert(a, scratch.p, ctx->stream));
  HIP_TRY(ctx, launch_lookup_count(a, ctx->stream));
  ps.end();
  return lookup_read(ctx, a.counters, n_missing, first_missing_row);
}

mlh_status mlh_trace_lookup_counts(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                   uint32_t width, uint32_t value_column_mask,
                                   uint32_t table_column, uint32_t count_column,
                                   uint64_t* n_missing, uint64_t* first_missing_row) {
  const uint32_t log_slots = lk_default_log_slots(log_height);
  return mlh_trace_lookup_counts_shaped(ctx, dev_matrix, log_height, width, value_column_mask,
                                        table_column, count_column, n_missing, first_missing_row,
                                        log_slots, log_slots, 0, 0);
}

mlh_status mlh_trace_lookup_counts_launch_info(uint32_t log_height, uint32_t n_value_columns,
                                               uint32_t* threads, uint32_t* blocks,
                                               uint32_t* log_slots) {
  return lookup_launch_info(log_height, n_value_columns, kCsMaxWidth - 2, threads, blocks, log_slots);
}

// ---- the same for tuple keys ----

// Checks the column lists and copies them into a (table columns) and lists.
static bool lookup_tuple_columns_ok(uint32_t width, uint32_t arity, const uint32_t* table,
                                    uint32_t n_tuples, const uint32_t* values,
                                    const uint32_t* selectors, uint32_t C, LookupTupleArgs& a,
                                    LookupTupleLists& lists) {
  if (!table || !values || width < 1 || width > kCsMaxWidth || arity < 1 || arity > kLkMaxArity ||
      n_tuples < 1 || n_tuples > kLkMaxTuples || arity * n_tuples > kLkMaxTupleColumns || C >= width)
    return false;
  uint32_t tmask = 0;
  for (uint32_t c = 0; c < arity; ++c) {
    if (table[c] >= width || table[c] == C || ((tmask >> table[c]) & 1u)) return false;
    tmask |= 1u << table[c];
    a.table_columns[c] = table[c];
  }
  for (uint32_t k = 0; k < arity * n_tuples; ++k) {
    if (values[k] >= width || values[k] == C || ((tmask >> values[k]) & 1u)) return false;
    lists.value_columns[k] = values[k];
  }
  for (uint32_t l = 0; l < n_tuples; ++l) {
    const uint32_t s = selectors ? selectors[l] : kLkNoSelector;
    if (s != kLkNoSelector && (s >= width || s == C)) return false;
    lists.selector_columns[l] = s;
  }
  return true;
}

mlh_status mlh_trace_lookup_tuple_counts_shaped(mlh_ctx* ctx, void* dev_matrix,
                                                uint32_t log_height, uint32_t width,
                                                uint32_t arity, const uint32_t* table_columns,
                                                uint32_t n_tuples, const uint32_t* value_columns,
                                                const uint32_t* selector_columns,
                                                uint32_t count_column, uint64_t* n_missing,
                                                uint64_t* first_missing_row, uint32_t log_slots,
                                                uint32_t hash_bits, uint32_t max_blocks,
                                                uint32_t flags) {
  LookupTupleArgs a{};
  LookupTupleLists lists{};
  if (!ctx || !dev_matrix || !n_missing || !first_missing_row ||
      !lookup_tuple_columns_ok(width, arity, table_columns, n_tuples, value_columns,
                               selector_columns, count_column, a, lists) ||
      !lookup_shape_ok(log_height, log_slots, hash_bits, flags))
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_lookup_tuple_counts: bad argument");
  PoolBuf scratch(ctx);  // the counters, the column lists and the slot array
  MLH_TRY(scratch.alloc(lk_scratch_bytes(log_slots)));
  a.m = reinterpret_cast<fe*>(dev_matrix);
  a.log_height = log_height;
  a.width = width;
  a.arity = arity;
  a.n_tuples = n_tuples;
  a.count_column = count_column;
  a.log_slots = log_slots;
  a.hash_bits = hash_bits;
  a.max_blocks = max_blocks;
  a.flags = flags;
  ProfScope ps(ctx, "trace_lookup_tuple_counts");
  HIP_TRY(ctx, launch_lookup_tuple_insert(a, lists, scratch.p, ctx->stream));
  HIP_TRY(ctx, launch_lookup_tuple_count(a, ctx->stream));
  ps.end();
  return lookup_read(ctx, a.counters, n_missing, first_missing_row);
}

mlh_status mlh_trace_lookup_tuple_counts(mlh_ctx* ctx, void* dev_matrix, uint32_t log_height,
                                         uint32_t width, uint32_t arity,
                                         const uint32_t* table_columns, uint32_t n_tuples,
                                         const uint32_t* value_columns,
                                         const uint32_t* selector_columns, uint32_t count_column,
                                         uint64_t* n_missing, uint64_t* first_missing_row) {
  const uint32_t log_slots = lk_default_log_slots(log_height);
  return mlh_trace_lookup_tuple_counts_shaped(ctx, dev_matrix, log_height, width, arity,
                                              table_columns, n_tuples, value_columns,
                                              selector_columns, count_column, n_missing,
                                              first_missing_row, log_slots, log_slots, 0, 0);
}

mlh_status mlh_trace_lookup_tuple_counts_launch_info(uint32_t log_height, uint32_t n_tuples,
                                                     uint32_t* threads, uint32_t* blocks,
                                                     uint32_t* log_slots) {
  return lookup_launch_info(log_height, n_tuples, kLkMaxTuples, threads, blocks, log_slots);
}

// ---- shifted columns (trace_shift.hip; mlhip.h gives the protocol) -------------

static_assert(kTsMaxWidth == kCsMaxWidth, "an extension is as wide as a program at the most");

// Columns and copies fit an extension, each bounded alone as their sum may wrap; sources are columns
static bool shift_range_ok(uint32_t width, uint32_t n_shifts) {
  return width >= 1 && width <= kTsMaxWidth && n_shifts <= kTsMaxWidth && width + n_shifts <= kTsMaxWidth;
}
static bool shift_sources_ok(uint32_t width, const uint32_t* cols, uint32_t n_shifts) {
  for (uint32_t k = 0; k < n_shifts; ++k)
    if (cols[k] >= width) return false;
  return true;
}

mlh_status mlh_trace_extend_next(mlh_ctx* ctx, const void* dev_matrix, uint32_t log_height,
                                 uint32_t width, const uint32_t* shift_columns, uint32_t n_shifts,
                                 void* dev_out) {
  if (!ctx || !dev_matrix || !dev_out || (n_shifts && !shift_columns))
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  if (!shift_range_ok(width, n_shifts) || log_height > kCsMaxLogHeight)
    return fail(ctx, MLH_ERR_INVALID, "width + n_shifts 1..32, log_height 0..32");
  if (!shift_sources_ok(width, shift_columns, n_shifts))
    return fail(ctx, MLH_ERR_INVALID, "source column outside the trace");
  const uint64_t in_bytes = (16ull * width) << log_height;
  const uint64_t out_bytes = (16ull * (width + n_shifts)) << log_height;
  if (ranges_overlap(dev_matrix, dev_out, (uintptr_t)dev_matrix < (uintptr_t)dev_out ? in_bytes : out_bytes))
    return fail(ctx, MLH_ERR_INVALID, "the extension is out of place: the buffers overlap");
  ProfScope ps(ctx, "trace_extend_next");
  HIP_TRY(ctx, launch_trace_extend_next(reinterpret_cast<const fe*>(dev_matrix),
                                        reinterpret_cast<fe*>(dev_out), log_height, width,
                                        shift_columns, n_shifts, ctx->stream));
  ps.end();
  return MLH_OK;
}

mlh_status mlh_trace_extend_next_launch_info(uint32_t log_height, uint32_t width, uint32_t n_shifts,
                                             uint32_t* tile_rows, uint32_t* blocks) {
  if (!tile_rows || !blocks || !shift_range_ok(width, n_shifts) || log_height > kCsMaxLogHeight)
    return MLH_ERR_INVALID;
  *tile_rows = 1u << ts_log_rows(log_height, width + n_shifts);
  *blocks = ts_blocks(log_height, width + n_shifts);
  return MLH_OK;
}

mlh_status mlh_eq_table_rotate(mlh_ctx* ctx, const void* dev_in, uint32_t log_n, void* dev_out) {
  if (!ctx || !dev_in || !dev_out || log_n > 32) return fail(ctx, MLH_ERR_INVALID, "bad argument");
  if (ranges_overlap(dev_in, dev_out, 16ull << log_n))
    return fail(ctx, MLH_ERR_INVALID, "the rotation is out of place: the buffers overlap");
  ProfScope ps(ctx, "eq_rotate");
  HIP_TRY(ctx, launch_eq_rotate(reinterpret_cast<const fe*>(dev_in), reinterpret_cast<fe*>(dev_out),
                                log_n, ctx->stream));
  ps.end();
  return MLH_OK;
}

// ---- public columns (trace_public.hip; mlhip.h gives the format and the protocol) ----

// The spec against a trace of this shape, then its image into img.
static mlh_status public_upload(mlh_ctx* ctx, const PublicColumns& s, uint32_t log_height,
                                uint32_t width, PoolBuf& img) {
  if (width < 1 || width > kTpMaxWidth || s.count() > width || log_height > kCsMaxLogHeight)
    return fail(ctx, MLH_ERR_INVALID, "width 1..32, at most width public columns, log_height 0..32");
  if (!s.fits(log_height))
    return fail(ctx, MLH_ERR_INVALID, "a period or a sparse row of the spec is beyond the height");
  return upload_image(ctx, img, s.image);
}

mlh_status mlh_trace_fill_public(mlh_ctx* ctx, const mlh_public_columns* spec, void* dev_matrix,
                                 uint32_t log_height, uint32_t width) {
  if (!ctx || !spec || !dev_matrix) return fail(ctx, MLH_ERR_INVALID, "null argument");
  const PublicColumns& s = spec->p;
  PoolBuf img(ctx);
  MLH_TRY(public_upload(ctx, s, log_height, width, img));
  ProfScope ps(ctx, "trace_fill_public");
  HIP_TRY(ctx, launch_trace_fill_public(reinterpret_cast<fe*>(dev_matrix), img.p, s.count(),
                                        s.sparse_off, s.n_sparse, log_height, width, ctx->stream));
  ps.end();
  return MLH_OK;  // (the image goes back to the pool: its next user is behind these launches on the stream)
}

mlh_status mlh_trace_fill_public_launch_info(uint32_t log_height, uint32_t width, uint32_t n_public,
                                             uint32_t* tile_rows, uint32_t* blocks) {
  if (!tile_rows || !blocks || width < 1 || width > kTpMaxWidth || n_public < 1 ||
      n_public > kPcMaxColumns || n_public > width || log_height > kCsMaxLogHeight)
    return MLH_ERR_INVALID;
  *tile_rows = 1u << tp_log_rows(log_height, n_public);
  *blocks = tp_blocks(log_height, n_public);
  return MLH_OK;
}

// ---- the witness check (trace_check.hip, trace_public.hip; mlhip.h gives the semantics) ----

// Zeroes the counts and the row count and sets the first rows to all ones,
// behind the pool's poison fill on the stream (tk_counter_words' layout).
static mlh_status check_counters_init(mlh_ctx* ctx, PoolBuf& buf, uint32_t n) {
  MLH_TRY(buf.alloc(8 * tk_counter_words(n)));
  uint8_t* p = buf.as<uint8_t>();
  HIP_TRY(ctx, hipMemsetAsync(p, 0, 8ull * (n + 1), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(p + 8ull * (n + 1), 0xFF, 8ull * n, ctx->stream));
  return MLH_OK;
}

// The one wait of a check: the counters to the host; counts / first rows to
// the caller's arrays where given.  -> the rows with any failure, the first of
// them and the lowest of the n counters that fails there (none: all ones).
static mlh_status check_counters_read(mlh_ctx* ctx, const PoolBuf& buf, uint32_t n,
                                      uint64_t* counts_out, uint64_t* first_rows_out,
                                      uint64_t* n_bad, uint64_t* first_row, uint32_t* first_index) {
  static_assert(8 * (2 * kCsMaxConstraints + 1) <= kPinnedBytes, "the counters fit the staging buffer");
  std::vector<uint64_t> w(tk_counter_words(n));
  MLH_TRY(read_back(ctx, buf.p, 8 * w.size(), w.data()));
  const uint64_t* firsts = w.data() + n + 1;
  if (counts_out) memcpy(counts_out, w.data(), 8ull * n);
  if (first_rows_out) memcpy(first_rows_out, firsts, 8ull * n);
  *n_bad = w[n];
  *first_row = UINT64_MAX;
  *first_index = UINT32_MAX;
  for (uint32_t c = 0; c < n; ++c)
    if (firsts[c] < *first_row) {
      *first_row = firsts[c];
      *first_index = c;
    }
  return MLH_OK;
}

static mlh_status trace_check_run(mlh_ctx* ctx, const mlh_cs_program* prog, const void* dev_matrix,
                                  uint32_t log_height, uint32_t width, const uint32_t* shift_columns,
                                  uint32_t n_shifts, const uint8_t* host_randoms,
                                  uint64_t* counts_out, uint64_t* first_rows_out,
                                  mlh_trace_check_report* report, bool shaped, uint32_t threads,
                                  uint32_t max_blocks) {
  if (!ctx || !prog || !dev_matrix || !report || (n_shifts && !shift_columns))
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_check: null argument");
  const CsProgram& p = prog->p;
  if (!shift_range_ok(width, n_shifts) || width + n_shifts != p.width || log_height > kCsMaxLogHeight)
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_check: width 1..32, width + n_shifts the program's "
                                      "width (at most 32), log_height 0..32");
  if (!shift_sources_ok(width, shift_columns, n_shifts))
    return fail(ctx, MLH_ERR_INVALID, "mlh_trace_check: source column outside the trace");
  if (p.n_randoms && !host_randoms) return fail(ctx, MLH_ERR_INVALID, "mlh_trace_check: randoms missing");
  const uint64_t H = 1ull << log_height;
  uint32_t blocks;
  if (shaped) {
    if (!tk_shape_ok(tk_slots(p), threads, max_blocks))
      return fail(ctx, MLH_ERR_INVALID, "mlh_trace_check_shaped: threads 64, 128 or 256 whose slots "
                                        "fit 152 KiB of LDS, max_blocks 1..1024");
    blocks = tk_blocks_shaped(H, threads, max_blocks);
  } else {
    threads = cs_threads(tk_slots(p));
    blocks = tk_blocks(H, threads);
  }
  const uint32_t NC = p.n_constraints;
  const std::vector<uint8_t> no_mask(16ull * NC, 0);  // (the mask plays no part: its pool entries are zero)
  CsCall cc(ctx);
  MLH_TRY(cc.init(ctx, prog, host_randoms, no_mask.data()));  // (checks the randoms before it enqueues)
  PoolBuf counters(ctx);
  MLH_TRY(check_counters_init(ctx, counters, NC));
  ProfScope ps(ctx, "trace_check");
  HIP_TRY(ctx, launch_trace_check(cc.dev, reinterpret_cast<const fe*>(dev_matrix), log_height, width,
                                  shift_columns, n_shifts, counters.as<uint64_t>(), threads, blocks,
                                  ctx->stream));
  ps.end();
  MLH_TRY(check_counters_read(ctx, counters, NC, counts_out, first_rows_out, &report->n_bad_rows,
                              &report->first_bad_row, &report->first_bad_constraint));
  report->reserved = 0;
  return MLH_OK;
}

mlh_status mlh_trace_check(mlh_ctx* ctx, const mlh_cs_program* prog, const void* dev_matrix,
                           uint32_t log_height, uint32_t width, const uint32_t* shift_columns,
                           uint32_t n_shifts, const uint8_t* host_randoms, uint64_t* counts_out,
                           uint64_t* first_rows_out, mlh_trace_check_report* report) {
  return trace_check_run(ctx, prog, dev_matrix, log_height, width, shift_columns, n_shifts,
                         host_randoms, counts_out, first_rows_out, report, false, 0, 0);
}

mlh_status mlh_trace_check_shaped(mlh_ctx* ctx, const mlh_cs_program* prog, const void* dev_matrix,
                                  uint32_t log_height, uint32_t width,
                                  const uint32_t* shift_columns, uint32_t n_shifts,
                                  const uint8_t* host_randoms, uint64_t* counts_out,
                                  uint64_t* first_rows_out, mlh_trace_check_report* report,
                                  uint32_t threads, uint32_t max_blocks) {
  return trace_check_run(ctx, prog, dev_matrix, log_height, width, shift_columns, n_shifts,
                         host_randoms, counts_out, first_rows_out, report, true, threads, max_blocks);
}

mlh_status mlh_trace_check_launch_info(const mlh_cs_program* prog, uint32_t log_height,
                                       uint32_t* threads, uint32_t* blocks) {
  if (!prog || !threads || !blocks || log_height > kCsMaxLogHeight) return MLH_ERR_INVALID;
  *threads = cs_threads(tk_slots(prog->p));
  *blocks = tk_blocks(1ull << log_height, *threads);
  return MLH_OK;
}

mlh_status mlh_trace_check_public(mlh_ctx* ctx, const mlh_public_columns* spec,
                                  const void* dev_matrix, uint32_t log_height, uint32_t width,
                                  uint64_t* counts_out, uint64_t* first_rows_out,
                                  uint64_t* n_bad_rows, uint64_t* first_bad_row) {
  if (!ctx || !spec || !dev_matrix || !n_bad_rows || !first_bad_row)
    return fail(ctx, MLH_ERR_INVALID, "null argument");
  const PublicColumns& s = spec->p;
  const uint32_t F = s.count();
  PoolBuf img(ctx), counters(ctx);
  MLH_TRY(public_upload(ctx, s, log_height, width, img));
  MLH_TRY(check_counters_init(ctx, counters, F));
  ProfScope ps(ctx, "trace_check_public");
  HIP_TRY(ctx, launch_trace_check_public(reinterpret_cast<const fe*>(dev_matrix), img.p, F,
                                         s.sparse_off, log_height, width, counters.as<uint64_t>(),
                                         ctx->stream));
  ps.end();
  uint32_t first_column;
  return check_counters_read(ctx, counters, F, counts_out, first_rows_out, n_bad_rows, first_bad_row,
                             &first_column);
}

}  // extern "C"
