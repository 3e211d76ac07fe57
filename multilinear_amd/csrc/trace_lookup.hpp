// Launch interface of trace_lookup.hip (internal to libmlhip): the
// multiplicity column of a log-derivative lookup, counted in place on the
// row-major trace by a hash join over its 16-byte elements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

namespace mlh {

// Launch rule of both kernels: 256 threads, min(ceil(work / 256), cap) blocks
// that loop with the grid's stride; work = rows (insert) or rows * value
// columns (count); 2^(log_height + 2) slots (cap and slots as measured: DESIGN.md
// 6g).  Row indices are 32-bit slot values with kLkEmpty reserved,
// hence the height limit.
constexpr uint32_t kLkThreads = 256, kLkMaxBlocks = 1024, kLkMaxLogHeight = 28;
constexpr uint32_t kLkMaxLogSlots = 31, kLkEmpty = 0xFFFFFFFFu;
constexpr uint32_t kLkNoAggregate = 1u;  // flags bit 0: one atomic per lane in count

static inline uint32_t lk_default_log_slots(uint32_t log_height) { return log_height + 2; }
static inline uint32_t lk_blocks(uint64_t work, uint32_t cap) {
  const uint64_t b = (work + kLkThreads - 1) / kLkThreads;
  if (!cap) cap = kLkMaxBlocks;
  return b < cap ? (uint32_t)(b ? b : 1) : cap;
}

// The counters the count kernel leaves behind (device memory, 16 bytes).
struct LookupCounters {
  unsigned long long n_missing;  // pairs (row, value column) whose value is no table entry
  uint32_t first_missing_row;    // the lowest such row, kLkEmpty when none
  uint32_t pad;
};

struct LookupArgs {
  fe* m;            // 2^log_height x width, row-major
  uint32_t* slots;  // 2^log_slots row indices, kLkEmpty at entry
  LookupCounters* counters;
  uint32_t log_height, width, value_mask, table_column, count_column;
  uint32_t log_slots, hash_bits, max_blocks, flags;
};

// Tuple keys (mlh_trace_lookup_tuple_counts): key(j) is the concatenation of
// `arity` elements of row j, a pair is (row, value tuple).  The table columns
// travel as kernel arguments; the value columns and the selectors are indexed
// by the tuple at run time and stand in the scratch header behind the
// counters, where the count kernel reads them from memory (a scalar load: a
// wave's pairs are of one tuple): no per-thread array, no private segment.
constexpr uint32_t kLkMaxArity = 8, kLkMaxTuples = 16, kLkMaxTupleColumns = 32;
constexpr uint32_t kLkNoSelector = 0xFFFFFFFFu;

// The scratch header behind the counters: value_columns[l * arity + c], then
// selector_columns[l] (kLkNoSelector: every row of tuple l is enabled).
struct LookupTupleLists {
  uint32_t value_columns[kLkMaxTupleColumns];
  uint32_t selector_columns[kLkMaxTuples];
};

struct LookupTupleArgs {
  fe* m;            // 2^log_height x width, row-major
  uint32_t* slots;  // 2^log_slots row indices, kLkEmpty at entry
  LookupCounters* counters;
  const LookupTupleLists* lists;  // in the scratch header
  uint32_t log_height, width, arity, n_tuples, count_column;
  uint32_t log_slots, hash_bits, max_blocks, flags;
  uint32_t table_columns[kLkMaxArity];
};

// One scratch buffer per call: the counters (and the tuple entry's column
// lists), then the slot array.
constexpr size_t kLkSlotsOffset = 256, kLkListsOffset = 16;
static_assert(sizeof(LookupCounters) <= kLkListsOffset &&
                  kLkListsOffset + sizeof(LookupTupleLists) <= kLkSlotsOffset,
              "the column lists fit the scratch header");
static inline size_t lk_scratch_bytes(uint32_t log_slots) {
  return kLkSlotsOffset + (sizeof(uint32_t) << log_slots);
}

// Points a.counters and a.slots into scratch (lk_scratch_bytes(a.log_slots)
// bytes) and sets both to their initial state, then column count_column to
// zero and every table row into the slot array (the lowest row of a key wins).
hipError_t launch_lookup_insert(LookupArgs& a, void* scratch, hipStream_t st);
// One count per (row, value column) into the owner's count element; behind
// launch_lookup_insert on the same stream.
hipError_t launch_lookup_count(const LookupArgs& a, hipStream_t st);

// The same two steps for tuple keys.  launch_lookup_tuple_insert also copies
// `lists` (pageable host memory, as the fill image of mlh_trace_fill) into the
// scratch header on st.
hipError_t launch_lookup_tuple_insert(LookupTupleArgs& a, const LookupTupleLists& lists,
                                      void* scratch, hipStream_t st);
// One count per enabled (row, value tuple) pair; work = rows * n_tuples.
hipError_t launch_lookup_tuple_count(const LookupTupleArgs& a, hipStream_t st);

}  // namespace mlh
