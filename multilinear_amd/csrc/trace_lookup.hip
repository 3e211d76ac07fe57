// The multiplicity column of a log-derivative lookup on gfx950: how often each
// entry of the table column T occurs among the value columns, counted in place
// on the row-major trace.  A hash join over the 16-byte elements
// with open addressing; the slot array holds row indices, not keys, so a probe
// compares against the matrix itself (one global_load_dwordx4 per visited slot).
//
// lookup_insert_kernel, one thread per table row j: zero matrix[j][C], then
// probe linearly from hash(key(j)).  An empty slot is taken by atomicCAS; a
// slot that holds a row of the same key is lowered to j by atomicMin when j is
// lower; a slot of another key sends the thread on, wrapping at the end.  A
// slot is never emptied and its key never changes, so all rows of one key walk
// past the same slots and meet in one, which ends as the lowest of them (the
// owner) whatever the arrival order.  The plain read before the CAS may be
// stale, but only by showing "empty" or a higher row of the same key, and both
// lead to the atomic: a table padded by repeating an entry costs one atomic per
// duplicate only until the first of them is visible.
//
// lookup_count_kernel, one thread per (row, value column) pair, in a second
// launch so that the slot array is complete: probe from hash(value) until the
// slot's row has that key (one count for it) or the slot is empty (missing).
// The count is a 64-bit atomicAdd on the low 8 bytes of matrix[owner][C]: it
// stays below 2^37, the element canonical.  Before the atomic the lanes of a
// wave that found the same owner combine (the owner of the lowest pending lane
// by v_readlane, a ballot of the lanes that match, the popcount), and the group
// goes to a 64-entry direct-mapped cache of (owner, count) that the wave keeps
// in registers, one entry per lane, from one grid-stride step to the next; an
// entry is added to the matrix when another owner takes its lane and at the
// end.  A range check sends 2^L counts to a handful of addresses: its owners
// stay in the cache and cost one atomic per wave, not one per step.  Missing
// pairs are counted per thread and reduced per wave at the end.
//
// Every probe loop visits at most 2^log_slots slots and no lane waits for a
// value another lane will write.
//
// lookup_tuple_insert_kernel<A> / lookup_tuple_count_kernel<A> are the same join
// for keys of A columns and pairs (row, value tuple) with a selector
// (DESIGN.md 6h), further down.
#include "field.hpp"
#include "trace_lookup.hpp"

namespace mlh {

// Rounds of wave aggregation per step: each takes the owner of the lowest lane
// still pending.  A lane found alone adds its own 1, and the loop ends at the
// kLkAggSingles-th of them (the wave's owners are mostly distinct: per-lane
// atomics for the rest, which is one wave instruction).  Build-time overrides
// for measurements.
#ifndef MLH_LK_AGG_ROUNDS
#define MLH_LK_AGG_ROUNDS 32
#define MLH_LK_AGG_SINGLES 4
#endif
constexpr uint32_t kLkAggRounds = MLH_LK_AGG_ROUNDS, kLkAggSingles = MLH_LK_AGG_SINGLES;

// MurmurHash3 (x86_32) over the four limbs, seed 0.
__device__ __forceinline__ uint32_t lk_rotl(uint32_t x, uint32_t r) {
  return __builtin_amdgcn_alignbit(x, x, 32 - r);
}
__device__ __forceinline__ uint32_t lk_hash(const fe& k) {
  uint32_t h = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t w = k.w[i] * 0xCC9E2D51u;
    w = lk_rotl(w, 15) * 0x1B873593u;
    h = lk_rotl(h ^ w, 13) * 5u + 0xE6546B64u;
  }
  h ^= 16u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__global__ void __launch_bounds__(kLkThreads)
lookup_insert_kernel(const LookupArgs a) {
  const uint64_t h = 1ull << a.log_height, stride = (uint64_t)gridDim.x * kLkThreads;
  const uint32_t W = a.width, T = a.table_column;
  const uint32_t nslots = 1u << a.log_slots, smask = nslots - 1u;
  const uint32_t hmask = smask & ((1u << a.hash_bits) - 1u);
  uint32_t* slots = a.slots;
  for (uint64_t j = (uint64_t)blockIdx.x * kLkThreads + threadIdx.x; j < h; j += stride) {
    fe* row = a.m + j * W;
    const fe k = fe_load(row + T);
    fe_store(row + a.count_column, fe_zero());
    uint32_t s = lk_hash(k) & hmask;
    for (uint32_t n = 0; n < nslots; ++n) {
      uint32_t cur = slots[s];
      if (cur == kLkEmpty) {
        cur = atomicCAS(slots + s, kLkEmpty, (uint32_t)j);
        if (cur == kLkEmpty) break;  // taken
      }
      if (fe_eq(fe_load(a.m + (uint64_t)cur * W + T), k)) {
        if ((uint32_t)j < cur) atomicMin(slots + s, (uint32_t)j);
        break;
      }
      s = (s + 1u) & smask;
    }
  }
}

// The index of the (n + 1)-th set bit of mask.
__device__ __forceinline__ uint32_t lk_nth_column(uint32_t mask, uint32_t n) {
  for (; n; --n) mask &= mask - 1u;
  return (uint32_t)__ffs(mask) - 1u;
}

template <class Args>
__device__ __forceinline__ void lk_add(const Args& a, uint32_t owner, uint32_t n) {
  atomicAdd(reinterpret_cast<unsigned long long*>(a.m + (uint64_t)owner * a.width + a.count_column),
            (unsigned long long)n);
}

// One step of a count kernel's wave, after the probe: every lane brings the
// owner it found (kLkEmpty: none, or a lane with no pair) and the counts go to
// the matrix, through the wave's cache (c_owner, c_n) when aggregating.  The
// tuple kernels call this and lk_wave_finish; lookup_count_kernel below has
// the same statements inline, so that its instructions stay as measured in
// DESIGN.md 6g.
template <class Args>
__device__ __forceinline__ void lk_wave_add(const Args& a, uint32_t owner, bool aggregate,
                                            uint32_t lane, uint32_t& c_owner, uint32_t& c_n) {
  uint64_t direct = __ballot(owner != kLkEmpty);  // lanes that add their own 1
  if (aggregate) {
    uint64_t pending = direct;
    direct = 0;
    uint32_t singles = 0;
    for (uint32_t round = 0; pending && round < kLkAggRounds; ++round) {
      const uint32_t leader = (uint32_t)__ffsll((unsigned long long)pending) - 1u;
      const uint32_t lo = __builtin_amdgcn_readlane(owner, leader);
      const uint64_t same = __ballot(owner == lo);
      const uint32_t n = (uint32_t)__popcll(same);
      pending &= ~same;
      if (n == 1) {  // alone: not worth a cache entry
        direct |= same;
        if (++singles == kLkAggSingles) break;
        continue;
      }
      if (lane == (lo * 0x9E3779B1u) >> 26) {  // the owner's home lane
        if (c_owner != lo) {
          if (c_n) lk_add(a, c_owner, c_n);
          c_owner = lo;
          c_n = 0;
        }
        c_n += n;
      }
    }
    direct |= pending;
  }
  if ((direct >> lane) & 1u) lk_add(a, owner, 1u);
}

// The end of a count kernel: the cache written out, the missing pairs reduced
// per wave.
template <class Args>
__device__ __forceinline__ void lk_wave_finish(const Args& a, uint32_t lane, uint32_t c_owner,
                                               uint32_t c_n, uint32_t miss, uint32_t miss_row) {
  if (c_n) lk_add(a, c_owner, c_n);
  if (__ballot(miss != 0)) {
    unsigned long long sum = miss;
    for (int d = 32; d; d >>= 1) {
      sum += __shfl_xor(sum, d);
      const uint32_t o = __shfl_xor(miss_row, d);
      miss_row = o < miss_row ? o : miss_row;
    }
    if (lane == 0) {
      atomicAdd(&a.counters->n_missing, sum);
      atomicMin(&a.counters->first_missing_row, miss_row);
    }
  }
}

__global__ void __launch_bounds__(kLkThreads)
lookup_count_kernel(const LookupArgs a, uint64_t total) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t stride = (uint64_t)gridDim.x * kLkThreads;
  const uint32_t W = a.width, T = a.table_column, rmask = (1u << a.log_height) - 1u;
  const uint32_t nslots = 1u << a.log_slots, smask = nslots - 1u;
  const uint32_t hmask = smask & ((1u << a.hash_bits) - 1u);
  const bool aggregate = !(a.flags & kLkNoAggregate);
  const uint32_t* slots = a.slots;
  // this lane's entry of the wave's 64-entry direct-mapped cache of (owner, count)
  uint32_t c_owner = kLkEmpty, c_n = 0;
  uint32_t miss = 0, miss_row = kLkEmpty;
  // (the loop is per wave, not per lane: the ballots below see every lane)
  for (uint64_t base = (uint64_t)blockIdx.x * kLkThreads + wave * 64u; base < total;
       base += stride) {
    const uint64_t e = base + lane;
    uint32_t owner = kLkEmpty;
    if (e < total) {
      const uint32_t row = (uint32_t)e & rmask;
      const uint32_t col = lk_nth_column(a.value_mask, (uint32_t)(e >> a.log_height));
      const fe v = fe_load(a.m + (uint64_t)row * W + col);
      uint32_t s = lk_hash(v) & hmask;
      for (uint32_t n = 0; n < nslots; ++n) {
        const uint32_t r = slots[s];
        if (r == kLkEmpty) break;
        if (fe_eq(fe_load(a.m + (uint64_t)r * W + T), v)) {
          owner = r;
          break;
        }
        s = (s + 1u) & smask;
      }
      if (owner == kLkEmpty) {
        ++miss;
        miss_row = row < miss_row ? row : miss_row;
      }
    }
    uint64_t direct = __ballot(owner != kLkEmpty);  // lanes that add their own 1
    if (aggregate) {
      uint64_t pending = direct;
      direct = 0;
      uint32_t singles = 0;
      for (uint32_t round = 0; pending && round < kLkAggRounds; ++round) {
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)pending) - 1u;
        const uint32_t lo = __builtin_amdgcn_readlane(owner, leader);
        const uint64_t same = __ballot(owner == lo);
        const uint32_t n = (uint32_t)__popcll(same);
        pending &= ~same;
        if (n == 1) {  // alone: not worth a cache entry
          direct |= same;
          if (++singles == kLkAggSingles) break;
          continue;
        }
        if (lane == (lo * 0x9E3779B1u) >> 26) {  // the owner's home lane
          if (c_owner != lo) {
            if (c_n) lk_add(a, c_owner, c_n);
            c_owner = lo;
            c_n = 0;
          }
          c_n += n;
        }
      }
      direct |= pending;
    }
    if ((direct >> lane) & 1u) lk_add(a, owner, 1u);
  }
  if (c_n) lk_add(a, c_owner, c_n);
  if (__ballot(miss != 0)) {
    unsigned long long sum = miss;
    for (int d = 32; d; d >>= 1) {
      sum += __shfl_xor(sum, d);
      const uint32_t o = __shfl_xor(miss_row, d);
      miss_row = o < miss_row ? o : miss_row;
    }
    if (lane == 0) {
      atomicAdd(&a.counters->n_missing, sum);
      atomicMin(&a.counters->first_missing_row, miss_row);
    }
  }
}

// ---- tuple keys ---------------------------------------------
// The same join with key(j) = A elements of row j.  One instance per arity:
// the thread's own tuple stays in 4 * A registers through the probe (a loop
// over a run-time arity would index it per thread and send it to private
// memory, or load it again at every visited slot).

// MurmurHash3 (x86_32), seed 0, over the 4 * A limbs in component order with
// the length word 16 * A: lk_hash at A = 1.
__device__ __forceinline__ uint32_t lk_hash_mix(uint32_t h, const fe& k) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t w = k.w[i] * 0xCC9E2D51u;
    w = lk_rotl(w, 15) * 0x1B873593u;
    h = lk_rotl(h ^ w, 13) * 5u + 0xE6546B64u;
  }
  return h;
}
__device__ __forceinline__ uint32_t lk_hash_final(uint32_t h, uint32_t len) {
  h ^= len;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// key(r) == k, component by component; the first that differs ends it.
template <uint32_t A>
__device__ __forceinline__ bool lk_tuple_eq(const LookupTupleArgs& a, uint32_t r, const fe (&k)[A]) {
  const fe* row = a.m + (uint64_t)r * a.width;
#pragma unroll
  for (uint32_t c = 0; c < A; ++c)
    if (!fe_eq(fe_load(row + a.table_columns[c]), k[c])) return false;
  return true;
}

template <uint32_t A>
__global__ void __launch_bounds__(kLkThreads)
lookup_tuple_insert_kernel(const LookupTupleArgs a) {
  const uint64_t h = 1ull << a.log_height, stride = (uint64_t)gridDim.x * kLkThreads;
  const uint32_t W = a.width;
  const uint32_t nslots = 1u << a.log_slots, smask = nslots - 1u;
  const uint32_t hmask = smask & ((1u << a.hash_bits) - 1u);
  uint32_t* slots = a.slots;
  for (uint64_t j = (uint64_t)blockIdx.x * kLkThreads + threadIdx.x; j < h; j += stride) {
    fe* row = a.m + j * W;
    fe k[A];
    uint32_t hash = 0;
#pragma unroll
    for (uint32_t c = 0; c < A; ++c) {
      k[c] = fe_load(row + a.table_columns[c]);
      hash = lk_hash_mix(hash, k[c]);
    }
    fe_store(row + a.count_column, fe_zero());
    uint32_t s = lk_hash_final(hash, 16u * A) & hmask;
    for (uint32_t n = 0; n < nslots; ++n) {
      uint32_t cur = slots[s];
      if (cur == kLkEmpty) {
        cur = atomicCAS(slots + s, kLkEmpty, (uint32_t)j);
        if (cur == kLkEmpty) break;  // taken
      }
      if (lk_tuple_eq<A>(a, cur, k)) {
        if ((uint32_t)j < cur) atomicMin(slots + s, (uint32_t)j);
        break;
      }
      s = (s + 1u) & smask;
    }
  }
}

// A wave's step is 64 consecutive rows of one tuple: step index base / 64 =
// tuple * (rows / 64, at least 1) + 64-row group, so the tuple index is
// wave-uniform at every height (below 64 rows the lanes past the last row have
// no pair).  Its columns come from the lists in the scratch header, which are
// written before the launch and constant through it: through the constant
// address space a wave-uniform index is a scalar load.  A disabled pair loads
// nothing more and goes through the ballots as a lane that found nothing and
// misses nothing.
typedef __attribute__((address_space(4))) const LookupTupleLists LkConstLists;

static inline uint32_t lk_tuple_log_span(uint32_t log_height) {
  return log_height < 6 ? 6 : log_height;
}

template <uint32_t A>
__global__ void __launch_bounds__(kLkThreads)
lookup_tuple_count_kernel(const LookupTupleArgs a, uint32_t log_span, uint64_t total) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t stride = (uint64_t)gridDim.x * kLkThreads;
  const uint32_t W = a.width, h = 1u << a.log_height, span_mask = (1u << log_span) - 1u;
  const uint32_t nslots = 1u << a.log_slots, smask = nslots - 1u;
  const uint32_t hmask = smask & ((1u << a.hash_bits) - 1u);
  const bool aggregate = !(a.flags & kLkNoAggregate);
  const uint32_t* slots = a.slots;
  const LkConstLists* lists = (const LkConstLists*)(uintptr_t)a.lists;
  uint32_t c_owner = kLkEmpty, c_n = 0;
  uint32_t miss = 0, miss_row = kLkEmpty;
  for (uint64_t base = (uint64_t)blockIdx.x * kLkThreads + wave * 64u; base < total;
       base += stride) {
    const uint32_t l = (uint32_t)(base >> log_span);  // wave-uniform
    const uint32_t row = ((uint32_t)base & span_mask) + lane;
    uint32_t owner = kLkEmpty;
    if (row < h) {
      const fe* vrow = a.m + (uint64_t)row * W;
      const uint32_t sel = lists->selector_columns[l];
      uint32_t col[A];
#pragma unroll
      for (uint32_t c = 0; c < A; ++c) col[c] = lists->value_columns[l * A + c];
      bool enabled = true;
      if (sel != kLkNoSelector) enabled = !fe_eq(fe_load(vrow + sel), fe_zero());
      if (enabled) {
        fe v[A];
        uint32_t hash = 0;
#pragma unroll
        for (uint32_t c = 0; c < A; ++c) {
          v[c] = fe_load(vrow + col[c]);
          hash = lk_hash_mix(hash, v[c]);
        }
        uint32_t s = lk_hash_final(hash, 16u * A) & hmask;
        for (uint32_t n = 0; n < nslots; ++n) {
          const uint32_t r = slots[s];
          if (r == kLkEmpty) break;
          if (lk_tuple_eq<A>(a, r, v)) {
            owner = r;
            break;
          }
          s = (s + 1u) & smask;
        }
        if (owner == kLkEmpty) {
          ++miss;
          miss_row = row < miss_row ? row : miss_row;
        }
      }
    }
    lk_wave_add(a, owner, aggregate, lane, c_owner, c_n);
  }
  lk_wave_finish(a, lane, c_owner, c_n, miss, miss_row);
}

hipError_t launch_lookup_insert(LookupArgs& a, void* scratch, hipStream_t st) {
  if (!a.m || !scratch || a.log_height > kLkMaxLogHeight || a.log_slots < a.log_height ||
      a.log_slots > kLkMaxLogSlots || a.hash_bits > a.log_slots)
    return hipErrorInvalidValue;
  a.counters = reinterpret_cast<LookupCounters*>(scratch);
  a.slots = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(scratch) + kLkSlotsOffset);
  // every slot and first_missing_row to kLkEmpty, then n_missing to zero
  hipError_t e = hipMemsetAsync(scratch, 0xFF, lk_scratch_bytes(a.log_slots), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(scratch, 0, sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lookup_insert_kernel, dim3(lk_blocks(1ull << a.log_height, a.max_blocks)),
                     dim3(kLkThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_lookup_count(const LookupArgs& a, hipStream_t st) {
  const uint64_t total = (uint64_t)__builtin_popcount(a.value_mask) << a.log_height;
  if (!total || !a.slots || !a.counters) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lookup_count_kernel, dim3(lk_blocks(total, a.max_blocks)), dim3(kLkThreads), 0,
                     st, a, total);
  return hipGetLastError();
}

static bool lk_tuple_shape_ok(const LookupTupleArgs& a) {
  return a.arity >= 1 && a.arity <= kLkMaxArity && a.n_tuples >= 1 && a.n_tuples <= kLkMaxTuples &&
         a.arity * a.n_tuples <= kLkMaxTupleColumns;
}

// f.template operator()<A>() for the run-time arity.
template <class F>
static void lk_for_arity(uint32_t arity, F&& f) {
  switch (arity) {
    case 1: return f.template operator()<1>();
    case 2: return f.template operator()<2>();
    case 3: return f.template operator()<3>();
    case 4: return f.template operator()<4>();
    case 5: return f.template operator()<5>();
    case 6: return f.template operator()<6>();
    case 7: return f.template operator()<7>();
    default: return f.template operator()<8>();
  }
}

struct LkLaunchTupleInsert {
  const LookupTupleArgs& a;
  hipStream_t st;
  template <uint32_t A>
  void operator()() const {
    hipLaunchKernelGGL(lookup_tuple_insert_kernel<A>,
                       dim3(lk_blocks(1ull << a.log_height, a.max_blocks)), dim3(kLkThreads), 0, st, a);
  }
};
struct LkLaunchTupleCount {
  const LookupTupleArgs& a;
  hipStream_t st;
  template <uint32_t A>
  void operator()() const {
    // the grid by the rule (one thread per pair); the loop runs over the
    // steps, which below 64 rows are more than the pairs fill
    const uint32_t log_span = lk_tuple_log_span(a.log_height);
    hipLaunchKernelGGL(lookup_tuple_count_kernel<A>,
                       dim3(lk_blocks((uint64_t)a.n_tuples << a.log_height, a.max_blocks)),
                       dim3(kLkThreads), 0, st, a, log_span, (uint64_t)a.n_tuples << log_span);
  }
};

hipError_t launch_lookup_tuple_insert(LookupTupleArgs& a, const LookupTupleLists& lists,
                                      void* scratch, hipStream_t st) {
  if (!a.m || !scratch || a.log_height > kLkMaxLogHeight || a.log_slots < a.log_height ||
      a.log_slots > kLkMaxLogSlots || a.hash_bits > a.log_slots || !lk_tuple_shape_ok(a))
    return hipErrorInvalidValue;
  uint8_t* base = reinterpret_cast<uint8_t*>(scratch);
  a.counters = reinterpret_cast<LookupCounters*>(base);
  a.lists = reinterpret_cast<const LookupTupleLists*>(base + kLkListsOffset);
  a.slots = reinterpret_cast<uint32_t*>(base + kLkSlotsOffset);
  // every slot and first_missing_row to kLkEmpty, n_missing to zero, the lists
  hipError_t e = hipMemsetAsync(scratch, 0xFF, lk_scratch_bytes(a.log_slots), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(scratch, 0, sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(base + kLkListsOffset, &lists, sizeof(lists), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  lk_for_arity(a.arity, LkLaunchTupleInsert{a, st});
  return hipGetLastError();
}

hipError_t launch_lookup_tuple_count(const LookupTupleArgs& a, hipStream_t st) {
  if (!lk_tuple_shape_ok(a) || !a.slots || !a.counters || !a.lists) return hipErrorInvalidValue;
  lk_for_arity(a.arity, LkLaunchTupleCount{a, st});
  return hipGetLastError();
}

}  // namespace mlh
