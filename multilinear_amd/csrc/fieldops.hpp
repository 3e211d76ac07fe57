#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

namespace mlh {
// op: 0 add, 1 sub, 2 mul, 3 neg (b unused)
// op: 0 add, 1 sub, 2 mul, 3 neg, 4 scale by c
hipError_t launch_vec_op(int op, const fe* a, const fe* b, fe* out, uint64_t n, hipStream_t st,
                         fe c = fe{});

// Elements a thread inverts with one power (Montgomery's trick), fieldops.hip.
#ifndef MLH_INV_K
#define MLH_INV_K 16
#endif
constexpr uint32_t kInvK = MLH_INV_K, kInvThreads = 256;
// out[i] = a[i]^(M - 2), zero -> zero; out == a allowed, any other overlap not.
hipError_t launch_field_inv(const fe* a, fe* out, uint64_t n, hipStream_t st);
}  // namespace mlh
