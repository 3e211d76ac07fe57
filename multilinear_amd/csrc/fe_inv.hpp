// The inverse of a Field128 element on the device (field.rs:113-118: Div
// through winter-math's inv, zero -> zero), shared by field_inv_kernel
// (fieldops.hip) and the fill kernel (trace_fill.hip).
//
// x^(M - 2), M - 2 = 2^128 - 45 * 2^40 - 1 = [80 ones] 1101 0010 [40 ones] in
// binary.  With x_k = x^(2^k - 1): x_2, x_4, x_5, x_10, x_20, x_40, x_80 by
// x_(a+b) = x_a^(2^b) * x_b (79 squarings, 7 products), then the windows 11, 0,
// 1 (4 squarings, 2 products), 0010 (4 squarings, 1 product) and the 40 ones
// (40 squarings, 1 product): 127 squarings + 11 products = 138, against 127 +
// 121 for square-and-multiply.
#pragma once
#include "field.hpp"

namespace mlh {

__device__ __forceinline__ fe fe_sqr_n(fe x, uint32_t n) {
#pragma unroll 1
  for (uint32_t i = 0; i < n; ++i) x = fe_sqr(x);
  return x;
}
__device__ __forceinline__ fe fe_inv_chain(const fe& x) {
  const fe x2 = fe_mul(fe_sqr(x), x);
  const fe x4 = fe_mul(fe_sqr_n(x2, 2), x2);
  const fe x5 = fe_mul(fe_sqr(x4), x);
  const fe x10 = fe_mul(fe_sqr_n(x5, 5), x5);
  const fe x20 = fe_mul(fe_sqr_n(x10, 10), x10);
  const fe x40 = fe_mul(fe_sqr_n(x20, 20), x20);
  fe r = fe_mul(fe_sqr_n(x40, 40), x40);  // x_80
  r = fe_mul(fe_sqr_n(r, 2), x2);         // .. 11
  r = fe_mul(fe_sqr_n(r, 2), x);          // .. 01
  r = fe_sqr(fe_mul(fe_sqr_n(r, 3), x));  // .. 0010
  return fe_mul(fe_sqr_n(r, 40), x40);    // .. 40 ones
}

__device__ __forceinline__ bool fe_is_zero(const fe& a) {
  return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) == 0u;
}

}  // namespace mlh
