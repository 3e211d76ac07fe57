// Elementwise Field128 ops on device vectors (src/field.rs:66-136: Add, Sub,
// Mul, Neg of winter-math f128 BaseElement), streaming dwordx4 per lane.
#include "fe_inv.hpp"
#include "field.hpp"
#include "fieldops.hpp"

namespace mlh {

template <int OP>
__global__ void __launch_bounds__(256)
vec_op_kernel(const fe* a, const fe* b, fe* out, uint64_t n, fe c) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const fe x = fe_load(a + i);
    fe r;
    if (OP == 0) r = fe_add(x, fe_load(b + i));
    if (OP == 1) r = fe_sub(x, fe_load(b + i));
    if (OP == 2) r = fe_mul(x, fe_load(b + i));
    if (OP == 3) r = fe_neg(x);
    if (OP == 4) r = fe_mul(x, c);
    fe_store(out + i, r);
  }
}

hipError_t launch_vec_op(int op, const fe* a, const fe* b, fe* out, uint64_t n, hipStream_t st,
                         fe c) {
  uint64_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks == 0) return hipSuccess;
  switch (op) {
    case 0: hipLaunchKernelGGL(vec_op_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, a, b, out, n, c); break;
    case 1: hipLaunchKernelGGL(vec_op_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a, b, out, n, c); break;
    case 2: hipLaunchKernelGGL(vec_op_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, st, a, b, out, n, c); break;
    case 3: hipLaunchKernelGGL(vec_op_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, a, b, out, n, c); break;
    case 4: hipLaunchKernelGGL(vec_op_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, a, b, out, n, c); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ---- inverse (field.rs:113-118: Div through winter-math's inv, zero -> zero) ----
// (the x^(M - 2) chain: fe_inv.hpp)
// Montgomery's trick per thread: a thread takes the kInvK elements base + k *
// kInvThreads of its block's chunk (consecutive lanes, consecutive elements),
// keeps the prefix products p_k = a'_0 .. a'_k in registers (a' = a with zeros
// replaced by one), raises p_(K-1) to M - 2 once, and walks back: out_k = inv *
// p_(k-1), inv *= a'_k, with a_k read a second time (the kernel is bound by
// the multiplier, and holding the inputs as well would double the registers).
// 3 products per element + 138 / kInvK.  An element is read and written by one
// thread only and a_k is loaded before out_k is stored, so out == a is allowed.
__global__ void __launch_bounds__(kInvThreads)
field_inv_kernel(const fe* a, fe* out, uint64_t n, uint64_t chunks) {
  constexpr uint32_t K = kInvK;
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const uint64_t base = c * (uint64_t)(kInvThreads * K) + threadIdx.x;
    if (base >= n) continue;
    fe p[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
      const uint64_t i = base + (uint64_t)k * kInvThreads;
      fe x = i < n ? fe_load(a + i) : fe_one();
      if (fe_is_zero(x)) x = fe_one();
      p[k] = k ? fe_mul(p[k - 1], x) : x;
    }
    fe inv = fe_inv_chain(p[K - 1]);
    const uint64_t last = base + (uint64_t)(K - 1) * kInvThreads;
    fe x = last < n ? fe_load(a + last) : fe_one();
#pragma unroll
    for (uint32_t k = K; k-- > 0;) {
      const uint64_t i = base + (uint64_t)k * kInvThreads;
      fe xn = fe_one();  // the next step's input, loaded before this step's store
      if (k && i - kInvThreads < n) xn = fe_load(a + (i - kInvThreads));
      if (i < n) {
        const bool z = fe_is_zero(x);
        const fe o = k ? fe_mul(inv, p[k - 1]) : inv;
        fe_store(out + i, z ? fe_zero() : o);
        if (k && !z) inv = fe_mul(inv, x);
      }
      x = xn;
    }
  }
}

hipError_t launch_field_inv(const fe* a, fe* out, uint64_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const uint64_t chunks = (n + (uint64_t)kInvThreads * kInvK - 1) / ((uint64_t)kInvThreads * kInvK);
  const uint64_t blocks = chunks < 65536 ? chunks : 65536;
  hipLaunchKernelGGL(field_inv_kernel, dim3((unsigned)blocks), dim3(kInvThreads), 0, st, a, out, n,
                     chunks);
  return hipGetLastError();
}

}  // namespace mlh
