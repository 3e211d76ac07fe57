// What the entries that run a program on the device share (capi.hip: the constraint-system
// sumcheck; trace_host.hip: the fill and the witness check): the canonical load of field elements,
// the one-copy upload of a program image and CsCall, a call's device image of a constraint program.
#pragma once
#include "context.hpp"
#include "cs_program.hpp"
#include "cs_sumcheck.hpp"

// n little-endian 16-byte values of src into out.  -> the index of the first
// one at or above the modulus (out is valid below it), n when there is none.
static inline uint32_t load_canonical(const uint8_t* src, uint32_t n, u128* out) {
  for (uint32_t i = 0; i < n; ++i)
    if ((out[i] = mlh::h_load(src + 16ull * i)) >= mlh::kModulus) return i;
  return n;
}
// A host image into a pooled buffer of its size, by one copy on the stream.
static inline mlh_status upload_image(mlh_ctx* ctx, PoolBuf& buf, const std::vector<uint8_t>& img) {
  MLH_TRY(buf.alloc(img.size()));
  HIP_TRY(ctx, hipMemcpyAsync(buf.p, img.data(), img.size(), hipMemcpyHostToDevice, ctx->stream));
  return MLH_OK;
}
// The same for the image (cs_build_image, fill_build_image; layout l) of the program p, and
// dev's (CsDev, FillDev) uniform pool, instruction and output words carved out of the buffer.
template <class Program, class Layout, class Dev>
static inline mlh_status upload_program(mlh_ctx* ctx, PoolBuf& buf, const std::vector<uint8_t>& img,
                                        const Program& p, const Layout& l, Dev& dev) {
  MLH_TRY(upload_image(ctx, buf, img));
  dev.width = p.width;
  dev.n_temps = p.n_temps;
  dev.n_instr = p.n_instr;
  const uint8_t* b = buf.as<uint8_t>();
  dev.uni = reinterpret_cast<const fe*>(b);
  dev.code = reinterpret_cast<const uint32_t*>(b + l.code_off);
  dev.outs = reinterpret_cast<const uint32_t*>(b + l.outs_off);
  return MLH_OK;
}

// One call's device image of a program: the uniform pool (this call's randoms
// and mask beside the program's constants), the interpolation matrix and the
// instruction words, in one pooled buffer filled by one copy.
struct CsCall {
  PoolBuf buf;
  std::vector<uint8_t> img;  // (kept until the call's sync: the copy's source)
  mlh::CsDev dev{};
  const fe* vinv = nullptr;
  uint32_t threads = 0;
  explicit CsCall(mlh_ctx* c) : buf(c) {}
  mlh_status init(mlh_ctx* ctx, const mlh_cs_program* prog, const uint8_t* host_randoms,
                  const uint8_t* host_mask) {
    const mlh::CsProgram& p = prog->p;
    std::vector<u128> rnd(p.n_randoms), mask(p.n_constraints);
    if (load_canonical(host_randoms, p.n_randoms, rnd.data()) < p.n_randoms)
      return fail(ctx, MLH_ERR_INVALID, "non-canonical random");
    if (load_canonical(host_mask, p.n_constraints, mask.data()) < p.n_constraints)
      return fail(ctx, MLH_ERR_INVALID, "non-canonical mask");
    const mlh::CsImageLayout l = mlh::cs_image_layout(p);
    img = mlh::cs_build_image(p, rnd.data(), mask.data());
    MLH_TRY(upload_program(ctx, buf, img, p, l, dev));
    dev.n_constraints = p.n_constraints;
    dev.D = p.points();
    vinv = dev.uni + l.vinv_off;
    threads = mlh::cs_threads(mlh::cs_slots(p));
    return MLH_OK;
  }
};
