// Device-side helpers.
#pragma once

#include <hip/hip_runtime.h>

namespace stencil_amd {

// Make a pointer loaded from memory provably wave-uniform so the compiler
// keeps it in SGPRs and emits scalar-base addressing for every dependent
// load/store (instead of 64-bit per-lane VGPR address math). The slot
// values ARE uniform (same slot for the whole grid); the compiler just
// cannot prove it.
template <typename T> __device__ __forceinline__ T *uniform_ptr(T *p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (T *)(((uint64_t)hi << 32) | lo);
}

// x / 6.0f without the IEEE division expansion (about 11 vector ALU
// instructions per value on gfx950): one multiply by c = RN(1/6) and one
// Newton correction of the quotient, 3 instructions.
//   q = x * c;  r = fma(-6, q, x);  q' = fma(r, c, q)
// q' equals the correctly rounded x / 6.0f bit for bit for EVERY finite x
// with |x| >= 2^-125 (biased exponent >= 2): checked over all 2^32 inputs by
// tools/div6_exhaustive.cpp, which compiles these two functions for the
// host. Below that (denormals, the smallest normals, -0) the residual r loses
// bits, and for +-inf it is NaN: div6_fast_ok() is the guard, and callers
// take the true division when it fails (div6 below).
// The fused operations are explicit and contraction is switched off inside,
// so the result does not depend on -ffp-contract.
__host__ __device__ inline float div6_fast(float x) {
#pragma clang fp contract(off)
  const float c = 0x1.555556p-3f; // RN(1/6) = 0x3e2aaaab
  const float q = x * c;
  const float r = __builtin_fmaf(-6.0f, q, x);
  return __builtin_fmaf(r, c, q);
}

// 2^-125 <= |x| <= FLT_MAX (false for NaN)
__host__ __device__ inline bool div6_fast_ok(float x) {
  const float a = __builtin_fabsf(x);
  return a >= 0x1p-125f && a <= 0x1.fffffep+127f;
}

#if defined(__HIPCC__)
// x / 6.0f, correctly rounded for every input: the fast form when every
// active lane of the wave passes the guard (one wave-uniform branch), the
// true division otherwise.
__device__ __forceinline__ float div6(float x) {
  if (__any(!div6_fast_ok(x))) return x / 6.0f;
  return div6_fast(x);
}

__device__ __forceinline__ float4 div6(float4 v) {
  const bool ok =
      div6_fast_ok(v.x) && div6_fast_ok(v.y) && div6_fast_ok(v.z) && div6_fast_ok(v.w);
  if (__any(!ok)) return make_float4(v.x / 6.0f, v.y / 6.0f, v.z / 6.0f, v.w / 6.0f);
  return make_float4(div6_fast(v.x), div6_fast(v.y), div6_fast(v.z), div6_fast(v.w));
}
#endif

} // namespace stencil_amd
