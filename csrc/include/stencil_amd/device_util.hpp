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

// Lane shifts of one VGPR by data-parallel-primitive moves (no LDS, no
// memory). Every lane of the wave must be active where they are used.
//   lane_below: lane i gets v of lane i-1 of the wave, lane 0 gets `first`
//   lane_above: lane i gets v of lane i+1 of the wave, lane 63 keeps its own
//   row_above<N>: lane i gets lane i+N of its 16-lane row (0 past the row)
//   lane_value: every lane gets v of lane `lane` (a scalar register)
__device__ __forceinline__ float lane_below(float v, float first) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v),
                                                    0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_above(float v) {
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}
template <int N> __device__ __forceinline__ float row_above(float v) {
  static_assert(N >= 1 && N <= 15, "row shift");
  return __int_as_float(
      __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + N /* row_shl:N */, 0xf, 0xf, true));
}
__device__ __forceinline__ float lane_value(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// A wave-uniform address as a scalar-register base in the GLOBAL address
// space: loads and stores through it then take the form scalar base + 32-bit
// lane offset. (Through a generic pointer they would become flat
// instructions, and without the pin the compiler folds the lane offset into a
// per-lane 64-bit pointer and multiplies per load.)
typedef __attribute__((address_space(1))) char gchar;
__device__ __forceinline__ gchar *global_base(const void *p) {
  return (gchar *)uniform_ptr(p);
}
// A loop-invariant 32-bit lane offset, made opaque at its use: the zero
// extension then stays next to the access, where instruction selection folds
// it into the scalar-base form; hoisted out of the loop it becomes a 64-bit
// register pair and a 64-bit vector add per access.
__device__ __forceinline__ uint32_t lane_offset(uint32_t o) {
  asm volatile("" : "+v"(o));
  return o;
}

// Nontemporal 16 B store (a write-only stream: bypass cache pollution; plain
// stores measured 9% slower on the jacobi kernels), through a generic pointer
// or a global_base address.
typedef float vfloat4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store4(void *dst, const float4 &v) {
  const vfloat4 ov = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(ov, (vfloat4 *)dst);
}
__device__ __forceinline__ void store4(gchar *dst, const float4 &v) {
  const vfloat4 ov = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(ov, (__attribute__((address_space(1))) vfloat4 *)dst);
}
#endif

} // namespace stencil_amd
