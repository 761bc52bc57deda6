// sputnik-amd: the e8m0 scale rules and the e2m1 encoder of
// sputnik/block/mx.h, as the quantisers (mx_quantize.hip) evaluate them. The
// e4m3 element is fp8_math.h's. Plain fp32 and integer steps with no
// contraction, so the bytes are defined and tests/mx_ref.py reproduces them.
#ifndef SPUTNIK_AMD_MX_MATH_H_
#define SPUTNIK_AMD_MX_MATH_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fp8_math.h"

namespace sputnik_amd {

constexpr uint32_t kE8m0Nan = 0xFFu;

// amax of a 32-block -> its power-of-two scale: the smallest s >= 2^-126
// with amax / s <= 448 (e4m3) or <= 6 (e2m1).
template <bool kE2m1>
__device__ __forceinline__ float mx_scale(float amax) {
  if (amax == 0.0f) return kFp8ScaleFloor;
  int e;
  const float m = frexpf(amax, &e);  // amax = m 2^e, m in [0.5, 1)
  if (kE2m1) e -= m <= 0.75f ? 3 : 2;
  else e -= m <= 0.875f ? 9 : 8;
  return ldexpf(1.0f, e > -126 ? e : -126);
}

// The e8m0 byte of a scale mx_scale returned (a normal power of two).
__device__ __forceinline__ uint32_t mx_scale_byte(float s) {
  return __float_as_uint(s) >> 23;
}

// rne_e2m1 of a finite v with |v| <= 6 as a 4-bit code. The grid is 0.5 wide
// below 2, 1 wide below 4 and 2 wide above; rint is ties-to-even and an even
// multiple of the step is the code with mantissa bit 0.
__device__ __forceinline__ uint32_t mx_encode_e2m1(float v) {
  const uint32_t sign = (__float_as_uint(v) >> 28) & 0x8u;
  const float a = fabsf(v);
  uint32_t mag;
  if (a < 2.0f) mag = (uint32_t)__builtin_rintf(a * 2.0f);           // 0 .. 4
  else if (a < 4.0f) mag = 2u + (uint32_t)__builtin_rintf(a);        // 4 .. 6
  else mag = 4u + (uint32_t)__builtin_rintf(a * 0.5f);               // 6 .. 7
  return sign | (mag < 7u ? mag : 7u);
}

// The code of element x under `scale` (a block with a non-finite element
// never gets here: its codes are 0).
__device__ __forceinline__ uint32_t mx_quantize_e2m1(float x, float scale) {
#pragma clang fp contract(off)
  return mx_encode_e2m1(x / scale);
}

}  // namespace sputnik_amd

#endif  // SPUTNIK_AMD_MX_MATH_H_
