// sputnik-amd: the e4m3 encoder and the two scale rules of
// sputnik/block/fp8.h, as the quantisers (fp8_quantize.hip) evaluate them.
// Plain fp32 and integer steps with no contraction, so the bytes are defined
// and tests/fp8_ref.py reproduces them exactly.
#ifndef SPUTNIK_AMD_FP8_MATH_H_
#define SPUTNIK_AMD_FP8_MATH_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sputnik_amd {

constexpr float kFp8Max = 448.0f;
constexpr float kFp8ScaleFloor = 0x1p-126f;

__device__ __forceinline__ bool fp8_finite(float v) {
  return (__float_as_uint(v) & 0x7fffffffu) <= 0x7f7fffffu;
}

// amax of a tile -> its scale.
__device__ __forceinline__ float fp8_scale(float amax, bool pow2) {
#pragma clang fp contract(off)
  if (!pow2) return fmaxf(amax / kFp8Max, kFp8ScaleFloor);
  if (amax == 0.0f) return kFp8ScaleFloor;
  int e;
  const float m = frexpf(amax, &e);  // amax = m 2^e, m in [0.5, 1)
  e -= m <= 0.875f ? 9 : 8;
  return ldexpf(1.0f, e > -126 ? e : -126);
}

// rne_e4m3 of a finite v with |v| < 464 (fp8.h: |x / scale| <= 448.00003),
// as a byte. The largest finite code is the result for anything the contract
// rules out.
__device__ __forceinline__ uint32_t fp8_encode(float v) {
  const uint32_t u = __float_as_uint(v);
  const uint32_t a = u & 0x7fffffffu;
  uint32_t mag;
  if (a >= 0x3c800000u) {
    // |v| >= 2^-6, a normal e4m3: keep 3 mantissa bits, ties to even, and
    // move the exponent bias from 127 to 7.
    mag = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3);
    mag = mag < 0x7eu ? mag : 0x7eu;
  } else {
    // a multiple of 2^-9; 8 of them are the smallest normal, code 0x08
    mag = (uint32_t)__builtin_rintf(__uint_as_float(a) * 512.0f);
  }
  return ((u >> 24) & 0x80u) | mag;
}

// The byte of element x under `scale`: NaN and +-Inf give the e4m3 NaN with
// x's sign.
__device__ __forceinline__ uint32_t fp8_quantize(float x, float scale) {
#pragma clang fp contract(off)
  if (!fp8_finite(x)) return ((__float_as_uint(x) >> 24) & 0x80u) | 0x7fu;
  return fp8_encode(x / scale);
}

}  // namespace sputnik_amd

#endif  // SPUTNIK_AMD_FP8_MATH_H_
