// sputnik-amd: the activation math of the SDD activation and gated products
// (sputnik/block/activation.h, gated.h), evaluated in fp32, and the table of
// SDD epilogue ops built on it (SddEpilogue, at the end). One definition,
// used by the 8-wave kernel's epilogue (block_gemm.h kOutMode) and by the
// elementwise kernel (block_epilogue.hip): the two routes must agree bit for
// bit, so floating-point contraction is off in every function here (the
// compiler forms no fma on its own, whatever the surrounding code looks like)
// and the only transcendental steps are the hardware's exp2 and reciprocal.
//
//   relu   max(x, 0)                        relu'  x > 0 ? 1 : 0
//   gelu   x s, s = 1 / (1 + exp(-2u)),     gelu'  s + x s (1 - s) 2 c
//          u = c (x + 0.044715 x^3),                 (1 + 0.134145 x^2)
//          c = sqrt(2 / pi)   (the tanh form, written as a sigmoid)
//   silu   x s, s = 1 / (1 + exp(-x))       silu'  s (1 + x (1 - s))
//
// Every finite x gives a finite result: the argument of s and of the
// derivative is clamped to where s is already exactly 0 or 1 in fp32 (gelu
// |x| <= 11, silu |x| <= 100: exp overflows to inf, or drops below 2^-24,
// long before), so x^2 and x^3 never overflow; the forward x s uses the
// unclamped x. NaN or +-inf in x gives what these formulas yield (NaN for
// gelu / silu of -inf, since -inf * 0).
#ifndef SPUTNIK_AMD_ACT_MATH_H_
#define SPUTNIK_AMD_ACT_MATH_H_

#include <hip/hip_runtime.h>

namespace sputnik_amd {

constexpr int kActRelu = 0, kActGelu = 1, kActSilu = 2;

// Every function below is written once for F = float and F = act_f2 (two
// elements side by side): the pair form compiles to the packed fp32
// multiplies and adds, which round exactly as the scalar ones, so a value
// gets the same bits whichever form evaluates it.
typedef float act_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float act_exp2(float x) {
  return __builtin_amdgcn_exp2f(x);
}
__device__ __forceinline__ act_f2 act_exp2(act_f2 x) {
  return act_f2{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)};
}
__device__ __forceinline__ float act_rcp(float x) {
  return __builtin_amdgcn_rcpf(x);
}
__device__ __forceinline__ act_f2 act_rcp(act_f2 x) {
  return act_f2{__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)};
}
__device__ __forceinline__ float act_clamp(float x, float lim) {
  return __builtin_amdgcn_fmed3f(x, -lim, lim);
}
__device__ __forceinline__ act_f2 act_clamp(act_f2 x, float lim) {
  return act_f2{act_clamp(x.x, lim), act_clamp(x.y, lim)};
}
template <typename F>
__device__ __forceinline__ F act_splat(float v);
template <>
__device__ __forceinline__ float act_splat<float>(float v) {
  return v;
}
template <>
__device__ __forceinline__ act_f2 act_splat<act_f2>(float v) {
  return act_f2{v, v};
}
// x > 0 ? a : b
__device__ __forceinline__ float act_pos(float x, float a, float b) {
  return x > 0.0f ? a : b;
}
__device__ __forceinline__ act_f2 act_pos(act_f2 x, act_f2 a, act_f2 b) {
  return act_f2{x.x > 0.0f ? a.x : b.x, x.y > 0.0f ? a.y : b.y};
}

// 1 / (1 + exp(-t)); t = -inf .. inf gives 0 .. 1.
template <typename F>
__device__ __forceinline__ F act_sigmoid(F t) {
#pragma clang fp contract(off)
  const F e = act_exp2(t * -1.44269504088896340736f);
  return act_rcp(1.0f + e);
}

// s of gelu at the clamped argument xc.
template <typename F>
__device__ __forceinline__ F act_gelu_s(F xc) {
#pragma clang fp contract(off)
  const F x3 = xc * xc * xc;
  const F u = 0.7978845608028654f * (xc + 0.044715f * x3);
  return act_sigmoid<F>(2.0f * u);
}

template <typename F>
__device__ __forceinline__ F act_apply(int act, F x) {
#pragma clang fp contract(off)
  if (act == kActRelu) return act_pos(x, x, act_splat<F>(0.0f));
  if (act == kActGelu) return x * act_gelu_s<F>(act_clamp(x, 11.0f));
  return x * act_sigmoid<F>(act_clamp(x, 100.0f));
}

template <typename F>
__device__ __forceinline__ F act_grad(int act, F x) {
#pragma clang fp contract(off)
  if (act == kActRelu)
    return act_pos(x, act_splat<F>(1.0f), act_splat<F>(0.0f));
  if (act == kActGelu) {
    const F xc = act_clamp(x, 11.0f);
    const F s = act_gelu_s<F>(xc);
    const F poly = 1.0f + 0.134145f * (xc * xc);
    return s + xc * s * (1.0f - s) * (2.0f * 0.7978845608028654f) * poly;
  }
  const F xc = act_clamp(x, 100.0f);
  const F s = act_sigmoid<F>(xc);
  return s * (1.0f + xc * (1.0f - s));
}

// The two elementwise stages, on values of the operand type T:
//   H = round_T(act(float(Z)))       C = round_T(float(G) act'(float(Z)))
// + 0.0f before the rounding makes an exact zero +0 whatever its factors'
// signs: the compiler may fuse a multiply and the conversion to fp16 into
// one mixed-precision fma with a +0 addend where it sees a single element,
// and not where it sees a pair, and -0 + +0 = +0 only there. With the add
// spelled out both forms give +0. (A result that merely underflows to zero
// in T keeps its sign in both.)
template <typename T>
__device__ __forceinline__ T act_forward(int act, T z) {
#pragma clang fp contract(off)
  return (T)(act_apply<float>(act, (float)z) + 0.0f);
}
template <typename T>
__device__ __forceinline__ T act_gate(int act, T g, T z) {
#pragma clang fp contract(off)
  return (T)((float)g * act_grad<float>(act, (float)z) + 0.0f);
}

// ... and on 8 of them (one 16-byte chunk), as 4 pairs.
template <typename T>
using act_t8 = T __attribute__((ext_vector_type(8)));

template <typename T>
__device__ __forceinline__ act_t8<T> act_forward8(int act, act_t8<T> z) {
#pragma clang fp contract(off)
  act_t8<T> r;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const act_f2 h =
        act_apply<act_f2>(act, act_f2{(float)z[i], (float)z[i + 1]}) + 0.0f;
    r[i] = (T)h.x;
    r[i + 1] = (T)h.y;
  }
  return r;
}
template <typename T>
__device__ __forceinline__ act_t8<T> act_gate8(int act, act_t8<T> g,
                                               act_t8<T> z) {
#pragma clang fp contract(off)
  act_t8<T> r;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const act_f2 d =
        act_grad<act_f2>(act, act_f2{(float)z[i], (float)z[i + 1]});
    const act_f2 c = act_f2{(float)g[i], (float)g[i + 1]} * d + 0.0f;
    r[i] = (T)c.x;
    r[i + 1] = (T)c.y;
  }
  return r;
}

// The gated (GLU) stages (sputnik/block/gated.h), on values of T:
//   H  = round_T(float(U) act(float(G)))
//   dU = round_T(float(D) act(float(G)))
//   dG = round_T((float(D) float(U)) act'(float(G)))
// float(D) float(U) is exact in fp32 (two 8- or 11-bit significands). The
// gradient calls act_apply and act_grad as they stand, so each output has the
// bits those give on their own; where both evaluate the same sigmoid of the
// same clamped argument the compiler may keep one copy, which changes nothing.
template <typename F>
__device__ __forceinline__ F gate_mul(int act, F u, F g) {
#pragma clang fp contract(off)
  return u * act_apply<F>(act, g) + 0.0f;
}
template <typename F>
__device__ __forceinline__ F gate_mul_grad(int act, F d, F u, F g) {
#pragma clang fp contract(off)
  return (d * u) * act_grad<F>(act, g) + 0.0f;
}

template <typename T>
__device__ __forceinline__ T gate_forward(int act, T u, T g) {
  return (T)gate_mul<float>(act, (float)u, (float)g);
}
template <typename T>
__device__ __forceinline__ void gate_grad(int act, T d, T g, T u, T *dg,
                                          T *du) {
  const float df = (float)d, gf = (float)g, uf = (float)u;
  *du = (T)gate_mul<float>(act, df, gf);
  *dg = (T)gate_mul_grad<float>(act, df, uf, gf);
}

template <typename T>
__device__ __forceinline__ act_t8<T> gate_forward8(int act, act_t8<T> u,
                                                   act_t8<T> g) {
  act_t8<T> r;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const act_f2 h =
        gate_mul<act_f2>(act, act_f2{(float)u[i], (float)u[i + 1]},
                         act_f2{(float)g[i], (float)g[i + 1]});
    r[i] = (T)h.x;
    r[i + 1] = (T)h.y;
  }
  return r;
}
template <typename T>
__device__ __forceinline__ void gate_grad8(int act, act_t8<T> d, act_t8<T> g,
                                           act_t8<T> u, act_t8<T> *dg,
                                           act_t8<T> *du) {
  act_t8<T> rg, ru;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const act_f2 df = act_f2{(float)d[i], (float)d[i + 1]};
    const act_f2 gf = act_f2{(float)g[i], (float)g[i + 1]};
    const act_f2 uf = act_f2{(float)u[i], (float)u[i + 1]};
    const act_f2 a = gate_mul<act_f2>(act, df, gf);
    const act_f2 b = gate_mul_grad<act_f2>(act, df, uf, gf);
    ru[i] = (T)a.x;
    ru[i + 1] = (T)a.y;
    rg[i] = (T)b.x;
    rg[i + 1] = (T)b.y;
  }
  *dg = rg;
  *du = ru;
}

// ---- The SDD epilogue ops ----
//
// An epilogue op turns x = round_T(A B) and up to two side buffers s0, s1
// (block data in C's storage order) into C (o0) and, for one op, a second
// output o1. The 8-wave kernel applies it to the staged tile (block_gemm.h
// kOutMode, x = round_T(acc)); the elementwise kernel (block_epilogue.hip)
// applies it to an x the plain SDD stored. Both go through the trait below,
// so an op is described once:
//
//   mode          x   s0   s1   o0   o1    x kept to
//   kOutAct       Z             H          z     o0 = act(x)
//   kOutActGrad   G   Z         C                o0 = x act'(s0)
//   kOutGate      U   G         H          up    o0 = x act(s0)
//   kOutGateGrad  D   G    U    dG   dU          o0 = x s1 act'(s0),
//                                                o1 = x act(s0)
//
//   kOutBias      C             C                o0 = x
//
// kKeepsX: the fused route also stores x itself, on request, to the first
// side slot the op does not read (GemmParams z_data for kOutAct, u_data for
// kOutGate); the two-kernel route has the plain SDD write x there instead.
//
// kTakesBias (sputnik/block/bias.h): with a bias b of C's columns set, the
// forward ops see xb = round_T((float(x) + float(b[col])) + 0.0f) wherever
// the table says x, the kept x included (bias_add below). kOutBias is that
// stage alone; without a bias it is the plain product.
constexpr int kOutAct = 3, kOutActGrad = 4;
constexpr int kOutGate = 5, kOutGateGrad = 6;
constexpr int kOutBias = 7;
constexpr bool OutModeIsSddEpilogue(int m) {
  return m == kOutAct || m == kOutActGrad || m == kOutGate ||
         m == kOutGateGrad || m == kOutBias;
}

// The bias stage on one value and on a chunk of 8 (as 4 pairs).
template <typename T>
__device__ __forceinline__ T bias_add(T x, T b) {
#pragma clang fp contract(off)
  return (T)(((float)x + (float)b) + 0.0f);
}
template <typename T>
__device__ __forceinline__ act_t8<T> bias_add8(act_t8<T> x, act_t8<T> b) {
#pragma clang fp contract(off)
  act_t8<T> r;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const act_f2 s = (act_f2{(float)x[i], (float)x[i + 1]} +
                      act_f2{(float)b[i], (float)b[i + 1]}) + 0.0f;
    r[i] = (T)s.x;
    r[i + 1] = (T)s.y;
  }
  return r;
}
// 8 bias elements from b + col (col % 8 == 0): one 16-byte load when b is
// 16-byte aligned, 8 element loads otherwise.
template <typename T>
__device__ __forceinline__ act_t8<T> bias_load8(const T *b, long long col,
                                                bool aligned) {
  if (aligned) return *reinterpret_cast<const act_t8<T> *>(b + col);
  act_t8<T> r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = b[col + i];
  return r;
}

template <int kMode>
struct SddEpilogue;

template <>
struct SddEpilogue<kOutAct> {
  static constexpr int kMode = kOutAct;
  static constexpr bool kTakesBias = true;
  static constexpr int kSideInputs = 0;
  static constexpr bool kKeepsX = true, kSecondOutput = false;
  template <typename T>
  __device__ __forceinline__ static void apply8(int act, act_t8<T> x,
                                                act_t8<T>, act_t8<T>,
                                                act_t8<T> *o0, act_t8<T> *) {
    *o0 = act_forward8<T>(act, x);
  }
  template <typename T>
  __device__ __forceinline__ static void apply(int act, T x, T, T, T *o0,
                                               T *) {
    *o0 = act_forward<T>(act, x);
  }
};

template <>
struct SddEpilogue<kOutActGrad> {
  static constexpr int kMode = kOutActGrad;
  static constexpr bool kTakesBias = false;
  static constexpr int kSideInputs = 1;
  static constexpr bool kKeepsX = false, kSecondOutput = false;
  template <typename T>
  __device__ __forceinline__ static void apply8(int act, act_t8<T> x,
                                                act_t8<T> s0, act_t8<T>,
                                                act_t8<T> *o0, act_t8<T> *) {
    *o0 = act_gate8<T>(act, x, s0);
  }
  template <typename T>
  __device__ __forceinline__ static void apply(int act, T x, T s0, T, T *o0,
                                               T *) {
    *o0 = act_gate<T>(act, x, s0);
  }
};

template <>
struct SddEpilogue<kOutGate> {
  static constexpr int kMode = kOutGate;
  static constexpr bool kTakesBias = true;
  static constexpr int kSideInputs = 1;
  static constexpr bool kKeepsX = true, kSecondOutput = false;
  template <typename T>
  __device__ __forceinline__ static void apply8(int act, act_t8<T> x,
                                                act_t8<T> s0, act_t8<T>,
                                                act_t8<T> *o0, act_t8<T> *) {
    *o0 = gate_forward8<T>(act, x, s0);
  }
  template <typename T>
  __device__ __forceinline__ static void apply(int act, T x, T s0, T, T *o0,
                                               T *) {
    *o0 = gate_forward<T>(act, x, s0);
  }
};

template <>
struct SddEpilogue<kOutGateGrad> {
  static constexpr int kMode = kOutGateGrad;
  static constexpr bool kTakesBias = false;
  static constexpr int kSideInputs = 2;
  static constexpr bool kKeepsX = false, kSecondOutput = true;
  template <typename T>
  __device__ __forceinline__ static void apply8(int act, act_t8<T> x,
                                                act_t8<T> s0, act_t8<T> s1,
                                                act_t8<T> *o0, act_t8<T> *o1) {
    gate_grad8<T>(act, x, s0, s1, o0, o1);
  }
  template <typename T>
  __device__ __forceinline__ static void apply(int act, T x, T s0, T s1,
                                               T *o0, T *o1) {
    gate_grad<T>(act, x, s0, s1, o0, o1);
  }
};

template <>
struct SddEpilogue<kOutBias> {
  static constexpr int kMode = kOutBias;
  static constexpr bool kTakesBias = true;
  static constexpr int kSideInputs = 0;
  static constexpr bool kKeepsX = false, kSecondOutput = false;
  template <typename T>
  __device__ __forceinline__ static void apply8(int, act_t8<T> x, act_t8<T>,
                                                act_t8<T>, act_t8<T> *o0,
                                                act_t8<T> *) {
    *o0 = x;
  }
  template <typename T>
  __device__ __forceinline__ static void apply(int, T x, T, T, T *o0, T *) {
    *o0 = x;
  }
};

// f(SddEpilogue<mode>{}) for a mode known at run time: the one place that
// lists the ops for the host code (launchers, dispatch). Not an epilogue
// mode: `otherwise`.
template <typename R, typename F>
R WithSddEpilogue(int mode, R otherwise, F &&f) {
  switch (mode) {
    case kOutAct: return f(SddEpilogue<kOutAct>{});
    case kOutActGrad: return f(SddEpilogue<kOutActGrad>{});
    case kOutGate: return f(SddEpilogue<kOutGate>{});
    case kOutGateGrad: return f(SddEpilogue<kOutGateGrad>{});
    case kOutBias: return f(SddEpilogue<kOutBias>{});
  }
  return otherwise;
}

}  // namespace sputnik_amd

#endif  // SPUTNIK_AMD_ACT_MATH_H_
