// sputnik-amd: the elementwise stage of the gated SDD products
// (sputnik/block/gated.h) as a kernel of its own, for the two-kernel route
// behind a plain SDD and for sputnik_block_gate[_grad]:
//
//   gate        out[i] = round_T(float(u[i]) * act(float(g[i])))
//   gate grad   du[i]  = round_T(float(d[i]) * act(float(g[i])))
//               dg[i]  = round_T((float(d[i]) * float(u[i])) * act'(float(g[i])))
//
// over n contiguous elements of block data. The structure is
// block_act_kernel's (block_act.hip): 16-byte loads and stores in a
// grid-stride loop, 8 elements per chunk, 4 chunks per lane in flight, a
// workgroup's chunks of one step contiguous; every chunk is read before any
// of its slots is written, by the same lane, so `out` may be `u` or `g`, `dg`
// may be `d` and `du` may be `u`. Buffers that are not 16-byte aligned, and
// the n % 8 elements at the end, take the scalar loop. The math is
// act_math.h, shared with the 8-wave kernel's fused epilogue, so both routes
// give the same bits.
#include <cstdint>

#include "act_math.h"
#include "api_internal.h"

namespace sputnik_amd {
namespace {

constexpr int kGateThreads = 256;

// kGrad false: a = u, b = g, o0 = out. kGrad true: a = d, b = g, c = u,
// o0 = dg, o1 = du.
template <typename T, bool kGrad>
__global__ void __launch_bounds__(kGateThreads)
    block_gate_kernel(const T *a, const T *b, const T *c, T *o0, T *o1,
                      long long chunks, long long n, int act) {
  typedef T t8 __attribute__((ext_vector_type(8)));
  const long long stride = (long long)gridDim.x * kGateThreads;
  const long long first = (long long)blockIdx.x * kGateThreads + threadIdx.x;
  constexpr int kUnroll = 4;
  const t8 *a8 = reinterpret_cast<const t8 *>(a);
  const t8 *b8 = reinterpret_cast<const t8 *>(b);
  const t8 *c8 = reinterpret_cast<const t8 *>(c);
  t8 *o08 = reinterpret_cast<t8 *>(o0);
  t8 *o18 = reinterpret_cast<t8 *>(o1);
  auto one = [&](long long i, const t8 &av, const t8 &bv, const t8 &cv) {
    if constexpr (kGrad) {
      t8 dg, du;
      gate_grad8<T>(act, av, bv, cv, &dg, &du);
      o08[i] = dg;
      o18[i] = du;
    } else {
      o08[i] = gate_forward8<T>(act, av, bv);
    }
  };
  constexpr long long kSpan = (long long)kUnroll * kGateThreads;
  const long long step = (long long)gridDim.x * kSpan;
  long long base = (long long)blockIdx.x * kSpan;
  for (; base + kSpan <= chunks; base += step) {
    const long long ch = base + threadIdx.x;
    t8 av[kUnroll], bv[kUnroll], cv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      av[u] = a8[ch + u * kGateThreads];
      bv[u] = b8[ch + u * kGateThreads];
      cv[u] = kGrad ? c8[ch + u * kGateThreads] : av[u];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      one(ch + u * kGateThreads, av[u], bv[u], cv[u]);
  }
  // (the last, partial run: at most one workgroup has one)
  if (base < chunks)
    for (long long ch = base + threadIdx.x; ch < chunks; ch += kGateThreads) {
      const t8 av = a8[ch];
      const t8 bv = b8[ch];
      const t8 cv = kGrad ? c8[ch] : av;
      one(ch, av, bv, cv);
    }
  for (long long i = chunks * 8 + first; i < n; i += stride) {
    if constexpr (kGrad) {
      T dg, du;
      gate_grad<T>(act, a[i], b[i], c[i], &dg, &du);
      o0[i] = dg;
      o1[i] = du;
    } else {
      o0[i] = gate_forward<T>(act, a[i], b[i]);
    }
  }
}

template <typename T>
hipError_t Launch(int act, const void *a, const void *b, const void *c,
                  void *o0, void *o1, long long n, bool grad, int cus,
                  hipStream_t stream) {
  uintptr_t bits = reinterpret_cast<uintptr_t>(a) |
                   reinterpret_cast<uintptr_t>(b) |
                   reinterpret_cast<uintptr_t>(o0);
  if (grad)
    bits |= reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(o1);
  const long long chunks = (bits & 15) == 0 ? n / 8 : 0;
  // (vector path: 4 chunks per lane and step; scalar path: one element)
  const long long work = chunks > 0 ? (chunks + 3) / 4 : n;
  long long grid = (work + kGateThreads - 1) / kGateThreads;
  const long long cap = 8LL * (cus > 0 ? cus : 256);
  if (grid > cap) grid = cap;
  if (grad)
    hipLaunchKernelGGL((block_gate_kernel<T, true>), dim3((unsigned)grid),
                       dim3(kGateThreads), 0, stream,
                       static_cast<const T *>(a), static_cast<const T *>(b),
                       static_cast<const T *>(c), static_cast<T *>(o0),
                       static_cast<T *>(o1), chunks, n, act);
  else
    hipLaunchKernelGGL((block_gate_kernel<T, false>), dim3((unsigned)grid),
                       dim3(kGateThreads), 0, stream,
                       static_cast<const T *>(a), static_cast<const T *>(b),
                       static_cast<const T *>(nullptr), static_cast<T *>(o0),
                       static_cast<T *>(nullptr), chunks, n, act);
  return hipGetLastError();
}

}  // namespace

hipError_t LaunchBlockGate(int dtype, int act, const void *u, const void *g,
                           void *out, long long n, int cus,
                           hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (dtype == 1)
    return Launch<__bf16>(act, u, g, nullptr, out, nullptr, n, false, cus,
                          stream);
  return Launch<_Float16>(act, u, g, nullptr, out, nullptr, n, false, cus,
                          stream);
}

hipError_t LaunchBlockGateGrad(int dtype, int act, const void *d, const void *g,
                               const void *u, void *dg, void *du, long long n,
                               int cus, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (dtype == 1)
    return Launch<__bf16>(act, d, g, u, dg, du, n, true, cus, stream);
  return Launch<_Float16>(act, d, g, u, dg, du, n, true, cus, stream);
}

}  // namespace sputnik_amd
