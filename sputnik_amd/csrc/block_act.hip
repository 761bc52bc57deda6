// sputnik-amd: the elementwise stage of the SDD activation products
// (sputnik/block/activation.h) as a kernel of its own, for the two-kernel
// route behind a plain SDD and for sputnik_block_activation[_grad]:
//
//   activation   out[i] = round_T(act(float(z[i])))
//   gate         out[i] = round_T(float(g[i]) * act'(float(z[i])))
//
// over n contiguous elements of block data. 16-byte loads and stores in a
// grid-stride loop (8 elements per chunk, 4 chunks per lane in flight, a
// workgroup's chunks of one step contiguous); every chunk is read before its
// slot is written, by the same lane, so `out` may be `z` or `g`.
// Buffers that are not 16-byte aligned, and the n % 8 elements at the end,
// take the scalar loop. The math is act_math.h, shared with the 8-wave
// kernel's fused epilogue, so both routes give the same bits.
#include <cstdint>

#include "act_math.h"
#include "api_internal.h"

namespace sputnik_amd {
namespace {

constexpr int kActThreads = 256;

template <typename T, bool kGate>
__global__ void __launch_bounds__(kActThreads)
    block_act_kernel(const T *g, const T *z, T *out,
                     long long chunks, long long n, int act) {
  typedef T t8 __attribute__((ext_vector_type(8)));
  const long long stride = (long long)gridDim.x * kActThreads;
  const long long first = (long long)blockIdx.x * kActThreads + threadIdx.x;
  // kUnroll chunks per lane in flight (their loads issued before any math):
  // the loop is bound by memory latency, not by the activation.
  constexpr int kUnroll = 4;
  auto one = [&](const t8 &zv, const t8 &gv) {
    if constexpr (kGate)
      return act_gate8<T>(act, gv, zv);
    else
      return act_forward8<T>(act, zv);
  };
  const t8 *z8 = reinterpret_cast<const t8 *>(z);
  const t8 *g8 = reinterpret_cast<const t8 *>(g);
  t8 *o8 = reinterpret_cast<t8 *>(out);
  // A workgroup takes kUnroll * kActThreads consecutive chunks (16 KiB) per
  // step, so the loads it has in flight are one contiguous run.
  constexpr long long kSpan = (long long)kUnroll * kActThreads;
  const long long step = (long long)gridDim.x * kSpan;
  long long base = (long long)blockIdx.x * kSpan;
  for (; base + kSpan <= chunks; base += step) {
    const long long c = base + threadIdx.x;
    t8 zv[kUnroll], gv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      zv[u] = z8[c + u * kActThreads];
      gv[u] = kGate ? g8[c + u * kActThreads] : zv[u];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      o8[c + u * kActThreads] = one(zv[u], gv[u]);
  }
  // (the last, partial run: at most one workgroup has one)
  if (base < chunks)
    for (long long c = base + threadIdx.x; c < chunks; c += kActThreads) {
      const t8 zv = z8[c];
      o8[c] = one(zv, kGate ? g8[c] : zv);
    }
  for (long long i = chunks * 8 + first; i < n; i += stride) {
    if constexpr (kGate)
      out[i] = act_gate<T>(act, g[i], z[i]);
    else
      out[i] = act_forward<T>(act, z[i]);
  }
}

template <typename T>
hipError_t Launch(int act, const void *g, const void *z, void *out,
                  long long n, int cus, hipStream_t stream) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(g) |
                         reinterpret_cast<uintptr_t>(z) |
                         reinterpret_cast<uintptr_t>(out);
  const long long chunks = (bits & 15) == 0 ? n / 8 : 0;
  // (vector path: 4 chunks per lane and step; scalar path: one element)
  const long long work = chunks > 0 ? (chunks + 3) / 4 : n;
  long long grid = (work + kActThreads - 1) / kActThreads;
  // (a few workgroups per CU hide the load latency; the loop takes the rest)
  const long long cap = 8LL * (cus > 0 ? cus : 256);
  if (grid > cap) grid = cap;
  if (g != nullptr)
    hipLaunchKernelGGL((block_act_kernel<T, true>), dim3((unsigned)grid),
                       dim3(kActThreads), 0, stream,
                       static_cast<const T *>(g), static_cast<const T *>(z),
                       static_cast<T *>(out), chunks, n, act);
  else
    hipLaunchKernelGGL((block_act_kernel<T, false>), dim3((unsigned)grid),
                       dim3(kActThreads), 0, stream,
                       static_cast<const T *>(nullptr),
                       static_cast<const T *>(z), static_cast<T *>(out),
                       chunks, n, act);
  return hipGetLastError();
}

}  // namespace

hipError_t LaunchBlockAct(int dtype, int act, const void *g, const void *z,
                          void *out, long long n, int cus,
                          hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (dtype == 1) return Launch<__bf16>(act, g, z, out, n, cus, stream);
  return Launch<_Float16>(act, g, z, out, n, cus, stream);
}

}  // namespace sputnik_amd
