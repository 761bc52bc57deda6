// sputnik-amd: the SDD epilogue ops (act_math.h SddEpilogue) as an
// elementwise kernel of their own, for the two-kernel route behind a plain
// SDD and for sputnik_block_activation[_grad] / sputnik_block_gate[_grad]:
//
//   (o0[i], o1[i]) = op(x[i], s0[i], s1[i])
//
// over n contiguous elements of block data, with only the buffers the mode
// has. 16-byte loads and stores in a grid-stride loop (8 elements per chunk,
// 4 chunks per lane in flight, a workgroup's chunks of one step contiguous);
// every chunk is read before any of its slots is written, by the same lane,
// so an output may be one of the inputs (activation: out = z or g; gate:
// out = u or g, dg = d, du = u). Buffers that are not 16-byte aligned, and
// the n % 8 elements at the end, take the scalar loop. The math is
// act_math.h, shared with the 8-wave kernel's fused epilogue, so both routes
// give the same bits.
//
// With a column bias (sputnik/block/bias.h; kBias instantiations, the forward
// ops only) x[i] is first replaced by xb = bias_add(x[i], bias[col]), col =
// 128 column_indices[i / 16384] + i % 128: a chunk lies inside one block row,
// so its 8 bias elements are contiguous. Where x is a buffer of its own (the
// op keeps it) xb is written back over it, by the lane that read the chunk.
// A column index outside [0, col_blocks) stands for a bias of zeros.
#include <cstdint>

#include "act_math.h"
#include "api_internal.h"

namespace sputnik_amd {
namespace {

constexpr int kThreads = 256;

// What a kBias kernel needs besides the buffers.
template <typename T>
struct BiasArgs {
  const T *bias;
  const short *column_indices;
  int col_blocks;
  T *x_out;  // where xb goes as well (nullptr: nowhere)
};

template <typename T, int kMode, bool kBias>
__global__ void __launch_bounds__(kThreads)
    block_epilogue_kernel(const T *x, const T *s0, const T *s1, T *o0, T *o1,
                          long long chunks, long long n, int act,
                          BiasArgs<T> ba) {
  using E = SddEpilogue<kMode>;
  const bool bias_aligned = (reinterpret_cast<uintptr_t>(ba.bias) & 15) == 0;
  // First logical column of element i's block, or -1.
  auto block_col = [&](long long i) {
    const int cb = ba.column_indices[i >> 14];
    return cb >= 0 && cb < ba.col_blocks ? (long long)cb * 128 : -1LL;
  };
  typedef T t8 __attribute__((ext_vector_type(8)));
  const long long stride = (long long)gridDim.x * kThreads;
  const long long first = (long long)blockIdx.x * kThreads + threadIdx.x;
  // kUnroll chunks per lane in flight (their loads issued before any math):
  // the loop is bound by memory latency, not by the math.
  constexpr int kUnroll = 4;
  const t8 *x8 = reinterpret_cast<const t8 *>(x);
  const t8 *s08 = reinterpret_cast<const t8 *>(s0);
  const t8 *s18 = reinterpret_cast<const t8 *>(s1);
  t8 *o08 = reinterpret_cast<t8 *>(o0);
  t8 *o18 = reinterpret_cast<t8 *>(o1);
  // (an input the mode does not have is never loaded: it stands for x)
  struct In { t8 x, s0, s1, b; };
  auto load = [&](long long i) {
    In v;
    v.x = x8[i];
    if constexpr (kBias) {
      const long long c0 = block_col(i * 8);
      v.b = c0 >= 0 ? bias_load8<T>(ba.bias, c0 + (i * 8) % 128, bias_aligned)
                    : t8{};
    }
    if constexpr (E::kSideInputs >= 1) v.s0 = s08[i]; else v.s0 = v.x;
    if constexpr (E::kSideInputs >= 2) v.s1 = s18[i]; else v.s1 = v.x;
    return v;
  };
  auto one = [&](long long i, const In &v) {
    t8 r0, r1, xv = v.x;
    if constexpr (kBias) {
      xv = bias_add8<T>(xv, v.b);
      if (ba.x_out != nullptr) reinterpret_cast<t8 *>(ba.x_out)[i] = xv;
    }
    E::template apply8<T>(act, xv, v.s0, v.s1, &r0, &r1);
    o08[i] = r0;
    if constexpr (E::kSecondOutput) o18[i] = r1;
  };
  // A workgroup takes kUnroll * kThreads consecutive chunks (16 KiB) per
  // step, so the loads it has in flight are one contiguous run.
  constexpr long long kSpan = (long long)kUnroll * kThreads;
  const long long step = (long long)gridDim.x * kSpan;
  long long base = (long long)blockIdx.x * kSpan;
  for (; base + kSpan <= chunks; base += step) {
    const long long c = base + threadIdx.x;
    In v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = load(c + u * kThreads);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) one(c + u * kThreads, v[u]);
  }
  // (the last, partial run: at most one workgroup has one)
  if (base < chunks)
    for (long long c = base + threadIdx.x; c < chunks; c += kThreads)
      one(c, load(c));
  for (long long i = chunks * 8 + first; i < n; i += stride) {
    T xv = x[i];
    if constexpr (kBias) {
      const long long c0 = block_col(i);
      xv = bias_add<T>(xv, c0 >= 0 ? ba.bias[c0 + i % 128] : (T)0.0f);
      if (ba.x_out != nullptr) ba.x_out[i] = xv;
    }
    T sv0 = xv, sv1 = xv, r0, r1;
    if constexpr (E::kSideInputs >= 1) sv0 = s0[i];
    if constexpr (E::kSideInputs >= 2) sv1 = s1[i];
    E::template apply<T>(act, xv, sv0, sv1, &r0, &r1);
    o0[i] = r0;
    if constexpr (E::kSecondOutput) o1[i] = r1;
  }
}

template <typename T, int kMode>
hipError_t Launch(int act, const void *x, const void *s0, const void *s1,
                  void *o0, void *o1, long long n, int cus,
                  const void *bias, const short *column_indices,
                  int col_blocks, hipStream_t stream) {
  using E = SddEpilogue<kMode>;
  // (the vector path needs every pointer the mode uses 16-byte aligned)
  uintptr_t bits = reinterpret_cast<uintptr_t>(x) |
                   reinterpret_cast<uintptr_t>(o0);
  if (E::kSideInputs >= 1) bits |= reinterpret_cast<uintptr_t>(s0);
  if (E::kSideInputs >= 2) bits |= reinterpret_cast<uintptr_t>(s1);
  if (E::kSecondOutput) bits |= reinterpret_cast<uintptr_t>(o1);
  const long long chunks = (bits & 15) == 0 ? n / 8 : 0;
  // (vector path: 4 chunks per lane and step; scalar path: one element)
  const long long work = chunks > 0 ? (chunks + 3) / 4 : n;
  long long grid = (work + kThreads - 1) / kThreads;
  // (a few workgroups per CU hide the load latency; the loop takes the rest)
  const long long cap = 8LL * (cus > 0 ? cus : 256);
  if (grid > cap) grid = cap;
  BiasArgs<T> ba{static_cast<const T *>(bias), column_indices, col_blocks,
                 nullptr};
  if constexpr (E::kTakesBias) {
    if (bias != nullptr) {
      // (x a buffer of its own is the kept x: it gets xb too)
      if (x != o0) ba.x_out = static_cast<T *>(const_cast<void *>(x));
      hipLaunchKernelGGL((block_epilogue_kernel<T, kMode, true>),
                         dim3((unsigned)grid), dim3(kThreads), 0, stream,
                         static_cast<const T *>(x), static_cast<const T *>(s0),
                         static_cast<const T *>(s1), static_cast<T *>(o0),
                         static_cast<T *>(o1), chunks, n, act, ba);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((block_epilogue_kernel<T, kMode, false>),
                     dim3((unsigned)grid), dim3(kThreads), 0, stream,
                     static_cast<const T *>(x), static_cast<const T *>(s0),
                     static_cast<const T *>(s1), static_cast<T *>(o0),
                     static_cast<T *>(o1), chunks, n, act, ba);
  return hipGetLastError();
}

}  // namespace

hipError_t LaunchBlockEpilogue(int dtype, int mode, int act, const void *x,
                               const void *s0, const void *s1, void *o0,
                               void *o1, long long n, int cus,
                               hipStream_t stream, const void *bias,
                               const short *column_indices, int col_blocks) {
  if (n <= 0) return hipSuccess;
  // (a bias: block data of whole 128 x 128 blocks with their column indices)
  if (bias != nullptr && (column_indices == nullptr || n % 16384 != 0))
    return hipErrorInvalidValue;
  return WithSddEpilogue(mode, hipErrorInvalidValue, [&](auto e) {
    using E = decltype(e);
    constexpr int kMode = E::kMode;
    if (bias != nullptr && !E::kTakesBias) return hipErrorInvalidValue;
    if (dtype == 1)
      return Launch<__bf16, kMode>(act, x, s0, s1, o0, o1, n, cus, bias,
                                   column_indices, col_blocks, stream);
    return Launch<_Float16, kMode>(act, x, s0, s1, o0, o1, n, cus, bias,
                                   column_indices, col_blocks, stream);
  });
}

}  // namespace sputnik_amd
