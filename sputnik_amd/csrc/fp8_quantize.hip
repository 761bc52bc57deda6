// sputnik-amd: the e4m3 quantisers of sputnik/block/fp8.h.
//
// quantize_rows_kernel: one 1 x 128 tile per 16 lanes, 8 elements (one
// 16-byte load, one 8-byte store) per lane, the tile's amax by four
// cross-lane steps inside the 16 lanes. Memory-bound: one pass, x is read
// once and never written back. With kOutAct / kOutGate the forward op of
// act_math.h's SddEpilogue table is applied to the chunk first, through the
// same apply8 block_epilogue.hip calls, so the quantised value is the
// quantisation of the H the 16-bit path stores. Buffers that are not 16-byte
// (x, gate) and 8-byte (q) aligned take element accesses; same results.
//
// quantize_weight_kernel: runs at load time. One workgroup per 128 x 128
// block: the block goes through LDS in [n][k] order (the 2-byte transpose,
// as layout.hip does it, when the source is [k, n]), the block's amax is
// reduced through LDS, and the bytes go out k-contiguous.
#include <climits>
#include <cstdint>

#include "act_math.h"
#include "fp8_math.h"
#include "sputnik/block/fp8.h"

namespace sputnik_amd {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 128;
constexpr int kModeNone = 0;  // besides kOutAct and kOutGate

template <typename T>
__device__ __forceinline__ act_t8<T> load8(const T *p, bool aligned) {
  if (aligned) return *reinterpret_cast<const act_t8<T> *>(p);
  act_t8<T> r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = p[i];
  return r;
}

__device__ __forceinline__ void store8(uint8_t *p, uint32_t lo, uint32_t hi,
                                       bool aligned) {
  if (aligned) {
    *reinterpret_cast<uint2 *>(p) = make_uint2(lo, hi);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = (uint8_t)(lo >> (8 * i));
    p[4 + i] = (uint8_t)(hi >> (8 * i));
  }
}

template <typename T>
__device__ __forceinline__ float amax8(act_t8<T> v, float amax) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float f = (float)v[i];
    if (fp8_finite(f)) amax = fmaxf(amax, fabsf(f));
  }
  return amax;
}

template <typename T>
__device__ __forceinline__ void quantize8(act_t8<T> v, float scale,
                                          uint32_t *lo, uint32_t *hi) {
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i)
    w[i >> 2] |= fp8_quantize((float)v[i], scale) << (8 * (i & 3));
  *lo = w[0];
  *hi = w[1];
}

template <typename T, int kMode>
__global__ void __launch_bounds__(kThreads)
    quantize_rows_kernel(const T *x, const T *gate, uint8_t *q, float *scales,
                         long long tiles, int act, bool pow2, bool aligned) {
  const int sub = threadIdx.x & 15;
  const long long step = (long long)gridDim.x * (kThreads / 16);
  // (every lane of a wave runs the same trips: the cross-lane steps below
  // are executed by whole waves)
  for (long long base = (long long)blockIdx.x * (kThreads / 16); base < tiles;
       base += step) {
    const long long tile = base + (threadIdx.x >> 4);
    const bool live = tile < tiles;
    const long long at = tile * kTile + sub * 8;
    act_t8<T> v{};
    if (live) {
      v = load8<T>(x + at, aligned);
      if constexpr (kMode != kModeNone) {
        using E = SddEpilogue<kMode>;
        act_t8<T> g = v, h, unused;
        if constexpr (E::kSideInputs >= 1) g = load8<T>(gate + at, aligned);
        E::template apply8<T>(act, v, g, v, &h, &unused);
        v = h;
      }
    }
    float amax = amax8<T>(v, 0.0f);
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
    const float scale = fp8_scale(amax, pow2);
    if (live) {
      uint32_t lo, hi;
      quantize8<T>(v, scale, &lo, &hi);
      store8(q + at, lo, hi, aligned);
      if (sub == 0) scales[tile] = scale;
    }
  }
}

// The [n][k] image of one block; two elements of padding per row keep the
// transposing writes off one bank.
constexpr int kImageRow = kTile + 2;

template <typename T>
__global__ void __launch_bounds__(kThreads)
    quantize_weight_kernel(const T *w, int k, int n, bool transpose,
                           uint8_t *q, float *scales, bool pow2,
                           bool aligned) {
  __shared__ T image[kTile * kImageRow];
  __shared__ float wave_amax[kThreads / 64];
  const int nb = blockIdx.x, kb = blockIdx.y;
  // The source's rows are k (stride n) or, transposed, n (stride k).
  const long long src_stride = transpose ? k : n;
  const T *src = transpose ? w + (long long)nb * kTile * k + kb * kTile
                           : w + (long long)kb * kTile * n + nb * kTile;
  float amax = 0.0f;
  for (int id = threadIdx.x; id < kTile * kTile / 8; id += kThreads) {
    const int r = id >> 4, c = (id & 15) * 8;
    const act_t8<T> v = load8<T>(src + r * src_stride + c, aligned);
    amax = amax8<T>(v, amax);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (transpose) image[r * kImageRow + c + i] = v[i];
      else image[(c + i) * kImageRow + r] = v[i];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
  if ((threadIdx.x & 63) == 0) wave_amax[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(wave_amax[0], wave_amax[1]),
               fmaxf(wave_amax[2], wave_amax[3]));
  const float scale = fp8_scale(amax, pow2);
  if (threadIdx.x == 0) scales[(long long)kb * (n / kTile) + nb] = scale;
  uint8_t *dst = q + (long long)nb * kTile * k + kb * kTile;
  for (int id = threadIdx.x; id < kTile * kTile / 8; id += kThreads) {
    const int j = id >> 4, c = (id & 15) * 8;
    act_t8<T> v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = image[j * kImageRow + c + i];
    uint32_t lo, hi;
    quantize8<T>(v, scale, &lo, &hi);
    store8(dst + (long long)j * k + c, lo, hi, aligned);
  }
}

bool Aligned(std::initializer_list<const void *> ps, uintptr_t mask) {
  uintptr_t bits = 0;
  for (const void *p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & mask) == 0;
}

template <int kMode>
hipError_t QuantizeRowsImpl(const void *x, const void *gate, int rows,
                            int cols, int act, void *q, float *scales,
                            bool pow2, int dtype, hipStream_t stream) {
  if (rows < 0 || cols < 0 || cols % kTile != 0 || (dtype != 0 && dtype != 1))
    return hipErrorInvalidValue;
  if (kMode != kModeNone && (act < kActRelu || act > kActSilu))
    return hipErrorInvalidValue;
  if (rows == 0 || cols == 0) return hipSuccess;
  if (x == nullptr || q == nullptr || scales == nullptr ||
      (kMode == kOutGate && gate == nullptr))
    return hipErrorInvalidValue;
  if (q == x || q == gate || q == (const void *)scales || scales == x ||
      (const void *)scales == gate)
    return hipErrorInvalidValue;
  const long long tiles = (long long)rows * (cols / kTile);
  const bool aligned = Aligned({x, gate}, 15) && Aligned({q}, 7);
  const long long want = (tiles + kThreads / 16 - 1) / (kThreads / 16);
  // (a few workgroups per CU hide the load latency; the loop takes the rest)
  const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
  auto launch = [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((quantize_rows_kernel<T, kMode>), dim3(grid),
                       dim3(kThreads), 0, stream, static_cast<const T *>(x),
                       static_cast<const T *>(gate), static_cast<uint8_t *>(q),
                       scales, tiles, act, pow2, aligned);
    return hipGetLastError();
  };
  return dtype == 1 ? launch(__bf16{}) : launch(_Float16{});
}

}  // namespace
}  // namespace sputnik_amd

// The host entry points (sputnik/block/fp8.h), also behind the C-ABI.
namespace sputnik {
namespace block {

using namespace sputnik_amd;  // NOLINT: the kernels and launchers above

hipError_t QuantizeRows(const void *x, int rows, int cols, void *q,
                        float *scales, bool pow2, DataType dtype,
                        hipStream_t stream) {
  return QuantizeRowsImpl<kModeNone>(x, nullptr, rows, cols, 0, q, scales,
                                     pow2, (int)dtype, stream);
}

hipError_t QuantizeRowsActivation(const void *x, int rows, int cols,
                                  Activation activation, void *q,
                                  float *scales, bool pow2, DataType dtype,
                                  hipStream_t stream) {
  return QuantizeRowsImpl<kOutAct>(x, nullptr, rows, cols, (int)activation, q,
                                   scales, pow2, (int)dtype, stream);
}

hipError_t QuantizeRowsGated(const void *x, const void *gate, int rows,
                             int cols, Activation activation, void *q,
                             float *scales, bool pow2, DataType dtype,
                             hipStream_t stream) {
  return QuantizeRowsImpl<kOutGate>(x, gate, rows, cols, (int)activation, q,
                                    scales, pow2, (int)dtype, stream);
}

hipError_t QuantizeWeight(const void *w, int k, int n, bool transpose,
                          void *q, float *scales, bool pow2, DataType dtype,
                          hipStream_t stream) {
  if (k < 0 || n < 0 || k % kTile != 0 || n % kTile != 0 ||
      ((int)dtype != 0 && (int)dtype != 1))
    return hipErrorInvalidValue;
  if (k == 0 || n == 0) return hipSuccess;
  if (w == nullptr || q == nullptr || scales == nullptr)
    return hipErrorInvalidValue;
  if (q == w || q == (const void *)scales || (const void *)scales == w)
    return hipErrorInvalidValue;
  // (grid.y holds the k blocks)
  if (k / kTile > 65535) return hipErrorInvalidValue;
  const bool aligned = Aligned({w}, 15) && Aligned({q}, 7);
  auto launch = [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((quantize_weight_kernel<T>),
                       dim3(n / kTile, k / kTile), dim3(kThreads), 0, stream,
                       static_cast<const T *>(w), k, n, transpose,
                       static_cast<uint8_t *>(q), scales, pow2, aligned);
    return hipGetLastError();
  };
  return (int)dtype == 1 ? launch(__bf16{}) : launch(_Float16{});
}

}  // namespace block
}  // namespace sputnik
