// sputnik-amd: the MX quantisers of sputnik/block/mx.h.
//
// quantize_rows_mx_kernel: quantize_rows_kernel's lane layout (fp8_quantize.hip):
// one 1 x 128 row tile per 16 lanes, 8 elements (one 16-byte load, one 8-byte
// store) per lane. A 32-block is 4 lanes, so its amax takes two cross-lane
// steps instead of four; the four e8m0 bytes of the row tile are collected in
// the tile's first lane and leave as one dword (bytes when the scale buffer
// is not 4-byte aligned). With kOutAct / kOutGate the forward op of
// act_math.h's SddEpilogue table is applied first, through the same apply8, so
// the bytes are the quantisation of the H the 16-bit path stores.
//
// quantize_weight_mx_kernel: runs at load time. One workgroup per 128 x 128
// block through an LDS image in [n][k] order (the 2-byte transpose when the
// source is [k, n]); then one thread per (row n, 32-block): amax, scale byte,
// 32 elements as 32 e4m3 bytes or 16 bytes of e2m1 pairs, low nibble first.
#include <climits>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

#include "act_math.h"
#include "mx_math.h"
#include "sputnik/block/mx.h"

namespace sputnik_amd {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 128;
constexpr int kMxBlock = 32;
constexpr int kModeNone = 0;  // besides kOutAct and kOutGate

template <typename T>
__device__ __forceinline__ act_t8<T> load8(const T *p, bool aligned) {
  if (aligned) return *reinterpret_cast<const act_t8<T> *>(p);
  act_t8<T> r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = p[i];
  return r;
}

__device__ __forceinline__ void store_bytes(uint8_t *p, const uint32_t *w,
                                            int words, bool aligned) {
  if (aligned) {
    for (int i = 0; i < words; ++i) reinterpret_cast<uint32_t *>(p)[i] = w[i];
    return;
  }
  for (int i = 0; i < 4 * words; ++i) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

template <typename T, int kMode>
__global__ void __launch_bounds__(kThreads)
    quantize_rows_mx_kernel(const T *x, const T *gate, uint8_t *q,
                            uint8_t *scales, long long tiles, int act,
                            bool aligned, bool scales_aligned) {
  const int sub = threadIdx.x & 15;
  const long long step = (long long)gridDim.x * (kThreads / 16);
  // (every lane of a wave runs the same trips: the cross-lane steps below are
  // executed by whole waves)
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
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float f = (float)v[i];
      if (fp8_finite(f)) amax = fmaxf(amax, fabsf(f));
    }
    // the 32-block: lanes sub & ~3 .. sub | 3
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    const float scale = mx_scale<false>(amax);
    // the tile's four scale bytes, in its first lane
    const uint32_t byte = mx_scale_byte(scale);
    const int lane0 = (threadIdx.x & 63) & ~15;
    const uint32_t dword = (uint32_t)__shfl((int)byte, lane0) |
                           (uint32_t)__shfl((int)byte, lane0 + 4) << 8 |
                           (uint32_t)__shfl((int)byte, lane0 + 8) << 16 |
                           (uint32_t)__shfl((int)byte, lane0 + 12) << 24;
    if (live) {
      uint32_t w[2] = {0, 0};
#pragma unroll
      for (int i = 0; i < 8; ++i)
        w[i >> 2] |= fp8_quantize((float)v[i], scale) << (8 * (i & 3));
      if (aligned) *reinterpret_cast<uint2 *>(q + at) = make_uint2(w[0], w[1]);
      else store_bytes(q + at, w, 2, false);
      if (sub == 0) store_bytes(scales + tile * 4, &dword, 1, scales_aligned);
    }
  }
}

// The [n][k] image of one block; two elements of padding per row keep the
// transposing writes off one bank.
constexpr int kImageRow = kTile + 2;

template <typename T, bool kE2m1>
__global__ void __launch_bounds__(kThreads)
    quantize_weight_mx_kernel(const T *w, int k, int n, bool transpose,
                              uint8_t *q, uint8_t *scales, bool aligned,
                              bool q_aligned) {
  __shared__ T image[kTile * kImageRow];
  const int nb = blockIdx.x, kb = blockIdx.y;
  // The source's rows are k (stride n) or, transposed, n (stride k).
  const long long src_stride = transpose ? k : n;
  const T *src = transpose ? w + (long long)nb * kTile * k + kb * kTile
                           : w + (long long)kb * kTile * n + nb * kTile;
  for (int id = threadIdx.x; id < kTile * kTile / 8; id += kThreads) {
    const int r = id >> 4, c = (id & 15) * 8;
    const act_t8<T> v = load8<T>(src + r * src_stride + c, aligned);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (transpose) image[r * kImageRow + c + i] = v[i];
      else image[(c + i) * kImageRow + r] = v[i];
    }
  }
  __syncthreads();
  // (row j of the block, 32-block u of its 128 k-elements)
  for (int id = threadIdx.x; id < kTile * (kTile / kMxBlock); id += kThreads) {
    const int j = id >> 2, u = id & 3;
    const T *from = image + j * kImageRow + u * kMxBlock;
    float amax = 0.0f;
    bool finite = true;
    for (int i = 0; i < kMxBlock; ++i) {
      const float f = (float)from[i];
      if (fp8_finite(f)) amax = fmaxf(amax, fabsf(f));
      else finite = false;
    }
    const float scale = mx_scale<kE2m1>(amax);
    const long long row = (long long)nb * kTile + j;
    const int kk = kb * kTile + u * kMxBlock;
    uint32_t byte = mx_scale_byte(scale);
    if (kE2m1 && !finite) byte = kE8m0Nan;
    scales[row * (k / kMxBlock) + kk / kMxBlock] = (uint8_t)byte;
    if constexpr (kE2m1) {
      uint32_t out[4] = {0, 0, 0, 0};
      if (finite) {
        for (int i = 0; i < kMxBlock; ++i)
          out[i >> 3] |= mx_quantize_e2m1((float)from[i], scale) << (4 * (i & 7));
      }
      store_bytes(q + (row * k + kk) / 2, out, 4, q_aligned);
    } else {
      uint32_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int i = 0; i < kMxBlock; ++i)
        out[i >> 2] |= fp8_quantize((float)from[i], scale) << (8 * (i & 3));
      store_bytes(q + row * k + kk, out, 8, q_aligned);
    }
  }
}

bool Aligned(std::initializer_list<const void *> ps, uintptr_t mask) {
  uintptr_t bits = 0;
  for (const void *p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & mask) == 0;
}

template <int kMode>
hipError_t QuantizeRowsMxImpl(const void *x, const void *gate, int rows,
                              int cols, int act, void *q, uint8_t *scales,
                              int dtype, hipStream_t stream) {
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
    hipLaunchKernelGGL((quantize_rows_mx_kernel<T, kMode>), dim3(grid),
                       dim3(kThreads), 0, stream, static_cast<const T *>(x),
                       static_cast<const T *>(gate), static_cast<uint8_t *>(q),
                       scales, tiles, act, aligned, Aligned({scales}, 3));
    return hipGetLastError();
  };
  return dtype == 1 ? launch(__bf16{}) : launch(_Float16{});
}

}  // namespace
}  // namespace sputnik_amd

// The host entry points (sputnik/block/mx.h), also behind the C-ABI.
namespace sputnik {
namespace block {

using namespace sputnik_amd;  // NOLINT: the kernels and launchers above

hipError_t QuantizeRowsMx(const void *x, const void *gate, int rows, int cols,
                          MxStage stage, Activation activation, void *q,
                          uint8_t *scales, DataType dtype,
                          hipStream_t stream) {
  switch (stage) {
    case MxStage::kNone:
      return QuantizeRowsMxImpl<kModeNone>(x, nullptr, rows, cols, 0, q,
                                           scales, (int)dtype, stream);
    case MxStage::kActivation:
      return QuantizeRowsMxImpl<kOutAct>(x, nullptr, rows, cols,
                                         (int)activation, q, scales,
                                         (int)dtype, stream);
    case MxStage::kGated:
      return QuantizeRowsMxImpl<kOutGate>(x, gate, rows, cols, (int)activation,
                                          q, scales, (int)dtype, stream);
  }
  return hipErrorInvalidValue;
}

hipError_t QuantizeWeightMx(const void *w, int k, int n, bool transpose,
                            MxFormat format, void *q, uint8_t *scales,
                            DataType dtype, hipStream_t stream) {
  if (k < 0 || n < 0 || k % kTile != 0 || n % kTile != 0 ||
      ((int)dtype != 0 && (int)dtype != 1) ||
      (format != MxFormat::kE4M3 && format != MxFormat::kE2M1))
    return hipErrorInvalidValue;
  if (k == 0 || n == 0) return hipSuccess;
  if (w == nullptr || q == nullptr || scales == nullptr)
    return hipErrorInvalidValue;
  if (q == w || q == (const void *)scales || (const void *)scales == w)
    return hipErrorInvalidValue;
  // (grid.y holds the k blocks)
  if (k / kTile > 65535) return hipErrorInvalidValue;
  const bool aligned = Aligned({w}, 15), q_aligned = Aligned({q}, 3);
  auto launch = [&](auto t, auto e2m1) {
    using T = decltype(t);
    hipLaunchKernelGGL((quantize_weight_mx_kernel<T, decltype(e2m1)::value>),
                       dim3(n / kTile, k / kTile), dim3(kThreads), 0, stream,
                       static_cast<const T *>(w), k, n, transpose,
                       static_cast<uint8_t *>(q), scales, aligned, q_aligned);
    return hipGetLastError();
  };
  auto kind = [&](auto t) {
    return format == MxFormat::kE2M1 ? launch(t, std::true_type{})
                                     : launch(t, std::false_type{});
  };
  return (int)dtype == 1 ? kind(__bf16{}) : kind(_Float16{});
}

}  // namespace block
}  // namespace sputnik
