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
//
// quantize_tiles_kernel (QuantizeTiles, QuantizeBlocks) and
// transpose_weight_fp8_kernel are the backward pass's: one 128 x 128 tile
// per workgroup, quantised along the rows, the columns or both from one
// read, and the byte transpose of a quantised weight. Their comments have
// the LDS layouts.
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

// One 128 x 128 tile of 16-bit values per workgroup, read once, quantised
// along either axis or both. `rows` x `cols` is the matrix the tiles cut: x
// itself (QuantizeTiles) or the block values as [nnz_blocks 128, 128]
// (QuantizeBlocks), whose column outputs go out in the transposed order:
// workgroup j takes source block block_offsets[j].
struct TileParams {
  const void *x, *z;
  uint8_t *q;
  float *scales;
  uint8_t *qt;
  float *scales_t;
  const int *block_offsets;
  long long rows, cols;
  int nnz_blocks, act;
  bool pow2, blocks, aligned, aligned_t;
};

// 16 bytes of a column at q, by one store where the buffer allows it.
__device__ __forceinline__ void store16(uint8_t *p, const uint32_t (&w)[4],
                                        bool aligned) {
  if (aligned) {
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// Rows: the tile's 128 row tiles exactly as quantize_rows_kernel takes them
// (16 lanes per row, the same cross-lane amax). Columns: the values wait in
// LDS as T, [row][column] with the image's padding, and a thread walks down
// one column, so consecutive lanes read consecutive elements of one image
// row: no byte transpose and no bank conflict. Thread (c, half) owns 64 rows
// of column c: the two halves meet through col_amax, then each quantises its
// 64 bytes, which are contiguous in qt.
template <typename T, int kMode>
__global__ void __launch_bounds__(kThreads)
    quantize_tiles_kernel(const TileParams p) {
  __shared__ T image[kTile * kImageRow];
  __shared__ float col_amax[2][kTile];
  const long long col_blocks = p.cols / kTile;
  long long rb = blockIdx.x, cb = 0;
  if (p.blocks) {
    if (p.qt != nullptr) {
      const int b = p.block_offsets[blockIdx.x];
      if (b < 0 || b >= p.nnz_blocks) return;
      rb = b;
    }
  } else {
    rb = blockIdx.x / col_blocks;
    cb = blockIdx.x % col_blocks;
  }
  const T *x = static_cast<const T *>(p.x), *z = static_cast<const T *>(p.z);
  const int sub = threadIdx.x & 15;
  for (int id = threadIdx.x; id < kTile * kTile / 8; id += kThreads) {
    const int r = id >> 4, c = sub * 8;
    const long long at = (rb * kTile + r) * p.cols + cb * kTile + c;
    act_t8<T> v = load8<T>(x + at, p.aligned);
    if constexpr (kMode != kModeNone) {
      using E = SddEpilogue<kMode>;
      act_t8<T> g = v, h, unused;
      if constexpr (E::kSideInputs >= 1) g = load8<T>(z + at, p.aligned);
      E::template apply8<T>(p.act, v, g, v, &h, &unused);
      v = h;
    }
    if (p.q != nullptr) {
      float amax = amax8<T>(v, 0.0f);
#pragma unroll
      for (int d = 8; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
      const float scale = fp8_scale(amax, p.pow2);
      uint32_t lo, hi;
      quantize8<T>(v, scale, &lo, &hi);
      store8(p.q + at, lo, hi, p.aligned);
      if (sub == 0) p.scales[(rb * kTile + r) * col_blocks + cb] = scale;
    }
    if (p.qt != nullptr) {
#pragma unroll
      for (int i = 0; i < 8; ++i) image[r * kImageRow + c + i] = v[i];
    }
  }
  if (p.qt == nullptr) return;
  __syncthreads();
  const int c = threadIdx.x & (kTile - 1), half = threadIdx.x >> 7;
  const T *column = image + half * (kTile / 2) * kImageRow + c;
  float amax = 0.0f;
  for (int r = 0; r < kTile / 2; ++r) {
    const float f = (float)column[r * kImageRow];
    if (fp8_finite(f)) amax = fmaxf(amax, fabsf(f));
  }
  col_amax[half][c] = amax;
  __syncthreads();
  const float scale =
      fp8_scale(fmaxf(col_amax[0][c], col_amax[1][c]), p.pow2);
  uint8_t *dst;
  if (p.blocks) {
    dst = p.qt + (long long)blockIdx.x * kTile * kTile + c * kTile;
    if (half == 0) p.scales_t[(long long)blockIdx.x * kTile + c] = scale;
  } else {
    dst = p.qt + (cb * kTile + c) * p.rows + rb * kTile;
    if (half == 0) p.scales_t[rb * p.cols + cb * kTile + c] = scale;
  }
  dst += half * (kTile / 2);
  for (int piece = 0; piece < kTile / 2; piece += 16) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
      w[i >> 2] |= fp8_quantize((float)column[(piece + i) * kImageRow], scale)
                   << (8 * (i & 3));
    store16(dst + piece, w, p.aligned_t);
  }
}

// qt [k, n] of q [n, k], bytes: one 128 x 128 block per workgroup through an
// LDS image in source order. The transposing side reads single bytes with
// consecutive lanes along an image row (four lanes share a dword, 64 lanes
// cover 16 banks once) and leaves 16 bytes of an output row per lane.
__global__ void __launch_bounds__(kThreads)
    transpose_weight_fp8_kernel(const uint8_t *q, const float *scales, int k,
                                int n, uint8_t *qt, float *scales_t,
                                bool aligned) {
  __shared__ __attribute__((aligned(16))) uint8_t image[kTile * kTile];
  const int nb = blockIdx.x, kb = blockIdx.y;
  const uint8_t *src = q + (long long)nb * kTile * k + kb * kTile;
  for (int id = threadIdx.x; id < kTile * kTile / 16; id += kThreads) {
    const int row = id >> 3, chunk = (id & 7) * 16;
    const uint8_t *from = src + (long long)row * k + chunk;
    uint8_t *to = image + row * kTile + chunk;
    if (aligned) {
      *reinterpret_cast<uint4 *>(to) = *reinterpret_cast<const uint4 *>(from);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) to[i] = from[i];
    }
  }
  __syncthreads();
  uint8_t *dst = qt + (long long)kb * kTile * n + nb * kTile;
  for (int id = threadIdx.x; id < kTile * kTile / 16; id += kThreads) {
    const int kk = id & (kTile - 1), piece = (id >> 7) * 16;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
      w[i >> 2] |= (uint32_t)image[(piece + i) * kTile + kk] << (8 * (i & 3));
    store16(dst + (long long)kk * n + piece, w, aligned);
  }
  if (threadIdx.x == 0)
    scales_t[(long long)nb * (k / kTile) + kb] =
        scales[(long long)kb * (n / kTile) + nb];
}

bool Aligned(std::initializer_list<const void *> ps, uintptr_t mask) {
  uintptr_t bits = 0;
  for (const void *p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & mask) == 0;
}

// No output may be an input or another output.
bool Distinct(std::initializer_list<const void *> outs,
              std::initializer_list<const void *> ins) {
  for (auto a = outs.begin(); a != outs.end(); ++a) {
    if (*a == nullptr) continue;
    for (const void *in : ins)
      if (*a == in) return false;
    for (auto b = a + 1; b != outs.end(); ++b)
      if (*a == *b) return false;
  }
  return true;
}

template <int kMode>
hipError_t LaunchQuantizeTiles(TileParams p, long long tiles, int dtype,
                               hipStream_t stream) {
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  p.aligned = Aligned({p.x, p.z}, 15) && Aligned({p.q}, 7);
  p.aligned_t = Aligned({p.qt}, 15);
  auto launch = [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((quantize_tiles_kernel<T, kMode>),
                       dim3((unsigned)tiles), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
  };
  return dtype == 1 ? launch(__bf16{}) : launch(_Float16{});
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

hipError_t QuantizeTiles(const void *x, int rows, int cols, void *q,
                         float *scales, void *qt, float *scales_t, bool pow2,
                         DataType dtype, hipStream_t stream) {
  if (rows < 0 || cols < 0 || rows % kTile != 0 || cols % kTile != 0 ||
      ((int)dtype != 0 && (int)dtype != 1))
    return hipErrorInvalidValue;
  // (a pair is given whole or not at all, and one of the two is given)
  if ((q == nullptr) != (scales == nullptr) ||
      (qt == nullptr) != (scales_t == nullptr) ||
      (q == nullptr && qt == nullptr))
    return hipErrorInvalidValue;
  if (rows == 0 || cols == 0) return hipSuccess;
  if (x == nullptr || !Distinct({q, scales, qt, scales_t}, {x}))
    return hipErrorInvalidValue;
  TileParams p{x, nullptr, static_cast<uint8_t *>(q), scales,
               static_cast<uint8_t *>(qt), scales_t, nullptr, rows, cols, 0,
               0, pow2, false, false, false};
  return LaunchQuantizeTiles<kModeNone>(
      p, (long long)(rows / kTile) * (cols / kTile), (int)dtype, stream);
}

hipError_t QuantizeBlocks(const BlockMatrix s, Fp8Stage stage,
                          Activation activation, const void *z, void *q,
                          float *scales, void *qt, float *scales_t, bool pow2,
                          DataType dtype, hipStream_t stream) {
  if (s.block_size != BlockSize::k128 || s.nonzeros < 0 ||
      s.nonzeros % (kTile * kTile) != 0 ||
      ((int)dtype != 0 && (int)dtype != 1))
    return hipErrorInvalidValue;
  if (stage != Fp8Stage::kNone && stage != Fp8Stage::kActivation &&
      stage != Fp8Stage::kActivationGrad)
    return hipErrorInvalidValue;
  const int act = (int)activation;
  if (stage != Fp8Stage::kNone && (act < kActRelu || act > kActSilu))
    return hipErrorInvalidValue;
  if ((q == nullptr) != (scales == nullptr) ||
      (qt == nullptr) != (scales_t == nullptr) ||
      (q == nullptr && qt == nullptr))
    return hipErrorInvalidValue;
  if (s.nonzeros == 0) return hipSuccess;
  if (s.data == nullptr ||
      (stage == Fp8Stage::kActivationGrad && z == nullptr) ||
      (qt != nullptr && s.block_offsets == nullptr))
    return hipErrorInvalidValue;
  if (!Distinct({q, scales, qt, scales_t},
                {s.data, z, (const void *)s.block_offsets}))
    return hipErrorInvalidValue;
  const int blocks = s.nonzeros / (kTile * kTile);
  TileParams p{s.data, stage == Fp8Stage::kActivationGrad ? z : nullptr,
               static_cast<uint8_t *>(q), scales, static_cast<uint8_t *>(qt),
               scales_t, static_cast<const int *>(s.block_offsets),
               (long long)blocks * kTile, kTile, blocks, act, pow2, true,
               false, false};
  switch (stage) {
    case Fp8Stage::kActivation:
      return LaunchQuantizeTiles<kOutAct>(p, blocks, (int)dtype, stream);
    case Fp8Stage::kActivationGrad:
      return LaunchQuantizeTiles<kOutActGrad>(p, blocks, (int)dtype, stream);
    default:
      return LaunchQuantizeTiles<kModeNone>(p, blocks, (int)dtype, stream);
  }
}

hipError_t TransposeWeightFp8(const void *q, const float *scales, int k,
                              int n, void *qt, float *scales_t,
                              hipStream_t stream) {
  if (k < 0 || n < 0 || k % kTile != 0 || n % kTile != 0)
    return hipErrorInvalidValue;
  if (k == 0 || n == 0) return hipSuccess;
  if (q == nullptr || scales == nullptr || qt == nullptr ||
      scales_t == nullptr || !Distinct({qt, scales_t}, {q, scales}))
    return hipErrorInvalidValue;
  // (grid.y holds the k blocks)
  if (k / kTile > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(transpose_weight_fp8_kernel, dim3(n / kTile, k / kTile),
                     dim3(kThreads), 0, stream,
                     static_cast<const uint8_t *>(q), scales, k, n,
                     static_cast<uint8_t *>(qt), scales_t,
                     Aligned({q, qt}, 15));
  return hipGetLastError();
}

}  // namespace block
}  // namespace sputnik
