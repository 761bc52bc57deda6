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
// quantize_rows_mx_fp4_kernel: the same rows as MXFP4 (its comment has the
// steps).
//
// quantize_weight_mx_kernel: runs at load time. One workgroup per 128 x 128
// block through an LDS image in [n][k] order (the 2-byte transpose when the
// source is [k, n]); then one thread per (row n, 32-block): amax, scale byte,
// 32 elements as 32 e4m3 bytes or 16 bytes of e2m1 pairs, low nibble first.
//
// quantize_tiles_mx_kernel (QuantizeTilesMx, QuantizeBlocksMx) is the backward
// pass's: one 128 x 128 tile per workgroup, read once with 16-byte loads,
// quantised in 1 x 32 groups along the rows, in 32 x 1 groups down the
// columns, or both. quantize_tile_mx has the thread map and the LDS bank
// argument; its row pass (mx_row_chunk) and its column pass (mx_column_pass)
// are helpers.
//
// quantize_gated_grad_mx_kernel (QuantizeBlocksMxGatedGrad) is the GLU
// backward's: both gated gradients of a 128 x 128 block from one read of D, G
// and U, each quantised along either axis or both through the same two
// helpers, neither ever stored as 16 bits. Its comment has the staging.
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

__device__ __forceinline__ void store16(uint8_t *p, const uint32_t *w,
                                        bool aligned) {
  if (aligned) {
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    return;
  }
  store_bytes(p, w, 4, false);
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

// The e8m0 byte of an e2m1 32-block from its finite amax, mx_scale<true>'s
// rule on the bits: amax = 1.M 2^(E - 127) = m 2^(E - 126) with m = 1.M / 2,
// so m <= 0.75 is M <= 0x400000 and the scale's exponent is E - 126 - 3 (or -
// 2), floored at -126: byte max(E - 2 + (M > 0x400000), 1). A subnormal or
// zero amax has E = 0 and lands on the floor.
__device__ __forceinline__ uint32_t mx_e2m1_scale_byte(float amax) {
  const uint32_t bits = __float_as_uint(amax);
  const int e = (int)(bits >> 23) - 2 + ((bits & 0x7FFFFFu) > 0x400000u ? 1 : 0);
  return (uint32_t)(e > 1 ? e : 1);
}

// quantize_rows_mx_fp4_kernel (QuantizeRowsMxFp4): quantize_rows_mx_kernel's
// lane layout, loads and stage, so H is the same 16-bit value; then the e2m1
// rules. A lane's 8 elements are 8 codes, one dword. No division: the scale
// is 2^(byte - 127) with byte in 1 .. 253, its reciprocal the normal float
// with exponent field 254 - byte, and x times it is the exact quotient (at
// most 6 in magnitude, at least 2^-7 times the smallest subnormal of T). A
// non-finite element is met across the 32-block's four lanes like the amax:
// scale byte 0xFF, codes 0. The four dwords of a 32-block meet in its first
// lane and leave as one 16-byte store; the row tile's four scale bytes leave
// as one dword.
template <typename T, int kMode>
__global__ void __launch_bounds__(kThreads)
    quantize_rows_mx_fp4_kernel(const T *x, const T *gate, uint8_t *q,
                                uint8_t *scales, long long tiles, int act,
                                bool aligned, bool q_aligned,
                                bool scales_aligned) {
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
    int finite = 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float f = (float)v[i];
      if (fp8_finite(f)) amax = fmaxf(amax, fabsf(f));
      else finite = 0;
    }
    // the 32-block: lanes sub & ~3 .. sub | 3
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    finite &= __shfl_xor(finite, 2);
    finite &= __shfl_xor(finite, 1);
    const uint32_t byte = finite ? mx_e2m1_scale_byte(amax) : kE8m0Nan;
    uint32_t w = 0;
    if (finite) {
      const float inverse = __uint_as_float((254u - byte) << 23);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        w |= mx_encode_e2m1((float)v[i] * inverse) << (4 * i);
    }
    const int lane0 = (threadIdx.x & 63) & ~15;
    const uint32_t dword = (uint32_t)__shfl((int)byte, lane0) |
                           (uint32_t)__shfl((int)byte, lane0 + 4) << 8 |
                           (uint32_t)__shfl((int)byte, lane0 + 8) << 16 |
                           (uint32_t)__shfl((int)byte, lane0 + 12) << 24;
    const uint32_t block[4] = {w, (uint32_t)__shfl_down((int)w, 1),
                               (uint32_t)__shfl_down((int)w, 2),
                               (uint32_t)__shfl_down((int)w, 3)};
    if (live) {
      if ((sub & 3) == 0)
        store16(q + tile * (kTile / 2) + sub * 4, block, q_aligned);
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

// One 128 x 128 tile of 16-bit values per workgroup, read once, quantised
// along the rows, down the columns or both. `rows` x `cols` is the matrix the
// tiles cut: x itself (QuantizeTilesMx) or the block values as [nnz_blocks
// 128, 128] (QuantizeBlocksMx), whose column outputs go out in the transposed
// order: workgroup j takes source block block_offsets[j].
struct MxTileParams {
  const void *x, *z;
  uint8_t *q, *scales, *qt, *scales_t;
  const int *block_offsets;
  long long rows, cols;
  int nnz_blocks, act;
  bool blocks, aligned, scales_aligned, aligned_t, scales_t_aligned;
};

// Where one tile's two images go: the address of the tile's first byte of
// each output and the bytes between consecutive rows (q, scales) or
// consecutive columns (qt, scales_t) of the tile.
struct MxTileSinks {
  uint8_t *q, *scales, *qt, *scales_t;
  long long q_pitch, scales_pitch, qt_pitch, scales_t_pitch;
};

// The row pass on one chunk: lane `sub` of a row's 16 holds 8 elements; the 4
// lanes of a 32-block meet for the amax, each lane stores its 8 bytes at `q`
// and the row's first lane the row's scale dword at `scales`. Whole waves
// call it.
template <typename T>
__device__ __forceinline__ void mx_row_chunk(act_t8<T> v, int sub, uint8_t *q,
                                             uint8_t *scales, bool aligned,
                                             bool scales_aligned) {
  float amax = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float f = (float)v[i];
    if (fp8_finite(f)) amax = fmaxf(amax, fabsf(f));
  }
  amax = fmaxf(amax, __shfl_xor(amax, 2));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  const float scale = mx_scale<false>(amax);
  const uint32_t byte = mx_scale_byte(scale);
  const int lane0 = (threadIdx.x & 63) & ~15;
  const uint32_t dword = (uint32_t)__shfl((int)byte, lane0) |
                         (uint32_t)__shfl((int)byte, lane0 + 4) << 8 |
                         (uint32_t)__shfl((int)byte, lane0 + 8) << 16 |
                         (uint32_t)__shfl((int)byte, lane0 + 12) << 24;
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i)
    w[i >> 2] |= fp8_quantize((float)v[i], scale) << (8 * (i & 3));
  if (aligned) *reinterpret_cast<uint2 *>(q) = make_uint2(w[0], w[1]);
  else store_bytes(q, w, 2, false);
  if (sub == 0) store_bytes(scales, &dword, 1, scales_aligned);
}

// The column pass over a staged [128][128] image of T (quantize_tile_mx has
// the map): `qt` / `scales_t` are the tile's first byte of each output,
// the pitches the bytes between consecutive columns. Every thread of the
// workgroup calls it, after the barrier that follows the staging.
template <typename T>
__device__ __forceinline__ void mx_column_pass(
    const T *image, uint8_t *col_scales, uint8_t *qt, long long qt_pitch,
    uint8_t *scales_t, long long scales_t_pitch, bool aligned_t,
    bool scales_t_aligned) {
  typedef T t2 __attribute__((ext_vector_type(2)));
  const int u = threadIdx.x >> 6, pair = threadIdx.x & 63;
  const T *from = image + u * kMxBlock * kTile + 2 * pair;
  t2 v[kMxBlock];
  float amax[2] = {0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < kMxBlock; ++i) {
    v[i] = *reinterpret_cast<const t2 *>(from + i * kTile);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float f = (float)v[i][j];
      if (fp8_finite(f)) amax[j] = fmaxf(amax[j], fabsf(f));
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = 2 * pair + j;
    const float scale = mx_scale<false>(amax[j]);
    col_scales[c * 4 + u] = (uint8_t)mx_scale_byte(scale);
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i)
      w[i >> 2] |= fp8_quantize((float)v[i][j], scale) << (8 * (i & 3));
    uint8_t *dst = qt + c * qt_pitch + u * kMxBlock;
    store16(dst, w, aligned_t);
    store16(dst + 16, w + 4, aligned_t);
  }
  __syncthreads();
  if (threadIdx.x < kTile) {
    const uint32_t dword = reinterpret_cast<const uint32_t *>(
        col_scales)[threadIdx.x];
    store_bytes(scales_t + threadIdx.x * scales_t_pitch, &dword, 1,
                scales_t_aligned);
  }
}

// A 128 x 128 tile of T at `x` (`pitch` elements between rows; z likewise
// for kOutActGrad) -> both MXFP8 images, the body QuantizeTilesMx and
// QuantizeBlocksMx share. Every thread of the workgroup calls it.
//
// Rows: 8 passes of 16 rows; a row is 16 lanes of 8 elements, a 32-block 4
// lanes: quantize_rows_mx_kernel's layout, shuffles and stores, so its bits.
// Columns: the staged values wait in `image`, [row][column] of T, and thread
// (wave u, lane l) owns the two units (column 2 l, rows 32 u .. 32 u + 31)
// and (column 2 l + 1, the same rows): 256 threads, 512 units. It reads the
// 32 dwords image[32 u + i][2 l .. 2 l + 1], has both amaxes and scales in
// registers with no cross-lane step, and leaves each unit's 32 bytes, which
// are contiguous along the tokens in qt, as two 16-byte stores. The four e8m0
// bytes of a column belong to four waves: they meet in `col_scales` [column]
// [u] and leave as one dword per column.
//
// LDS banks. The image needs neither padding nor a swizzle, because the lanes
// run along the image's rows on both sides. Write: lane `sub` of a row puts
// 16 bytes at byte 256 r + 16 sub and a wave covers rows 4 w' .. 4 w' + 3, so
// the wave's 64 x 16 bytes are one contiguous, 16-byte aligned kilobyte: every
// bank the same number of times, the minimum for that many bytes. Read: the
// 64 lanes of a wave take dword l of image row 32 u + i, 64 consecutive
// dwords: 64 banks once each (two rounds of 32 on a 32-bank view). A padded
// pitch would only misalign the 16-byte writes. col_scales is written by
// bytes, 2 per thread (columns 2 l and 2 l + 1 are dwords 2 l and 2 l + 1:
// two lanes per bank, twice per tile) and read as consecutive dwords.
template <typename T, int kMode>
__device__ __forceinline__ void quantize_tile_mx(
    const T *x, const T *z, long long pitch, int act, const MxTileSinks &o,
    const MxTileParams &p, T *image, uint8_t *col_scales) {
  const int sub = threadIdx.x & 15;
#pragma unroll 2
  for (int pass = 0; pass < kTile * kTile / 8 / kThreads; ++pass) {
    const int r = pass * (kThreads / 16) + (threadIdx.x >> 4);
    const long long at = r * pitch + sub * 8;
    act_t8<T> v = load8<T>(x + at, p.aligned);
    if constexpr (kMode != kModeNone) {
      using E = SddEpilogue<kMode>;
      act_t8<T> g = v, h, unused;
      if constexpr (E::kSideInputs >= 1) g = load8<T>(z + at, p.aligned);
      E::template apply8<T>(act, v, g, v, &h, &unused);
      v = h;
    }
    if (o.q != nullptr)
      mx_row_chunk<T>(v, sub, o.q + r * o.q_pitch + sub * 8,
                      o.scales + r * o.scales_pitch, p.aligned,
                      p.scales_aligned);
    if (o.qt != nullptr)
      *reinterpret_cast<act_t8<T> *>(image + r * kTile + sub * 8) = v;
  }
  if (o.qt == nullptr) return;
  __syncthreads();
  mx_column_pass<T>(image, col_scales, o.qt, o.qt_pitch, o.scales_t,
                    o.scales_t_pitch, p.aligned_t, p.scales_t_aligned);
}

template <typename T, int kMode>
__global__ void __launch_bounds__(kThreads)
    quantize_tiles_mx_kernel(const MxTileParams p) {
  __shared__ __attribute__((aligned(16))) T image[kTile * kTile];
  __shared__ __attribute__((aligned(4))) uint8_t col_scales[kTile * 4];
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
  const long long at = rb * kTile * p.cols + cb * kTile;
  const long long scale_pitch = p.cols / kMxBlock;
  MxTileSinks o{};
  if (p.q != nullptr) {
    o.q = p.q + at;
    o.q_pitch = p.cols;
    o.scales = p.scales + rb * kTile * scale_pitch + cb * 4;
    o.scales_pitch = scale_pitch;
  }
  if (p.qt != nullptr) {
    if (p.blocks) {  // output block blockIdx.x, [column][row]
      o.qt = p.qt + (long long)blockIdx.x * kTile * kTile;
      o.qt_pitch = kTile;
      o.scales_t = p.scales_t + (long long)blockIdx.x * kTile * 4;
      o.scales_t_pitch = 4;
    } else {
      o.qt = p.qt + cb * kTile * p.rows + rb * kTile;
      o.qt_pitch = p.rows;
      o.scales_t_pitch = p.rows / kMxBlock;
      o.scales_t = p.scales_t + cb * kTile * o.scales_t_pitch + rb * 4;
    }
  }
  const T *z = static_cast<const T *>(p.z);
  quantize_tile_mx<T, kMode>(static_cast<const T *>(p.x) + at,
                             z == nullptr ? nullptr : z + at, p.cols, p.act, o,
                             p, image, col_scales);
}

// QuantizeBlocksMxGatedGrad: one 128 x 128 block per workgroup. D, G and U are
// each read once, in quantize_tile_mx's row map (8 passes of 16 rows, 16
// lanes x 8 elements per row, 16-byte loads). The chunk's (dG, dU) come from
// the trait MatmulGatedGrad's elementwise stage calls, rounded to T. Set 0 is
// dG, set 1 dU. A set's row image is quantised from the registers by
// mx_row_chunk; for its column image the chunk is staged in the set's own
// unpadded [128][128] image of T and mx_column_pass walks it after one
// barrier. 2 x 32 KiB of images and 2 x 512 bytes of col_scales are 65 KiB:
// two workgroups still share a CU's 160 KiB.
//
// LDS banks: each image is written and read exactly as quantize_tile_mx's
// (its comment has the argument): a wave's 16-byte writes are one contiguous
// kilobyte, the column reads 64 consecutive dwords. The two images are 32 KiB
// apart, a multiple of every bank period, and are never touched by the same
// instruction, so they do not meet. A null pair is a workgroup-uniform test:
// it costs neither its shuffles and stores nor, for a column pair, its
// staging and its pass.
struct MxGateGradParams {
  const void *d, *g, *u;
  uint8_t *q[2], *scales[2], *qt[2], *scales_t[2];
  const int *block_offsets;
  int nnz_blocks, act;
  bool aligned, scales_aligned, aligned_t, scales_t_aligned;
};

template <typename T>
__global__ void __launch_bounds__(kThreads)
    quantize_gated_grad_mx_kernel(const MxGateGradParams p) {
  __shared__ __attribute__((aligned(16))) T image[2][kTile * kTile];
  __shared__ __attribute__((aligned(4))) uint8_t col_scales[2][kTile * 4];
  static_assert(2 * (sizeof(image) + sizeof(col_scales)) <= 160 * 1024,
                "two workgroups per CU");
  const bool columns = p.qt[0] != nullptr || p.qt[1] != nullptr;
  long long rb = blockIdx.x;
  if (columns) {  // output block blockIdx.x is source block block_offsets[..]
    const int b = p.block_offsets[blockIdx.x];
    if (b < 0 || b >= p.nnz_blocks) return;
    rb = b;
  }
  const T *d = static_cast<const T *>(p.d), *g = static_cast<const T *>(p.g),
          *u = static_cast<const T *>(p.u);
  const int sub = threadIdx.x & 15;
#pragma unroll 2
  for (int pass = 0; pass < kTile * kTile / 8 / kThreads; ++pass) {
    const int r = pass * (kThreads / 16) + (threadIdx.x >> 4);
    const long long row = rb * kTile + r, at = row * kTile + sub * 8;
    act_t8<T> o[2];
    SddEpilogue<kOutGateGrad>::template apply8<T>(
        p.act, load8<T>(d + at, p.aligned), load8<T>(g + at, p.aligned),
        load8<T>(u + at, p.aligned), &o[0], &o[1]);
#pragma unroll
    for (int set = 0; set < 2; ++set) {
      if (p.q[set] != nullptr)
        mx_row_chunk<T>(o[set], sub, p.q[set] + at, p.scales[set] + row * 4,
                        p.aligned, p.scales_aligned);
      if (p.qt[set] != nullptr)
        *reinterpret_cast<act_t8<T> *>(image[set] + r * kTile + sub * 8) =
            o[set];
    }
  }
  if (!columns) return;
  __syncthreads();
#pragma unroll
  for (int set = 0; set < 2; ++set)
    if (p.qt[set] != nullptr)
      mx_column_pass<T>(image[set], col_scales[set],
                        p.qt[set] + (long long)blockIdx.x * kTile * kTile,
                        kTile,
                        p.scales_t[set] + (long long)blockIdx.x * kTile * 4, 4,
                        p.aligned_t, p.scales_t_aligned);
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

// (a pair is given whole or not at all, and one of the two is given)
bool PairsOk(const void *q, const void *scales, const void *qt,
             const void *scales_t) {
  return (q == nullptr) == (scales == nullptr) &&
         (qt == nullptr) == (scales_t == nullptr) &&
         (q != nullptr || qt != nullptr);
}

template <int kMode>
hipError_t LaunchQuantizeTilesMx(MxTileParams p, long long tiles, int dtype,
                                 hipStream_t stream) {
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  p.aligned = Aligned({p.x, p.z}, 15) && Aligned({p.q}, 7);
  p.scales_aligned = Aligned({p.scales}, 3);
  p.aligned_t = Aligned({p.qt}, 15);
  p.scales_t_aligned = Aligned({p.scales_t}, 3);
  auto launch = [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((quantize_tiles_mx_kernel<T, kMode>),
                       dim3((unsigned)tiles), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
  };
  return dtype == 1 ? launch(__bf16{}) : launch(_Float16{});
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

template <int kMode>
hipError_t QuantizeRowsMxFp4Impl(const void *x, const void *gate, int rows,
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
  if (!Distinct({q, scales}, {x, gate})) return hipErrorInvalidValue;
  const long long tiles = (long long)rows * (cols / kTile);
  const long long want = (tiles + kThreads / 16 - 1) / (kThreads / 16);
  const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
  auto launch = [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((quantize_rows_mx_fp4_kernel<T, kMode>), dim3(grid),
                       dim3(kThreads), 0, stream, static_cast<const T *>(x),
                       static_cast<const T *>(gate), static_cast<uint8_t *>(q),
                       scales, tiles, act, Aligned({x, gate}, 15),
                       Aligned({q}, 15), Aligned({scales}, 3));
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

hipError_t QuantizeRowsMxFp4(const void *x, const void *gate, int rows,
                             int cols, MxStage stage, Activation activation,
                             void *q, uint8_t *scales, DataType dtype,
                             hipStream_t stream) {
  switch (stage) {
    case MxStage::kNone:
      return QuantizeRowsMxFp4Impl<kModeNone>(x, nullptr, rows, cols, 0, q,
                                              scales, (int)dtype, stream);
    case MxStage::kActivation:
      return QuantizeRowsMxFp4Impl<kOutAct>(x, nullptr, rows, cols,
                                            (int)activation, q, scales,
                                            (int)dtype, stream);
    case MxStage::kGated:
      return QuantizeRowsMxFp4Impl<kOutGate>(x, gate, rows, cols,
                                             (int)activation, q, scales,
                                             (int)dtype, stream);
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

hipError_t QuantizeTilesMx(const void *x, int rows, int cols, void *q,
                           uint8_t *scales, void *qt, uint8_t *scales_t,
                           DataType dtype, hipStream_t stream) {
  if (rows < 0 || cols < 0 || rows % kTile != 0 || cols % kTile != 0 ||
      ((int)dtype != 0 && (int)dtype != 1))
    return hipErrorInvalidValue;
  if (!PairsOk(q, scales, qt, scales_t)) return hipErrorInvalidValue;
  if (rows == 0 || cols == 0) return hipSuccess;
  if (x == nullptr || !Distinct({q, scales, qt, scales_t}, {x}))
    return hipErrorInvalidValue;
  MxTileParams p{x, nullptr, static_cast<uint8_t *>(q), scales,
                 static_cast<uint8_t *>(qt), scales_t, nullptr, rows, cols, 0,
                 0, false, false, false, false, false};
  return LaunchQuantizeTilesMx<kModeNone>(
      p, (long long)(rows / kTile) * (cols / kTile), (int)dtype, stream);
}

hipError_t QuantizeBlocksMx(const BlockMatrix s, MxBlockStage stage,
                            Activation activation, const void *z, void *q,
                            uint8_t *scales, void *qt, uint8_t *scales_t,
                            DataType dtype, hipStream_t stream) {
  if (s.block_size != BlockSize::k128 || s.nonzeros < 0 ||
      s.nonzeros % (kTile * kTile) != 0 ||
      ((int)dtype != 0 && (int)dtype != 1))
    return hipErrorInvalidValue;
  if (stage != MxBlockStage::kNone && stage != MxBlockStage::kActivation &&
      stage != MxBlockStage::kActivationGrad)
    return hipErrorInvalidValue;
  const int act = (int)activation;
  if (stage != MxBlockStage::kNone && (act < kActRelu || act > kActSilu))
    return hipErrorInvalidValue;
  if (!PairsOk(q, scales, qt, scales_t)) return hipErrorInvalidValue;
  if (s.nonzeros == 0) return hipSuccess;
  if (s.data == nullptr ||
      (stage == MxBlockStage::kActivationGrad && z == nullptr) ||
      (qt != nullptr && s.block_offsets == nullptr))
    return hipErrorInvalidValue;
  if (!Distinct({q, scales, qt, scales_t},
                {s.data, z, (const void *)s.block_offsets}))
    return hipErrorInvalidValue;
  const int blocks = s.nonzeros / (kTile * kTile);
  MxTileParams p{s.data,
                 stage == MxBlockStage::kActivationGrad ? z : nullptr,
                 static_cast<uint8_t *>(q), scales, static_cast<uint8_t *>(qt),
                 scales_t, static_cast<const int *>(s.block_offsets),
                 (long long)blocks * kTile, kTile, blocks, act, true, false,
                 false, false, false};
  switch (stage) {
    case MxBlockStage::kActivation:
      return LaunchQuantizeTilesMx<kOutAct>(p, blocks, (int)dtype, stream);
    case MxBlockStage::kActivationGrad:
      return LaunchQuantizeTilesMx<kOutActGrad>(p, blocks, (int)dtype, stream);
    default:
      return LaunchQuantizeTilesMx<kModeNone>(p, blocks, (int)dtype, stream);
  }
}

namespace {

bool MxBlocksOk(const BlockMatrix &s, Activation activation, DataType dtype) {
  const int act = (int)activation;
  return s.block_size == BlockSize::k128 && s.nonzeros >= 0 &&
         s.nonzeros % (kTile * kTile) == 0 &&
         ((int)dtype == 0 || (int)dtype == 1) && act >= kActRelu &&
         act <= kActSilu;
}

// Both pointers of each pair or neither, and `any`: one pair at least.
bool MxImagesOk(const MxImages &o, bool *any) {
  if ((o.q == nullptr) != (o.scales == nullptr) ||
      (o.qt == nullptr) != (o.scales_t == nullptr))
    return false;
  *any = *any || o.q != nullptr || o.qt != nullptr;
  return true;
}

}  // namespace

hipError_t QuantizeBlocksMxGated(const BlockMatrix s, const void *gate,
                                 Activation activation, MxImages h,
                                 DataType dtype, hipStream_t stream) {
  bool any = false;
  if (!MxBlocksOk(s, activation, dtype) || !MxImagesOk(h, &any) || !any)
    return hipErrorInvalidValue;
  if (s.nonzeros == 0) return hipSuccess;
  if (s.data == nullptr || gate == nullptr ||
      (h.qt != nullptr && s.block_offsets == nullptr))
    return hipErrorInvalidValue;
  if (!Distinct({h.q, h.scales, h.qt, h.scales_t},
                {s.data, gate, (const void *)s.block_offsets}))
    return hipErrorInvalidValue;
  const int blocks = s.nonzeros / (kTile * kTile);
  MxTileParams p{s.data, gate, static_cast<uint8_t *>(h.q), h.scales,
                 static_cast<uint8_t *>(h.qt), h.scales_t,
                 static_cast<const int *>(s.block_offsets),
                 (long long)blocks * kTile, kTile, blocks, (int)activation,
                 true, false, false, false, false};
  return LaunchQuantizeTilesMx<kOutGate>(p, blocks, (int)dtype, stream);
}

hipError_t QuantizeBlocksMxGatedGrad(const BlockMatrix d, const void *gate,
                                     const void *up, Activation activation,
                                     MxImages dg, MxImages du, DataType dtype,
                                     hipStream_t stream) {
  bool any = false;
  if (!MxBlocksOk(d, activation, dtype) || !MxImagesOk(dg, &any) ||
      !MxImagesOk(du, &any) || !any)
    return hipErrorInvalidValue;
  if (d.nonzeros == 0) return hipSuccess;
  const bool columns = dg.qt != nullptr || du.qt != nullptr;
  if (d.data == nullptr || gate == nullptr || up == nullptr ||
      (columns && d.block_offsets == nullptr))
    return hipErrorInvalidValue;
  if (!Distinct({dg.q, dg.scales, dg.qt, dg.scales_t, du.q, du.scales, du.qt,
                 du.scales_t},
                {d.data, gate, up, (const void *)d.block_offsets}))
    return hipErrorInvalidValue;
  const MxGateGradParams p{
      d.data, gate, up,
      {static_cast<uint8_t *>(dg.q), static_cast<uint8_t *>(du.q)},
      {dg.scales, du.scales},
      {static_cast<uint8_t *>(dg.qt), static_cast<uint8_t *>(du.qt)},
      {dg.scales_t, du.scales_t},
      static_cast<const int *>(d.block_offsets),
      d.nonzeros / (kTile * kTile), (int)activation,
      Aligned({d.data, gate, up}, 15) && Aligned({dg.q, du.q}, 7),
      Aligned({dg.scales, du.scales}, 3), Aligned({dg.qt, du.qt}, 15),
      Aligned({dg.scales_t, du.scales_t}, 3)};
  auto launch = [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((quantize_gated_grad_mx_kernel<T>),
                       dim3((unsigned)p.nnz_blocks), dim3(kThreads), 0, stream,
                       p);
    return hipGetLastError();
  };
  return (int)dtype == 1 ? launch(__bf16{}) : launch(_Float16{});
}

}  // namespace block
}  // namespace sputnik
