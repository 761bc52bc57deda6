// sputnik-amd: the fp8 (e4m3) block GEMM of sputnik/block/fp8.h: one kernel
// template, two tile sources (SDD and DSD). Both operands arrive
// k-contiguous, so no transposed LDS read is needed.
//
// One 256-thread workgroup (2 x 2 waves, 64 x 64 each) per 128 x 128 output
// tile. A step is one scale interval, a 128 x 128 e4m3 tile of each operand
// (16 KiB) plus the 128 row scales of A:
//
//   staging  16-byte LDS-DMA (global_load_lds) into a ring of kStages stages.
//            The DMA's LDS image is lane-linear, so the swizzle sits on the
//            source address: the lane that lands on 16-byte slot p of row r
//            fetches chunk p ^ key(r) of that row, key(r) = (r >> 1) & 7.
//            8 lanes still read one whole 128-byte line. The row scales go
//            the same way, 4 bytes per lane, so the loop has no
//            register-destination load beside the DMA.
//   reads    lane l of a wave (r = l % 16, g = l / 16) takes chunks g and
//            g + 4 of row r of a 16-row fragment with two ds_read_b128. With
//            128-byte rows two rows share a 256-byte bank row, and with that
//            key every 16-lane group of ds_read_b128 covers its 16 slots
//            once: conflict-free.
//   MFMA     kFp32 (the default): the e4m3 bytes are converted to fp16 in
//            registers, exactly (v_cvt_scalef32_pk_f16_fp8 with scale 1:
//            every e4m3 value is an fp16 value), and an interval is four
//            v_mfma_f32_16x16x32_f16 chained from zero. The fp8 forms
//            (v_mfma_scale_f32_16x16x128_f8f6f4, v_mfma_f32_16x16x32_fp8_fp8)
//            pass the exact lane-map test but do not sum in fp32: addends
//            far below the largest product of their group are dropped
//            (DESIGN has the measurement), past that mode's 2^-23 per
//            operation. kFast (Fp8Accumulate::kFast) is the scaled form: the
//            32 bytes of the two reads go to one
//            v_mfma_scale_f32_16x16x128_f8f6f4 as they come, both e8m0
//            scales 2^0, from +0; no convert, twice the MFMA rate. A and B
//            take the same (g, byte) -> k assignment, so the sum runs over
//            matching k whatever that assignment is; rows and columns are
//            l % 16 and the C/D map is the usual 16 x 16 one.
//   scaling  acc = fma(sa[row] * sb, P, acc) in fp32 with P the interval's
//            MFMA sum from zero, in both modes.
//   output   round_T(acc) once, through LDS, as 16-byte row pieces.
//
// The step order is the k order (SDD) or the row's storage order (DSD), no
// split-K and no atomics: the same inputs give the same bits. Every index
// read from device memory is checked before it is used as an address.
//
// kWgrad (DsdFp8Wgrad) is the DSD with a column-scaled dense operand: the
// interval scale is sa[row] * sb[kb, col]. The 128 column scales of a step
// ride in its stage behind the row scales, by the same 4-byte DMA (waves 2
// and 3; waves 0 and 1 fetch the row scales), so the loop still has no
// register-destination load; the stage grows by 512 bytes, two stages are
// 66 KiB and two workgroups still share a CU's 160 KiB. The output leaves
// through an fp32 image of the tile (64 KiB, inside the ring): round_out(acc)
// or round_out(acc + float(C_old)), to T or fp32. The forward kernels are the
// kWgrad = false instantiations, whose code does not change.
//
// fp8_interval_sums_kernel is the P of the contract as a callable
// (Fp8IntervalSums): cold, one wave per 16 x 16 tile and interval, the same
// two 16-byte reads per lane straight from global memory.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "api_internal.h"

namespace sputnik_amd {
namespace {

constexpr int kThreads = 256;
constexpr int kB = 128;                  // block edge = scale interval
constexpr int kTileBytes = kB * kB;      // one e4m3 operand tile
constexpr int kScaleBytes = kB * 4;      // the row scales of an A tile
// (kWgrad: the column scales of the B tile follow the row scales)
constexpr int StageBytes(bool wgrad) {
  return 2 * kTileBytes + (wgrad ? 2 : 1) * kScaleBytes;
}
// Two stages (65 KiB; 66 KiB with column scales) leave room for two
// workgroups per CU (the registers allow two waves per SIMD), which hide
// each other's barriers; the output tile reuses the ring.
constexpr int kStages = 2;
constexpr int LdsBytes(bool wgrad) { return kStages * StageBytes(wgrad); }
static_assert(kB * kB * 2 <= LdsBytes(false), "the output tile reuses the ring");
// (the wgrad's fp32 image: four floats of padding per row put the four row
// groups of a wave's store on different banks)
constexpr int kImagePitch = kB + 4;
static_assert(kB * kImagePitch * 4 <= LdsBytes(true), "... as fp32 too");
static_assert(2 * LdsBytes(true) <= 160 * 1024, "two workgroups per CU");

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#define SPUTNIK_FP8_LDS(p) ((__attribute__((address_space(3))) void *)(p))
#define SPUTNIK_FP8_GLOBAL(p) \
  ((const __attribute__((address_space(1))) void *)(p))

// Wave-uniform loads through the scalar cache: metadata and weight scales
// are read-only for the whole launch.
__device__ __forceinline__ int scalar_int(const int *p) {
  return *(const __attribute__((address_space(4))) int *)p;
}
__device__ __forceinline__ float scalar_float(const float *p) {
  return *(const __attribute__((address_space(4))) float *)p;
}
// (an int16 entry from its aligned dword: any 2-byte-aligned base works)
__device__ __forceinline__ int scalar_short(const short *p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const int v = *reinterpret_cast<const __attribute__((address_space(4))) int *>(
      a & ~uintptr_t(3));
  return (short)((a & 2) ? (v >> 16) : v);
}

__device__ __forceinline__ int swizzle_key(int row) { return (row >> 1) & 7; }

// 8 e4m3 bytes as 8 fp16 values, exactly (NaN bytes stay NaN).
__device__ __forceinline__ f16x8 e4m3_to_f16x8(int lo, int hi) {
  const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false);
  const f16x2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true);
  const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false);
  const f16x2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true);
  return f16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// The operands of an interval's MFMAs from a lane's two 16-byte reads (k =
// 16 g .. 16 g + 15 and 64 + 16 g .. 64 + 16 g + 15): four fp16 quarters
// (kFp32), or the 32 bytes as they come (kFast).
template <bool kFast>
struct Fragment;
template <>
struct Fragment<false> {
  f16x8 k[4];
  __device__ __forceinline__ Fragment() = default;
  __device__ __forceinline__ Fragment(i32x4 lo, i32x4 hi)
      : k{e4m3_to_f16x8(lo[0], lo[1]), e4m3_to_f16x8(lo[2], lo[3]),
          e4m3_to_f16x8(hi[0], hi[1]), e4m3_to_f16x8(hi[2], hi[3])} {}
};
template <>
struct Fragment<true> {
  i32x8 v;
  __device__ __forceinline__ Fragment() = default;
  __device__ __forceinline__ Fragment(i32x4 lo, i32x4 hi)
      : v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]} {}
};

// P of one interval and one 16 x 16 tile, from +0.
constexpr int kE8m0One = 0x7F7F7F7F;  // 2^0 in every byte
__device__ __forceinline__ f32x4 interval_sum(const Fragment<false> &a,
                                              const Fragment<false> &b) {
  f32x4 sum{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int q = 0; q < 4; ++q)
    sum = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.k[q], b.k[q], sum, 0, 0, 0);
  return sum;
}
__device__ __forceinline__ f32x4 interval_sum(const Fragment<true> &a,
                                              const Fragment<true> &b) {
  // (cbsz = blgp = 0: both operands e4m3; opsel 0: the scales' byte 0)
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a.v, b.v, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0, kE8m0One, 0,
      kE8m0One);
}

struct Fp8GemmParams {
  const char *a;          // SDD: Aq [m, k]; DSD: the stored blocks of Sq
  const float *a_scales;  // SDD: [m, k / 128]; DSD: [nnz_blocks * 128]
  const char *b;          // Bq [n, k]
  const float *b_scales;  // [k / 128, n / 128]; kWgrad: [k / 128, n]
  void *c;                // SDD: block values of C; DSD: C [m, n]
  const int *offsets;     // DSD: the sparse operand's row offsets
  const short *indices;   // SDD: C's column indices; DSD: Sq's
  const short *row_indices;  // SDD: C's
  int m_blocks, n_blocks, k_blocks, nnz_blocks;
  int out_f32, add;       // kWgrad: C holds fp32; C += (accumulate.h)
};

template <typename T, bool kDsd, bool kFast, bool kWgrad = false>
__global__ void __launch_bounds__(kThreads)
    fp8_gemm_kernel(const Fp8GemmParams p) {
  static_assert(kDsd || !kWgrad, "the column-scaled product is a DSD");
  constexpr int kStageBytes = StageBytes(kWgrad);
  constexpr int kLdsBytes = LdsBytes(kWgrad);
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long k_bytes = (long long)p.k_blocks * kB;

  // The output tile and its steps.
  int rb, nb, first = 0, steps;
  if constexpr (kDsd) {
    rb = blockIdx.x / p.n_blocks;
    nb = blockIdx.x % p.n_blocks;
    int begin = scalar_int(p.offsets + rb), end = scalar_int(p.offsets + rb + 1);
    begin = begin < 0 ? 0 : begin;
    end = end > p.nnz_blocks ? p.nnz_blocks : end;
    first = begin;
    steps = end > begin ? end - begin : 0;
    // (accumulate.h: a block row without blocks is neither read nor written)
    if constexpr (kWgrad) if (p.add && steps == 0) return;
  } else {
    rb = scalar_short(p.row_indices + blockIdx.x);
    nb = scalar_short(p.indices + blockIdx.x);
    if (rb < 0 || rb >= p.m_blocks || nb < 0 || nb >= p.n_blocks) return;
    steps = p.k_blocks;
  }
  // The k-block of step i, or -1 for a stored block to skip.
  auto k_block = [&](int i) {
    if constexpr (!kDsd) return i;
    const int kb = scalar_short(p.indices + first + i);
    return kb >= 0 && kb < p.k_blocks ? kb : -1;
  };

  // One step's DMA into `stage`.
  auto issue = [&](int i, char *stage) {
    const int kb = k_block(i);
    if (kb < 0) return;
    const char *a_tile;
    long long a_pitch;
    const float *a_scale;
    long long a_scale_stride;
    if constexpr (kDsd) {
      a_tile = p.a + (long long)(first + i) * kTileBytes;
      a_pitch = kB;
      a_scale = p.a_scales + (long long)(first + i) * kB;
      a_scale_stride = 1;
    } else {
      a_tile = p.a + (long long)rb * kB * k_bytes + (long long)kb * kB;
      a_pitch = k_bytes;
      a_scale = p.a_scales + (long long)rb * kB * p.k_blocks + kb;
      a_scale_stride = p.k_blocks;
    }
    const char *b_tile = p.b + (long long)nb * kB * k_bytes + (long long)kb * kB;
#pragma unroll
    for (int pass = 0; pass < kTileBytes / (kThreads * 16); ++pass) {
      // (a wave's 64 x 16 bytes are 8 rows of the image)
      const int piece = pass * (kThreads * 16) + wave * 1024;
      const int row = (piece >> 7) + (lane >> 3);
      const int chunk = (lane & 7) ^ swizzle_key(row);
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_FP8_GLOBAL(a_tile + row * a_pitch + chunk * 16),
          SPUTNIK_FP8_LDS(stage + piece), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_FP8_GLOBAL(b_tile + row * k_bytes + chunk * 16),
          SPUTNIK_FP8_LDS(stage + kTileBytes + piece), 16, 0, 0);
    }
    if (wave < kB / 64) {
      const int row = wave * 64 + lane;
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_FP8_GLOBAL(a_scale + row * a_scale_stride),
          SPUTNIK_FP8_LDS(stage + 2 * kTileBytes + wave * 256), 4, 0, 0);
    } else if constexpr (kWgrad) {
      const int col = (wave - kB / 64) * 64 + lane;
      const long long n = (long long)p.n_blocks * kB;
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_FP8_GLOBAL(p.b_scales + kb * n + (long long)nb * kB + col),
          SPUTNIK_FP8_LDS(stage + 2 * kTileBytes + wave * 256), 4, 0, 0);
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 15, g = lane >> 4;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // A 16-row fragment of an operand image: chunks g and g + 4 of row r.
  using Frag = Fragment<kFast>;
  auto fragment = [&](const char *image, int row0) {
    const int row = row0 + r;
    const char *at = image + row * kB;
    const int key = swizzle_key(row);
    const i32x4 lo = *reinterpret_cast<const i32x4 *>(at + ((g ^ key) << 4));
    const i32x4 hi =
        *reinterpret_cast<const i32x4 *>(at + (((g + 4) ^ key) << 4));
    return Frag(lo, hi);
  };

  auto compute = [&](int i, const char *stage) {
    const int kb = k_block(i);
    if (kb < 0) return;
    float sb = 1.0f;  // kWgrad: per column, from the stage
    if constexpr (!kWgrad)
      sb = scalar_float(p.b_scales + (long long)kb * p.n_blocks + nb);
    const float *sa_lds =
        reinterpret_cast<const float *>(stage + 2 * kTileBytes);
    Frag a[4];
    f32x4 s[4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
      a[ti] = fragment(stage, wm * 64 + ti * 16);
      // (the lane's four accumulator rows of this fragment)
      s[ti] = *reinterpret_cast<const f32x4 *>(sa_lds + wm * 64 + ti * 16 +
                                               4 * g) * sb;
    }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      const Frag b = fragment(stage + kTileBytes, wn * 64 + tj * 16);
      if constexpr (kWgrad) sb = sa_lds[kB + wn * 64 + tj * 16 + r];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        const f32x4 sum = interval_sum(a[ti], b);
        // (kWgrad: s is sa alone so far; sa * sb is rounded, then the fma)
        const f32x4 st = kWgrad ? s[ti] * sb : s[ti];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[ti][tj][e] = __builtin_fmaf(st[e], sum[e], acc[ti][tj][e]);
      }
    }
  };

  // Stage i lands while stage i - 1 is consumed: the barrier that follows
  // the wait also says every wave is done with the stage about to be
  // refilled.
  if (steps > 0) issue(0, lds);
  for (int i = 0; i < steps; ++i) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (i + 1 < steps) issue(i + 1, lds + ((i + 1) % kStages) * kStageBytes);
    compute(i, lds + (i % kStages) * kStageBytes);
  }

  __syncthreads();
  if constexpr (kWgrad) {
    // acc into a [128][kImagePitch] fp32 image, then 16-byte row pieces of the
    // output type: round_out(acc), or round_out(acc + float(C_old)).
    float *image = reinterpret_cast<float *>(lds);
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          image[(wm * 64 + ti * 16 + 4 * g + e) * kImagePitch + wn * 64 +
                tj * 16 + r] = acc[ti][tj][e];
    __syncthreads();
    const long long n = (long long)p.n_blocks * kB;
    const long long at = (long long)rb * kB * n + (long long)nb * kB;
    if (p.out_f32) {
      float *out = static_cast<float *>(p.c) + at;
      for (int id = threadIdx.x; id < kB * kB / 4; id += kThreads) {
        const int row = id >> 5, col = (id & 31) * 4;
        f32x4 v = *reinterpret_cast<const f32x4 *>(image + row * kImagePitch + col);
        f32x4 *dst = reinterpret_cast<f32x4 *>(out + row * n + col);
        if (p.add) v += *dst;
        *dst = v;
      }
    } else {
      typedef T t8 __attribute__((ext_vector_type(8)));
      T *out = static_cast<T *>(p.c) + at;
      for (int id = threadIdx.x; id < kB * kB / 8; id += kThreads) {
        const int row = id >> 4, col = (id & 15) * 8;
        t8 *dst = reinterpret_cast<t8 *>(out + row * n + col);
        t8 old{}, res;
        if (p.add) old = *dst;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float v = image[row * kImagePitch + col + i];
          if (p.add) v += (float)old[i];
          res[i] = (T)v;
        }
        *dst = res;
      }
    }
    return;
  }
  // round_T(acc) into a [128][128] image of T, then 16-byte row pieces.
  T *image = reinterpret_cast<T *>(lds);
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        image[(wm * 64 + ti * 16 + 4 * g + e) * kB + wn * 64 + tj * 16 + r] =
            (T)acc[ti][tj][e];
  __syncthreads();
  char *out;
  long long out_pitch;  // bytes
  if constexpr (kDsd) {
    out_pitch = (long long)p.n_blocks * kB * 2;
    out = static_cast<char *>(p.c) + (long long)rb * kB * out_pitch +
          (long long)nb * kB * 2;
  } else {
    out_pitch = kB * 2;
    out = static_cast<char *>(p.c) + (long long)blockIdx.x * kB * kB * 2;
  }
  for (int id = threadIdx.x; id < kB * kB * 2 / 16; id += kThreads) {
    const int row = id >> 4, piece = (id & 15) * 16;
    *reinterpret_cast<i32x4 *>(out + row * out_pitch + piece) =
        *reinterpret_cast<const i32x4 *>(lds + row * kB * 2 + piece);
  }
}

// P [k / 128, m, n] of aq [m, k] and bq [n, k]: workgroup (kb, tm, tn) is
// one wave and one 16 x 16 tile of one interval.
template <bool kFast>
__global__ void __launch_bounds__(64)
    fp8_interval_sums_kernel(const char *aq, const char *bq, float *out,
                             int m, int n, int k) {
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int tiles_n = n >> 4, tiles_m = m >> 4;
  const int tn = blockIdx.x % tiles_n;
  const int tm = blockIdx.x / tiles_n % tiles_m;
  const int kb = blockIdx.x / tiles_n / tiles_m;
  auto fragment = [&](const char *base, int row0) {
    const char *at = base + (long long)(row0 + r) * k + (long long)kb * kB;
    return Fragment<kFast>(
        *reinterpret_cast<const i32x4 *>(at + 16 * g),
        *reinterpret_cast<const i32x4 *>(at + 64 + 16 * g));
  };
  const f32x4 sum =
      interval_sum(fragment(aq, tm * 16), fragment(bq, tn * 16));
  float *tile = out + ((long long)kb * m + tm * 16 + 4 * g) * n + tn * 16 + r;
#pragma unroll
  for (int e = 0; e < 4; ++e) tile[(long long)e * n] = sum[e];
}

}  // namespace

hipError_t LaunchFp8IntervalSums(const void *aq, const void *bq, int m, int n,
                                 int k, bool fast, float *out,
                                 hipStream_t stream) {
  const long long tiles = (long long)(m / 16) * (n / 16) * (k / kB);
  if (tiles == 0) return hipSuccess;
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  const char *a = static_cast<const char *>(aq);
  const char *b = static_cast<const char *>(bq);
  if (fast)
    hipLaunchKernelGGL(fp8_interval_sums_kernel<true>, dim3((unsigned)tiles),
                       dim3(64), 0, stream, a, b, out, m, n, k);
  else
    hipLaunchKernelGGL(fp8_interval_sums_kernel<false>, dim3((unsigned)tiles),
                       dim3(64), 0, stream, a, b, out, m, n, k);
  return hipGetLastError();
}

hipError_t LaunchFp8Gemm(bool dsd, bool fast, int dtype, const void *a,
                         const float *a_scales, const void *b,
                         const float *b_scales, void *c, const int *offsets,
                         const short *indices, const short *row_indices,
                         int m_blocks, int n_blocks, int k_blocks,
                         int nnz_blocks, hipStream_t stream) {
  const long long tiles =
      dsd ? (long long)m_blocks * n_blocks : (long long)nnz_blocks;
  if (tiles == 0) return hipSuccess;
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  const Fp8GemmParams p{static_cast<const char *>(a), a_scales,
                        static_cast<const char *>(b), b_scales, c, offsets,
                        indices, row_indices, m_blocks, n_blocks, k_blocks,
                        nnz_blocks, 0, 0};
  auto launch = [&](auto t, auto d, auto f) {
    hipLaunchKernelGGL((fp8_gemm_kernel<decltype(t), decltype(d)::value,
                                        decltype(f)::value>),
                       dim3((unsigned)tiles), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
  };
  auto kind = [&](auto t, auto d) {
    return fast ? launch(t, d, std::true_type{})
                : launch(t, d, std::false_type{});
  };
  if (dsd)
    return dtype == 1 ? kind(__bf16{}, std::true_type{})
                      : kind(_Float16{}, std::true_type{});
  return dtype == 1 ? kind(__bf16{}, std::false_type{})
                    : kind(_Float16{}, std::false_type{});
}

hipError_t LaunchFp8Wgrad(bool fast, int dtype, bool out_f32, bool add,
                          const void *s, const float *s_scales, const void *b,
                          const float *b_scales, void *c, const int *offsets,
                          const short *indices, int m_blocks, int n_blocks,
                          int k_blocks, int nnz_blocks, hipStream_t stream) {
  const long long tiles = (long long)m_blocks * n_blocks;
  if (tiles == 0) return hipSuccess;
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  const Fp8GemmParams p{static_cast<const char *>(s), s_scales,
                        static_cast<const char *>(b), b_scales, c, offsets,
                        indices, nullptr, m_blocks, n_blocks, k_blocks,
                        nnz_blocks, out_f32, add};
  auto launch = [&](auto t, auto f) {
    hipLaunchKernelGGL((fp8_gemm_kernel<decltype(t), true, decltype(f)::value,
                                        true>),
                       dim3((unsigned)tiles), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
  };
  auto kind = [&](auto t) {
    return fast ? launch(t, std::true_type{}) : launch(t, std::false_type{});
  };
  return dtype == 1 ? kind(__bf16{}) : kind(_Float16{});
}

}  // namespace sputnik_amd
