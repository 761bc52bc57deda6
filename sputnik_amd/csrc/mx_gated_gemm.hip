// sputnik-amd: the fused gated MX SDD of sputnik/block/mx.h (SddMxGated): both
// products of a GLU expert, G = Aq . gate^T and U = Aq . up^T at the stored
// blocks, their biases, the gate stage and the MXFP8 image of H = U * act(G)
// (or the clamped SwiGLU) from one kernel. A kernel of its own beside
// mx_gemm.hip: that file's instantiations are untouched.
//
// One 256-thread workgroup (2 x 2 waves, 64 x 64 each) per stored block. A step
// is one k-block of 128. A stage of the ring holds
//
//   A tile       128 rows x 128 bytes, fetched once         16 KiB
//   gate tile    128 rows x 128 bytes (e4m3) or 64 (e2m1)   16 / 8 KiB
//   up tile      likewise                                   16 / 8 KiB
//   scales       three dword columns: A rows, gate columns,
//                up columns, 128 dwords each                1.5 KiB
//
// 49.5 KiB (e4m3) or 33.5 KiB (e2m1); two stages: 99 KiB, one workgroup per
// CU, or 67 KiB, two per CU. Timed against the three launches it replaces
// ("MX forward path"): the e2m1 kernel takes 0.94 x / 0.90 x of
// their time, the e4m3 kernel 1.36 x / 1.13 x: with one resident workgroup
// nothing runs under its wait and barrier. The e4m3 alternative, 128 x 64 H
// tiles with two workgroups resident (A read twice per hidden block, 16 MFMAs
// behind each barrier again), has not been timed against this one.
//
//   staging  mx_gemm.hip's: 16-byte LDS-DMA (global_load_lds) for the tiles,
//            4-byte for the scale dwords, the swizzle on the source address.
//            The six 64-dword scale units (A 0 - 1, gate 2 - 3, up 4 - 5) go
//            to waves 0 .. 3 and again to waves 0, 1. Logical weight row n is
//            physical row b_row_step n of its base pointer, bytes and scales
//            alike: an interleaved [2 F, k] tensor is gate = base, up = base +
//            one row, step 2.
//   banks    The DMA's image is lane-linear and each tile starts on a 16 KiB
//            or 8 KiB boundary of the stage, the stage on a multiple of 512
//            bytes (49.5 KiB = 99 x 512, 33.5 KiB = 67 x 512): a multiple of the
//            256-byte bank row. So inside every tile, whichever stage, row r of
//            128 bytes sits in half r & 1 of bank row r >> 1, exactly as in
//            mx_gemm.hip, and its argument carries over unchanged: the 16 lanes
//            of a group read chunk c of rows r = 0 .. 15 at slots (r & 1, c ^
//            key8(r)), key8(r) = (r >> 1) & 7: 16 different pairs, 16 slots
//            once each, for any c. A 64-byte e2m1 row: slot (r & 3, c ^
//            key4(r)), key4(r) = (r >> 2) & 3, again 16 different pairs. The
//            scale columns are read as dword r of 16 consecutive dwords per
//            lane group (the four groups the same 16: a broadcast).
//   compute  per wave acc_g[4][4] and acc_u[4][4], 128 accumulator registers.
//            The four A fragments and their shifted scale dwords are read once
//            per step and meet the gate and then the up fragment of each
//            column tile: 32 MFMAs behind one wait and one barrier. Each
//            product is SddMx's: v_mfma_scale_f32_16x16x128_f8f6f4 from a +0
//            accumulator, then one fp32 add, k ascending.
//   epilogue in registers, per element, fp32 with no contraction (mx.h has the
//            contract): G = round_T(acc_g) (+ bias, bias.h's rule), U
//            likewise, H = round_T(U act(G) + 0) or the clamped SwiGLU.
//            Each of G, U (when kept) and H then passes through one [128]
//            [128] image of T at the start of the ring, one after the other
//            (the e2m1 ring has room for two, not three), and leaves as
//            16-byte row pieces; an output that is null is never staged. The
//            32-column amax of H is taken through that image, not across the
//            accumulator lanes: 8 lanes per row, 16 elements (two 16-byte LDS
//            reads, consecutive lanes consecutive addresses) per lane, so a
//            32-block is 2 lanes and one cross-lane step; the lane stores its
//            16 e4m3 bytes as one piece, and the row's four e8m0 bytes meet
//            in the row's first lane and leave as one dword. The values are
//            the T image's and the rules mx_math.h's, so the bytes are
//            QuantizeRowsMx(kNone)'s of h_out whether or not h_out is stored.
//
// No split-K, no atomics, no hand-off: the same inputs give the same bits.
// The two indices read from device memory are checked before they are used
// as addresses; an out-of-range block is skipped.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "act_math.h"
#include "api_internal.h"
#include "lowp_tile.h"
#include "mx_math.h"

namespace sputnik_amd {
namespace {

// kThreads, kB (the block edge = one step of k), the vector types, the
// scalar loads and the swizzle keys: lowp_tile.h.
using namespace lowp;

constexpr int kATileBytes = kB * kB;
constexpr int BTileBytes(bool b4) { return b4 ? kB * kB / 2 : kB * kB; }
constexpr int kScaleBytes = kB * 4;      // one dword per row (column)
constexpr int StageBytes(bool b4) {
  return kATileBytes + 2 * BTileBytes(b4) + 3 * kScaleBytes;
}
constexpr int kStages = 2;
constexpr int LdsBytes(bool b4) { return kStages * StageBytes(b4); }
static_assert(StageBytes(false) == 49 * 1024 + 512 &&
                  StageBytes(true) == 33 * 1024 + 512,
              "the stage sizes of the header");
static_assert(LdsBytes(false) <= 160 * 1024 && 2 * LdsBytes(false) > 160 * 1024,
              "e4m3: one workgroup per CU");
static_assert(2 * LdsBytes(true) <= 160 * 1024, "e2m1: two workgroups per CU");
static_assert(StageBytes(false) % 256 == 0 && StageBytes(true) % 256 == 0 &&
                  BTileBytes(true) % 256 == 0,
              "every tile starts on a bank row");
static_assert(kB * kB * 2 <= LdsBytes(true), "the output image reuses the ring");

struct MxGatedParams {
  const char *a;            // Aq [m, k]
  const uint8_t *a_scales;  // [m, k / 32]
  const char *gate, *up;    // row n at b_row_step n rows of [k] or [k / 2] bytes
  const uint8_t *gate_scales, *up_scales;  // likewise, rows of k / 32 bytes
  const void *gate_bias, *up_bias;         // T [n] or null
  uint8_t *hq, *h_scales;   // [nnz_blocks, 128, 128], [nnz_blocks 128, 4]
  void *g_out, *u_out, *h_out;  // block values of T or null
  const short *indices, *row_indices;
  int m_blocks, n_blocks, k_blocks, b_row_step;
  int clamped, act;         // MxGluKind; Activation of kPlain
  float alpha, limit;
};

// H of one element from G and U as floats of T values (mx.h, "Fused gated
// SDD"). The sigmoid of the clamped kind is silu's: act_sigmoid of the
// argument held to +-100.
template <typename T>
__device__ __forceinline__ T glu_stage(const MxGatedParams &p, T g, T u) {
#pragma clang fp contract(off)
  if (!p.clamped) return gate_forward<T>(p.act, u, g);
  const float gf = (float)g, uf = (float)u;
  const float gc = gf > p.limit ? p.limit : gf;
  const float uc = uf > p.limit ? p.limit : (uf < -p.limit ? -p.limit : uf);
  const float s = act_sigmoid<float>(act_clamp(p.alpha * gc, 100.0f));
  return (T)((uc + 1.0f) * (gc * s) + 0.0f);
}

template <typename T, bool kB4>
__global__ void __launch_bounds__(kThreads)
    mx_gated_kernel(const MxGatedParams p) {
  constexpr int kStageBytes = StageBytes(kB4);
  constexpr int kGateOff = kATileBytes;
  constexpr int kUpOff = kATileBytes + BTileBytes(kB4);
  constexpr int kScaleOff = kATileBytes + 2 * BTileBytes(kB4);
  constexpr int kBRow = kB4 ? kB / 2 : kB;  // bytes of a B row in a tile
  __shared__ __attribute__((aligned(256))) char lds[LdsBytes(kB4)];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long k_bytes = (long long)p.k_blocks * kB;
  // (bytes between consecutive logical weight rows, and between their scales)
  const long long b_pitch = (kB4 ? k_bytes / 2 : k_bytes) * p.b_row_step;
  const long long b_scale_pitch = (long long)p.k_blocks * 4 * p.b_row_step;

  const int rb = scalar_short(p.row_indices + blockIdx.x);
  const int nb = scalar_short(p.indices + blockIdx.x);
  if (rb < 0 || rb >= p.m_blocks || nb < 0 || nb >= p.n_blocks) return;
  const int steps = p.k_blocks;

  // One step's DMA into `stage`.
  auto issue = [&](int kb, char *stage) {
    const char *a_tile = p.a + (long long)rb * kB * k_bytes + (long long)kb * kB;
#pragma unroll
    for (int pass = 0; pass < kATileBytes / (kThreads * 16); ++pass) {
      // (a wave's 64 x 16 bytes are 8 rows of the image)
      const int piece = pass * (kThreads * 16) + wave * 1024;
      const int row = (piece >> 7) + (lane >> 3);
      const int chunk = (lane & 7) ^ key8(row);
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL(a_tile + row * k_bytes + chunk * 16),
          SPUTNIK_LOWP_LDS(stage + piece), 16, 0, 0);
    }
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      const char *b_tile = (which ? p.up : p.gate) +
                           (long long)nb * kB * b_pitch + (long long)kb * kBRow;
      char *to = stage + (which ? kUpOff : kGateOff);
#pragma unroll
      for (int pass = 0; pass < BTileBytes(kB4) / (kThreads * 16); ++pass) {
        const int piece = pass * (kThreads * 16) + wave * 1024;
        int row, chunk;
        if constexpr (kB4) {  // 16 rows of 64 bytes
          row = (piece >> 6) + (lane >> 2);
          chunk = (lane & 3) ^ key4(row);
        } else {
          row = (piece >> 7) + (lane >> 3);
          chunk = (lane & 7) ^ key8(row);
        }
        __builtin_amdgcn_global_load_lds(
            SPUTNIK_LOWP_GLOBAL(b_tile + row * b_pitch + chunk * 16),
            SPUTNIK_LOWP_LDS(to + piece), 16, 0, 0);
      }
    }
    // Scale units of 64 dwords: 0, 1 the A rows, 2, 3 the gate columns, 4, 5
    // the up columns; wave w takes unit w, waves 0 and 1 also unit w + 4.
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int unit = wave + 4 * round;
      if (unit >= 6) break;
      const int at = (unit & 1) * 64 + lane;  // row or column of the tile
      const uint8_t *src;
      if (unit < 2) {
        src = p.a_scales +
              ((long long)(rb * kB + at) * p.k_blocks + kb) * 4;
      } else {
        src = (unit < 4 ? p.gate_scales : p.up_scales) +
              (long long)(nb * kB + at) * b_scale_pitch + kb * 4;
      }
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL(src),
          SPUTNIK_LOWP_LDS(stage + kScaleOff + unit * 256), 4, 0, 0);
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 15, g = lane >> 4;
  f32x4 acc_g[4][4], acc_u[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc_g[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      acc_u[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

  // The lane's 32 k-elements of row row0 + r, where the instruction wants
  // them (mx_gemm.hip): e4m3, chunks g and g + 4; e2m1, chunk g.
  auto fragment8 = [&](const char *image, int row0) {
    const int row = row0 + r;
    const char *at = image + row * kB;
    const int key = key8(row);
    const i32x4 lo = *reinterpret_cast<const i32x4 *>(at + ((g ^ key) << 4));
    const i32x4 hi =
        *reinterpret_cast<const i32x4 *>(at + (((g + 4) ^ key) << 4));
    return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  auto fragment4 = [&](const char *image, int row0) {
    const int row = row0 + r;
    const i32x4 v = *reinterpret_cast<const i32x4 *>(
        image + row * (kB / 2) + ((g ^ key4(row)) << 4));
    return i32x8{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
  };
  auto b_fragment = [&](const char *image, int row0) {
    if constexpr (kB4) return fragment4(image, row0);
    else return fragment8(image, row0);
  };

  auto compute = [&](const char *stage) {
    const int *scale_lds = reinterpret_cast<const int *>(stage + kScaleOff);
    i32x8 a[4];
    int sa[4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
      a[ti] = fragment8(stage, wm * 64 + ti * 16);
      sa[ti] = (unsigned)scale_lds[wm * 64 + ti * 16 + r] >> (8 * g);
    }
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      const int col = wn * 64 + tj * 16;
      const i32x8 bg = b_fragment(stage + kGateOff, col);
      const int sg = (unsigned)scale_lds[kB + col + r] >> (8 * g);
      const i32x8 bu = b_fragment(stage + kUpOff, col);
      const int su = (unsigned)scale_lds[2 * kB + col + r] >> (8 * g);
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        // (cbsz 0: A is e4m3; blgp 0 / 4: B is e4m3 / e2m1; opsel 0: byte 0)
        const f32x4 pg = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a[ti], bg, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, kB4 ? 4 : 0, 0, sa[ti],
            0, sg);
        acc_g[ti][tj] += pg;
      }
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        const f32x4 pu = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a[ti], bu, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, kB4 ? 4 : 0, 0, sa[ti],
            0, su);
        acc_u[ti][tj] += pu;
      }
    }
  };

  // Stage i + 1 lands while stage i is consumed: the barrier that follows the
  // wait also says every wave is done with the stage about to be refilled.
  if (steps > 0) issue(0, lds);
  for (int i = 0; i < steps; ++i) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (i + 1 < steps) issue(i + 1, lds + ((i + 1) % kStages) * kStageBytes);
    compute(lds + (i % kStages) * kStageBytes);
  }

  // G, U and H of the lane's elements, each a value of T, in place of the
  // accumulators: element e of acc_x[ti][tj] holds the T value as a float.
  const T *gate_bias = static_cast<const T *>(p.gate_bias);
  const T *up_bias = static_cast<const T *>(p.up_bias);
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    const long long col = (long long)nb * kB + wn * 64 + tj * 16 + r;
    T bg = (T)0.0f, bu = (T)0.0f;
    if (gate_bias != nullptr) bg = gate_bias[col];
    if (up_bias != nullptr) bu = up_bias[col];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        T gv = (T)acc_g[ti][tj][e], uv = (T)acc_u[ti][tj][e];
        if (gate_bias != nullptr) gv = bias_add<T>(gv, bg);
        if (up_bias != nullptr) uv = bias_add<T>(uv, bu);
        acc_g[ti][tj][e] = (float)gv;
        acc_u[ti][tj][e] = (float)uv;
      }
  }

  // One [128][128] image of T at a time, then 16-byte row pieces.
  T *image = reinterpret_cast<T *>(lds);
  auto stage_image = [&](f32x4 (&v)[4][4]) {
    __syncthreads();  // the ring, or the image before this one, is done with
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          image[(wm * 64 + ti * 16 + 4 * g + e) * kB + wn * 64 + tj * 16 + r] =
              (T)v[ti][tj][e];
    __syncthreads();
  };
  auto store_image = [&](void *out_blocks) {
    char *out = static_cast<char *>(out_blocks) +
                (long long)blockIdx.x * kB * kB * 2;
    for (int id = threadIdx.x; id < kB * kB * 2 / 16; id += kThreads)
      *reinterpret_cast<i32x4 *>(out + id * 16) =
          *reinterpret_cast<const i32x4 *>(lds + id * 16);
  };
  if (p.g_out != nullptr) {
    stage_image(acc_g);
    store_image(p.g_out);
  }
  if (p.u_out != nullptr) {
    stage_image(acc_u);
    store_image(p.u_out);
  }
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        acc_u[ti][tj][e] = (float)glu_stage<T>(p, (T)acc_g[ti][tj][e],
                                               (T)acc_u[ti][tj][e]);
  stage_image(acc_u);
  if (p.h_out != nullptr) store_image(p.h_out);

  // The MXFP8 image of H: lane `sub` of a row's 8 holds 16 elements, a
  // 32-block is lanes sub & ~1, sub | 1.
  uint8_t *hq = p.hq + (long long)blockIdx.x * kB * kB;
  uint8_t *h_scales = p.h_scales + (long long)blockIdx.x * kB * 4;
  const int sub = threadIdx.x & 7;
#pragma unroll 1
  for (int pass = 0; pass < kB * 8 / kThreads; ++pass) {
    const int row = pass * (kThreads / 8) + (threadIdx.x >> 3);
    typedef T t8 __attribute__((ext_vector_type(8)));
    const t8 lo = *reinterpret_cast<const t8 *>(image + row * kB + sub * 16);
    const t8 hi = *reinterpret_cast<const t8 *>(image + row * kB + sub * 16 + 8);
    float v[16];
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      v[i] = (float)(i < 8 ? lo[i] : hi[i - 8]);
      if (fp8_finite(v[i])) amax = fmaxf(amax, fabsf(v[i]));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    const float scale = mx_scale<false>(amax);
    const uint32_t byte = mx_scale_byte(scale);
    const int lane0 = lane & ~7;
    const uint32_t dword = (uint32_t)__shfl((int)byte, lane0) |
                           (uint32_t)__shfl((int)byte, lane0 + 2) << 8 |
                           (uint32_t)__shfl((int)byte, lane0 + 4) << 16 |
                           (uint32_t)__shfl((int)byte, lane0 + 6) << 24;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
      w[i >> 2] |= fp8_quantize(v[i], scale) << (8 * (i & 3));
    *reinterpret_cast<uint4 *>(hq + row * kB + sub * 16) =
        make_uint4(w[0], w[1], w[2], w[3]);
    if (sub == 0) *reinterpret_cast<uint32_t *>(h_scales + row * 4) = dword;
  }
}

}  // namespace

hipError_t LaunchMxGated(bool b4, int dtype, const void *a,
                         const uint8_t *a_scales, const void *gate,
                         const uint8_t *gate_scales, const void *up,
                         const uint8_t *up_scales, int b_row_step,
                         const void *gate_bias, const void *up_bias,
                         bool clamped, int act, float alpha, float limit,
                         void *hq, uint8_t *h_scales, void *g_out, void *u_out,
                         void *h_out, const short *indices,
                         const short *row_indices, int m_blocks, int n_blocks,
                         int k_blocks, int nnz_blocks, hipStream_t stream) {
  if (nnz_blocks == 0) return hipSuccess;
  const MxGatedParams p{static_cast<const char *>(a), a_scales,
                        static_cast<const char *>(gate),
                        static_cast<const char *>(up), gate_scales, up_scales,
                        gate_bias, up_bias, static_cast<uint8_t *>(hq),
                        h_scales, g_out, u_out, h_out, indices, row_indices,
                        m_blocks, n_blocks, k_blocks, b_row_step, clamped, act,
                        alpha, limit};
  auto launch = [&](auto t, auto f) {
    hipLaunchKernelGGL((mx_gated_kernel<decltype(t), decltype(f)::value>),
                       dim3((unsigned)nnz_blocks), dim3(kThreads), 0, stream,
                       p);
    return hipGetLastError();
  };
  auto kind = [&](auto t) {
    return b4 ? launch(t, std::true_type{}) : launch(t, std::false_type{});
  };
  return dtype == 1 ? kind(__bf16{}) : kind(_Float16{});
}

}  // namespace sputnik_amd
