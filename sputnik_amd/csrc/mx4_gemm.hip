// sputnik-amd: the A4W4 block GEMM of sputnik/block/mx.h ("MXFP4
// activations"): e2m1 rows against e2m1 weight rows, every 32 k-elements under
// an e8m0 scale that the matrix instruction applies. One kernel template, two
// tile sources (SDD and DSD). Both operands arrive k-contiguous, two codes per
// byte, low nibble first.
//
// With both operands e2m1 the MFMA of a k-block takes half the passes of any
// form with an fp8 operand, so what a step costs besides its MFMAs (the wait,
// the barrier, the address arithmetic of the DMA) weighs twice as much as in
// mx_gemm.hip. A k-block of an e2m1 operand is also only 64 bytes of a row. So
// a stage of the ring holds two k-blocks and the loop pays its fixed cost once
// per 256 k-elements:
//
//   A image    128 rows x 128 bytes: k-block 2 i in chunks 0 - 3 of a row,
//              k-block 2 i + 1 in chunks 4 - 7                     16 KiB
//   B image    the same shape, rows = output columns                16 KiB
//   A scales   two dwords per row, [half][row]: the row's four e8m0 bytes of
//              k-block 2 i, then of 2 i + 1                          1 KiB
//   B scales   two dwords per column, likewise                       1 KiB
//
// 34 KiB a stage, two stages 68 KiB: two workgroups per CU (160 KiB).
//
//   staging  16-byte LDS-DMA (global_load_lds) for the images, 4-byte for the
//            scale dwords. The DMA's LDS image is lane-linear, so the swizzle
//            sits on the source address, as mx_gemm.hip derives it for
//            128-byte rows: the lane that lands on slot p of row r fetches
//            chunk p ^ key(r), key(r) = (r >> 1) & 7. SDD: chunk c of a row
//            is byte 16 c of the row's 128 contiguous bytes of the stage. DSD:
//            the two halves come from two stored blocks ([128][64] bytes
//            each) and from the two k-blocks of B their indices name; a half
//            has its own base and chunk c is byte 16 (c & 3) of half c >> 2.
//   reads    lane l (r = l % 16, g = l / 16) of a 16-row fragment takes chunk
//            g of row r for the first MFMA of the stage (k = 32 g .. 32 g + 31
//            of k-block 2 i, registers 0 - 3) and chunk g + 4 for the second:
//            the two ds_read_b128 patterns mx_gemm.hip shows to be
//            conflict-free (16 lanes of a group, one chunk c, slots (r & 1,
//            c ^ key(r)): 16 different ones).
//   scales   lane group g supplies byte g of the half's dword of its row
//            (column), shifted into byte 0.
//   MFMA     per stage and 16 x 16 tile two
//            v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz 4, blgp 4), each from a
//            +0 accumulator, and two fp32 adds in k order.
//   output   round_T(acc) once, through LDS (the image reuses the ring), as
//            16-byte row pieces.
//
// Half stages. A half of a stage is absent when the step count is odd (the
// last stage has only k-block 2 i) or, DSD, when its stored block's index is
// out of range. An absent half is neither fetched nor consumed. Which halves
// a stage has is wave-uniform; the DMA keeps every lane busy either way: a
// lane whose slot belongs to the absent half fetches the same chunk of the
// present half instead (an address inside the operands, bytes nobody reads),
// so no lane-divergent DMA and no read past a row's end. A stage without
// either half issues nothing. steps == 0 writes +0 rows.
//
// The step order is the k order (SDD) or the row's storage order (DSD), no
// split-K and no atomics: the same inputs give the same bits, and SDD on a
// full topology and DSD over the same bytes give the same bits. Every index
// read from device memory is checked before it is used as an address.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "api_internal.h"
#include "lowp_tile.h"

namespace sputnik_amd {
namespace {

// kThreads, kB (the block edge = one k-block), the vector types, the
// scalar loads and the swizzle keys: lowp_tile.h.
using namespace lowp;

constexpr int kHalfRow = kB / 2;      // bytes of a k-block in an e2m1 row
constexpr int kImageBytes = kB * kB;  // 128 rows x two k-blocks of 64 bytes
constexpr int kScaleBytes = kB * 2 * 4;  // two dwords per row (column)
constexpr int kBOff = kImageBytes;
constexpr int kAScaleOff = 2 * kImageBytes;
constexpr int kBScaleOff = kAScaleOff + kScaleBytes;
constexpr int kStageBytes = kBScaleOff + kScaleBytes;
constexpr int kStages = 2;
constexpr int kLdsBytes = kStages * kStageBytes;
static_assert(kStageBytes == 34 * 1024, "the stage size of the header");
static_assert(2 * kLdsBytes <= 160 * 1024, "two workgroups per CU");
static_assert(kB * kB * 2 <= kLdsBytes, "the output tile reuses the ring");

struct Mx4GemmParams {
  const char *a;            // SDD: Aq [m, k / 2]; DSD: the stored blocks of Sq
  const uint8_t *a_scales;  // SDD: [m, k / 32]; DSD: [nnz_blocks * 128, 4]
  const char *b;            // Bq [n, k / 2]
  const uint8_t *b_scales;  // [n, k / 32]
  void *c;                  // SDD: block values of C; DSD: C [m, n]
  const int *offsets;       // DSD: the sparse operand's row offsets
  const short *indices;     // SDD: C's column indices; DSD: Sq's
  const short *row_indices;  // SDD: C's
  int m_blocks, n_blocks, k_blocks, nnz_blocks;
};

// The sources of one half of a stage: row 0 of the tile, this k-block.
struct Mx4Half {
  const char *a, *b;
  const uint8_t *a_scale, *b_scale;
};

template <typename T, bool kDsd>
__global__ void __launch_bounds__(kThreads)
    mx4_gemm_kernel(const Mx4GemmParams p) {
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytes];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long row_bytes = (long long)p.k_blocks * kHalfRow;  // of Aq, Bq
  const long long scale_row = (long long)p.k_blocks * 4;

  // The output tile and its steps (k-blocks).
  int rb, nb, first = 0, steps;
  if constexpr (kDsd) {
    rb = blockIdx.x / p.n_blocks;
    nb = blockIdx.x % p.n_blocks;
    int begin = scalar_int(p.offsets + rb), end = scalar_int(p.offsets + rb + 1);
    begin = begin < 0 ? 0 : begin;
    end = end > p.nnz_blocks ? p.nnz_blocks : end;
    first = begin;
    steps = end > begin ? end - begin : 0;
  } else {
    rb = scalar_short(p.row_indices + blockIdx.x);
    nb = scalar_short(p.indices + blockIdx.x);
    if (rb < 0 || rb >= p.m_blocks || nb < 0 || nb >= p.n_blocks) return;
    steps = p.k_blocks;
  }
  const int stages = (steps + 1) / 2;
  // The k-block of step s, or -1 for a step past the end or a stored block to
  // skip.
  auto k_block = [&](int s) {
    if (s >= steps) return -1;
    if constexpr (!kDsd) return s;
    const int kb = scalar_short(p.indices + first + s);
    return kb >= 0 && kb < p.k_blocks ? kb : -1;
  };
  // A's tile rows lie `a_pitch` bytes apart, its scale dwords `a_scale_pitch`.
  const long long a_pitch = kDsd ? kHalfRow : row_bytes;
  const long long a_scale_pitch = kDsd ? 4 : scale_row;
  auto half_of = [&](int s, int kb) {
    Mx4Half h;
    if constexpr (kDsd) {
      const long long at = first + s;
      h.a = p.a + at * (kB * kHalfRow);
      h.a_scale = p.a_scales + at * kB * 4;
    } else {
      h.a = p.a + (long long)rb * kB * row_bytes + (long long)kb * kHalfRow;
      h.a_scale = p.a_scales + (long long)rb * kB * scale_row + kb * 4;
    }
    h.b = p.b + (long long)nb * kB * row_bytes + (long long)kb * kHalfRow;
    h.b_scale = p.b_scales + (long long)nb * kB * scale_row + kb * 4;
    return h;
  };

  // One stage's DMA into `stage`: steps 2 i and 2 i + 1.
  auto issue = [&](int i, char *stage) {
    const int kb0 = k_block(2 * i), kb1 = k_block(2 * i + 1);
    if (kb0 < 0 && kb1 < 0) return;
    // (an absent half borrows the present one's sources: its lanes stay busy
    // on addresses inside the operands, and nobody reads what they bring)
    const Mx4Half h0 = kb0 >= 0 ? half_of(2 * i, kb0) : half_of(2 * i + 1, kb1);
    const Mx4Half h1 = kb1 >= 0 ? half_of(2 * i + 1, kb1) : h0;
#pragma unroll
    for (int pass = 0; pass < kImageBytes / (kThreads * 16); ++pass) {
      // (a wave's 64 x 16 bytes are 8 rows of the image)
      const int piece = pass * (kThreads * 16) + wave * 1024;
      const int row = (piece >> 7) + (lane >> 3);
      const int chunk = (lane & 7) ^ key8(row);
      const bool second = chunk >= 4;
      const int at = (chunk & 3) * 16;
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL((second ? h1.a : h0.a) + row * a_pitch + at),
          SPUTNIK_LOWP_LDS(stage + piece), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL((second ? h1.b : h0.b) + row * row_bytes + at),
          SPUTNIK_LOWP_LDS(stage + kBOff + piece), 16, 0, 0);
    }
    // Scale dwords, [half][row]: waves 0, 1 the first half's, 2, 3 the
    // second's; an absent half's are not fetched.
    if ((wave < 2 ? kb0 : kb1) >= 0) {
      const Mx4Half &h = wave < 2 ? h0 : h1;
      const int row = (wave & 1) * 64 + lane;
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL(h.a_scale + row * a_scale_pitch),
          SPUTNIK_LOWP_LDS(stage + kAScaleOff + wave * 256), 4, 0, 0);
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL(h.b_scale + row * scale_row),
          SPUTNIK_LOWP_LDS(stage + kBScaleOff + wave * 256), 4, 0, 0);
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 15, g = lane >> 4;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // The lane's 32 k-elements of row row0 + r in half `half` of the stage:
  // chunk g + 4 half, 16 bytes of pairs for registers 0 - 3.
  auto fragment = [&](const char *image, int row0, int half) {
    const int row = row0 + r;
    const i32x4 v = *reinterpret_cast<const i32x4 *>(
        image + row * kB + (((g + 4 * half) ^ key8(row)) << 4));
    return i32x8{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
  };

  auto compute = [&](int i, const char *stage) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (k_block(2 * i + half) < 0) continue;
      const int *sa_lds =
          reinterpret_cast<const int *>(stage + kAScaleOff) + half * kB;
      const int *sb_lds =
          reinterpret_cast<const int *>(stage + kBScaleOff) + half * kB;
      i32x8 a[4];
      int sa[4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        a[ti] = fragment(stage, wm * 64 + ti * 16, half);
        sa[ti] = (unsigned)sa_lds[wm * 64 + ti * 16 + r] >> (8 * g);
      }
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) {
        const i32x8 b = fragment(stage + kBOff, wn * 64 + tj * 16, half);
        const int sb = (unsigned)sb_lds[wn * 64 + tj * 16 + r] >> (8 * g);
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
          // (cbsz 4, blgp 4: both e2m1; opsel 0: scale byte 0)
          const f32x4 sum = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              a[ti], b, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 4, 4, 0, sa[ti], 0, sb);
          acc[ti][tj] += sum;
        }
      }
    }
  };

  // Stage i + 1 lands while stage i is consumed: the barrier that follows
  // the wait also says every wave is done with the stage about to be
  // refilled.
  if (stages > 0) issue(0, lds);
  for (int i = 0; i < stages; ++i) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (i + 1 < stages) issue(i + 1, lds + ((i + 1) % kStages) * kStageBytes);
    compute(i, lds + (i % kStages) * kStageBytes);
  }

  // round_T(acc) into a [128][128] image of T, then 16-byte row pieces.
  __syncthreads();
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

}  // namespace

hipError_t LaunchMx4Gemm(bool dsd, int dtype, const void *a,
                         const uint8_t *a_scales, const void *b,
                         const uint8_t *b_scales, void *c, const int *offsets,
                         const short *indices, const short *row_indices,
                         int m_blocks, int n_blocks, int k_blocks,
                         int nnz_blocks, hipStream_t stream) {
  const long long tiles =
      dsd ? (long long)m_blocks * n_blocks : (long long)nnz_blocks;
  if (tiles == 0) return hipSuccess;
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  const Mx4GemmParams p{static_cast<const char *>(a), a_scales,
                        static_cast<const char *>(b), b_scales, c, offsets,
                        indices, row_indices, m_blocks, n_blocks, k_blocks,
                        nnz_blocks};
  auto launch = [&](auto t, auto d) {
    hipLaunchKernelGGL((mx4_gemm_kernel<decltype(t), decltype(d)::value>),
                       dim3((unsigned)tiles), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
  };
  if (dsd)
    return dtype == 1 ? launch(__bf16{}, std::true_type{})
                      : launch(_Float16{}, std::true_type{});
  return dtype == 1 ? launch(__bf16{}, std::false_type{})
                    : launch(_Float16{}, std::false_type{});
}

}  // namespace sputnik_amd
