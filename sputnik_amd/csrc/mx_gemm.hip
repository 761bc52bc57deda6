// sputnik-amd: the MX block GEMM of sputnik/block/mx.h: e4m3 rows against
// e4m3 or e2m1 weight rows, every 32 k-elements under an e8m0 scale that the
// matrix instruction applies. One kernel template, two tile sources (SDD and
// DSD), two B element types. Both operands arrive k-contiguous.
//
// One 256-thread workgroup (2 x 2 waves, 64 x 64 each) per 128 x 128 output
// tile. A step is one k-block of 128. A stage of the ring holds
//
//   A tile     128 rows x 128 bytes                        16 KiB
//   B tile     128 rows x 128 bytes (e4m3) or 64 (e2m1)    16 / 8 KiB
//   A scales   one dword per row: the row's four e8m0 bytes of the step
//   B scales   one dword per column, likewise              512 B each
//
//   staging  16-byte LDS-DMA (global_load_lds) for the tiles, 4-byte for the
//            scale dwords (waves 0, 1: rows; waves 2, 3: columns), so the loop
//            has no register-destination load. The DMA's LDS image is
//            lane-linear, so the swizzle sits on the source address
//            (lowp_tile.h has the keys and why the reads below are
//            conflict-free).
//   reads    lane l (r = l % 16, g = l / 16) of a 16-row fragment. The k map
//            of the instruction, measured (mx.h): an e4m3 operand wants k =
//            16 g .. 16 g + 15 in registers 0 - 3 and k = 64 + 16 g .. 64 +
//            16 g + 15 in registers 4 - 7, so the lane takes chunks g and
//            g + 4 of row r by two ds_read_b128 (not the 32 contiguous bytes
//            at 32 g: the scale of 32-block b still comes from lane group b,
//            so that reading multiplies half of every block by a
//            neighbour's scale); an e2m1 operand wants k = 32 g .. 32 g + 31,
//            low nibble first: the 16 bytes of chunk g by one read. Every
//            lane of a 16-lane group reads the same chunk c, so the group's
//            slots are (r & 1, c ^ key(r)) in the 256-byte bank row two
//            128-byte rows share: with key(r) = (r >> 1) & 7 the pairs (r &
//            1, r >> 1) are 16 different ones, 16 slots once each, for any
//            c: groups g = 0 .. 3 read chunks {0, 1, 2, 3} then {4, 5, 6, 7},
//            conflict-free each. A 64-byte e2m1 row has 4 chunks and four
//            rows share a bank row: slot (r & 3, c ^ key4(r)), key4(r) = (r >>
//            2) & 3, again 16 different pairs for r = 0 .. 15 and any c.
//   scales   lane group g supplies the e8m0 byte of 32-block g of its row
//            (column), for both element types: byte g of the row's dword,
//            shifted into byte 0 (op_sel is an immediate).
//   MFMA     one v_mfma_scale_f32_16x16x128_f8f6f4 per 16 x 16 tile and step
//            from a +0 accumulator (cbsz 0; blgp 0 or 4), then one fp32 add.
//   output   round_T(acc) once, through LDS, as 16-byte row pieces.
//
// Ring: two stages for both element types. e4m3 stages are 33 KiB (66 KiB: a
// third would cost the second workgroup of a CU's 160 KiB); e2m1 stages are
// 25 KiB (50 KiB), and a third stage buys them nothing: the barrier of a step
// waits for every DMA in flight, so no more than one step can run ahead.
//
// The step order is the k order (SDD) or the row's storage order (DSD), no
// split-K and no atomics: the same inputs give the same bits. Every index
// read from device memory is checked before it is used as an address.
//
// kWgrad (DsdMxWgrad) is the e4m3 DSD with a gradient sink for an output. MX
// scales belong to one operand and run along k, so the steps, the k map and
// the adds are the DSD's, untouched: only the epilogue differs. The sink may
// hold fp32 and may be added into, and round_out(acc + float(C_old)) needs
// the unrounded acc next to C_old, so the tile leaves the registers as an
// fp32 image at pitch kImagePitch (lowp_tile.h has the bank argument) and
// then as 16-byte pieces of the output type, so the global accesses of C and
// C_old are row-contiguous. A block row without stored blocks is left alone
// under `add` (neither read nor written) and is +0 otherwise. The kWgrad =
// false instantiations keep their code.
//
// kPair (DsdMxPair) is the e4m3 DSD over two operand pairs that share one
// topology, C = S1 B1 + S2 B2 through one accumulator: the step count doubles,
// steps [0, blocks) walk the block row with the first pair's pointers and
// steps [blocks, 2 blocks) walk it again with the second pair's, the indices
// coming through the scalar cache a second time. Which pair a step takes is
// wave-uniform and changes only the source addresses of issue(): the ring
// keeps alternating (i % 2, so with an odd block count the second pair starts
// in the other stage), compute() reads whatever stage i holds, and the +0
// MFMA and the one fp32 add per step are the DSD's. Bit for bit DsdMx over
// [S1 | S2] . [B1; B2], with no copy of either. The kPair = false
// instantiations compile to what they were.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "api_internal.h"
#include "lowp_tile.h"

namespace sputnik_amd {
namespace {

// kThreads, kB (the block edge = one step of k), the vector types, the
// scalar loads and the swizzle keys: lowp_tile.h.
using namespace lowp;

constexpr int kATileBytes = kB * kB;
constexpr int BTileBytes(bool b4) { return b4 ? kB * kB / 2 : kB * kB; }
constexpr int kScaleBytes = kB * 4;      // one dword per row (column)
constexpr int StageBytes(bool b4) {
  return kATileBytes + BTileBytes(b4) + 2 * kScaleBytes;
}
constexpr int kStages = 2;
constexpr int LdsBytes(bool b4) { return kStages * StageBytes(b4); }
static_assert(StageBytes(false) == 33 * 1024 && StageBytes(true) == 25 * 1024,
              "the stage sizes of the header");
static_assert(2 * LdsBytes(false) <= 160 * 1024 &&
                  2 * LdsBytes(true) <= 160 * 1024,
              "two workgroups per CU");
static_assert(3 * StageBytes(false) * 2 > 160 * 1024,
              "a third e4m3 stage would cost the second workgroup");
static_assert(kB * kB * 2 <= LdsBytes(false) && kB * kB * 2 <= LdsBytes(true),
              "the output tile reuses the ring");
static_assert(kB * kImagePitch * 4 <= LdsBytes(false),
              "the fp32 image of the wgrad reuses the e4m3 ring");

struct MxGemmParams {
  const char *a;            // SDD: Aq [m, k]; DSD: the stored blocks of Sq
  const uint8_t *a_scales;  // SDD: [m, k / 32]; DSD: [nnz_blocks * 128, 4]
  const char *b;            // Bq [n, k] or, e2m1, [n, k / 2]
  const uint8_t *b_scales;  // [n, k / 32]
  void *c;                  // SDD: block values of C; DSD: C [m, n]
  const int *offsets;       // DSD: the sparse operand's row offsets
  const short *indices;     // SDD: C's column indices; DSD: Sq's
  const short *row_indices;  // SDD: C's
  int m_blocks, n_blocks, k_blocks, nnz_blocks;
  int out_f32, add;  // kWgrad: C holds fp32; C += (accumulate.h)
  // kPair: the second pair's blocks, row scales, Bq and its scales
  const char *a2;
  const uint8_t *a2_scales;
  const char *b2;
  const uint8_t *b2_scales;
};

template <typename T, bool kDsd, bool kB4, bool kWgrad = false,
          bool kPair = false>
__global__ void __launch_bounds__(kThreads)
    mx_gemm_kernel(const MxGemmParams p) {
  static_assert(!kWgrad || (kDsd && !kB4), "the wgrad is the e4m3 DSD");
  static_assert(!kPair || (kDsd && !kB4 && !kWgrad),
                "the paired product is the e4m3 DSD");
  constexpr int kStageBytes = StageBytes(kB4);
  constexpr int kBOff = kATileBytes;
  constexpr int kScaleOff = kATileBytes + BTileBytes(kB4);
  constexpr int kBRow = kB4 ? kB / 2 : kB;  // bytes of a B row in a tile
  __shared__ __attribute__((aligned(16))) char lds[LdsBytes(kB4)];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long k_bytes = (long long)p.k_blocks * kB;
  const long long b_pitch = kB4 ? k_bytes / 2 : k_bytes;

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
    if constexpr (kWgrad) if (p.add && steps == 0) return;
  } else {
    rb = scalar_short(p.row_indices + blockIdx.x);
    nb = scalar_short(p.indices + blockIdx.x);
    if (rb < 0 || rb >= p.m_blocks || nb < 0 || nb >= p.n_blocks) return;
    steps = p.k_blocks;
  }
  // kPair: step i takes stored block i - blocks of the second pair once i
  // has passed the row's blocks.
  [[maybe_unused]] const int blocks = steps;
  if constexpr (kPair) steps *= 2;
  auto second = [&](int i) {
    if constexpr (kPair) return i >= blocks;
    return false;
  };
  auto stored = [&](int i) {
    if constexpr (kPair) return i >= blocks ? i - blocks : i;
    return i;
  };
  // The k-block of step i, or -1 for a stored block to skip.
  auto k_block = [&](int i) {
    if constexpr (!kDsd) return i;
    const int kb = scalar_short(p.indices + first + stored(i));
    return kb >= 0 && kb < p.k_blocks ? kb : -1;
  };

  // One step's DMA into `stage`.
  auto issue = [&](int i, char *stage) {
    const int kb = k_block(i);
    if (kb < 0) return;
    const char *a_tile;
    long long a_pitch;
    const uint8_t *a_scale;   // of row 0 of the tile, this step's dword
    long long a_scale_pitch;  // bytes between rows
    if constexpr (kDsd) {
      const long long at = first + stored(i);
      a_tile = (second(i) ? p.a2 : p.a) + at * kATileBytes;
      a_pitch = kB;
      a_scale = (second(i) ? p.a2_scales : p.a_scales) + at * kB * 4;
      a_scale_pitch = 4;
    } else {
      a_tile = p.a + (long long)rb * kB * k_bytes + (long long)kb * kB;
      a_pitch = k_bytes;
      a_scale_pitch = (long long)p.k_blocks * 4;
      a_scale = p.a_scales + (long long)rb * kB * a_scale_pitch + kb * 4;
    }
    const char *b_tile = (second(i) ? p.b2 : p.b) +
                         (long long)nb * kB * b_pitch + (long long)kb * kBRow;
    const uint8_t *b_scales = second(i) ? p.b2_scales : p.b_scales;
#pragma unroll
    for (int pass = 0; pass < kATileBytes / (kThreads * 16); ++pass) {
      // (a wave's 64 x 16 bytes are 8 rows of the image)
      const int piece = pass * (kThreads * 16) + wave * 1024;
      const int row = (piece >> 7) + (lane >> 3);
      const int chunk = (lane & 7) ^ key8(row);
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL(a_tile + row * a_pitch + chunk * 16),
          SPUTNIK_LOWP_LDS(stage + piece), 16, 0, 0);
    }
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
          SPUTNIK_LOWP_LDS(stage + kBOff + piece), 16, 0, 0);
    }
    if (wave < kB / 64) {
      const int row = wave * 64 + lane;
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL(a_scale + row * a_scale_pitch),
          SPUTNIK_LOWP_LDS(stage + kScaleOff + wave * 256), 4, 0, 0);
    } else {
      const int col = (wave - kB / 64) * 64 + lane;
      __builtin_amdgcn_global_load_lds(
          SPUTNIK_LOWP_GLOBAL(b_scales +
                            ((long long)(nb * kB + col) * p.k_blocks + kb) * 4),
          SPUTNIK_LOWP_LDS(stage + kScaleOff + wave * 256), 4, 0, 0);
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 15, g = lane >> 4;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // The lane's 32 k-elements of row row0 + r, where the instruction wants
  // them: e4m3, k = 16 g .. 16 g + 15 in registers 0 - 3 and k = 64 + 16 g ..
  // in registers 4 - 7 (chunks g and g + 4); e2m1, k = 32 g .. 32 g + 31 as 16
  // bytes of pairs in registers 0 - 3 (chunk g).
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

  auto compute = [&](int i, const char *stage) {
    if (k_block(i) < 0) return;
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
      i32x8 b;
      if constexpr (kB4) b = fragment4(stage + kBOff, wn * 64 + tj * 16);
      else b = fragment8(stage + kBOff, wn * 64 + tj * 16);
      const int sb = (unsigned)scale_lds[kB + wn * 64 + tj * 16 + r] >> (8 * g);
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        // (cbsz 0: A is e4m3; blgp 0 / 4: B is e4m3 / e2m1; opsel 0: byte 0)
        const f32x4 sum = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            a[ti], b, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, kB4 ? 4 : 0, 0, sa[ti],
            0, sb);
        acc[ti][tj] += sum;
      }
    }
  };

  // Stage i + 1 lands while stage i is consumed: the barrier that follows
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
        f32x4 v =
            *reinterpret_cast<const f32x4 *>(image + row * kImagePitch + col);
        f32x4 *dst = reinterpret_cast<f32x4 *>(out + row * n + col);
        if (p.add) v += *dst;
        *dst = v;
      }
    } else {
      typedef T t8 __attribute__((ext_vector_type(8)));
      T *out = static_cast<T *>(p.c) + at;
      for (int id = threadIdx.x; id < kB * kB / 8; id += kThreads) {
        const int row = id >> 4, col = (id & 15) * 8;
        const float *from = image + row * kImagePitch + col;
        const f32x4 lo = *reinterpret_cast<const f32x4 *>(from);
        const f32x4 hi = *reinterpret_cast<const f32x4 *>(from + 4);
        t8 *dst = reinterpret_cast<t8 *>(out + row * n + col);
        t8 old{}, res;
        if (p.add) old = *dst;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float v = i < 4 ? lo[i] : hi[i - 4];
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

}  // namespace

hipError_t LaunchMxGemm(bool dsd, bool b4, int dtype, const void *a,
                        const uint8_t *a_scales, const void *b,
                        const uint8_t *b_scales, void *c, const int *offsets,
                        const short *indices, const short *row_indices,
                        int m_blocks, int n_blocks, int k_blocks,
                        int nnz_blocks, hipStream_t stream) {
  const long long tiles =
      dsd ? (long long)m_blocks * n_blocks : (long long)nnz_blocks;
  if (tiles == 0) return hipSuccess;
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  const MxGemmParams p{static_cast<const char *>(a), a_scales,
                       static_cast<const char *>(b), b_scales, c, offsets,
                       indices, row_indices, m_blocks, n_blocks, k_blocks,
                       nnz_blocks, 0, 0, nullptr, nullptr, nullptr, nullptr};
  auto launch = [&](auto t, auto d, auto f) {
    hipLaunchKernelGGL((mx_gemm_kernel<decltype(t), decltype(d)::value,
                                       decltype(f)::value>),
                       dim3((unsigned)tiles), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
  };
  auto kind = [&](auto t, auto d) {
    return b4 ? launch(t, d, std::true_type{})
              : launch(t, d, std::false_type{});
  };
  if (dsd)
    return dtype == 1 ? kind(__bf16{}, std::true_type{})
                      : kind(_Float16{}, std::true_type{});
  return dtype == 1 ? kind(__bf16{}, std::false_type{})
                    : kind(_Float16{}, std::false_type{});
}

hipError_t LaunchMxWgrad(int dtype, bool out_f32, bool add, const void *a,
                         const uint8_t *a_scales, const void *b,
                         const uint8_t *b_scales, void *c, const int *offsets,
                         const short *indices, int m_blocks, int n_blocks,
                         int k_blocks, int nnz_blocks, hipStream_t stream) {
  const long long tiles = (long long)m_blocks * n_blocks;
  if (tiles == 0) return hipSuccess;
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  const MxGemmParams p{static_cast<const char *>(a), a_scales,
                       static_cast<const char *>(b), b_scales, c, offsets,
                       indices, nullptr, m_blocks, n_blocks, k_blocks,
                       nnz_blocks, out_f32, add, nullptr, nullptr, nullptr,
                       nullptr};
  auto launch = [&](auto t) {
    hipLaunchKernelGGL((mx_gemm_kernel<decltype(t), true, false, true>),
                       dim3((unsigned)tiles), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
  };
  return dtype == 1 ? launch(__bf16{}) : launch(_Float16{});
}

hipError_t LaunchMxPair(int dtype, const void *s1, const uint8_t *s1_scales,
                        const void *b1, const uint8_t *b1_scales,
                        const void *s2, const uint8_t *s2_scales,
                        const void *b2, const uint8_t *b2_scales, void *c,
                        const int *offsets, const short *indices, int m_blocks,
                        int n_blocks, int k_blocks, int nnz_blocks,
                        hipStream_t stream) {
  const long long tiles = (long long)m_blocks * n_blocks;
  if (tiles == 0) return hipSuccess;
  if (tiles > INT_MAX) return hipErrorInvalidValue;
  const MxGemmParams p{static_cast<const char *>(s1), s1_scales,
                       static_cast<const char *>(b1), b1_scales, c, offsets,
                       indices, nullptr, m_blocks, n_blocks, k_blocks,
                       nnz_blocks, 0, 0, static_cast<const char *>(s2),
                       s2_scales, static_cast<const char *>(b2), b2_scales};
  auto launch = [&](auto t) {
    hipLaunchKernelGGL((mx_gemm_kernel<decltype(t), true, false, false, true>),
                       dim3((unsigned)tiles), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
  };
  return dtype == 1 ? launch(__bf16{}) : launch(_Float16{});
}

}  // namespace sputnik_amd
