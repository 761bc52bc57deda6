// sputnik-amd: what the low-precision block GEMMs (fp8_gemm.hip, mx_gemm.hip,
// mx_gated_gemm.hip, mx4_gemm.hip) share: one 256-thread workgroup (2 x 2
// waves, 64 x 64 each) per 128 x 128 output tile, operands staged by LDS-DMA
// into a ring of stages, the tile leaving through LDS as 16-byte row pieces.
// Internal. Here: the tile constants, the vector types, the address-space
// casts of the DMA, the scalar-cache loads, the swizzle keys and the pitch of
// the sink image. Each file keeps its Params struct, its stage layout, its
// tile walk, ring and epilogue: written as shared function templates these
// compile to other code (profiles/lowp_refactor/README.md).
//
// The swizzle. The DMA's LDS image is lane-linear, so the swizzle sits on the
// source address: the lane that lands on 16-byte slot p of row r fetches chunk
// p ^ key(r) of that row. Every lane of a 16-lane group of a fragment read
// takes the same chunk c of rows r = 0 .. 15. With 128-byte rows two rows
// share a 256-byte bank row, the group's slots are (r & 1, c ^ key8(r)), and
// with key8(r) = (r >> 1) & 7 the pairs (r & 1, r >> 1) are 16 different ones:
// 16 slots once each, for any c, conflict-free. A 64-byte row (an e2m1 tile)
// has 4 chunks and four rows share a bank row: slot (r & 3, c ^ key4(r)),
// key4(r) = (r >> 2) & 3, again 16 different pairs.
#ifndef SPUTNIK_AMD_CSRC_LOWP_TILE_H_
#define SPUTNIK_AMD_CSRC_LOWP_TILE_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sputnik_amd {
namespace lowp {

constexpr int kThreads = 256;
constexpr int kB = 128;  // block edge = one step of k

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SPUTNIK_LOWP_LDS(p) ((__attribute__((address_space(3))) void *)(p))
#define SPUTNIK_LOWP_GLOBAL(p) \
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

__device__ __forceinline__ int key8(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int key4(int row) { return (row >> 2) & 3; }

// The fp32 image of a gradient sink's epilogue (the kWgrad DSDs of
// fp8_gemm.hip and mx_gemm.hip): the sink may hold fp32 and may be
// added into, and round_out(acc + float(C_old)) needs the unrounded acc next
// to C_old, so the tile leaves the registers as an fp32 image. 128 rows of
// 512 bytes are 64 KiB; a 66 KiB ring leaves exactly 16 bytes of padding per
// row (pitch 132 dwords). A wave's store of acc[ti][tj][e] puts lane (r, g) at
// row 4 g + e, column r of a 16 x 16 tile: dword 132 (4 g) + r, bank (16 g + r)
// % 64: 64 lanes, 64 banks, once each (in halves of 32 lanes on a 32-bank view:
// banks r and 16 + r). Without the padding the four lane groups would meet on
// one bank. The image then leaves as 16-byte pieces of the output type: a lane
// reads 16 (fp32: 4 x f32) or 32 (T: 8 x f32 -> 8 x T) consecutive bytes of an
// image row, consecutive lanes consecutive pieces, so both the LDS reads and
// the global accesses of C and C_old are row-contiguous.
constexpr int kImagePitch = kB + 4;

}  // namespace lowp
}  // namespace sputnik_amd

#endif  // SPUTNIK_AMD_CSRC_LOWP_TILE_H_
