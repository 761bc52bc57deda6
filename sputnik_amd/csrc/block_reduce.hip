// sputnik-amd: column sums of a block-sparse matrix (sputnik/block/bias.h
// BlockColumnSum), the bias gradient of a sparse dZ:
//
//   out[c] = sum_r float(S[r, c])   over S's stored blocks, fp32 [S.cols]
//
// One workgroup per column block. It walks the column through the transposed
// metadata (entries offsets_t[cb] .. offsets_t[cb + 1], storage block
// block_offsets[entry]). A block row is 256 bytes, 16 lanes of 16 bytes, so
// the workgroup's 1024 threads cover 64 rows per step: thread (g, l) takes
// rows g and g + 64 of every block and columns 8 l .. 8 l + 7, two blocks in
// flight, and adds them in entry order. The 64 partial sums of a column are
// then added through LDS in g order by one thread. No atomics, no workspace:
// the order is a function of the topology alone. Every entry read from device
// memory is range-checked before it forms an address; an entry out of range
// is skipped, a column block without entries gives +0.
#include <hip/hip_runtime.h>

#include "api_internal.h"
#include "sputnik/block/bias.h"

namespace sputnik_amd {
namespace {

constexpr int kThreads = 1024;
constexpr int kRowGroups = kThreads / 16;  // 64
constexpr int kBlockDim = 128;

template <typename T>
__global__ void __launch_bounds__(kThreads)
    block_column_sum_kernel(const T *__restrict__ data,
                            const int *__restrict__ offsets_t,
                            const int *__restrict__ block_offsets,
                            float *__restrict__ out, int num_blocks) {
#pragma clang fp contract(off)
  typedef T t8 __attribute__((ext_vector_type(8)));
  __shared__ float part[kRowGroups][kBlockDim];
  const int cb = blockIdx.x;
  const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
  int e0 = offsets_t[cb], e1 = offsets_t[cb + 1];
  e0 = min(max(e0, 0), num_blocks);
  e1 = min(max(e1, e0), num_blocks);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
  // This thread's two chunks of storage block blk (zeros: blk out of range).
  auto load = [&](int e, t8 *v) {
    const int blk = e < e1 ? block_offsets[e] : -1;
    const bool ok = blk >= 0 && blk < num_blocks;
    const t8 *src = reinterpret_cast<const t8 *>(
        data + (long long)(ok ? blk : 0) * (kBlockDim * kBlockDim));
    v[0] = ok ? src[g * 16 + l] : t8{};
    v[1] = ok ? src[(g + kRowGroups) * 16 + l] : t8{};
  };
  for (int e = e0; e < e1; e += 2) {
    t8 v[4];
    load(e, v);
    load(e + 1, v + 2);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = acc[j] + (float)v[u][j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[g][l * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < kBlockDim) {
    float s = 0.0f;
#pragma unroll 8
    for (int r = 0; r < kRowGroups; ++r) s = s + part[r][threadIdx.x];
    out[(long long)cb * kBlockDim + threadIdx.x] = s + 0.0f;
  }
}

}  // namespace

hipError_t RunBlockColumnSum(const BlockMatrix &s, int dtype, float *out,
                             hipStream_t stream) {
  if ((dtype != 0 && dtype != 1) || s.cols < 0 || s.nonzeros < 0 ||
      s.cols % kBlockDim != 0 || s.nonzeros % (kBlockDim * kBlockDim) != 0 ||
      sputnik::block::AsInt(s.block_size) != kBlockDim)
    return hipErrorInvalidValue;
  if (s.cols == 0) return hipSuccess;
  if (out == nullptr || s.offsets_t == nullptr ||
      s.block_offsets == nullptr || (s.nonzeros > 0 && s.data == nullptr) ||
      out == s.data)
    return hipErrorInvalidValue;
  const int col_blocks = s.cols / kBlockDim;
  const int num_blocks = s.nonzeros / (kBlockDim * kBlockDim);
  const int *offsets_t = static_cast<const int *>(s.offsets_t);
  const int *block_offsets = static_cast<const int *>(s.block_offsets);
  if (dtype == 1)
    hipLaunchKernelGGL(block_column_sum_kernel<__bf16>, dim3(col_blocks),
                       dim3(kThreads), 0, stream,
                       static_cast<const __bf16 *>(s.data), offsets_t,
                       block_offsets, out, num_blocks);
  else
    hipLaunchKernelGGL(block_column_sum_kernel<_Float16>, dim3(col_blocks),
                       dim3(kThreads), 0, stream,
                       static_cast<const _Float16 *>(s.data), offsets_t,
                       block_offsets, out, num_blocks);
  return hipGetLastError();
}

}  // namespace sputnik_amd
