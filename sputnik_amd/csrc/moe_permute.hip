// sputnik-amd: MoE token permutation (sputnik/block/moe.h): the padded
// gather in front of the expert MLP, the weighted scatter behind it, the
// router-weight gradient, and the two metadata kernels that turn the sorted
// bin ids into bins / padded bins and the assignment -> padded row map.
//
// The three row movers are memory bound and share one shape. A task is
// kRowsInFlight consecutive destination rows and belongs to one wave; per
// step the wave issues one 16-byte load per lane for each of its rows (one
// contiguous 1 KiB piece per row) before any math or store, so a wave keeps
// kRowsInFlight pieces in flight whether rows are short or long. 4 waves per
// workgroup, the grid capped at 4 workgroups per CU (16 waves per CU), a
// grid-stride loop over the remaining tasks. Element offsets are long long
// (rows * hidden may pass 2^31). The vector path needs hidden % 8 == 0 and
// 16-byte aligned buffers (every row base is then aligned); anything else
// takes the same loop with one element per lane.
//
//   gather   driven by output rows: the expert of padded row r is the upper
//            bound of r in padded_bins (as expert_topology_kernel), its
//            sorted position bins[e-1] + (r - padded_bins[e-1]); padding rows
//            and rows past padded_bins[E-1] are written as +0 by the same
//            wave, so the output needs no memset.
//   scatter  driven by token: reads its top_k rows through row_of, sums in
//            fp32 from 0 in ascending k, rounds once. No atomics.
//   wgrad    one wave per assignment: a dot product of two rows, reduced by
//            shuffles.
//
// Every index read from device memory (indices[i], bins / padded_bins
// entries, row_of[a]) is range-checked before it forms an address; an entry
// out of range stands for a row of zeros.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

#include "moe_permute.h"
#include "sputnik/block/moe.h"

namespace sputnik_amd {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsInFlight = 4;
constexpr int kWorkgroupsPerCu = 4;
constexpr int kMetaThreads = 1024;

// #{e : v[e] <= key}, v ascending (any v terminates with a result in [0, n]).
__device__ __forceinline__ int upper_bound(const int *__restrict__ v, int n,
                                           int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The assignment stored in padded row r, or -1 for a row of zeros (padding,
// a row past the last bin, or metadata out of range).
__device__ __forceinline__ int row_assignment(
    int r, const int *__restrict__ indices, const int *__restrict__ bins,
    const int *__restrict__ padded_bins, int num_experts, int n) {
  const int e = upper_bound(padded_bins, num_experts, r);
  if (e >= num_experts) return -1;
  const int pad0 = e ? padded_bins[e - 1] : 0;
  const int bin0 = e ? bins[e - 1] : 0;
  if (pad0 < 0 || pad0 > r || bin0 < 0) return -1;
  const long long i = (long long)bin0 + (r - pad0);
  if (i >= n || i >= bins[e]) return -1;
  const int a = indices[i];
  return a >= 0 && a < n ? a : -1;
}

// One lane's piece of a row: 8 elements (16 bytes) or one.
template <typename T, bool kVec>
struct Piece {
  typedef T t8 __attribute__((ext_vector_type(8)));
  using type = typename std::conditional<kVec, t8, T>::type;
  static constexpr int kElems = kVec ? 8 : 1;
};

template <typename T, bool kVec>
__device__ __forceinline__ float piece_get(
    const typename Piece<T, kVec>::type &p, int j) {
  if constexpr (kVec) return (float)p[j]; else return (float)p;
}

template <typename T, bool kVec>
__device__ __forceinline__ void piece_set(typename Piece<T, kVec>::type *p,
                                          int j, float v) {
  if constexpr (kVec) (*p)[j] = (T)v; else *p = (T)v;
}

template <typename T, bool kVec>
__device__ __forceinline__ typename Piece<T, kVec>::type piece_zero() {
  typename Piece<T, kVec>::type p;
#pragma unroll
  for (int j = 0; j < Piece<T, kVec>::kElems; ++j)
    piece_set<T, kVec>(&p, j, 0.0f);
  return p;
}

// The wave index as a scalar, so that everything derived from it (rows,
// searches, row bases) stays in scalar registers.
__device__ __forceinline__ int wave_index() {
  return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

template <typename T, typename W, bool kVec>
__global__ void __launch_bounds__(kThreads)
    padded_gather_kernel(const T *__restrict__ x,
                         const int *__restrict__ indices,
                         const int *__restrict__ bins,
                         const int *__restrict__ padded_bins,
                         const W *__restrict__ weights, T *__restrict__ out,
                         int n, int hidden, int top_k, int num_experts,
                         int rows) {
  using P = typename Piece<T, kVec>::type;
  constexpr int kElems = Piece<T, kVec>::kElems;
  const int lane = threadIdx.x & 63;
  const int pieces = hidden / kElems;
  const int tasks = rows / kRowsInFlight + (rows % kRowsInFlight != 0);
  const int stride = gridDim.x * kWaves;
  for (int task = blockIdx.x * kWaves + wave_index(); task < tasks;
       task += stride) {
    const P *src[kRowsInFlight];
    P *dst[kRowsInFlight];
    float wt[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      const int r = task * kRowsInFlight + u;
      const int a = r < rows ? row_assignment(r, indices, bins, padded_bins,
                                              num_experts, n)
                             : -1;
      src[u] = a >= 0 ? reinterpret_cast<const P *>(
                            x + (long long)(a / top_k) * hidden)
                      : nullptr;
      dst[u] = r < rows ? reinterpret_cast<P *>(out + (long long)r * hidden)
                        : nullptr;
      wt[u] = a >= 0 && weights != nullptr ? (float)weights[a] : 1.0f;
    }
    for (int c = lane; c < pieces; c += 64) {
      P v[kRowsInFlight];
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u)
        v[u] = src[u] != nullptr ? src[u][c] : piece_zero<T, kVec>();
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u) {
        if (dst[u] == nullptr) continue;
        // (unweighted: the bits as they are; a zero row has wt 1)
        if (weights != nullptr) {
#pragma unroll
          for (int j = 0; j < kElems; ++j)
            piece_set<T, kVec>(&v[u], j,
                               wt[u] * piece_get<T, kVec>(v[u], j));
        }
        dst[u][c] = v[u];
      }
    }
  }
}

template <typename T, typename W, bool kVec>
__global__ void __launch_bounds__(kThreads)
    padded_scatter_kernel(const T *__restrict__ y,
                          const int *__restrict__ row_of,
                          const W *__restrict__ weights, T *__restrict__ out,
                          int tokens, int hidden, int top_k, int rows) {
  using P = typename Piece<T, kVec>::type;
  constexpr int kElems = Piece<T, kVec>::kElems;
  const int lane = threadIdx.x & 63;
  const int pieces = hidden / kElems;
  const int tasks =
      tokens / kRowsInFlight + (tokens % kRowsInFlight != 0);
  const int stride = gridDim.x * kWaves;
  for (int task = blockIdx.x * kWaves + wave_index(); task < tasks;
       task += stride) {
    const int t0 = task * kRowsInFlight;
    for (int c = lane; c < pieces; c += 64) {
      float acc[kRowsInFlight][kElems];
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
        for (int j = 0; j < kElems; ++j) acc[u][j] = 0.0f;
      for (int k = 0; k < top_k; ++k) {
        P v[kRowsInFlight];
        float wt[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
          const int t = t0 + u;
          const int a = t < tokens ? t * top_k + k : 0;  // < n <= INT_MAX
          const int row = t < tokens ? row_of[a] : -1;
          const bool ok = row >= 0 && row < rows;
          v[u] = ok ? reinterpret_cast<const P *>(
                          y + (long long)row * hidden)[c]
                    : piece_zero<T, kVec>();
          wt[u] = ok && weights != nullptr ? (float)weights[a] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
          for (int j = 0; j < kElems; ++j)
            acc[u][j] += wt[u] * piece_get<T, kVec>(v[u], j);
      }
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u) {
        const int t = t0 + u;
        if (t >= tokens) continue;
        P r;
#pragma unroll
        for (int j = 0; j < kElems; ++j) piece_set<T, kVec>(&r, j, acc[u][j]);
        reinterpret_cast<P *>(out + (long long)t * hidden)[c] = r;
      }
    }
  }
}

template <typename T, typename W, bool kVec>
__global__ void __launch_bounds__(kThreads)
    padded_scatter_wgrad_kernel(const T *__restrict__ dout,
                                const T *__restrict__ y,
                                const int *__restrict__ row_of,
                                W *__restrict__ dw, int n, int hidden,
                                int top_k, int rows) {
  using P = typename Piece<T, kVec>::type;
  constexpr int kElems = Piece<T, kVec>::kElems;
  const int lane = threadIdx.x & 63;
  const int pieces = hidden / kElems;
  const int stride = gridDim.x * kWaves;
  for (long long a = blockIdx.x * kWaves + wave_index(); a < n;
       a += stride) {
    const int row = row_of[a];
    float s = 0.0f;
    if (row >= 0 && row < rows) {
      const P *d = reinterpret_cast<const P *>(
          dout + (long long)(a / top_k) * hidden);
      const P *r = reinterpret_cast<const P *>(y + (long long)row * hidden);
      // kRowsInFlight pieces of each of the two rows in flight per lane.
      for (int c0 = lane; c0 < pieces; c0 += 64 * kRowsInFlight) {
        P dv[kRowsInFlight], rv[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
          const int c = c0 + 64 * u;
          dv[u] = c < pieces ? d[c] : piece_zero<T, kVec>();
          rv[u] = c < pieces ? r[c] : piece_zero<T, kVec>();
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
          for (int j = 0; j < kElems; ++j)
            s += piece_get<T, kVec>(dv[u], j) * piece_get<T, kVec>(rv[u], j);
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) dw[a] = (W)s;
  }
}

// ---- metadata ---------------------------------------------------------------
// One workgroup. bins[e] = #{i : bin_ids[i] <= e}, a binary search of the
// sorted ids per expert; then tokens_per_expert (the differences) and
// padded_bins (the inclusive scan of the counts rounded up to 128): each
// thread a contiguous run of experts, the run totals scanned through LDS.
__global__ void __launch_bounds__(kMetaThreads)
    moe_bins_kernel(const int *__restrict__ bin_ids, int n, int num_experts,
                    int *bins, int *__restrict__ tokens_per_expert,
                    int *__restrict__ padded_bins) {
  __shared__ int partial[kMetaThreads];
  const int tid = threadIdx.x;
  for (int e = tid; e < num_experts; e += kMetaThreads)
    bins[e] = upper_bound(bin_ids, n, e);
  __syncthreads();  // (bins written above are read by other threads below)
  const int per = (num_experts + kMetaThreads - 1) / kMetaThreads;
  const int e0 = min(tid * per, num_experts);
  const int e1 = min(e0 + per, num_experts);
  // (a count is in [0, n] for sorted ids, and clamped to that for ids that
  // are not: they give some bins, which every consumer range-checks)
  auto count = [&](int e) {
    const int c = bins[e] - (e ? bins[e - 1] : 0);
    return min(max(c, 0), n);
  };
  int sum = 0;
  for (int e = e0; e < e1; ++e) sum += (count(e) + 127) & ~127;
  partial[tid] = sum;
  __syncthreads();
  for (int stride = 1; stride < kMetaThreads; stride <<= 1) {
    const int v = tid >= stride ? partial[tid - stride] : 0;
    __syncthreads();
    partial[tid] += v;
    __syncthreads();
  }
  int run = partial[tid] - sum;
  for (int e = e0; e < e1; ++e) {
    const int c = count(e);
    run += (c + 127) & ~127;
    tokens_per_expert[e] = c;
    padded_bins[e] = run;
  }
}

__global__ void __launch_bounds__(256)
    moe_row_map_kernel(const int *__restrict__ indices,
                       const int *__restrict__ bin_ids,
                       const int *__restrict__ bins,
                       const int *__restrict__ padded_bins, int n,
                       int num_experts, int rows, int *__restrict__ row_of) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int a = indices[i];
  if (a < 0 || a >= n) return;
  const int e = bin_ids[i];
  long long row = -1;
  if (e >= 0 && e < num_experts) {
    const int pad0 = e ? padded_bins[e - 1] : 0;
    const int bin0 = e ? bins[e - 1] : 0;
    row = (long long)pad0 + ((long long)i - bin0);
    if (i < bin0 || row < 0 || row >= rows) row = -1;
  }
  row_of[a] = (int)row;
}

// ---- launchers ----------------------------------------------------------------

int DeviceCus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      cus <= 0)
    return 256;
  return cus;
}

// Workgroups for `tasks` wave tasks: one wave each, capped per CU.
unsigned GridFor(long long tasks) {
  long long grid = (tasks + kWaves - 1) / kWaves;
  const long long cap = (long long)kWorkgroupsPerCu * DeviceCus();
  if (grid > cap) grid = cap;
  return (unsigned)(grid < 1 ? 1 : grid);
}

bool Aligned16(std::initializer_list<const void *> ptrs) {
  uintptr_t bits = 0;
  for (const void *p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15) == 0;
}

bool SizesOk(int tokens, int hidden, int top_k, int rows, int dtype) {
  return tokens >= 0 && hidden >= 0 && top_k >= 1 && rows >= 0 &&
         rows % 128 == 0 && (dtype == 0 || dtype == 1) &&
         (long long)tokens * top_k <= INT_MAX;
}

// f(T, W, kVec) for the call's types: T the operand type, W the weights'.
template <typename F>
hipError_t WithTypes(int dtype, int weights_dtype, bool vec, F f) {
  auto with_vec = [&](auto t, auto w) {
    using T = decltype(t);
    using W = decltype(w);
    return vec ? f(T{}, W{}, std::true_type{}) : f(T{}, W{}, std::false_type{});
  };
  if (dtype == 1)
    return weights_dtype == 1 ? with_vec(__bf16{}, float{})
                              : with_vec(__bf16{}, __bf16{});
  return weights_dtype == 1 ? with_vec(_Float16{}, float{})
                            : with_vec(_Float16{}, _Float16{});
}

}  // namespace

hipError_t RunMoeBins(const int *bin_ids, int n, int num_experts, int *bins,
                      int *tokens_per_expert, int *padded_bins,
                      hipStream_t stream) {
  if (n < 0 || num_experts < 0 ||
      (long long)n + 127LL * num_experts > INT_MAX)
    return hipErrorInvalidValue;
  if (num_experts == 0) return hipSuccess;
  if (bins == nullptr || tokens_per_expert == nullptr ||
      padded_bins == nullptr || (n > 0 && bin_ids == nullptr))
    return hipErrorInvalidValue;
  if (bins == tokens_per_expert || bins == padded_bins ||
      tokens_per_expert == padded_bins || bins == bin_ids ||
      tokens_per_expert == bin_ids || padded_bins == bin_ids)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(moe_bins_kernel, dim3(1), dim3(kMetaThreads), 0, stream,
                     bin_ids, n, num_experts, bins, tokens_per_expert,
                     padded_bins);
  return hipGetLastError();
}

hipError_t RunMoeRowMap(const int *indices, const int *bin_ids,
                        const int *bins, const int *padded_bins, int n,
                        int num_experts, int rows, int *row_of,
                        hipStream_t stream) {
  if (n < 0 || num_experts < 0 || rows < 0 || rows % 128 != 0)
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (indices == nullptr || bin_ids == nullptr || row_of == nullptr ||
      (num_experts > 0 && (bins == nullptr || padded_bins == nullptr)))
    return hipErrorInvalidValue;
  if (row_of == indices || row_of == bin_ids || row_of == bins ||
      row_of == padded_bins)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(moe_row_map_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     stream, indices, bin_ids, bins, padded_bins, n,
                     num_experts, rows, row_of);
  return hipGetLastError();
}

hipError_t RunPaddedGather(const void *x, const int *indices, const int *bins,
                           const int *padded_bins, const void *weights,
                           void *out, int tokens, int hidden, int top_k,
                           int num_experts, int rows, int dtype,
                           int weights_dtype, hipStream_t stream) {
  if (!SizesOk(tokens, hidden, top_k, rows, dtype) || num_experts < 0 ||
      (weights != nullptr && weights_dtype != 0 && weights_dtype != 1))
    return hipErrorInvalidValue;
  if (rows == 0 || hidden == 0) return hipSuccess;
  const int n = tokens * top_k;
  // (without assignments or experts every row is a zero row)
  const bool routed = n > 0 && num_experts > 0;
  if (out == nullptr ||
      (routed && (x == nullptr || indices == nullptr || bins == nullptr ||
                  padded_bins == nullptr)))
    return hipErrorInvalidValue;
  if (out == x || out == weights || out == indices || out == bins ||
      out == padded_bins)
    return hipErrorInvalidValue;
  const bool vec = hidden % 8 == 0 && Aligned16({x, out});
  const unsigned grid =
      GridFor(((long long)rows + kRowsInFlight - 1) / kRowsInFlight);
  return WithTypes(dtype, weights != nullptr ? weights_dtype : 0, vec,
                   [&](auto t, auto w, auto v) {
    using T = decltype(t);
    using W = decltype(w);
    hipLaunchKernelGGL((padded_gather_kernel<T, W, decltype(v)::value>),
                       dim3(grid), dim3(kThreads), 0, stream,
                       static_cast<const T *>(x), indices, bins, padded_bins,
                       static_cast<const W *>(weights), static_cast<T *>(out),
                       routed ? n : 0, hidden, top_k,
                       routed ? num_experts : 0, rows);
    return hipGetLastError();
  });
}

hipError_t RunPaddedScatter(const void *y, const int *row_of,
                            const void *weights, void *out, int tokens,
                            int hidden, int top_k, int rows, int dtype,
                            int weights_dtype, hipStream_t stream) {
  if (!SizesOk(tokens, hidden, top_k, rows, dtype) ||
      (weights != nullptr && weights_dtype != 0 && weights_dtype != 1))
    return hipErrorInvalidValue;
  if (tokens == 0 || hidden == 0) return hipSuccess;
  if (out == nullptr || row_of == nullptr || (rows > 0 && y == nullptr))
    return hipErrorInvalidValue;
  if (out == y || out == weights || out == row_of)
    return hipErrorInvalidValue;
  const bool vec = hidden % 8 == 0 && Aligned16({y, out});
  const unsigned grid =
      GridFor(((long long)tokens + kRowsInFlight - 1) / kRowsInFlight);
  return WithTypes(dtype, weights != nullptr ? weights_dtype : 0, vec,
                   [&](auto t, auto w, auto v) {
    using T = decltype(t);
    using W = decltype(w);
    hipLaunchKernelGGL((padded_scatter_kernel<T, W, decltype(v)::value>),
                       dim3(grid), dim3(kThreads), 0, stream,
                       static_cast<const T *>(y), row_of,
                       static_cast<const W *>(weights), static_cast<T *>(out),
                       tokens, hidden, top_k, rows);
    return hipGetLastError();
  });
}

hipError_t RunPaddedScatterWgrad(const void *dout, const void *y,
                                 const int *row_of, void *dw, int tokens,
                                 int hidden, int top_k, int rows, int dtype,
                                 int weights_dtype, hipStream_t stream) {
  if (!SizesOk(tokens, hidden, top_k, rows, dtype) ||
      (weights_dtype != 0 && weights_dtype != 1))
    return hipErrorInvalidValue;
  if (tokens == 0) return hipSuccess;
  if (dw == nullptr || row_of == nullptr ||
      (hidden > 0 && (dout == nullptr || (rows > 0 && y == nullptr))))
    return hipErrorInvalidValue;
  if (dw == dout || dw == y || dw == row_of) return hipErrorInvalidValue;
  const int n = tokens * top_k;
  const bool vec = hidden % 8 == 0 && Aligned16({dout, y});
  const unsigned grid = GridFor(n);
  return WithTypes(dtype, weights_dtype, vec, [&](auto t, auto w, auto v) {
    using T = decltype(t);
    using W = decltype(w);
    hipLaunchKernelGGL(
        (padded_scatter_wgrad_kernel<T, W, decltype(v)::value>), dim3(grid),
        dim3(kThreads), 0, stream, static_cast<const T *>(dout),
        static_cast<const T *>(y), row_of, static_cast<W *>(dw), n, hidden,
        top_k, rows);
    return hipGetLastError();
  });
}

}  // namespace sputnik_amd

namespace sputnik {
namespace block {

hipError_t MoeBins(const int *bin_ids, int n, int num_experts, int *bins,
                   int *tokens_per_expert, int *padded_bins,
                   hipStream_t stream) {
  return sputnik_amd::RunMoeBins(bin_ids, n, num_experts, bins,
                                 tokens_per_expert, padded_bins, stream);
}

hipError_t MoeRowMap(const int *indices, const int *bin_ids, const int *bins,
                     const int *padded_bins, int n, int num_experts, int rows,
                     int *row_of, hipStream_t stream) {
  return sputnik_amd::RunMoeRowMap(indices, bin_ids, bins, padded_bins, n,
                                   num_experts, rows, row_of, stream);
}

hipError_t PaddedGather(const void *x, const int *indices, const int *bins,
                        const int *padded_bins, const void *weights,
                        void *out, int tokens, int hidden, int top_k,
                        int num_experts, int rows, DataType dtype,
                        WeightType weights_type, hipStream_t stream) {
  return sputnik_amd::RunPaddedGather(x, indices, bins, padded_bins, weights,
                                      out, tokens, hidden, top_k, num_experts,
                                      rows, (int)dtype, (int)weights_type,
                                      stream);
}

hipError_t PaddedScatter(const void *y, const int *row_of,
                         const void *weights, void *out, int tokens,
                         int hidden, int top_k, int rows, DataType dtype,
                         WeightType weights_type, hipStream_t stream) {
  return sputnik_amd::RunPaddedScatter(y, row_of, weights, out, tokens, hidden,
                                       top_k, rows, (int)dtype,
                                       (int)weights_type, stream);
}

hipError_t PaddedScatterWeightGrad(const void *dout, const void *y,
                                   const int *row_of, void *dw, int tokens,
                                   int hidden, int top_k, int rows,
                                   DataType dtype, WeightType weights_type,
                                   hipStream_t stream) {
  return sputnik_amd::RunPaddedScatterWgrad(dout, y, row_of, dw, tokens,
                                            hidden, top_k, rows, (int)dtype,
                                            (int)weights_type, stream);
}

}  // namespace block
}  // namespace sputnik
