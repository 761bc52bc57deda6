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
// The scatter and the weight gradient are each one kernel body and one
// launcher, instantiated on `bool kBias` for the calls with an output bias
// (PaddedScatterBias, PaddedScatterBiasWeightGrad): kBias adds the expert
// read off the row, the load of its bias piece and the bias arithmetic, and
// nothing to the plain instantiation. The bias gradient is a column
// reduction of its own shape.
//
// Every index read from device memory (indices[i], bins / padded_bins
// entries, row_of[a]) is range-checked before it forms an address; an entry
// out of range stands for a row of zeros.
//
// The sputnik::block functions at the end are the host entry points, of the
// C++ API and (through c_api.cpp) of the C-ABI: they validate and launch.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

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

// The expert that owns padded row `row`, or -1: #{e : padded_bins[e] <= row}
// for a row in [0, rows) that lies in front of padded_bins[E-1].
__device__ __forceinline__ int row_expert(int row, int rows,
                                          const int *__restrict__ padded_bins,
                                          int num_experts) {
  if (row < 0 || row >= rows) return -1;
  const int e = upper_bound(padded_bins, num_experts, row);
  return e < num_experts ? e : -1;
}

// The scatter, with kBias the scatter with an output bias (moe.h
// PaddedScatterBias). kBias adds the expert of every pick, read off its row
// through padded_bins (a row that no expert owns contributes zero, bias
// included), one more load per pick (the piece of bias[e]) and the arithmetic
// as moe.h states it: one add, one multiply (with weights) and one accumulate
// per k, contraction off. Without it the sum is acc += wt * y under the
// compiler's default contraction, and padded_bins and bias are not read.
//
// kHoist picks are looked up in front of the piece loop: 4 with a bias, whose
// lookup is a search of padded_bins, and 1 without, where it is a range check
// and a weight load. Measured (profiles/moe_permute_refactor/README.md):
// holding 4 plain picks across the loop is 3% slower with fp32 weights at
// top_k 2, holding none 3% slower with weights of T at top_k 1.
template <typename T, typename W, bool kVec, bool kBias>
__global__ void __launch_bounds__(kThreads)
    padded_scatter_kernel(const T *__restrict__ y,
                          const int *__restrict__ row_of,
                          const int *__restrict__ padded_bins,
                          const T *__restrict__ bias,
                          const W *__restrict__ weights, T *__restrict__ out,
                          int tokens, int hidden, int top_k, int num_experts,
                          int rows) {
  constexpr int kHoist = kBias ? 4 : 1;
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
    // The row, expert (0 without a bias) and weight of pick k of the task's
    // tokens (e < 0: contributes zero). Wave-uniform; the first kHoist picks
    // are looked up once per task, so that the searches are not on every
    // piece's path to its loads.
    struct Pick { int row, e; float wt; };
    auto pick = [&](int u, int k) {
      const int t = t0 + u;
      const int a = t < tokens ? t * top_k + k : 0;  // < n <= INT_MAX
      const int row = t < tokens ? row_of[a] : -1;
      int e;
      if constexpr (kBias)
        e = row_expert(row, rows, padded_bins, num_experts);
      else
        e = row >= 0 && row < rows ? 0 : -1;
      return Pick{row, e,
                  e >= 0 && weights != nullptr ? (float)weights[a] : 1.0f};
    };
    Pick first[kHoist][kRowsInFlight];
#pragma unroll
    for (int k = 0; k < kHoist; ++k)
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u)
        first[k][u] = k < top_k ? pick(u, k) : Pick{-1, -1, 1.0f};
    for (int c = lane; c < pieces; c += 64) {
      float acc[kRowsInFlight][kElems];
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
        for (int j = 0; j < kElems; ++j) acc[u][j] = 0.0f;
      // One pick of every token: the loads, then the sum.
      auto step = [&](const Pick (&q)[kRowsInFlight]) {
        P v[kRowsInFlight], b[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
          const bool ok = q[u].e >= 0;
          v[u] = ok ? reinterpret_cast<const P *>(
                          y + (long long)q[u].row * hidden)[c]
                    : piece_zero<T, kVec>();
          if constexpr (kBias)
            b[u] = ok ? reinterpret_cast<const P *>(
                            bias + (long long)q[u].e * hidden)[c]
                      : piece_zero<T, kVec>();
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
          for (int j = 0; j < kElems; ++j) {
            if constexpr (kBias) {
#pragma clang fp contract(off)
              float s =
                  piece_get<T, kVec>(v[u], j) + piece_get<T, kVec>(b[u], j);
              if (weights != nullptr) s = q[u].wt * s;
              acc[u][j] = acc[u][j] + s;
            } else {
              acc[u][j] += q[u].wt * piece_get<T, kVec>(v[u], j);
            }
          }
      };
#pragma unroll
      for (int k = 0; k < kHoist; ++k)
        if (k < top_k) step(first[k]);
      for (int k = kHoist; k < top_k; ++k) {
        Pick q[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) q[u] = pick(u, k);
        step(q);
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

// The router-weight gradient; with kBias of the scatter with a bias:
// dot(dout, y + bias[e]), e read off the row as above.
template <typename T, typename W, bool kVec, bool kBias>
__global__ void __launch_bounds__(kThreads)
    padded_scatter_wgrad_kernel(const T *__restrict__ dout,
                                const T *__restrict__ y,
                                const int *__restrict__ row_of,
                                W *__restrict__ dw, int n, int hidden,
                                int top_k, int rows,
                                const int *__restrict__ padded_bins,
                                const T *__restrict__ bias, int num_experts) {
  using P = typename Piece<T, kVec>::type;
  constexpr int kElems = Piece<T, kVec>::kElems;
  const int lane = threadIdx.x & 63;
  const int pieces = hidden / kElems;
  const int stride = gridDim.x * kWaves;
  for (long long a = blockIdx.x * kWaves + wave_index(); a < n;
       a += stride) {
    const int row = row_of[a];
    int e = 0;
    if constexpr (kBias) e = row_expert(row, rows, padded_bins, num_experts);
    float s = 0.0f;
    if (kBias ? e >= 0 : row >= 0 && row < rows) {
      const P *d = reinterpret_cast<const P *>(
          dout + (long long)(a / top_k) * hidden);
      const P *r = reinterpret_cast<const P *>(y + (long long)row * hidden);
      const P *b = nullptr;
      if constexpr (kBias)
        b = reinterpret_cast<const P *>(bias + (long long)e * hidden);
      // kRowsInFlight pieces of each of the rows in flight per lane.
      for (int c0 = lane; c0 < pieces; c0 += 64 * kRowsInFlight) {
        P dv[kRowsInFlight], rv[kRowsInFlight], bv[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
          const int c = c0 + 64 * u;
          dv[u] = c < pieces ? d[c] : piece_zero<T, kVec>();
          rv[u] = c < pieces ? r[c] : piece_zero<T, kVec>();
          if constexpr (kBias)
            bv[u] = c < pieces ? b[c] : piece_zero<T, kVec>();
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
          for (int j = 0; j < kElems; ++j) {
            if constexpr (kBias)
              s += piece_get<T, kVec>(dv[u], j) *
                   (piece_get<T, kVec>(rv[u], j) +
                    piece_get<T, kVec>(bv[u], j));
            else
              s += piece_get<T, kVec>(dv[u], j) * piece_get<T, kVec>(rv[u], j);
          }
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) dw[a] = (W)s;
  }
}

// db2[e, h] = sum over expert e's sorted positions i of w[indices[i]] *
// dout[indices[i] / top_k, h]. One workgroup per (expert, slice of 16 pieces
// of a row: 256 bytes on the vector path). Thread (g, l), g = 0..63, takes
// piece l of positions b0 + g, b0 + g + 64, ..., kRowsInFlight of them in
// flight, and adds them in that order; the 64 partial sums of a column are
// then added through LDS in g order by one thread. No atomics, no workspace;
// the order depends on the bins alone.
constexpr int kReduceThreads = 1024;
constexpr int kReduceGroups = kReduceThreads / 16;

template <typename T, typename W, bool kVec>
__global__ void __launch_bounds__(kReduceThreads)
    padded_scatter_bias_grad_kernel(const T *__restrict__ dout,
                                    const int *__restrict__ indices,
                                    const int *__restrict__ bins,
                                    const W *__restrict__ weights,
                                    float *__restrict__ db, int n, int hidden,
                                    int top_k, int slices) {
#pragma clang fp contract(off)
  using P = typename Piece<T, kVec>::type;
  constexpr int kElems = Piece<T, kVec>::kElems;
  __shared__ float part[kReduceGroups][16 * kElems];
  const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int e = blockIdx.x / slices, slice = blockIdx.x % slices;
  const int c = slice * 16 + l;  // this thread's piece
  const int pieces = hidden / kElems;
  int b0 = e ? bins[e - 1] : 0, b1 = bins[e];
  // (bins out of range: the part of them that is in range)
  b0 = min(max(b0, 0), n);
  b1 = min(max(b1, b0), n);
  float acc[kElems];
#pragma unroll
  for (int j = 0; j < kElems; ++j) acc[j] = 0.0f;
  for (int i0 = b0 + g; i0 < b1; i0 += kReduceGroups * kRowsInFlight) {
    P v[kRowsInFlight];
    float wt[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      const int i = i0 + u * kReduceGroups;
      const int a = i < b1 ? indices[i] : -1;
      const bool ok = a >= 0 && a < n && c < pieces;
      v[u] = ok ? reinterpret_cast<const P *>(
                      dout + (long long)(a / top_k) * hidden)[c]
                : piece_zero<T, kVec>();
      wt[u] = ok && weights != nullptr ? (float)weights[a] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
      for (int j = 0; j < kElems; ++j)
        acc[j] = acc[j] + wt[u] * piece_get<T, kVec>(v[u], j);
  }
#pragma unroll
  for (int j = 0; j < kElems; ++j) part[g][l * kElems + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < 16 * kElems) {
    float s = 0.0f;
#pragma unroll 8
    for (int r = 0; r < kReduceGroups; ++r) s = s + part[r][threadIdx.x];
    const long long h = (long long)slice * 16 * kElems + threadIdx.x;
    if (h < hidden) db[(long long)e * hidden + h] = s + 0.0f;
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

// PaddedScatter (`biased` false: bias and padded_bins null, num_experts 0)
// and PaddedScatterBias. The plain entry reads y whenever there are rows and
// passes `rows` through; the bias entry reads y, bias and padded_bins only
// with both rows and experts, and otherwise runs with num_experts = rows = 0
// (every assignment contributes zero). The kernel takes its bias form when
// there is a bias.
hipError_t LaunchScatter(const void *y, const int *row_of,
                         const int *padded_bins, const void *bias,
                         const void *weights, void *out, int tokens,
                         int hidden, int top_k, int num_experts, int rows,
                         int dtype, int weights_dtype, bool biased,
                         hipStream_t stream) {
  if (!SizesOk(tokens, hidden, top_k, rows, dtype) || num_experts < 0 ||
      (weights != nullptr && weights_dtype != 0 && weights_dtype != 1))
    return hipErrorInvalidValue;
  if (tokens == 0 || hidden == 0) return hipSuccess;
  const bool routed = rows > 0 && (!biased || num_experts > 0);
  if (out == nullptr || row_of == nullptr ||
      (routed && (y == nullptr ||
                  (biased && (bias == nullptr || padded_bins == nullptr)))))
    return hipErrorInvalidValue;
  if (out == y || out == weights || out == row_of ||
      (biased && (out == bias || out == padded_bins)))
    return hipErrorInvalidValue;
  const bool vec = hidden % 8 == 0 && Aligned16({y, out, bias});
  const unsigned grid =
      GridFor(((long long)tokens + kRowsInFlight - 1) / kRowsInFlight);
  return WithTypes(dtype, weights != nullptr ? weights_dtype : 0, vec,
                   [&](auto t, auto w, auto v) {
    using T = decltype(t);
    using W = decltype(w);
    auto launch = [&](auto b) {
      hipLaunchKernelGGL(
          (padded_scatter_kernel<T, W, decltype(v)::value, decltype(b)::value>),
          dim3(grid), dim3(kThreads), 0, stream, static_cast<const T *>(y),
          row_of, padded_bins, static_cast<const T *>(bias),
          static_cast<const W *>(weights), static_cast<T *>(out), tokens,
          hidden, top_k, routed ? num_experts : 0, routed ? rows : 0);
      return hipGetLastError();
    };
    return bias != nullptr ? launch(std::true_type{})
                           : launch(std::false_type{});
  });
}

// PaddedScatterWeightGrad and PaddedScatterBiasWeightGrad, as above. The
// plain entry reads dout whenever hidden > 0 and y with rows; the bias entry
// reads its operands only with rows, experts and hidden all there.
hipError_t LaunchScatterWgrad(const void *dout, const void *y,
                              const int *row_of, const int *padded_bins,
                              const void *bias, void *dw, int tokens,
                              int hidden, int top_k, int num_experts,
                              int rows, int dtype, int weights_dtype,
                              bool biased, hipStream_t stream) {
  if (!SizesOk(tokens, hidden, top_k, rows, dtype) || num_experts < 0 ||
      (weights_dtype != 0 && weights_dtype != 1))
    return hipErrorInvalidValue;
  if (tokens == 0) return hipSuccess;
  const bool routed = !biased || (rows > 0 && num_experts > 0 && hidden > 0);
  const bool reads_dout = biased ? routed : hidden > 0;
  const bool reads_y = biased ? routed : hidden > 0 && rows > 0;
  if (dw == nullptr || row_of == nullptr || (reads_dout && dout == nullptr) ||
      (reads_y && y == nullptr) ||
      (biased && routed && (bias == nullptr || padded_bins == nullptr)))
    return hipErrorInvalidValue;
  if (dw == dout || dw == y || dw == row_of ||
      (biased && (dw == bias || dw == padded_bins)))
    return hipErrorInvalidValue;
  const int n = tokens * top_k;
  const bool vec = hidden % 8 == 0 && Aligned16({dout, y, bias});
  const unsigned grid = GridFor(n);
  return WithTypes(dtype, weights_dtype, vec, [&](auto t, auto w, auto v) {
    using T = decltype(t);
    using W = decltype(w);
    auto launch = [&](auto b) {
      hipLaunchKernelGGL(
          (padded_scatter_wgrad_kernel<T, W, decltype(v)::value,
                                       decltype(b)::value>),
          dim3(grid), dim3(kThreads), 0, stream, static_cast<const T *>(dout),
          static_cast<const T *>(y), row_of, static_cast<W *>(dw), n, hidden,
          top_k, routed ? rows : 0, padded_bins, static_cast<const T *>(bias),
          routed ? num_experts : 0);
      return hipGetLastError();
    };
    return bias != nullptr ? launch(std::true_type{})
                           : launch(std::false_type{});
  });
}

}  // namespace
}  // namespace sputnik_amd

// The host entry points (sputnik/block/moe.h), also behind the C-ABI: each
// validates its arguments (hipErrorInvalidValue, nothing launched; the enums
// by their integer value, 0 or 1), returns hipSuccess for zero-sized work,
// and otherwise enqueues its kernel on `stream`. None allocates or
// synchronises.
namespace sputnik {
namespace block {

using namespace sputnik_amd;  // NOLINT: the kernels and launchers above

hipError_t MoeBins(const int *bin_ids, int n, int num_experts, int *bins,
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

hipError_t MoeRowMap(const int *indices, const int *bin_ids, const int *bins,
                     const int *padded_bins, int n, int num_experts, int rows,
                     int *row_of, hipStream_t stream) {
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

hipError_t PaddedGather(const void *x, const int *indices, const int *bins,
                        const int *padded_bins, const void *weights,
                        void *out, int tokens, int hidden, int top_k,
                        int num_experts, int rows, DataType dtype,
                        WeightType weights_type, hipStream_t stream) {
  const int weights_dtype = (int)weights_type;
  if (!SizesOk(tokens, hidden, top_k, rows, (int)dtype) || num_experts < 0 ||
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
  return WithTypes((int)dtype, weights != nullptr ? weights_dtype : 0, vec,
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

hipError_t PaddedScatter(const void *y, const int *row_of,
                         const void *weights, void *out, int tokens,
                         int hidden, int top_k, int rows, DataType dtype,
                         WeightType weights_type, hipStream_t stream) {
  return LaunchScatter(y, row_of, nullptr, nullptr, weights, out, tokens,
                       hidden, top_k, 0, rows, (int)dtype, (int)weights_type,
                       false, stream);
}

hipError_t PaddedScatterWeightGrad(const void *dout, const void *y,
                                   const int *row_of, void *dw, int tokens,
                                   int hidden, int top_k, int rows,
                                   DataType dtype, WeightType weights_type,
                                   hipStream_t stream) {
  return LaunchScatterWgrad(dout, y, row_of, nullptr, nullptr, dw, tokens,
                            hidden, top_k, 0, rows, (int)dtype,
                            (int)weights_type, false, stream);
}

hipError_t PaddedScatterBias(const void *y, const int *row_of,
                             const int *padded_bins, const void *bias,
                             const void *weights, void *out, int tokens,
                             int hidden, int top_k, int num_experts, int rows,
                             DataType dtype, WeightType weights_type,
                             hipStream_t stream) {
  return LaunchScatter(y, row_of, padded_bins, bias, weights, out, tokens,
                       hidden, top_k, num_experts, rows, (int)dtype,
                       (int)weights_type, true, stream);
}

hipError_t PaddedScatterBiasWeightGrad(const void *dout, const void *y,
                                       const int *row_of,
                                       const int *padded_bins,
                                       const void *bias, void *dw, int tokens,
                                       int hidden, int top_k, int num_experts,
                                       int rows, DataType dtype,
                                       WeightType weights_type,
                                       hipStream_t stream) {
  return LaunchScatterWgrad(dout, y, row_of, padded_bins, bias, dw, tokens,
                            hidden, top_k, num_experts, rows, (int)dtype,
                            (int)weights_type, true, stream);
}

hipError_t PaddedScatterBiasGrad(const void *dout, const int *indices,
                                 const int *bins, const void *weights,
                                 float *bias_grad, int tokens, int hidden,
                                 int top_k, int num_experts, DataType dtype,
                                 WeightType weights_type, hipStream_t stream) {
  const int weights_dtype = (int)weights_type;
  if (!SizesOk(tokens, hidden, top_k, 0, (int)dtype) || num_experts < 0 ||
      (weights != nullptr && weights_dtype != 0 && weights_dtype != 1))
    return hipErrorInvalidValue;
  if (num_experts == 0 || hidden == 0) return hipSuccess;
  const int n = tokens * top_k;
  if (bias_grad == nullptr || bins == nullptr ||
      (n > 0 && (dout == nullptr || indices == nullptr)))
    return hipErrorInvalidValue;
  if (bias_grad == dout || bias_grad == weights ||
      bias_grad == (const void *)indices || bias_grad == (const void *)bins)
    return hipErrorInvalidValue;
  const bool vec = hidden % 8 == 0 && Aligned16({dout});
  const int per_slice = 16 * (vec ? 8 : 1);
  const long long slices = ((long long)hidden + per_slice - 1) / per_slice;
  if (slices * num_experts > INT_MAX) return hipErrorInvalidValue;
  return WithTypes((int)dtype, weights != nullptr ? weights_dtype : 0, vec,
                   [&](auto t, auto w, auto v) {
    using T = decltype(t);
    using W = decltype(w);
    hipLaunchKernelGGL(
        (padded_scatter_bias_grad_kernel<T, W, decltype(v)::value>),
        dim3((unsigned)(slices * num_experts)), dim3(kReduceThreads), 0,
        stream, static_cast<const T *>(dout), indices, bins,
        static_cast<const W *>(weights), bias_grad, n, hidden, top_k,
        (int)slices);
    return hipGetLastError();
  });
}

}  // namespace block
}  // namespace sputnik

