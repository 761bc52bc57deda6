// sputnik-amd: the MoE router (sputnik/block/router.h): fused softmax / top-k
// of the router logits, its gradient, the same for sigmoid scores with a
// selection bias and a group-limited choice, and the stable counting sort that
// turns top_experts into MegaBlocks' routing tensors.
//
// Router kernels: one wave per token, 4 waves per workgroup, a token's E
// logits spread over the lanes as e = lane + 64 j with j < kPer = ceil(E / 64)
// rounded up to a power of two (a template parameter, so the logits stay in
// registers: every loop over j is unrolled, nothing is indexed dynamically).
//
//   top-k   k rounds of a wave arg-max over 64-bit keys: the order-preserving
//           image of the fp32 value in the high word (NaN below -inf, -0 as
//           +0), ~e in the low word, so that the larger key is the larger
//           value and, among equal values, the lower index. A picked entry's
//           key becomes 0, below every live key. The key carries the value,
//           so the row maximum (pick 0) and every picked logit come out of
//           the reduction itself. Lane r keeps pick r; the softmax sum is one
//           more wave reduction.
//   grad    recomputes p from the logits; lane r < k reads pick r's id and
//           gradient (the id range-checked before it addresses the logits),
//           the per-pick terms are reduced across the wave and added to the
//           owning lane's dp by k broadcast rounds, so a duplicated id adds
//           twice and nothing is written through an id.
//   aux     the forward pass with the loss statistics: a workgroup covers
//           kRouterAuxTokens = 64 consecutive tokens, 16 per wave in order;
//           each lane adds its columns' unrounded probabilities into kPer
//           registers (no cross-lane traffic) and the wave (m + log s)^2. The
//           four waves meet in LDS and are added in wave order; the E + 1
//           partials go to workspace[group]. A second launch adds the groups
//           in ascending order, one thread per column. No atomics: the sums
//           are a function of the input alone. The gradient takes the sums'
//           gradients as one [E] vector and one device scalar.
//
//   score   RouterScoreTopK / RouterScoreTopKGrad, the same layout and the
//           same keys on c = sigmoid(l) + bias, with a body of their own
//           (router_score_token, router_score_grad_kernel; the softmax bodies
//           know nothing of them). Before the pick rounds the group step
//           kills the keys of the experts outside the topk_groups best
//           groups: the wave stages the keys' high words in LDS, 64 / G lanes
//           per group scan for the group's two largest, a few shuffle steps
//           merge them, and topk_groups arg-max rounds rank the group keys.
//
// Each pass is written once and instantiated twice on `bool kStats`:
// router_topk_token is one token of RouterTopK (false: no accumulators) and of
// RouterTopKAux (true), and router_topk_grad_kernel is RouterTopKGrad (false)
// and RouterTopKAuxGrad (true; false again when it is given neither
// statistic's gradient). That the plain and the aux results agree bit for bit
// is therefore a property of the source: what only the statistics need sits
// under `if constexpr (kStats)`, every other statement is shared.
//
// The host functions at the end are sputnik/block/router.h's own; the C-ABI
// (c_api.cpp) calls them.
//
// Sort: chunks of kMoeSortChunk = 1024 assignments, one per thread.
//   histogram  per chunk: LDS integer adds into E + 1 counters (column E
//              counts the ids outside [0, E)), stored to the workspace
//              [chunks, E + 1]; every entry is written, so the workspace
//              needs no initialisation.
//   scan       one workgroup: column totals -> bins, tokens_per_expert,
//              padded_bins; each workspace entry becomes the first sorted
//              position of its (chunk, id): the exclusive scan over ids of
//              the totals plus the counts of the earlier chunks.
//   placement  per chunk: inside a wave an assignment's rank among equal ids
//              is the popcount of the lower lanes of a ballot-built match
//              mask; across the chunk's 16 waves a running counter per id in
//              LDS is advanced wave by wave in wave order. Position = first
//              position + earlier waves + rank: a function of the input
//              alone, no global atomics.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

#include "sputnik/block/router.h"

namespace sputnik_amd {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxExperts = 1024;
constexpr int kMaxTopK = 32;
constexpr int kMaxGroups = sputnik::block::kRouterMaxGroups;
constexpr int kChunk = sputnik::block::kMoeSortChunk;
constexpr int kSortThreads = 1024;
static_assert(kChunk == kSortThreads, "one assignment per thread");
constexpr int kAuxTokens = sputnik::block::kRouterAuxTokens;
constexpr int kAuxPerWave = kAuxTokens / kWaves;
static_assert(kAuxPerWave * kWaves == kAuxTokens, "whole tokens per wave");

__device__ __forceinline__ int wave_index() {
  return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// Order-preserving image of an fp32 value: a < b  <=>  image(a) < image(b),
// -0 == +0, every NaN the image 1 (below -inf's 0x007fffff, above the 0 of a
// dead key).
__device__ __forceinline__ uint32_t order_image(float v) {
  uint32_t b = __float_as_uint(v);
  if (v != v) return 1u;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float image_value(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long k) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(k, d, 64);
    k = o > k ? o : k;
  }
  return k;
}

// One token of the forward pass, by one wave: the body of router_topk_kernel
// (kStats false; acc and zacc are not touched and may be null) and of
// router_topk_aux_kernel (kStats true), which also adds the token's unrounded
// probabilities to acc[j] (column lane + 64 j, kPer registers) and its
// (m + log s)^2 to *zacc, the same value in every lane.
template <typename T, typename W, int kPer, bool kStats>
__device__ __forceinline__ void router_topk_token(
    const T *__restrict__ logits, int *__restrict__ top_experts,
    W *__restrict__ weights, W *__restrict__ scores, long long t,
    int num_experts, int top_k, int normalize, int lane, float *acc,
    float *zacc) {
  const T *row = logits + t * num_experts;
  float v[kPer];
  unsigned long long key[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int e = lane + 64 * j;
    const bool live = e < num_experts;
    v[j] = live ? (float)row[e] : 0.0f;
    key[j] = live ? ((unsigned long long)order_image(v[j]) << 32) |
                        (uint32_t)~e
                  : 0ull;
  }
  float m = 0.0f, my_val = 0.0f;
  int my_id = 0;
  for (int r = 0; r < top_k; ++r) {
    unsigned long long best = key[0];
#pragma unroll
    for (int j = 1; j < kPer; ++j) best = key[j] > best ? key[j] : best;
    best = wave_max(best);
    // (top_k <= num_experts: a live key remains, so idx is in [0, E))
    const int idx = (int)~(uint32_t)best;
    const float val = image_value((uint32_t)(best >> 32));
    if (r == 0) m = val;
    if (lane == r) {
      my_id = idx;
      my_val = val;
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (idx == lane + 64 * j) key[j] = 0ull;
  }
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (lane + 64 * j < num_experts) s += expf(v[j] - m);
  s = wave_sum(s);
  float p = lane < top_k ? expf(my_val - m) / s : 0.0f;
  if (normalize) p = p / wave_sum(p);
  if (lane < top_k) {
    top_experts[t * top_k + lane] = my_id;
    weights[t * top_k + lane] = (W)p;
  }
  if constexpr (kStats) {
    const float lse = m + logf(s);
    *zacc += lse * lse;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int e = lane + 64 * j;
      if (e < num_experts) {
        const float pe = expf(v[j] - m) / s;
        acc[j] += pe;
        if (scores != nullptr) scores[t * num_experts + e] = (W)pe;
      }
    }
  } else if (scores != nullptr) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int e = lane + 64 * j;
      if (e < num_experts)
        scores[t * num_experts + e] = (W)(expf(v[j] - m) / s);
    }
  }
}

template <typename T, typename W, int kPer>
__global__ void __launch_bounds__(kThreads)
    router_topk_kernel(const T *__restrict__ logits,
                       int *__restrict__ top_experts, W *__restrict__ weights,
                       W *__restrict__ scores, int tokens, int num_experts,
                       int top_k, int normalize) {
  const long long t = (long long)blockIdx.x * kWaves + wave_index();
  if (t >= tokens) return;
  router_topk_token<T, W, kPer, false>(logits, top_experts, weights, scores, t,
                                       num_experts, top_k, normalize,
                                       threadIdx.x & 63, nullptr, nullptr);
}

// RouterTopK plus the column sums of the probabilities and the sum of
// (m + log s)^2: wave w of workgroup g walks tokens [g kAuxTokens + w
// kAuxPerWave, + kAuxPerWave) in order, the four waves' registers meet in LDS
// and are added in wave order, and the E + 1 partials go to partial[g] (column
// E: the z partial; every entry written).
template <typename T, typename W, int kPer>
__global__ void __launch_bounds__(kThreads)
    router_topk_aux_kernel(const T *__restrict__ logits,
                           int *__restrict__ top_experts,
                           W *__restrict__ weights, W *__restrict__ scores,
                           float *__restrict__ partial, int tokens,
                           int num_experts, int top_k, int normalize) {
  __shared__ float cols[kWaves][kPer * 64];
  __shared__ float zs[kWaves];
  const int lane = threadIdx.x & 63;
  const int wave = wave_index();
  const long long t0 =
      (long long)blockIdx.x * kAuxTokens + (long long)wave * kAuxPerWave;
  float acc[kPer], zacc = 0.0f;
#pragma unroll
  for (int j = 0; j < kPer; ++j) acc[j] = 0.0f;
  for (int i = 0; i < kAuxPerWave && t0 + i < tokens; ++i)
    router_topk_token<T, W, kPer, true>(logits, top_experts, weights, scores,
                                        t0 + i, num_experts, top_k, normalize,
                                        lane, acc, &zacc);
#pragma unroll
  for (int j = 0; j < kPer; ++j) cols[wave][lane + 64 * j] = acc[j];
  if (lane == 0) zs[wave] = zacc;
  __syncthreads();
  float *out = partial + (long long)blockIdx.x * (num_experts + 1);
  for (int e = threadIdx.x; e <= num_experts; e += kThreads) {
    float sum = e < num_experts ? cols[0][e] : zs[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
      sum += e < num_experts ? cols[w][e] : zs[w];
    out[e] = sum;
  }
}

// Column c of score_sums / z_sum: the groups' partials added in ascending
// group order from +0, one thread per column.
__global__ void __launch_bounds__(kThreads)
    router_aux_reduce_kernel(const float *__restrict__ partial, int groups,
                             int num_experts, float *__restrict__ score_sums,
                             float *__restrict__ z_sum) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c > num_experts || (c == num_experts && z_sum == nullptr)) return;
  float sum = 0.0f;
  for (int g = 0; g < groups; ++g)
    sum += partial[(long long)g * (num_experts + 1) + c];
  if (c < num_experts)
    score_sums[c] = sum;
  else
    z_sum[0] = sum;
}

// The gradient of both forward passes. kStats false: RouterTopKGrad, and
// RouterTopKAuxGrad given neither statistic's gradient (dscore_sums and dz_sum
// are not looked at). kStats true: dscore_sums[e] (when not null) joins dp and
// 2 dz (m + log s) p_j (when dz_sum is not null) the result.
template <typename T, typename W, int kPer, bool kStats>
__global__ void __launch_bounds__(kThreads)
    router_topk_grad_kernel(const T *__restrict__ logits,
                            const int *__restrict__ top_experts,
                            const W *__restrict__ dweights,
                            const W *__restrict__ dscores,
                            const float *__restrict__ dscore_sums,
                            const float *__restrict__ dz_sum,
                            T *__restrict__ dlogits, int tokens,
                            int num_experts, int top_k, int normalize) {
  const int lane = threadIdx.x & 63;
  const long long t = (long long)blockIdx.x * kWaves + wave_index();
  if (t >= tokens) return;
  const T *row = logits + t * num_experts;
  float v[kPer], dp[kPer];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int e = lane + 64 * j;
    const bool live = e < num_experts;
    v[j] = live ? (float)row[e] : 0.0f;
    dp[j] = live && dscores != nullptr
                ? (float)dscores[t * num_experts + e] : 0.0f;
    if constexpr (kStats)
      if (live && dscore_sums != nullptr) dp[j] += dscore_sums[e];
    if (live) m = fmaxf(m, v[j]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (lane + 64 * j < num_experts) s += expf(v[j] - m);
  s = wave_sum(s);

  // Lane r < top_k holds pick r: its id (-1 when out of range), its incoming
  // gradient and, for normalize, its probability.
  int id = -1;
  float g = 0.0f;
  if (lane < top_k) {
    const int raw = top_experts[t * top_k + lane];
    if (raw >= 0 && raw < num_experts) {
      id = raw;
      g = (float)dweights[t * top_k + lane];
    }
  }
  if (normalize) {
    const float psel = id >= 0 ? expf((float)row[id] - m) / s : 0.0f;
    const float total = wave_sum(psel);             // S
    const float c = wave_sum(g * psel) / total;     // sum_j dw_j w_j
    g = id >= 0 ? (g - c) / total : 0.0f;
  }
  for (int r = 0; r < top_k; ++r) {
    const int rid = __shfl(id, r, 64);
    const float rg = __shfl(g, r, 64);
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (rid == lane + 64 * j) dp[j] += rg;
  }
  float p[kPer];
  float dot = 0.0f;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const bool live = lane + 64 * j < num_experts;
    p[j] = live ? expf(v[j] - m) / s : 0.0f;
    if (live) dot += dp[j] * p[j];
  }
  dot = wave_sum(dot);
  [[maybe_unused]] float zc = 0.0f;  // 2 dz lse
  if constexpr (kStats)
    if (dz_sum != nullptr) zc = 2.0f * dz_sum[0] * (m + logf(s));
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int e = lane + 64 * j;
    if (e < num_experts) {
      float out = p[j] * (dp[j] - dot);
      if constexpr (kStats)
        if (dz_sum != nullptr) out += zc * p[j];
      dlogits[t * num_experts + e] = (T)out;
    }
  }
}

// ---- sigmoid scores, selection bias, group-limited top-k ----------------------

__device__ __forceinline__ float sigmoid(float l) {
  return 1.0f / (1.0f + expf(-l));
}

// One token of RouterScoreTopK, by one wave. The keys are built on c = s +
// bias. The group step works on their high words alone (a group's score needs
// its two largest values, not where they sit): the wave stages the images in
// LDS (`stage`, kPer * 64 words of its own), group g gets the 2^shift = 64 / G
// (rounded down to a power of two) lanes from g << shift on, each lane scans
// its share of the group for a local (a, b), the two largest, `shift` shuffle
// steps merge the pairs, and lane g << shift keeps the group's key. Then
// topk_groups arg-max rounds over the group keys mark the eligible groups'
// experts, the other keys die, and the pick rounds follow. A pick's unbiased
// score comes from the lane that owns it.
template <typename T, typename W, int kPer>
__device__ __forceinline__ void router_score_token(
    const T *__restrict__ logits, const float *__restrict__ bias,
    int *__restrict__ top_experts, W *__restrict__ weights,
    W *__restrict__ scores, long long t, int num_experts, int top_k,
    int num_groups, int topk_groups, int normalize, float scale, int lane,
    uint32_t *stage) {
  const T *row = logits + t * num_experts;
  float s[kPer];
  unsigned long long key[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int e = lane + 64 * j;
    const bool live = e < num_experts;
    s[j] = live ? sigmoid((float)row[e]) : 0.0f;
    const float c = live && bias != nullptr ? s[j] + bias[e] : s[j];
    key[j] = live ? ((unsigned long long)order_image(c) << 32) | (uint32_t)~e
                  : 0ull;
  }
  if (num_groups > 1) {
    const int gs = num_experts / num_groups;
    unsigned long long gkey = 0ull;
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      stage[lane + 64 * j] = (uint32_t)(key[j] >> 32);
    // (one wave writes and reads: its LDS operations complete in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int shift = 31 - __clz(64 / num_groups);
    const int g = lane >> shift, per = 1 << shift;
    uint32_t a = 0u, b = 0u;  // the two largest images seen, a >= b
    if (g < num_groups)
      for (int i = lane & (per - 1); i < gs; i += per) {
        const uint32_t img = stage[g * gs + i];
        b = img > a ? a : (img > b ? img : b);
        a = img > a ? img : a;
      }
    for (int d = 1; d < per; d <<= 1) {
      const uint32_t oa = __shfl_xor(a, d, 64), ob = __shfl_xor(b, d, 64);
      const uint32_t low = oa < a ? oa : a, high = ob > b ? ob : b;
      a = oa > a ? oa : a;
      b = low > high ? low : high;
    }
    if (g < num_groups && lane == g << shift) {
      const float score =
          gs > 1 ? image_value(a) + image_value(b) : image_value(a);
      gkey = ((unsigned long long)order_image(score) << 32) | (uint32_t)~g;
    }
    unsigned keep = 0u;  // bit j: expert lane + 64 j is eligible
    for (int r = 0; r < topk_groups; ++r) {
      // (topk_groups <= num_groups: a live group key remains)
      const int best = (int)~(uint32_t)wave_max(gkey);
      if (lane == best << shift) gkey = 0ull;
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if ((unsigned)(lane + 64 * j - best * gs) < (unsigned)gs)
          keep |= 1u << j;
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (!((keep >> j) & 1u)) key[j] = 0ull;
  }
  float my_s = 0.0f;
  int my_id = 0;
  for (int r = 0; r < top_k; ++r) {
    unsigned long long best = key[0];
#pragma unroll
    for (int j = 1; j < kPer; ++j) best = key[j] > best ? key[j] : best;
    best = wave_max(best);
    // (top_k <= topk_groups * gs: a live key remains, so idx is in [0, E))
    const int idx = (int)~(uint32_t)best;
    float mine = 0.0f;
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (idx == lane + 64 * j) {
        mine = s[j];
        key[j] = 0ull;
      }
    const float sel = __shfl(mine, idx & 63, 64);
    if (lane == r) {
      my_id = idx;
      my_s = sel;
    }
  }
  float p = my_s;  // (0 in the lanes from top_k on)
  if (normalize) p = p / wave_sum(p);
  p *= scale;
  if (lane < top_k) {
    top_experts[t * top_k + lane] = my_id;
    weights[t * top_k + lane] = (W)p;
  }
  if (scores != nullptr) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int e = lane + 64 * j;
      if (e < num_experts) scores[t * num_experts + e] = (W)s[j];
    }
  }
}

template <typename T, typename W, int kPer>
__global__ void __launch_bounds__(kThreads)
    router_score_topk_kernel(const T *__restrict__ logits,
                             const float *__restrict__ bias,
                             int *__restrict__ top_experts,
                             W *__restrict__ weights, W *__restrict__ scores,
                             int tokens, int num_experts, int top_k,
                             int num_groups, int topk_groups, int normalize,
                             float scale) {
  __shared__ uint32_t stage[kWaves][kPer * 64];
  const int wave = wave_index();
  const long long t = (long long)blockIdx.x * kWaves + wave;
  if (t >= tokens) return;
  router_score_token<T, W, kPer>(logits, bias, top_experts, weights, scores, t,
                                 num_experts, top_k, num_groups, topk_groups,
                                 normalize, scale, threadIdx.x & 63,
                                 stage[wave]);
}

// RouterScoreTopKGrad: the layout of router_topk_grad_kernel, without a
// softmax (no row maximum, no dot product): ds = dscores (or 0) plus the
// picks' terms, dlogits = ds s (1 - s).
template <typename T, typename W, int kPer>
__global__ void __launch_bounds__(kThreads)
    router_score_grad_kernel(const T *__restrict__ logits,
                             const int *__restrict__ top_experts,
                             const W *__restrict__ dweights,
                             const W *__restrict__ dscores,
                             T *__restrict__ dlogits, int tokens,
                             int num_experts, int top_k, int normalize,
                             float scale) {
  const int lane = threadIdx.x & 63;
  const long long t = (long long)blockIdx.x * kWaves + wave_index();
  if (t >= tokens) return;
  const T *row = logits + t * num_experts;
  float s[kPer], ds[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int e = lane + 64 * j;
    const bool live = e < num_experts;
    s[j] = live ? sigmoid((float)row[e]) : 0.0f;
    ds[j] = live && dscores != nullptr
                ? (float)dscores[t * num_experts + e] : 0.0f;
  }
  // Lane r < top_k holds pick r: its id (-1 when out of range) and its
  // incoming gradient.
  int id = -1;
  float g = 0.0f;
  if (lane < top_k) {
    const int raw = top_experts[t * top_k + lane];
    if (raw >= 0 && raw < num_experts) {
      id = raw;
      g = (float)dweights[t * top_k + lane];
    }
  }
  if (normalize) {
    const float ssel = id >= 0 ? sigmoid((float)row[id]) : 0.0f;
    const float total = wave_sum(ssel);             // S
    const float c = wave_sum(g * ssel) / total;     // sum_j dw_j s_j / S
    g = id >= 0 ? scale * (g - c) / total : 0.0f;
  } else {
    g *= scale;
  }
  for (int r = 0; r < top_k; ++r) {
    const int rid = __shfl(id, r, 64);
    const float rg = __shfl(g, r, 64);
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (rid == lane + 64 * j) ds[j] += rg;
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int e = lane + 64 * j;
    if (e < num_experts)
      dlogits[t * num_experts + e] = (T)(ds[j] * s[j] * (1.0f - s[j]));
  }
}

// ---- sort -------------------------------------------------------------------

// The counter column of an id: itself, or num_experts when out of range.
__device__ __forceinline__ int sort_column(int id, int num_experts) {
  return id >= 0 && id < num_experts ? id : num_experts;
}

__global__ void __launch_bounds__(kSortThreads)
    moe_sort_histogram_kernel(const int *__restrict__ top_experts, int n,
                              int num_experts, int *__restrict__ counts) {
  __shared__ int hist[kMaxExperts + 1];
  const int tid = threadIdx.x;
  const int cols = num_experts + 1;
  for (int e = tid; e < cols; e += kSortThreads) hist[e] = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * kChunk + tid;
  if (i < n) atomicAdd(&hist[sort_column(top_experts[i], num_experts)], 1);
  __syncthreads();
  int *out = counts + (long long)blockIdx.x * cols;
  for (int e = tid; e < cols; e += kSortThreads) out[e] = hist[e];
}

// One workgroup. With at most 1024 columns the threads split into `parts`
// groups of `cols` threads, each group walking its share of the chunks.
__global__ void __launch_bounds__(kSortThreads)
    moe_sort_scan_kernel(int *__restrict__ counts, int chunks, int num_experts,
                         int *__restrict__ bins,
                         int *__restrict__ tokens_per_expert,
                         int *__restrict__ padded_bins) {
  __shared__ int part_sum[kMaxExperts + 1];  // [parts][cols]
  __shared__ int first[kMaxExperts + 1];     // totals, then first positions
  __shared__ int run[kSortThreads], padded_run[kSortThreads];
  const int tid = threadIdx.x;
  const int cols = num_experts + 1;
  const int parts = cols <= kSortThreads ? kSortThreads / cols : 1;
  const int per_part = (chunks + parts - 1) / parts;
  for (int slot = tid; slot < parts * cols; slot += kSortThreads) {
    const int e = slot % cols, part = slot / cols;
    const int c0 = min(part * per_part, chunks);
    const int c1 = min(c0 + per_part, chunks);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += counts[(long long)c * cols + e];
    part_sum[slot] = sum;
  }
  __syncthreads();
  for (int e = tid; e < cols; e += kSortThreads) {
    int sum = 0;
    for (int part = 0; part < parts; ++part) sum += part_sum[part * cols + e];
    first[e] = sum;
  }
  __syncthreads();
  // Inclusive scans over the experts of the counts and of the counts rounded
  // up to 128 (num_experts <= 1024 = one per thread).
  const int count = tid < num_experts ? first[tid] : 0;
  run[tid] = count;
  padded_run[tid] = (count + 127) & ~127;
  __syncthreads();
  for (int stride = 1; stride < kSortThreads; stride <<= 1) {
    const int a = tid >= stride ? run[tid - stride] : 0;
    const int b = tid >= stride ? padded_run[tid - stride] : 0;
    __syncthreads();
    run[tid] += a;
    padded_run[tid] += b;
    __syncthreads();
  }
  if (tid < num_experts) {
    bins[tid] = run[tid];
    tokens_per_expert[tid] = count;
    padded_bins[tid] = padded_run[tid];
    first[tid] = run[tid] - count;
  }
  // (the ids out of range follow the last bin)
  if (tid == 0) first[num_experts] = run[num_experts - 1];
  __syncthreads();
  for (int slot = tid; slot < parts * cols; slot += kSortThreads) {
    const int e = slot % cols, part = slot / cols;
    const int c0 = min(part * per_part, chunks);
    const int c1 = min(c0 + per_part, chunks);
    int pos = first[e];
    for (int q = 0; q < part; ++q) pos += part_sum[q * cols + e];
    for (int c = c0; c < c1; ++c) {
      const long long at = (long long)c * cols + e;
      const int here = counts[at];
      counts[at] = pos;
      pos += here;
    }
  }
}

__global__ void __launch_bounds__(kSortThreads)
    moe_sort_place_kernel(const int *__restrict__ top_experts,
                          const int *__restrict__ first_pos,
                          const int *__restrict__ bins,
                          const int *__restrict__ padded_bins, int n,
                          int num_experts, int rows, int *__restrict__ indices,
                          int *__restrict__ bin_ids, int *__restrict__ row_of) {
  __shared__ int next[kMaxExperts + 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = wave_index();
  const int cols = num_experts + 1;
  const int *mine = first_pos + (long long)blockIdx.x * cols;
  for (int e = tid; e < cols; e += kSortThreads) next[e] = mine[e];
  const long long i = (long long)blockIdx.x * kChunk + tid;
  const bool active = i < n;
  const int col = active ? sort_column(top_experts[i], num_experts) : 0;
  // Rank among the wave's equal columns, by lane.
  int rank = 0, same = 0;
  bool pending = active;
  while (true) {
    const unsigned long long todo = __ballot(pending);
    if (todo == 0ull) break;
    const int leader = __ffsll((long long)todo) - 1;
    const int lead_col = __shfl(col, leader, 64);
    const bool match = pending && col == lead_col;
    const unsigned long long mask = __ballot(match);
    if (match) {
      rank = __popcll(mask & ((1ull << lane) - 1ull));
      same = __popcll(mask);
      pending = false;
    }
  }
  __syncthreads();
  // The waves take their turns in wave order; within a wave the reads of
  // next[] precede the leaders' updates (program order, one wave).
  int base = 0;
  for (int w = 0; w < kSortThreads / 64; ++w) {
    if (w == wave && active) {
      base = next[col];
      __builtin_amdgcn_wave_barrier();
      if (rank == 0) next[col] = base + same;
    }
    __syncthreads();
  }
  if (!active) return;
  const int pos = base + rank;
  if (pos < 0 || pos >= n) return;  // (cannot happen for a consistent input)
  int row = -1;
  if (col < num_experts) {
    const int bin0 = col ? bins[col - 1] : 0;
    const int pad0 = col ? padded_bins[col - 1] : 0;
    const long long r = (long long)pad0 + (pos - bin0);
    if (pos >= bin0 && r >= 0 && r < rows) row = (int)r;
  }
  indices[pos] = (int)i;
  bin_ids[pos] = col;
  row_of[i] = row;
}

// ---- host: sputnik/block/router.h ---------------------------------------------

using Buffers = std::initializer_list<const void *>;

// No output is one of the inputs or another output (null: absent).
bool Distinct(Buffers outs, Buffers ins) {
  for (auto a = outs.begin(); a != outs.end(); ++a) {
    if (*a == nullptr) continue;
    for (auto b = a + 1; b != outs.end(); ++b)
      if (*a == *b) return false;
    for (const void *in : ins)
      if (*a == in) return false;
  }
  return true;
}

// What the four router calls check first: the sizes and types and, unless
// there are no tokens, that every required buffer is there.
bool RouterArgsOk(int tokens, int num_experts, int top_k,
                  sputnik::block::RouterType logits_type,
                  sputnik::block::WeightType weights_type, Buffers required) {
  const int l = (int)logits_type, w = (int)weights_type;
  if (tokens < 0 || num_experts < 1 || num_experts > kMaxExperts ||
      top_k < 1 || top_k > kMaxTopK || top_k > num_experts || l < 0 ||
      l > 2 || (w != 0 && w != 1))
    return false;
  for (const void *p : required)
    if (tokens > 0 && p == nullptr) return false;
  return true;
}

// The arguments converted to the kernel's parameter types (void pointers to
// its T and W pointers).
template <typename... P, typename... A>
void Enqueue(void (*kernel)(P...), unsigned grid, hipStream_t stream,
             A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, stream,
                     (P)args...);
}

// Enqueues pick(T{}, W{}, kPer), the call's kernel for its types and expert
// count, over `grid` workgroups.
template <typename Pick, typename... A>
hipError_t LaunchRouter(sputnik::block::RouterType logits_type,
                        sputnik::block::WeightType weights_type,
                        int num_experts, unsigned grid, hipStream_t stream,
                        Pick pick, A... args) {
  auto with_per = [&](auto t, auto w) {
    const int per = (num_experts + 63) / 64;
    if (per <= 1)
      Enqueue(pick(t, w, std::integral_constant<int, 1>{}), grid, stream,
              args...);
    else if (per <= 2)
      Enqueue(pick(t, w, std::integral_constant<int, 2>{}), grid, stream,
              args...);
    else if (per <= 4)
      Enqueue(pick(t, w, std::integral_constant<int, 4>{}), grid, stream,
              args...);
    else if (per <= 8)
      Enqueue(pick(t, w, std::integral_constant<int, 8>{}), grid, stream,
              args...);
    else
      Enqueue(pick(t, w, std::integral_constant<int, 16>{}), grid, stream,
              args...);
  };
  const bool f32 = weights_type == sputnik::block::WeightType::kF32;
  if (logits_type == sputnik::block::RouterType::kF32)
    with_per(float{}, float{});
  else if (logits_type == sputnik::block::RouterType::kBF16)
    f32 ? with_per(__bf16{}, float{}) : with_per(__bf16{}, __bf16{});
  else
    f32 ? with_per(_Float16{}, float{}) : with_per(_Float16{}, _Float16{});
  return hipGetLastError();
}

unsigned TokenGrid(int tokens) {
  return (unsigned)(((long long)tokens + kWaves - 1) / kWaves);
}

}  // namespace
}  // namespace sputnik_amd

namespace sputnik {
namespace block {

using namespace sputnik_amd;  // NOLINT: the kernels and helpers above

hipError_t RouterTopK(const void *logits, int *top_experts, void *weights,
                      void *scores, int tokens, int num_experts, int top_k,
                      bool normalize, RouterType logits_type,
                      WeightType weights_type, hipStream_t stream) {
  if (!RouterArgsOk(tokens, num_experts, top_k, logits_type, weights_type,
                    {logits, top_experts, weights}))
    return hipErrorInvalidValue;
  if (tokens == 0) return hipSuccess;
  if (!Distinct({top_experts, weights, scores}, {logits}))
    return hipErrorInvalidValue;
  return LaunchRouter(
      logits_type, weights_type, num_experts, TokenGrid(tokens), stream,
      [](auto t, auto w, auto per) {
        return router_topk_kernel<decltype(t), decltype(w),
                                  decltype(per)::value>;
      },
      logits, top_experts, weights, scores, tokens, num_experts, top_k,
      normalize ? 1 : 0);
}

size_t RouterAuxWorkspaceBytes(int tokens, int num_experts) {
  if (tokens < 0 || num_experts < 1 || num_experts > kMaxExperts) return 0;
  const size_t groups = ((size_t)tokens + kAuxTokens - 1) / kAuxTokens;
  return groups * (size_t)(num_experts + 1) * sizeof(float);
}

hipError_t RouterTopKAux(const void *logits, int *top_experts, void *weights,
                         void *scores, float *score_sums, float *z_sum,
                         int tokens, int num_experts, int top_k,
                         bool normalize, RouterType logits_type,
                         WeightType weights_type, void *workspace,
                         size_t workspace_bytes, hipStream_t stream) {
  if (!RouterArgsOk(tokens, num_experts, top_k, logits_type, weights_type,
                    {logits, top_experts, weights, workspace}))
    return hipErrorInvalidValue;
  // (the sums are written even for no tokens)
  if (score_sums == nullptr ||
      !Distinct({top_experts, weights, scores, score_sums, z_sum, workspace},
                {logits}))
    return hipErrorInvalidValue;
  if (tokens > 0 &&
      (workspace_bytes < RouterAuxWorkspaceBytes(tokens, num_experts) ||
       reinterpret_cast<uintptr_t>(workspace) % alignof(float) != 0))
    return hipErrorInvalidValue;
  float *partial = static_cast<float *>(workspace);
  const unsigned groups =
      (unsigned)(((long long)tokens + kAuxTokens - 1) / kAuxTokens);
  if (groups > 0) {
    const hipError_t e = LaunchRouter(
        logits_type, weights_type, num_experts, groups, stream,
        [](auto t, auto w, auto per) {
          return router_topk_aux_kernel<decltype(t), decltype(w),
                                        decltype(per)::value>;
        },
        logits, top_experts, weights, scores, partial, tokens, num_experts,
        top_k, normalize ? 1 : 0);
    if (e != hipSuccess) return e;
  }
  // (no tokens: no groups, and the sums are written as zeros)
  hipLaunchKernelGGL(router_aux_reduce_kernel,
                     dim3((num_experts + 1 + kThreads - 1) / kThreads),
                     dim3(kThreads), 0, stream, partial, (int)groups,
                     num_experts, score_sums, z_sum);
  return hipGetLastError();
}

// Neither statistic's gradient: the kStats = false instantiation, which is
// RouterTopKGrad's, so the result is its bit for bit by construction.
hipError_t RouterTopKAuxGrad(const void *logits, const int *top_experts,
                             const void *dweights, const void *dscores,
                             const float *dscore_sums, const float *dz_sum,
                             void *dlogits, int tokens, int num_experts,
                             int top_k, bool normalize, RouterType logits_type,
                             WeightType weights_type, hipStream_t stream) {
  if (!RouterArgsOk(tokens, num_experts, top_k, logits_type, weights_type,
                    {logits, top_experts, dweights, dlogits}))
    return hipErrorInvalidValue;
  if (tokens == 0) return hipSuccess;
  if (!Distinct({dlogits}, {logits, top_experts, dweights, dscores,
                            dscore_sums, dz_sum}))
    return hipErrorInvalidValue;
  const bool stats = dscore_sums != nullptr || dz_sum != nullptr;
  return LaunchRouter(
      logits_type, weights_type, num_experts, TokenGrid(tokens), stream,
      [stats](auto t, auto w, auto per) {
        using T = decltype(t);
        using W = decltype(w);
        constexpr int kPer = decltype(per)::value;
        return stats ? router_topk_grad_kernel<T, W, kPer, true>
                     : router_topk_grad_kernel<T, W, kPer, false>;
      },
      logits, top_experts, dweights, dscores, dscore_sums, dz_sum, dlogits,
      tokens, num_experts, top_k, normalize ? 1 : 0);
}

hipError_t RouterTopKGrad(const void *logits, const int *top_experts,
                          const void *dweights, const void *dscores,
                          void *dlogits, int tokens, int num_experts,
                          int top_k, bool normalize, RouterType logits_type,
                          WeightType weights_type, hipStream_t stream) {
  return RouterTopKAuxGrad(logits, top_experts, dweights, dscores, nullptr,
                           nullptr, dlogits, tokens, num_experts, top_k,
                           normalize, logits_type, weights_type, stream);
}

hipError_t RouterScoreTopK(const void *logits, const float *bias,
                           int *top_experts, void *weights, void *scores,
                           int tokens, int num_experts, int top_k,
                           int num_groups, int topk_groups, bool normalize,
                           float scale, RouterType logits_type,
                           WeightType weights_type, hipStream_t stream) {
  if (!RouterArgsOk(tokens, num_experts, top_k, logits_type, weights_type,
                    {logits, top_experts, weights}))
    return hipErrorInvalidValue;
  if (num_groups < 1 || num_groups > kMaxGroups || topk_groups < 1 ||
      topk_groups > num_groups || num_experts % num_groups != 0 ||
      top_k > topk_groups * (num_experts / num_groups) ||
      !(fabsf(scale) <= FLT_MAX))
    return hipErrorInvalidValue;
  if (tokens == 0) return hipSuccess;
  if (!Distinct({top_experts, weights, scores}, {logits, bias}))
    return hipErrorInvalidValue;
  return LaunchRouter(
      logits_type, weights_type, num_experts, TokenGrid(tokens), stream,
      [](auto t, auto w, auto per) {
        return router_score_topk_kernel<decltype(t), decltype(w),
                                        decltype(per)::value>;
      },
      logits, bias, top_experts, weights, scores, tokens, num_experts, top_k,
      num_groups, topk_groups, normalize ? 1 : 0, scale);
}

hipError_t RouterScoreTopKGrad(const void *logits, const int *top_experts,
                               const void *dweights, const void *dscores,
                               void *dlogits, int tokens, int num_experts,
                               int top_k, bool normalize, float scale,
                               RouterType logits_type,
                               WeightType weights_type, hipStream_t stream) {
  if (!RouterArgsOk(tokens, num_experts, top_k, logits_type, weights_type,
                    {logits, top_experts, dweights, dlogits}) ||
      !(fabsf(scale) <= FLT_MAX))
    return hipErrorInvalidValue;
  if (tokens == 0) return hipSuccess;
  if (!Distinct({dlogits}, {logits, top_experts, dweights, dscores}))
    return hipErrorInvalidValue;
  return LaunchRouter(
      logits_type, weights_type, num_experts, TokenGrid(tokens), stream,
      [](auto t, auto w, auto per) {
        return router_score_grad_kernel<decltype(t), decltype(w),
                                        decltype(per)::value>;
      },
      logits, top_experts, dweights, dscores, dlogits, tokens, num_experts,
      top_k, normalize ? 1 : 0, scale);
}

size_t MoeSortWorkspaceBytes(int n, int num_experts) {
  if (n < 0 || num_experts < 1 || num_experts > kMaxExperts ||
      (long long)n + 127LL * num_experts > INT_MAX)
    return 0;
  const size_t chunks = ((size_t)n + kChunk - 1) / kChunk;
  return chunks * (size_t)(num_experts + 1) * sizeof(int);
}

hipError_t MoeSort(const int *top_experts, int n, int num_experts, int rows,
                   int *indices, int *bin_ids, int *bins,
                   int *tokens_per_expert, int *padded_bins, int *row_of,
                   void *workspace, size_t workspace_bytes,
                   hipStream_t stream) {
  if (n < 0 || num_experts < 1 || num_experts > kMaxExperts || rows < 0 ||
      rows % 128 != 0 || (long long)n + 127LL * num_experts > INT_MAX)
    return hipErrorInvalidValue;
  if (bins == nullptr || tokens_per_expert == nullptr ||
      padded_bins == nullptr)
    return hipErrorInvalidValue;
  const size_t need = MoeSortWorkspaceBytes(n, num_experts);
  if (n > 0 &&
      (top_experts == nullptr || indices == nullptr || bin_ids == nullptr ||
       row_of == nullptr || workspace == nullptr || workspace_bytes < need ||
       reinterpret_cast<uintptr_t>(workspace) % alignof(int) != 0))
    return hipErrorInvalidValue;
  if (!Distinct({indices, bin_ids, bins, tokens_per_expert, padded_bins,
                 row_of, workspace}, {top_experts}))
    return hipErrorInvalidValue;
  int *counts = static_cast<int *>(workspace);
  const int chunks = (int)(((long long)n + kChunk - 1) / kChunk);
  if (chunks > 0) {
    hipLaunchKernelGGL(moe_sort_histogram_kernel, dim3(chunks),
                       dim3(kSortThreads), 0, stream, top_experts, n,
                       num_experts, counts);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(moe_sort_scan_kernel, dim3(1), dim3(kSortThreads), 0,
                     stream, counts, chunks, num_experts, bins,
                     tokens_per_expert, padded_bins);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (chunks > 0) {
    hipLaunchKernelGGL(moe_sort_place_kernel, dim3(chunks),
                       dim3(kSortThreads), 0, stream, top_experts, counts,
                       bins, padded_bins, n, num_experts, rows, indices,
                       bin_ids, row_of);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace block
}  // namespace sputnik
