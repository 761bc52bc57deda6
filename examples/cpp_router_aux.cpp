// A C++ caller of the router with the auxiliary-loss statistics
// (sputnik/block/router.h):
//   RouterTopKAux      fp32 logits [200, 5] -> the 2 picks per token, their
//                      weights, score_sums [5] = sum_t p_te and z_sum [1] =
//                      sum_t lse_t^2, into a workspace of 0xff bytes
//   RouterTopKAuxGrad  dlogits from dweights, dscore_sums and dz_sum
// Everything is checked on the host against double arithmetic: the ids
// exactly (and equal to RouterTopK's, like the weights, bit for bit),
//   score_sums  within (E + 64 + tokens) 2^-24 ref,
//   z_sum       within sum_t 2 |lse_t| d_t + (tokens + 2) 2^-24 ref,
//               d_t = (E + 64) 2^-24 + 2^-23 (|m_t| + |lse_t - m_t|),
//   dlogits     within 2^-24 |ref| + (2 E + 2 k + 128) 2^-24 image, image the
//               gradient with every term by its absolute value and
//               2 |dz| (|lse_t| + 1) p_tj for the z term.
// Built against libsputnik.so by sputnik_amd/Makefile;
// tests/test_cpp_router_aux.py runs it on the GPU. Exit status 0 = all passed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "sputnik/sputnik.h"

namespace sb = sputnik::block;

#define CHECK_HIP(x)                                                   \
  do {                                                                 \
    hipError_t e_ = (x);                                               \
    if (e_ != hipSuccess) {                                            \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__,           \
                   hipGetErrorString(e_));                             \
      std::exit(2);                                                    \
    }                                                                  \
  } while (0)

namespace {

bool Expect(bool cond, const char *what) {
  std::printf("%s: %s\n", what, cond ? "ok" : "FAIL");
  return cond;
}

template <typename T>
T *ToDevice(const std::vector<T> &h) {
  T *d = nullptr;
  CHECK_HIP(hipMalloc(&d, std::max<size_t>(h.size(), 1) * sizeof(T)));
  CHECK_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

template <typename T>
T *DeviceBuffer(size_t n) {
  T *d = nullptr;
  CHECK_HIP(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
  CHECK_HIP(hipMemset(d, 0xff, std::max<size_t>(n, 1) * sizeof(T)));
  return d;
}

template <typename T>
std::vector<T> FromDevice(const T *d, size_t n) {
  std::vector<T> h(n);
  CHECK_HIP(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

}  // namespace

int main() {
  const int tokens = 200, experts = 5, top_k = 2;
  const int n = tokens * top_k;
  const size_t cells = (size_t)tokens * experts;
  std::mt19937 gen(17);
  std::uniform_real_distribution<float> logit(-8.f, 8.f), grad(-2.f, 2.f);

  std::vector<float> logits(cells), dw(n), dsums(experts), dz(1);
  for (auto &l : logits) l = logit(gen);
  for (auto &g : dw) g = grad(gen);
  for (auto &g : dsums) g = grad(gen);
  dz[0] = 0.375f;

  float *d_logits = ToDevice(logits), *d_dw = ToDevice(dw);
  float *d_dsums = ToDevice(dsums), *d_dz = ToDevice(dz);
  int *d_top = DeviceBuffer<int>(n), *d_top_plain = DeviceBuffer<int>(n);
  float *d_w = DeviceBuffer<float>(n), *d_w_plain = DeviceBuffer<float>(n);
  float *d_sums = DeviceBuffer<float>(experts), *d_z = DeviceBuffer<float>(1);
  float *d_dlogits = DeviceBuffer<float>(cells);
  const size_t ws_bytes = sb::RouterAuxWorkspaceBytes(tokens, experts);
  // (the workspace starts as 0xff bytes: it needs no initialisation)
  char *d_ws = DeviceBuffer<char>(ws_bytes);

  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  bool ok = true;
  ok &= Expect(ws_bytes == (size_t)((tokens + sb::kRouterAuxTokens - 1) /
                                    sb::kRouterAuxTokens) *
                               (experts + 1) * sizeof(float),
               "workspace bytes");

  CHECK_HIP(sb::RouterTopKAux(d_logits, d_top, d_w, nullptr, d_sums, d_z,
                              tokens, experts, top_k, false,
                              sb::RouterType::kF32, sb::WeightType::kF32, d_ws,
                              ws_bytes, stream));
  CHECK_HIP(sb::RouterTopK(d_logits, d_top_plain, d_w_plain, nullptr, tokens,
                           experts, top_k, false, sb::RouterType::kF32,
                           sb::WeightType::kF32, stream));
  CHECK_HIP(sb::RouterTopKAuxGrad(d_logits, d_top, d_dw, nullptr, d_dsums, d_dz,
                                  d_dlogits, tokens, experts, top_k, false,
                                  sb::RouterType::kF32, sb::WeightType::kF32,
                                  stream));
  CHECK_HIP(hipStreamSynchronize(stream));

  // Host: the picks by a stable sort, everything else in double.
  const double unit = std::ldexp(1.0, -24);
  std::vector<int> top(n);
  std::vector<double> sums(experts, 0.0), ref(cells), image(cells);
  double z = 0, z_slack = 0;
  for (int t = 0; t < tokens; ++t) {
    const float *l = &logits[(size_t)t * experts];
    std::vector<int> order(experts);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return l[a] > l[b]; });
    const double m = l[order[0]];
    double sum = 0;
    for (int e = 0; e < experts; ++e) sum += std::exp((double)l[e] - m);
    const double lse = m + std::log(sum);
    z += lse * lse;
    z_slack += 2 * std::fabs(lse) *
               ((experts + 64) * unit +
                2 * unit * (std::fabs(m) + std::fabs(lse - m)));
    std::vector<double> p(experts), dp(experts), a(experts);
    for (int e = 0; e < experts; ++e) {
      p[e] = std::exp((double)l[e] - m) / sum;
      sums[e] += p[e];
      dp[e] = dsums[e];
      a[e] = std::fabs((double)dsums[e]);
    }
    for (int k = 0; k < top_k; ++k) {
      top[t * top_k + k] = order[k];
      dp[order[k]] += dw[t * top_k + k];
      a[order[k]] += std::fabs((double)dw[t * top_k + k]);
    }
    double dot = 0, adot = 0;
    for (int e = 0; e < experts; ++e) {
      dot += dp[e] * p[e];
      adot += a[e] * p[e];
    }
    for (int e = 0; e < experts; ++e) {
      ref[(size_t)t * experts + e] =
          p[e] * (dp[e] - dot) + 2 * (double)dz[0] * lse * p[e];
      image[(size_t)t * experts + e] =
          p[e] * (a[e] + adot) +
          2 * std::fabs((double)dz[0]) * (std::fabs(lse) + 1) * p[e];
    }
  }

  ok &= Expect(FromDevice(d_top, n) == top, "top_experts: exact");
  ok &= Expect(FromDevice(d_top_plain, n) == top, "RouterTopK's ids the same");
  ok &= Expect(FromDevice(d_w, n) == FromDevice(d_w_plain, n),
               "weights: RouterTopK's bit for bit");
  const std::vector<float> got_sums = FromDevice(d_sums, experts);
  bool sums_ok = true;
  double total = 0;
  for (int e = 0; e < experts; ++e) {
    sums_ok &= std::fabs(got_sums[e] - sums[e]) <=
               (experts + 64 + tokens) * unit * sums[e];
    total += got_sums[e];
  }
  ok &= Expect(sums_ok, "score_sums within bound");
  ok &= Expect(std::fabs(total - tokens) < 1e-3 * tokens,
               "score_sums add up to the token count");
  const float got_z = FromDevice(d_z, 1)[0];
  ok &= Expect(std::fabs(got_z - z) <= z_slack + (tokens + 2) * unit * z,
               "z_sum within bound");
  const std::vector<float> got = FromDevice(d_dlogits, cells);
  size_t bad = 0;
  for (size_t i = 0; i < cells; ++i)
    bad += !(std::fabs(got[i] - ref[i]) <=
             unit * std::fabs(ref[i]) +
                 (2 * experts + 2 * top_k + 128) * unit * image[i]);
  ok &= Expect(bad == 0, "dlogits within bound");

  // ---- rejected, never aborted ----------------------------------------------
  ok &= Expect(sb::RouterTopKAux(d_logits, d_top, d_w, nullptr, nullptr, d_z,
                                 tokens, experts, top_k, false,
                                 sb::RouterType::kF32, sb::WeightType::kF32,
                                 d_ws, ws_bytes, stream) ==
                   hipErrorInvalidValue,
               "no score_sums: hipErrorInvalidValue");
  ok &= Expect(sb::RouterTopKAux(d_logits, d_top, d_w, nullptr, d_sums, d_z,
                                 tokens, experts, top_k, false,
                                 sb::RouterType::kF32, sb::WeightType::kF32,
                                 d_ws, ws_bytes - 1, stream) ==
                   hipErrorInvalidValue,
               "workspace too small: hipErrorInvalidValue");
  ok &= Expect(sb::RouterTopKAuxGrad(d_logits, d_top, d_dw, nullptr, d_dlogits,
                                     d_dz, d_dlogits, tokens, experts, top_k,
                                     false, sb::RouterType::kF32,
                                     sb::WeightType::kF32, stream) ==
                   hipErrorInvalidValue,
               "dlogits == dscore_sums: hipErrorInvalidValue");

  for (void *p : {(void *)d_logits, (void *)d_dw, (void *)d_dsums, (void *)d_dz,
                  (void *)d_top, (void *)d_top_plain, (void *)d_w,
                  (void *)d_w_plain, (void *)d_sums, (void *)d_z,
                  (void *)d_dlogits, (void *)d_ws})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(stream));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
