// A C++ caller of the sigmoid-score router (sputnik/block/router.h):
//   RouterScoreTopK  fp32 logits [300, 16] and a selection bias -> the 3
//                    picks per token among the experts of the 2 best of 4
//                    groups, their weights (plain, and renormalised and
//                    scaled by 2.5) and the sigmoid scores
// The bias takes four values, so experts share one, and some rows are tied on
// purpose (all logits equal; the best two experts of a group equal; two groups
// with the same score): the picks must then be the lower indices. The other
// rows are redrawn until, in double precision, neighbouring selection values
// and group scores are 2^-14 apart, far above the fp32 error, so that the
// picks of a host loop in double are the only right answer. Ids are checked
// exactly, weights and scores against double precision within (1 + 14 + k)
// 2^-24 |ref|. Built against libsputnik.so by sputnik_amd/Makefile;
// tests/test_cpp_router_score.py runs it on the GPU. Exit status 0 = all
// passed.
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

constexpr int kTokens = 300, kExperts = 16, kTopK = 3, kGroups = 4,
              kTopGroups = 2, kGroupSize = kExperts / kGroups;

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

bool Within(const std::vector<float> &got, const std::vector<double> &ref,
            double rel) {
  size_t bad = 0;
  for (size_t i = 0; i < ref.size(); ++i)
    bad += !(std::fabs((double)got[i] - ref[i]) <= rel * std::fabs(ref[i]));
  return bad == 0;
}

// One row in double: the scores s, the picks (stable sorts: the larger value
// first, then the lower index) and whether every decision is either an exact
// tie or 2^-14 clear.
struct Row {
  double s[kExperts];
  int pick[kTopK];
  bool clear;
};

Row HostRow(const float *l, const std::vector<float> &bias) {
  Row r;
  double c[kExperts], score[kGroups];
  const double gap = std::ldexp(1.0, -14);
  auto apart = [&](double a, double b) { return a == b || a - b >= gap; };
  r.clear = true;
  for (int e = 0; e < kExperts; ++e) {
    r.s[e] = 1.0 / (1.0 + std::exp(-(double)l[e]));
    c[e] = r.s[e] + (double)bias[e];
  }
  for (int g = 0; g < kGroups; ++g) {
    std::vector<double> v(c + g * kGroupSize, c + (g + 1) * kGroupSize);
    std::sort(v.begin(), v.end(), [](double a, double b) { return a > b; });
    score[g] = v[0] + v[1];
    r.clear &= apart(v[0], v[1]) && apart(v[1], v[2]);
  }
  std::vector<int> groups(kGroups);
  std::iota(groups.begin(), groups.end(), 0);
  std::stable_sort(groups.begin(), groups.end(),
                   [&](int a, int b) { return score[a] > score[b]; });
  for (int i = 0; i + 1 < kGroups; ++i)
    r.clear &= apart(score[groups[i]], score[groups[i + 1]]);
  std::vector<int> order;
  for (int e = 0; e < kExperts; ++e)
    for (int i = 0; i < kTopGroups; ++i)
      if (e / kGroupSize == groups[i]) order.push_back(e);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return c[a] > c[b]; });
  for (int k = 0; k < kTopK; ++k) {
    r.pick[k] = order[k];
    r.clear &= apart(c[order[k]], c[order[k + 1]]);
  }
  return r;
}

}  // namespace

int main() {
  const int n = kTokens * kTopK;
  const float scale = 2.5f;
  std::mt19937 gen(23);
  std::uniform_real_distribution<float> logit(-6.f, 6.f);

  // (experts 0, 4, 8, 12 share a bias, and so on: one value per position in
  // the group)
  std::vector<float> bias(kExperts);
  for (int e = 0; e < kExperts; ++e) bias[e] = 0.125f * (float)((e + 2) % 4) - 0.25f;

  std::vector<float> logits((size_t)kTokens * kExperts);
  std::vector<Row> rows(kTokens);
  int redraws = 0;
  for (int t = 0; t < kTokens; ++t) {
    float *l = &logits[(size_t)t * kExperts];
    for (;; ++redraws) {
      for (int e = 0; e < kExperts; ++e) l[e] = logit(gen);
      if (t == 7)  // all tied: groups 0 and 1, then the larger biases
        for (int e = 0; e < kExperts; ++e) l[e] = 0.75f;
      if (t == 9) {  // experts 2 and 6 lead their groups, equal: 2, then 6
        for (int e = 0; e < kExperts; ++e) l[e] = -3.f - 0.125f * (float)e;
        l[2] = l[6] = 4.f;
      }
      if (t == 11)  // every group the same: groups 0 and 1 by index
        for (int e = 0; e < kExperts; ++e) l[e] = 0.5f * (float)(e % 4) - 1.f;
      rows[t] = HostRow(l, bias);
      if (rows[t].clear) break;
      if (t == 7 || t == 9 || t == 11 || redraws > 10000) {
        std::fprintf(stderr, "row %d is not clear\n", t);
        return 2;
      }
    }
  }
  std::printf("rows redrawn: %d\n", redraws);

  float *d_logits = ToDevice(logits), *d_bias = ToDevice(bias);
  int *d_top = DeviceBuffer<int>(n), *d_top_n = DeviceBuffer<int>(n);
  float *d_w = DeviceBuffer<float>(n), *d_wn = DeviceBuffer<float>(n);
  float *d_scores = DeviceBuffer<float>((size_t)kTokens * kExperts);
  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  bool ok = true;

  CHECK_HIP(sb::RouterScoreTopK(d_logits, d_bias, d_top, d_w, d_scores, kTokens,
                                kExperts, kTopK, kGroups, kTopGroups, false,
                                1.0f, sb::RouterType::kF32,
                                sb::WeightType::kF32, stream));
  CHECK_HIP(sb::RouterScoreTopK(d_logits, d_bias, d_top_n, d_wn, nullptr,
                                kTokens, kExperts, kTopK, kGroups, kTopGroups,
                                true, scale, sb::RouterType::kF32,
                                sb::WeightType::kOperand, stream));
  CHECK_HIP(hipStreamSynchronize(stream));

  std::vector<int> top(n);
  std::vector<double> w(n), wn(n), scores((size_t)kTokens * kExperts);
  for (int t = 0; t < kTokens; ++t) {
    double picked = 0;
    for (int e = 0; e < kExperts; ++e)
      scores[(size_t)t * kExperts + e] = rows[t].s[e];
    for (int k = 0; k < kTopK; ++k) {
      top[t * kTopK + k] = rows[t].pick[k];
      w[t * kTopK + k] = rows[t].s[rows[t].pick[k]];
      picked += w[t * kTopK + k];
    }
    for (int k = 0; k < kTopK; ++k)
      wn[t * kTopK + k] = w[t * kTopK + k] / picked * (double)scale;
  }
  auto picks = [&](int t, int a, int b, int c) {
    return top[t * kTopK] == a && top[t * kTopK + 1] == b &&
           top[t * kTopK + 2] == c;
  };
  ok &= Expect(picks(7, 1, 5, 0) && picks(9, 2, 6, 1) && picks(11, 1, 5, 3),
               "tied rows pick the lower indices (host)");
  ok &= Expect(FromDevice(d_top, n) == top, "top_experts: exact");
  ok &= Expect(FromDevice(d_top_n, n) == top, "top_experts (normalize): exact");
  const double unit = std::ldexp(1.0, -24);
  ok &= Expect(Within(FromDevice(d_w, n), w, unit * (1 + 14 + kTopK)),
               "weights within bound");
  ok &= Expect(Within(FromDevice(d_wn, n), wn, unit * (1 + 14 + kTopK)),
               "normalised, scaled weights within bound");
  ok &= Expect(Within(FromDevice(d_scores, (size_t)kTokens * kExperts), scores,
                      unit * (1 + 6)),
               "scores within bound");

  // ---- rejected, never aborted ----------------------------------------------
  auto rejected = [&](int top_k, int groups, int top_groups, float sc) {
    return sb::RouterScoreTopK(d_logits, d_bias, d_top, d_w, nullptr, kTokens,
                               kExperts, top_k, groups, top_groups, false, sc,
                               sb::RouterType::kF32, sb::WeightType::kF32,
                               stream) == hipErrorInvalidValue;
  };
  ok &= Expect(rejected(9, 4, 2, 1.f), "top_k > topk_groups * gs: rejected");
  ok &= Expect(rejected(3, 5, 2, 1.f), "E % num_groups != 0: rejected");
  ok &= Expect(rejected(3, 4, 5, 1.f), "topk_groups > num_groups: rejected");
  ok &= Expect(rejected(3, 4, 2, INFINITY), "scale not finite: rejected");

  for (void *p : {(void *)d_logits, (void *)d_bias, (void *)d_top,
                  (void *)d_top_n, (void *)d_w, (void *)d_wn,
                  (void *)d_scores})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(stream));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
