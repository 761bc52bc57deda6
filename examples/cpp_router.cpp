// A C++ caller of the MoE router (sputnik/block/router.h), the calls a
// dropless MoE layer makes between its router GEMM and the token permutation:
//   RouterTopK   fp32 logits [200, 5] -> the 2 picks per token, their softmax
//                weights (plain and renormalised) and the scores
//   MoeSort      the picks -> MegaBlocks' routing tensors, one call
// Some rows are tied on purpose (all logits equal; the top two equal): the
// picks must then be the lower expert indices. The ids and every routing
// tensor are checked exactly against host loops (a stable sort), the weights
// and scores against double precision within the header's bound
// (2^-24 + (E + k + 64) 2^-24) |ref|. Built against libsputnik.so by
// sputnik_amd/Makefile; tests/test_cpp_router.py runs it on the GPU. Exit
// status 0 = all passed.
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

bool Within(const std::vector<float> &got, const std::vector<double> &ref,
            double rel) {
  size_t bad = 0;
  for (size_t i = 0; i < ref.size(); ++i)
    bad += !(std::fabs((double)got[i] - ref[i]) <= rel * std::fabs(ref[i]));
  return bad == 0;
}

}  // namespace

int main() {
  const int tokens = 200, experts = 5, top_k = 2;
  const int n = tokens * top_k;
  const int rows = (n + 127 * experts + 127) / 128 * 128;  // the worst case
  std::mt19937 gen(11);
  std::uniform_real_distribution<float> logit(-8.f, 8.f);

  std::vector<float> logits((size_t)tokens * experts);
  for (auto &l : logits) l = logit(gen);
  for (int e = 0; e < experts; ++e) logits[7 * experts + e] = 1.5f;  // all tied
  logits[9 * experts + 1] = logits[9 * experts + 4] = 9.f;  // the top two tied
  logits[11 * experts + 0] = logits[11 * experts + 3] = -9.f;
  logits[11 * experts + 1] = logits[11 * experts + 2] =
      logits[11 * experts + 4] = -9.f;                       // again, negative

  float *d_logits = ToDevice(logits);
  int *d_top = DeviceBuffer<int>(n);
  float *d_w = DeviceBuffer<float>(n), *d_wn = DeviceBuffer<float>(n);
  float *d_scores = DeviceBuffer<float>((size_t)tokens * experts);
  int *d_top_n = DeviceBuffer<int>(n);
  int *d_indices = DeviceBuffer<int>(n), *d_bin_ids = DeviceBuffer<int>(n);
  int *d_row_of = DeviceBuffer<int>(n);
  int *d_bins = DeviceBuffer<int>(experts), *d_tpe = DeviceBuffer<int>(experts);
  int *d_padded = DeviceBuffer<int>(experts);
  const size_t ws_bytes = sb::MoeSortWorkspaceBytes(n, experts);
  // (the workspace starts as 0xff bytes: it needs no initialisation)
  char *d_ws = DeviceBuffer<char>(ws_bytes);

  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  bool ok = true;
  ok &= Expect(ws_bytes == (size_t)((n + sb::kMoeSortChunk - 1) /
                                    sb::kMoeSortChunk) *
                               (experts + 1) * sizeof(int),
               "workspace bytes");

  // ---- router, then sort: one stream, nothing read back in between ----------
  CHECK_HIP(sb::RouterTopK(d_logits, d_top, d_w, d_scores, tokens, experts,
                           top_k, false, sb::RouterType::kF32,
                           sb::WeightType::kF32, stream));
  CHECK_HIP(sb::RouterTopK(d_logits, d_top_n, d_wn, nullptr, tokens, experts,
                           top_k, true, sb::RouterType::kF32,
                           sb::WeightType::kOperand, stream));
  CHECK_HIP(sb::MoeSort(d_top, n, experts, rows, d_indices, d_bin_ids, d_bins,
                        d_tpe, d_padded, d_row_of, d_ws, ws_bytes, stream));
  CHECK_HIP(hipStreamSynchronize(stream));

  // Host router: a stable sort by descending logit; the softmax in double.
  std::vector<int> top(n);
  std::vector<double> w(n), wn(n), scores((size_t)tokens * experts);
  for (int t = 0; t < tokens; ++t) {
    const float *l = &logits[(size_t)t * experts];
    std::vector<int> order(experts);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return l[a] > l[b]; });
    const double m = l[order[0]];
    double sum = 0, picked = 0;
    for (int e = 0; e < experts; ++e) sum += std::exp((double)l[e] - m);
    for (int e = 0; e < experts; ++e)
      scores[(size_t)t * experts + e] = std::exp((double)l[e] - m) / sum;
    for (int k = 0; k < top_k; ++k) {
      top[t * top_k + k] = order[k];
      w[t * top_k + k] = scores[(size_t)t * experts + order[k]];
      picked += w[t * top_k + k];
    }
    for (int k = 0; k < top_k; ++k) wn[t * top_k + k] = w[t * top_k + k] / picked;
  }
  ok &= Expect(top[7 * top_k] == 0 && top[7 * top_k + 1] == 1 &&
                   top[9 * top_k] == 1 && top[9 * top_k + 1] == 4 &&
                   top[11 * top_k] == 0 && top[11 * top_k + 1] == 1,
               "tied rows pick the lower indices (host)");
  ok &= Expect(FromDevice(d_top, n) == top, "top_experts: exact");
  ok &= Expect(FromDevice(d_top_n, n) == top, "top_experts (normalize): exact");
  const double unit = std::ldexp(1.0, -24);
  ok &= Expect(Within(FromDevice(d_w, n), w, unit * (1 + experts + top_k + 64)),
               "weights within bound");
  ok &= Expect(Within(FromDevice(d_wn, n), wn,
                      unit * (1 + experts + top_k + 64)),
               "normalised weights within bound");
  ok &= Expect(Within(FromDevice(d_scores, (size_t)tokens * experts), scores,
                      unit * (1 + experts + 64)),
               "scores within bound");

  // Host route: a stable sort by expert.
  std::vector<int> indices(n), bin_ids(n), bins(experts), tpe(experts, 0),
      padded(experts), row_of(n);
  std::iota(indices.begin(), indices.end(), 0);
  std::stable_sort(indices.begin(), indices.end(),
                   [&](int a, int b) { return top[a] < top[b]; });
  for (int i = 0; i < n; ++i) bin_ids[i] = top[indices[i]];
  for (int e : top) ++tpe[e];
  for (int e = 0, run = 0, prun = 0; e < experts; ++e) {
    run += tpe[e];
    prun += (tpe[e] + 127) / 128 * 128;
    bins[e] = run;
    padded[e] = prun;
  }
  for (int i = 0; i < n; ++i) {
    const int e = bin_ids[i];
    row_of[indices[i]] =
        (e ? padded[e - 1] : 0) + (i - (e ? bins[e - 1] : 0));
  }
  ok &= Expect(FromDevice(d_indices, n) == indices, "indices");
  ok &= Expect(FromDevice(d_bin_ids, n) == bin_ids, "bin_ids");
  ok &= Expect(FromDevice(d_bins, experts) == bins, "bins");
  ok &= Expect(FromDevice(d_tpe, experts) == tpe, "tokens_per_expert");
  ok &= Expect(FromDevice(d_padded, experts) == padded, "padded_bins");
  ok &= Expect(FromDevice(d_row_of, n) == row_of, "row_of");

  // ---- rejected, never aborted ----------------------------------------------
  ok &= Expect(sb::RouterTopK(d_logits, d_top, d_w, nullptr, tokens, experts,
                              experts + 1, false, sb::RouterType::kF32,
                              sb::WeightType::kF32, stream) ==
                   hipErrorInvalidValue,
               "top_k > E: hipErrorInvalidValue");
  ok &= Expect(sb::MoeSort(d_top, n, experts, rows, d_indices, d_bin_ids,
                           d_bins, d_tpe, d_padded, d_row_of, d_ws,
                           ws_bytes - 1, stream) == hipErrorInvalidValue,
               "workspace too small: hipErrorInvalidValue");
  ok &= Expect(sb::MoeSort(d_top, n, experts, rows, d_top, d_bin_ids, d_bins,
                           d_tpe, d_padded, d_row_of, d_ws, ws_bytes,
                           stream) == hipErrorInvalidValue,
               "indices == top_experts: hipErrorInvalidValue");

  for (void *p : {(void *)d_logits, (void *)d_top, (void *)d_w, (void *)d_wn,
                  (void *)d_scores, (void *)d_top_n, (void *)d_indices,
                  (void *)d_bin_ids, (void *)d_row_of, (void *)d_bins,
                  (void *)d_tpe, (void *)d_padded, (void *)d_ws})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(stream));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
