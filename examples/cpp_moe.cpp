// A C++ caller of the MoE token permutation (sputnik/block/moe.h), the calls
// a dropless MoE layer makes around its expert MLP:
//   route     MoeBins + MoeRowMap from the sorted expert ids
//   forward   X_padded = PaddedGather(X); Y = PaddedScatter(X_padded, w)
//   backward  dw = PaddedScatterWeightGrad(dY, X_padded)
// The padded matrix is sized by the worst case (n + 127 E rounded up to 128),
// so nothing is read back before the launches. Activations are small
// integers and the router weights powers of two, so every sum is exact in
// fp16 and every result is checked bit for bit against host loops, the +0
// padding rows included (the output starts as NaN). Built against
// libsputnik.so by sputnik_amd/Makefile; tests/test_cpp_moe.py runs it on
// the GPU. Exit status 0 = all passed.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
std::vector<T> FromDevice(const T *d, size_t n) {
  std::vector<T> h(n);
  CHECK_HIP(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

std::vector<__half> ToHalf(const std::vector<float> &x) {
  std::vector<__half> h(x.size());
  for (size_t i = 0; i < x.size(); ++i) h[i] = __float2half(x[i]);
  return h;
}

unsigned short Bits(__half h) {
  unsigned short b;
  std::memcpy(&b, &h, sizeof(b));
  return b;
}

}  // namespace

int main() {
  const int tokens = 200, hidden = 72, top_k = 2, experts = 4;
  const int n = tokens * top_k;
  const int rows = (n + 127 * experts + 127) / 128 * 128;  // the worst case
  std::mt19937 gen(7);
  std::uniform_int_distribution<int> expert(0, experts - 2);  // last: empty
  std::uniform_int_distribution<int> small(-3, 3);

  // The router's choice and its stable sort (a caller's own sort).
  std::vector<int> top(n), indices(n), bin_ids(n);
  for (auto &e : top) e = expert(gen);
  std::iota(indices.begin(), indices.end(), 0);
  std::stable_sort(indices.begin(), indices.end(),
                   [&](int a, int b) { return top[a] < top[b]; });
  for (int i = 0; i < n; ++i) bin_ids[i] = top[indices[i]];

  std::vector<float> x((size_t)tokens * hidden), dy((size_t)tokens * hidden);
  for (auto *v : {&x, &dy})
    for (auto &e : *v) e = (float)small(gen);
  std::vector<float> w(n);
  for (int a = 0; a < n; ++a) w[a] = a % 2 ? 0.25f : 0.5f;

  int *d_indices = ToDevice(indices), *d_bin_ids = ToDevice(bin_ids);
  __half *d_x = ToDevice(ToHalf(x)), *d_dy = ToDevice(ToHalf(dy));
  float *d_w = ToDevice(w), *d_dw;
  int *d_bins, *d_tpe, *d_padded, *d_row_of;
  __half *d_xp, *d_y;
  CHECK_HIP(hipMalloc(&d_bins, experts * sizeof(int)));
  CHECK_HIP(hipMalloc(&d_tpe, experts * sizeof(int)));
  CHECK_HIP(hipMalloc(&d_padded, experts * sizeof(int)));
  CHECK_HIP(hipMalloc(&d_row_of, n * sizeof(int)));
  CHECK_HIP(hipMalloc(&d_dw, n * sizeof(float)));
  CHECK_HIP(hipMalloc(&d_xp, (size_t)rows * hidden * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_y, (size_t)tokens * hidden * sizeof(__half)));
  CHECK_HIP(hipMemset(d_xp, 0xff, (size_t)rows * hidden * sizeof(__half)));

  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  bool ok = true;

  // ---- route, gather, weighted scatter, weight gradient: one stream --------
  CHECK_HIP(sb::MoeBins(d_bin_ids, n, experts, d_bins, d_tpe, d_padded,
                        stream));
  CHECK_HIP(sb::MoeRowMap(d_indices, d_bin_ids, d_bins, d_padded, n, experts,
                          rows, d_row_of, stream));
  CHECK_HIP(sb::PaddedGather(d_x, d_indices, d_bins, d_padded, nullptr, d_xp,
                             tokens, hidden, top_k, experts, rows,
                             sb::DataType::kF16, sb::WeightType::kOperand,
                             stream));
  CHECK_HIP(sb::PaddedScatter(d_xp, d_row_of, d_w, d_y, tokens, hidden, top_k,
                              rows, sb::DataType::kF16, sb::WeightType::kF32,
                              stream));
  CHECK_HIP(sb::PaddedScatterWeightGrad(d_dy, d_xp, d_row_of, d_dw, tokens,
                                        hidden, top_k, rows,
                                        sb::DataType::kF16,
                                        sb::WeightType::kF32, stream));
  CHECK_HIP(hipStreamSynchronize(stream));

  // Host route.
  std::vector<int> bins(experts), tpe(experts, 0), padded(experts), row_of(n);
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
  ok &= Expect(FromDevice(d_bins, experts) == bins, "bins");
  ok &= Expect(FromDevice(d_tpe, experts) == tpe, "tokens_per_expert");
  ok &= Expect(FromDevice(d_padded, experts) == padded, "padded_bins");
  ok &= Expect(FromDevice(d_row_of, n) == row_of, "row_of");

  {
    std::vector<__half> ref((size_t)rows * hidden, __float2half(0.f));
    const std::vector<__half> xh = ToHalf(x);
    for (int a = 0; a < n; ++a)
      std::copy_n(&xh[(size_t)(a / top_k) * hidden], hidden,
                  &ref[(size_t)row_of[a] * hidden]);
    const std::vector<__half> got = FromDevice(d_xp, ref.size());
    size_t bad = 0;
    for (size_t i = 0; i < ref.size(); ++i) bad += Bits(got[i]) != Bits(ref[i]);
    ok &= Expect(bad == 0, "padded gather: bit exact, +0 padding rows");
  }
  {
    // Each copy of x[t] comes back times 0.5 and 0.25: y = 0.75 x, exact.
    const std::vector<__half> got = FromDevice(d_y, (size_t)tokens * hidden);
    size_t bad = 0;
    for (size_t i = 0; i < got.size(); ++i)
      bad += __half2float(got[i]) != 0.75f * x[i];
    ok &= Expect(bad == 0, "weighted scatter (fp32 weights): exact");
  }
  {
    const std::vector<float> got = FromDevice(d_dw, n);
    size_t bad = 0;
    for (int a = 0; a < n; ++a) {
      float s = 0.f;  // small integers: exact in any order
      for (int h = 0; h < hidden; ++h)
        s += dy[(size_t)(a / top_k) * hidden + h] *
             x[(size_t)(a / top_k) * hidden + h];
      bad += got[a] != s;
    }
    ok &= Expect(bad == 0, "weight gradient: exact");
  }

  // ---- rejected, never aborted ----------------------------------------------
  ok &= Expect(sb::PaddedGather(d_x, d_indices, d_bins, d_padded, nullptr,
                                d_xp, tokens, hidden, top_k, experts,
                                rows - 1, sb::DataType::kF16,
                                sb::WeightType::kOperand, stream) ==
                   hipErrorInvalidValue,
               "rows % 128 != 0: hipErrorInvalidValue");
  ok &= Expect(sb::PaddedScatter(d_xp, d_row_of, nullptr, d_xp, tokens, hidden,
                                 top_k, rows, sb::DataType::kF16,
                                 sb::WeightType::kOperand, stream) ==
                   hipErrorInvalidValue,
               "out == y: hipErrorInvalidValue");

  for (void *p : {(void *)d_indices, (void *)d_bin_ids, (void *)d_x,
                  (void *)d_dy, (void *)d_w, (void *)d_dw, (void *)d_bins,
                  (void *)d_tpe, (void *)d_padded, (void *)d_row_of,
                  (void *)d_xp, (void *)d_y})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(stream));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
