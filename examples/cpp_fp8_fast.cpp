// A C++ caller of the fp8 products' opt-in fast accumulation
// (sputnik/block/fp8.h, Fp8Accumulate::kFast) and of Fp8IntervalSums, the
// interval sums P of the contract as a callable:
//   Xq = QuantizeRows(X), W1q = QuantizeWeight(W1),
//   P = Fp8IntervalSums(Xq, W1q) in both modes,
//   C = SddFp8(Xq, W1q, kFast), Y = DsdFp8(Sq, W1q, kFast) with Sq the blocks
//   of X quantised as a sparse operand
// on the known-answer data of examples/cpp_fp8.cpp with power-of-two scales:
// X is one-hot per row (row i holds one value, at a k that differs per row
// and covers every k), W1 holds distinct small integers in an asymmetric
// pattern times a power of two per block. Every dot product has one non-zero
// term, so the scaled MFMA's limited-precision sum is exact too, and P, C and
// Y are checked bit for bit against host loops: C[i][n] = X[i][k(i)]
// W1[k(i)][n] pins every (row, k, column) of the lane map of the fast
// instantiations. Built against libsputnik.so by sputnik_amd/Makefile;
// tests/test_cpp_fp8_fast.py runs it on the GPU. Exit status 0 = all passed.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

constexpr int kB = 128;

bool Expect(bool cond, const char *what) {
  std::printf("%s: %s\n", what, cond ? "ok" : "FAIL");
  return cond;
}

template <typename T>
T *ToDevice(const std::vector<T> &h) {
  T *d = nullptr;
  CHECK_HIP(hipMalloc(&d, h.size() * sizeof(T)));
  CHECK_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

template <typename T>
T *DeviceBuffer(size_t n, int fill) {
  T *d = nullptr;
  CHECK_HIP(hipMalloc(&d, n * sizeof(T)));
  CHECK_HIP(hipMemset(d, fill, n * sizeof(T)));
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

bool AllHalf(const __half *d, size_t n, uint16_t bits) {
  const std::vector<__half> h = FromDevice(d, n);
  for (const __half &v : h)
    if (*reinterpret_cast<const uint16_t *>(&v) != bits) return false;
  return true;
}

}  // namespace

int main() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) {
    std::fprintf(stderr, "no HIP device\n");
    return 2;
  }
  const int m = 256, k = 256, n = 384;
  const int mb = m / kB, kb = k / kB, nb = n / kB;
  bool ok = true;

  auto k_of = [&](int i) { return (i * 37 + 11) % k; };
  auto x_of = [&](int i) {
    return (i % 2 ? -1.0f : 1.0f) * (8 + i % 8) / 8.0f *
           std::ldexp(1.0f, i % 7 - 3);
  };
  std::vector<float> x((size_t)m * k, 0.0f);
  for (int i = 0; i < m; ++i) x[(size_t)i * k + k_of(i)] = x_of(i);
  auto w1_of = [&](int kk, int nn) {
    return (float)((kk * 7 + nn * 11) % 15 - 7) *
           std::ldexp(1.0f, (kk / kB + 2 * (nn / kB)) % 3);
  };
  std::vector<float> w1((size_t)k * n);
  for (int kk = 0; kk < k; ++kk)
    for (int nn = 0; nn < n; ++nn) w1[(size_t)kk * n + nn] = w1_of(kk, nn);

  // C's topology: 2 x 3 blocks, (1, 2) missing, column indices unordered.
  const std::vector<int> c_offsets = {0, 3, 5};
  const std::vector<short> c_indices = {2, 0, 1, 1, 0};
  const std::vector<short> c_rows = {0, 0, 0, 1, 1};
  const int c_blocks = (int)c_indices.size();
  // X as a sparse operand: every block stored, the second block row out of
  // k order.
  const std::vector<int> s_offsets = {0, 2, 4};
  const std::vector<short> s_indices = {0, 1, 1, 0};
  const int s_blocks = (int)s_indices.size();
  std::vector<float> xs_blocks((size_t)s_blocks * kB * kB);
  for (int b = 0; b < s_blocks; ++b)
    for (int a = 0; a < kB; ++a)
      for (int j = 0; j < kB; ++j)
        xs_blocks[((size_t)b * kB + a) * kB + j] =
            x[(size_t)((b / kb) * kB + a) * k + s_indices[b] * kB + j];

  __half *d_x = ToDevice(ToHalf(x));
  __half *d_w1 = ToDevice(ToHalf(w1));
  __half *d_sx = ToDevice(ToHalf(xs_blocks));
  int *d_c_offsets = ToDevice(c_offsets);
  short *d_c_indices = ToDevice(c_indices);
  short *d_c_rows = ToDevice(c_rows);
  int *d_s_offsets = ToDevice(s_offsets);
  short *d_s_indices = ToDevice(s_indices);
  uint8_t *d_xq = DeviceBuffer<uint8_t>((size_t)m * k, 0x55);
  float *d_xs = DeviceBuffer<float>((size_t)m * kb, 0x55);
  uint8_t *d_w1q = DeviceBuffer<uint8_t>((size_t)n * k, 0x55);
  float *d_w1s = DeviceBuffer<float>((size_t)kb * nb, 0x55);
  uint8_t *d_sq = DeviceBuffer<uint8_t>((size_t)s_blocks * kB * kB, 0x55);
  float *d_ss = DeviceBuffer<float>((size_t)s_blocks * kB, 0x55);
  float *d_p = DeviceBuffer<float>((size_t)kb * m * n, 0x55);
  __half *d_c = DeviceBuffer<__half>((size_t)c_blocks * kB * kB, 0x55);
  __half *d_y = DeviceBuffer<__half>((size_t)m * n, 0x55);

  CHECK_HIP(sb::QuantizeRows(d_x, m, k, d_xq, d_xs, true, sb::DataType::kF16,
                             nullptr));
  CHECK_HIP(sb::QuantizeWeight(d_w1, k, n, false, d_w1q, d_w1s, true,
                               sb::DataType::kF16, nullptr));
  CHECK_HIP(sb::QuantizeRows(d_sx, s_blocks * kB, kB, d_sq, d_ss, true,
                             sb::DataType::kF16, nullptr));
  CHECK_HIP(hipDeviceSynchronize());
  const std::vector<float> xs = FromDevice(d_xs, (size_t)m * kb);
  const std::vector<float> ws = FromDevice(d_w1s, (size_t)kb * nb);

  // P of both modes: x_i / sa times w1 / sb in the interval that holds k(i),
  // +0 in the others.
  for (sb::Fp8Accumulate mode :
       {sb::Fp8Accumulate::kFp32, sb::Fp8Accumulate::kFast}) {
    CHECK_HIP(hipMemset(d_p, 0x55, (size_t)kb * m * n * sizeof(float)));
    CHECK_HIP(sb::Fp8IntervalSums(d_xq, d_w1q, m, n, k, mode, d_p, nullptr));
    CHECK_HIP(hipDeviceSynchronize());
    const std::vector<float> p = FromDevice(d_p, (size_t)kb * m * n);
    size_t bad = 0;
    for (int t = 0; t < kb; ++t)
      for (int i = 0; i < m; ++i)
        for (int nn = 0; nn < n; ++nn) {
          const int kk = k_of(i);
          const float want =
              kk / kB == t ? (x_of(i) / xs[(size_t)i * kb + t]) *
                                 (w1_of(kk, nn) / ws[(size_t)t * nb + nn / kB])
                           : 0.0f;
          const float got = p[((size_t)t * m + i) * n + nn];
          bad += !(got == want) ||
                 (want == 0.0f && kk / kB != t && std::signbit(got));
        }
    std::printf("Fp8IntervalSums mode %d: %zu of %zu elements differ\n",
                (int)mode, bad, p.size());
    ok &= Expect(bad == 0, "Fp8IntervalSums equals the one product exactly");
  }

  // C = X W1 at the stored blocks, Y = X W1 everywhere, in the fast mode.
  sb::BlockMatrix c(m, n, sb::BlockSize::k128, c_blocks * kB * kB, d_c,
                    d_c_offsets, d_c_indices, d_c_rows);
  CHECK_HIP(sb::SddFp8(d_xq, d_xs, k, d_w1q, d_w1s, c, sb::DataType::kF16,
                       sb::Fp8Accumulate::kFast, nullptr));
  sb::BlockMatrix s(m, k, sb::BlockSize::k128, s_blocks * kB * kB, d_sq,
                    d_s_offsets, d_s_indices);
  CHECK_HIP(sb::DsdFp8(s, d_ss, d_w1q, d_w1s, sb::Matrix(m, n, d_y),
                       sb::DataType::kF16, sb::Fp8Accumulate::kFast, nullptr));
  CHECK_HIP(hipDeviceSynchronize());
  {
    const std::vector<__half> got = FromDevice(d_c, (size_t)c_blocks * kB * kB);
    size_t bad = 0;
    for (int b = 0; b < c_blocks; ++b)
      for (int a = 0; a < kB; ++a)
        for (int j = 0; j < kB; ++j) {
          const int i = c_rows[b] * kB + a, nn = c_indices[b] * kB + j;
          bad += __half2float(got[((size_t)b * kB + a) * kB + j]) !=
                 x_of(i) * w1_of(k_of(i), nn);
        }
    std::printf("SddFp8 kFast: %zu of %zu elements differ\n", bad, got.size());
    ok &= Expect(bad == 0, "SddFp8 kFast equals X W1 exactly");
  }
  {
    const std::vector<__half> got = FromDevice(d_y, (size_t)m * n);
    size_t bad = 0;
    for (int i = 0; i < m; ++i)
      for (int nn = 0; nn < n; ++nn)
        bad += __half2float(got[(size_t)i * n + nn]) !=
               x_of(i) * w1_of(k_of(i), nn);
    std::printf("DsdFp8 kFast: %zu of %zu elements differ\n", bad, got.size());
    ok &= Expect(bad == 0, "DsdFp8 kFast equals X W1 exactly");
  }

  // Rejections: nothing is launched, the output keeps its fill.
  {
    const sb::Fp8Accumulate other = static_cast<sb::Fp8Accumulate>(2);
    CHECK_HIP(hipMemset(d_c, 0x55, (size_t)c_blocks * kB * kB * sizeof(__half)));
    CHECK_HIP(hipMemset(d_y, 0x55, (size_t)m * n * sizeof(__half)));
    CHECK_HIP(hipMemset(d_p, 0x55, (size_t)kb * m * n * sizeof(float)));
    ok &= Expect(sb::SddFp8(d_xq, d_xs, k, d_w1q, d_w1s, c, sb::DataType::kF16,
                            other, nullptr) == hipErrorInvalidValue,
                 "SddFp8 rejects an accumulation mode of 2");
    ok &= Expect(sb::DsdFp8(s, d_ss, d_w1q, d_w1s, sb::Matrix(m, n, d_y),
                            sb::DataType::kF16, other,
                            nullptr) == hipErrorInvalidValue,
                 "DsdFp8 rejects an accumulation mode of 2");
    ok &= Expect(sb::Fp8IntervalSums(d_xq, d_w1q, m, n, k, other, d_p,
                                     nullptr) == hipErrorInvalidValue,
                 "Fp8IntervalSums rejects an accumulation mode of 2");
    ok &= Expect(sb::Fp8IntervalSums(d_xq, d_w1q, m, n, 192,
                                     sb::Fp8Accumulate::kFast, d_p,
                                     nullptr) == hipErrorInvalidValue,
                 "k = 192 is rejected");
    ok &= Expect(sb::Fp8IntervalSums(d_xq, d_w1q, m, n, k,
                                     sb::Fp8Accumulate::kFast, nullptr,
                                     nullptr) == hipErrorInvalidValue,
                 "a null P is rejected");
    ok &= Expect(sb::Fp8IntervalSums(d_xq, d_w1q, m, n, k,
                                     sb::Fp8Accumulate::kFast,
                                     reinterpret_cast<float *>(d_xq),
                                     nullptr) == hipErrorInvalidValue,
                 "a P that is an input is rejected");
    ok &= Expect(sb::Fp8IntervalSums(d_xq, d_w1q, 0, n, k,
                                     sb::Fp8Accumulate::kFast, d_p,
                                     nullptr) == hipSuccess,
                 "zero-sized work succeeds");
    CHECK_HIP(hipDeviceSynchronize());
    ok &= Expect(AllHalf(d_c, (size_t)c_blocks * kB * kB, 0x5555) &&
                     AllHalf(d_y, (size_t)m * n, 0x5555) &&
                     AllHalf(reinterpret_cast<__half *>(d_p),
                             (size_t)kb * m * n * 2, 0x5555),
                 "the rejected calls left their outputs untouched");
  }

  for (void *p : {(void *)d_x, (void *)d_w1, (void *)d_sx, (void *)d_c_offsets,
                  (void *)d_c_indices, (void *)d_c_rows, (void *)d_s_offsets,
                  (void *)d_s_indices, (void *)d_xq, (void *)d_xs,
                  (void *)d_w1q, (void *)d_w1s, (void *)d_sq, (void *)d_ss,
                  (void *)d_p, (void *)d_c, (void *)d_y})
    CHECK_HIP(hipFree(p));
  std::printf(ok ? "ALL OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
