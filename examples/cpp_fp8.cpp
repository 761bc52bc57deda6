// A C++ caller of the fp8 products (sputnik/block/fp8.h), the forward calls of
// an expert MLP with e4m3 operands and block scales:
//   Xq = QuantizeRows(X), W1q = QuantizeWeight(W1), C = SddFp8(Xq, W1q),
//   Hq = QuantizeRowsActivation(relu, C's block values),
//   W2q = QuantizeWeight(W2), Y = DsdFp8(Hq, W2q)
// on known-answer data with power-of-two scales, so everything is exact and
// is checked bit for bit against host loops: X is one-hot per row (row i
// holds one value, at a k that differs per row and covers every k), W1 holds
// distinct small integers in an asymmetric pattern times a power of two per
// block, so C[i][n] = X[i][k(i)] W1[k(i)][n] pins every (row, k, column) of
// the MFMA lane map; W2 is one-hot per column, so Y[i][n] is one product of
// the dequantised H. C's topology has an empty block, unordered column
// indices and a block row whose blocks are not in k order. Built against
// libsputnik.so by sputnik_amd/Makefile; tests/test_cpp_fp8.py runs it on the
// GPU. Exit status 0 = all passed.
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

// ---- the format on the host (fp8.h), for finite values and pow2 scales ----

float Pow2Scale(float amax) {
  if (amax == 0.0f) return 0x1p-126f;
  int e;
  const float m = std::frexp(amax, &e);
  e -= m <= 0.875f ? 9 : 8;
  return std::ldexp(1.0f, e > -126 ? e : -126);
}

// rne_e4m3(y) as a value, |y| <= 448.
float RoundE4m3(float y) {
  const float a = std::fabs(y);
  int e;
  std::frexp(a, &e);  // a in [2^(e-1), 2^e)
  const float step = std::ldexp(1.0f, (a >= 0x1p-6f ? e - 1 : -6) - 3);
  return std::copysign(std::nearbyint(a / step) * step, y);
}

uint8_t EncodeE4m3(float q) {  // q exactly representable
  const uint8_t sign = std::signbit(q) ? 0x80 : 0;
  const float a = std::fabs(q);
  if (a < 0x1p-6f) return sign | (uint8_t)(a * 512.0f);
  int e;
  const float m = std::frexp(a, &e);
  return sign | (uint8_t)(((e - 1 + 7) << 3) | (int)((m * 2.0f - 1.0f) * 8.0f));
}

// One tile of `count` values at x[i * stride]: its scale, bytes and
// dequantised values.
float QuantizeTile(const float *x, int count, int stride, uint8_t *q,
                   int q_stride, float *dq) {
  float amax = 0.0f;
  for (int i = 0; i < count; ++i) amax = std::fmax(amax, std::fabs(x[i * stride]));
  const float s = Pow2Scale(amax);
  for (int i = 0; i < count; ++i) {
    const float v = RoundE4m3(x[i * stride] / s);
    q[i * q_stride] = EncodeE4m3(v);
    dq[i * stride] = v * s;
  }
  return s;
}

}  // namespace

int main() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) {
    std::fprintf(stderr, "no HIP device\n");
    return 2;
  }
  const int m = 256, k = 256, n = 384, n2 = 128;
  const int kb = k / kB, nb = n / kB;
  bool ok = true;

  // X: row i holds x_i at column k(i); 4 significant bits, so its e4m3 form
  // is exact, and the scale depends on the row.
  auto k_of = [&](int i) { return (i * 37 + 11) % k; };
  auto x_of = [&](int i) {
    return (i % 2 ? -1.0f : 1.0f) * (8 + i % 8) / 8.0f *
           std::ldexp(1.0f, i % 7 - 3);
  };
  std::vector<float> x((size_t)m * k, 0.0f);
  for (int i = 0; i < m; ++i) x[(size_t)i * k + k_of(i)] = x_of(i);
  // W1 [k, n]: integers in [-7, 7] times a power of two per block.
  auto w1_of = [&](int kk, int nn) {
    return (float)((kk * 7 + nn * 11) % 15 - 7) *
           std::ldexp(1.0f, (kk / kB + 2 * (nn / kB)) % 3);
  };
  std::vector<float> w1((size_t)k * n);
  for (int kk = 0; kk < k; ++kk)
    for (int nn = 0; nn < n; ++nn) w1[(size_t)kk * n + nn] = w1_of(kk, nn);
  // W2 [n, n2]: column j holds w2_j at row r(j).
  auto r_of = [&](int j) { return (j * 3 + 1) % n; };
  std::vector<float> w2((size_t)n * n2, 0.0f);
  for (int j = 0; j < n2; ++j)
    w2[(size_t)r_of(j) * n2 + j] =
        (j % 2 ? -1.0f : 1.0f) * (j % 7 + 1) * std::ldexp(1.0f, -(j % 3));

  // C's topology: 2 x 3 blocks, (1, 2) missing.
  const std::vector<int> offsets = {0, 3, 5};
  const std::vector<short> indices = {2, 0, 1, 1, 0};
  const std::vector<short> row_indices = {0, 0, 0, 1, 1};
  const int blocks = (int)indices.size();

  __half *d_x = ToDevice(ToHalf(x));
  __half *d_w1 = ToDevice(ToHalf(w1));
  __half *d_w2 = ToDevice(ToHalf(w2));
  int *d_offsets = ToDevice(offsets);
  short *d_indices = ToDevice(indices);
  short *d_row_indices = ToDevice(row_indices);
  uint8_t *d_xq = DeviceBuffer<uint8_t>((size_t)m * k, 0x55);
  float *d_xs = DeviceBuffer<float>((size_t)m * kb, 0x55);
  uint8_t *d_w1q = DeviceBuffer<uint8_t>((size_t)n * k, 0x55);
  float *d_w1s = DeviceBuffer<float>((size_t)kb * nb, 0x55);
  uint8_t *d_w2q = DeviceBuffer<uint8_t>((size_t)n2 * n, 0x55);
  float *d_w2s = DeviceBuffer<float>((size_t)nb, 0x55);
  __half *d_c = DeviceBuffer<__half>((size_t)blocks * kB * kB, 0x55);
  uint8_t *d_hq = DeviceBuffer<uint8_t>((size_t)blocks * kB * kB, 0x55);
  float *d_hs = DeviceBuffer<float>((size_t)blocks * kB, 0x55);
  __half *d_y = DeviceBuffer<__half>((size_t)m * n2, 0x55);

  CHECK_HIP(sb::QuantizeRows(d_x, m, k, d_xq, d_xs, true, sb::DataType::kF16,
                             nullptr));
  CHECK_HIP(sb::QuantizeWeight(d_w1, k, n, false, d_w1q, d_w1s, true,
                               sb::DataType::kF16, nullptr));
  CHECK_HIP(sb::QuantizeWeight(d_w2, n, n2, false, d_w2q, d_w2s, true,
                               sb::DataType::kF16, nullptr));
  sb::BlockMatrix c(m, n, sb::BlockSize::k128, blocks * kB * kB, d_c,
                    d_offsets, d_indices, d_row_indices);
  CHECK_HIP(sb::SddFp8(d_xq, d_xs, k, d_w1q, d_w1s, c, sb::DataType::kF16,
                       nullptr));
  CHECK_HIP(sb::QuantizeRowsActivation(d_c, blocks * kB, kB,
                                       sb::Activation::kRelu, d_hq, d_hs, true,
                                       sb::DataType::kF16, nullptr));
  sb::BlockMatrix h(m, n, sb::BlockSize::k128, blocks * kB * kB, d_hq,
                    d_offsets, d_indices);
  CHECK_HIP(sb::DsdFp8(h, d_hs, d_w2q, d_w2s, sb::Matrix(m, n2, d_y),
                       sb::DataType::kF16, nullptr));
  CHECK_HIP(hipDeviceSynchronize());

  // The quantised operands.
  {
    std::vector<uint8_t> q((size_t)m * k), wq((size_t)n * k);
    std::vector<float> s((size_t)m * kb), ws((size_t)kb * nb), dq(x.size()),
        wdq(w1.size());
    for (int i = 0; i < m; ++i)
      for (int t = 0; t < kb; ++t)
        s[(size_t)i * kb + t] =
            QuantizeTile(&x[(size_t)i * k + t * kB], kB, 1,
                         &q[(size_t)i * k + t * kB], 1,
                         &dq[(size_t)i * k + t * kB]);
    ok &= Expect(FromDevice(d_xq, q.size()) == q, "QuantizeRows bytes");
    ok &= Expect(FromDevice(d_xs, s.size()) == s, "QuantizeRows scales");
    ok &= Expect(dq == x, "the row quantisation of X is exact");
    // (a weight block: the amax over 128 x 128, bytes stored [n][k])
    for (int t = 0; t < kb; ++t)
      for (int u = 0; u < nb; ++u) {
        float amax = 0.0f;
        for (int a = 0; a < kB; ++a)
          for (int b = 0; b < kB; ++b)
            amax = std::fmax(amax, std::fabs(w1_of(t * kB + a, u * kB + b)));
        const float sc = Pow2Scale(amax);
        ws[(size_t)t * nb + u] = sc;
        for (int a = 0; a < kB; ++a)
          for (int b = 0; b < kB; ++b) {
            const int kk = t * kB + a, nn = u * kB + b;
            const float v = RoundE4m3(w1_of(kk, nn) / sc);
            wq[(size_t)nn * k + kk] = EncodeE4m3(v);
            wdq[(size_t)kk * n + nn] = v * sc;
          }
      }
    ok &= Expect(FromDevice(d_w1q, wq.size()) == wq, "QuantizeWeight bytes");
    ok &= Expect(FromDevice(d_w1s, ws.size()) == ws, "QuantizeWeight scales");
    ok &= Expect(wdq == w1, "the block quantisation of W1 is exact");
  }

  // C = X W1 at the stored blocks: one product per element.
  std::vector<float> c_ref((size_t)blocks * kB * kB);
  for (int b = 0; b < blocks; ++b)
    for (int a = 0; a < kB; ++a)
      for (int j = 0; j < kB; ++j) {
        const int i = row_indices[b] * kB + a, nn = indices[b] * kB + j;
        c_ref[((size_t)b * kB + a) * kB + j] = x_of(i) * w1_of(k_of(i), nn);
      }
  {
    const std::vector<__half> got = FromDevice(d_c, c_ref.size());
    size_t bad = 0;
    for (size_t i = 0; i < got.size(); ++i)
      bad += __half2float(got[i]) != c_ref[i];
    std::printf("SddFp8: %zu of %zu elements differ\n", bad, got.size());
    ok &= Expect(bad == 0, "SddFp8 equals X W1 exactly");
  }

  // Hq = quantised relu(C), one scale per row of each stored block.
  std::vector<float> h_dq(c_ref.size());
  {
    std::vector<uint8_t> q(c_ref.size());
    std::vector<float> s((size_t)blocks * kB), relu(c_ref.size());
    for (size_t i = 0; i < relu.size(); ++i)
      relu[i] = c_ref[i] > 0.0f ? c_ref[i] : 0.0f;
    for (int row = 0; row < blocks * kB; ++row)
      s[row] = QuantizeTile(&relu[(size_t)row * kB], kB, 1,
                            &q[(size_t)row * kB], 1, &h_dq[(size_t)row * kB]);
    ok &= Expect(FromDevice(d_hq, q.size()) == q,
                 "QuantizeRowsActivation bytes");
    ok &= Expect(FromDevice(d_hs, s.size()) == s,
                 "QuantizeRowsActivation scales");
  }

  // Y = H W2: Y[i][j] = H[i][r(j)] w2_j where that block of H is stored.
  {
    const std::vector<__half> got = FromDevice(d_y, (size_t)m * n2);
    size_t bad = 0;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < n2; ++j) {
        float want = 0.0f;
        for (int b = 0; b < blocks; ++b)
          if (row_indices[b] == i / kB && indices[b] == r_of(j) / kB)
            want = h_dq[((size_t)b * kB + i % kB) * kB + r_of(j) % kB] *
                   w2[(size_t)r_of(j) * n2 + j];
        bad += __half2float(got[(size_t)i * n2 + j]) != want;
      }
    std::printf("DsdFp8: %zu of %d elements differ\n", bad, m * n2);
    ok &= Expect(bad == 0, "DsdFp8 equals H W2 exactly");
  }

  // Rejections: nothing is launched, the output keeps its fill.
  {
    ok &= Expect(sb::QuantizeRows(d_x, m, 192, d_xq, d_xs, true,
                                  sb::DataType::kF16,
                                  nullptr) == hipErrorInvalidValue,
                 "cols = 192 is rejected");
    ok &= Expect(sb::SddFp8(d_xq, nullptr, k, d_w1q, d_w1s, c,
                            sb::DataType::kF16,
                            nullptr) == hipErrorInvalidValue,
                 "a null scale pointer is rejected");
    sb::BlockMatrix alias = c;
    alias.data = d_w1q;
    ok &= Expect(sb::SddFp8(d_xq, d_xs, k, d_w1q, d_w1s, alias,
                            sb::DataType::kF16,
                            nullptr) == hipErrorInvalidValue,
                 "an output that is an input is rejected");
    ok &= Expect(sb::DsdFp8(h, d_hs, d_w2q, d_w2s, sb::Matrix(m, 0, d_y),
                            sb::DataType::kF16, nullptr) == hipSuccess,
                 "zero-sized work succeeds");
  }

  for (void *p : {(void *)d_x, (void *)d_w1, (void *)d_w2, (void *)d_offsets,
                  (void *)d_indices, (void *)d_row_indices, (void *)d_xq,
                  (void *)d_xs, (void *)d_w1q, (void *)d_w1s, (void *)d_w2q,
                  (void *)d_w2s, (void *)d_c, (void *)d_hq, (void *)d_hs,
                  (void *)d_y})
    CHECK_HIP(hipFree(p));
  std::printf(ok ? "ALL OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
