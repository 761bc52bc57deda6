// A C++ caller of the fp8 gradient pieces (sputnik/block/fp8.h, "Gradients"):
// the weight gradient dW [F, h] = S^T B of a sparse S [T, F] (16-bit block
// values) and a dense B [T, h], both quantised along the token dimension:
//   Transpose(S) for offsets_t / indices_t / block_offsets,
//   QuantizeBlocks(S): S^T's blocks with one scale per source column (and the
//     row outputs, which are QuantizeRows' bytes),
//   QuantizeTiles(B): B in 128 x 1 column tiles, stored [h, T],
//   DsdFp8Wgrad into an fp32 dW, then once more with `add`,
// and TransposeWeightFp8 against QuantizeWeight of the transposed buffer.
// Known-answer data with power-of-two scales, so everything is exact and is
// checked bit for bit against host loops: S holds small integers times a
// power of two per column, B is one-hot per column, so dW[f][j] is one
// product. S's topology has an empty block column (an empty block row of
// S^T: +0 rows, left alone under `add`) and a block row stored out of order.
// Built against libsputnik.so by sputnik_amd/Makefile;
// tests/test_cpp_fp8_grad.py runs it on the GPU. Exit status 0 = all passed.
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

uint8_t EncodeE4m3(float q) {  // q exactly representable
  const uint8_t sign = std::signbit(q) ? 0x80 : 0;
  const float a = std::fabs(q);
  if (a < 0x1p-6f) return sign | (uint8_t)(a * 512.0f);
  int e;
  const float m = std::frexp(a, &e);
  return sign | (uint8_t)(((e - 1 + 7) << 3) | (int)((m * 2.0f - 1.0f) * 8.0f));
}

// One tile of `count` values at x[i * stride], each exact in e4m3 under the
// tile's power-of-two scale: the scale, and the bytes at q[i * q_stride].
float QuantizeTile(const float *x, int count, int stride, uint8_t *q,
                   int q_stride) {
  float amax = 0.0f;
  for (int i = 0; i < count; ++i) amax = std::fmax(amax, std::fabs(x[i * stride]));
  const float s = Pow2Scale(amax);
  for (int i = 0; i < count; ++i) q[i * q_stride] = EncodeE4m3(x[i * stride] / s);
  return s;
}

}  // namespace

int main() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) {
    std::fprintf(stderr, "no HIP device\n");
    return 2;
  }
  const int tokens = 256, ffn = 384, hidden = 128;
  bool ok = true;

  // S [tokens, ffn]: 2 x 3 blocks, block column 1 empty, block row 0 stored
  // out of order.
  const std::vector<int> offsets = {0, 2, 3};
  const std::vector<short> indices = {2, 0, 0};
  const std::vector<short> row_of_block = {0, 0, 1};
  const int blocks = (int)indices.size();
  auto s_of = [&](int b, int r, int c) {
    return (float)((r * 7 + c * 11 + b * 5) % 15 - 7) *
           std::ldexp(1.0f, (c + b) % 3);
  };
  std::vector<float> s((size_t)blocks * kB * kB);
  for (int b = 0; b < blocks; ++b)
    for (int r = 0; r < kB; ++r)
      for (int c = 0; c < kB; ++c)
        s[((size_t)b * kB + r) * kB + c] = s_of(b, r, c);
  // B [tokens, hidden]: column j holds b_j at token t(j).
  auto t_of = [&](int j) { return (j * 5 + 3) % tokens; };
  auto b_of = [&](int j) {
    return (j % 2 ? -1.0f : 1.0f) * (j % 7 + 1) * std::ldexp(1.0f, -(j % 3));
  };
  std::vector<float> bmat((size_t)tokens * hidden, 0.0f);
  for (int j = 0; j < hidden; ++j) bmat[(size_t)t_of(j) * hidden + j] = b_of(j);

  __half *d_s = ToDevice(ToHalf(s));
  __half *d_b = ToDevice(ToHalf(bmat));
  int *d_offsets = ToDevice(offsets);
  short *d_indices = ToDevice(indices);
  const size_t nnz = (size_t)blocks * kB * kB;
  uint8_t *d_q = DeviceBuffer<uint8_t>(nnz, 0x55);
  float *d_qs = DeviceBuffer<float>((size_t)blocks * kB, 0x55);
  uint8_t *d_qr = DeviceBuffer<uint8_t>(nnz, 0x55);
  float *d_qrs = DeviceBuffer<float>((size_t)blocks * kB, 0x55);
  uint8_t *d_qt = DeviceBuffer<uint8_t>(nnz, 0x55);
  float *d_qts = DeviceBuffer<float>((size_t)blocks * kB, 0x55);
  uint8_t *d_bqt = DeviceBuffer<uint8_t>((size_t)hidden * tokens, 0x55);
  float *d_bst = DeviceBuffer<float>((size_t)(tokens / kB) * hidden, 0x55);
  float *d_dw = DeviceBuffer<float>((size_t)ffn * hidden, 0x55);

  sb::BlockMatrix sm(tokens, ffn, sb::BlockSize::k128, (int)nnz, d_s, d_offsets,
                     d_indices);
  sb::AllocateTransposeBuffers(sm);
  CHECK_HIP(sb::Transpose(sm, nullptr));
  CHECK_HIP(sb::QuantizeBlocks(sm, sb::Fp8Stage::kNone, sb::Activation::kRelu,
                               nullptr, d_q, d_qs, d_qt, d_qts, true,
                               sb::DataType::kF16, nullptr));
  CHECK_HIP(sb::QuantizeRows(d_s, blocks * kB, kB, d_qr, d_qrs, true,
                             sb::DataType::kF16, nullptr));
  CHECK_HIP(sb::QuantizeTiles(d_b, tokens, hidden, nullptr, nullptr, d_bqt,
                              d_bst, true, sb::DataType::kF16, nullptr));
  // S^T [ffn, tokens] over the transposed metadata.
  sb::BlockMatrix st(ffn, tokens, sb::BlockSize::k128, (int)nnz, d_qt,
                     sm.offsets_t, sm.indices_t);
  const sb::Matrix dw(ffn, hidden, d_dw);
  CHECK_HIP(sb::DsdFp8Wgrad(st, d_qts, d_bqt, d_bst, dw, sb::DataType::kF16,
                            sb::OutputType::kF32, false,
                            sb::Fp8Accumulate::kFp32, nullptr));
  CHECK_HIP(hipDeviceSynchronize());

  // The transposed order: the stored blocks by column.
  const std::vector<int> block_offsets = {1, 2, 0};
  ok &= Expect(FromDevice((const int *)sm.block_offsets, blocks) == block_offsets,
               "Transpose's block_offsets");
  // Row outputs: QuantizeRows' bits.
  ok &= Expect(FromDevice(d_q, nnz) == FromDevice(d_qr, nnz),
               "QuantizeBlocks' row bytes are QuantizeRows'");
  ok &= Expect(FromDevice(d_qs, (size_t)blocks * kB) ==
                   FromDevice(d_qrs, (size_t)blocks * kB),
               "QuantizeBlocks' row scales are QuantizeRows'");
  // Column outputs: output block j is source block block_offsets[j] stored
  // [column][row], one scale per source column.
  {
    std::vector<uint8_t> q(nnz);
    std::vector<float> sc((size_t)blocks * kB);
    for (int j = 0; j < blocks; ++j)
      for (int c = 0; c < kB; ++c)
        sc[(size_t)j * kB + c] =
            QuantizeTile(&s[(size_t)block_offsets[j] * kB * kB + c], kB, kB,
                         &q[((size_t)j * kB + c) * kB], 1);
    ok &= Expect(FromDevice(d_qt, nnz) == q, "QuantizeBlocks' column bytes");
    ok &= Expect(FromDevice(d_qts, sc.size()) == sc,
                 "QuantizeBlocks' column scales");
  }
  // B in 128 x 1 tiles, stored [hidden, tokens].
  {
    std::vector<uint8_t> q((size_t)hidden * tokens);
    std::vector<float> sc((size_t)(tokens / kB) * hidden);
    for (int tb = 0; tb < tokens / kB; ++tb)
      for (int j = 0; j < hidden; ++j)
        sc[(size_t)tb * hidden + j] =
            QuantizeTile(&bmat[(size_t)tb * kB * hidden + j], kB, hidden,
                         &q[(size_t)j * tokens + tb * kB], 1);
    ok &= Expect(FromDevice(d_bqt, q.size()) == q, "QuantizeTiles' column bytes");
    ok &= Expect(FromDevice(d_bst, sc.size()) == sc,
                 "QuantizeTiles' column scales");
  }
  // dW[f][j] = S[t(j)][f] b_j where that block of S is stored.
  std::vector<float> want((size_t)ffn * hidden, 0.0f);
  for (int f = 0; f < ffn; ++f)
    for (int j = 0; j < hidden; ++j)
      for (int b = 0; b < blocks; ++b)
        if (row_of_block[b] == t_of(j) / kB && indices[b] == f / kB)
          want[(size_t)f * hidden + j] = s_of(b, t_of(j) % kB, f % kB) * b_of(j);
  {
    const std::vector<float> got = FromDevice(d_dw, want.size());
    size_t bad = 0, negative_zero = 0;
    for (size_t i = 0; i < got.size(); ++i) bad += got[i] != want[i];
    for (size_t i = (size_t)kB * hidden; i < (size_t)2 * kB * hidden; ++i)
      negative_zero += std::signbit(got[i]) || got[i] != 0.0f;
    std::printf("DsdFp8Wgrad: %zu of %zu elements differ\n", bad, got.size());
    ok &= Expect(bad == 0, "DsdFp8Wgrad equals S^T B exactly");
    ok &= Expect(negative_zero == 0, "the empty block row is +0");
  }
  // Once more with add: twice the product, and the empty block row keeps
  // what it held.
  {
    std::vector<float> before = FromDevice(d_dw, want.size());
    for (size_t i = (size_t)kB * hidden; i < (size_t)2 * kB * hidden; ++i)
      before[i] = 7.0f;
    CHECK_HIP(hipMemcpy(d_dw, before.data(), before.size() * sizeof(float),
                        hipMemcpyHostToDevice));
    CHECK_HIP(sb::DsdFp8Wgrad(st, d_qts, d_bqt, d_bst, dw, sb::DataType::kF16,
                              sb::OutputType::kF32, true,
                              sb::Fp8Accumulate::kFast, nullptr));
    CHECK_HIP(hipDeviceSynchronize());
    const std::vector<float> got = FromDevice(d_dw, want.size());
    size_t bad = 0;
    for (size_t i = 0; i < got.size(); ++i) {
      const bool empty = i / ((size_t)kB * hidden) == 1;
      bad += got[i] != (empty ? 7.0f : 2.0f * want[i]);
    }
    ok &= Expect(bad == 0, "add gives twice the product and skips empty rows");
  }

  // The backward layout of a weight that exists only as fp8.
  {
    const int k = 256, n = 128;
    std::vector<float> w((size_t)k * n);
    for (int kk = 0; kk < k; ++kk)
      for (int nn = 0; nn < n; ++nn)
        w[(size_t)kk * n + nn] = (float)((kk * 3 + nn * 5) % 17 - 8) / 4.0f;
    __half *d_w = ToDevice(ToHalf(w));
    uint8_t *d_wq = DeviceBuffer<uint8_t>((size_t)n * k, 0x55);
    float *d_ws = DeviceBuffer<float>((size_t)(k / kB) * (n / kB), 0x55);
    uint8_t *d_wt = DeviceBuffer<uint8_t>((size_t)n * k, 0x55);
    float *d_wts = DeviceBuffer<float>((size_t)(k / kB) * (n / kB), 0x55);
    uint8_t *d_ref = DeviceBuffer<uint8_t>((size_t)n * k, 0x55);
    float *d_refs = DeviceBuffer<float>((size_t)(k / kB) * (n / kB), 0x55);
    CHECK_HIP(sb::QuantizeWeight(d_w, k, n, false, d_wq, d_ws, false,
                                 sb::DataType::kF16, nullptr));
    CHECK_HIP(sb::TransposeWeightFp8(d_wq, d_ws, k, n, d_wt, d_wts, nullptr));
    // (the same buffer read as the weight [n, k] given transposed)
    CHECK_HIP(sb::QuantizeWeight(d_w, n, k, true, d_ref, d_refs, false,
                                 sb::DataType::kF16, nullptr));
    CHECK_HIP(hipDeviceSynchronize());
    ok &= Expect(FromDevice(d_wt, (size_t)n * k) == FromDevice(d_ref, (size_t)n * k),
                 "TransposeWeightFp8 bytes");
    ok &= Expect(FromDevice(d_wts, 2) == FromDevice(d_refs, 2),
                 "TransposeWeightFp8 scales");
    for (void *p : {(void *)d_w, (void *)d_wq, (void *)d_ws, (void *)d_wt,
                    (void *)d_wts, (void *)d_ref, (void *)d_refs})
      CHECK_HIP(hipFree(p));
  }

  // Rejections: nothing is launched.
  {
    sb::BlockMatrix plain(tokens, ffn, sb::BlockSize::k128, (int)nnz, d_s,
                          d_offsets, d_indices);
    ok &= Expect(sb::QuantizeBlocks(plain, sb::Fp8Stage::kNone,
                                    sb::Activation::kRelu, nullptr, nullptr,
                                    nullptr, d_qt, d_qts, true,
                                    sb::DataType::kF16,
                                    nullptr) == hipErrorInvalidValue,
                 "column outputs without block_offsets are rejected");
    ok &= Expect(sb::QuantizeTiles(d_b, tokens, hidden, nullptr, nullptr,
                                   nullptr, nullptr, true, sb::DataType::kF16,
                                   nullptr) == hipErrorInvalidValue,
                 "no output pair is rejected");
    ok &= Expect(sb::DsdFp8Wgrad(st, d_qts, d_bqt, d_bst,
                                 sb::Matrix(ffn, hidden, d_bqt),
                                 sb::DataType::kF16, sb::OutputType::kF32,
                                 false, sb::Fp8Accumulate::kFp32,
                                 nullptr) == hipErrorInvalidValue,
                 "an output that is an input is rejected");
  }

  sb::FreeTransposeBuffers(sm);
  for (void *p : {(void *)d_s, (void *)d_b, (void *)d_offsets,
                  (void *)d_indices, (void *)d_q, (void *)d_qs, (void *)d_qr,
                  (void *)d_qrs, (void *)d_qt, (void *)d_qts, (void *)d_bqt,
                  (void *)d_bst, (void *)d_dw})
    CHECK_HIP(hipFree(p));
  std::printf(ok ? "ALL OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
