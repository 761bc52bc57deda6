// A C++ caller of the bias products (sputnik/block/bias.h, moe.h), the calls
// an expert MLP with per-expert biases makes:
//   forward   C = X W1 + b (MatmulBias), H = relu(X W1 + b) with Z kept
//             (MatmulBiasActivation), out = y + b2[expert] (PaddedScatterBias)
//   backward  db = column sums of the sparse Z (BlockColumnSum)
// Operands are -1 / 0 / 1, K is 40 and the bias of column c is (c - n/2) / 8,
// a distinct value per logical column, so every biased value is a multiple of
// 1/8 below 128, exact in fp16, and every column sum is exact in fp32:
// everything is checked bit for bit against host loops. Built against
// libsputnik.so by sputnik_amd/Makefile; tests/test_cpp_bias.py runs it on
// the GPU. Exit status 0 = all passed.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
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

std::vector<__half> ToHalf(const std::vector<float> &x) {
  std::vector<__half> h(x.size());
  for (size_t i = 0; i < x.size(); ++i) h[i] = __float2half(x[i]);
  return h;
}

std::vector<float> FromDevice(const __half *d, size_t n) {
  std::vector<__half> h(n);
  CHECK_HIP(hipMemcpy(h.data(), d, n * sizeof(__half), hipMemcpyDeviceToHost));
  std::vector<float> out(n);
  for (size_t i = 0; i < n; ++i) out[i] = __half2float(h[i]);
  return out;
}

}  // namespace

int main() {
  // Tokens x hidden: 384 x 512 in 128 x 128 blocks, block-row 1 empty.
  const int m = 384, n = 512, k = 40;
  std::mt19937 gen(17);
  std::uniform_int_distribution<int> tri(-1, 1);
  std::bernoulli_distribution keep(0.6);

  std::vector<int> offsets{0};
  std::vector<short> indices;
  for (int r = 0; r < m / kB; ++r) {
    for (int c = n / kB - 1; c >= 0; --c)  // (descending: unsorted columns)
      if (r != 1 && (keep(gen) || c == r)) indices.push_back((short)c);
    offsets.push_back((int)indices.size());
  }
  const int nb = (int)indices.size();
  const size_t nnz = (size_t)nb * kB * kB;

  std::vector<float> x((size_t)m * k), w1((size_t)k * n), bias(n);
  for (auto *v : {&x, &w1})
    for (auto &e : *v) e = (float)tri(gen);
  for (int c = 0; c < n; ++c) bias[c] = (float)(c - n / 2) / 8.0f;
  __half *d_x = ToDevice(ToHalf(x)), *d_w1 = ToDevice(ToHalf(w1));
  __half *d_b = ToDevice(ToHalf(bias));
  __half *d_c, *d_h, *d_z;
  CHECK_HIP(hipMalloc(&d_c, nnz * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_h, nnz * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_z, nnz * sizeof(__half)));
  int *d_off = ToDevice(offsets);
  short *d_idx = ToDevice(indices);

  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  sb::BlockMatrix c(m, n, sb::AsBlockSize(kB), (int)nnz, d_c, d_off, d_idx);
  sb::AllocateRowIndicesBuffer(c);
  CHECK_HIP(sb::RowIndices(c, static_cast<short *>(c.row_indices), stream));
  sb::AllocateTransposeBuffers(c);
  CHECK_HIP(sb::Transpose(c, stream));
  sb::BlockMatrix h = c, z = c;
  h.data = d_h;
  z.data = d_z;
  bool ok = true;

  // Host: Z = X W1 + b at the stored blocks and its column sums (exact).
  std::vector<float> z_ref(nnz), sum_ref(n, 0.f);
  for (int r = 0; r < m / kB; ++r)
    for (int e = offsets[r]; e < offsets[r + 1]; ++e)
      for (int i = 0; i < kB; ++i)
        for (int j = 0; j < kB; ++j) {
          const int row = r * kB + i, col = indices[e] * kB + j;
          float acc = 0.f;
          for (int l = 0; l < k; ++l)
            acc += x[(size_t)row * k + l] * w1[(size_t)l * n + col];
          z_ref[((size_t)e * kB + i) * kB + j] = acc + bias[col];
          sum_ref[col] += acc + bias[col];
        }

  // ---- C = X W1 + b -------------------------------------------------------
  CHECK_HIP(sb::MatmulBias(sb::Matrix(m, k, d_x), false,
                           sb::Matrix(k, n, d_w1), false, c, d_b,
                           sb::DataType::kF16, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  {
    const std::vector<float> cv = FromDevice(d_c, nnz);
    size_t bad = 0;
    for (size_t i = 0; i < nnz; ++i) bad += cv[i] != z_ref[i];
    ok &= Expect(bad == 0, "C = X W1 + b: exact");
  }

  // ---- H = relu(X W1 + b), Z kept ----------------------------------------
  CHECK_HIP(sb::MatmulBiasActivation(sb::Matrix(m, k, d_x), false,
                                     sb::Matrix(k, n, d_w1), false, h, d_b,
                                     sb::Activation::kRelu, d_z,
                                     sb::DataType::kF16, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  {
    const std::vector<float> hv = FromDevice(d_h, nnz), zv = FromDevice(d_z, nnz);
    size_t bad_z = 0, bad_h = 0;
    for (size_t i = 0; i < nnz; ++i) {
      bad_z += zv[i] != z_ref[i];
      bad_h += hv[i] != (z_ref[i] > 0.f ? z_ref[i] : 0.f);
    }
    ok &= Expect(bad_z == 0, "Z = X W1 + b kept: exact");
    ok &= Expect(bad_h == 0, "H = relu(Z): exact");
  }

  // ---- db = column sums of Z ---------------------------------------------
  {
    float *d_sum = nullptr;
    CHECK_HIP(hipMalloc(&d_sum, n * sizeof(float)));
    CHECK_HIP(hipMemsetAsync(d_sum, 0xff, n * sizeof(float), stream));
    CHECK_HIP(sb::BlockColumnSum(z, sb::DataType::kF16, d_sum, stream));
    std::vector<float> sum(n);
    CHECK_HIP(hipMemcpyAsync(sum.data(), d_sum, n * sizeof(float),
                             hipMemcpyDeviceToHost, stream));
    CHECK_HIP(hipStreamSynchronize(stream));
    size_t bad = 0;
    for (int j = 0; j < n; ++j) bad += sum[j] != sum_ref[j];
    ok &= Expect(bad == 0, "BlockColumnSum(Z): exact");
    sb::BlockMatrix bare = z;
    bare.offsets_t = nullptr;
    ok &= Expect(sb::BlockColumnSum(bare, sb::DataType::kF16, d_sum, stream) ==
                     hipErrorInvalidValue,
                 "no transposed metadata: hipErrorInvalidValue");
    CHECK_HIP(hipFree(d_sum));
  }

  // ---- a bias that is missing or aliases is rejected ----------------------
  ok &= Expect(sb::MatmulBias(sb::Matrix(m, k, d_x), false,
                              sb::Matrix(k, n, d_w1), false, c, nullptr,
                              sb::DataType::kF16, stream) ==
                   hipErrorInvalidValue,
               "null bias: hipErrorInvalidValue");
  ok &= Expect(sb::MatmulBias(sb::Matrix(m, k, d_x), false,
                              sb::Matrix(k, n, d_w1), false, c, d_c,
                              sb::DataType::kF16, stream) ==
                   hipErrorInvalidValue,
               "bias == c.data: hipErrorInvalidValue");

  // ---- out[t] = y[row_of[t]] + b2[expert of the row] -----------------------
  {
    const int tokens = 3, hidden = 8, experts = 2, rows = 256;
    const std::vector<int> row_of{0, 128, 1}, padded_bins{128, 256};
    std::vector<float> y((size_t)rows * hidden), b2((size_t)experts * hidden);
    for (auto &e : y) e = (float)tri(gen);
    for (size_t i = 0; i < b2.size(); ++i) b2[i] = (float)i / 4.0f;
    __half *d_y = ToDevice(ToHalf(y)), *d_b2 = ToDevice(ToHalf(b2)), *d_out;
    int *d_row = ToDevice(row_of), *d_pad = ToDevice(padded_bins);
    CHECK_HIP(hipMalloc(&d_out, tokens * hidden * sizeof(__half)));
    CHECK_HIP(sb::PaddedScatterBias(d_y, d_row, d_pad, d_b2, nullptr, d_out,
                                    tokens, hidden, 1, experts, rows,
                                    sb::DataType::kF16,
                                    sb::WeightType::kOperand, stream));
    CHECK_HIP(hipStreamSynchronize(stream));
    const std::vector<float> ov = FromDevice(d_out, (size_t)tokens * hidden);
    size_t bad = 0;
    for (int t = 0; t < tokens; ++t)
      for (int j = 0; j < hidden; ++j)
        bad += ov[t * hidden + j] != y[(size_t)row_of[t] * hidden + j] +
                                         b2[(row_of[t] / 128) * hidden + j];
    ok &= Expect(bad == 0, "PaddedScatterBias: exact");
    for (void *p : {(void *)d_y, (void *)d_b2, (void *)d_out, (void *)d_row,
                    (void *)d_pad})
      CHECK_HIP(hipFree(p));
  }

  sb::FreeTransposeBuffers(c);
  sb::FreeRowIndicesBuffer(c);
  for (void *p : {(void *)d_x, (void *)d_w1, (void *)d_b, (void *)d_c,
                  (void *)d_h, (void *)d_z, (void *)d_off, (void *)d_idx})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(stream));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
