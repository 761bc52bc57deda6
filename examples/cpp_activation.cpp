// A C++ caller of the SDD activation products (sputnik/block/activation.h),
// the two calls an expert MLP makes around its sparse hidden matrix:
//   forward   H = relu(X W1) at the topology's blocks, Z = X W1 kept
//   backward  dZ = (dY W2^T) * relu'(Z)
// Operands are -1 / 0 / 1, so every product is a small integer, exact in
// fp16, and relu is exact: H, Z and dZ are checked bit for bit against host
// loops. A second forward with silu is checked to one part in 2^9 (two fp16
// steps). Built against libsputnik.so by sputnik_amd/Makefile;
// tests/test_cpp_activation.py runs it on the GPU. Exit status 0 = all passed.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
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
  const int m = 384, n = 512, k = 72;
  std::mt19937 gen(11);
  std::uniform_int_distribution<int> tri(-1, 1);
  std::bernoulli_distribution keep(0.6);

  std::vector<int> offsets{0};
  std::vector<short> indices;
  for (int r = 0; r < m / kB; ++r) {
    for (int c = 0; c < n / kB; ++c)
      if (r != 1 && (keep(gen) || c == r)) indices.push_back((short)c);
    offsets.push_back((int)indices.size());
  }
  const int nb = (int)indices.size();
  const size_t nnz = (size_t)nb * kB * kB;

  std::vector<float> x((size_t)m * k), w1((size_t)k * n), dy((size_t)m * k),
      w2((size_t)n * k);
  for (auto *v : {&x, &w1, &dy, &w2})
    for (auto &e : *v) e = (float)tri(gen);
  __half *d_x = ToDevice(ToHalf(x)), *d_w1 = ToDevice(ToHalf(w1));
  __half *d_dy = ToDevice(ToHalf(dy)), *d_w2 = ToDevice(ToHalf(w2));
  __half *d_h, *d_z, *d_dz;
  CHECK_HIP(hipMalloc(&d_h, nnz * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_z, nnz * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_dz, nnz * sizeof(__half)));
  int *d_off = ToDevice(offsets);
  short *d_idx = ToDevice(indices);

  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  sb::BlockMatrix h(m, n, sb::AsBlockSize(kB), (int)nnz, d_h, d_off, d_idx);
  sb::AllocateRowIndicesBuffer(h);
  CHECK_HIP(sb::RowIndices(h, static_cast<short *>(h.row_indices), stream));
  sb::BlockMatrix dz = h;
  dz.data = d_dz;
  bool ok = true;

  // Host: Z = X W1 and G = dY W2^T at the stored blocks (exact integers).
  std::vector<float> z_ref(nnz), g_ref(nnz);
  for (int r = 0; r < m / kB; ++r)
    for (int e = offsets[r]; e < offsets[r + 1]; ++e)
      for (int i = 0; i < kB; ++i)
        for (int j = 0; j < kB; ++j) {
          const int row = r * kB + i, col = indices[e] * kB + j;
          float z = 0.f, g = 0.f;
          for (int l = 0; l < k; ++l) {
            z += x[(size_t)row * k + l] * w1[(size_t)l * n + col];
            g += dy[(size_t)row * k + l] * w2[(size_t)col * k + l];
          }
          z_ref[((size_t)e * kB + i) * kB + j] = z;
          g_ref[((size_t)e * kB + i) * kB + j] = g;
        }

  // ---- forward: H = relu(X W1), Z kept ------------------------------------
  CHECK_HIP(sb::MatmulActivation(sb::Matrix(m, k, d_x), false,
                                 sb::Matrix(k, n, d_w1), false, h,
                                 sb::Activation::kRelu, d_z,
                                 sb::DataType::kF16, stream));
  // ---- backward: dZ = (dY W2^T) * relu'(Z) --------------------------------
  CHECK_HIP(sb::MatmulActivationGrad(sb::Matrix(m, k, d_dy), false,
                                     sb::Matrix(n, k, d_w2), true, dz,
                                     sb::Activation::kRelu, d_z,
                                     sb::DataType::kF16, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  {
    const std::vector<float> hv = FromDevice(d_h, nnz), zv = FromDevice(d_z, nnz),
                             dv = FromDevice(d_dz, nnz);
    size_t bad_z = 0, bad_h = 0, bad_d = 0;
    for (size_t i = 0; i < nnz; ++i) {
      bad_z += zv[i] != z_ref[i];
      bad_h += hv[i] != (z_ref[i] > 0.f ? z_ref[i] : 0.f);
      bad_d += dv[i] != (z_ref[i] > 0.f ? g_ref[i] : 0.f);
    }
    ok &= Expect(bad_z == 0, "pre-activation Z = X W1: exact");
    ok &= Expect(bad_h == 0, "H = relu(Z): exact");
    ok &= Expect(bad_d == 0, "dZ = (dY W2^T) relu'(Z): exact");
  }

  // ---- forward with silu, Z not stored ------------------------------------
  CHECK_HIP(sb::MatmulActivation(sb::Matrix(m, k, d_x), false,
                                 sb::Matrix(k, n, d_w1), false, h,
                                 sb::Activation::kSilu, nullptr,
                                 sb::DataType::kF16, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  {
    const std::vector<float> hv = FromDevice(d_h, nnz);
    size_t bad = 0;
    for (size_t i = 0; i < nnz; ++i) {
      const double zz = z_ref[i];
      const double ref = zz / (1.0 + std::exp(-zz));
      bad += !(std::fabs(hv[i] - ref) <= std::fabs(ref) / 512 + 1.2e-7);
    }
    ok &= Expect(bad == 0, "H = silu(Z): within two fp16 steps");
  }

  sb::FreeRowIndicesBuffer(h);
  for (void *p : {(void *)d_x, (void *)d_w1, (void *)d_dy, (void *)d_w2,
                  (void *)d_h, (void *)d_z, (void *)d_dz, (void *)d_off,
                  (void *)d_idx})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(stream));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
