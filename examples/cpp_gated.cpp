// A C++ caller of the gated SDD products (sputnik/block/gated.h), the calls
// a GLU expert MLP y = (act(x w1) * (x v1)) w2 makes around its sparse
// hidden matrices:
//   forward   G = X W1 (plain SDD), H = (X V1) * relu(G), U = X V1 kept
//   backward  D = dY W2^T, dU = D * relu(G) written over U,
//             dG = D * U * relu'(G)
// Operands are -1 / 0 / 1 and K is 40, so every product and every gated value
// is an integer below 2048, exact in fp16, and relu is exact: U, H, dU and dG
// are checked bit for bit against host loops. A second forward with silu and
// no U is checked to one part in 2^9 (two fp16 steps). Built against
// libsputnik.so by sputnik_amd/Makefile; tests/test_cpp_gated.py runs it on
// the GPU. Exit status 0 = all passed.
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
  const int m = 384, n = 512, k = 40;
  std::mt19937 gen(13);
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

  std::vector<float> x((size_t)m * k), w1((size_t)k * n), v1((size_t)k * n),
      dy((size_t)m * k), w2((size_t)n * k);
  for (auto *v : {&x, &w1, &v1, &dy, &w2})
    for (auto &e : *v) e = (float)tri(gen);
  __half *d_x = ToDevice(ToHalf(x)), *d_w1 = ToDevice(ToHalf(w1));
  __half *d_v1 = ToDevice(ToHalf(v1));
  __half *d_dy = ToDevice(ToHalf(dy)), *d_w2 = ToDevice(ToHalf(w2));
  __half *d_h, *d_g, *d_u, *d_dg;
  CHECK_HIP(hipMalloc(&d_h, nnz * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_g, nnz * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_u, nnz * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_dg, nnz * sizeof(__half)));
  int *d_off = ToDevice(offsets);
  short *d_idx = ToDevice(indices);

  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  sb::BlockMatrix h(m, n, sb::AsBlockSize(kB), (int)nnz, d_h, d_off, d_idx);
  sb::AllocateRowIndicesBuffer(h);
  CHECK_HIP(sb::RowIndices(h, static_cast<short *>(h.row_indices), stream));
  sb::BlockMatrix g = h, dg = h;
  g.data = d_g;
  dg.data = d_dg;
  bool ok = true;

  // Host: G = X W1, U = X V1 and D = dY W2^T at the stored blocks (exact
  // integers).
  std::vector<float> g_ref(nnz), u_ref(nnz), d_ref(nnz);
  for (int r = 0; r < m / kB; ++r)
    for (int e = offsets[r]; e < offsets[r + 1]; ++e)
      for (int i = 0; i < kB; ++i)
        for (int j = 0; j < kB; ++j) {
          const int row = r * kB + i, col = indices[e] * kB + j;
          float gg = 0.f, uu = 0.f, dd = 0.f;
          for (int l = 0; l < k; ++l) {
            gg += x[(size_t)row * k + l] * w1[(size_t)l * n + col];
            uu += x[(size_t)row * k + l] * v1[(size_t)l * n + col];
            dd += dy[(size_t)row * k + l] * w2[(size_t)col * k + l];
          }
          const size_t at = ((size_t)e * kB + i) * kB + j;
          g_ref[at] = gg;
          u_ref[at] = uu;
          d_ref[at] = dd;
        }

  // ---- forward: G = X W1, then H = (X V1) * relu(G), U kept ---------------
  CHECK_HIP(sb::Matmul(sb::Matrix(m, k, d_x), false, sb::Matrix(k, n, d_w1),
                       false, g, sb::DataType::kF16, stream));
  CHECK_HIP(sb::MatmulGated(sb::Matrix(m, k, d_x), false,
                            sb::Matrix(k, n, d_v1), false, h,
                            sb::Activation::kRelu, d_g, d_u,
                            sb::DataType::kF16, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  {
    const std::vector<float> hv = FromDevice(d_h, nnz), uv = FromDevice(d_u, nnz);
    size_t bad_u = 0, bad_h = 0;
    for (size_t i = 0; i < nnz; ++i) {
      bad_u += uv[i] != u_ref[i];
      bad_h += hv[i] != (g_ref[i] > 0.f ? u_ref[i] * g_ref[i] : 0.f);
    }
    ok &= Expect(bad_u == 0, "U = X V1: exact");
    ok &= Expect(bad_h == 0, "H = U relu(G): exact");
  }

  // ---- backward: D = dY W2^T; dU over U, dG -------------------------------
  CHECK_HIP(sb::MatmulGatedGrad(sb::Matrix(m, k, d_dy), false,
                                sb::Matrix(n, k, d_w2), true, dg,
                                sb::Activation::kRelu, d_g, d_u, d_u,
                                sb::DataType::kF16, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  {
    const std::vector<float> gv = FromDevice(d_dg, nnz), uv = FromDevice(d_u, nnz);
    size_t bad_g = 0, bad_u = 0;
    for (size_t i = 0; i < nnz; ++i) {
      const bool on = g_ref[i] > 0.f;
      bad_u += uv[i] != (on ? d_ref[i] * g_ref[i] : 0.f);
      bad_g += gv[i] != (on ? d_ref[i] * u_ref[i] : 0.f);
    }
    ok &= Expect(bad_u == 0, "dU = D relu(G), in place over U: exact");
    ok &= Expect(bad_g == 0, "dG = D U relu'(G): exact");
  }

  // ---- a buffer that must not alias is rejected ---------------------------
  ok &= Expect(sb::MatmulGated(sb::Matrix(m, k, d_x), false,
                               sb::Matrix(k, n, d_v1), false, h,
                               sb::Activation::kRelu, d_g, d_h,
                               sb::DataType::kF16, stream) ==
                   hipErrorInvalidValue,
               "up == c.data: hipErrorInvalidValue");

  // ---- forward with silu, U not stored ------------------------------------
  CHECK_HIP(sb::MatmulGated(sb::Matrix(m, k, d_x), false,
                            sb::Matrix(k, n, d_v1), false, h,
                            sb::Activation::kSilu, d_g, nullptr,
                            sb::DataType::kF16, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  {
    const std::vector<float> hv = FromDevice(d_h, nnz);
    size_t bad = 0;
    for (size_t i = 0; i < nnz; ++i) {
      const double gg = g_ref[i];
      const double ref = u_ref[i] * (gg / (1.0 + std::exp(-gg)));
      bad += !(std::fabs(hv[i] - ref) <= std::fabs(ref) / 512 + 1.2e-7);
    }
    ok &= Expect(bad == 0, "H = U silu(G): within two fp16 steps");
  }

  sb::FreeRowIndicesBuffer(h);
  for (void *p : {(void *)d_x, (void *)d_w1, (void *)d_v1, (void *)d_dy,
                  (void *)d_w2, (void *)d_h, (void *)d_g, (void *)d_u,
                  (void *)d_dg, (void *)d_off, (void *)d_idx})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(stream));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
