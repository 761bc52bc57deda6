// A C++ caller of the accumulating products (sputnik/block/accumulate.h): one
// DSD and one DDS, C += op(A) op(B) into an fp32 C that already holds values.
// Operands are -1 / 0 / 1 and C starts from small integers, so the result is
// exact and every element is checked against a host dot product; block-rows
// (DSD) and block-columns (DDS) without blocks must keep C bit for bit. Built
// against libsputnik.so by sputnik_amd/Makefile; tests/test_cpp_accumulate.py
// runs it on the GPU. Exit status 0 = all passed.
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

}  // namespace

int main() {
  // S is 512 x 384 in 128 x 128 blocks, block-row 2 empty; D is dense.
  const int sr = 512, sc = 384, n = 264;
  std::mt19937 gen(7);
  std::uniform_int_distribution<int> tri(-1, 1), c0(-8, 8);
  std::bernoulli_distribution keep(0.6);

  std::vector<int> offsets{0};
  std::vector<short> indices;
  for (int r = 0; r < sr / kB; ++r) {
    for (int c = 0; c < sc / kB; ++c)
      if (r != 2 && (keep(gen) || c == r % (sc / kB))) indices.push_back((short)c);
    offsets.push_back((int)indices.size());
  }
  const int nb = (int)indices.size();
  std::vector<float> blocks((size_t)nb * kB * kB), s_dense((size_t)sr * sc, 0.f);
  for (auto &v : blocks) v = (float)tri(gen);
  for (int r = 0; r < sr / kB; ++r)
    for (int e = offsets[r]; e < offsets[r + 1]; ++e)
      for (int i = 0; i < kB; ++i)
        for (int j = 0; j < kB; ++j)
          s_dense[(size_t)(r * kB + i) * sc + indices[e] * kB + j] =
              blocks[((size_t)e * kB + i) * kB + j];

  __half *d_blocks = ToDevice(ToHalf(blocks));
  int *d_off = ToDevice(offsets);
  short *d_idx = ToDevice(indices);
  sb::BlockMatrix s(sr, sc, sb::AsBlockSize(kB), nb * kB * kB, d_blocks, d_off,
                    d_idx);
  sb::AllocateTransposeBuffers(s);
  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  bool ok = true;

  // ---- DSD: C[512 x 264] += S B, B [384 x 264] ----------------------------
  {
    std::vector<float> b((size_t)sc * n), c((size_t)sr * n);
    for (auto &v : b) v = (float)tri(gen);
    for (auto &v : c) v = (float)c0(gen);
    __half *d_b = ToDevice(ToHalf(b));
    float *d_c = ToDevice(c);
    CHECK_HIP(sb::MatmulAccumulate(s, false, sb::Matrix(sc, n, d_b), false,
                                   sb::Matrix(sr, n, d_c), sb::DataType::kF16,
                                   sb::OutputType::kF32, stream));
    CHECK_HIP(hipStreamSynchronize(stream));
    std::vector<float> out(c.size());
    CHECK_HIP(hipMemcpy(out.data(), d_c, out.size() * sizeof(float),
                        hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (int i = 0; i < sr; ++i)
      for (int j = 0; j < n; ++j) {
        double sum = c[(size_t)i * n + j];
        for (int l = 0; l < sc; ++l)
          sum += (double)s_dense[(size_t)i * sc + l] * b[(size_t)l * n + j];
        bad += out[(size_t)i * n + j] != (float)sum;
      }
    ok &= Expect(bad == 0, "dsd accumulate into fp32: exact");
    CHECK_HIP(hipFree(d_b));
    CHECK_HIP(hipFree(d_c));
  }

  // ---- DDS: C[264 x 512] += A S^T, A [264 x 384] --------------------------
  // (op(B) = S^T: its empty block-column is S's empty block-row 2)
  {
    std::vector<float> a((size_t)n * sc), c((size_t)n * sr);
    for (auto &v : a) v = (float)tri(gen);
    for (auto &v : c) v = (float)c0(gen);
    __half *d_a = ToDevice(ToHalf(a));
    float *d_c = ToDevice(c);
    CHECK_HIP(sb::MatmulAccumulate(sb::Matrix(n, sc, d_a), false, s, true,
                                   sb::Matrix(n, sr, d_c), sb::DataType::kF16,
                                   sb::OutputType::kF32, stream));
    CHECK_HIP(hipStreamSynchronize(stream));
    std::vector<float> out(c.size());
    CHECK_HIP(hipMemcpy(out.data(), d_c, out.size() * sizeof(float),
                        hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < sr; ++j) {
        double sum = c[(size_t)i * sr + j];
        for (int l = 0; l < sc; ++l)
          sum += (double)a[(size_t)i * sc + l] * s_dense[(size_t)j * sc + l];
        bad += out[(size_t)i * sr + j] != (float)sum;
      }
    ok &= Expect(bad == 0, "dds accumulate into fp32: exact");
    CHECK_HIP(hipFree(d_a));
    CHECK_HIP(hipFree(d_c));
  }

  sb::FreeTransposeBuffers(s);
  for (void *p : {(void *)d_blocks, (void *)d_off, (void *)d_idx})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(stream));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
