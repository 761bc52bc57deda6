// A C++ caller bound to the reference's fixed Matmul signature that owns the
// transposed-B workspace (sputnik/block/workspace.h): it asks for the size,
// registers its own device memory for a stream, and checks that the library
// then holds no memory of its own; a second stream with a registration that
// is too small keeps the NT kernel; after unregistering, the library-owned
// buffer appears in RetainedBytes() and ReleaseWorkspaces() returns it.
// Operand values are -1 / 0 / 1, so every route must give the same bits, and
// sampled elements are checked against a host dot product. Built against
// libsputnik.so by sputnik_amd/Makefile; tests/test_cpp_workspace.py runs it
// on the GPU. Exit status 0 = all passed.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

std::vector<__half> FromDevice(const __half *d, size_t n) {
  std::vector<__half> t(n);
  CHECK_HIP(hipMemcpy(t.data(), d, n * sizeof(__half), hipMemcpyDeviceToHost));
  return t;
}

bool SameBits(const std::vector<__half> &x, const std::vector<__half> &y) {
  return x.size() == y.size() &&
         std::memcmp(x.data(), y.data(), x.size() * sizeof(__half)) == 0;
}

}  // namespace

int main() {
  // The path's size gate from 1 MiB of B on (default: 256 MiB), read by the
  // library on its first call.
  setenv("SPUTNIK_AMD_SDD_BT_MIN_MIB", "1", 1);
  const int m = 8192, k = 256, n = 4096;
  std::mt19937 gen(11);
  std::uniform_int_distribution<int> tri(-1, 1);
  std::bernoulli_distribution keep(0.7);

  std::vector<float> a((size_t)m * k), bt((size_t)n * k);  // B^T stored [N][K]
  for (auto &v : a) v = (float)tri(gen);
  for (auto &v : bt) v = (float)tri(gen);
  std::vector<__half> ha(a.size()), hbt(bt.size());
  for (size_t i = 0; i < a.size(); ++i) ha[i] = __float2half(a[i]);
  for (size_t i = 0; i < bt.size(); ++i) hbt[i] = __float2half(bt[i]);
  std::vector<int> offsets{0};
  std::vector<short> indices;
  for (int r = 0; r < m / kB; ++r) {
    for (int c = 0; c < n / kB; ++c)
      if (keep(gen)) indices.push_back((short)c);
    offsets.push_back((int)indices.size());
  }
  const int nb = (int)indices.size();
  const size_t out_elems = (size_t)nb * kB * kB;

  __half *d_a = ToDevice(ha), *d_bt = ToDevice(hbt), *d_c = nullptr;
  int *d_off = ToDevice(offsets);
  short *d_idx = ToDevice(indices);
  CHECK_HIP(hipMalloc(&d_c, out_elems * sizeof(__half)));
  sb::BlockMatrix sc(m, n, sb::AsBlockSize(kB), nb * kB * kB, d_c, d_off, d_idx);
  sb::AllocateRowIndicesBuffer(sc);
  hipStream_t s1, s2;
  CHECK_HIP(hipStreamCreate(&s1));
  CHECK_HIP(hipStreamCreate(&s2));
  CHECK_HIP(sb::RowIndices(sc, static_cast<short *>(sc.row_indices), s1));
  CHECK_HIP(hipStreamSynchronize(s1));
  sb::Matrix ma(m, k, d_a), mbt(n, k, d_bt);

  bool ok = true;
  const size_t base = sb::RetainedBytes();
  const size_t need = sb::SddWorkspaceBytes(ma, false, mbt, true, sc);
  ok &= Expect(need == (size_t)n * k * 2, "SddWorkspaceBytes = K N 2");
  ok &= Expect(sb::SddWorkspaceBytes(ma, false, sb::Matrix(k, n, d_bt), false, sc) == 0,
               "SddWorkspaceBytes(NN) = 0");

  // ---- the caller's memory, registered for s1 ---------------------------
  char *ws = nullptr, *small = nullptr;
  CHECK_HIP(hipMalloc(&ws, need));
  CHECK_HIP(hipMalloc(&small, 256));
  ok &= Expect(sb::SetStreamWorkspace(s1, ws + 8, need - 8) == hipErrorInvalidValue,
               "misaligned pointer rejected");
  ok &= Expect(sb::SetStreamWorkspace(s1, ws, 0) == hipErrorInvalidValue,
               "zero size rejected");
  CHECK_HIP(sb::SetStreamWorkspace(s1, ws, need));
  CHECK_HIP(hipMemsetAsync(d_c, 0xff, out_elems * sizeof(__half), s1));
  CHECK_HIP(sb::Matmul(ma, false, mbt, true, sc, s1));
  CHECK_HIP(hipStreamSynchronize(s1));
  const std::vector<__half> r1 = FromDevice(d_c, out_elems);
  ok &= Expect(sb::RetainedBytes() == base, "registered stream: nothing retained");

  // sampled elements against a host dot product (exact: integers)
  size_t bad = 0;
  std::uniform_int_distribution<size_t> pick(0, out_elems - 1);
  std::vector<int> row_of(nb);
  for (int r = 0; r < m / kB; ++r)
    for (int e = offsets[r]; e < offsets[r + 1]; ++e) row_of[e] = r;
  for (int t = 0; t < 4096; ++t) {
    const size_t at = pick(gen);
    const int e = (int)(at / (kB * kB)), i = (int)(at / kB % kB), j = (int)(at % kB);
    const size_t row = (size_t)row_of[e] * kB + i, col = (size_t)indices[e] * kB + j;
    double sum = 0;
    for (int l = 0; l < k; ++l) sum += (double)a[row * k + l] * bt[col * k + l];
    bad += __half2float(r1[at]) != (float)sum;
  }
  ok &= Expect(bad == 0, "sampled elements exact");

  // ---- a registration that is too small keeps the NT kernel --------------
  CHECK_HIP(sb::SetStreamWorkspace(s2, small, 256));
  CHECK_HIP(hipMemsetAsync(d_c, 0xff, out_elems * sizeof(__half), s2));
  CHECK_HIP(sb::Matmul(ma, false, mbt, true, sc, s2));
  CHECK_HIP(hipStreamSynchronize(s2));
  ok &= Expect(SameBits(FromDevice(d_c, out_elems), r1), "small workspace: same bits");
  ok &= Expect(sb::RetainedBytes() == base, "small workspace: nothing retained");

  // ---- unregistered: the library's own buffer, seen and returned ---------
  CHECK_HIP(sb::SetStreamWorkspace(s1, nullptr, 0));
  CHECK_HIP(sb::SetStreamWorkspace(s2, nullptr, 0));
  CHECK_HIP(hipMemsetAsync(d_c, 0xff, out_elems * sizeof(__half), s1));
  CHECK_HIP(sb::Matmul(ma, false, mbt, true, sc, s1));
  CHECK_HIP(hipStreamSynchronize(s1));
  ok &= Expect(SameBits(FromDevice(d_c, out_elems), r1), "library route: same bits");
  const size_t held = sb::RetainedBytes();
  ok &= Expect(held >= base + (size_t)n * k * 2, "library route: buffer retained");
  const size_t freed = sb::ReleaseWorkspaces();
  ok &= Expect(freed == held - sb::RetainedBytes() && freed >= (size_t)n * k * 2,
               "ReleaseWorkspaces returns what it freed");
  ok &= Expect(sb::ReleaseWorkspaces() == 0, "second release frees nothing");

  sb::FreeRowIndicesBuffer(sc);
  for (void *p : {(void *)d_a, (void *)d_bt, (void *)d_c, (void *)d_off,
                  (void *)d_idx, (void *)ws, (void *)small})
    CHECK_HIP(hipFree(p));
  CHECK_HIP(hipStreamDestroy(s1));
  CHECK_HIP(hipStreamDestroy(s2));
  std::printf("%s\n", ok ? "ALL OK" : "FAILED");
  return ok ? 0 : 1;
}
