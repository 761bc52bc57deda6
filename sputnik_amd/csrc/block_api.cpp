// sputnik-amd: the sputnik::block C++ overload set (drop-in for the
// reference's), over the Run* entry points of dispatch.cpp.
#include <cstdint>
#include <initializer_list>

#include "api_internal.h"
#include "dispatch_internal.h"
#include "metadata.h"
#include "sputnik/sputnik.h"

namespace sputnik_amd {
namespace {

// C++ API convention: abort where the reference aborts.
hipError_t OrAbort(Status st, const char *op) {
  switch (st) {
    case Status::kOk: return hipSuccess;
    case Status::kNotSupported: return hipErrorNotSupported;
    case Status::kNoKernel:
      SPUTNIK_LOG(FATAL) << "No compatible kernel for " << op << " problem.";
      break;
    case Status::kMissingMetadata:
      SPUTNIK_LOG(FATAL) << "Check failed: offsets_t && indices_t && "
                            "block_offsets (" << op << ")";
      break;
    case Status::kMissingRowIndices:
      SPUTNIK_LOG(FATAL) << "Check failed: c.row_indices (" << op << ")";
      break;
  }
  return hipErrorUnknown;
}

}  // namespace
}  // namespace sputnik_amd

// ---- C++ API (drop-in for the reference's sputnik::block) ---------------

namespace sputnik {
namespace block {

using sputnik_amd::Status;

hipError_t Matmul(const BlockMatrix a, bool transpose_a, const Matrix b,
                  bool transpose_b, Matrix c, DataType dtype,
                  hipStream_t stream) {
  Status st;
  const hipError_t e =
      sputnik_amd::RunDsd(a, transpose_a, b, transpose_b, c, (int)dtype,
                          stream, &st);
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, "dsd");
}

hipError_t MatmulEx(const BlockMatrix a, bool transpose_a, const Matrix b,
                    bool transpose_b, Matrix c, DataType dtype,
                    hipStream_t stream) {
  BlockMatrix acp = a;
  acp.create_metadata = false;
  return Matmul(acp, transpose_a, b, transpose_b, c, dtype, stream);
}

hipError_t Matmul(const BlockMatrix a, bool transpose_a, const Matrix b,
                  bool transpose_b, Matrix c, hipStream_t stream) {
  return Matmul(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

hipError_t MatmulEx(const BlockMatrix a, bool transpose_a, const Matrix b,
                    bool transpose_b, Matrix c, hipStream_t stream) {
  return MatmulEx(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

hipError_t Matmul(const Matrix a, bool transpose_a, const BlockMatrix b,
                  bool transpose_b, Matrix c, DataType dtype,
                  hipStream_t stream) {
  Status st;
  const hipError_t e =
      sputnik_amd::RunDds(a, transpose_a, b, transpose_b, c, (int)dtype,
                          stream, &st);
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, "dds");
}

hipError_t MatmulEx(const Matrix a, bool transpose_a, const BlockMatrix b,
                    bool transpose_b, Matrix c, DataType dtype,
                    hipStream_t stream) {
  BlockMatrix bcp = b;
  bcp.create_metadata = false;
  return Matmul(a, transpose_a, bcp, transpose_b, c, dtype, stream);
}

hipError_t Matmul(const Matrix a, bool transpose_a, const BlockMatrix b,
                  bool transpose_b, Matrix c, hipStream_t stream) {
  return Matmul(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

hipError_t MatmulEx(const Matrix a, bool transpose_a, const BlockMatrix b,
                    bool transpose_b, Matrix c, hipStream_t stream) {
  return MatmulEx(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

// ---- accumulating DSD / DDS (sputnik/block/accumulate.h) ----

static sputnik_amd::OutMode AccMode(OutputType c_type) {
  return c_type == OutputType::kF32 ? sputnik_amd::OutMode::kAccF32
                                    : sputnik_amd::OutMode::kAccT;
}

hipError_t MatmulAccumulate(const BlockMatrix a, bool transpose_a,
                            const Matrix b, bool transpose_b, Matrix c,
                            DataType dtype, OutputType c_type,
                            hipStream_t stream) {
  Status st;
  const hipError_t e = sputnik_amd::RunDsd(
      a, transpose_a, b, transpose_b, c, (int)dtype, stream, &st,
      sputnik_amd::Workspace{}, AccMode(c_type));
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, "dsd (accumulate)");
}

hipError_t MatmulAccumulateEx(const BlockMatrix a, bool transpose_a,
                              const Matrix b, bool transpose_b, Matrix c,
                              DataType dtype, OutputType c_type,
                              hipStream_t stream) {
  BlockMatrix acp = a;
  acp.create_metadata = false;
  return MatmulAccumulate(acp, transpose_a, b, transpose_b, c, dtype, c_type,
                          stream);
}

hipError_t MatmulAccumulate(const Matrix a, bool transpose_a,
                            const BlockMatrix b, bool transpose_b, Matrix c,
                            DataType dtype, OutputType c_type,
                            hipStream_t stream) {
  Status st;
  const hipError_t e = sputnik_amd::RunDds(
      a, transpose_a, b, transpose_b, c, (int)dtype, stream, &st,
      AccMode(c_type));
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, "dds (accumulate)");
}

hipError_t MatmulAccumulateEx(const Matrix a, bool transpose_a,
                              const BlockMatrix b, bool transpose_b, Matrix c,
                              DataType dtype, OutputType c_type,
                              hipStream_t stream) {
  BlockMatrix bcp = b;
  bcp.create_metadata = false;
  return MatmulAccumulate(a, transpose_a, bcp, transpose_b, c, dtype, c_type,
                          stream);
}

hipError_t Matmul(const Matrix a, bool transpose_a, const Matrix b,
                  bool transpose_b, BlockMatrix c, DataType dtype,
                  hipStream_t stream) {
  Status st;
  const hipError_t e = sputnik_amd::RunSdd(a, transpose_a, b, transpose_b, c,
                                           (int)dtype, stream, &st);
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, "sdd");
}

hipError_t Matmul(const Matrix a, bool transpose_a, const Matrix b,
                  bool transpose_b, BlockMatrix c, hipStream_t stream) {
  return Matmul(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

// ---- SDD epilogue products (sputnik/block/activation.h, gated.h) ----

static hipError_t MatmulEpilogue(const char *what, const Matrix &a, bool ta,
                                 const Matrix &b, bool tb,
                                 const BlockMatrix &c, Activation activation,
                                 int mode, const void *side0,
                                 const void *side1, void *out1, DataType dtype,
                                 hipStream_t stream) {
  Status st;
  const hipError_t e = sputnik_amd::RunSddEpilogue(
      a, ta, b, tb, c, (int)dtype, (int)activation, mode,
      const_cast<void *>(side0), const_cast<void *>(side1), out1, stream, &st);
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, what);
}

hipError_t MatmulActivation(const Matrix a, bool transpose_a, const Matrix b,
                            bool transpose_b, BlockMatrix c,
                            Activation activation, void *pre_activation,
                            DataType dtype, hipStream_t stream) {
  return MatmulEpilogue("sdd (activation)", a, transpose_a, b, transpose_b, c,
                        activation, sputnik_amd::kOutAct, pre_activation,
                        nullptr, nullptr, dtype, stream);
}

hipError_t MatmulActivationGrad(const Matrix a, bool transpose_a,
                                const Matrix b, bool transpose_b,
                                BlockMatrix c, Activation activation,
                                const void *pre_activation, DataType dtype,
                                hipStream_t stream) {
  return MatmulEpilogue("sdd (activation grad)", a, transpose_a, b,
                        transpose_b, c, activation, sputnik_amd::kOutActGrad,
                        pre_activation, nullptr, nullptr, dtype, stream);
}

hipError_t MatmulGated(const Matrix a, bool transpose_a, const Matrix b,
                       bool transpose_b, BlockMatrix c, Activation activation,
                       const void *gate, void *up, DataType dtype,
                       hipStream_t stream) {
  return MatmulEpilogue("sdd (gated)", a, transpose_a, b, transpose_b, c,
                        activation, sputnik_amd::kOutGate, gate, up, nullptr,
                        dtype, stream);
}

hipError_t MatmulGatedGrad(const Matrix a, bool transpose_a, const Matrix b,
                           bool transpose_b, BlockMatrix c,
                           Activation activation, const void *gate,
                           const void *up, void *up_grad, DataType dtype,
                           hipStream_t stream) {
  return MatmulEpilogue("sdd (gated grad)", a, transpose_a, b, transpose_b, c,
                        activation, sputnik_amd::kOutGateGrad, gate, up,
                        up_grad, dtype, stream);
}

// ---- SDD with a column bias, column sums (sputnik/block/bias.h) ----

static hipError_t MatmulBiasEpilogue(const char *what, const Matrix &a,
                                     bool ta, const Matrix &b, bool tb,
                                     const BlockMatrix &c, const void *bias,
                                     int act, int mode, const void *side0,
                                     void *side1, DataType dtype,
                                     hipStream_t stream) {
  Status st;
  const hipError_t e = sputnik_amd::RunSddEpilogueBias(
      a, ta, b, tb, c, (int)dtype, act, mode, const_cast<void *>(side0),
      side1, bias, stream, &st);
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, what);
}

hipError_t MatmulBias(const Matrix a, bool transpose_a, const Matrix b,
                      bool transpose_b, BlockMatrix c, const void *bias,
                      DataType dtype, hipStream_t stream) {
  return MatmulBiasEpilogue("sdd (bias)", a, transpose_a, b, transpose_b, c,
                            bias, 0, sputnik_amd::kOutBias, nullptr, nullptr,
                            dtype, stream);
}

hipError_t MatmulBiasActivation(const Matrix a, bool transpose_a,
                                const Matrix b, bool transpose_b,
                                BlockMatrix c, const void *bias,
                                Activation activation, void *pre_activation,
                                DataType dtype, hipStream_t stream) {
  return MatmulBiasEpilogue("sdd (bias, activation)", a, transpose_a, b,
                            transpose_b, c, bias, (int)activation,
                            sputnik_amd::kOutAct, pre_activation, nullptr,
                            dtype, stream);
}

hipError_t MatmulBiasGated(const Matrix a, bool transpose_a, const Matrix b,
                           bool transpose_b, BlockMatrix c, const void *bias,
                           Activation activation, const void *gate, void *up,
                           DataType dtype, hipStream_t stream) {
  return MatmulBiasEpilogue("sdd (bias, gated)", a, transpose_a, b,
                            transpose_b, c, bias, (int)activation,
                            sputnik_amd::kOutGate, gate, up, dtype, stream);
}

hipError_t BlockColumnSum(const BlockMatrix s, DataType dtype, float *out,
                          hipStream_t stream) {
  return sputnik_amd::RunBlockColumnSum(s, (int)dtype, out, stream);
}

// SSD (reference sputnik/block/ssd/ssd.h:10-22) and SDS (sds.h:10-22).
hipError_t Matmul(const BlockMatrix a, bool transpose_a, const Matrix b,
                  bool transpose_b, BlockMatrix c, DataType dtype,
                  hipStream_t stream) {
  Status st;
  const hipError_t e =
      sputnik_amd::RunSsd(a, transpose_a, b, transpose_b, c, (int)dtype,
                          stream, &st);
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, "ssd");
}

hipError_t MatmulEx(const BlockMatrix a, bool transpose_a, const Matrix b,
                    bool transpose_b, BlockMatrix c, DataType dtype,
                    hipStream_t stream) {
  BlockMatrix acp = a;
  acp.create_metadata = false;
  return Matmul(acp, transpose_a, b, transpose_b, c, dtype, stream);
}

hipError_t Matmul(const BlockMatrix a, bool transpose_a, const Matrix b,
                  bool transpose_b, BlockMatrix c, hipStream_t stream) {
  return Matmul(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

hipError_t MatmulEx(const BlockMatrix a, bool transpose_a, const Matrix b,
                    bool transpose_b, BlockMatrix c, hipStream_t stream) {
  return MatmulEx(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

hipError_t Matmul(const Matrix a, bool transpose_a, const BlockMatrix b,
                  bool transpose_b, BlockMatrix c, DataType dtype,
                  hipStream_t stream) {
  Status st;
  const hipError_t e =
      sputnik_amd::RunSds(a, transpose_a, b, transpose_b, c, (int)dtype,
                          stream, &st);
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, "sds");
}

hipError_t MatmulEx(const Matrix a, bool transpose_a, const BlockMatrix b,
                    bool transpose_b, BlockMatrix c, DataType dtype,
                    hipStream_t stream) {
  BlockMatrix bcp = b;
  bcp.create_metadata = false;
  return Matmul(a, transpose_a, bcp, transpose_b, c, dtype, stream);
}

hipError_t Matmul(const Matrix a, bool transpose_a, const BlockMatrix b,
                  bool transpose_b, BlockMatrix c, hipStream_t stream) {
  return Matmul(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

hipError_t MatmulEx(const Matrix a, bool transpose_a, const BlockMatrix b,
                    bool transpose_b, BlockMatrix c, hipStream_t stream) {
  return MatmulEx(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

// DSS (reference sputnik/block/dss/dss.h:10-22).
hipError_t Matmul(const BlockMatrix a, bool transpose_a, const BlockMatrix b,
                  bool transpose_b, Matrix c, DataType dtype,
                  hipStream_t stream) {
  Status st;
  const hipError_t e = sputnik_amd::RunDss(a, transpose_a, b, transpose_b, c,
                                           (int)dtype, stream, &st);
  return st == Status::kOk ? e : sputnik_amd::OrAbort(st, "dss");
}

hipError_t MatmulEx(const BlockMatrix a, bool transpose_a, const BlockMatrix b,
                    bool transpose_b, Matrix c, DataType dtype,
                    hipStream_t stream) {
  BlockMatrix acp = a, bcp = b;
  acp.create_metadata = false;
  bcp.create_metadata = false;
  return Matmul(acp, transpose_a, bcp, transpose_b, c, dtype, stream);
}

hipError_t Matmul(const BlockMatrix a, bool transpose_a, const BlockMatrix b,
                  bool transpose_b, Matrix c, hipStream_t stream) {
  return Matmul(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

hipError_t MatmulEx(const BlockMatrix a, bool transpose_a, const BlockMatrix b,
                    bool transpose_b, Matrix c, hipStream_t stream) {
  return MatmulEx(a, transpose_a, b, transpose_b, c, DataType::kF16, stream);
}

// Caller-owned workspaces (sputnik/block/workspace.h).
hipError_t SetStreamWorkspace(hipStream_t stream, void *ptr, size_t bytes) {
  return sputnik_amd::SetStreamWorkspace(stream, ptr, bytes);
}

size_t SddWorkspaceBytes(const Matrix a, bool transpose_a, const Matrix b,
                         bool transpose_b, const BlockMatrix c) {
  return sputnik_amd::SddWorkspaceBytes(a, transpose_a, b, transpose_b, c);
}

size_t DsdWorkspaceBytes(const BlockMatrix a, bool transpose_a, const Matrix b,
                         bool transpose_b, const Matrix c) {
  return sputnik_amd::DsdWorkspaceBytes(a, transpose_a, b, transpose_b, c);
}

size_t RetainedBytes() { return sputnik_amd::RetainedBytes(); }

size_t ReleaseWorkspaces() { return sputnik_amd::ReleaseWorkspaces(); }

hipError_t RowIndices(BlockMatrix a, short *row_indices, hipStream_t stream) {
  if (AsInt(a.block_size) == 0) return hipErrorNotSupported;
  return sputnik_amd::LaunchRowIndices(a.rows / AsInt(a.block_size),
                                       static_cast<const int *>(a.offsets),
                                       row_indices, stream);
}

hipError_t Bitmask(BlockMatrix m, hipStream_t stream) {
  // bitmask.cu:8-16: the orientation follows offsets_t.
  const bool trans = m.offsets_t != nullptr;
  const int b = AsInt(m.block_size);
  if (b == 0) return hipErrorNotSupported;
  SPUTNIK_CHECK(m.bitmask);
  const int block_rows = (trans ? m.cols : m.rows) / b;
  const int block_cols = (trans ? m.rows : m.cols) / b;
  return sputnik_amd::LaunchBitmask(
      block_rows, block_cols,
      static_cast<const int *>(trans ? m.offsets_t : m.offsets),
      static_cast<const short *>(trans ? m.indices_t : m.indices),
      static_cast<unsigned long long *>(m.bitmask), stream);
}

// ---- fp8 products (sputnik/block/fp8.h): never abort ----

namespace {

bool Fp8SizesOk(const BlockMatrix &s, int other, int dtype) {
  return s.block_size == BlockSize::k128 && s.rows >= 0 && s.cols >= 0 &&
         s.nonzeros >= 0 && other >= 0 && s.rows % 128 == 0 &&
         s.cols % 128 == 0 && other % 128 == 0 &&
         s.nonzeros % (128 * 128) == 0 && (dtype == 0 || dtype == 1);
}

// (the DMA, the fragment reads and the output stores move 16 bytes)
bool Aligned16(std::initializer_list<const void *> ps) {
  uintptr_t bits = 0;
  for (const void *p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15) == 0;
}

bool Fp8AccumulateOk(Fp8Accumulate accumulate) {
  return accumulate == Fp8Accumulate::kFp32 ||
         accumulate == Fp8Accumulate::kFast;
}

}  // namespace

hipError_t SddFp8(const void *aq, const float *a_scales, int k,
                  const void *bq, const float *b_scales, BlockMatrix c,
                  DataType dtype, hipStream_t stream) {
  return SddFp8(aq, a_scales, k, bq, b_scales, c, dtype, Fp8Accumulate::kFp32,
                stream);
}

hipError_t SddFp8(const void *aq, const float *a_scales, int k,
                  const void *bq, const float *b_scales, BlockMatrix c,
                  DataType dtype, Fp8Accumulate accumulate,
                  hipStream_t stream) {
  if (!Fp8AccumulateOk(accumulate)) return hipErrorInvalidValue;
  if (!Fp8SizesOk(c, k, (int)dtype)) return hipErrorInvalidValue;
  if (c.nonzeros == 0) return hipSuccess;
  if (c.data == nullptr || c.indices == nullptr || c.row_indices == nullptr ||
      (k > 0 && (aq == nullptr || a_scales == nullptr || bq == nullptr ||
                 b_scales == nullptr)))
    return hipErrorInvalidValue;
  for (const void *in : {aq, (const void *)a_scales, bq,
                         (const void *)b_scales, (const void *)c.indices,
                         (const void *)c.row_indices})
    if (c.data == in) return hipErrorInvalidValue;
  if (!Aligned16({aq, bq, c.data})) return hipErrorInvalidValue;
  return sputnik_amd::LaunchFp8Gemm(
      false, accumulate == Fp8Accumulate::kFast, (int)dtype, aq, a_scales, bq, b_scales, c.data, nullptr,
      static_cast<const short *>(c.indices),
      static_cast<const short *>(c.row_indices), c.rows / 128, c.cols / 128,
      k / 128, c.nonzeros / (128 * 128), stream);
}

hipError_t DsdFp8(const BlockMatrix s, const float *s_scales, const void *bq,
                  const float *b_scales, Matrix c, DataType dtype,
                  hipStream_t stream) {
  return DsdFp8(s, s_scales, bq, b_scales, c, dtype, Fp8Accumulate::kFp32,
                stream);
}

hipError_t DsdFp8(const BlockMatrix s, const float *s_scales, const void *bq,
                  const float *b_scales, Matrix c, DataType dtype,
                  Fp8Accumulate accumulate, hipStream_t stream) {
  if (!Fp8AccumulateOk(accumulate)) return hipErrorInvalidValue;
  if (!Fp8SizesOk(s, c.cols, (int)dtype) || c.rows != s.rows)
    return hipErrorInvalidValue;
  if (c.rows == 0 || c.cols == 0) return hipSuccess;
  if (c.data == nullptr || s.offsets == nullptr ||
      (s.nonzeros > 0 && (s.data == nullptr || s.indices == nullptr ||
                          s_scales == nullptr || bq == nullptr ||
                          b_scales == nullptr)))
    return hipErrorInvalidValue;
  for (const void *in : {(const void *)s.data, (const void *)s_scales, bq,
                         (const void *)b_scales, (const void *)s.offsets,
                         (const void *)s.indices})
    if (c.data == in) return hipErrorInvalidValue;
  if (!Aligned16({s.data, bq, c.data})) return hipErrorInvalidValue;
  return sputnik_amd::LaunchFp8Gemm(
      true, accumulate == Fp8Accumulate::kFast, (int)dtype, s.data, s_scales,
      bq, b_scales, c.data, static_cast<const int *>(s.offsets),
      static_cast<const short *>(s.indices), nullptr, s.rows / 128,
      c.cols / 128, s.cols / 128, s.nonzeros / (128 * 128), stream);
}

hipError_t DsdFp8Wgrad(const BlockMatrix s, const float *s_scales,
                       const void *bq, const float *b_scales, Matrix c,
                       DataType dtype, OutputType out, bool add,
                       Fp8Accumulate accumulate, hipStream_t stream) {
  if (!Fp8AccumulateOk(accumulate)) return hipErrorInvalidValue;
  if (out != OutputType::kOperand && out != OutputType::kF32)
    return hipErrorInvalidValue;
  if (!Fp8SizesOk(s, c.cols, (int)dtype) || c.rows != s.rows)
    return hipErrorInvalidValue;
  if (c.rows == 0 || c.cols == 0) return hipSuccess;
  if (c.data == nullptr || s.offsets == nullptr ||
      (s.nonzeros > 0 && (s.data == nullptr || s.indices == nullptr ||
                          s_scales == nullptr || bq == nullptr ||
                          b_scales == nullptr)))
    return hipErrorInvalidValue;
  for (const void *in : {(const void *)s.data, (const void *)s_scales, bq,
                         (const void *)b_scales, (const void *)s.offsets,
                         (const void *)s.indices})
    if (c.data == in) return hipErrorInvalidValue;
  if (!Aligned16({s.data, bq, c.data})) return hipErrorInvalidValue;
  return sputnik_amd::LaunchFp8Wgrad(
      accumulate == Fp8Accumulate::kFast, (int)dtype, out == OutputType::kF32,
      add, s.data, s_scales, bq, b_scales, c.data,
      static_cast<const int *>(s.offsets),
      static_cast<const short *>(s.indices), s.rows / 128, c.cols / 128,
      s.cols / 128, s.nonzeros / (128 * 128), stream);
}

hipError_t Fp8IntervalSums(const void *aq, const void *bq, int m, int n,
                           int k, Fp8Accumulate accumulate, float *p,
                           hipStream_t stream) {
  if (!Fp8AccumulateOk(accumulate)) return hipErrorInvalidValue;
  if (m < 0 || n < 0 || k < 0 || m % 128 != 0 || n % 128 != 0 ||
      k % 128 != 0)
    return hipErrorInvalidValue;
  if (m == 0 || n == 0 || k == 0) return hipSuccess;
  if (aq == nullptr || bq == nullptr || p == nullptr)
    return hipErrorInvalidValue;
  if (p == aq || p == bq) return hipErrorInvalidValue;
  if (!Aligned16({aq, bq, p})) return hipErrorInvalidValue;
  return sputnik_amd::LaunchFp8IntervalSums(
      aq, bq, m, n, k, accumulate == Fp8Accumulate::kFast, p, stream);
}

hipError_t Transpose(BlockMatrix a, hipStream_t stream) {
  // transpose.cu:107-109 checks the three workspaces; with no nonzero block
  // the two per-block ones are legitimately empty.
  SPUTNIK_CHECK(a.offsets_t);
  if (a.nonzeros > 0) {
    SPUTNIK_CHECK(a.indices_t);
    SPUTNIK_CHECK(a.block_offsets);
  }
  return sputnik_amd::BuildTransposed(a, stream);
}

}  // namespace block
}  // namespace sputnik

