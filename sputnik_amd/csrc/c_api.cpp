// sputnik-amd: extern "C" boundary (declared in include/sputnik_amd.h).
//
// Each function converts the plain-C descriptors to the C++ ones (identical
// layout, checked below) and runs the same host path as the C++ API, but
// returns an error code in every case where the reference would abort.
#include <cstddef>
#include <cstring>

#include "act_math.h"
#include "api_internal.h"
#include "sputnik/block/router.h"
#include "sputnik/sputnik.h"
#include "metadata.h"
#include "sputnik_amd.h"

using sputnik::block::BlockMatrix;
using sputnik::block::BlockSize;
using sputnik::block::DataType;
using sputnik::block::Matrix;
using sputnik::block::RouterType;
using sputnik::block::WeightType;

static_assert(sizeof(BlockMatrix) == 88, "BlockMatrix ABI");
static_assert(sizeof(sputnik_block_matrix_t) == 88, "C BlockMatrix ABI");
static_assert(offsetof(BlockMatrix, block_size) == 12, "ABI");
static_assert(offsetof(BlockMatrix, data) == 16, "ABI");
static_assert(offsetof(BlockMatrix, row_indices) == 64, "ABI");
static_assert(offsetof(BlockMatrix, bitmask) == 72, "ABI");
static_assert(offsetof(BlockMatrix, create_metadata) == 80, "ABI");
static_assert(offsetof(sputnik_block_matrix_t, create_metadata) == 80, "ABI");
static_assert(offsetof(sputnik_block_matrix_t, row_indices) == 64, "ABI");
static_assert(sizeof(Matrix) == 16 && sizeof(sputnik_matrix_t) == 16, "ABI");
static_assert(offsetof(Matrix, data) == 8, "ABI");

namespace {

BlockMatrix ToCpp(const sputnik_block_matrix_t *m) {
  BlockMatrix out(m->rows, m->cols, static_cast<BlockSize>(m->block_size),
                  m->nonzeros, m->data, m->offsets, m->indices, m->offsets_t,
                  m->indices_t, m->block_offsets, m->bitmask);
  out.row_indices = m->row_indices;
  out.create_metadata = m->create_metadata != 0;
  return out;
}

Matrix ToCpp(const sputnik_matrix_t *m) {
  return Matrix(m->rows, m->cols, m->data);
}

int Code(hipError_t launch, int status_code) {
  return status_code != 0 ? status_code : static_cast<int>(launch);
}

}  // namespace


extern "C" {

// DSD / DDS, plain or accumulating (out). ex: the ...Ex forms use the
// transposed metadata as it is (create_metadata cleared on the copy).
static int DsdEntry(bool ex, const sputnik_block_matrix_t *a, int transpose_a,
                    const sputnik_matrix_t *b, int transpose_b,
                    const sputnik_matrix_t *c, int dtype, void *ws,
                    size_t ws_bytes, void *stream,
                    sputnik_amd::OutMode out = sputnik_amd::OutMode::kStore) {
  if (!a || !b || !c) return hipErrorInvalidValue;
  BlockMatrix ca = ToCpp(a);
  if (ex) ca.create_metadata = false;
  sputnik_amd::Status st;
  const hipError_t e = sputnik_amd::RunDsd(
      ca, transpose_a != 0, ToCpp(b), transpose_b != 0, ToCpp(c), dtype,
      static_cast<hipStream_t>(stream), &st,
      sputnik_amd::Workspace{ws, ws_bytes}, out);
  return Code(e, sputnik_amd::StatusCode(st));
}

static int DdsEntry(bool ex, const sputnik_matrix_t *a, int transpose_a,
                    const sputnik_block_matrix_t *b, int transpose_b,
                    const sputnik_matrix_t *c, int dtype, void *stream,
                    sputnik_amd::OutMode out = sputnik_amd::OutMode::kStore) {
  if (!a || !b || !c) return hipErrorInvalidValue;
  BlockMatrix cb = ToCpp(b);
  if (ex) cb.create_metadata = false;
  sputnik_amd::Status st;
  const hipError_t e = sputnik_amd::RunDds(
      ToCpp(a), transpose_a != 0, cb, transpose_b != 0, ToCpp(c), dtype,
      static_cast<hipStream_t>(stream), &st, out);
  return Code(e, sputnik_amd::StatusCode(st));
}

int sputnik_dsd_ws(const sputnik_block_matrix_t *a, int transpose_a,
                   const sputnik_matrix_t *b, int transpose_b,
                   const sputnik_matrix_t *c, int dtype, void *ws,
                   size_t ws_bytes, void *stream) {
  return DsdEntry(false, a, transpose_a, b, transpose_b, c, dtype, ws,
                  ws_bytes, stream);
}

int sputnik_dsd(const sputnik_block_matrix_t *a, int transpose_a,
                const sputnik_matrix_t *b, int transpose_b,
                const sputnik_matrix_t *c, int dtype, void *stream) {
  return DsdEntry(false, a, transpose_a, b, transpose_b, c, dtype, nullptr, 0,
                  stream);
}

int sputnik_dsd_ex_ws(const sputnik_block_matrix_t *a, int transpose_a,
                      const sputnik_matrix_t *b, int transpose_b,
                      const sputnik_matrix_t *c, int dtype, void *ws,
                      size_t ws_bytes, void *stream) {
  return DsdEntry(true, a, transpose_a, b, transpose_b, c, dtype, ws, ws_bytes,
                  stream);
}

int sputnik_dsd_ex(const sputnik_block_matrix_t *a, int transpose_a,
                   const sputnik_matrix_t *b, int transpose_b,
                   const sputnik_matrix_t *c, int dtype, void *stream) {
  return DsdEntry(true, a, transpose_a, b, transpose_b, c, dtype, nullptr, 0,
                  stream);
}

int sputnik_dds(const sputnik_matrix_t *a, int transpose_a,
                const sputnik_block_matrix_t *b, int transpose_b,
                const sputnik_matrix_t *c, int dtype, void *stream) {
  return DdsEntry(false, a, transpose_a, b, transpose_b, c, dtype, stream);
}

int sputnik_dds_ex(const sputnik_matrix_t *a, int transpose_a,
                   const sputnik_block_matrix_t *b, int transpose_b,
                   const sputnik_matrix_t *c, int dtype, void *stream) {
  return DdsEntry(true, a, transpose_a, b, transpose_b, c, dtype, stream);
}

// Accumulating DSD / DDS. c_type: SPUTNIK_OUT_OPERAND / SPUTNIK_OUT_F32.
static bool AccOutMode(int c_type, sputnik_amd::OutMode *out) {
  if (c_type == SPUTNIK_OUT_OPERAND) {
    *out = sputnik_amd::OutMode::kAccT;
    return true;
  }
  if (c_type == SPUTNIK_OUT_F32) {
    *out = sputnik_amd::OutMode::kAccF32;
    return true;
  }
  return false;
}

static int DsdAcc(bool ex, const sputnik_block_matrix_t *a, int transpose_a,
                  const sputnik_matrix_t *b, int transpose_b,
                  const sputnik_matrix_t *c, int dtype, int c_type,
                  void *stream) {
  sputnik_amd::OutMode out;
  if (!AccOutMode(c_type, &out)) return hipErrorInvalidValue;
  return DsdEntry(ex, a, transpose_a, b, transpose_b, c, dtype, nullptr, 0,
                  stream, out);
}

static int DdsAcc(bool ex, const sputnik_matrix_t *a, int transpose_a,
                  const sputnik_block_matrix_t *b, int transpose_b,
                  const sputnik_matrix_t *c, int dtype, int c_type,
                  void *stream) {
  sputnik_amd::OutMode out;
  if (!AccOutMode(c_type, &out)) return hipErrorInvalidValue;
  return DdsEntry(ex, a, transpose_a, b, transpose_b, c, dtype, stream, out);
}

int sputnik_dsd_acc(const sputnik_block_matrix_t *a, int transpose_a,
                    const sputnik_matrix_t *b, int transpose_b,
                    const sputnik_matrix_t *c, int dtype, int c_type,
                    void *stream) {
  return DsdAcc(false, a, transpose_a, b, transpose_b, c, dtype, c_type,
                stream);
}

int sputnik_dsd_ex_acc(const sputnik_block_matrix_t *a, int transpose_a,
                       const sputnik_matrix_t *b, int transpose_b,
                       const sputnik_matrix_t *c, int dtype, int c_type,
                       void *stream) {
  return DsdAcc(true, a, transpose_a, b, transpose_b, c, dtype, c_type,
                stream);
}

int sputnik_dds_acc(const sputnik_matrix_t *a, int transpose_a,
                    const sputnik_block_matrix_t *b, int transpose_b,
                    const sputnik_matrix_t *c, int dtype, int c_type,
                    void *stream) {
  return DdsAcc(false, a, transpose_a, b, transpose_b, c, dtype, c_type,
                stream);
}

int sputnik_dds_ex_acc(const sputnik_matrix_t *a, int transpose_a,
                       const sputnik_block_matrix_t *b, int transpose_b,
                       const sputnik_matrix_t *c, int dtype, int c_type,
                       void *stream) {
  return DdsAcc(true, a, transpose_a, b, transpose_b, c, dtype, c_type,
                stream);
}

int sputnik_sdd_ws(const sputnik_matrix_t *a, int transpose_a,
                   const sputnik_matrix_t *b, int transpose_b,
                   const sputnik_block_matrix_t *c, int dtype, void *ws,
                   size_t ws_bytes, void *stream) {
  if (!a || !b || !c) return hipErrorInvalidValue;
  sputnik_amd::Status st;
  const hipError_t e = sputnik_amd::RunSdd(
      ToCpp(a), transpose_a != 0, ToCpp(b), transpose_b != 0, ToCpp(c), dtype,
      static_cast<hipStream_t>(stream), &st,
      sputnik_amd::Workspace{ws, ws_bytes});
  return Code(e, sputnik_amd::StatusCode(st));
}

// SDD epilogue products (sputnik/block/activation.h, sputnik/block/gated.h):
// mode and side buffers as RunSddEpilogue takes them.
static int SddEpilogueCall(const sputnik_matrix_t *a, int transpose_a,
                           const sputnik_matrix_t *b, int transpose_b,
                           const sputnik_block_matrix_t *c, int act, int mode,
                           const void *side0, const void *side1, void *out1,
                           int dtype, void *ws, size_t ws_bytes,
                           void *stream) {
  if (!a || !b || !c) return hipErrorInvalidValue;
  if (act != SPUTNIK_ACT_RELU && act != SPUTNIK_ACT_GELU &&
      act != SPUTNIK_ACT_SILU)
    return hipErrorInvalidValue;
  const bool required_set =
      sputnik_amd::WithSddEpilogue(mode, false, [&](auto e) {
        using E = decltype(e);
        return !(E::kSideInputs >= 1 && side0 == nullptr) &&
               !(E::kSideInputs >= 2 && side1 == nullptr) &&
               !(E::kSecondOutput && out1 == nullptr);
      });
  if (!required_set) return hipErrorInvalidValue;
  sputnik_amd::Status st;
  const hipError_t e = sputnik_amd::RunSddEpilogue(
      ToCpp(a), transpose_a != 0, ToCpp(b), transpose_b != 0, ToCpp(c), dtype,
      act, mode, const_cast<void *>(side0), const_cast<void *>(side1), out1,
      static_cast<hipStream_t>(stream), &st,
      sputnik_amd::Workspace{ws, ws_bytes});
  return Code(e, sputnik_amd::StatusCode(st));
}

int sputnik_sdd_act(const sputnik_matrix_t *a, int transpose_a,
                    const sputnik_matrix_t *b, int transpose_b,
                    const sputnik_block_matrix_t *c, int act, void *z,
                    int dtype, void *ws, size_t ws_bytes, void *stream) {
  return SddEpilogueCall(a, transpose_a, b, transpose_b, c, act,
                         sputnik_amd::kOutAct, z, nullptr, nullptr, dtype, ws,
                         ws_bytes, stream);
}

int sputnik_sdd_act_grad(const sputnik_matrix_t *a, int transpose_a,
                         const sputnik_matrix_t *b, int transpose_b,
                         const sputnik_block_matrix_t *c, int act,
                         const void *z, int dtype, void *ws, size_t ws_bytes,
                         void *stream) {
  return SddEpilogueCall(a, transpose_a, b, transpose_b, c, act,
                         sputnik_amd::kOutActGrad, z, nullptr, nullptr, dtype,
                         ws, ws_bytes, stream);
}

int sputnik_sdd_gated(const sputnik_matrix_t *a, int transpose_a,
                      const sputnik_matrix_t *b, int transpose_b,
                      const sputnik_block_matrix_t *c, int act,
                      const void *gate, void *up, int dtype, void *ws,
                      size_t ws_bytes, void *stream) {
  return SddEpilogueCall(a, transpose_a, b, transpose_b, c, act,
                         sputnik_amd::kOutGate, gate, up, nullptr, dtype, ws,
                         ws_bytes, stream);
}

int sputnik_sdd_gated_grad(const sputnik_matrix_t *a, int transpose_a,
                           const sputnik_matrix_t *b, int transpose_b,
                           const sputnik_block_matrix_t *c, int act,
                           const void *gate, const void *up, void *up_grad,
                           int dtype, void *ws, size_t ws_bytes,
                           void *stream) {
  return SddEpilogueCall(a, transpose_a, b, transpose_b, c, act,
                         sputnik_amd::kOutGateGrad, gate, up, up_grad, dtype,
                         ws, ws_bytes, stream);
}

// SDD with a column bias (sputnik/block/bias.h).
static int SddBiasCall(const sputnik_matrix_t *a, int transpose_a,
                       const sputnik_matrix_t *b, int transpose_b,
                       const sputnik_block_matrix_t *c, const void *bias,
                       int act, int mode, const void *side0, void *side1,
                       int dtype, void *ws, size_t ws_bytes, void *stream) {
  if (!a || !b || !c) return hipErrorInvalidValue;
  if (act != SPUTNIK_ACT_RELU && act != SPUTNIK_ACT_GELU &&
      act != SPUTNIK_ACT_SILU)
    return hipErrorInvalidValue;
  if (mode == sputnik_amd::kOutGate && side0 == nullptr)
    return hipErrorInvalidValue;
  sputnik_amd::Status st;
  const hipError_t e = sputnik_amd::RunSddEpilogueBias(
      ToCpp(a), transpose_a != 0, ToCpp(b), transpose_b != 0, ToCpp(c), dtype,
      act, mode, const_cast<void *>(side0), side1, bias,
      static_cast<hipStream_t>(stream), &st,
      sputnik_amd::Workspace{ws, ws_bytes});
  return Code(e, sputnik_amd::StatusCode(st));
}

int sputnik_sdd_bias(const sputnik_matrix_t *a, int transpose_a,
                     const sputnik_matrix_t *b, int transpose_b,
                     const sputnik_block_matrix_t *c, const void *bias,
                     int dtype, void *ws, size_t ws_bytes, void *stream) {
  return SddBiasCall(a, transpose_a, b, transpose_b, c, bias,
                     SPUTNIK_ACT_RELU, sputnik_amd::kOutBias, nullptr, nullptr,
                     dtype, ws, ws_bytes, stream);
}

int sputnik_sdd_bias_act(const sputnik_matrix_t *a, int transpose_a,
                         const sputnik_matrix_t *b, int transpose_b,
                         const sputnik_block_matrix_t *c, const void *bias,
                         int act, void *z, int dtype, void *ws,
                         size_t ws_bytes, void *stream) {
  return SddBiasCall(a, transpose_a, b, transpose_b, c, bias, act,
                     sputnik_amd::kOutAct, z, nullptr, dtype, ws, ws_bytes,
                     stream);
}

int sputnik_sdd_bias_gated(const sputnik_matrix_t *a, int transpose_a,
                           const sputnik_matrix_t *b, int transpose_b,
                           const sputnik_block_matrix_t *c, const void *bias,
                           int act, const void *gate, void *up, int dtype,
                           void *ws, size_t ws_bytes, void *stream) {
  return SddBiasCall(a, transpose_a, b, transpose_b, c, bias, act,
                     sputnik_amd::kOutGate, gate, up, dtype, ws, ws_bytes,
                     stream);
}

int sputnik_block_column_sum(const sputnik_block_matrix_t *s, int dtype,
                             float *out, void *stream) {
  if (!s) return hipErrorInvalidValue;
  return sputnik_amd::RunBlockColumnSum(ToCpp(s), dtype, out,
                                        static_cast<hipStream_t>(stream));
}

// The elementwise stages alone, in the trait's argument order (x, s0, s1;
// o0, o1).
int sputnik_block_activation(const void *z, void *h, long long n, int act,
                             int dtype, void *stream) {
  return sputnik_amd::RunBlockEpilogue(
      dtype, act, sputnik_amd::kOutAct, z, nullptr, nullptr, h, nullptr, n,
      static_cast<hipStream_t>(stream));
}

int sputnik_block_activation_grad(const void *g, const void *z, void *out,
                                  long long n, int act, int dtype,
                                  void *stream) {
  return sputnik_amd::RunBlockEpilogue(
      dtype, act, sputnik_amd::kOutActGrad, g, z, nullptr, out, nullptr, n,
      static_cast<hipStream_t>(stream));
}

int sputnik_block_gate(const void *u, const void *g, void *out, long long n,
                       int act, int dtype, void *stream) {
  return sputnik_amd::RunBlockEpilogue(
      dtype, act, sputnik_amd::kOutGate, u, g, nullptr, out, nullptr, n,
      static_cast<hipStream_t>(stream));
}

int sputnik_block_gate_grad(const void *d, const void *g, const void *u,
                            void *dg, void *du, long long n, int act,
                            int dtype, void *stream) {
  return sputnik_amd::RunBlockEpilogue(
      dtype, act, sputnik_amd::kOutGateGrad, d, g, u, dg, du, n,
      static_cast<hipStream_t>(stream));
}

int sputnik_sdd_act_route(const sputnik_matrix_t *a, int transpose_a,
                          const sputnik_matrix_t *b, int transpose_b,
                          const sputnik_block_matrix_t *c) {
  if (!a || !b || !c) return -1;
  return sputnik_amd::SddActRoute(ToCpp(a), transpose_a != 0, ToCpp(b),
                                  transpose_b != 0, ToCpp(c));
}

int sputnik_sdd(const sputnik_matrix_t *a, int transpose_a,
                const sputnik_matrix_t *b, int transpose_b,
                const sputnik_block_matrix_t *c, int dtype, void *stream) {
  return sputnik_sdd_ws(a, transpose_a, b, transpose_b, c, dtype, nullptr, 0,
                        stream);
}

size_t sputnik_sdd_workspace_bytes(const sputnik_matrix_t *a, int transpose_a,
                                   const sputnik_matrix_t *b, int transpose_b,
                                   const sputnik_block_matrix_t *c) {
  if (!a || !b || !c) return 0;
  return sputnik_amd::SddWorkspaceBytes(ToCpp(a), transpose_a != 0, ToCpp(b),
                                        transpose_b != 0, ToCpp(c));
}

size_t sputnik_dsd_workspace_bytes(const sputnik_block_matrix_t *a,
                                   int transpose_a, const sputnik_matrix_t *b,
                                   int transpose_b, const sputnik_matrix_t *c) {
  if (!a || !b || !c) return 0;
  return sputnik_amd::DsdWorkspaceBytes(ToCpp(a), transpose_a != 0, ToCpp(b),
                                        transpose_b != 0, ToCpp(c));
}

int sputnik_set_stream_workspace(void *stream, void *ptr, size_t bytes) {
  return sputnik_amd::SetStreamWorkspace(static_cast<hipStream_t>(stream), ptr,
                                         bytes);
}

size_t sputnik_retained_bytes(void) { return sputnik_amd::RetainedBytes(); }

size_t sputnik_release_workspaces(void) {
  return sputnik_amd::ReleaseWorkspaces();
}

unsigned long long sputnik_incall_events(void) {
  return sputnik_amd::InCallEvents();
}

unsigned long long sputnik_bt_launches(void) {
  return sputnik_amd::BtLaunches();
}

static int SparseInOut(bool ssd, bool ex, const void *a, int ta,
                       const void *b, int tb,
                       const sputnik_block_matrix_t *c, int dtype,
                       void *stream) {
  if (!a || !b || !c) return hipErrorInvalidValue;
  sputnik_amd::Status st;
  hipError_t e;
  if (ssd) {
    BlockMatrix ca = ToCpp(static_cast<const sputnik_block_matrix_t *>(a));
    if (ex) ca.create_metadata = false;
    e = sputnik_amd::RunSsd(ca, ta != 0,
                            ToCpp(static_cast<const sputnik_matrix_t *>(b)),
                            tb != 0, ToCpp(c), dtype,
                            static_cast<hipStream_t>(stream), &st);
  } else {
    BlockMatrix cb = ToCpp(static_cast<const sputnik_block_matrix_t *>(b));
    if (ex) cb.create_metadata = false;
    e = sputnik_amd::RunSds(ToCpp(static_cast<const sputnik_matrix_t *>(a)),
                            ta != 0, cb, tb != 0, ToCpp(c), dtype,
                            static_cast<hipStream_t>(stream), &st);
  }
  return Code(e, sputnik_amd::StatusCode(st));
}

int sputnik_ssd(const sputnik_block_matrix_t *a, int transpose_a,
                const sputnik_matrix_t *b, int transpose_b,
                const sputnik_block_matrix_t *c, int dtype, void *stream) {
  return SparseInOut(true, false, a, transpose_a, b, transpose_b, c, dtype,
                     stream);
}

int sputnik_ssd_ex(const sputnik_block_matrix_t *a, int transpose_a,
                   const sputnik_matrix_t *b, int transpose_b,
                   const sputnik_block_matrix_t *c, int dtype, void *stream) {
  return SparseInOut(true, true, a, transpose_a, b, transpose_b, c, dtype,
                     stream);
}

int sputnik_sds(const sputnik_matrix_t *a, int transpose_a,
                const sputnik_block_matrix_t *b, int transpose_b,
                const sputnik_block_matrix_t *c, int dtype, void *stream) {
  return SparseInOut(false, false, a, transpose_a, b, transpose_b, c, dtype,
                     stream);
}

int sputnik_sds_ex(const sputnik_matrix_t *a, int transpose_a,
                   const sputnik_block_matrix_t *b, int transpose_b,
                   const sputnik_block_matrix_t *c, int dtype, void *stream) {
  return SparseInOut(false, true, a, transpose_a, b, transpose_b, c, dtype,
                     stream);
}

static int DssEntry(bool ex, const sputnik_block_matrix_t *a, int ta,
                    const sputnik_block_matrix_t *b, int tb,
                    const sputnik_matrix_t *c, int dtype, void *stream) {
  if (!a || !b || !c) return hipErrorInvalidValue;
  BlockMatrix ca = ToCpp(a), cb = ToCpp(b);
  if (ex) ca.create_metadata = cb.create_metadata = false;
  sputnik_amd::Status st;
  const hipError_t e =
      sputnik_amd::RunDss(ca, ta != 0, cb, tb != 0, ToCpp(c), dtype,
                          static_cast<hipStream_t>(stream), &st);
  return Code(e, sputnik_amd::StatusCode(st));
}

int sputnik_dss(const sputnik_block_matrix_t *a, int transpose_a,
                const sputnik_block_matrix_t *b, int transpose_b,
                const sputnik_matrix_t *c, int dtype, void *stream) {
  return DssEntry(false, a, transpose_a, b, transpose_b, c, dtype, stream);
}

int sputnik_dss_ex(const sputnik_block_matrix_t *a, int transpose_a,
                   const sputnik_block_matrix_t *b, int transpose_b,
                   const sputnik_matrix_t *c, int dtype, void *stream) {
  return DssEntry(true, a, transpose_a, b, transpose_b, c, dtype, stream);
}

int sputnik_row_indices(const sputnik_block_matrix_t *a, int16_t *row_indices,
                        void *stream) {
  if (!a || (!row_indices && a->nonzeros > 0)) return hipErrorInvalidValue;
  return sputnik::block::RowIndices(ToCpp(a), row_indices,
                                    static_cast<hipStream_t>(stream));
}

int sputnik_transpose(const sputnik_block_matrix_t *a, void *stream) {
  // A matrix without nonzero blocks has empty (possibly null) per-block
  // workspaces; only offsets_t must exist.
  if (!a || !a->offsets_t || !a->offsets) return hipErrorInvalidValue;
  if (a->nonzeros > 0 && (!a->indices_t || !a->block_offsets || !a->indices))
    return hipErrorInvalidValue;
  if (a->block_size != 128 && a->block_size != 64 && a->block_size != 32 &&
      a->block_size != 16)
    return hipErrorNotSupported;
  return sputnik::block::Transpose(ToCpp(a), static_cast<hipStream_t>(stream));
}

int sputnik_bitmask(const sputnik_block_matrix_t *m, void *stream) {
  if (!m || !m->bitmask) return hipErrorInvalidValue;
  const bool trans = m->offsets_t != nullptr;
  if ((trans ? !m->offsets_t : !m->offsets) ||
      (m->nonzeros > 0 && !(trans ? m->indices_t : m->indices)))
    return hipErrorInvalidValue;
  if (m->block_size != 128 && m->block_size != 64 && m->block_size != 32 &&
      m->block_size != 16)
    return hipErrorNotSupported;
  return sputnik::block::Bitmask(ToCpp(m), static_cast<hipStream_t>(stream));
}

size_t sputnik_bitmask_bytes(const sputnik_block_matrix_t *m) {
  if (!m) return 0;
  const int b = m->block_size;
  if (b != 128 && b != 64 && b != 32 && b != 16) return 0;
  const bool trans = m->offsets_t != nullptr;
  return sputnik::block::BitMatrix::SizeInBytes(
      (trans ? m->cols : m->rows) / b, (trans ? m->rows : m->cols) / b);
}

int sputnik_mask_to_bcsr(const uint8_t *mask, int block_rows, int block_cols,
                         int32_t *offsets, int16_t *indices, void *stream) {
  if (!offsets || (block_rows > 0 && block_cols > 0 && (!mask || !indices)))
    return hipErrorInvalidValue;
  return sputnik_amd::LaunchMaskToBcsr(block_rows, block_cols, mask, offsets,
                                       indices,
                                       static_cast<hipStream_t>(stream));
}

int sputnik_expert_topology(const int32_t *padded_bins, int num_experts,
                            int block_rows, int blocks_per_expert,
                            int32_t *offsets, int16_t *indices, void *stream) {
  if (!padded_bins || !offsets || (block_rows > 0 && !indices))
    return hipErrorInvalidValue;
  return sputnik_amd::LaunchExpertTopology(
      padded_bins, num_experts, block_rows, blocks_per_expert, offsets,
      indices, static_cast<hipStream_t>(stream));
}

// MoE token permutation (sputnik/block/moe.h): moe_permute.hip validates.
int sputnik_moe_bins(const int32_t *bin_ids, int n, int num_experts,
                     int32_t *bins, int32_t *tokens_per_expert,
                     int32_t *padded_bins, void *stream) {
  return sputnik::block::MoeBins(bin_ids, n, num_experts, bins,
                                 tokens_per_expert, padded_bins,
                                 static_cast<hipStream_t>(stream));
}

int sputnik_moe_row_map(const int32_t *indices, const int32_t *bin_ids,
                        const int32_t *bins, const int32_t *padded_bins,
                        int n, int num_experts, int rows, int32_t *row_of,
                        void *stream) {
  return sputnik::block::MoeRowMap(indices, bin_ids, bins, padded_bins, n,
                                   num_experts, rows, row_of,
                                   static_cast<hipStream_t>(stream));
}

int sputnik_padded_gather(const void *x, const int32_t *indices,
                          const int32_t *bins, const int32_t *padded_bins,
                          const void *weights, void *out, int tokens,
                          int hidden, int top_k, int num_experts, int rows,
                          int dtype, int weights_dtype, void *stream) {
  return sputnik::block::PaddedGather(
      x, indices, bins, padded_bins, weights, out, tokens, hidden, top_k,
      num_experts, rows, static_cast<DataType>(dtype),
      static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_padded_scatter(const void *y, const int32_t *row_of,
                           const void *weights, void *out, int tokens,
                           int hidden, int top_k, int rows, int dtype,
                           int weights_dtype, void *stream) {
  return sputnik::block::PaddedScatter(
      y, row_of, weights, out, tokens, hidden, top_k, rows,
      static_cast<DataType>(dtype), static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_padded_scatter_wgrad(const void *dout, const void *y,
                                 const int32_t *row_of, void *dw, int tokens,
                                 int hidden, int top_k, int rows, int dtype,
                                 int weights_dtype, void *stream) {
  return sputnik::block::PaddedScatterWeightGrad(
      dout, y, row_of, dw, tokens, hidden, top_k, rows,
      static_cast<DataType>(dtype), static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_padded_scatter_bias(const void *y, const int32_t *row_of,
                                const int32_t *padded_bins, const void *bias,
                                const void *weights, void *out, int tokens,
                                int hidden, int top_k, int num_experts,
                                int rows, int dtype, int weights_dtype,
                                void *stream) {
  return sputnik::block::PaddedScatterBias(
      y, row_of, padded_bins, bias, weights, out, tokens, hidden, top_k,
      num_experts, rows, static_cast<DataType>(dtype),
      static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_padded_scatter_bias_wgrad(const void *dout, const void *y,
                                      const int32_t *row_of,
                                      const int32_t *padded_bins,
                                      const void *bias, void *dw, int tokens,
                                      int hidden, int top_k, int num_experts,
                                      int rows, int dtype, int weights_dtype,
                                      void *stream) {
  return sputnik::block::PaddedScatterBiasWeightGrad(
      dout, y, row_of, padded_bins, bias, dw, tokens, hidden, top_k,
      num_experts, rows, static_cast<DataType>(dtype),
      static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_padded_scatter_bias_grad(const void *dout, const int32_t *indices,
                                     const int32_t *bins, const void *weights,
                                     float *bias_grad, int tokens, int hidden,
                                     int top_k, int num_experts, int dtype,
                                     int weights_dtype, void *stream) {
  return sputnik::block::PaddedScatterBiasGrad(
      dout, indices, bins, weights, bias_grad, tokens, hidden, top_k,
      num_experts, static_cast<DataType>(dtype),
      static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

// FP8 products (sputnik/block/fp8.h): fp8_quantize.hip and block_api.cpp
// validate.
int sputnik_quantize_rows(const void *x, int rows, int cols, void *q,
                          float *scales, int pow2, int dtype, void *stream) {
  return sputnik::block::QuantizeRows(x, rows, cols, q, scales, pow2 != 0,
                                      static_cast<DataType>(dtype),
                                      static_cast<hipStream_t>(stream));
}

int sputnik_quantize_rows_act(const void *x, int rows, int cols, int act,
                              void *q, float *scales, int pow2, int dtype,
                              void *stream) {
  return sputnik::block::QuantizeRowsActivation(
      x, rows, cols, static_cast<sputnik::block::Activation>(act), q, scales,
      pow2 != 0, static_cast<DataType>(dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_quantize_rows_gated(const void *x, const void *gate, int rows,
                                int cols, int act, void *q, float *scales,
                                int pow2, int dtype, void *stream) {
  return sputnik::block::QuantizeRowsGated(
      x, gate, rows, cols, static_cast<sputnik::block::Activation>(act), q,
      scales, pow2 != 0, static_cast<DataType>(dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_quantize_weight(const void *w, int k, int n, int transpose,
                            void *q, float *scales, int pow2, int dtype,
                            void *stream) {
  return sputnik::block::QuantizeWeight(w, k, n, transpose != 0, q, scales,
                                        pow2 != 0,
                                        static_cast<DataType>(dtype),
                                        static_cast<hipStream_t>(stream));
}

int sputnik_sdd_fp8(const void *aq, const float *a_scales, int k,
                    const void *bq, const float *b_scales,
                    const sputnik_block_matrix_t *c, int dtype, void *stream) {
  if (!c) return hipErrorInvalidValue;
  return sputnik::block::SddFp8(aq, a_scales, k, bq, b_scales, ToCpp(c),
                                static_cast<DataType>(dtype),
                                static_cast<hipStream_t>(stream));
}

int sputnik_dsd_fp8(const sputnik_block_matrix_t *s, const float *s_scales,
                    const void *bq, const float *b_scales,
                    const sputnik_matrix_t *c, int dtype, void *stream) {
  if (!s || !c) return hipErrorInvalidValue;
  return sputnik::block::DsdFp8(ToCpp(s), s_scales, bq, b_scales, ToCpp(c),
                                static_cast<DataType>(dtype),
                                static_cast<hipStream_t>(stream));
}

int sputnik_sdd_fp8_acc(const void *aq, const float *a_scales, int k,
                        const void *bq, const float *b_scales,
                        const sputnik_block_matrix_t *c, int dtype,
                        int accumulate, void *stream) {
  if (!c) return hipErrorInvalidValue;
  return sputnik::block::SddFp8(
      aq, a_scales, k, bq, b_scales, ToCpp(c), static_cast<DataType>(dtype),
      static_cast<sputnik::block::Fp8Accumulate>(accumulate),
      static_cast<hipStream_t>(stream));
}

int sputnik_dsd_fp8_acc(const sputnik_block_matrix_t *s, const float *s_scales,
                        const void *bq, const float *b_scales,
                        const sputnik_matrix_t *c, int dtype, int accumulate,
                        void *stream) {
  if (!s || !c) return hipErrorInvalidValue;
  return sputnik::block::DsdFp8(
      ToCpp(s), s_scales, bq, b_scales, ToCpp(c), static_cast<DataType>(dtype),
      static_cast<sputnik::block::Fp8Accumulate>(accumulate),
      static_cast<hipStream_t>(stream));
}

int sputnik_fp8_interval_sums(const void *aq, const void *bq, int m, int n,
                              int k, int accumulate, float *p, void *stream) {
  return sputnik::block::Fp8IntervalSums(
      aq, bq, m, n, k, static_cast<sputnik::block::Fp8Accumulate>(accumulate),
      p, static_cast<hipStream_t>(stream));
}

// ... and their gradients' pieces.
int sputnik_quantize_tiles(const void *x, int rows, int cols, void *q,
                           float *scales, void *qt, float *scales_t, int pow2,
                           int dtype, void *stream) {
  return sputnik::block::QuantizeTiles(x, rows, cols, q, scales, qt, scales_t,
                                       pow2 != 0, static_cast<DataType>(dtype),
                                       static_cast<hipStream_t>(stream));
}

int sputnik_quantize_blocks(const sputnik_block_matrix_t *s, int stage,
                            int act, const void *z, void *q, float *scales,
                            void *qt, float *scales_t, int pow2, int dtype,
                            void *stream) {
  if (!s) return hipErrorInvalidValue;
  return sputnik::block::QuantizeBlocks(
      ToCpp(s), static_cast<sputnik::block::Fp8Stage>(stage),
      static_cast<sputnik::block::Activation>(act), z, q, scales, qt,
      scales_t, pow2 != 0, static_cast<DataType>(dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_fp8_transpose_weight(const void *q, const float *scales, int k,
                                 int n, void *qt, float *scales_t,
                                 void *stream) {
  return sputnik::block::TransposeWeightFp8(q, scales, k, n, qt, scales_t,
                                            static_cast<hipStream_t>(stream));
}

int sputnik_dsd_fp8_wgrad(const sputnik_block_matrix_t *s,
                          const float *s_scales, const void *bq,
                          const float *b_scales, const sputnik_matrix_t *c,
                          int dtype, int out, int add, int accumulate,
                          void *stream) {
  if (!s || !c) return hipErrorInvalidValue;
  return sputnik::block::DsdFp8Wgrad(
      ToCpp(s), s_scales, bq, b_scales, ToCpp(c), static_cast<DataType>(dtype),
      static_cast<sputnik::block::OutputType>(out), add != 0,
      static_cast<sputnik::block::Fp8Accumulate>(accumulate),
      static_cast<hipStream_t>(stream));
}

// MoE router and device sort (sputnik/block/router.h): moe_router.hip
// validates.
int sputnik_router_topk(const void *logits, int32_t *top_experts,
                        void *weights, void *scores, int tokens,
                        int num_experts, int top_k, int normalize,
                        int logits_dtype, int weights_dtype, void *stream) {
  return sputnik::block::RouterTopK(logits, top_experts, weights, scores,
                                    tokens, num_experts, top_k, normalize != 0,
                                    static_cast<RouterType>(logits_dtype),
                                    static_cast<WeightType>(weights_dtype),
                                    static_cast<hipStream_t>(stream));
}

int sputnik_router_topk_grad(const void *logits, const int32_t *top_experts,
                             const void *dweights, const void *dscores,
                             void *dlogits, int tokens, int num_experts,
                             int top_k, int normalize, int logits_dtype,
                             int weights_dtype, void *stream) {
  return sputnik::block::RouterTopKGrad(
      logits, top_experts, dweights, dscores, dlogits, tokens, num_experts,
      top_k, normalize != 0, static_cast<RouterType>(logits_dtype),
      static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

size_t sputnik_router_aux_workspace_bytes(int tokens, int num_experts) {
  return sputnik::block::RouterAuxWorkspaceBytes(tokens, num_experts);
}

int sputnik_router_topk_aux(const void *logits, int32_t *top_experts,
                            void *weights, void *scores, float *score_sums,
                            float *z_sum, int tokens, int num_experts,
                            int top_k, int normalize, int logits_dtype,
                            int weights_dtype, void *workspace,
                            size_t workspace_bytes, void *stream) {
  return sputnik::block::RouterTopKAux(
      logits, top_experts, weights, scores, score_sums, z_sum, tokens,
      num_experts, top_k, normalize != 0,
      static_cast<RouterType>(logits_dtype),
      static_cast<WeightType>(weights_dtype), workspace, workspace_bytes,
      static_cast<hipStream_t>(stream));
}

int sputnik_router_topk_aux_grad(const void *logits,
                                 const int32_t *top_experts,
                                 const void *dweights, const void *dscores,
                                 const float *dscore_sums, const float *dz_sum,
                                 void *dlogits, int tokens, int num_experts,
                                 int top_k, int normalize, int logits_dtype,
                                 int weights_dtype, void *stream) {
  return sputnik::block::RouterTopKAuxGrad(
      logits, top_experts, dweights, dscores, dscore_sums, dz_sum, dlogits,
      tokens, num_experts, top_k, normalize != 0,
      static_cast<RouterType>(logits_dtype),
      static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_router_score_topk(const void *logits, const float *bias,
                              int32_t *top_experts, void *weights,
                              void *scores, int tokens, int num_experts,
                              int top_k, int num_groups, int topk_groups,
                              int normalize, float scale, int logits_dtype,
                              int weights_dtype, void *stream) {
  return sputnik::block::RouterScoreTopK(
      logits, bias, top_experts, weights, scores, tokens, num_experts, top_k,
      num_groups, topk_groups, normalize != 0, scale,
      static_cast<RouterType>(logits_dtype),
      static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

int sputnik_router_score_topk_grad(const void *logits,
                                   const int32_t *top_experts,
                                   const void *dweights, const void *dscores,
                                   void *dlogits, int tokens, int num_experts,
                                   int top_k, int normalize, float scale,
                                   int logits_dtype, int weights_dtype,
                                   void *stream) {
  return sputnik::block::RouterScoreTopKGrad(
      logits, top_experts, dweights, dscores, dlogits, tokens, num_experts,
      top_k, normalize != 0, scale, static_cast<RouterType>(logits_dtype),
      static_cast<WeightType>(weights_dtype),
      static_cast<hipStream_t>(stream));
}

size_t sputnik_moe_sort_workspace_bytes(int n, int num_experts) {
  return sputnik::block::MoeSortWorkspaceBytes(n, num_experts);
}

int sputnik_moe_sort(const int32_t *top_experts, int n, int num_experts,
                     int rows, int32_t *indices, int32_t *bin_ids,
                     int32_t *bins, int32_t *tokens_per_expert,
                     int32_t *padded_bins, int32_t *row_of, void *workspace,
                     size_t workspace_bytes, void *stream) {
  return sputnik::block::MoeSort(top_experts, n, num_experts, rows, indices,
                                 bin_ids, bins, tokens_per_expert, padded_bins,
                                 row_of, workspace, workspace_bytes,
                                 static_cast<hipStream_t>(stream));
}

int sputnik_can_implement(int op, const void *a, int transpose_a,
                          const void *b, int transpose_b, const void *c) {
  return sputnik_amd::CanImplement(op, a, transpose_a != 0, b,
                                   transpose_b != 0, c)
             ? 1
             : 0;
}

int sputnik_sdd_plan(const sputnik_matrix_t *a, int transpose_a,
                     const sputnik_matrix_t *b, int transpose_b,
                     const sputnik_block_matrix_t *c) {
  if (!a || !b || !c) return -1;
  const Matrix ca = ToCpp(a), cb = ToCpp(b);
  const BlockMatrix cc = ToCpp(c);
  return sputnik_amd::SddPlan(&ca, transpose_a != 0, &cb, transpose_b != 0,
                              &cc);
}

int sputnik_sdd_kernel(const sputnik_matrix_t *a, int transpose_a,
                       const sputnik_matrix_t *b, int transpose_b,
                       const sputnik_block_matrix_t *c) {
  if (!a || !b || !c) return -1;
  const Matrix ca = ToCpp(a), cb = ToCpp(b);
  const BlockMatrix cc = ToCpp(c);
  return sputnik_amd::SddKernel(&ca, transpose_a != 0, &cb, transpose_b != 0,
                                &cc);
}

int sputnik_dds_plan(const sputnik_matrix_t *a, int transpose_a,
                     const sputnik_block_matrix_t *b, int transpose_b,
                     const sputnik_matrix_t *c, hipStream_t stream) {
  if (!a || !b || !c) return -1;
  const Matrix ca = ToCpp(a), cc = ToCpp(c);
  const BlockMatrix cb = ToCpp(b);
  return sputnik_amd::DdsPlan(&ca, transpose_a != 0, &cb, transpose_b != 0, &cc,
                              stream);
}

int sputnik_dsd_plan(const sputnik_block_matrix_t *a, int transpose_a,
                     const sputnik_matrix_t *b, int transpose_b,
                     const sputnik_matrix_t *c, hipStream_t stream) {
  if (!a || !b || !c) return -1;
  const BlockMatrix ca = ToCpp(a);
  const Matrix cb = ToCpp(b), cc = ToCpp(c);
  return sputnik_amd::DsdPlan(&ca, transpose_a != 0, &cb, transpose_b != 0, &cc,
                              stream);
}

int sputnik_pair_errors(void) { return sputnik_amd::PairErrors(); }

void sputnik_debug_pair_fault(int on) { sputnik_amd::SetPairFault(on); }

int sputnik_capture_workspaces(void) {
  return sputnik_amd::CaptureWorkspaces();
}

int sputnik_select_dsd_kernel(int four_wave) {
  return sputnik_amd::SelectDsdKernel(four_wave);
}

int sputnik_tuning_get(const char *name) { return sputnik_amd::TuningGet(name); }

int sputnik_tuning_set(const char *name, int value) {
  return sputnik_amd::TuningSet(name, value);
}

size_t sputnik_abi_block_matrix_size(void) { return sizeof(BlockMatrix); }

size_t sputnik_abi_block_matrix_offset(int field) {
  switch (field) {
    case 0: return offsetof(BlockMatrix, rows);
    case 1: return offsetof(BlockMatrix, cols);
    case 2: return offsetof(BlockMatrix, nonzeros);
    case 3: return offsetof(BlockMatrix, block_size);
    case 4: return offsetof(BlockMatrix, data);
    case 5: return offsetof(BlockMatrix, offsets);
    case 6: return offsetof(BlockMatrix, indices);
    case 7: return offsetof(BlockMatrix, offsets_t);
    case 8: return offsetof(BlockMatrix, indices_t);
    case 9: return offsetof(BlockMatrix, block_offsets);
    case 10: return offsetof(BlockMatrix, row_indices);
    case 11: return offsetof(BlockMatrix, bitmask);
    case 12: return offsetof(BlockMatrix, create_metadata);
    default: return (size_t)-1;
  }
}

size_t sputnik_abi_matrix_size(void) { return sizeof(Matrix); }

#ifndef SPUTNIK_BUILD_HASH
#define SPUTNIK_BUILD_HASH "unknown"
#endif
const char *sputnik_version(void) { return "sputnik-amd 0.2 (gfx950)"; }
const char *sputnik_build_hash(void) { return SPUTNIK_BUILD_HASH; }

}  // extern "C"
