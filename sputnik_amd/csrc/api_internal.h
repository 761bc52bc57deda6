// sputnik-amd: host entry points shared by the C++ API and the C-ABI.
#ifndef SPUTNIK_AMD_API_INTERNAL_H_
#define SPUTNIK_AMD_API_INTERNAL_H_

#include <cstddef>

#include "sputnik/block/arguments.h"

namespace sputnik_amd {

// Outcome of the host-side acceptance checks of one call.
enum class Status {
  kOk,
  kNotSupported,     // block size != 128 -> hipErrorNotSupported (dsd.cu:16)
  kNoKernel,         // reference: "No compatible kernel" -> abort
  kMissingMetadata,  // reference: SPUTNIK_CHECK(offsets_t ...) -> abort
  kMissingRowIndices,
};

using sputnik::block::BlockMatrix;
using sputnik::block::Matrix;

// Caller-owned device memory for the transposed copy of B (SDD NT / TT, DSD
// NT; workspaces.cpp "caller-owned transposed-B workspaces"). Empty: none was
// supplied with the call.
struct Workspace {
  void *ptr = nullptr;
  size_t bytes = 0;
};

// What a dense-output product does with C. kStore: overwrite it with the
// operand type (the plain products). kAccT / kAccF32: C += op(A) op(B) into a
// C of the operand type / of fp32, rounded once after the add; C is left
// untouched where the sparse operand has no blocks. An accumulating call
// always runs the 8-wave kernel (pairs or the tall configuration as the
// plain call would, never split mode, never the transposed-B route).
enum class OutMode { kStore = 0, kAccT = 1, kAccF32 = 2 };

// Validate, build the transposed metadata a sparse input is read through
// when its descriptor's create_metadata is set (the ...Ex forms clear it on
// their copy), launch. A non-kOk *status means nothing was launched.
hipError_t RunDsd(const BlockMatrix &a, bool ta, const Matrix &b, bool tb,
                  const Matrix &c, int dtype, hipStream_t stream,
                  Status *status, Workspace ws = Workspace{},
                  OutMode out = OutMode::kStore);
hipError_t RunDds(const Matrix &a, bool ta, const BlockMatrix &b, bool tb,
                  const Matrix &c, int dtype, hipStream_t stream,
                  Status *status, OutMode out = OutMode::kStore);
hipError_t RunSdd(const Matrix &a, bool ta, const Matrix &b, bool tb,
                  const BlockMatrix &c, int dtype, hipStream_t stream,
                  Status *status, Workspace ws = Workspace{});

// SDD epilogue products (sputnik/block/activation.h, sputnik/block/gated.h):
// c.data = op(round(A B), side buffers), `mode` one of kOutAct, kOutActGrad,
// kOutGate, kOutGateGrad (act_math.h SddEpilogue has the table). The side
// buffers are GemmParams' z_data, u_data and du_data:
//   kOutAct       side0 = z, receives Z = round(A B) when not null
//   kOutActGrad   side0 = z, the Z to gate with (required)
//   kOutGate      side0 = gate (required); side1 = up, receives U when not
//                 null
//   kOutGateGrad  side0 = gate, side1 = up, out1 = up_grad (all required)
// act: kActRelu / kActGelu / kActSilu (act_math.h). A bad act, a null
// required pointer or two buffers that must not coincide (activation: z ==
// c.data; gated: any two of gate, up, up_grad, c.data, A, B, up_grad == up
// excepted) is hipErrorInvalidValue before anything is launched. Two routes,
// bit-identical (knob "sdd_act_route": 0 auto, 1 fused, 2 two kernels):
// fused, the 8-wave kernel's epilogue (never the transposed-B path); two
// kernels, RunSdd as it stands into the buffer that keeps x (or c.data) and
// RunBlockEpilogue behind it. Auto: fused where the plain call would run the
// 8-wave kernel alone (SddKernel 0 / 1), read off the call's SDD route
// (dispatch.cpp RouteSdd, SddActRouteOf), whose params the fused launch then
// uses; two kernels wherever the transposed-B path applies to the problem.
hipError_t RunSddEpilogue(const Matrix &a, bool ta, const Matrix &b, bool tb,
                          const BlockMatrix &c, int dtype, int act, int mode,
                          void *side0, void *side1, void *out1,
                          hipStream_t stream, Status *status,
                          Workspace ws = Workspace{});
// The same with a column bias (sputnik/block/bias.h): `mode` kOutBias,
// kOutAct or kOutGate, bias c.columns elements of the operand type at any
// 2-byte alignment. The op sees xb = round(x + bias[col]) for x, and the kept
// Z / U is xb. A bias that is null or equals c.data, a side buffer, A or B is
// hipErrorInvalidValue with nothing launched. Same routes: fused, the column
// from the tile's block; two kernels, the elementwise stage reads
// c.indices and writes xb back over the kept x in place.
hipError_t RunSddEpilogueBias(const Matrix &a, bool ta, const Matrix &b,
                              bool tb, const BlockMatrix &c, int dtype,
                              int act, int mode, void *side0, void *side1,
                              const void *bias, hipStream_t stream,
                              Status *status, Workspace ws = Workspace{});
// out[c] = sum over the stored blocks of column c of float(s[r, c]), fp32
// [s.columns] (block_reduce.hip). Walks s's transposed metadata; null there:
// hipErrorInvalidValue.
hipError_t RunBlockColumnSum(const BlockMatrix &s, int dtype, float *out,
                             hipStream_t stream);
// The route RunSddEpilogue would take now: 1 fused, 2 two kernels, -1
// rejected.
int SddActRoute(const Matrix &a, bool ta, const Matrix &b, bool tb,
                const BlockMatrix &c);
// The elementwise stage alone over n elements (block_epilogue.hip), in the
// trait's argument order: (o0, o1) = op(x, s0, s1), buffers the mode does
// not have null. An output may be an input (act_math.h); o0 == o1 is
// rejected. Validates act, dtype, n and the pointers (hipErrorInvalidValue);
// n == 0 succeeds whatever the pointers.
hipError_t RunBlockEpilogue(int dtype, int act, int mode, const void *x,
                            const void *s0, const void *s1, void *o0,
                            void *o1, long long n, hipStream_t stream);
hipError_t LaunchBlockEpilogue(int dtype, int mode, int act, const void *x,
                               const void *s0, const void *s1, void *o0,
                               void *o1, long long n, int cus,
                               hipStream_t stream, const void *bias = nullptr,
                               const short *column_indices = nullptr,
                               int col_blocks = 0);

// The fp8 block GEMM (sputnik/block/fp8.h, fp8_gemm.hip), arguments already
// validated by SddFp8 / DsdFp8 (block_api.cpp). SDD (`dsd` false): a = Aq
// [m, k] with a_scales [m, k / 128], one workgroup per stored block of C
// (indices, row_indices; offsets unused). DSD: a = the sparse operand's e4m3
// blocks with a_scales [nnz_blocks * 128], offsets / indices its BCSR
// metadata, c dense [m, n]. b = Bq [n, k] with b_scales [k / 128, n / 128].
// Sizes in blocks of 128. `fast` selects Fp8Accumulate::kFast, the scaled
// e4m3 MFMA per interval.
hipError_t LaunchFp8Gemm(bool dsd, bool fast, int dtype, const void *a,
                         const float *a_scales, const void *b,
                         const float *b_scales, void *c, const int *offsets,
                         const short *indices, const short *row_indices,
                         int m_blocks, int n_blocks, int k_blocks,
                         int nnz_blocks, hipStream_t stream);
// The same DSD with b_scales [k / 128, n], one per column and interval
// (DsdFp8Wgrad): c holds T or, with `out_f32`, fp32; `add` accumulates into
// it.
hipError_t LaunchFp8Wgrad(bool fast, int dtype, bool out_f32, bool add,
                          const void *s, const float *s_scales, const void *b,
                          const float *b_scales, void *c, const int *offsets,
                          const short *indices, int m_blocks, int n_blocks,
                          int k_blocks, int nnz_blocks, hipStream_t stream);
// P [k / 128, m, n] of Fp8IntervalSums, arguments already validated
// (block_api.cpp): m, n and k multiples of 128.
hipError_t LaunchFp8IntervalSums(const void *aq, const void *bq, int m, int n,
                                 int k, bool fast, float *out,
                                 hipStream_t stream);

// Per-(current device, stream) registration of caller memory (ptr null:
// unregister); the plain entry points look it up.
hipError_t SetStreamWorkspace(hipStream_t stream, void *ptr, size_t bytes);
// Bytes the transposed-B path would use for a problem (0: it does not apply).
size_t SddWorkspaceBytes(const Matrix &a, bool ta, const Matrix &b, bool tb,
                         const BlockMatrix &c);
size_t DsdWorkspaceBytes(const BlockMatrix &a, bool ta, const Matrix &b, bool tb,
                         const Matrix &c);
// Device memory the library holds on the current device; the transposed-B
// buffers of it freed (after a device synchronize), bytes freed.
size_t RetainedBytes();
size_t ReleaseWorkspaces();
// Monotonic process-wide counters: allocations / frees / synchronizes
// executed inside a product call; transposed-B launches enqueued.
unsigned long long InCallEvents();
unsigned long long BtLaunches();

hipError_t RunSsd(const BlockMatrix &a, bool ta, const Matrix &b, bool tb,
                  const BlockMatrix &c, int dtype, hipStream_t stream,
                  Status *status);
hipError_t RunSds(const Matrix &a, bool ta, const BlockMatrix &b, bool tb,
                  const BlockMatrix &c, int dtype, hipStream_t stream,
                  Status *status);
hipError_t RunDss(const BlockMatrix &a, bool ta, const BlockMatrix &b,
                  bool tb, const Matrix &c, int dtype, hipStream_t stream,
                  Status *status);

// hipError_t value the C-ABI returns for a status (never aborts).
int StatusCode(Status st);

// Host-only acceptance test. op 0 = DSD, 1 = DDS, 2 = SDD, 3 = SSD, 4 = SDS, 5 = DSS.
bool CanImplement(int op, const void *a, bool ta, const void *b, bool tb,
                  const void *c);

// The queries below report the route a launch would take (dispatch.cpp
// RouteSdd / RouteDds / RouteDsd, computed dry: no launch, nothing allocated).
// SDD tile plan of a valid problem: 1 = grouped 128x512 tiles, 2 = grouped
// tiles with each group's K split, 0 = one k-split 128x128 block per
// workgroup, -1 = rejected. Reads the CU count of the current device.
int SddPlan(const void *a, bool ta, const void *b, bool tb, const void *c);
// SDD kernel (dispatch.cpp SddKernel): 0 8-wave k-split tile, 1 8-wave
// grouped, 2 4-wave K-split, 3 4-wave grouped, 4 B transposed first (null
// stream, no workspace known), -1 rejected.
int SddKernel(const void *a, bool ta, const void *b, bool tb, const void *c);
// DDS kernel plan (dispatch.cpp DdsPlan): 0 8-wave tile, 1 4-wave kernel,
// 2 tall, 3 split (8-wave), -1 rejected.
int DdsPlan(const void *a, bool ta, const void *b, bool tb, const void *c,
            hipStream_t stream);
// DSD kernel plan (dispatch.cpp DsdPlan): 0 8-wave tile, 1 4-wave kernel,
// 2 tall, 3 split mode, 4 tall pipeline, -1 rejected.
int DsdPlan(const void *a, bool ta, const void *b, bool tb, const void *c,
            hipStream_t stream);

// Pair hand-offs that timed out (see workspaces.cpp), and the test knob that
// makes every pair producer skip its publish.
int PairErrors();
void SetPairFault(int on);
int CaptureWorkspaces();
// DSD / DDS / grouped SDD: 4-wave kernel on (1) / off (0) / forced
// regardless of density with kEpi = mode - 2 (modes 2-7, dsd4w.h
// LaunchDsd4w); -1 queries. Returns the previous. (= knob "dsd4w")
int SelectDsdKernel(int four_wave);
bool Dsd4wEnabled();
bool Dsd4wForced();
int Dsd4wEpi();

// Unsupported tuning knobs (knobs.cpp kKnobs: name, environment
// variable, default, range). Knob() reads one; TuningGet / TuningSet back
// sputnik_tuning_get / sputnik_tuning_set (INT_MIN: unknown name or value
// out of range).
enum KnobId {
  kKnobPairs,
  kKnobPairXcd2,
  kKnobSplit,
  kKnobSplitMinBn,
  kKnobDsd4w,
  kKnobGroupedSdd,
  kKnobGroupedMinPerCu,
  kKnobTall,
  kKnobTallPersistent,
  kKnobDdsXcd2,
  kKnobSdd4wMaxLd,
  kKnobPairFault,
  kKnobSddKsplit,
  kKnobSddKsplitMinK,
  kKnobSddOrder,
  kKnobTall4w,
  kKnobTallFlushW,
  kKnobTallOddShare,
  kKnobMinHandoff,
  kKnobXcdRows,
  kKnobSddKrot,
  kKnobSddSpread,
  kKnobSddBtMinMib,
  kKnobSddTailMinK,
  kKnobSddActRoute,
  kNumKnobs
};
int Knob(KnobId k);
int TuningGet(const char *name);
int TuningSet(const char *name, int value);

}  // namespace sputnik_amd

#endif  // SPUTNIK_AMD_API_INTERNAL_H_
