// sputnik-amd: what the host files of the dispatcher share (host only, not
// part of include/): knobs.cpp (the tuning knobs), workspaces.cpp (every
// piece of device memory the library keeps, and the caller's), operands.cpp
// (which descriptors a product accepts and how they bind to GemmParams: pure
// host arithmetic), dispatch.cpp (route, run, the queries) and block_api.cpp
// (the sputnik::block overload set).
#ifndef SPUTNIK_AMD_DISPATCH_INTERNAL_H_
#define SPUTNIK_AMD_DISPATCH_INTERNAL_H_

#include <mutex>

#include "api_internal.h"
#include "block_gemm.h"

namespace sputnik_amd {

// ---- workspaces.cpp ----
// On the stack of every product entry point (a Run* function): the HIP
// allocations, frees and synchronizes executed meanwhile on this thread are
// counted (InCallEvents).
struct InProduct {
  InProduct();
  ~InProduct();
  InProduct(const InProduct &) = delete;
  InProduct &operator=(const InProduct &) = delete;
};

// Compute units of a device, queried once per device.
int DeviceCUs(int dev);

// The pair workspace of (device, stream) -- or of the capture under way on
// `stream` -- found, re-tied or allocated, and a new epoch and its pointers
// bound into *p for one launch that needs `need` resident workgroup slots.
// Returns the workspace's slots, 0: none available or fewer than `need`
// (nothing bound). dry: decide only, for the workspace a launch would get;
// nothing is allocated, re-tied, advanced or bound.
int BindPairWorkspace(GemmParams *p, long long need, hipStream_t stream, bool dry);

// The persistent form of a tall 8-wave launch (p as UseTall left it): one
// workgroup per slot and a per-(device, stream) or per-capture tile counter,
// where the tiles outnumber the slots. dry: as above.
void BindTileCounter(GemmParams *p, hipStream_t stream, bool dry);

// The size, alignment and knob gate of the transposed copy of B that SDD NT /
// TT and DSD NT share: B^T ([N][K]) in whole 64 x 64 tiles of 16-byte
// vectors, at least sdd_bt_min_mib MiB.
bool BtGate(const Matrix &b);
// The library-owned copy buffer may serve `stream`: not hipStreamPerThread
// and not while it is being captured.
bool BtLibraryStreamOk(hipStream_t stream);
// Bytes of the copy (a multiple of 256).
size_t BtBytes(const Matrix &b);
// One transposed-B step. B^T is copied transposed on `stream` into the
// call's workspace or the one registered for the stream (no lock, no slot,
// no allocation; memory that does not fit keeps the NT / TT kernel), else
// into the library's buffer of the stream under g_bt_mu, which `lock` then
// holds until the caller has enqueued the product. data == nullptr: keep
// the NT / TT kernel (nothing was enqueued).
struct BtCopy {
  std::unique_lock<std::mutex> lock;
  hipError_t error = hipSuccess;
  void *data = nullptr;  // [b.cols][b.rows]
};
BtCopy TransposeB(const Matrix &b, hipStream_t stream, Workspace ws);

// ---- operands.cpp ----
constexpr long long kMaxLaneOffset = 0x7fffffffLL;  // 31-bit buffer offsets
constexpr int kDssMaxK = 32768;

// One operand of a product as the caller described it: a dense matrix
// (sparse == nullptr) or a BCSR one, whose descriptor must outlive the
// Product bound from it.
struct Operand {
  int rows, cols;
  const void *data;
  const BlockMatrix *sparse;
  Operand(const Matrix &m) : rows(m.rows), cols(m.cols), data(m.data), sparse(nullptr) {}
  Operand(const BlockMatrix &m) : rows(m.rows), cols(m.cols), data(m.data), sparse(&m) {}
};

// A product in the kernel's terms, O = S . D over 128-row tiles of the row
// operand S (the table is at Bind, operands.cpp). Which of A, B, C are sparse
// says which of the six products it is.
struct Product {
  Status status = Status::kNoKernel;
  // What the launches take: S / D k-contiguous in memory, O written
  // transposed (DDS / SDS: S = op(B)^T, D = op(A)^T).
  bool s_kc = false, d_kc = false, out_t = false;
  // The sparse descriptor behind S / D (nullptr: dense), and whether it is
  // read through its transposed metadata, which a launch builds first when
  // the descriptor's create_metadata is set.
  const BlockMatrix *s_sparse = nullptr, *d_sparse = nullptr;
  bool s_meta = false, d_meta = false;
  GemmParams p{};  // valid when status == kOk
};
Product Bind(const Operand &a, bool ta, const Operand &b, bool tb, const Operand &c);

// ---- dispatch.cpp ----
hipError_t BuildTransposed(const BlockMatrix &a, hipStream_t stream);

}  // namespace sputnik_amd

#endif  // SPUTNIK_AMD_DISPATCH_INTERNAL_H_
