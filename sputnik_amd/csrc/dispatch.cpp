// sputnik-amd: host side of the sputnik::block API (C++ overloads) and its
// C-ABI twin (include/sputnik_amd.h).
//
// Replaces, for the hot path:
//   sputnik/block/dsd/dsd.cu:9-27, dds/dds.cu:7-24, sdd/sdd.cu:7-15
//     (block-size gate, Matmul/MatmulEx),
//   sputnik/block/{dsd,dds,sdd}/cutlass/<op>.cu (first-fit registries),
//   the can_launch_* / launch_* bodies of the 12 *_align8.cu variants
//     (shape rules, metadata checks, operand bundling),
//   sputnik/block/row_indices/row_indices.cu:24-36 and
//   sputnik/block/transpose/transpose.cu:69-125 (entry points).
//
// Problem -> kernel mapping (see block_gemm.h). Every product is phrased as
// O = S * D over 128-row tiles of a "row operand" S:
//   DSD  C = op(A) op(B):  S = op(A) (sparse), D = op(B), O = C.
//   DDS  C = op(A) op(B):  S = op(B)^T (sparse), D = op(A)^T, O = C^T.
//   SDD  C = op(A) op(B):  S = op(A) (dense),  D = op(B), O = C's blocks.
// A sparse S read in column order (DSD TN/TT, DDS NN/TN) uses the transposed
// metadata (offsets_t, indices_t, block_offsets), exactly like the reference.
//
// operands.cpp states that mapping once (Bind) and says which descriptors a
// product accepts. One function per product (RouteDsd / RouteDds / RouteSdd)
// decides which kernel runs the bound product with which GemmParams; the
// Run* entry points execute that route and the queries (DsdPlan, DdsPlan, SddPlan, SddKernel, SddActRoute,
// the *WorkspaceBytes) report it. The knobs live in knobs.cpp, every kept or
// borrowed piece of device memory in workspaces.cpp, the sputnik::block
// overload set in block_api.cpp.
#include <algorithm>
#include <cstdint>
#include <mutex>

#include "api_internal.h"
#include "block_gemm.h"
#include "dispatch_internal.h"
#include "dsd4w.h"
#include "metadata.h"
#include "sputnik/sputnik.h"
#include "sputnik_amd.h"

namespace sputnik_amd {

// Experiment builds (SPUTNIK_EXP & 128 / 512) copy this into
// GemmParams::debug.
static unsigned long long *g_debug = nullptr;

static bool PairsEnabled() {
#ifdef SPUTNIK_NO_PAIRS
  return false;
#endif
  return Knob(kKnobPairs) != 0;
}

// Fills the pair fields of p when pair balancing applies: a staggered
// one-workgroup-per-CU tile config, every tile resident at once (the point
// is the tail of a single wave of tiles) and rows rankable in-kernel. Below
// a mean of 2 blocks per row the hand-offs cost more than the tail they
// shorten (DSD 4096² at 5%: 23.7 µs with pairs, 20.3 µs without; unchanged
// from 7% up, same-process A/B r01l).
#ifndef SPUTNIK_PAIR_MIN_MEAN4
#define SPUTNIK_PAIR_MIN_MEAN4 8  // 4 x mean blocks per row
#endif
// dry: decide only (the queries): no workspace is allocated, re-tied or
// advanced, and the pointers stay null.
// allow_split = false (accumulating calls): pairs only, never split mode; the
// tile widths and the grid stay those of the non-split launch.
static void PreparePairs(GemmParams *p, long long blocks, hipStream_t stream,
                         bool dry = false, bool allow_split = true) {
  p->pair = 0;
  if (!CfgSparse::kStagger || CfgSparse::kWGs != 1)
    return;
  if (!PairsEnabled() || p->num_rows < 2 || p->num_rows > kLptRows) return;
  if (blocks * 4 < (long long)p->num_rows * SPUTNIK_PAIR_MIN_MEAN4) return;
  if (stream == hipStreamPerThread) return;  // many streams, one handle
  // More tiles than resident workgroups never pair (the check on slot->slots
  // below): decided here, before a workspace is looked up or allocated, so
  // such a launch allocates nothing (e.g. DSD NT through a caller's
  // transposed-B workspace, 16384 x 2048 out of a dense A).
  {
    int dev = 0;
    const int cus = hipGetDevice(&dev) == hipSuccess ? DeviceCUs(dev) : 0;
    if (cus > 0 && p->num_tiles > cus * CfgSparse::kWGs) return;
  }
  const int slots = BindPairWorkspace(p, p->num_tiles, stream, dry);
  if (slots == 0) return;
  p->pair = 1;
  p->pair_fault = Knob(kKnobPairFault);
  // Two panels x half the pairs per XCD (GemmParams::pair_xcd2) from a mean
  // of 8 blocks per row: DSD 4096^3 A/B (r02m) 30% / 50% / 90% +1.2 / +2.7
  // / +2.8%, 10% -4.4%. SPUTNIK_AMD_PAIR_XCD2=0 turns it off. Mode 3 (the
  // default) gives the heavy half of the pairs (the ones with hand-offs) to
  // the odd XCD of each panel pair: per-workgroup timelines (r04f/g,
  // scripts/exp_timeline4w.py) show logical XCDs 0/2/4/6 running the same
  // k-loop ~6% slower per block than 1/3/7 on every box measured, and mode
  // 1 had put the critical pairs exactly there (4-wave A/B, separate
  // processes, 30/50/90%: +1.0/+2.1/+1.4%, 10% +0.5%). Mode 2 interleaves
  // the pairs (r04d: +0.5% at 50%).
  const int xcd2 = Knob(kKnobPairXcd2);
  p->pair_xcd2 = xcd2 != 0 && blocks >= 8LL * p->num_rows ? xcd2 : 0;
  p->min_handoff = Knob(kKnobMinHandoff);
  // Split mode (GemmParams::pair_split) when the tiles fill at most half of
  // the workgroup slots (e.g. 512-2048-row panels of a strong-scaled 4096^2,
  // or narrow N) and the rows hold at least 4 blocks on average: two
  // workgroups per tile. SPUTNIK_AMD_SPLIT=0 turns it off. (r03b, DSD
  // K=N=4096 50%: M=512 45.2 -> 34.6 us, 1024 47.6 -> 38.4, 2048 48.8 ->
  // 45.2; 4 or 8 workgroups per tile were slower.)
  const int split_on = Knob(kKnobSplit);
  // Tile width: the narrowest of 512 / 256 / 128 columns whose tiles (two
  // workgroups each) still fit the slots, so a panel of few block-rows
  // fills the CUs (r03: M = 512 on 128-column tiles, M = 1024 on 256).
  int split = 1;
  if (allow_split && split_on != 0 &&
      (long long)p->num_tiles * 2 <= slots &&
      blocks >= 4LL * p->num_rows) {
    split = 2;
    int bn = CfgSparse::kBN;
    for (int cand : {256, 128}) {
      const long long tiles =
          (long long)p->num_rows * ((p->j_limit + cand - 1) / cand);
      if (tiles * 2 > slots) break;
      bn = cand;
    }
    // Tuning floor of the tile width: 512 keeps the wide tile. Only the
    // three instantiated widths are valid (Launch has split kernels for 128,
    // 256 and 512 columns); anything else is rounded up to the next one.
    const int mbn = Knob(kKnobSplitMinBn);
    const int max_narrow = mbn <= 128 ? 128 : mbn <= 256 ? 256 : CfgSparse::kBN;
    if (bn < max_narrow) bn = max_narrow;
    p->split_bn = bn;
    p->num_jtiles = (p->j_limit + bn - 1) / bn;
    p->num_tiles = p->num_rows * p->num_jtiles;
  }
  p->pair_split = split;
  if (split > 1) p->grid = split * p->num_tiles;
}

using sputnik::block::AsInt;

hipError_t BuildTransposed(const BlockMatrix &a, hipStream_t stream) {
  const int b = AsInt(a.block_size);
  if (b == 0) return hipErrorNotSupported;
  return LaunchTransposeMetadata(
      a.rows / b, a.cols / b, static_cast<int>(a.nonzeros / (b * b)),
      static_cast<const int *>(a.offsets),
      static_cast<const short *>(a.indices), static_cast<int *>(a.offsets_t),
      static_cast<short *>(a.indices_t), static_cast<int *>(a.block_offsets),
      stream);
}

namespace {

// C-ABI convention: never abort.
int AsCode(Status st) {
  switch (st) {
    case Status::kOk: return hipSuccess;
    case Status::kNotSupported: return hipErrorNotSupported;
    default: return hipErrorInvalidValue;
  }
}

// Grouped SDD tiles (CfgSddGrouped: up to 4 stored blocks of a block-row per
// workgroup) when there are enough groups to fill the CUs, the rows fit the
// in-kernel group scan, and every gathered D offset fits the 31-bit lane
// offset. Sets the grid to the upper bound nb/4 + rows; surplus workgroups
// exit at once.
constexpr int kMaxGroupRows = 32767;
bool UseGroupedSdd(GemmParams *p, const BlockMatrix &c, bool d_kc) {
#ifdef SPUTNIK_NO_GROUPED_SDD
  return false;
#endif
  if (Knob(kKnobGroupedSdd) == 0 || c.offsets == nullptr) return false;
  constexpr int kGrp = CfgSddGrouped::kBN / kBlock;
  const int blocks = p->num_tiles;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const int cus = DeviceCUs(dev);
  if (cus <= 0) return false;
  // From 4 blocks per CU the grouped tile is faster: the 4-wave grouped
  // kernel with its groups mapped over the actual group count (r05 gm2,
  // same process: SDD 4096^3 dense = 4 per CU, every transpose 100-103 us
  // vs 158-164 us on the k-split tile; 2 per CU 77 vs 76, 3.2 per CU 286 vs
  // 286: tie). r02's 8-wave grouped tile needed 5 per CU (scripts/
  // exp_grp.sh: 4 per CU k-split 318 vs grouped 362 us, 5 per CU 399 vs 365).
  // Knob "grouped_min_per_cu" (default 4) moves the switch (tuning only;
  // never below kGrp, so a grouped grid still fills every CU).
  static_assert(4 >= kGrp, "a grouped grid fills every CU");
  const int min_per_cu = Knob(kKnobGroupedMinPerCu) < kGrp ? kGrp
                                                             : Knob(kKnobGroupedMinPerCu);
  if (blocks < min_per_cu * cus || p->num_rows > kMaxGroupRows)
    return false;
  // D lane offsets: k-contiguous D gathers whole rows (n * ldb); otherwise
  // one 32-row k panel plus any column.
  const long long span = d_kc ? (long long)p->j_limit * p->d_ld
                              : 32LL * p->d_ld + (long long)p->j_limit * 2;
  if (span > kMaxLaneOffset) return false;
  p->c_offsets = static_cast<const int *>(c.offsets);
  p->num_tiles = blocks / kGrp + p->num_rows + 1;
  return true;
}

// SDD NN with too few stored blocks for the grouped grid (UseGroupedSdd
// false) and few enough groups that every group can take 2 or more
// workgroups: the 4-wave grouped kernel with each group's K split over S in
// {2, 4, 8} workgroups (GemmParams::sdd_ksplit, S chosen in-kernel from the
// actual group count), the partials reduced through the pair workspace.
// Grid = one workgroup per CU, all resident at once (one 160-KiB-LDS
// workgroup fits a CU): every chunk of a group is running while its peers
// wait for it. That all-to-all wait is why it is OFF by default (knob
// sdd_ksplit = 1): a launch that shares the device with another
// kernel holding CUs for longer than the 0.2 s bounded wait (an RCCL kernel
// on a side stream, a CU-masked stream) would leave chunks undispatched
// while their peers time out, and the launch would return NaN tiles (counted
// by sputnik_pair_errors()). Unlike the DSD pair hand-off -- a consumer waits
// only on a producer dispatched before it -- no chunk order avoids this, and
// a last-arriver reduction would serialize S - 1 partials on one CU (the
// gain at K = 8192 was 5%). Opt in with sputnik_tuning_set("sdd_ksplit", 8)
// when the launch has the device to itself.
// dry: decide only (SddPlan), no workspace allocated, re-tied or advanced.
static bool PrepareSddKsplit(GemmParams *p, const BlockMatrix &c, bool ta, bool tb,
                             hipStream_t stream, bool dry = false) {
  const int max_s = Knob(kKnobSddKsplit);
  if (max_s < 2 || ta || tb || c.offsets == nullptr || !Dsd4wEnabled()) return false;
  // From K = 6144 (knob sdd_ksplit_min_k): its fixed cost -- every chunk
  // publishes (S - 1) / S of its fp32 tile and reads as much back, ~10 us of
  // fabric traffic at 248 workgroups -- is paid back by the shorter k-loop
  // only on long K (A/B r05 ks2, us, 8-wave k-split tile vs K-split: 205
  // blocks of 4096^2 at K = 4096 40.2 vs 42.0 (S = 4), K = 8192 68.9 vs
  // 62.9 (S = 8); 60 blocks of 2048 x 4096, K = 4096 30.8 vs 31.0; 300
  // blocks, K = 2048 37.5 vs 38.0).
  if (p->num_rows > kMaxGroupRows || p->k_limit < Knob(kKnobSddKsplitMinK) ||
      p->k_limit % 128 != 0)
    return false;
  if (stream == hipStreamPerThread) return false;  // many streams, one handle
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const int cus = DeviceCUs(dev);
  if (cus <= 0) return false;
  // groups: sum over rows of ceil(n_r / 4) <= (blocks + 3 rows) / 4
  const long long blocks = p->num_tiles;
  const long long groups_ub = (blocks + 3LL * p->num_rows) / 4;
  if (groups_ub * 2 > cus) return false;
  const long long span = 32LL * p->d_ld + (long long)p->j_limit * 2;
  if (span > kMaxLaneOffset) return false;
  GemmParams q = *p;
  q.c_offsets = static_cast<const int *>(c.offsets);
  if (!Sdd4wApplies(q, true, ta, tb)) return false;
  if (BindPairWorkspace(&q, cus, stream, dry) == 0) return false;
  *p = q;
  p->num_tiles = cus;
  p->pair = 1;  // (the epoch and capture protocol of pair launches)
  p->pair_fault = Knob(kKnobPairFault);
  p->sdd_ksplit = max_s;
  return true;
}

// Tall sparse operands (more block-rows than the in-kernel row ranking
// handles, so no LPT order and no pair balancing) have many more tiles than
// CUs: they run on CfgTall, two workgroups per CU. Decides and sets the tall
// tile grid only; the persistent form and its tile counter are the 8-wave
// tall launch's alone (BindTileCounter, once the route knows it is that).
bool UseTall(GemmParams *p) {
  // knob "tall": 0 never, 2 always (experiments), 1 (default): tall only.
  const int mode = Knob(kKnobTall);
  if (mode == 0) return false;
  if (mode == 2) {
    // Forced tall (experiments): drop every pair-launch setting PreparePairs
    // made, split mode's grid and tile width included.
    p->pair = 0;
    p->pair_split = 1;
    p->split_bn = 0;
    p->grid = 0;
  } else if (p->num_rows <= kLptRows || p->pair != 0) {
    return false;
  }
  p->num_jtiles = (p->j_limit + CfgTall::kBN - 1) / CfgTall::kBN;
  p->num_tiles = p->num_rows * p->num_jtiles;
  return true;
}

}  // namespace

// Tall DSD NN on the 4-wave kernel, persistent (dsd4w.hip kEpi 7): one
// workgroup per CU walks a cost-balanced contiguous range of the
// panel-major block sequence (512-column panels) and stores each 128 x 512
// tile through a free ring slot as soon as its last block is done, the next
// tile's first DMAs in flight meanwhile; the empty rows' tiles are
// zero-filled after, an equal share per workgroup. Needs whole 512-column
// panels, at most 128 blocks and 64 zero chunks per workgroup, and rows that
// fit the LDS copy of the offsets.
static bool UseTallPipe(const GemmParams &p, long long blocks, long long row_max, bool s_kc,
                        bool d_kc) {
  if (Knob(kKnobTall4w) == 0 || !Dsd4wEnabled() || !s_kc || d_kc) return false;
  if (p.pair != 0 || p.pair_split > 1 || CfgSparse::kBN != 512) return false;
  if (p.j_limit % 512 != 0 || p.num_rows > 32767 || blocks <= 0) return false;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const int cus = DeviceCUs(dev);
  if (cus <= 0) return false;
  // blocks per workgroup: a weighted share (a tile weighs its blocks + 1:
  // blocks + non-empty rows per panel) plus the tile the cut runs into
  // (weight w quarter blocks per tile: blocks + w / 4 x non-empty rows)
  const long long fw = Knob(kKnobTallFlushW);
  const long long per =
      ((4 * blocks + fw * std::min<long long>(blocks, p.num_rows)) * (p.j_limit / 512) +
       4LL * cus - 1) / (4LL * cus);
  // (the empty rows' zero chunks: a share of at most panels x rows; the
  // odd-XCD share scales both by up to 2 max(odd, 100) / (100 + odd))
  const long long odd = Knob(kKnobTallOddShare), big = std::max<long long>(odd, 100);
  const long long zero_per =
      ((long long)(p.j_limit / 512) * p.num_rows * 2 * big + cus * (100 + odd) - 1) /
      (cus * (100 + odd));
  const long long per_x = (per * 2 * big + (100 + odd) - 1) / (100 + odd) + 1;
  return per_x + row_max <= 128 && zero_per <= 63 && blocks < (1LL << 24) &&
         p.j_limit / 512 < 256;
}

// ---- routes: decided once ---------------------------------------------------
// Which kernel runs a call, with which GemmParams, is decided by one function
// per product. A launch (Run*) computes the route in commit mode and
// executes it; a query computes it dry and reports it. dry is the `dry` of
// PreparePairs, PrepareSddKsplit and BindTileCounter: everything is decided,
// and no workspace is allocated, re-tied or advanced.

// How a route looks at the transposed copy of B (SDD NT / TT, DSD NT).
// kOff: not at all, the product runs on B as stored (what follows a copy, a
// call whose memory did not fit, SddPlan). kProblem: the path applies to the
// problem (what a launch asks before TransposeB looks for memory; the
// workspace and epilogue-route queries). kLibrary: it applies and the
// library's own buffer may serve `stream` -- no workspace known: DsdPlan and
// SddKernel have no workspace argument and do not consult the registrations,
// so with a registered or per-call workspace they can differ from the launch
// (which copies even where the library route is closed, and keeps the NT
// kernel where that memory does not fit).
enum class BtView { kOff, kProblem, kLibrary };

static bool BtViewOpen(BtView view, hipStream_t stream) {
  return view == BtView::kProblem || (view == BtView::kLibrary && BtLibraryStreamOk(stream));
}

// DSD and DDS. bt (DSD only): the call continues on the transposed copy of
// B; the rest of the route is then that of the NN product on the copy and
// is left undecided here. code: what DsdPlan / DdsPlan report, 0 the 8-wave
// 128 x 512 tile, 1 the 4-wave kernel, 2 the tall configuration, 3 split
// mode on the 8-wave kernel, 4 (DSD) the tall pipeline, -1 rejected.
struct DenseRoute : Product {
  explicit DenseRoute(const Product &bound) : Product(bound) {}
  bool bt = false;
  int code = -1;
  bool tall = false;
  int epi = 0;  // the 4-wave kernel's epilogue variant (codes 1 and 4)
};

// The chain both dense-output products share, on r->p as bound (r->out_t:
// DDS, the transposed-output product). Accumulating calls (out != kStore):
// always the 8-wave kernel, with pairs where PreparePairs grants them (never
// split mode) or the tall configuration; fp32 C has rows of ldc x 4 bytes.
static void RouteDenseOut(DenseRoute *r, hipStream_t stream, OutMode out, bool dry) {
  GemmParams &p = r->p;
  const bool dds = r->out_t;
  const long long blocks = r->s_sparse->nonzeros / (kBlock * kBlock);
  const bool acc = out != OutMode::kStore;
  if (out == OutMode::kAccF32) p.c_ld *= 2;
  if (!acc) p.xcd_rows = Knob(kKnobXcdRows);
  PreparePairs(&p, blocks, stream, dry, /*allow_split=*/!acc);
  GemmParams t = p;  // (p stays as it is before the tall configuration)
  r->tall = UseTall(&t);
  if (r->tall && !acc && !dds &&
      UseTallPipe(p, blocks, ((long long)r->s_sparse->cols + kBlock - 1) / kBlock, r->s_kc,
                  r->d_kc)) {
    p.persistent = 0;
    p.num_jtiles = p.j_limit / 512;
    p.tall_flush_w = Knob(kKnobTallFlushW);
    p.tall_odd_share = Knob(kKnobTallOddShare);
    int dev = 0;
    p.num_tiles = hipGetDevice(&dev) == hipSuccess ? DeviceCUs(dev) : 0;
    r->code = 4;
    r->epi = 7;
    return;
  }
  if (r->tall) {
    // the 8-wave tall path alone takes a persistent tile counter (the tall
    // pipeline above needs none)
    p = t;
    BindTileCounter(&p, stream, dry);
  }
  const long long blocks4w = Dsd4wForced() ? (1LL << 40) : blocks;
  if (acc || !Dsd4wEnabled() ||
      !(dds ? Dds4wApplies : Dsd4wApplies)(p, blocks4w, r->s_kc, r->d_kc, dds, r->tall)) {
    r->code = r->tall ? 2 : p.pair != 0 && p.pair_split > 1 ? 3 : 0;
    return;
  }
  r->code = 1;
  r->epi = Dsd4wEpi();
  if (dds) {
    // (the two-panel pair placement, heavy pairs on the odd XCDs: DDS NN
    // A/B r05 dx, same process, mode 0 -> 3: 10% 24.49 -> 24.41, 20% 32.44
    // -> 32.33, 30% 40.03 -> 38.69, 50% 56.75 -> 55.06, 90% 89.76 -> 87.64 us)
    if (p.pair_xcd2 != 0) p.pair_xcd2 = Knob(kKnobDdsXcd2);
  } else if (Knob(kKnobDsd4w) == 1 && blocks < 12LL * p.num_rows) {
    // Default epilogue by density: below a mean of 12 blocks per block-row
    // the copy-out interleaved with the staging (kEpi 5) is ahead (DSD NN
    // 4096^3 A/B r04ae, two runs: 10% +1.5 / +1.2%, 30% +1.0 / +0.5%), at
    // 50% behind (-0.6 / -0.3%).
    r->epi = 5;
  }
}

// The same for DSD NT over a nearly dense A as for SDD (BtAppliesSdd
// below; out = A . B with B^T stored [N][K] past the MALL): the sweep's DSD
// NT 16384^3 dense ran 7620 us against NN's 6354, while at 50% NT is as fast
// as NN (3352 vs 3397 us), so the gate asks for >= kDsdBtMinRatio FLOPs per
// byte of B, 16384 blocks / K (16384^3: dense 16384, 50% 8192). Never for an
// accumulating call: op(B) = B^T runs the NT kernel directly.
constexpr long long kDsdBtMinRatio = 15000;
static bool BtAppliesDsd(const BlockMatrix &a, bool ta, const Matrix &b, bool tb) {
  if (!tb || ta || !BtGate(b)) return false;
  const long long blocks = a.nonzeros / (kBlock * kBlock);
  return blocks * 16384 >= kDsdBtMinRatio * b.cols;
}

static DenseRoute RouteDsd(const BlockMatrix &a, bool ta, const Matrix &b, bool tb,
                           const Matrix &c, hipStream_t stream, OutMode out, bool dry,
                           BtView view) {
  DenseRoute r(Bind(a, ta, b, tb, c));
  if (r.status != Status::kOk) return r;
  r.bt = out == OutMode::kStore && view != BtView::kOff && BtAppliesDsd(a, ta, b, tb) &&
         BtViewOpen(view, stream);
  if (!r.bt) RouteDenseOut(&r, stream, out, dry);
  return r;
}

static DenseRoute RouteDds(const Matrix &a, bool ta, const BlockMatrix &b, bool tb,
                           const Matrix &c, hipStream_t stream, OutMode out, bool dry) {
  DenseRoute r(Bind(a, ta, b, tb, c));
  if (r.status == Status::kOk) RouteDenseOut(&r, stream, out, dry);
  return r;
}

// SDD. bt: the call continues on the transposed copy of B; the rest is then
// that of the N-major product on the copy and is left undecided here
// (kernel 4). plan: what SddPlan reports, 0 one k-split 128 x 128 block per
// workgroup, 1 grouped tiles, 2 grouped tiles with each group's K split, -1
// rejected. kernel: what SddKernel reports, 0 the 8-wave k-split tile, 1
// grouped tiles on the 8-wave kernel, 2 the 4-wave K-split, 3 grouped tiles
// on the 4-wave kernel, 4 B transposed first, -1 rejected.
struct SddRoute : Product {
  bool bt = false;
  bool grouped = false;
  int plan = -1;
  int kernel = -1;
  bool tail = false;  // kernel 3: the tail split's second launch follows
};

static bool BtAppliesSdd(const Matrix &a, bool ta, const Matrix &b, bool tb,
                         const BlockMatrix &c, hipStream_t stream);

// fused: the route of the fused epilogue products, which only the 8-wave
// kernel has: no transposed copy, no K-split, no 4-wave kernel.
static SddRoute RouteSdd(const Matrix &a, bool ta, const Matrix &b, bool tb,
                         const BlockMatrix &c, hipStream_t stream, bool dry, BtView view,
                         bool fused = false) {
  SddRoute r;
  GemmParams &p = r.p;
  static_cast<Product &>(r) = Bind(a, ta, b, tb, c);
  if (r.status != Status::kOk) return r;
  if (!fused && view != BtView::kOff && BtAppliesSdd(a, ta, b, tb, c, stream) &&
      BtViewOpen(view, stream)) {
    r.bt = true;
    r.kernel = 4;
    return r;
  }
  const long long blocks = p.num_tiles;
  r.grouped = UseGroupedSdd(&p, c, tb);
  r.plan = r.kernel = r.grouped ? 1 : 0;
  if (fused) return r;
  if (!r.grouped && PrepareSddKsplit(&p, c, ta, tb, stream, dry)) {
    r.plan = r.kernel = 2;
    return r;
  }
  if (Dsd4wEnabled() && Sdd4wApplies(p, r.grouped, ta, tb, blocks)) {
    r.kernel = 3;
    p.sdd_order = Knob(kKnobSddOrder);
    p.sdd_krot = Knob(kKnobSddKrot);
    const int spread = Knob(kKnobSddSpread);
    p.sdd_spread = spread == 1 || (spread == 2 && tb && !ta) ? 1 : 0;
    // Tail split (block_gemm.h sdd_tail_rows): with K >= sdd_tail_min_k a
    // grouped round is long, so the rows past the full rounds are better
    // served one block per workgroup by the 8-wave k-split tile, launched
    // right behind on the same stream (both launches find the same R0).
    // Only while A and B fit the 256-MB MALL: that tile streams a whole
    // row panel of A and column panel of B per block, and past the MALL it
    // ran slower than the round it saves (SDD 16384^3 50%: NN 3428 -> 3644
    // us, 8192^3 50%: 494 -> 445 us, profiles/r06/ab/sdd_tail_ab.jsonl).
    int dev = 0;
    const long long tail_k = Knob(kKnobSddTailMinK);
    const long long ab_bytes = 2LL * p.k_limit * ((long long)p.num_rows * kBM + p.j_limit);
    r.tail = tail_k > 0 && p.k_limit >= tail_k && ab_bytes <= (256LL << 20) &&
             hipGetDevice(&dev) == hipSuccess && DeviceCUs(dev) > 0;
    if (r.tail) {
      p.sdd_tail = 1;
      p.tail_cus = DeviceCUs(dev);
    }
  }
  return r;
}

// ---- SDD with B stored transposed, over operands past the MALL -------------
// (workspaces.cpp has the path and its memory.) Gate: B's K N 2 bytes >= knob
// sdd_bt_min_mib MiB (BtGate), and the product's FLOPs per byte of B (blocks
// 128^2 2 K / (K N 2) = 16384 blocks / N) >= kBtMinRatio, so the copy is a
// small part of the launch (16384^3: 50% 8192, dense 16384, 10% 1639 --
// below; MegaBlocks' x.w1^T 1024 -- below); the N-major product on the copy
// must take the 4-wave grouped kernel, which its own route says.
constexpr long long kBtMinRatio = 3000;
static bool BtAppliesSdd(const Matrix &a, bool ta, const Matrix &b, bool tb,
                         const BlockMatrix &c, hipStream_t stream) {
  if (!tb || !BtGate(b)) return false;
  const long long blocks = c.nonzeros / (kBlock * kBlock);
  if (blocks * 16384 < kBtMinRatio * b.rows) return false;
  const Matrix bt(b.cols, b.rows, b.data);
  return RouteSdd(a, ta, bt, false, c, stream, /*dry=*/true, BtView::kOff).kernel == 3;
}

// Bytes of the transposed copy the path would use for this problem under the
// current knobs (a multiple of 256), 0 when the path does not apply. Host
// only: ignores the capture state, allocates and launches nothing.
size_t SddWorkspaceBytes(const Matrix &a, bool ta, const Matrix &b, bool tb,
                         const BlockMatrix &c) {
  return RouteSdd(a, ta, b, tb, c, nullptr, /*dry=*/true, BtView::kProblem).bt ? BtBytes(b) : 0;
}
size_t DsdWorkspaceBytes(const BlockMatrix &a, bool ta, const Matrix &b, bool tb,
                         const Matrix &c) {
  return RouteDsd(a, ta, b, tb, c, nullptr, OutMode::kStore, /*dry=*/true, BtView::kProblem).bt
             ? BtBytes(b)
             : 0;
}

// ---- shared entry points: execute the route ---------------------------------

// What every product with a sparse input does between its route and its
// launch: the transposed metadata a flagged operand is read through is built
// when its descriptor says so (create_metadata; the ...Ex forms clear it on
// their copy), S's before D's.
static hipError_t BeforeLaunch(Product *r, hipStream_t stream) {
  for (const BlockMatrix *m : {r->s_meta ? r->s_sparse : nullptr, r->d_meta ? r->d_sparse : nullptr})
    if (m != nullptr && m->create_metadata) {
      const hipError_t e = BuildTransposed(*m, stream);
      if (e != hipSuccess) return e;
    }
  r->p.debug = g_debug;
  return hipSuccess;
}

// DSD and DDS once routed. (ta, tb pick the 4-wave kernel's variant: NT, TN
// or TT of the problem as the caller states it.)
static hipError_t LaunchDenseOut(DenseRoute *r, bool ta, bool tb, int dtype, OutMode out,
                                 hipStream_t stream) {
  const hipError_t e = BeforeLaunch(r, stream);
  if (e != hipSuccess) return e;
  if (out != OutMode::kStore)
    return LaunchBlockGemmAcc(dtype, r->s_kc, r->d_kc, r->out_t, r->tall,
                              out == OutMode::kAccF32 ? kOutAccF32 : kOutAccT, r->p, stream);
  switch (r->code) {
    case 4: return LaunchDsd4w(dtype, r->p, r->epi, false, stream, false, false);
    case 1:
      return (r->out_t ? LaunchDds4w : LaunchDsd4w)(dtype, r->p, r->epi, tb && !ta, stream,
                                                    ta && !tb, ta && tb);
    default:
      return LaunchBlockGemm(dtype, false, r->s_kc, r->d_kc, r->out_t, r->tall, r->p, stream);
  }
}

hipError_t RunDsd(const BlockMatrix &a, bool ta, const Matrix &b, bool tb,
                  const Matrix &c, int dtype, hipStream_t stream,
                  Status *st_out, Workspace ws, OutMode out) {
  const InProduct in_product;
  DenseRoute r = RouteDsd(a, ta, b, tb, c, stream, out, /*dry=*/false, BtView::kProblem);
  *st_out = r.status;
  if (r.status != Status::kOk) return hipSuccess;
  if (r.bt) {
    const BtCopy copy = TransposeB(b, stream, ws);
    if (copy.error != hipSuccess) return copy.error;
    if (copy.data != nullptr)
      return RunDsd(a, ta, Matrix(b.cols, b.rows, copy.data), false, c, dtype, stream, st_out,
                    Workspace{}, OutMode::kStore);
    r = RouteDsd(a, ta, b, tb, c, stream, out, /*dry=*/false, BtView::kOff);
  }
  return LaunchDenseOut(&r, ta, tb, dtype, out, stream);
}

hipError_t RunDds(const Matrix &a, bool ta, const BlockMatrix &b, bool tb,
                  const Matrix &c, int dtype, hipStream_t stream,
                  Status *st_out, OutMode out) {
  const InProduct in_product;
  DenseRoute r = RouteDds(a, ta, b, tb, c, stream, out, /*dry=*/false);
  *st_out = r.status;
  if (r.status != Status::kOk) return hipSuccess;
  return LaunchDenseOut(&r, ta, tb, dtype, out, stream);
}

hipError_t RunSdd(const Matrix &a, bool ta, const Matrix &b, bool tb,
                  const BlockMatrix &c, int dtype, hipStream_t stream,
                  Status *st_out, Workspace ws) {
  const InProduct in_product;
  SddRoute r = RouteSdd(a, ta, b, tb, c, stream, /*dry=*/false, BtView::kProblem);
  *st_out = r.status;
  if (r.status != Status::kOk) return hipSuccess;
  if (r.bt) {
    const BtCopy copy = TransposeB(b, stream, ws);
    if (copy.error != hipSuccess) return copy.error;
    if (copy.data != nullptr)
      return RunSdd(a, ta, Matrix(b.cols, b.rows, copy.data), false, c, dtype, stream, st_out,
                    Workspace{});
    r = RouteSdd(a, ta, b, tb, c, stream, /*dry=*/false, BtView::kOff);
  }
  r.p.debug = g_debug;
  switch (r.kernel) {
    case 2: return LaunchSdd4w(dtype, r.p, ta, tb, Dsd4wEpi(), stream);
    case 3: {
      const hipError_t e = LaunchSdd4w(dtype, r.p, ta, tb, Dsd4wEpi(), stream);
      if (e != hipSuccess || !r.tail) return e;
      GemmParams q = r.p;
      q.num_tiles = (int)(c.nonzeros / (kBlock * kBlock));
      q.grid = r.p.tail_cus;
      q.sdd_order = 0;
      return LaunchBlockGemm(dtype, true, /*s_kc=*/!ta, /*d_kc=*/tb, false,
                             /*grouped=*/false, q, stream);
    }
    default:
      return LaunchBlockGemm(dtype, true, /*s_kc=*/!ta, /*d_kc=*/tb, false, r.grouped, r.p,
                             stream);
  }
}

// ---- SDD epilogue products (sputnik/block/activation.h, gated.h) ----

static bool ActOk(int act) {
  return act == kActRelu || act == kActGelu || act == kActSilu;
}

// What the host code needs of SddEpilogue<mode>; side_inputs < 0: not an
// epilogue mode.
struct EpilogueShape {
  int side_inputs;
  bool keeps_x, second_output;
};
static EpilogueShape ShapeOf(int mode) {
  return WithSddEpilogue(mode, EpilogueShape{-1, false, false}, [](auto e) {
    using E = decltype(e);
    return EpilogueShape{E::kSideInputs, E::kKeepsX, E::kSecondOutput};
  });
}

hipError_t RunBlockEpilogue(int dtype, int act, int mode, const void *x,
                            const void *s0, const void *s1, void *o0,
                            void *o1, long long n, hipStream_t stream) {
  const EpilogueShape e = ShapeOf(mode);
  if (!ActOk(act) || e.side_inputs < 0 || (dtype != 0 && dtype != 1) || n < 0)
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (x == nullptr || o0 == nullptr || (e.side_inputs >= 1 && s0 == nullptr) ||
      (e.side_inputs >= 2 && s1 == nullptr) ||
      (e.second_output && o1 == nullptr) || o0 == o1)
    return hipErrorInvalidValue;
  int dev = 0;
  const int cus = hipGetDevice(&dev) == hipSuccess ? DeviceCUs(dev) : 0;
  return LaunchBlockEpilogue(dtype, mode, act, x, s0, s1, o0, o1, n, cus,
                             stream);
}

// The route of one epilogue call, a function of the SDD route and the knob
// sdd_act_route: 2 (two kernels) when the knob says so, or when it is 0 and
// the plain call would or might leave the 8-wave kernel -- the transposed-B
// path applies to the problem (whether it is then taken depends on the
// stream and the workspace: RunSdd's business), the 4-wave K-split, grouped
// tiles on the 4-wave kernel (with or without the tail split) -- and 1
// (fused) otherwise, the 8-wave k-split tile or grouped tile; *r then holds
// what the fused launch needs. -1 rejected (r->status).
// profiles/sdd_activation has the A/B behind the boundary.
static int SddActRouteOf(const Matrix &a, bool ta, const Matrix &b, bool tb,
                         const BlockMatrix &c, hipStream_t stream, SddRoute *r) {
  const int knob = Knob(kKnobSddActRoute);
  *r = RouteSdd(a, ta, b, tb, c, stream, /*dry=*/true, BtView::kProblem, /*fused=*/knob == 1);
  if (r->status != Status::kOk) return -1;
  if (knob != 0) return knob;
  return r->bt || r->kernel == 2 || r->kernel == 3 ? 2 : 1;
}

int SddActRoute(const Matrix &a, bool ta, const Matrix &b, bool tb,
                const BlockMatrix &c) {
  SddRoute r;
  return SddActRouteOf(a, ta, b, tb, c, nullptr, &r);
}

// The buffer rules of gated.h: required pointers set, and no two of gate,
// up, up_grad, c.data, A, B equal, up_grad == up excepted.
static bool GatedBuffersOk(const Matrix &a, const Matrix &b,
                           const BlockMatrix &c, const void *gate,
                           const void *up, const void *up_grad, bool grad) {
  if (gate == nullptr) return false;
  if (grad && (up == nullptr || up_grad == nullptr)) return false;
  const void *fixed[3] = {c.data, a.data, b.data};
  const void *side[3] = {gate, up, grad ? up_grad : nullptr};
  for (const void *s : side)
    for (const void *f : fixed)
      if (s != nullptr && s == f) return false;
  if (up != nullptr && up == gate) return false;
  if (grad && up_grad == gate) return false;
  return true;
}

// Both entry points: bias null, no bias stage (the caller has checked the
// bias's own rules).
static hipError_t SddEpilogueRun(const Matrix &a, bool ta, const Matrix &b,
                                 bool tb, const BlockMatrix &c, int dtype,
                                 int act, int mode, void *side0, void *side1,
                                 void *out1, const void *bias,
                                 hipStream_t stream, Status *st_out,
                                 Workspace ws) {
  SddRoute r;
  const int route = SddActRouteOf(a, ta, b, tb, c, stream, &r);
  *st_out = r.status;
  if (r.status != Status::kOk) return hipSuccess;
  const EpilogueShape e = ShapeOf(mode);
  if (!ActOk(act) || e.side_inputs < 0) return hipErrorInvalidValue;
  // (activation.h: Z required by the gradient, and never C itself)
  const bool buffers_ok =
      mode == kOutGate || mode == kOutGateGrad
          ? GatedBuffersOk(a, b, c, side0, side1, out1, mode == kOutGateGrad)
          : !(mode == kOutActGrad && side0 == nullptr) &&
                !(side0 != nullptr && side0 == c.data);  // (kOutBias: no side)
  if (!buffers_ok) return hipErrorInvalidValue;
  void *const side[2] = {side0, side1};
  if (route == 2) {
    // Two kernels: the plain SDD, whatever it runs, into the buffer that
    // keeps x (when the op has one and it is wanted) or C, and the
    // elementwise stage behind it on the stream, in place where x is in C.
    BlockMatrix prod = c;
    if (e.keeps_x && side[e.side_inputs] != nullptr)
      prod.data = side[e.side_inputs];
    const hipError_t err =
        RunSdd(a, ta, b, tb, prod, dtype, stream, st_out, ws);
    if (err != hipSuccess || *st_out != Status::kOk) return err;
    if (bias == nullptr)
      return RunBlockEpilogue(dtype, act, mode, prod.data,
                              e.side_inputs >= 1 ? side0 : nullptr,
                              e.side_inputs >= 2 ? side1 : nullptr, c.data,
                              e.second_output ? out1 : nullptr, c.nonzeros,
                              stream);
    // (the forward ops: at most one side input, no second output)
    if (c.nonzeros <= 0) return hipSuccess;
    if (c.indices == nullptr || (dtype != 0 && dtype != 1))
      return hipErrorInvalidValue;
    int dev = 0;
    const int cus = hipGetDevice(&dev) == hipSuccess ? DeviceCUs(dev) : 0;
    return LaunchBlockEpilogue(dtype, mode, act, prod.data,
                               e.side_inputs >= 1 ? side0 : nullptr, nullptr,
                               c.data, nullptr, c.nonzeros, cus, stream, bias,
                               static_cast<const short *>(c.indices),
                               c.cols / kBlock);
  }
  // Fused: the 8-wave kernel with the route's own params and tile plan.
  const InProduct in_product;
  GemmParams &p = r.p;
  p.debug = g_debug;
  p.act = act;
  p.z_data = static_cast<char *>(side0);
  p.u_data = static_cast<char *>(side1);
  p.du_data = static_cast<char *>(out1);
  p.bias = static_cast<const char *>(bias);
  return LaunchBlockGemmEpilogue(dtype, /*s_kc=*/!ta, /*d_kc=*/tb, r.grouped,
                                 mode, p, stream);
}

hipError_t RunSddEpilogue(const Matrix &a, bool ta, const Matrix &b, bool tb,
                          const BlockMatrix &c, int dtype, int act, int mode,
                          void *side0, void *side1, void *out1,
                          hipStream_t stream, Status *st_out, Workspace ws) {
  // (kOutBias is the bias entry point's alone)
  if (mode == kOutBias) {
    *st_out = Status::kOk;
    return hipErrorInvalidValue;
  }
  return SddEpilogueRun(a, ta, b, tb, c, dtype, act, mode, side0, side1, out1,
                        nullptr, stream, st_out, ws);
}

hipError_t RunSddEpilogueBias(const Matrix &a, bool ta, const Matrix &b,
                              bool tb, const BlockMatrix &c, int dtype,
                              int act, int mode, void *side0, void *side1,
                              const void *bias, hipStream_t stream,
                              Status *st_out, Workspace ws) {
  *st_out = Status::kOk;
  if (mode != kOutBias && mode != kOutAct && mode != kOutGate)
    return hipErrorInvalidValue;
  if (bias == nullptr || bias == c.data || bias == a.data || bias == b.data ||
      bias == side0 || bias == side1)
    return hipErrorInvalidValue;
  // (kOutBias has no activation: any valid code)
  return SddEpilogueRun(a, ta, b, tb, c, dtype,
                        mode == kOutBias ? kActRelu : act, mode, side0, side1,
                        nullptr, bias, stream, st_out, ws);
}

// SSD, SDS and DSS: no route to decide, one kernel each.
static hipError_t RunBound(Product r, int dtype, hipStream_t stream, Status *st_out) {
  const InProduct in_product;
  *st_out = r.status;
  if (r.status != Status::kOk) return hipSuccess;
  const hipError_t e = BeforeLaunch(&r, stream);
  if (e != hipSuccess) return e;
  return r.d_sparse != nullptr
             ? LaunchBlockGemmDss(dtype, r.s_kc, r.d_kc, r.p, stream)
             : LaunchBlockGemmSparseIn(dtype, r.s_kc, r.d_kc, r.out_t, r.p, stream);
}

hipError_t RunSsd(const BlockMatrix &a, bool ta, const Matrix &b, bool tb,
                  const BlockMatrix &c, int dtype, hipStream_t stream,
                  Status *st_out) {
  return RunBound(Bind(a, ta, b, tb, c), dtype, stream, st_out);
}

hipError_t RunSds(const Matrix &a, bool ta, const BlockMatrix &b, bool tb,
                  const BlockMatrix &c, int dtype, hipStream_t stream,
                  Status *st_out) {
  return RunBound(Bind(a, ta, b, tb, c), dtype, stream, st_out);
}

hipError_t RunDss(const BlockMatrix &a, bool ta, const BlockMatrix &b,
                  bool tb, const Matrix &c, int dtype, hipStream_t stream,
                  Status *st_out) {
  return RunBound(Bind(a, ta, b, tb, c), dtype, stream, st_out);
}

int StatusCode(Status st) { return AsCode(st); }

// ---- queries: report the route (dry: nothing launched, allocated, re-tied or
// advanced; safe during a capture) -------------------------------------------

// The SDD tile plan on B as it is stored, on the null stream.
int SddPlan(const void *a, bool ta, const void *b, bool tb, const void *c) {
  if (!a || !b || !c) return -1;
  return RouteSdd(*static_cast<const Matrix *>(a), ta, *static_cast<const Matrix *>(b), tb,
                  *static_cast<const BlockMatrix *>(c), nullptr, /*dry=*/true, BtView::kOff)
      .plan;
}

// The kernel behind SddPlan's tile plan. It has no stream and no workspace
// argument: it answers for the null stream with no workspace known
// (BtView::kLibrary), and reports 4 only where the product on B as it is
// stored would take grouped tiles, while a launch copies B wherever the path
// applies to the problem.
int SddKernel(const void *a, bool ta, const void *b, bool tb, const void *c) {
  if (!a || !b || !c) return -1;
  const Matrix &am = *static_cast<const Matrix *>(a), &bm = *static_cast<const Matrix *>(b);
  const BlockMatrix &cm = *static_cast<const BlockMatrix *>(c);
  const SddRoute r = RouteSdd(am, ta, bm, tb, cm, nullptr, /*dry=*/true, BtView::kOff);
  if (r.plan == 1 && RouteSdd(am, ta, bm, tb, cm, nullptr, /*dry=*/true, BtView::kLibrary).bt)
    return 4;
  return r.kernel;
}

int DdsPlan(const void *a, bool ta, const void *b, bool tb, const void *c,
            hipStream_t stream) {
  if (!a || !b || !c) return -1;
  return RouteDds(*static_cast<const Matrix *>(a), ta, *static_cast<const BlockMatrix *>(b),
                  tb, *static_cast<const Matrix *>(c), stream, OutMode::kStore, /*dry=*/true)
      .code;
}

// Where DSD NT transposes B first, the plan of the NN product that follows.
// It has no workspace argument and does not consult the registrations: no
// workspace known (BtView::kLibrary).
int DsdPlan(const void *a, bool ta, const void *b, bool tb, const void *c,
            hipStream_t stream) {
  if (!a || !b || !c) return -1;
  const BlockMatrix &am = *static_cast<const BlockMatrix *>(a);
  const Matrix &bm = *static_cast<const Matrix *>(b), &cm = *static_cast<const Matrix *>(c);
  const DenseRoute r =
      RouteDsd(am, ta, bm, tb, cm, stream, OutMode::kStore, /*dry=*/true, BtView::kLibrary);
  if (!r.bt) return r.code;
  return RouteDsd(am, ta, Matrix(bm.cols, bm.rows, bm.data), false, cm, stream,
                  OutMode::kStore, /*dry=*/true, BtView::kOff)
      .code;
}

// Host-only acceptance test (no launch, no device needed): op 0 = DSD
// (a: block, b/c: dense), 1 = DDS (b: block), 2 = SDD (c: block), 3 = SSD
// (a, c: block), 4 = SDS (b, c: block), 5 = DSS (a, b: block). The C
// descriptors share the C++ layout (static_asserts in c_api.cpp).
bool CanImplement(int op, const void *a, bool ta, const void *b, bool tb,
                  const void *c) {
  static const bool kIsBlock[6][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1},
                                    {1, 0, 1}, {0, 1, 1}, {1, 1, 0}};
  if (!a || !b || !c || op < 0 || op > 5) return false;
  const auto as = [](const void *x, bool block) {
    return block ? Operand(*static_cast<const BlockMatrix *>(x))
                 : Operand(*static_cast<const Matrix *>(x));
  };
  return Bind(as(a, kIsBlock[op][0]), ta, as(b, kIsBlock[op][1]), tb, as(c, kIsBlock[op][2]))
             .status == Status::kOk;
}

}  // namespace sputnik_amd

// Experiment hook (not part of include/sputnik_amd.h): per-segment cycle
// sums / timelines of SPUTNIK_EXP & 128 / 512 builds (scripts/exp_build.sh).
// Only experiment builds export it; the shipped library has no such entry.
#if SPUTNIK_EXP != 0
extern "C" void sputnik_exp_set_debug(void *buffer) {
  sputnik_amd::g_debug = static_cast<unsigned long long *>(buffer);
}
#endif
