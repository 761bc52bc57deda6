// sputnik-amd: the pure part of the dispatcher: which descriptors a product
// accepts (Status) and how its operands bind to the kernel's GemmParams.
// Host arithmetic on descriptors only: no HIP call, no knob, no workspace.
// tests/operands_host.cpp pins every Status, metadata flag and GemmParams
// field it produces against tests/golden/operands.txt, recorded from the six
// hand-written functions this replaced; the order of the checks below (which
// Status a doubly wrong call gets) is part of that record.
//
// Replaces the can_launch_* bodies of the reference's *_align8.cu variants
// (shape rules, metadata checks, operand bundling; ssd.cu:7-24, sds.cu:7-24,
// dss.cu:9-24 for the sparse-sparse forms).
#include "api_internal.h"
#include "block_gemm.h"
#include "dispatch_internal.h"

namespace sputnik_amd {
namespace {

using sputnik::block::AsInt;
using sputnik::block::BlockSize;
using sputnik::block::MatmulShape;
using sputnik::block::ValidMatmul;

bool DenseOk(const Operand &m) {
  return m.rows >= 0 && m.cols >= 0 &&
         (m.data != nullptr || (long long)m.rows * m.cols == 0);
}

bool SparseOk(const BlockMatrix &s) {
  const int b = AsInt(s.block_size);
  if (b != 128) return false;
  if (s.rows < 0 || s.cols < 0 || s.nonzeros < 0) return false;
  if (s.rows % b != 0 || s.cols % b != 0 || s.nonzeros % (b * b) != 0)
    return false;
  if ((s.cols / b) > 32767 || (s.rows / b) > 32767) return false;  // int16
  if (s.offsets == nullptr) return false;
  if (s.nonzeros > 0 && (s.data == nullptr || s.indices == nullptr))
    return false;
  return true;
}

bool OperandOk(const Operand &x) {
  return x.sparse != nullptr ? SparseOk(*x.sparse) : DenseOk(x);
}

// The reference's BlockGemm::can_implement: m, n, k multiples of 8
// (block_gemm.h:728-745; 8 x fp16 = one 16-byte access).
bool Aligned8(const MatmulShape &s) {
  return s.m % 8 == 0 && s.n % 8 == 0 && s.k % 8 == 0 && s.m >= 0 &&
         s.n >= 0 && s.k >= 0;
}

// The stride rule of a dense operand: the rows of one DMA tile (`width` of
// them when the operand is k-contiguous, else a 64-deep k slice) times the
// byte stride must fit a 31-bit lane offset.
bool StrideOk(bool kc, int width, long long ld_elems) {
  return (kc ? width : 64) * ld_elems * 2 <= kMaxLaneOffset;
}

// A sparse operand's entry lists, in row order or, col_order, through its
// transposed metadata, which must then exist.
bool BindSparse(const BlockMatrix &s, bool col_order, const int **offsets,
                const short **indices, const int **block_offsets) {
  if (col_order && (s.offsets_t == nullptr || s.indices_t == nullptr ||
                    s.block_offsets == nullptr))
    return false;
  *offsets = static_cast<const int *>(col_order ? s.offsets_t : s.offsets);
  *indices = static_cast<const short *>(col_order ? s.indices_t : s.indices);
  *block_offsets =
      col_order ? static_cast<const int *>(s.block_offsets) : nullptr;
  return true;
}

// Dense C in tiles of `tile` columns of the j extent.
void BindDenseOut(const Operand &c, long long ldc, int tile, GemmParams *p) {
  p->c_data = static_cast<char *>(const_cast<void *>(c.data));
  p->c_ld = ldc * 2;
  p->num_jtiles = (p->j_limit + tile - 1) / tile;
  p->num_tiles = p->num_rows * p->num_jtiles;
}

// Sparse C, one stored block per tile: its row_indices are needed as soon as
// it has a block.
Status BindSparseOut(const BlockMatrix &c, GemmParams *p) {
  if (c.block_size != BlockSize::k128) return Status::kNotSupported;
  if (!SparseOk(c)) return Status::kNoKernel;
  const int blocks = c.nonzeros / (kBlock * kBlock);
  if (blocks > 0 && c.row_indices == nullptr)
    return Status::kMissingRowIndices;
  p->c_data = static_cast<char *>(c.data);
  p->c_row_indices = static_cast<const short *>(c.row_indices);
  p->c_indices = static_cast<const short *>(c.indices);
  p->num_tiles = blocks;
  return Status::kOk;
}

}  // namespace

// The kernel computes O = S . D over 128-row tiles of the row operand S:
//
//   product  S                  column order  D, its ld        D k-contiguous  O
//   DSD      op(A), sparse      ta            B, ldb           tb              dense C
//   DDS      op(B)^T, sparse    !tb           A, lda           !ta             dense C^T
//   SSD      as DSD                                                            sparse C
//   SDS      as DDS                                                            sparse C^T
//   DSS      op(A), sparse      ta            op(B), sparse: its column lists, dense C
//                                             transposed metadata unless tb
//   SDD      A, dense, lda      -             B, ldb           tb              sparse C
//
// DDS / SDS are DSD / SSD of the transposed problem C^T = op(B)^T op(A)^T;
// everything below the swap is written once, in S / D / i / j terms. A
// sparse S (and DSS's D) read in column order uses the transposed metadata
// (offsets_t, indices_t, block_offsets), exactly like the reference.
Product Bind(const Operand &a, bool ta, const Operand &b, bool tb,
             const Operand &c) {
  Product r;
  GemmParams &p = r.p;
  const bool swap = b.sparse != nullptr && a.sparse == nullptr;
  const Operand &s = swap ? b : a, &d = swap ? a : b;
  // (none or all three sparse: not a product of this library)
  if ((s.sparse != nullptr) == (c.sparse != nullptr) &&
      (d.sparse != nullptr) == (c.sparse != nullptr))
    return r;
  r.s_sparse = s.sparse;
  r.d_sparse = d.sparse;
  r.s_kc = swap ? tb : !ta;
  r.d_kc = swap ? !ta : tb;
  r.out_t = swap;

  // The sparse inputs gate first, and SDD, which has none, on C; SSD / SDS
  // reach the checks of their C last (BindSparseOut).
  const bool c_last = c.sparse != nullptr && s.sparse != nullptr;
  for (const Operand *x : {&a, &b, &c})
    if (x->sparse != nullptr && !(x == &c && c_last) &&
        x->sparse->block_size != BlockSize::k128) {
      r.status = Status::kNotSupported;
      return r;
    }
  if (!OperandOk(a) || !OperandOk(b) || !(c_last || OperandOk(c))) return r;
  if (!ValidMatmul(a, ta, b, tb, c)) return r;
  const MatmulShape shape(a, ta, b, tb);
  if (!Aligned8(shape)) return r;
  // DSS: K <= 32768 (dss_nn:67). The reference's bitmask workspaces are not
  // needed: the intersection is built per tile in LDS.
  if (d.sparse != nullptr && shape.k > kDssMaxK) return r;
  // Tile width of the j extent: one stored block of a sparse operand, else
  // the dense-output tile.
  const int tile =
      c.sparse != nullptr || d.sparse != nullptr ? kBlock : CfgSparse::kBN;
  const long long ld_s = swap ? shape.ldb : shape.lda;
  const long long ld_d = swap ? shape.lda : shape.ldb;
  if (s.sparse == nullptr && !StrideOk(r.s_kc, kBM, ld_s)) return r;
  if (d.sparse == nullptr && !StrideOk(r.d_kc, tile, ld_d)) return r;

  r.s_meta = s.sparse != nullptr && !r.s_kc;
  r.d_meta = d.sparse != nullptr && !r.d_kc;
  r.status = Status::kMissingMetadata;
  if (s.sparse != nullptr &&
      !BindSparse(*s.sparse, r.s_meta, &p.s_offsets, &p.s_indices,
                  &p.s_block_offsets))
    return r;
  if (d.sparse != nullptr &&
      !BindSparse(*d.sparse, r.d_meta, &p.d_offsets, &p.d_indices,
                  &p.d_block_offsets))
    return r;

  p.s_data = static_cast<const char *>(s.data);
  if (s.sparse == nullptr) {
    p.s_ld = ld_s * 2;
    p.k_limit = shape.k;
  }
  p.d_data = static_cast<const char *>(d.data);
  // (a sparse D: inside one stored 128x128 block)
  p.d_ld = d.sparse != nullptr ? kBlock * 2 : ld_d * 2;
  p.num_rows = (swap ? shape.n : shape.m) / kBM;
  p.j_limit = swap ? shape.m : shape.n;
  if (c.sparse != nullptr) {
    r.status = BindSparseOut(*c.sparse, &p);
    return r;
  }
  BindDenseOut(c, shape.ldc, tile, &p);
  // (the stored blocks of S: read by DSD / DDS's 4-wave kernel alone)
  if (d.sparse == nullptr)
    p.s_blocks = (int)(s.sparse->nonzeros / (kBlock * kBlock));
  r.status = Status::kOk;
  return r;
}

}  // namespace sputnik_amd
