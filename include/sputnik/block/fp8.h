// sputnik-amd: FP8 (e4m3) expert products with DeepSeek-style block scales,
// forward only: quantisers, an fp8 SDD and an fp8 DSD. The 128 x 128 BCSR
// block is the scale block of that recipe: a weight scale block is a sparse
// block, an activation scale tile is one row of a block, one k-step of the
// kernel is one scale interval. No counterpart in the reference.
//
// Format (part of the contract):
//
//   Elements  OCP e4m3fn, one byte each, as torch.float8_e4m3fn stores them:
//             1 sign, 4 exponent (bias 7), 3 mantissa bits; largest finite
//             value 448; 0x7F and 0xFF are NaN; no infinities. Not the fnuz
//             form.
//   Scales    fp32, multiplied at dequantisation: value = float(q) * scale.
//
//   Scale of a tile (1 x 128 of a row, or a 128 x 128 weight block): with
//   amax the largest |x| over the tile's finite elements (0 if it has none),
//     default   scale = max(amax / 448.0f, 2^-126), an IEEE fp32 division;
//     pow2      the smallest power of two s >= 2^-126 with amax / s <= 448:
//               from amax = m 2^e, m in [0.5, 1): s = 2^(e-9) if m <= 0.875,
//               otherwise 2^(e-8). Dequantisation is then exact.
//   Element   q = rne_e4m3(float(x) / scale), an IEEE fp32 division (no
//             reciprocal approximation: the bytes are defined). A NaN or
//             +-Inf element becomes the e4m3 NaN with its sign (0x7F / 0xFF).
//             |x / scale| never passes 448 by more than an fp32 rounding, far
//             below the overflow edge at 464, so no saturation is involved;
//             the 2^-126 floor is what keeps a tile whose amax / 448 is
//             subnormal from overflowing.
//
//   QuantizeRows   x [rows, cols] of T -> q [rows, cols] bytes and scales
//                  [rows, cols / 128] (row tiles). One pass.
//   QuantizeRowsActivation
//                  the same of H = act(x), evaluated as MatmulActivation's
//                  elementwise stage evaluates it (H = round_T(act(float(x)))),
//                  so q is the quantisation of the H the 16-bit path stores.
//   QuantizeRowsGated
//                  the same of H = x * act(gate), as MatmulGated's stage.
//                  The H is never written: the hidden matrix goes from the
//                  16-bit SDD output straight to fp8.
//                  A BCSR matrix's block values [nnz_blocks, 128, 128] are
//                  quantised by these calls as the matrix [nnz_blocks 128,
//                  128]: one scale per row of each stored block, in storage
//                  order.
//   QuantizeWeight w [k, n] of T (transpose: the buffer holds w^T, [n, k])
//                  -> q stored k-contiguous as [n, k] and scales [k / 128,
//                  n / 128], one per 128 x 128 block. Tensors a checkpoint
//                  already holds in this layout are used as they are.
//
//   SddFp8   C (BCSR, T) = Aq [m, k] . Bq at C's stored blocks (c.row_indices
//            and c.indices as the SDD Matmul): a_scales [m, k / 128], Bq
//            [n, k] with b_scales [k / 128, n / 128] as QuantizeWeight
//            leaves them; m = c.rows, n = c.cols.
//   DsdFp8   C [m, n] (T) = Sq (BCSR, bytes in s.data) . Bq: s_scales
//            [nnz_blocks 128] as the quantisers leave them, k = s.cols. A
//            block row without stored blocks gives +0 rows; column indices
//            need not be ordered.
//
//   Arithmetic of both: per scale interval (a k-block kb; SDD ascending, DSD
//   in the row's storage order) P is the fp32 MFMA sum, from zero, of the 128
//   e4m3 products, and acc = fma(sa[row, kb] * sb[kb, nb], P, acc) in fp32:
//   the scale product rounded, the multiply-add rounded once. C =
//   round_T(acc), rounded once. Every product and every partial sum of P is
//   held to fp32 precision (the operands are widened to fp16, exactly, in
//   front of the matrix cores; the fp8 MFMA forms of gfx950 drop small
//   addends and are not used), so |C - exact| <= 2^-p |exact| + (K + 2 K /
//   128) 2^-23 sum |terms| with p = 11 (fp16) or 8 (bf16). No split-K, no
//   atomics, no hand-off between workgroups: the same inputs give the same
//   bits. A stored block whose row or column index is out of range is
//   skipped (SDD: left unwritten; DSD: contributes zero).
//
// `dtype` is T, the 16-bit type (DataType keeps its two values). Every call
// is stream-ordered, allocates nothing and never synchronises or aborts:
// hipErrorInvalidValue, with nothing launched, for a null required buffer, a
// negative size, a dimension that is not a multiple of 128, a block size
// other than 128, or an output that is one of the inputs; SddFp8 and DsdFp8
// also for an Aq / Sq / Bq / C that is not 16-byte aligned (the quantisers
// take any alignment). Zero-sized work succeeds.
//
// Out of scope: gradients, e5m2, other operand layouts (weights are re-laid
// once by QuantizeWeight), DDS / SSD / SDS / DSS in fp8, e8m0 hardware
// scales, fp8 outputs from the GEMM epilogue.
#ifndef SPUTNIK_BLOCK_FP8_H_
#define SPUTNIK_BLOCK_FP8_H_

#include "sputnik/block/activation.h"
#include "sputnik/block/arguments.h"
#include "sputnik/block/dtype.h"

namespace sputnik {
namespace block {

hipError_t QuantizeRows(const void *x, int rows, int cols, void *q,
                        float *scales, bool pow2, DataType dtype,
                        hipStream_t stream);

hipError_t QuantizeRowsActivation(const void *x, int rows, int cols,
                                  Activation activation, void *q,
                                  float *scales, bool pow2, DataType dtype,
                                  hipStream_t stream);

hipError_t QuantizeRowsGated(const void *x, const void *gate, int rows,
                             int cols, Activation activation, void *q,
                             float *scales, bool pow2, DataType dtype,
                             hipStream_t stream);

hipError_t QuantizeWeight(const void *w, int k, int n, bool transpose,
                          void *q, float *scales, bool pow2, DataType dtype,
                          hipStream_t stream);

hipError_t SddFp8(const void *aq, const float *a_scales, int k,
                  const void *bq, const float *b_scales, BlockMatrix c,
                  DataType dtype, hipStream_t stream);

hipError_t DsdFp8(const BlockMatrix s, const float *s_scales, const void *bq,
                  const float *b_scales, Matrix c, DataType dtype,
                  hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_FP8_H_
