// sputnik-amd: FP8 (e4m3) expert products with DeepSeek-style block scales:
// quantisers, an fp8 SDD and an fp8 DSD for the forward pass, and for the
// gradients (below, "Gradients") quantisers along the token dimension, an
// exact transpose of a quantised weight and a DSD whose dense operand is
// scaled per column. The 128 x 128 BCSR block is the scale block of that
// recipe: a weight scale block is a sparse block, an activation scale tile
// is one row of a block, one k-step of the kernel is one scale interval.
// Extensions, all of them: no counterpart in the reference.
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
//   addends and are used only in the opt-in mode below), so |C - exact| <= 2^-p |exact| + (K + 2 K /
//   128) 2^-23 sum |terms| with p = 11 (fp16) or 8 (bf16). No split-K, no
//   atomics, no hand-off between workgroups: the same inputs give the same
//   bits. A stored block whose row or column index is out of range is
//   skipped (SDD: left unwritten; DSD: contributes zero).
//
// Accumulation modes (Fp8Accumulate; the overloads of SddFp8 and DsdFp8 that
// take one, and Fp8IntervalSums). The overloads without it mean kFp32, the
// arithmetic above, bit for bit. Any other value of the enum is
// hipErrorInvalidValue with nothing launched.
//
//   kFast   opt-in: twice the matrix-core rate and no conversion, with an
//           interval sum of limited precision, as DeepSeek-V3's fp8 GEMMs
//           have. Everything outside P is as above: the format and the
//           scales, the interval order (SDD ascending, DSD in storage order),
//           s = float32(sa * sb), one fp32 fma per interval, round_T once,
//           the skipping of out-of-range blocks, no split-K and no atomics,
//           the argument checks. Only P changes. P[i, j] of an interval is
//           what one v_mfma_scale_f32_16x16x128_f8f6f4 of gfx950 returns for
//           the 16 x 16 tile that holds (i, j) when
//             - both operands are e4m3 (cbsz = blgp = 0),
//             - both e8m0 scales are 2^0 (0x7F),
//             - the accumulator input is +0,
//             - lane l (row or column l % 16 of the tile, group g = l / 16)
//               holds in its 32 operand bytes k = 16 g .. 16 g + 15 of the
//               interval followed by k = 64 + 16 g .. 64 + 16 g + 15, in A
//               and in B alike (the kernel's two 16-byte reads),
//           and D[e] of lane l is P[4 g + e, l % 16]. With that assignment
//           the mode is defined bit for bit by the hardware:
//           Fp8IntervalSums(kFast) is that P as a callable, and C =
//           round_T of the fma chain over it. The same inputs give the same
//           bits from run to run, and SDD and DSD give the same bits for the
//           same interval operands in the same order.
//
//           The instruction does not sum in fp32: addends far below the
//           largest product of their group are dropped. The error is
//             |C - exact| <= 2^-p |exact|
//                            + (eps_fast + (2 K / 128 + 1) 2^-23) sum |terms|
//           with eps_fast = 2^-7, measured, not chosen: the worst
//           |P - exact| / sum |products| of Fp8IntervalSums(kFast) against
//           the float64 dot product of the decoded bytes was 2^-8.24, over
//           random finite bytes (2^-12.18), bytes quantised from normal data
//           (2^-12.73), one large product among small ones at every k
//           position and ratio 2^-1 .. 2^-17 (2^-8.28) and two cancelling
//           large products (2^-8.24) (DESIGN 3.6,
//           profiles/fp8/accum_probe.jsonl); eps_fast is the smallest power
//           of two at or above twice that, because a sampled maximum over a
//           sum the hardware does not document is not a proof. The worst
//           case is a product 2^11 times its neighbours: from that ratio on
//           seven of the 127 small addends are dropped, none at 2^10. Data
//           without such outliers inside an interval sees the 2^-12 figures.
//
//           A NaN byte makes NaN exactly the outputs of its row (a byte of A
//           or S) or of its column (a byte of B) in that interval's 128 x
//           128 tile, and makes nothing else NaN.
//
//           Out of scope in this mode: a CPU model of the instruction's
//           internal sum (the tests hold the product to Fp8IntervalSums, and
//           Fp8IntervalSums to float64 within eps_fast), the non-scaled
//           v_mfma_f32_16x16x32_fp8_fp8 form, e8m0 hardware scales carrying
//           real scale values, gradients and other layouts.
//
//   Fp8IntervalSums   P [k / 128, m, n], fp32, of aq [m, k] and bq [n, k]:
//                     P[kb] is the interval sum of k-block kb as the product
//                     kernels form it in the given mode (kFp32: the four
//                     fp16 MFMAs chained from +0 over the byte quarters k =
//                     16 g .., 16 g + 8 .., 64 + 16 g .., 64 + 16 g + 8 .. of
//                     lane group g, in that order). A cold kernel, one wave
//                     per tile and interval; it is what "P" means above.
//                     m, n and k multiples of 128; aq, bq and p non-null,
//                     16-byte aligned, p none of the inputs.
//
// Gradients (extensions like everything here; the table reads X [T, h], W1t
// [F, h], W2 [F, h], topology [T, F], Z = X W1t^T at the blocks, H = act(Z),
// Y = H W2):
//
//   dH  = dY W2^T at the blocks   SddFp8: dY in row tiles (QuantizeRows), W2
//                                 as [n = F, k = h] bytes
//   dZ  = dH * act'(Z)            QuantizeBlocks, stage kActivationGrad
//   dX  = dZ W1t                  DsdFp8: dZ in row tiles, storage order;
//                                 W1t as [n = h, k = F] bytes
//   dW2  = H^T dY   [F, h]        DsdFp8Wgrad: H^T's blocks in the transposed
//   dW1t = dZ^T X   [F, h]        order with one scale per source column
//                                 (QuantizeBlocks' column outputs), dY / X in
//                                 128 x 1 column tiles, stored [h, T]
//                                 (QuantizeTiles' column outputs)
//
//   QuantizeTiles  x [rows, cols] of T, both multiples of 128, read once, one
//                  workgroup per 128 x 128 tile. Row outputs q [rows, cols],
//                  scales [rows, cols / 128]: QuantizeRows' bits. Column
//                  outputs qt [cols, rows] (the bytes of a column contiguous
//                  along the rows) and scales_t [rows / 128, cols]: the tile
//                  of scales_t[rb, c] is x[128 rb : 128 rb + 128, c], scale
//                  and element rules as above. Either pair may be null (both
//                  pointers of it), not both pairs.
//   QuantizeBlocks the block values [nnz_blocks, 128, 128] of s (s.data, T)
//                  after a stage: kNone; kActivation, act(x) as
//                  QuantizeRowsActivation evaluates it; kActivationGrad, x *
//                  act'(z) as MatmulActivationGrad's elementwise stage
//                  evaluates it (z: block values of the same layout), rounded
//                  to T before it is quantised. Row outputs q [nnz_blocks,
//                  128, 128], scales [nnz_blocks 128], in storage order:
//                  the row quantisers' bits on the same values. Column
//                  outputs in the transposed order: output block j is source
//                  block s.block_offsets[j] stored transposed ([column][row])
//                  with scales_t[128 j + c] for source column c. They are
//                  the Sq / s_scales of a DSD over the descriptor {rows =
//                  s.cols, cols = s.rows, offsets = s.offsets_t, indices =
//                  s.indices_t}. Column outputs need s.block_offsets
//                  (Transpose), hipErrorInvalidValue without; an entry
//                  outside [0, nnz_blocks) leaves its output block unwritten.
//                  The workgroup of output block j also writes the row
//                  outputs of its source block when both pairs are asked
//                  for, so block_offsets is then a permutation, as Transpose
//                  leaves it. Only s.data, s.nonzeros, s.block_size and
//                  s.block_offsets are read.
//   TransposeWeightFp8
//                  q [n, k] with scales [k / 128, n / 128] -> qt [k, n] with
//                  scales_t [n / 128, k / 128]: a byte transpose, exact. A
//                  block's scale depends on the block's amax alone, so the
//                  result is QuantizeWeight of the transposed 16-bit weight,
//                  bit for bit: the backward layout of a weight that exists
//                  only as fp8.
//   DsdFp8Wgrad    C [m, n] = Sq . Bq as DsdFp8, with b_scales [k / 128, n]:
//                  one scale per interval and output column, as
//                  QuantizeTiles' scales_t. Per interval, in the row's
//                  storage order, s = float32(sa[row] * sb[kb, col]) and acc
//                  = fma(s, P, acc); P as the mode defines it above, kFp32
//                  and kFast alike. C = round_out(acc), or with `add`
//                  round_out(acc + float(C_old)): one fp32 add, one rounding.
//                  `out` (accumulate.h) is kOperand, C of T, or kF32, C of
//                  fp32. A block row of s without stored blocks gives +0
//                  rows, and with `add` is neither read nor written, as
//                  MatmulAccumulate has it. No split-K, no atomics, no
//                  hand-off between workgroups: the same inputs give the
//                  same bits. Out-of-range indices, alignment (Sq, Bq and C
//                  16 bytes), checks and zero-sized work as DsdFp8; C being
//                  any input is rejected. Error, in the form above:
//                    |C - exact| <= 2^-p |exact|
//                                   + (K + 2 K / 128 + 1) 2^-23 sum |terms|
//                  (kFast: eps_fast + (2 K / 128 + 2) 2^-23 in place of the
//                  last factor): the scale product is still one rounding per
//                  interval and the fma another; the + 1 is the fp32 add of
//                  C_old, which with `add` is one of the terms, of exact and
//                  of sum |terms| alike. p = 11 (fp16) or 8 (bf16); the
//                  first summand is absent for fp32 output, which is not
//                  rounded again.
//
// `dtype` is T, the 16-bit type (DataType keeps its two values). Every call
// is stream-ordered, allocates nothing and never synchronises or aborts:
// hipErrorInvalidValue, with nothing launched, for a null required buffer, a
// negative size, a dimension that is not a multiple of 128, a block size
// other than 128, or an output that is one of the inputs; SddFp8 and DsdFp8
// also for an Aq / Sq / Bq / C that is not 16-byte aligned (the quantisers
// take any alignment). Zero-sized work succeeds.
//
// Out of scope: GLU gradients in fp8 (the kOutGateGrad stage makes them a
// follow-up with the same kernels), e5m2 (gradients included), other operand
// layouts (weights are re-laid once by QuantizeWeight and
// TransposeWeightFp8), DDS / SSD / SDS / DSS in fp8, e8m0 hardware scales,
// fp8 outputs from the GEMM epilogue, caching quantised weights across
// micro-batches, biases and the router.
#ifndef SPUTNIK_BLOCK_FP8_H_
#define SPUTNIK_BLOCK_FP8_H_

#include "sputnik/block/accumulate.h"
#include "sputnik/block/activation.h"
#include "sputnik/block/arguments.h"
#include "sputnik/block/dtype.h"

namespace sputnik {
namespace block {

// How an interval's P is summed (above): kFp32, the default, or the opt-in
// kFast.
enum class Fp8Accumulate { kFp32 = 0, kFast = 1 };

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

// The same with the accumulation mode of P (above).
hipError_t SddFp8(const void *aq, const float *a_scales, int k,
                  const void *bq, const float *b_scales, BlockMatrix c,
                  DataType dtype, Fp8Accumulate accumulate,
                  hipStream_t stream);

hipError_t DsdFp8(const BlockMatrix s, const float *s_scales, const void *bq,
                  const float *b_scales, Matrix c, DataType dtype,
                  Fp8Accumulate accumulate, hipStream_t stream);

hipError_t Fp8IntervalSums(const void *aq, const void *bq, int m, int n,
                           int k, Fp8Accumulate accumulate, float *p,
                           hipStream_t stream);

// ---- Gradients (above). Extensions: no counterpart in the reference. ----

// What QuantizeBlocks applies to the block values before it quantises them.
enum class Fp8Stage { kNone = 0, kActivation = 1, kActivationGrad = 2 };

hipError_t QuantizeTiles(const void *x, int rows, int cols, void *q,
                         float *scales, void *qt, float *scales_t, bool pow2,
                         DataType dtype, hipStream_t stream);

// `activation` is read when `stage` is not kNone, `z` when it is
// kActivationGrad.
hipError_t QuantizeBlocks(const BlockMatrix s, Fp8Stage stage,
                          Activation activation, const void *z, void *q,
                          float *scales, void *qt, float *scales_t, bool pow2,
                          DataType dtype, hipStream_t stream);

hipError_t TransposeWeightFp8(const void *q, const float *scales, int k,
                              int n, void *qt, float *scales_t,
                              hipStream_t stream);

hipError_t DsdFp8Wgrad(const BlockMatrix s, const float *s_scales,
                       const void *bq, const float *b_scales, Matrix c,
                       DataType dtype, OutputType out, bool add,
                       Fp8Accumulate accumulate, hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_FP8_H_
