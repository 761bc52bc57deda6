// sputnik-amd: OCP Microscaling (MX) expert products: MXFP8 (e4m3)
// activations against MXFP8 (e4m3) or MXFP4 (e2m1) weights, with the e8m0
// block scales applied by the matrix instruction itself. Quantisers, an SDD
// and a DSD for the forward pass; for the gradients (below, "Gradients")
// quantisers along the token dimension and a DSD into gradient sinks, MXFP8
// throughout. Extensions, all of them: no counterpart in the reference.
//
// Format (part of the contract, bit for bit):
//
//   Elements  MxFormat::kE4M3  OCP e4m3fn, one byte each, exactly as fp8.h has
//                              it (0x7F / 0xFF are NaN, no infinities).
//             MxFormat::kE2M1  4 bits: 1 sign, 2 exponent, 1 mantissa. Code c
//                              & 7 stands for {0, 0.5, 1, 1.5, 2, 3, 4, 6}[c &
//                              7], bit 3 is the sign. No NaN, no Inf. Two per
//                              byte: element 2 i in bits 3:0, element 2 i + 1
//                              in bits 7:4, as torch.float4_e2m1fn_x2 and the
//                              published MXFP4 checkpoints store them.
//   Scales    one e8m0 byte per 32 consecutive k-elements of a row: value =
//             2^(byte - 127); 0xFF is NaN. Activations [rows, k] have scales
//             uint8 [rows, k / 32]. Weights are stored k-contiguous, [n, k]
//             bytes (e2m1: [n, k / 2]), with scales uint8 [n, k / 32];
//             checkpoint tensors in this layout are used as they are.
//
//   Scale of a 32-block: fp8.h's pow2 rule, without saturation, one rule per
//   element type. With amax the largest finite |x| of the 32 elements, amax =
//   m 2^e, m in [0.5, 1):
//     e4m3   s = 2^(e-9) if m <= 0.875, otherwise 2^(e-8)   (amax / s <= 448)
//     e2m1   s = 2^(e-3) if m <= 0.75,  otherwise 2^(e-2)   (amax / s <= 6)
//   both floored at 2^-126 (byte 0x01), which also covers amax = 0.
//   Element  q = rne(x / s), ties to even; the division is exact.
//   Non-finite elements
//     e4m3   the element becomes the NaN byte with its sign and is left out
//            of amax, as QuantizeRows has it.
//     e2m1   the block's scale byte becomes 0xFF and its elements code 0.
//
//   QuantizeRowsMx   x [rows, cols] of T, cols a multiple of 128 -> q [rows,
//                    cols] e4m3 bytes and scales uint8 [rows, cols / 32].
//                    `stage`: kNone; kActivation, H = act(x) evaluated as
//                    QuantizeRowsActivation evaluates it; kGated, H = x *
//                    act(gate) as QuantizeRowsGated. Block values [nnz_blocks,
//                    128, 128] go in as [nnz_blocks 128, 128]: one scale dword
//                    per stored-block row, in storage order. `gate` is read
//                    for kGated, `activation` unless kNone.
//   QuantizeWeightMx w [k, n] of T (transpose: the buffer holds w^T, [n, k])
//                    -> q [n, k] bytes (kE2M1: [n, k / 2]) and scales uint8
//                    [n, k / 32]. k and n multiples of 128.
//   SddMx   C (BCSR, T) = Aq [m, k] . Bq at C's stored blocks, a_scales [m,
//           k / 32], Bq / b_scales as QuantizeWeightMx leaves them in
//           `b_format`; m = c.rows, n = c.cols.
//   DsdMx   C [m, n] (T) = Sq (BCSR, e4m3 bytes in s.data) . Bq: s_scales
//           [nnz_blocks 128, 4] as QuantizeRowsMx leaves them, k = s.cols.
//   A / S is e4m3 in these two ("MXFP4 activations", below, has the e2m1 A /
//   S). Shapes, index checks, the skipping of out-of-range
//   blocks, +0 rows for empty block rows and alias rejection follow SddFp8 /
//   DsdFp8; Aq / Sq / Bq / C are 16-byte and the scale arrays 4-byte aligned
//   (a step's four scale bytes of a row are fetched as one dword).
//
//   Arithmetic of both: a step is one k-block of 128 (SDD ascending, DSD in
//   the row's storage order). P is what one
//   v_mfma_scale_f32_16x16x128_f8f6f4 returns from a +0 accumulator for the
//   16 x 16 tile when lane l (row / column l % 16, group g = l / 16) passes
//   the e8m0 byte of 32-block g of its row (A) or column (B) and
//     an e4m3 operand (8 registers) as k = 16 g .. 16 g + 15 of the step in
//       registers 0 - 3 and k = 64 + 16 g .. 64 + 16 g + 15 in registers 4 -
//       7, bytes in memory order;
//     an e2m1 operand (4 registers) as k = 32 g .. 32 g + 31, nibbles in
//       memory order, low first;
//   D[e] of lane l is P[4 g + e, l % 16]. That is the instruction's map as
//   measured on the hardware with one-hot rows and a scale ramp: element k
//   meets element k and the scale byte of block k / 32. (A lane that holds 32
//   contiguous e4m3 bytes instead gets half of each block multiplied by a
//   neighbour's scale.) The known-answer tests (tests/test_gpu_mx.py) hold
//   the kernels to it: scales that differ per (row, 32-block) and per (column,
//   32-block), one-hot rows per 32-block and per nibble. acc = acc + P is one
//   fp32 add per step, C = round_T(acc), rounded once. No split-K, no atomics,
//   no hand-off: the same inputs give the same bits, and SDD and DSD give the
//   same bits for the same step operands in the same order. P starts from +0
//   on purpose: what the instruction does with a large accumulator input has
//   not been measured, so the accumulator is not chained through the MFMA.
//
//   Error: |C - exact| <= 2^-p |exact| + (eps_fast + (K / 128 + 1) 2^-23)
//   sum |terms|, eps_fast = 2^-7 as fp8.h has it, p = 11 (fp16) or 8 (bf16).
//   e8m0 scaling is exact, so a step is the instruction fp8.h characterised
//   with products that span a wider ratio (profiles/fp8/accum_probe.jsonl,
//   family (c), covers ratios out to 2^-17). Measured on SddMx with fp16
//   output, the rounding to fp16 (up to 2^-12 |exact|) included, both weight
//   formats (scripts/probe_mx_accum.py, profiles/mx/accum_probe.jsonl):
//   worst |C - exact| / sum |terms| 2^-11.6 on bytes quantised from normal
//   data with block scales over 16 binades (K = 640), 2^-10.9 on uniformly
//   random finite bytes under scales over 8 binades, and 2^-11.1 on one
//   product 2^11 .. 2^17 above its 127 neighbours with the gap split between
//   its element and its block's scale (2^-11.1 at 2^11, halving with every
//   doubling of the gap: the output rounding alone; with part of the gap in
//   the scale no neighbour was lost). No family passes 2^-8, so eps_mx =
//   eps_fast = 2^-7 stands: an outlier inside one 32-block, all of its gap
//   in the elements, is fp8.h's own worst case (2^-8.28). The tests assert
//   eps_fast / 2 = 2^-8 on their data.
//
//   A NaN byte of A / S makes NaN exactly its row of that step's tile, a 0xFF
//   scale byte of B exactly its column (the OCP rule).
//
// Gradients (e4m3 throughout; the table reads X [T, h], W1t [F, h], W2 [F,
// h], topology [T, F], Z = X W1t^T at the blocks, H = act(Z), Y = H W2). MX
// scales belong to one operand and run along k, so every product is SddMx /
// DsdMx's step with operands that arrive contiguous along its own k:
//
//   dH  = dY W2^T at the blocks   SddMx: dY [T, k = h] (QuantizeTilesMx' row
//                                 outputs), W2 as [n = F, k = h] bytes
//                                 (QuantizeWeightMx(w2, transpose))
//   dZ  = dH * act'(Z)            QuantizeBlocksMx, stage kActivationGrad
//   dX  = dZ W1t                  DsdMx: dZ's row outputs, storage order; W1t
//                                 as [n = h, k = F] bytes (QuantizeWeightMx(
//                                 w1t), from the buffer read as [k = F, n = h])
//   dW2  = H^T dY   [F, h]        DsdMxWgrad: H^T's / dZ^T's blocks in the
//   dW1t = dZ^T X   [F, h]        transposed order, scaled along the tokens
//                                 (QuantizeBlocksMx' column outputs; H from
//                                 stage kActivation of Z), dY / X as [n = h,
//                                 k = T] with one byte per column and 32
//                                 tokens (QuantizeTilesMx' column outputs)
//
//   An MX weight cannot be transposed exactly (its scale groups are 1 x 32,
//   not square), so the backward layouts of the weights are quantised from
//   the 16-bit master weights by QuantizeWeightMx.
//
//   QuantizeTilesMx  x [rows, cols] of T, both multiples of 128, read once,
//                    one workgroup per 128 x 128 tile. Row outputs q [rows,
//                    cols], scales [rows, cols / 32]: QuantizeRowsMx(kNone)'s
//                    bits. Column outputs qt [cols, rows] (the bytes of a
//                    column contiguous along the rows) and scales_t [cols,
//                    rows / 32]: the group of scales_t[c, g] is x[32 g : 32 g
//                    + 32, c], scale, element and non-finite rules as above
//                    for e4m3. qt / scales_t are a Bq [n = cols, k = rows] /
//                    b_scales of SddMx / DsdMx / DsdMxWgrad as they stand.
//                    Either pair may be null (both pointers of it), not both
//                    pairs.
//   QuantizeBlocksMx the block values [nnz_blocks, 128, 128] of s (s.data, T)
//                    after a stage: kNone; kActivation, act(x) as
//                    QuantizeRowsMx(kActivation) evaluates it;
//                    kActivationGrad, x * act'(z) as MatmulActivationGrad's
//                    elementwise stage evaluates it (z: block values of the
//                    same layout), rounded to T before it is quantised. Row
//                    outputs q [nnz_blocks, 128, 128], scales [nnz_blocks 128,
//                    4], in storage order: QuantizeRowsMx's bits on the same
//                    values, the Sq / s_scales of DsdMx. Column outputs in the
//                    transposed order: output block j is source block
//                    s.block_offsets[j] stored transposed ([column][row]),
//                    scales_t[128 j + c] the dword of the four 32-row groups
//                    of source column c. They are the Sq / s_scales of a DSD
//                    over the descriptor {rows = s.cols, cols = s.rows,
//                    offsets = s.offsets_t, indices = s.indices_t}. Column
//                    outputs need s.block_offsets (Transpose),
//                    hipErrorInvalidValue without; an entry outside [0,
//                    nnz_blocks) leaves its output block unwritten. The
//                    workgroup of output block j also writes the row outputs
//                    of its source block when both pairs are asked for, so
//                    block_offsets is then a permutation, as Transpose leaves
//                    it. Only s.data, s.nonzeros, s.block_size and
//                    s.block_offsets are read.
//   DsdMxWgrad       C [m, n] = Sq . Bq as DsdMx with an e4m3 B: the steps in
//                    the row's storage order, the k map, the +0 accumulator
//                    input and the one fp32 add per step are DsdMx's. C =
//                    round_out(acc), or with `add` round_out(acc +
//                    float(C_old)): one fp32 add, one rounding. `out`
//                    (accumulate.h) is kOperand, C of T, or kF32, C of fp32.
//                    With kOperand and no `add` the bits are DsdMx's. A block
//                    row of s without stored blocks gives +0 rows, and with
//                    `add` is neither read nor written, as MatmulAccumulate
//                    has it. No split-K, no atomics, no hand-off: the same
//                    inputs give the same bits. Out-of-range indices,
//                    alignment (Sq, Bq and C 16 bytes, scales 4), checks and
//                    zero-sized work as DsdMx; C being any input is rejected.
//                    Error, K the tokens of the row (128 per stored block):
//                      |C - exact| <= 2^-p |exact|
//                          + (eps_fast + (K / 128 + 1 + add) 2^-23) sum |terms|
//                    the + add is the fp32 add of C_old, which with `add` is
//                    one of the terms, of exact and of sum |terms| alike; the
//                    first summand is absent for fp32 output, which is not
//                    rounded again.
//
// Gradients of a gated expert (GLU: V1t [F, h] beside W1t, G = X W1t^T and
// U = X V1t^T at the blocks, H = U * act(G), Y = H W2; e4m3 throughout, the
// weights' backward layouts quantised from 16 bits as above):
//
//   dW2  = H^T dY                 H from the kept G and U:
//                                 QuantizeBlocksMxGated (column outputs) ->
//                                 DsdMxWgrad
//   D    = dY W2^T at the blocks  SddMx, as dH above
//   dG   = D * U * act'(G)        QuantizeBlocksMxGatedGrad: one read of D, G
//   dU   = D * act(G)             and U, row and column images of both,
//                                 neither stored as 16 bits
//   dX   = dG W1t + dU V1t        DsdMxPair: one accumulator, one rounding;
//                                 W1t and V1t as [n = h, k = F] bytes
//   dW1t = dG^T X, dV1t = dU^T X  DsdMxWgrad on the column images, X's
//                                 column outputs from forward
//
//   MxImages       the outputs of a block quantiser, {q, scales, qt,
//                  scales_t} with QuantizeBlocksMx' meaning and sizes: the row
//                  pair in storage order, the column pair in the transposed
//                  order. Either pair may be null (both pointers of it).
//   QuantizeBlocksMxGated
//                  the block values of H = x * act(gate), x = s.data, as
//                  QuantizeRowsMx(kGated) evaluates it: QuantizeBlocksMx with
//                  the forward gate as its stage, and its rules
//                  (block_offsets for the column pair, out-of-range entries,
//                  the row outputs written by the workgroup of the output
//                  block, either pair null but not both). MxBlockStage keeps
//                  its three values: the gated stages have entry points of
//                  their own.
//   QuantizeBlocksMxGatedGrad
//                  (dG, dU) of the block values D = d.data, `gate` = G and
//                  `up` = U (the same layout), exactly what MatmulGatedGrad's
//                  elementwise stage stores for them (BlockGateGrad), rounded
//                  to T, then quantised: every output is bit for bit
//                  QuantizeBlocksMx(kNone) of that 16-bit tensor, which is
//                  never written. `dg` and `du` are two MxImages; any of the
//                  four pairs may be null, all four null is
//                  hipErrorInvalidValue. A column pair needs
//                  d.block_offsets; with a row pair beside it block_offsets
//                  is a permutation. One workgroup per block, each input tile
//                  read once; a null pair costs neither its stores nor its
//                  LDS traffic. No output may be an input or another output.
//   DsdMxPair      C [m, n] (T) = S1q . B1q + S2q . B2q. S1 and S2 share one
//                  topology: s1 carries the offsets, the indices and the
//                  first pair's bytes, s2_data / s2_scales the second pair's
//                  in the same storage order; B1q and B2q are two e4m3 [n, k]
//                  weights with [n, k / 32] scales. The steps of a block row
//                  are pair 1's stored blocks in storage order, then pair
//                  2's in storage order; each is DsdMx's step (the k map, the
//                  +0 accumulator input, one fp32 add); C = round_T(acc),
//                  rounded once. So the result is, bit for bit, DsdMx over
//                  the concatenated operands [S1 | S2] . [B1; B2], with no
//                  concatenated copy of anything. Empty block rows give +0
//                  rows; an out-of-range index contributes zero in both
//                  pairs; no split-K, no atomics; alignment and alias checks
//                  are DsdMx's over both pairs. Error: DsdMx's with 2 K in
//                  place of K,
//                    |C - exact| <= 2^-p |exact|
//                        + (eps_fast + (2 K / 128 + 1) 2^-23) sum |terms|
//
// Fused gated SDD (forward of a GLU expert, either weight format):
//
//   SddMxGated   both products of SddMx at c's stored blocks from one read of
//                Aq, then the gate stage and QuantizeRowsMx, in one kernel:
//                acc_g = Aq . gate^T and acc_u = Aq . up^T, each SddMx's
//                arithmetic (the step, the +0 accumulator input, one fp32 add
//                per step, k ascending). `gate_q` / `up_q` and their scales
//                are two weights of `b_format` with n = c.cols logical rows;
//                logical row n is physical row b_row_step n of its pointer,
//                bytes and scales alike, b_row_step 1 or 2. Two separate
//                weights: step 1. One tensor [2 n, k] with rows 2 f = gate
//                and 2 f + 1 = up: gate = base, up = base + one row (k or k /
//                2 bytes; k / 32 scale bytes), step 2; nothing is copied.
//                `c` is the topology only (c.data is not read or written).
//                Per element, fp32 with no contraction:
//                  G = round_T((float(round_T(acc_g)) + float(gate_bias[col]))
//                      + 0.0f), U likewise with up_bias: bias.h's rule; a null
//                      bias skips the add, G = round_T(acc_g), SddMx's bits.
//                  kPlain          H = round_T(float(U) act(float(G)) + 0.0f),
//                                  MatmulGated's stage.
//                  kClampedSwiglu  Gc = G > limit ? limit : G
//                                  Uc = U > limit ? limit
//                                       : (U < -limit ? -limit : U)
//                                  s  = 1 / (1 + exp(-t)), t = alpha Gc held
//                                       to [-100, 100], the sigmoid as silu
//                                       evaluates it
//                                  H  = round_T((Uc + 1.0f) (Gc s) + 0.0f)
//                                  (a NaN in G or U passes through the
//                                  comparisons and makes H NaN; `activation`
//                                  is checked, not used).
//                hq [nnz_blocks, 128, 128] e4m3 and h_scales [nnz_blocks 128,
//                4] are QuantizeRowsMx(kNone) of H's block values, bit for
//                bit, the Sq / s_scales of DsdMx. keep.g / keep.u / keep.h,
//                each null or block values of T: G, U and H as above. With no
//                bias and kPlain, hq / h_scales / keep.g / keep.u are bit for
//                bit SddMx, SddMx, QuantizeRowsMx(kGated). No split-K, no
//                atomics: the same inputs give the same bits. An out-of-range
//                index leaves its block of every output unwritten. Error of G
//                and U before the bias: SddMx's. Besides SddMx's checks,
//                hipErrorInvalidValue for b_row_step outside {1, 2}, a kind or
//                activation outside its enum, limit not > 0 or alpha not
//                finite (kClampedSwiglu), a null hq / h_scales, misalignment
//                (Aq, the weights, hq and keep.* 16 bytes, scales 4, biases
//                2), or an output that is an input or another output.
//
// MXFP4 activations (A4W4: both operands e2m1, the form of the instruction
// with half the passes of any form that has an fp8 operand; forward only):
//
//   QuantizeRowsMxFp4  QuantizeRowsMx with e2m1 elements: x [rows, cols] of T,
//                cols a multiple of 128 -> q [rows, cols / 2] bytes, two codes
//                per byte, low nibble first, and scales uint8 [rows, cols /
//                32]. Scale, element and non-finite rules are the e2m1 rules
//                above (QuantizeWeightMx's): a non-finite element turns its
//                block's scale byte into 0xFF and the block's codes into 0.
//                The stages evaluate H exactly as QuantizeRowsMx does, rounded
//                to T before it is quantised. Block values go in as
//                [nnz_blocks 128, 128]: q [nnz_blocks, 128, 64] and one scale
//                dword per stored-block row. Any alignment.
//   SddMxFp4     SddMx with Aq [m, k / 2] e2m1 bytes.
//   DsdMxFp4     DsdMx with s.data [nnz_blocks, 128, 64] e2m1 bytes, s_scales
//                [nnz_blocks 128, 4] (s.nonzeros still counts elements: 128 x
//                128 per stored block).
//   B is always an e2m1 weight, as QuantizeWeightMx(kE2M1) or a checkpoint
//   leaves it; there is no e2m1 A against an e4m3 B. The arithmetic is the one
//   above, unchanged: per k-block of 128, P is the instruction's result from
//   a +0 accumulator (cbsz 4, blgp 4), lane (r, g) passing k = 32 g .. 32 g +
//   31 of its row / column in registers 0 - 3 and scale byte g, for both
//   operands; acc = acc + P, one fp32 add per k-block in k order (SDD) or the
//   row's storage order (DSD); C = round_T(acc), rounded once. No split-K, no
//   atomics: the same inputs give the same bits, and SDD on a full topology
//   and DSD over the same bytes give the same bits. A 0xFF scale byte of A /
//   S makes NaN exactly its row of the step's tile, one of B exactly its
//   column. Shape and index checks, the skipping of out-of-range blocks, +0
//   rows for empty block rows, alias rejection and the alignments (operands
//   and C 16 bytes, scales 4) are SddMx / DsdMx's.
//   Error: the bound above with eps_fast. Every e2m1 value is an e4m3 value
//   and the scales are the same e8m0, so the characterised families cover
//   these operands, provided the fp4 form of the instruction sums as the fp8
//   form does. Measured on SddMxFp4 / DsdMxFp4 (tests/test_gpu_mx_fp4.py, K =
//   640, bytes quantised from normal data with block scales over 16 binades,
//   the rounding to T beyond 2^-p |exact| left out): worst |C - exact| / sum
//   |terms| 0 for SDD (fp16 and bf16) and for DSD in bf16 (an earlier draw of
//   the same family gave 2^-26.2 and 2^-29.5), and 2^-9.9 for DSD in fp16,
//   which is no accumulation error: block rows with one or two stored blocks
//   under small scales give results in fp16's subnormal range, and round_fp16
//   of the exact result alone gives the same 2^-9.90 on the host. An e2m1 x
//   e2m1 product has two significant bits, and the fp4 form lost nothing
//   measurable beside what fp32 adds lose: it sums no worse than the fp8 form.
//   The tests assert eps_fast / 2 = 2^-8 on their data.
//
// `dtype` is T, the 16-bit type. Every call is stream-ordered, allocates
// nothing and never synchronises or aborts: hipErrorInvalidValue, with nothing
// launched, for a null required buffer, a negative size, a dimension that is
// not a multiple of 128, a block size other than 128, an MxFormat / MxStage /
// MxBlockStage / OutputType / Activation outside its enum, a misaligned
// buffer (above; the quantisers take any alignment) or an output that is one
// of the inputs. Zero-sized work succeeds.
//
// Out of scope: the backward of MXFP4 weights; folding the gated gradient
// into SddMx's epilogue, so that D is never written; e5m2, e3m2 and e2m3
// elements; the backward pass with e2m1 operands; an e2m1-A variant of
// SddMxGated; biases on the MXFP4-activation path; DDS / SSD / SDS / DSS;
// chaining the accumulator through the MFMA; a CPU model of the instruction's
// internal sum; caching the weights' backward layouts across micro-batches;
// biases outside SddMxGated (the training path, SddMx, DsdMx); a C++ example.
#ifndef SPUTNIK_BLOCK_MX_H_
#define SPUTNIK_BLOCK_MX_H_

#include <cstdint>

#include "sputnik/block/accumulate.h"
#include "sputnik/block/activation.h"
#include "sputnik/block/arguments.h"
#include "sputnik/block/dtype.h"

namespace sputnik {
namespace block {

enum class MxFormat { kE4M3 = 0, kE2M1 = 1 };

// What QuantizeRowsMx applies to x before it quantises.
enum class MxStage { kNone = 0, kActivation = 1, kGated = 2 };

hipError_t QuantizeRowsMx(const void *x, const void *gate, int rows, int cols,
                          MxStage stage, Activation activation, void *q,
                          uint8_t *scales, DataType dtype, hipStream_t stream);

hipError_t QuantizeWeightMx(const void *w, int k, int n, bool transpose,
                            MxFormat format, void *q, uint8_t *scales,
                            DataType dtype, hipStream_t stream);

hipError_t SddMx(const void *aq, const uint8_t *a_scales, int k,
                 const void *bq, const uint8_t *b_scales, MxFormat b_format,
                 BlockMatrix c, DataType dtype, hipStream_t stream);

hipError_t DsdMx(const BlockMatrix s, const uint8_t *s_scales, const void *bq,
                 const uint8_t *b_scales, MxFormat b_format, Matrix c,
                 DataType dtype, hipStream_t stream);

// ---- MXFP4 activations (above). ----

hipError_t QuantizeRowsMxFp4(const void *x, const void *gate, int rows,
                             int cols, MxStage stage, Activation activation,
                             void *q, uint8_t *scales, DataType dtype,
                             hipStream_t stream);

hipError_t SddMxFp4(const void *aq, const uint8_t *a_scales, int k,
                    const void *bq, const uint8_t *b_scales, BlockMatrix c,
                    DataType dtype, hipStream_t stream);

hipError_t DsdMxFp4(const BlockMatrix s, const uint8_t *s_scales,
                    const void *bq, const uint8_t *b_scales, Matrix c,
                    DataType dtype, hipStream_t stream);

// ---- Fused gated SDD (above). ----

enum class MxGluKind { kPlain = 0, kClampedSwiglu = 1 };

// `activation` is kPlain's; `alpha` and `limit` are kClampedSwiglu's.
struct MxGlu {
  MxGluKind kind;
  Activation activation;
  float alpha;
  float limit;
};

// Block values of T to keep beside the MXFP8 image; each may be null.
struct MxGluKeep {
  void *g;
  void *u;
  void *h;
};

hipError_t SddMxGated(const void *aq, const uint8_t *a_scales, int k,
                      const void *gate_q, const uint8_t *gate_scales,
                      const void *up_q, const uint8_t *up_scales,
                      int b_row_step, MxFormat b_format, const void *gate_bias,
                      const void *up_bias, MxGlu glu, BlockMatrix c, void *hq,
                      uint8_t *h_scales, MxGluKeep keep, DataType dtype,
                      hipStream_t stream);

// ---- Gradients (above). ----

// What QuantizeBlocksMx applies to the block values before it quantises them.
enum class MxBlockStage { kNone = 0, kActivation = 1, kActivationGrad = 2 };

hipError_t QuantizeTilesMx(const void *x, int rows, int cols, void *q,
                           uint8_t *scales, void *qt, uint8_t *scales_t,
                           DataType dtype, hipStream_t stream);

// `activation` is read when `stage` is not kNone, `z` when it is
// kActivationGrad.
hipError_t QuantizeBlocksMx(const BlockMatrix s, MxBlockStage stage,
                            Activation activation, const void *z, void *q,
                            uint8_t *scales, void *qt, uint8_t *scales_t,
                            DataType dtype, hipStream_t stream);

hipError_t DsdMxWgrad(const BlockMatrix s, const uint8_t *s_scales,
                      const void *bq, const uint8_t *b_scales, Matrix c,
                      OutputType out, bool add, DataType dtype,
                      hipStream_t stream);

// ---- Gradients of a gated expert (above). ----

struct MxImages {
  void *q;
  uint8_t *scales;
  void *qt;
  uint8_t *scales_t;
};

hipError_t QuantizeBlocksMxGated(const BlockMatrix s, const void *gate,
                                 Activation activation, MxImages h,
                                 DataType dtype, hipStream_t stream);

hipError_t QuantizeBlocksMxGatedGrad(const BlockMatrix d, const void *gate,
                                     const void *up, Activation activation,
                                     MxImages dg, MxImages du, DataType dtype,
                                     hipStream_t stream);

hipError_t DsdMxPair(const BlockMatrix s1, const uint8_t *s1_scales,
                     const void *b1q, const uint8_t *b1_scales,
                     const void *s2_data, const uint8_t *s2_scales,
                     const void *b2q, const uint8_t *b2_scales, Matrix c,
                     DataType dtype, hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_MX_H_
