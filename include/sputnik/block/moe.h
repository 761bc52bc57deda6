// sputnik-amd: MoE token permutation, the step on either side of the expert
// MLP: a router's top_experts become the padded, expert-sorted activation
// matrix that the dMoE topology (sputnik_expert_topology) describes, and the
// expert outputs come back to token order with the router weights. The
// counterparts of MegaBlocks' padded_gather, padded_scatter and
// padded_scatter_wgrad. No counterpart in the reference.
//
// Notation: T the operand type (fp16 / bf16), n = tokens * top_k assignments,
// assignment a = t * top_k + k, E = num_experts. The routing tensors are
// MegaBlocks' (indices_and_padded_bins), all int32:
//   bin_ids, indices   stable ascending sort of top_experts.flatten();
//                      indices[i] is the assignment at sorted position i
//   bins               inclusive cumsum of the per-expert counts
//   padded_bins        inclusive cumsum of the counts, each rounded up to a
//                      multiple of 128
//   row(i)             padded_bins[e-1] + (i - bins[e-1]) with e = bin_ids[i]
//                      (index -1 read as 0): the padded row of position i
//   row_of[indices[i]] = row(i), one padded row per assignment
//
//   MoeBins       bins, tokens_per_expert and padded_bins from the sorted
//                 bin_ids (the sort itself is the caller's).
//   MoeRowMap     row_of. A position whose bin id is outside [0, E) or whose
//                 row is outside [0, rows) gets -1; a position whose index
//                 is outside [0, n) is skipped.
//   PaddedGather  x [tokens, hidden] -> out [rows, hidden]:
//                   out[row(i)] = x[indices[i] / top_k], bit for bit, or with
//                   weights round_T(float(w[indices[i]]) * float(x[...])).
//                 Every other row of out is written as +0 by the same kernel
//                 (padding inside a bin, rows past padded_bins[E-1]); out
//                 needs no initialisation.
//   PaddedScatter y [rows, hidden] -> out [tokens, hidden]:
//                   out[t] = round_T(sum_k float(w[t top_k + k]) *
//                                          float(y[row_of[t top_k + k]]))
//                 summed in fp32 from 0 in ascending k and rounded once;
//                 without weights a plain sum. No atomics and no
//                 [n, hidden] intermediate, so the result is bitwise
//                 reproducible.
//   PaddedScatterWeightGrad
//                 dw[a] = sum_h float(dout[a / top_k, h]) *
//                               float(y[row_of[a], h]), accumulated in fp32
//                 (free order), stored in the weights' type.
//
//   PaddedScatterBias
//                 PaddedScatter with an output bias b2 [E, hidden] of T:
//                   out[t] = round_T(sum_k float(w_k) * (float(y[row_k]) +
//                                                        float(b2[e_k])))
//                 one fp32 add, one fp32 multiply (omitted without weights)
//                 and one fp32 accumulate per k, ascending k from 0, no
//                 contraction. e_k is read off the row: the number of experts
//                 with padded_bins[e] <= row_k. An assignment whose row is
//                 outside [0, rows), or at or past padded_bins[E-1],
//                 contributes zero, bias included.
//   PaddedScatterBiasWeightGrad
//                 dw[a] = sum_h float(dout[a / top_k, h]) *
//                         (float(y[row_of[a], h]) + float(b2[e, h])), as
//                 PaddedScatterWeightGrad.
//   PaddedScatterBiasGrad
//                 bias_grad[e, h] = sum over e's sorted positions i in
//                 [bins[e-1], bins[e]) of float(w[indices[i]]) *
//                 float(dout[indices[i] / top_k, h]): fp32 [E, hidden] from
//                 the unrounded products (without weights a plain sum). No
//                 atomics and no workspace; the order of the sum depends on
//                 the bins alone, so two runs give the same bits. An expert
//                 without tokens gives +0.
//
// The gradients are these same calls: d PaddedGather / dx is the unweighted
// PaddedScatter, d PaddedScatter / dy is PaddedGather of dout with the
// weights, d PaddedScatter / dw is PaddedScatterWeightGrad.
//
// With the bias, dy is unchanged and dw / db2 are the two calls above.
//
// weights: n elements of T (WeightType::kOperand) or of float
// (WeightType::kF32), indexed by assignment; null means unweighted.
//
// Bounds: every index read from device memory is checked before it is used
// as an address (indices[i], bin_ids[i], row_of[a], a row at or past rows);
// an entry out of range contributes zeros. No kernel reads or writes outside
// its buffers, whatever the metadata holds.
//
// 16-byte accesses when hidden % 8 == 0 and the row buffers are 16-byte
// aligned, element accesses otherwise; same results. Stream-ordered; no call
// allocates or synchronises. They never abort: hipErrorInvalidValue, with
// nothing launched, for a null required buffer, a negative size, top_k < 1,
// rows % 128 != 0, tokens * top_k or n + 127 E past INT_MAX, or an output
// that is one of the inputs. Zero-sized work succeeds.
#ifndef SPUTNIK_BLOCK_MOE_H_
#define SPUTNIK_BLOCK_MOE_H_

#include "sputnik/block/arguments.h"
#include "sputnik/block/dtype.h"

namespace sputnik {
namespace block {

enum class WeightType { kOperand = 0, kF32 = 1 };

hipError_t MoeBins(const int *bin_ids, int n, int num_experts, int *bins,
                   int *tokens_per_expert, int *padded_bins,
                   hipStream_t stream);

hipError_t MoeRowMap(const int *indices, const int *bin_ids, const int *bins,
                     const int *padded_bins, int n, int num_experts, int rows,
                     int *row_of, hipStream_t stream);

hipError_t PaddedGather(const void *x, const int *indices, const int *bins,
                        const int *padded_bins, const void *weights,
                        void *out, int tokens, int hidden, int top_k,
                        int num_experts, int rows, DataType dtype,
                        WeightType weights_type, hipStream_t stream);

hipError_t PaddedScatter(const void *y, const int *row_of,
                         const void *weights, void *out, int tokens,
                         int hidden, int top_k, int rows, DataType dtype,
                         WeightType weights_type, hipStream_t stream);

hipError_t PaddedScatterWeightGrad(const void *dout, const void *y,
                                   const int *row_of, void *dw, int tokens,
                                   int hidden, int top_k, int rows,
                                   DataType dtype, WeightType weights_type,
                                   hipStream_t stream);

hipError_t PaddedScatterBias(const void *y, const int *row_of,
                             const int *padded_bins, const void *bias,
                             const void *weights, void *out, int tokens,
                             int hidden, int top_k, int num_experts, int rows,
                             DataType dtype, WeightType weights_type,
                             hipStream_t stream);

hipError_t PaddedScatterBiasWeightGrad(const void *dout, const void *y,
                                       const int *row_of,
                                       const int *padded_bins,
                                       const void *bias, void *dw, int tokens,
                                       int hidden, int top_k, int num_experts,
                                       int rows, DataType dtype,
                                       WeightType weights_type,
                                       hipStream_t stream);

hipError_t PaddedScatterBiasGrad(const void *dout, const int *indices,
                                 const int *bins, const void *weights,
                                 float *bias_grad, int tokens, int hidden,
                                 int top_k, int num_experts, DataType dtype,
                                 WeightType weights_type, hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_MOE_H_
