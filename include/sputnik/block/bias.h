// sputnik-amd: SDD with a column bias, for expert MLPs whose projections have
// per-expert biases, and the bias gradient of a sparse matrix. No counterpart
// in the reference, whose callers add a bias as separate elementwise passes.
//
// A bias b holds c.cols elements of the operand type T, indexed by C's
// logical column. With x = round_T(acc), the value the plain SDD Matmul
// stores, the bias stage is
//
//   xb = round_T((float(x) + float(b[col])) + 0.0f)
//
// in fp32 with no contraction, and everything behind it sees xb where the
// bias-free product sees x:
//
//   MatmulBias            C = xb
//   MatmulBiasActivation  Z = xb, H = act(Z) as MatmulActivation;
//                         H -> c.data, Z -> pre_activation when not null
//   MatmulBiasGated       U = xb, H = U * act(G) as MatmulGated;
//                         H -> c.data, U -> up when not null, G <- gate
//                         (required; it would itself come from MatmulBias)
//
// The kept Z / U is the biased one, so the gradient products
// (MatmulActivationGrad, MatmulGatedGrad) read it as they stand. The rounding
// of acc before the add is part of the contract, as in activation.h: the
// results are those of the plain product followed by an elementwise pass, bit
// for bit, whichever kernel the dispatcher picks (the routes and the
// "sdd_act_route" knob are activation.h's), and H equals the activation or
// gate of the stored Z / (U, G).
//
// The bias may have any 2-byte alignment; it is read with 16-byte loads where
// it is 16-byte aligned. A bias that is null, or that equals c.data,
// pre_activation / gate / up, A or B, is rejected with hipErrorInvalidValue
// before anything is launched; the buffer rules of activation.h and gated.h
// hold besides.
//
//   BlockColumnSum        out[c] = sum_r float(S[r, c]) over the stored blocks
//                         of S, fp32 [S.cols]: the bias gradient of a sparse
//                         dZ / dG / dU.
//
// A column block without a stored block gives +0. No atomics and no
// workspace: the order of the sum is a function of the topology alone, so two
// runs give the same bits. It walks a column through S's transposed metadata
// (offsets_t, block_offsets), which must be there: a null buffer is
// hipErrorInvalidValue. Entries of that metadata out of range are skipped.
//
// Stream ordering, graph capture, the workspace rules and the acceptance
// rules are those of the SDD Matmul; the three products abort where it
// aborts. BlockColumnSum never aborts.
#ifndef SPUTNIK_BLOCK_BIAS_H_
#define SPUTNIK_BLOCK_BIAS_H_

#include "sputnik/block/activation.h"
#include "sputnik/block/arguments.h"
#include "sputnik/block/dtype.h"

namespace sputnik {
namespace block {

hipError_t MatmulBias(const Matrix a, bool transpose_a, const Matrix b,
                      bool transpose_b, BlockMatrix c, const void *bias,
                      DataType dtype, hipStream_t stream);

hipError_t MatmulBiasActivation(const Matrix a, bool transpose_a,
                                const Matrix b, bool transpose_b,
                                BlockMatrix c, const void *bias,
                                Activation activation, void *pre_activation,
                                DataType dtype, hipStream_t stream);

hipError_t MatmulBiasGated(const Matrix a, bool transpose_a, const Matrix b,
                           bool transpose_b, BlockMatrix c, const void *bias,
                           Activation activation, const void *gate, void *up,
                           DataType dtype, hipStream_t stream);

hipError_t BlockColumnSum(const BlockMatrix s, DataType dtype, float *out,
                          hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_BIAS_H_
