// sputnik-amd: SDD with a fused activation epilogue, the two products an
// expert MLP needs around its sparse hidden matrix. No counterpart in the
// reference, whose callers run the activation as a separate pass over
// c.data.
//
//   MatmulActivation      Z = round_T(acc),  H = round_T(act(float(Z)))
//                         H -> c.data;  Z -> pre_activation when not null
//   MatmulActivationGrad  C = round_T(float(round_T(acc)) * act'(float(Z)))
//                         C -> c.data;  Z <- pre_activation (required)
//
// at c's nonzero blocks. acc is the fp32 accumulator the plain SDD Matmul
// would round and T the operand type. pre_activation holds c.nonzeros
// elements of T in c's storage order, as c.data does. The intermediate
// rounding is part of the contract: H equals act(Z) of the stored Z bit for
// bit (a caller may drop H and recompute it), the results are those of the
// plain product followed by an elementwise pass, and they do not depend on
// which kernel the dispatcher picks.
//
// Activations, evaluated in fp32:
//   kRelu  max(x, 0);                       derivative x > 0 ? 1 : 0
//   kGelu  the tanh form as a sigmoid: u = sqrt(2/pi) (x + 0.044715 x^3),
//          s = 1 / (1 + exp(-2u)), gelu = x s;
//          derivative s + x s (1 - s) 2 sqrt(2/pi) (1 + 0.134145 x^2)
//   kSilu  s = 1 / (1 + exp(-x)), silu = x s; derivative s (1 + x (1 - s))
// An exactly zero result is stored as +0 (the fp32 value has +0 added before
// it is rounded), so it does not depend on which instructions evaluate it.
// Every finite Z gives a finite result. NaN or +-inf in Z gives what these
// formulas yield in fp32 (relu(NaN) = 0; gelu and silu of -inf are NaN).
//
// pre_activation must not overlap c.data, A or B. Stream ordering, graph
// capture, the transposed-B workspace rules and the acceptance rules are
// those of the SDD Matmul (c.row_indices is needed); these calls abort where
// it aborts. All four transposes, fp16 and bf16, block size 128.
#ifndef SPUTNIK_BLOCK_ACTIVATION_H_
#define SPUTNIK_BLOCK_ACTIVATION_H_

#include "sputnik/block/arguments.h"
#include "sputnik/block/dtype.h"

namespace sputnik {
namespace block {

enum class Activation { kRelu = 0, kGelu = 1, kSilu = 2 };

hipError_t MatmulActivation(const Matrix a, bool transpose_a, const Matrix b,
                            bool transpose_b, BlockMatrix c,
                            Activation activation, void *pre_activation,
                            DataType dtype, hipStream_t stream);

hipError_t MatmulActivationGrad(const Matrix a, bool transpose_a,
                                const Matrix b, bool transpose_b,
                                BlockMatrix c, Activation activation,
                                const void *pre_activation, DataType dtype,
                                hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_ACTIVATION_H_
