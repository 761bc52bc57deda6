// sputnik-amd: SDD with a gated (GLU) epilogue, the two products a gated
// expert MLP y = (act(x w1) * (x v1)) w2 needs around its sparse hidden
// matrices. No counterpart in the reference, whose callers run the gate as
// separate elementwise passes over c.data.
//
//   MatmulGated      U  = round_T(acc)
//                    H  = round_T(float(U) * act(float(G)) + 0.0f)
//                    H -> c.data;  U -> up when not null;  G <- gate (required)
//   MatmulGatedGrad  D  = round_T(acc)
//                    dU = round_T(float(D) * act(float(G)) + 0.0f)  -> up_grad
//                    dG = round_T((float(D) * float(U)) * act'(float(G)) + 0.0f)
//                                                                   -> c.data
//                    G <- gate, U <- up, up_grad: all required
//
// at c's nonzero blocks. acc is the fp32 accumulator the plain SDD Matmul
// would round and T the operand type. gate, up and up_grad hold c.nonzeros
// elements of T in c's storage order, as c.data does. act and act' are the
// activations of activation.h, evaluated in fp32 and not rounded to T in
// between; float(D) * float(U) is exact in fp32, so each result carries the
// activation's error, one fp32 rounding and one rounding to T. An exactly
// zero result is stored as +0. The rounding of acc before the elementwise
// stage is part of the contract: H equals the gate of the stored (U, G) bit
// for bit (a caller may drop H and recompute it), the results are those of
// the plain product followed by an elementwise pass, and they do not depend
// on which kernel the dispatcher picks. NaN or +-inf in G, U or D gives what
// the formulas yield in fp32.
//
// Buffers: up_grad may be exactly up (in place: every 16-byte chunk is read
// before it is written, by the same thread). Otherwise none of gate, up,
// up_grad, c.data, A, B may overlap; a pointer that equals one it must not
// overlap, or a required pointer that is null, is rejected with
// hipErrorInvalidValue before anything is launched.
//
// Stream ordering, graph capture, the transposed-B workspace rules and the
// acceptance rules are those of the SDD Matmul (c.row_indices is needed);
// these calls abort where it aborts. All four transposes, fp16 and bf16,
// block size 128.
#ifndef SPUTNIK_BLOCK_GATED_H_
#define SPUTNIK_BLOCK_GATED_H_

#include "sputnik/block/activation.h"
#include "sputnik/block/arguments.h"
#include "sputnik/block/dtype.h"

namespace sputnik {
namespace block {

hipError_t MatmulGated(const Matrix a, bool transpose_a, const Matrix b,
                       bool transpose_b, BlockMatrix c, Activation activation,
                       const void *gate, void *up, DataType dtype,
                       hipStream_t stream);

hipError_t MatmulGatedGrad(const Matrix a, bool transpose_a, const Matrix b,
                           bool transpose_b, BlockMatrix c,
                           Activation activation, const void *gate,
                           const void *up, void *up_grad, DataType dtype,
                           hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_GATED_H_
