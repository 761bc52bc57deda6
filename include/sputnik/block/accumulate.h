// sputnik-amd: accumulating dense-output products, C += op(A) * op(B) for
// DSD and DDS. No counterpart in the reference, whose products overwrite C;
// a caller that sums weight gradients over micro-batches otherwise pays a
// weight-sized temporary and a separate add per product.
//
//   C_out[i, j] = round_Tc(acc_fp32[i, j] + float(C_in[i, j]))
//
// acc_fp32 is the fp32 accumulator the plain product would round. Tc is the
// operands' type (OutputType::kOperand: c.data holds fp16 / bf16, as for
// Matmul) or fp32 (OutputType::kF32: c.data holds rows x cols floats; no
// rounding beyond the fp32 add). The sum is rounded once, after the add.
//
// Where the sparse operand has no blocks (empty block-rows of op(A) for DSD,
// empty block-columns of op(B) for DDS) C is neither read nor written. Every
// other element of C is read and written exactly once per call. C must not
// overlap A or B.
//
// Stream ordering, graph capture, the pair workspaces, the error word and
// the timeout behaviour are those of Matmul. These calls always run the
// 8-wave kernel: never the 4-wave kernel, split mode or the transposed-B
// route, so they use no transposed-B workspace. All four transposes, fp16
// and bf16 operands; they abort where Matmul aborts.
#ifndef SPUTNIK_BLOCK_ACCUMULATE_H_
#define SPUTNIK_BLOCK_ACCUMULATE_H_

#include "sputnik/block/arguments.h"
#include "sputnik/block/dtype.h"

namespace sputnik {
namespace block {

enum class OutputType { kOperand = 0, kF32 = 1 };

// DSD. Builds transposed metadata of `a` on the device when transpose_a
// (a.create_metadata == true); the Ex form uses what `a` already holds.
hipError_t MatmulAccumulate(const BlockMatrix a, bool transpose_a,
                            const Matrix b, bool transpose_b, Matrix c,
                            DataType dtype, OutputType c_type,
                            hipStream_t stream);
hipError_t MatmulAccumulateEx(const BlockMatrix a, bool transpose_a,
                              const Matrix b, bool transpose_b, Matrix c,
                              DataType dtype, OutputType c_type,
                              hipStream_t stream);

// DDS. Builds transposed metadata of `b` when !transpose_b.
hipError_t MatmulAccumulate(const Matrix a, bool transpose_a,
                            const BlockMatrix b, bool transpose_b, Matrix c,
                            DataType dtype, OutputType c_type,
                            hipStream_t stream);
hipError_t MatmulAccumulateEx(const Matrix a, bool transpose_a,
                              const BlockMatrix b, bool transpose_b, Matrix c,
                              DataType dtype, OutputType c_type,
                              hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_ACCUMULATE_H_
