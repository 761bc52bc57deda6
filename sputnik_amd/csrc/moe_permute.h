// sputnik-amd: MoE token permutation (see moe_permute.hip and
// sputnik/block/moe.h). Host entry points shared by the C++ API and the
// C-ABI: each validates its arguments (hipErrorInvalidValue, nothing
// launched), returns hipSuccess for zero-sized work, and otherwise enqueues
// its kernel on `stream`. None allocates or synchronises.
#ifndef SPUTNIK_AMD_MOE_PERMUTE_H_
#define SPUTNIK_AMD_MOE_PERMUTE_H_

#include <hip/hip_runtime_api.h>

namespace sputnik_amd {

// dtype: 0 fp16, 1 bf16. weights_dtype: 0 the operand type, 1 fp32.

hipError_t RunMoeBins(const int *bin_ids, int n, int num_experts, int *bins,
                      int *tokens_per_expert, int *padded_bins,
                      hipStream_t stream);

hipError_t RunMoeRowMap(const int *indices, const int *bin_ids,
                        const int *bins, const int *padded_bins, int n,
                        int num_experts, int rows, int *row_of,
                        hipStream_t stream);

hipError_t RunPaddedGather(const void *x, const int *indices, const int *bins,
                           const int *padded_bins, const void *weights,
                           void *out, int tokens, int hidden, int top_k,
                           int num_experts, int rows, int dtype,
                           int weights_dtype, hipStream_t stream);

hipError_t RunPaddedScatter(const void *y, const int *row_of,
                            const void *weights, void *out, int tokens,
                            int hidden, int top_k, int rows, int dtype,
                            int weights_dtype, hipStream_t stream);

hipError_t RunPaddedScatterWgrad(const void *dout, const void *y,
                                 const int *row_of, void *dw, int tokens,
                                 int hidden, int top_k, int rows, int dtype,
                                 int weights_dtype, hipStream_t stream);

// The scatter with an output bias [num_experts, hidden] of the operand type
// and its gradients (moe.h PaddedScatterBias*): the expert of an assignment
// is read off its row through padded_bins.
hipError_t RunPaddedScatterBias(const void *y, const int *row_of,
                                const int *padded_bins, const void *bias,
                                const void *weights, void *out, int tokens,
                                int hidden, int top_k, int num_experts,
                                int rows, int dtype, int weights_dtype,
                                hipStream_t stream);

hipError_t RunPaddedScatterBiasWgrad(const void *dout, const void *y,
                                     const int *row_of, const int *padded_bins,
                                     const void *bias, void *dw, int tokens,
                                     int hidden, int top_k, int num_experts,
                                     int rows, int dtype, int weights_dtype,
                                     hipStream_t stream);

hipError_t RunPaddedScatterBiasGrad(const void *dout, const int *indices,
                                    const int *bins, const void *weights,
                                    float *db, int tokens, int hidden,
                                    int top_k, int num_experts, int dtype,
                                    int weights_dtype, hipStream_t stream);

}  // namespace sputnik_amd

#endif  // SPUTNIK_AMD_MOE_PERMUTE_H_
