// sputnik-amd: the MoE router and the device sort (see moe_router.hip and
// sputnik/block/router.h). Host entry points shared by the C++ API and the
// C-ABI: each validates its arguments (hipErrorInvalidValue, nothing
// launched), returns hipSuccess for zero-sized work, and otherwise enqueues
// its kernels on `stream`. None allocates or synchronises.
#ifndef SPUTNIK_AMD_MOE_ROUTER_H_
#define SPUTNIK_AMD_MOE_ROUTER_H_

#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace sputnik_amd {

// logits_dtype: 0 fp16, 1 bf16, 2 fp32. weights_dtype: 0 the logits' type,
// 1 fp32 (weights, scores and their gradients).

hipError_t RunRouterTopK(const void *logits, int *top_experts, void *weights,
                         void *scores, int tokens, int num_experts, int top_k,
                         bool normalize, int logits_dtype, int weights_dtype,
                         hipStream_t stream);

hipError_t RunRouterTopKGrad(const void *logits, const int *top_experts,
                             const void *dweights, const void *dscores,
                             void *dlogits, int tokens, int num_experts,
                             int top_k, bool normalize, int logits_dtype,
                             int weights_dtype, hipStream_t stream);

size_t RouterAuxWorkspace(int tokens, int num_experts);

hipError_t RunRouterTopKAux(const void *logits, int *top_experts,
                            void *weights, void *scores, float *score_sums,
                            float *z_sum, int tokens, int num_experts,
                            int top_k, bool normalize, int logits_dtype,
                            int weights_dtype, void *workspace,
                            size_t workspace_bytes, hipStream_t stream);

hipError_t RunRouterTopKAuxGrad(const void *logits, const int *top_experts,
                                const void *dweights, const void *dscores,
                                const float *dscore_sums, const float *dz_sum,
                                void *dlogits, int tokens, int num_experts,
                                int top_k, bool normalize, int logits_dtype,
                                int weights_dtype, hipStream_t stream);

size_t MoeSortWorkspace(int n, int num_experts);

hipError_t RunMoeSort(const int *top_experts, int n, int num_experts, int rows,
                      int *indices, int *bin_ids, int *bins,
                      int *tokens_per_expert, int *padded_bins, int *row_of,
                      void *workspace, size_t workspace_bytes,
                      hipStream_t stream);

}  // namespace sputnik_amd

#endif  // SPUTNIK_AMD_MOE_ROUTER_H_
