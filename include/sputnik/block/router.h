// sputnik-amd: the MoE router in front of the token permutation (moe.h): the
// fused softmax / top-k of the router logits with its gradient, and the
// device sort that turns the router's choice into MegaBlocks' routing tensors
// in one call. The counterparts of MegaBlocks' LearnedRouter arithmetic and
// of its sort / histogram ops. No counterpart in the reference.
//
// Notation: L the logits' type (RouterType), E = num_experts, k = top_k,
// n = tokens * top_k assignments, assignment a = t * top_k + k. W is the type
// of weights, scores and their gradients: L (WeightType::kOperand) or float
// (WeightType::kF32).
//
//   RouterTopK      logits [tokens, E] -> top_experts int32 [tokens, k],
//                   weights W [tokens, k] and, when `scores` is not null,
//                   scores W [tokens, E].
//                   Selection is on the logits themselves: the k largest in
//                   descending order, equal values to the lower expert index
//                   (-0 equals +0), NaN below -inf (NaNs among themselves by
//                   index). Every row yields k distinct ids in [0, E) whatever
//                   the logits hold.
//                   Arithmetic in fp32: p_e = exp(l_e - m) / sum_j exp(l_j - m)
//                   with m the value of the first pick (the row maximum);
//                   w_k = p_{sel k}, or with `normalize`
//                   w_k = p_{sel k} / sum_k' p_{sel k'}; scores = p. Each
//                   output is rounded once to W. A row holding NaN, +inf or
//                   only -inf gets what that formula gives; only its ids are
//                   pinned.
//   RouterTopKGrad  dlogits L [tokens, E] from the logits, top_experts,
//                   dweights W [tokens, k] and an optional dscores W
//                   [tokens, E]. The softmax is recomputed (the forward pass
//                   saves nothing): dp = dscores (or 0) plus, at each selected
//                   column, dw_k, or with `normalize` (dw_k - sum_j dw_j w_j)
//                   / S with S = sum_k p_{sel k}; dlogits_j = p_j (dp_j -
//                   sum_i dp_i p_i). fp32, rounded once. A top_experts entry
//                   outside [0, E) contributes nothing (neither to dp nor to
//                   S); a duplicated entry adds twice.
//   RouterTopKAux   RouterTopK (the same ids, weights and scores bit for bit)
//                   plus the statistics the auxiliary losses are formed from,
//                   fp32 whatever L and W are and taken from the unrounded
//                   values: score_sums[e] = sum_t p_te (float [E], required)
//                   and, when `z_sum` is not null, z_sum[0] = sum_t lse_t^2
//                   with lse_t = m_t + log sum_j exp(l_tj - m_t) (float [1]).
//                   MegaBlocks' load-balancing loss of one layer is
//                   E / (tokens^2 k) sum_e tokens_per_expert_e score_sums_e,
//                   the router z-loss z_sum / tokens.
//                   A workgroup covers kRouterAuxTokens consecutive tokens, a
//                   wave a quarter of them in order; the waves are added in
//                   wave order and the workgroup stores its E + 1 partials to
//                   the workspace; a second launch adds the workgroups in
//                   ascending order. No atomics: the sums depend on the input
//                   alone, bit for bit.
//                   workspace: RouterAuxWorkspaceBytes(tokens, E) =
//                   ceil(tokens / kRouterAuxTokens) * (E + 1) * 4 bytes, the
//                   caller's, 4-byte aligned, no initialisation needed.
//                   tokens = 0 needs none and still writes E zeros and 0.
//                   A row holding NaN, +-inf or only -inf enters the sums
//                   with what the formulas give.
//   RouterTopKAuxGrad  RouterTopKGrad with the gradients of the statistics:
//                   dscore_sums (float [E]) and dz_sum (float [1], read on
//                   the device), either may be null. dp_j = dscores_j (or 0)
//                   + the pick terms + dscore_sums_j (or 0); dlogits_j = p_j
//                   (dp_j - sum_i dp_i p_i) + 2 dz_sum lse p_j, fp32, rounded
//                   once. With both null: RouterTopKGrad bit for bit.
//   RouterScoreTopK  the router of DeepSeek-V3 and its successors: sigmoid
//                   scores, a per-expert selection bias, a group-limited
//                   choice. logits [tokens, E], bias float [E] (null: 0) ->
//                   top_experts int32 [tokens, k], weights W [tokens, k] and,
//                   when `scores` is not null, scores W [tokens, E]. fp32
//                   throughout, each output rounded once.
//                   Scores: s_e = 1 / (1 + expf(-l_e)).
//                   Selection value: c_e = s_e + bias_e, as computed in fp32.
//                   Two different logits whose c rounds to the same float are
//                   a tie (saturated sigmoids, for instance) and go to the
//                   lower index.
//                   Order, here and below: the larger value first, equal
//                   values to the lower index (-0 equals +0), NaN below -inf
//                   (NaNs among themselves by index).
//                   Groups: G = num_groups, gs = E / G, group g owns the
//                   experts [g gs, (g + 1) gs). Its score is a + b in fp32
//                   with a, b the first two of its c values in that order (a
//                   alone when gs = 1). The topk_groups groups first in that
//                   order on the group scores are eligible (ties to the lower
//                   group, NaN last). G = 1: no group step.
//                   Picks: the k first eligible experts in that order on c:
//                   every row yields k distinct ids in [0, E) whatever the
//                   logits and the bias hold.
//                   Weights: w_k = s_{sel k} (without the bias); with
//                   `normalize` divided by sum_k' s_{sel k'} (no epsilon: a
//                   zero sum gives what the formula gives); then multiplied by
//                   `scale`. scores = s.
//   RouterScoreTopKGrad  dlogits L [tokens, E] from the logits, top_experts,
//                   dweights W [tokens, k] and an optional dscores W
//                   [tokens, E]; s is recomputed. g_k = scale dw_k, or with
//                   `normalize` g_k = scale (dw_k - sum_j dw_j s_j / S) / S
//                   with S = sum_k s_{sel k}; ds_e = dscores_e (or 0) +
//                   sum_{k: sel k = e} g_k; dlogits_e = ds_e s_e (1 - s_e).
//                   fp32, rounded once. A top_experts entry outside [0, E)
//                   contributes nothing (neither to ds nor to S); a
//                   duplicated entry adds twice. Bias and groups do not enter
//                   the gradient; the bias has none.
//   MoeSort         top_experts.flatten() int32 [n] -> indices, bin_ids [n],
//                   bins, tokens_per_expert, padded_bins [E] and row_of [n] as
//                   moe.h defines them: a stable counting sort by expert. For
//                   ids in [0, E) every output is bit-identical to a stable
//                   sort followed by MoeBins and MoeRowMap. An id outside
//                   [0, E) is counted in no bin, gets row_of = -1 and takes
//                   the sorted positions from bins[E-1] on, in assignment
//                   order, with bin_ids = E (PaddedGather ignores positions
//                   past bins[E-1]). `rows` as in MoeRowMap: a multiple of
//                   128; a row at or past it maps to -1.
//                   Three launches over chunks of kMoeSortChunk assignments:
//                   per-chunk histograms (LDS integer adds), one workgroup
//                   that scans [chunks, E + 1] counts into first positions and
//                   writes bins / tokens_per_expert / padded_bins, and the
//                   placement, which ranks an assignment among its chunk's
//                   equal ids by position (no global atomics). The result
//                   depends on the input alone.
//                   workspace: MoeSortWorkspaceBytes(n, E) =
//                   ceil(n / kMoeSortChunk) * (E + 1) * 4 bytes, the caller's,
//                   4-byte aligned, no initialisation needed.
//
// Limits: 1 <= E <= 1024; RouterTopK / RouterTopKGrad and their Aux forms
// 1 <= k <= min(E, 32). RouterScoreTopK: 1 <= topk_groups <= num_groups <= 64,
// E % num_groups == 0, 1 <= k <= min(32, topk_groups * E / num_groups);
// RouterScoreTopKGrad: 1 <= k <= min(E, 32); for both, `scale` is finite.
// Element offsets are long long (tokens * E may pass 2^31).
//
// Bounds: every id read from device memory (top_experts in RouterTopKGrad,
// RouterScoreTopKGrad and MoeSort) is range-checked before it forms an address.
//
// Stream-ordered; no call allocates or synchronises. They never abort:
// hipErrorInvalidValue, with nothing launched, for a null required buffer, a
// size outside the limits, an unknown type, rows % 128 != 0, n + 127 E past
// INT_MAX, a workspace that is too small or not 4-byte aligned, or an output
// that is one of the inputs, another output or the workspace. Zero-sized work
// succeeds (MoeSort with n = 0 still writes the E zero counts, RouterTopKAux
// with tokens = 0 the zero sums).
#ifndef SPUTNIK_BLOCK_ROUTER_H_
#define SPUTNIK_BLOCK_ROUTER_H_

#include <cstddef>

#include "sputnik/block/arguments.h"
#include "sputnik/block/moe.h"

namespace sputnik {
namespace block {

enum class RouterType { kF16 = 0, kBF16 = 1, kF32 = 2 };

// Assignments per histogram / placement workgroup of MoeSort.
constexpr int kMoeSortChunk = 1024;

hipError_t RouterTopK(const void *logits, int *top_experts, void *weights,
                      void *scores, int tokens, int num_experts, int top_k,
                      bool normalize, RouterType logits_type,
                      WeightType weights_type, hipStream_t stream);

hipError_t RouterTopKGrad(const void *logits, const int *top_experts,
                          const void *dweights, const void *dscores,
                          void *dlogits, int tokens, int num_experts,
                          int top_k, bool normalize, RouterType logits_type,
                          WeightType weights_type, hipStream_t stream);

// Tokens per workgroup of RouterTopKAux: four waves of 16 consecutive tokens.
// It fixes the summation order of score_sums / z_sum and the workspace size.
constexpr int kRouterAuxTokens = 64;

// 0 for sizes RouterTopKAux rejects.
size_t RouterAuxWorkspaceBytes(int tokens, int num_experts);

hipError_t RouterTopKAux(const void *logits, int *top_experts, void *weights,
                         void *scores, float *score_sums, float *z_sum,
                         int tokens, int num_experts, int top_k,
                         bool normalize, RouterType logits_type,
                         WeightType weights_type, void *workspace,
                         size_t workspace_bytes, hipStream_t stream);

hipError_t RouterTopKAuxGrad(const void *logits, const int *top_experts,
                             const void *dweights, const void *dscores,
                             const float *dscore_sums, const float *dz_sum,
                             void *dlogits, int tokens, int num_experts,
                             int top_k, bool normalize, RouterType logits_type,
                             WeightType weights_type, hipStream_t stream);

// Most groups RouterScoreTopK takes (one lane per group).
constexpr int kRouterMaxGroups = 64;

hipError_t RouterScoreTopK(const void *logits, const float *bias,
                           int *top_experts, void *weights, void *scores,
                           int tokens, int num_experts, int top_k,
                           int num_groups, int topk_groups, bool normalize,
                           float scale, RouterType logits_type,
                           WeightType weights_type, hipStream_t stream);

hipError_t RouterScoreTopKGrad(const void *logits, const int *top_experts,
                               const void *dweights, const void *dscores,
                               void *dlogits, int tokens, int num_experts,
                               int top_k, bool normalize, float scale,
                               RouterType logits_type,
                               WeightType weights_type, hipStream_t stream);

// 0 for sizes MoeSort rejects.
size_t MoeSortWorkspaceBytes(int n, int num_experts);

hipError_t MoeSort(const int *top_experts, int n, int num_experts, int rows,
                   int *indices, int *bin_ids, int *bins,
                   int *tokens_per_expert, int *padded_bins, int *row_of,
                   void *workspace, size_t workspace_bytes,
                   hipStream_t stream);

}  // namespace block
}  // namespace sputnik

#endif  // SPUTNIK_BLOCK_ROUTER_H_
