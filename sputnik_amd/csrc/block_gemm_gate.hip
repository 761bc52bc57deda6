// sputnik-amd: the gated SDD products on the 8-wave kernel,
// H = (A B) * act(G) (with U = A B stored on request) and the pair
// dU = (A B) * act(G), dG = (A B) * U * act'(G) (block_gemm.h kOutGate /
// kOutGateGrad). Their own translation unit, as block_gemm_act.hip is, so
// every other instantiation is compiled exactly as before. Which activation
// runs is a runtime field (GemmParams::act), so there are two modes x the
// plain SDD's instantiations: CfgSdd (one k-split block per workgroup) and
// CfgSddGrouped, four transposes, two types.
#include "block_gemm.h"

namespace sputnik_amd {
namespace {

template <typename T, bool kSKC, bool kDKC, class Cfg, int kMode>
hipError_t LaunchCfg(const GemmParams &p, hipStream_t stream) {
  hipLaunchKernelGGL((block_gemm_kernel<T, true, kSKC, kDKC, false, Cfg,
                                        false, false, kMode>),
                     dim3(p.grid > 0 ? p.grid : p.num_tiles),
                     dim3(64 * Cfg::kWaves), 0, stream, p);
  return hipGetLastError();
}

template <typename T, bool kSKC, bool kDKC>
hipError_t Launch(const GemmParams &p, bool grouped, int mode,
                  hipStream_t stream) {
  if (p.num_tiles <= 0) return hipSuccess;
  if (grouped) {
    if (mode == kOutGateGrad)
      return LaunchCfg<T, kSKC, kDKC, CfgSddGrouped, kOutGateGrad>(p, stream);
    return LaunchCfg<T, kSKC, kDKC, CfgSddGrouped, kOutGate>(p, stream);
  }
  if (mode == kOutGateGrad)
    return LaunchCfg<T, kSKC, kDKC, CfgSdd, kOutGateGrad>(p, stream);
  return LaunchCfg<T, kSKC, kDKC, CfgSdd, kOutGate>(p, stream);
}

template <typename T>
hipError_t LaunchTyped(bool s_kc, bool d_kc, bool grouped, int mode,
                       const GemmParams &p, hipStream_t stream) {
  if (s_kc && d_kc) return Launch<T, true, true>(p, grouped, mode, stream);     // NT
  if (s_kc) return Launch<T, true, false>(p, grouped, mode, stream);            // NN
  if (d_kc) return Launch<T, false, true>(p, grouped, mode, stream);            // TT
  return Launch<T, false, false>(p, grouped, mode, stream);                     // TN
}

}  // namespace

hipError_t LaunchBlockGemmGate(int dtype, bool s_kc, bool d_kc, bool grouped,
                               int out_mode, const GemmParams &params,
                               hipStream_t stream) {
  if (out_mode != kOutGate && out_mode != kOutGateGrad)
    return hipErrorInvalidValue;
  if (params.z_data == nullptr) return hipErrorInvalidValue;
  if (out_mode == kOutGateGrad &&
      (params.u_data == nullptr || params.du_data == nullptr))
    return hipErrorInvalidValue;
  if (params.sdd_tail != 0 || params.sdd_ksplit > 1) return hipErrorInvalidValue;
  if (dtype == 1)
    return LaunchTyped<__bf16>(s_kc, d_kc, grouped, out_mode, params, stream);
  return LaunchTyped<_Float16>(s_kc, d_kc, grouped, out_mode, params, stream);
}

}  // namespace sputnik_amd
