// sputnik-amd: the SDD epilogue ops (act_math.h SddEpilogue) fused into the
// 8-wave kernel: the activation products H = act(A B) (Z = A B stored on
// request) and C = (A B) * act'(Z), and the gated products H = (A B) * act(G)
// (U = A B stored on request) and the pair dU = (A B) * act(G), dG =
// (A B) * U * act'(G), and the column bias of the forward ops and on its own
// (sputnik/block/bias.h; block_gemm.h kOutMode). Their own translation unit,
// so the plain products' instantiations in block_gemm.hip are compiled
// exactly as before. Which activation runs is a runtime field
// (GemmParams::act), so there are five modes x the plain SDD's
// instantiations: CfgSdd (one k-split block per workgroup) and
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

template <typename T, bool kSKC, bool kDKC, int kMode>
hipError_t Launch(const GemmParams &p, bool grouped, hipStream_t stream) {
  if (p.num_tiles <= 0) return hipSuccess;
  if (grouped)
    return LaunchCfg<T, kSKC, kDKC, CfgSddGrouped, kMode>(p, stream);
  return LaunchCfg<T, kSKC, kDKC, CfgSdd, kMode>(p, stream);
}

template <typename T, int kMode>
hipError_t LaunchTyped(bool s_kc, bool d_kc, bool grouped,
                       const GemmParams &p, hipStream_t stream) {
  if (s_kc && d_kc) return Launch<T, true, true, kMode>(p, grouped, stream);  // NT
  if (s_kc) return Launch<T, true, false, kMode>(p, grouped, stream);         // NN
  if (d_kc) return Launch<T, false, true, kMode>(p, grouped, stream);         // TT
  return Launch<T, false, false, kMode>(p, grouped, stream);                  // TN
}

}  // namespace

hipError_t LaunchBlockGemmEpilogue(int dtype, bool s_kc, bool d_kc,
                                   bool grouped, int out_mode,
                                   const GemmParams &params,
                                   hipStream_t stream) {
  if (params.sdd_tail != 0 || params.sdd_ksplit > 1) return hipErrorInvalidValue;
  return WithSddEpilogue(out_mode, hipErrorInvalidValue, [&](auto e) {
    using E = decltype(e);
    // (the side inputs are read from z_data, then u_data; dU goes to du_data)
    if ((E::kSideInputs >= 1 && params.z_data == nullptr) ||
        (E::kSideInputs >= 2 && params.u_data == nullptr) ||
        (E::kSecondOutput && params.du_data == nullptr))
      return hipErrorInvalidValue;
    if (dtype == 1)
      return LaunchTyped<__bf16, E::kMode>(s_kc, d_kc, grouped, params, stream);
    return LaunchTyped<_Float16, E::kMode>(s_kc, d_kc, grouped, params, stream);
  });
}

}  // namespace sputnik_amd
