// sputnik-amd: the accumulating DSD / DDS kernels, C += op(A) op(B) into a
// C of the operand type or of fp32 (block_gemm.h kOutAccT / kOutAccF32).
// Their own translation unit, so the plain products' instantiations in
// block_gemm.hip are compiled exactly as before. Only what the dispatcher
// launches is instantiated: dense output, CfgSparse (plain or paired) and
// CfgTall; split mode is never used for an accumulating call.
#include "block_gemm.h"

namespace sputnik_amd {
namespace {

template <typename T, bool kSKC, bool kDKC, bool kOutT, class Cfg, int kMode>
hipError_t LaunchCfg(const GemmParams &p, hipStream_t stream) {
  hipLaunchKernelGGL((block_gemm_kernel<T, false, kSKC, kDKC, kOutT, Cfg,
                                        false, false, kMode>),
                     dim3(p.grid > 0 ? p.grid : p.num_tiles),
                     dim3(64 * Cfg::kWaves), 0, stream, p);
  return hipGetLastError();
}

template <typename T, bool kSKC, bool kDKC, bool kOutT>
hipError_t Launch(const GemmParams &p, bool tall, int mode,
                  hipStream_t stream) {
  if (p.num_tiles <= 0) return hipSuccess;
  if (tall) {
    if (mode == kOutAccF32)
      return LaunchCfg<T, kSKC, kDKC, kOutT, CfgTall, kOutAccF32>(p, stream);
    return LaunchCfg<T, kSKC, kDKC, kOutT, CfgTall, kOutAccT>(p, stream);
  }
  if (mode == kOutAccF32)
    return LaunchCfg<T, kSKC, kDKC, kOutT, CfgSparse, kOutAccF32>(p, stream);
  return LaunchCfg<T, kSKC, kDKC, kOutT, CfgSparse, kOutAccT>(p, stream);
}

template <typename T>
hipError_t LaunchTyped(bool s_kc, bool d_kc, bool out_t, bool tall, int mode,
                       const GemmParams &p, hipStream_t stream) {
  const int code = (s_kc ? 4 : 0) | (d_kc ? 2 : 0) | (out_t ? 1 : 0);
  switch (code) {
    case 4: return Launch<T, true, false, false>(p, tall, mode, stream);   // DSD NN
    case 6: return Launch<T, true, true, false>(p, tall, mode, stream);    // DSD NT
    case 0: return Launch<T, false, false, false>(p, tall, mode, stream);  // DSD TN
    case 2: return Launch<T, false, true, false>(p, tall, mode, stream);   // DSD TT
    case 3: return Launch<T, false, true, true>(p, tall, mode, stream);    // DDS NN
    case 7: return Launch<T, true, true, true>(p, tall, mode, stream);     // DDS NT
    case 1: return Launch<T, false, false, true>(p, tall, mode, stream);   // DDS TN
    default: return Launch<T, true, false, true>(p, tall, mode, stream);   // DDS TT
  }
}

}  // namespace

hipError_t LaunchBlockGemmAcc(int dtype, bool s_kc, bool d_kc, bool out_t,
                              bool tall, int out_mode,
                              const GemmParams &params, hipStream_t stream) {
  if (out_mode != kOutAccT && out_mode != kOutAccF32)
    return hipErrorInvalidValue;
  if (params.pair != 0 && params.pair_split > 1) return hipErrorInvalidValue;
  if (dtype == 1)
    return LaunchTyped<__bf16>(s_kc, d_kc, out_t, tall, out_mode, params,
                               stream);
  return LaunchTyped<_Float16>(s_kc, d_kc, out_t, tall, out_mode, params,
                               stream);
}

}  // namespace sputnik_amd
