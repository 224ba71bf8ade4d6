// LDS-DMA implicit-GEMM kernels on bf16-operand MFMA (x3 split / bf16): the launcher of the plan's LDS-DMA
// tiles (SP_GLDS_CONFIGS, conv_plan.h). The kernels live in conv_glds.h and are instantiated across
// conv_glds_p<k>.hip; a diagnostic build (tools/build_diag.sh: -DSP_GLDS_ONE_UNIT plus -DSP_GLDS_STAMP or
// -DSP_ABLATE=n) instantiates them all here instead.
#include "conv_glds.h"

namespace sp {

#if !(SP_GLDS_STAMP || SP_GLDS_ONE_UNIT)
int launch_glds_part0(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
int launch_glds_part1(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
int launch_glds_part2(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
int launch_glds_part3(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
int launch_glds_part4(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
int launch_glds_part5(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
#endif
static_assert(kGldsParts == 6, "one conv_glds_p<k>.hip per part");

int launch_glds(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
  switch (p.tile % kGldsParts) {
#if SP_GLDS_STAMP || SP_GLDS_ONE_UNIT
    case 0: return glds_part<0>(a, p, s);
    case 1: return glds_part<1>(a, p, s);
    case 2: return glds_part<2>(a, p, s);
    case 3: return glds_part<3>(a, p, s);
    case 4: return glds_part<4>(a, p, s);
    default: return glds_part<5>(a, p, s);
#else
    case 0: return launch_glds_part0(a, p, s);
    case 1: return launch_glds_part1(a, p, s);
    case 2: return launch_glds_part2(a, p, s);
    case 3: return launch_glds_part3(a, p, s);
    case 4: return launch_glds_part4(a, p, s);
    default: return launch_glds_part5(a, p, s);
#endif
  }
}

}  // namespace sp

#if SP_GLDS_STAMP
extern "C" int sp_debug_glds_stamps(void* dst) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(sp::g_glds_stamps), sizeof(sp::g_glds_stamps));
}
#endif
