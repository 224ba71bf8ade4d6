// One part of the LDS-DMA tile configurations (conv_glds.h: ids with id % 6 == 2), compiled as its own
// translation unit so the build runs the parts in parallel.
#include "conv_glds.h"

#if !(SP_GLDS_STAMP || SP_GLDS_ONE_UNIT)
namespace sp {
int launch_glds_part2(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
  return glds_part<2>(a, p, s);
}
}  // namespace sp
#endif
