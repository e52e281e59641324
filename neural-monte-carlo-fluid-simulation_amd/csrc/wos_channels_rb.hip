// wos_channels_rb.hip -- the multi-channel kernel instantiations (wos_channels.hip) with the
// robust float semantics (wos_robust.hip): Gfn<DIM, true> carrying kMaxChannels source
// channels.  A translation unit of their own, so the one-channel robust kernels are compiled
// exactly as before and the sets build in parallel.  The launchers of wos_kernel.hip get them
// through unit_kernels_channels_rb.
#include "wos_device.h"
#include "wos_select.h"

namespace wos {

constexpr int kNC = kMaxChannels;

// This unit's first-ball and walk kernels (wos_select.h).  Robust walks always carry the
// Neumann term and never spread their tails.
#define UNIT_FIRST_BALLS(X) X(2, true, kNC) X(3, true, kNC)
#define UNIT_WALKS(X)                        \
  X(2, false, false, true, true, false, kNC) \
  X(2, true, false, true, true, false, kNC)  \
  X(3, false, false, true, true, false, kNC) \
  X(3, true, false, true, true, false, kNC)
UNIT_FIRST_BALLS(WOS_FIRST_BALL_INSTANTIATE)
UNIT_WALKS(WOS_WALK_INSTANTIATE)
UnitKernels unit_kernels_channels_rb(const KernelVariant& v) {
  UnitKernels k;
  UNIT_FIRST_BALLS(WOS_FIRST_BALL_SELECT)
  UNIT_WALKS(WOS_WALK_SELECT)
  return k;
}

}  // namespace wos
