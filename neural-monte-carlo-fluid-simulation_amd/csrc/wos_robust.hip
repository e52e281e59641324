// wos_robust.hip -- the kernel instantiations of the robust float semantics
// (wos_solver_params.robust_float, DevParams::robust): Gfn<DIM, true>, whose Yukawa
// balls with mu R > kRobustMuR use exponentially scaled Bessels instead of the
// reference's float members (which overflow to NaN for 2D mu R > ~92,
// distributions.h:585-587,695; SURVEY.md section 7.2 hard part 4).  A translation unit
// of their own: the reference-semantics kernels (wos_kernel.hip, wos_bvc.hip) are
// compiled without any of this code, and the two sets build in parallel.  The launchers
// of wos_kernel.hip get them through unit_kernels_robust.
#include "wos_device.h"
#include "wos_select.h"

namespace wos {

// This unit's first-ball and walk kernels (wos_select.h).  Robust walks always carry the
// Neumann term and never spread their tails; the last two are the boundary-start walks of
// boundary value caching.
#define UNIT_FIRST_BALLS(X) X(2, true, 1) X(3, true, 1)
#define UNIT_WALKS(X)                      \
  X(2, false, false, true, true, false, 1) \
  X(2, true, false, true, true, false, 1)  \
  X(3, false, false, true, true, false, 1) \
  X(3, true, false, true, true, false, 1)  \
  X(2, false, true, true, true, false, 1)  \
  X(2, true, true, true, true, false, 1)
UNIT_FIRST_BALLS(WOS_FIRST_BALL_INSTANTIATE)
UNIT_WALKS(WOS_WALK_INSTANTIATE)
UnitKernels unit_kernels_robust(const KernelVariant& v) {
  UnitKernels k;
  UNIT_FIRST_BALLS(WOS_FIRST_BALL_SELECT)
  UNIT_WALKS(WOS_WALK_SELECT)
  return k;
}

}  // namespace wos
