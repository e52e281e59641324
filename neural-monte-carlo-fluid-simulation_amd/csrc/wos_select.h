// wos_select.h -- from a KernelVariant (wos_variant.h) to the kernel itself.  For the
// translation units that instantiate wos_first_ball_kernel and wos_walk_kernel only.
//
// A unit writes the template arguments of its instantiations once, as lists
//   #define UNIT_FIRST_BALLS(X) X(2, false, 1) X(3, false, 1)
//   #define UNIT_WALKS(X) X(2, false, false, false, true, false, 1) ...
// and applies two macros to them: *_INSTANTIATE is the explicit instantiation (in the
// list's order, which is the order of the kernels in the code object), *_SELECT the line
// of the unit's exported unit_kernels_* function that hands the kernel out for its
// variant.  launch_first_balls, launch_walks and occupancy_blocks_per_cu (wos_kernel.hip)
// launch and query through the pointer the owning unit returns, so the occupancy is
// always that of the kernel launched.
#pragma once
#include "wos_device.h"
#include "wos_variant.h"

namespace wos {

// every instantiation of a kernel has the same signature
#define WOS_FIRST_BALL_PARAMS \
  const DevScene, const DevParams, const float*, int64_t, int64_t, int64_t, const DevTasks, unsigned long long*, \
      unsigned int*, int
#define WOS_WALK_PARAMS \
  const DevScene, const DevParams, const DevTasks, int64_t, int64_t, unsigned long long*, unsigned int*, int
using FirstBallKernel = void (*)(WOS_FIRST_BALL_PARAMS);
using WalkKernel = void (*)(WOS_WALK_PARAMS);

// a unit's kernels for a variant; null: not this unit's (or no such kernel)
struct UnitKernels {
  FirstBallKernel first_ball = nullptr;
  WalkKernel walk = nullptr;
};
UnitKernels unit_kernels_plain(const KernelVariant& v);        // wos_kernel.hip
UnitKernels unit_kernels_channels(const KernelVariant& v);     // wos_channels.hip
UnitKernels unit_kernels_robust(const KernelVariant& v);       // wos_robust.hip
UnitKernels unit_kernels_channels_rb(const KernelVariant& v);  // wos_channels_rb.hip
UnitKernels unit_kernels_bstart(const KernelVariant& v);       // wos_bvc.hip

// X(DIM, RB, NC): wos_first_ball_kernel<DIM, RB, NC> (boundary-start walks have no first balls)
#define WOS_FIRST_BALL_INSTANTIATE(D, R, C) \
  template __global__ void wos_first_ball_kernel<D, R, C>(WOS_FIRST_BALL_PARAMS);
#define WOS_FIRST_BALL_SELECT(D, R, C) \
  if (v.valid && !v.bstart && v.dim == D && v.robust == R && v.channels == C) k.first_ball = wos_first_ball_kernel<D, R, C>;

// X(DIM, GG, BSTART, RB, NEU, SPR, NC): wos_walk_kernel<DIM, GG, BSTART, RB, NEU, SPR, NC>
#define WOS_WALK_INSTANTIATE(D, G, B, R, N, S, C) \
  template __global__ void wos_walk_kernel<D, G, B, R, N, S, C>(WOS_WALK_PARAMS);
#define WOS_WALK_SELECT(D, G, B, R, N, S, C)                                                                  \
  if (v.valid && v.dim == D && v.geom_global == G && v.bstart == B && v.robust == R && v.neumann == N && \
      v.spread == S && v.channels == C)                                                                       \
    k.walk = wos_walk_kernel<D, G, B, R, N, S, C>;

}  // namespace wos
