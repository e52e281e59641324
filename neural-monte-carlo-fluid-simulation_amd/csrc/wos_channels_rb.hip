// wos_channels_rb.hip -- the multi-channel kernel instantiations (wos_channels.hip) with the
// robust float semantics (wos_robust.hip): Gfn<DIM, true> carrying kMaxChannels source
// channels.  A translation unit of their own, so the one-channel robust kernels are compiled
// exactly as before and the sets build in parallel.
#include "wos_device.h"
#include "wos_launch.h"

namespace wos {

constexpr int kNC = kMaxChannels;

template __global__ void wos_first_ball_kernel<2, true, kNC>(const DevScene, const DevParams, const float*, int64_t,
                                                             int64_t, int64_t, const DevTasks, unsigned long long*,
                                                             unsigned int*, int);
template __global__ void wos_first_ball_kernel<3, true, kNC>(const DevScene, const DevParams, const float*, int64_t,
                                                             int64_t, int64_t, const DevTasks, unsigned long long*,
                                                             unsigned int*, int);
#define WOS_RB_WALK_MC(D, G)                                                                                       \
  template __global__ void wos_walk_kernel<D, G, false, true, true, false, kNC>(const DevScene, const DevParams,   \
                                                                                const DevTasks, int64_t, int64_t, \
                                                                                unsigned long long*, unsigned int*, int)
WOS_RB_WALK_MC(2, false);
WOS_RB_WALK_MC(2, true);
WOS_RB_WALK_MC(3, false);
WOS_RB_WALK_MC(3, true);
#undef WOS_RB_WALK_MC

hipError_t launch_first_balls_rb_mc(int dim, const DevScene& sc, const DevParams& prm, const float* pts, int64_t n,
                                    int64_t base, int64_t stride, const DevTasks& tk, unsigned long long* counters,
                                    unsigned int* work, int grid, size_t shmem, int lhs_floats, hipStream_t s) {
  if (dim == 2)
    hipLaunchKernelGGL((wos_first_ball_kernel<2, true, kNC>), dim3(grid), dim3(kBlock), shmem, s, sc, prm, pts, n, base,
                       stride, tk, counters, work, lhs_floats);
  else
    hipLaunchKernelGGL((wos_first_ball_kernel<3, true, kNC>), dim3(grid), dim3(kBlock), shmem, s, sc, prm, pts, n, base,
                       stride, tk, counters, work, lhs_floats);
  return hipGetLastError();
}

hipError_t launch_walks_rb_mc(int dim, const DevScene& sc, const DevParams& prm, const DevTasks& tk, int64_t base,
                              int64_t stride, unsigned long long* counters, unsigned int* tqueue, int grid,
                              size_t shmem, int geom_floats, hipStream_t s) {
#define WOS_LAUNCH_WALK(D, G)                                                                                     \
  hipLaunchKernelGGL((wos_walk_kernel<D, G, false, true, true, false, kNC>), dim3(grid), dim3(kBlock), shmem, s, sc, \
                     prm, tk, base, stride, counters, tqueue, geom_floats)
  if (dim == 2) {
    if (sc.geom_global) WOS_LAUNCH_WALK(2, true); else WOS_LAUNCH_WALK(2, false);
  } else {
    if (sc.geom_global) WOS_LAUNCH_WALK(3, true); else WOS_LAUNCH_WALK(3, false);
  }
#undef WOS_LAUNCH_WALK
  return hipGetLastError();
}

hipError_t occupancy_rb_mc(int which, int dim, bool geom_global, size_t shmem, int* blocks) {
#define WOS_OCC(K) hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, K, kBlock, shmem)
  if (which == 0)
    return dim == 2 ? WOS_OCC((wos_first_ball_kernel<2, true, kNC>)) : WOS_OCC((wos_first_ball_kernel<3, true, kNC>));
  if (dim == 2)
    return geom_global ? WOS_OCC((wos_walk_kernel<2, true, false, true, true, false, kNC>))
                       : WOS_OCC((wos_walk_kernel<2, false, false, true, true, false, kNC>));
  return geom_global ? WOS_OCC((wos_walk_kernel<3, true, false, true, true, false, kNC>))
                     : WOS_OCC((wos_walk_kernel<3, false, false, true, true, false, kNC>));
#undef WOS_OCC
}

}  // namespace wos
