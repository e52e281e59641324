// wos_channels.hip -- several source fields on one set of walks (wos_solve_channels):
// the first-ball and walk kernel instantiations that carry kMaxChannels source channels
// (device code in wos_device.h, NC = kMaxChannels), their launchers, and the kernel that
// packs the caller's planar source into one texel per grid cell.  A translation unit of its
// own: the one-channel kernels (wos_kernel.hip) are compiled exactly as before, and the two
// sets build in parallel.  Robust float semantics: wos_channels_rb.hip.
//
// A walk never looks at the source: radii, directions, the rejection-sampled source point,
// throughput, roulette and the recorded / dropped decision depend on geometry, lambda and
// the RNG key alone.  So the channels share every walk, and each channel repeats the scalar
// code's float operations on its own texel -- channel c is bit for bit the one-channel solve
// of source c.
#include "wos_device.h"
#include "wos_launch.h"

namespace wos {

constexpr int kNC = kMaxChannels;

template __global__ void wos_first_ball_kernel<2, false, kNC>(const DevScene, const DevParams, const float*, int64_t,
                                                              int64_t, int64_t, const DevTasks, unsigned long long*,
                                                              unsigned int*, int);
template __global__ void wos_first_ball_kernel<3, false, kNC>(const DevScene, const DevParams, const float*, int64_t,
                                                              int64_t, int64_t, const DevTasks, unsigned long long*,
                                                              unsigned int*, int);
// walk kernels <DIM, GG, BSTART = false, RB = false, NEU, SPR, NC>: the variants of wos_kernel.hip
#define WOS_WALK_MC(D, G, N, S)                                                                         \
  template __global__ void wos_walk_kernel<D, G, false, false, N, S, kNC>(const DevScene, const DevParams, \
                                                                          const DevTasks, int64_t, int64_t, \
                                                                          unsigned long long*, unsigned int*, int)
WOS_WALK_MC(2, false, true, false);
WOS_WALK_MC(2, false, false, false);
WOS_WALK_MC(2, true, true, false);
WOS_WALK_MC(2, true, false, false);
WOS_WALK_MC(2, false, true, true);
WOS_WALK_MC(2, false, false, true);
WOS_WALK_MC(3, false, true, false);
WOS_WALK_MC(3, false, false, false);
WOS_WALK_MC(3, true, true, false);
WOS_WALK_MC(3, true, false, false);
#undef WOS_WALK_MC

// One thread per grid cell: the cell's texel [kMaxChannels], channels beyond `channels` +0.
// Reads are coalesced per channel plane, the write is one 16-byte store.
__global__ __launch_bounds__(256) void wos_source_pack_kernel(const float* __restrict__ planar,
                                                              float4* __restrict__ texels, int64_t cells,
                                                              int channels) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cells) return;
  float v[kNC];
  for (int c = 0; c < kNC; c++) v[c] = c < channels ? planar[(int64_t)c * cells + i] : 0.0f;
  texels[i] = make_float4(v[0], v[1], v[2], v[3]);
}

hipError_t launch_source_pack(const float* planar, float* texels, int64_t cells, int channels, hipStream_t s) {
  if (cells < 1) return hipSuccess;
  if (channels < 1 || channels > kNC) return hipErrorInvalidValue;
  const int64_t grid = (cells + 255) / 256;
  if (grid > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wos_source_pack_kernel, dim3((unsigned)grid), dim3(256), 0, s, planar,
                     reinterpret_cast<float4*>(texels), cells, channels);
  return hipGetLastError();
}

hipError_t launch_first_balls_mc(int dim, const DevScene& sc, const DevParams& prm, const float* pts, int64_t n,
                                 int64_t base, int64_t stride, const DevTasks& tk, unsigned long long* counters,
                                 unsigned int* work, int grid, size_t shmem, int lhs_floats, hipStream_t s) {
  if (dim == 2)
    hipLaunchKernelGGL((wos_first_ball_kernel<2, false, kNC>), dim3(grid), dim3(kBlock), shmem, s, sc, prm, pts, n,
                       base, stride, tk, counters, work, lhs_floats);
  else
    hipLaunchKernelGGL((wos_first_ball_kernel<3, false, kNC>), dim3(grid), dim3(kBlock), shmem, s, sc, prm, pts, n,
                       base, stride, tk, counters, work, lhs_floats);
  return hipGetLastError();
}

// the dispatch of launch_walks (wos_kernel.hip), variant for variant
hipError_t launch_walks_mc(int dim, const DevScene& sc, const DevParams& prm, const DevTasks& tk, int64_t base,
                           int64_t stride, unsigned long long* counters, unsigned int* tqueue, int grid, size_t shmem,
                           int geom_floats, hipStream_t s) {
#define WOS_LAUNCH_WALK(D, G, N, S)                                                                               \
  hipLaunchKernelGGL((wos_walk_kernel<D, G, false, false, N, S, kNC>), dim3(grid), dim3(kBlock), shmem, s, sc, prm, \
                     tk, base, stride, counters, tqueue, geom_floats)
  const bool inert = prm.neumann_inert != 0;
  if (dim == 2) {
    if (sc.geom_global) {
      if (inert) WOS_LAUNCH_WALK(2, true, false, false); else WOS_LAUNCH_WALK(2, true, true, false);
    } else if (prm.tail_spread) {
      if (inert) WOS_LAUNCH_WALK(2, false, false, true); else WOS_LAUNCH_WALK(2, false, true, true);
    } else {
      if (inert) WOS_LAUNCH_WALK(2, false, false, false); else WOS_LAUNCH_WALK(2, false, true, false);
    }
  } else if (sc.geom_global) {
    if (inert) WOS_LAUNCH_WALK(3, true, false, false); else WOS_LAUNCH_WALK(3, true, true, false);
  } else {
    if (inert) WOS_LAUNCH_WALK(3, false, false, false); else WOS_LAUNCH_WALK(3, false, true, false);
  }
#undef WOS_LAUNCH_WALK
  return hipGetLastError();
}

hipError_t occupancy_first_ball_mc(int dim, size_t shmem, int* blocks) {
  return dim == 2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, wos_first_ball_kernel<2, false, kNC>, kBlock, shmem)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, wos_first_ball_kernel<3, false, kNC>, kBlock, shmem);
}

hipError_t occupancy_walk_mc(int dim, bool geom_global, const DevParams& prm, size_t shmem, int* blocks) {
#define WOS_OCC(D, G, N, S) \
  hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, (wos_walk_kernel<D, G, false, false, N, S, kNC>), kBlock, shmem)
  const bool inert = prm.neumann_inert != 0;
  if (dim == 2) {
    if (geom_global) return inert ? WOS_OCC(2, true, false, false) : WOS_OCC(2, true, true, false);
    if (prm.tail_spread) return inert ? WOS_OCC(2, false, false, true) : WOS_OCC(2, false, true, true);
    return inert ? WOS_OCC(2, false, false, false) : WOS_OCC(2, false, true, false);
  }
  if (geom_global) return inert ? WOS_OCC(3, true, false, false) : WOS_OCC(3, true, true, false);
  return inert ? WOS_OCC(3, false, false, false) : WOS_OCC(3, false, true, false);
#undef WOS_OCC
}

}  // namespace wos
