// wos_channels.hip -- several source fields on one set of walks (wos_solve_channels):
// the first-ball and walk kernel instantiations that carry kMaxChannels source channels
// (device code in wos_device.h, NC = kMaxChannels), handed to the launchers of wos_kernel.hip
// through unit_kernels_channels, and the kernel that packs the caller's planar source into
// one texel per grid cell.  A translation unit of its
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
#include "wos_select.h"

namespace wos {

constexpr int kNC = kMaxChannels;

// This unit's first-ball and walk kernels (wos_select.h): the variants of wos_kernel.hip
// with kMaxChannels channels.
#define UNIT_FIRST_BALLS(X) X(2, false, kNC) X(3, false, kNC)
#define UNIT_WALKS(X)                          \
  X(2, false, false, false, true, false, kNC)  \
  X(2, false, false, false, false, false, kNC) \
  X(2, true, false, false, true, false, kNC)   \
  X(2, true, false, false, false, false, kNC)  \
  X(2, false, false, false, true, true, kNC)   \
  X(2, false, false, false, false, true, kNC)  \
  X(3, false, false, false, true, false, kNC)  \
  X(3, false, false, false, false, false, kNC) \
  X(3, true, false, false, true, false, kNC)   \
  X(3, true, false, false, false, false, kNC)
UNIT_FIRST_BALLS(WOS_FIRST_BALL_INSTANTIATE)
UNIT_WALKS(WOS_WALK_INSTANTIATE)
UnitKernels unit_kernels_channels(const KernelVariant& v) {
  UnitKernels k;
  UNIT_FIRST_BALLS(WOS_FIRST_BALL_SELECT)
  UNIT_WALKS(WOS_WALK_SELECT)
  return k;
}

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

}  // namespace wos
