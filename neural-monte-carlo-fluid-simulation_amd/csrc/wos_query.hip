// wos_query.hip -- geometry queries of a scene's boundary meshes (wos_scene_query): per point
// the distance, the signed distance and the closest point of one boundary, and the state word
// a solve would give the point.
//
// wos_point_query_kernel follows the scans of wos_point_setup_kernel (wos_device.h): one point
// per lane, boundaries of up to kSetupLdsFloats record floats staged in LDS, larger ones read
// from global memory through closest_lane's group bounds.  It calls the solve's own
// closest_lane, signed_dist, bbox_far_dist and point_state, so what it reports is what a solve
// decides, by construction; it keeps no histogram, writes no DevTasks and does no Bessel work.
#include "wos_device.h"
#include "wos_launch.h"

namespace wos {

// which: 0 the Neumann boundary, 1 the Dirichlet boundary -- the one dist / sdist / closest
// describe (the host refuses a boundary the scene does not hold).  state (bit 0 estimated,
// bit 1 p masked, bit 2 grad masked as pstate; bit 3 insideDomain, fcpw_scene_loader.h:642-648)
// always takes both boundaries as the solver does: without Dirichlet geometry the bbox
// far-corner distance.  Every output may be null; a boundary no output needs is not scanned.
template <int DIM>
__global__ __launch_bounds__(256) void wos_point_query_kernel(const DevScene sc, int which, float mask,
                                                             const float* __restrict__ pts, int64_t n,
                                                             float* __restrict__ dist, float* __restrict__ sdist,
                                                             float* __restrict__ closest,
                                                             int32_t* __restrict__ state) {
  __shared__ __attribute__((aligned(16))) float s_prim[kSetupLdsFloats];
  constexpr int PS = Layout<DIM>::prim;
  const bool geo = dist != nullptr || sdist != nullptr || closest != nullptr;
  const bool need_n = sc.n_prims > 0 && (state != nullptr || (geo && which == 0));
  const bool need_d = sc.n_dprims > 0 && (state != nullptr || (geo && which == 1));
  // the records of the boundaries in use, each if it still fits.  (The group boxes stay in global
  // memory: every lane reads the same box, a scalar load; staged in LDS beside the records they
  // cost the 957k-point engine grid +41 % for -6 % on 16 384 random points, so they are not:
  // profiles/query_group_lds_ab.txt.)
  const int nfl = need_n ? sc.n_prims * PS : 0, dfl = need_d ? sc.n_dprims * PS : 0;
  const bool lds_n = nfl <= kSetupLdsFloats;
  const int noff = lds_n ? nfl : 0;
  const bool lds_d = noff + dfl <= kSetupLdsFloats;
  if (lds_n)
    for (int k = threadIdx.x; k < nfl; k += blockDim.x) s_prim[k] = sc.prim[k];
  if (lds_d)
    for (int k = threadIdx.x; k < dfl; k += blockDim.x) s_prim[noff + k] = sc.dprim[k];
  __syncthreads();
  const float* nprim = lds_n ? s_prim : sc.prim;
  const float* dprim = lds_d ? s_prim + noff : sc.dprim;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x[DIM];
  for (int k = 0; k < DIM; k++) x[k] = pts[i * DIM + k];
  Closest sel;
  sel.d = kFltMax;
  sel.p[0] = sel.p[1] = sel.p[2] = 0.0f;
  float selSigned = kFltMax;
  float nDist = kFltMax, nSigned = kFltMax;
  if (need_n) {
    const Closest c = closest_lane<DIM>(nprim, sc.pgroup, sc.n_prims, sc.n_pgroups, x);
    nDist = c.d;
    nSigned = signed_dist<DIM>(sc.paux, c, x);
    if (which == 0) { sel = c; selSigned = nSigned; }
  }
  float dDist, dSigned;
  if (need_d) {
    const Closest c = closest_lane<DIM>(dprim, sc.dgroup, sc.n_dprims, sc.n_dgroups, x);
    dDist = c.d;
    dSigned = signed_dist<DIM>(sc.dpaux, c, x);
    if (which == 1) { sel = c; selSigned = dSigned; }
  } else {
    dDist = dSigned = bbox_far_dist<DIM>(sc, x);
  }
  if (dist) dist[i] = sel.d;
  if (sdist) sdist[i] = selSigned;
  if (closest)
    for (int k = 0; k < DIM; k++) closest[i * DIM + k] = sel.p[k];
  if (state) {
    DevParams prm{};
    prm.boundary_distance_mask = mask;
    int bucket;
    float firstR;
    const int32_t ps = point_state<DIM>(sc, prm, nDist, nSigned, dDist, dSigned, &bucket, &firstR);
    // insideDomain from point_state itself, not a copy of its rule: single-sided and without
    // force_estimate (prm's is 0) its "estimated" bit is exactly `inside`
    DevScene one = sc;
    one.double_sided = 0;
    const int32_t in = point_state<DIM>(one, prm, nDist, nSigned, dDist, dSigned, &bucket, &firstR) & kPtEstimate;
    state[i] = (ps & (kPtEstimate | kPtMaskP | kPtMaskG)) | (in ? 8 : 0);
  }
}

hipError_t launch_point_query(int dim, const DevScene& sc, int which, float mask, const float* pts, int64_t n,
                              float* dist, float* sdist, float* closest, int32_t* state, hipStream_t s) {
  const int64_t grid = (n + 255) / 256;
  if (grid < 1) return hipSuccess;
  if (dim == 2)
    hipLaunchKernelGGL(wos_point_query_kernel<2>, dim3((unsigned)grid), dim3(256), 0, s, sc, which, mask, pts, n, dist,
                       sdist, closest, state);
  else
    hipLaunchKernelGGL(wos_point_query_kernel<3>, dim3((unsigned)grid), dim3(256), 0, s, sc, which, mask, pts, n, dist,
                       sdist, closest, state);
  return hipGetLastError();
}

}  // namespace wos
