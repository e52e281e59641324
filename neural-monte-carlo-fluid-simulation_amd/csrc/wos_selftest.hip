// wos_selftest.hip -- device probes of the first-ball kernel's stratified sampler
// (wos_selftest_lhs, wos_selftest_lhs_permute, wos_selftest_lhs_plan; include/wos.h).
// The probes call build_lhs, lhs_permute_reg and lhs_permute of wos_device.h themselves, on
// the LDS layout wos_first_ball_kernel gives one wave, so a test can pin every regime of the
// sampler against the oracle's sequential loop without a full solve.  A translation unit of
// its own: what a unit instantiates changes its kernels' inlining and scratch (DESIGN.md
// "Kernel variants"), and these instantiations must not touch the five kernel units.
#include "wos_device.h"
#include "wos_launch.h"
#include "../../include/wos.h"

namespace wos {

// One wave per block; block b builds the stratified samples of indices b P .. b P + P - 1
// (P = fb_points_per_wave) in the P slots of the wave's LDS region, as the first-ball kernel
// does for one pack of points: per slot and dimension, or -- when lhs_all_fits -- every slot's
// partners first and one lhs_permute_reg pass over all of them.
template <int DIM>
__global__ __launch_bounds__(kWave) void wos_lhs_selftest_kernel(const DevParams prm, const long long* __restrict__ gidx,
                                                                 int n, int lhs_floats, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float probe_smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int npairs = prm.n_pairs, nstrat = 2 * npairs, nd = nstrat * (DIM - 1);
  const int P = fb_points_per_wave(npairs);
  const int wave_floats = 2 * P * lhs_floats + (int)(fb_union_bytes(P * lhs_floats, nstrat) / sizeof(float));
  float* wbase = probe_smem;
  unsigned long long* ljump = reinterpret_cast<unsigned long long*>(probe_smem + wave_floats);
  for (int i = threadIdx.x; i < 2 * prm.lhs_jump_n; i += blockDim.x) ljump[i] = prm.jump[i];
  __syncthreads();
  char* scratch = reinterpret_cast<char*>(wbase + 2 * P * lhs_floats);
  const int first = (int)blockIdx.x * P;
  const int cnt = n - first < P ? n - first : P;
  const bool all = lhs_all_fits(npairs, DIM, P);
  for (int s = 0; s < cnt; s++) {
    float* strat_s = wbase + 2 * s * lhs_floats;
    build_lhs<DIM>(prm, ljump, (int64_t)gidx[first + s], strat_s, reinterpret_cast<int*>(strat_s + lhs_floats), scratch,
                   lane, !all);
  }
  if constexpr (DIM == 3)
    if (all) {
      const int* part0 = reinterpret_cast<const int*>(wbase + lhs_floats);
      if (nstrat <= kWave) lhs_permute_reg<DIM - 1, 1, 4>(wbase, part0, 2 * lhs_floats, 0, cnt * (DIM - 1), nstrat, lane);
      else lhs_permute_reg<DIM - 1, 2, 2>(wbase, part0, 2 * lhs_floats, 0, cnt * (DIM - 1), nstrat, lane);
    }
  wave_sync();
  for (int s = 0; s < cnt; s++) {
    const float* strat_s = wbase + 2 * s * lhs_floats;
    for (int k = lane; k < nd; k += kWave) out[(int64_t)(first + s) * nd + k] = strat_s[k];
  }
}

// One wave per block; block b runs implementation impl on table b: `cap` slots of values
// [nstrat][sd] and partners [sd][nstrat], laid out in LDS as the first-ball kernel lays out a
// wave's slots (samples, then partners, 2 lhs_floats per slot; the shuffle scratch after them).
// Every slot is written back, shuffled or not.
__global__ __launch_bounds__(kWave) void wos_lhs_permute_selftest_kernel(int impl, const int* __restrict__ partner,
                                                                         const float* __restrict__ values, int nstrat,
                                                                         int sd, int slots, int cap,
                                                                         float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float probe_smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int nd = nstrat * sd, lhs_floats = (nd + 3) & ~3;
  float* wbase = probe_smem;
  char* scratch = reinterpret_cast<char*>(wbase + 2 * cap * lhs_floats);
  const int64_t t0 = (int64_t)blockIdx.x * cap * nd;
  for (int s = 0; s < cap; s++) {
    float* strat_s = wbase + 2 * s * lhs_floats;
    int* part_s = reinterpret_cast<int*>(strat_s + lhs_floats);
    for (int k = lane; k < nd; k += kWave) {
      strat_s[k] = values[t0 + (int64_t)s * nd + k];
      part_s[k] = partner[t0 + (int64_t)s * nd + k];
    }
  }
  wave_sync();
  const int* part0 = reinterpret_cast<const int*>(wbase + lhs_floats);
  switch (impl) {
    case WOS_LHS_REG1:
      for (int i = 0; i < sd; ++i) {
        if (sd == 1) lhs_permute_reg<1, 1, 1>(wbase, part0, 0, i, 1, nstrat, lane);
        else lhs_permute_reg<2, 1, 1>(wbase, part0, 0, i, 1, nstrat, lane);
      }
      break;
    case WOS_LHS_REG2:
      for (int i = 0; i < sd; ++i) {
        if (sd == 1) lhs_permute_reg<1, 2, 1>(wbase, part0, 0, i, 1, nstrat, lane);
        else lhs_permute_reg<2, 2, 1>(wbase, part0, 0, i, 1, nstrat, lane);
      }
      break;
    case WOS_LHS_LDS:
      for (int i = 0; i < sd; ++i) lhs_permute(wbase, part0, nstrat, sd, i, scratch, lane);
      break;
    case WOS_LHS_PACK_R1:
      lhs_permute_reg<2, 1, 4>(wbase, part0, 2 * lhs_floats, 0, slots * 2, nstrat, lane);
      break;
    case WOS_LHS_PACK_R2:
      lhs_permute_reg<2, 2, 2>(wbase, part0, 2 * lhs_floats, 0, slots * 2, nstrat, lane);
      break;
    default:
      break;
  }
  wave_sync();
  for (int s = 0; s < cap; s++) {
    const float* strat_s = wbase + 2 * s * lhs_floats;
    for (int k = lane; k < nd; k += kWave) out[t0 + (int64_t)s * nd + k] = strat_s[k];
  }
}

size_t lhs_selftest_lds_bytes(int n_pairs, int dim, int jump_n) {
  const int lhs_floats = ((2 * n_pairs * (dim - 1)) + 3) & ~3;
  const int P = fb_points_per_wave(n_pairs);
  return (size_t)2 * P * lhs_floats * sizeof(float) + fb_union_bytes(P * lhs_floats, 2 * n_pairs) +
         (size_t)jump_n * 2 * sizeof(unsigned long long);
}

hipError_t launch_lhs_selftest(int dim, const DevParams& prm, const long long* gidx, int n, float* out, hipStream_t s) {
  const int lhs_floats = ((2 * prm.n_pairs * (dim - 1)) + 3) & ~3;
  const int P = fb_points_per_wave(prm.n_pairs);
  const int grid = (n + P - 1) / P;
  const size_t shmem = lhs_selftest_lds_bytes(prm.n_pairs, dim, prm.lhs_jump_n);
  if (dim == 2)
    hipLaunchKernelGGL(wos_lhs_selftest_kernel<2>, dim3(grid), dim3(kWave), shmem, s, prm, gidx, n, lhs_floats, out);
  else
    hipLaunchKernelGGL(wos_lhs_selftest_kernel<3>, dim3(grid), dim3(kWave), shmem, s, prm, gidx, n, lhs_floats, out);
  return hipGetLastError();
}

int lhs_permute_selftest_slots(int impl) { return impl == WOS_LHS_PACK_R1 ? 2 : 1; }

int lhs_permute_selftest_max_strata(int impl) {
  switch (impl) {
    case WOS_LHS_REG1: case WOS_LHS_PACK_R1: return kWave;
    case WOS_LHS_REG2: case WOS_LHS_PACK_R2: return 2 * kWave;
    case WOS_LHS_LDS: return 4 * kWave;
    default: return 0;
  }
}

hipError_t launch_lhs_permute_selftest(int impl, const int* partner, const float* values, int nstrat, int sd, int slots,
                                       int count, float* out, hipStream_t s) {
  const int cap = lhs_permute_selftest_slots(impl);
  const int lhs_floats = (nstrat * sd + 3) & ~3;
  // the slots, then lhs_permute's scratch as fb_union_bytes sizes it for a one-point wave
  const size_t shmem = (size_t)2 * cap * lhs_floats * sizeof(float) + (size_t)28 * lhs_floats + 64;
  hipLaunchKernelGGL(wos_lhs_permute_selftest_kernel, dim3(count), dim3(kWave), shmem, s, impl, partner, values, nstrat,
                     sd, slots, cap, out);
  return hipGetLastError();
}

// the sampler's schedule for n_pairs and dim, from the constants the kernels are built with
void lhs_plan(int n_pairs, int dim, int32_t* out) {
  const int nstrat = 2 * n_pairs, P = fb_points_per_wave(n_pairs);
  const int lhs_floats = ((nstrat * (dim - 1)) + 3) & ~3;
  const int draws = 2 * nstrat * (dim - 1);
  out[0] = P;
  out[1] = lhs_all_fits(n_pairs, dim, P) ? 1 : 0;
  out[2] = nstrat <= kWave ? WOS_LHS_REG1 : (nstrat <= 2 * kWave ? WOS_LHS_REG2 : (nstrat <= 4 * kWave ? WOS_LHS_LDS : WOS_LHS_SERIAL));
  out[3] = P > 1 ? 1 : (n_pairs + kWave - 1) / kWave;
  out[4] = draws <= kLhsJumpMax ? 0 : 1;
  out[5] = (int32_t)((size_t)2 * P * lhs_floats * sizeof(float) + fb_union_bytes(P * lhs_floats, nstrat));
  out[6] = 0;  // the LDS budget: the caller's (wos_capi.h kLdsDynamicMax)  
  out[7] = (int32_t)kPtGrab;
  out[8] = nstrat <= 4 * kWave ? (nstrat + kWave - 1) / kWave : 0;
}

}  // namespace wos
