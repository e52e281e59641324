// wos_selftest.hip -- device probes of the first-ball kernel's stratified sampler
// (wos_selftest_lhs, wos_selftest_lhs_permute, wos_selftest_lhs_plan; include/wos.h).
// The probes call build_lhs, lhs_permute_reg and lhs_permute of wos_device.h themselves, on
// the LDS layout wos_first_ball_kernel gives one wave, so a test can pin every regime of the
// sampler against the oracle's sequential loop without a full solve.  And a probe of the rejection
// sampler's decision functions (wos_selftest_rejection): the edge of each one over every draw a
// stream can produce.  A translation unit of its own: what a unit instantiates changes its
// kernels' inlining and scratch (DESIGN.md "Kernel variants"), and these instantiations must not
// touch the five kernel units.
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

// ---- the rejection sampler's decision functions (wos_selftest_rejection) ------------------------
// The u draws a stream can produce are k 2^-23, k = 0 .. 2^23 - 1 (draw_float).  Every predicate
// below compares u with values that do not depend on u, so over k it is a prefix or a suffix and
// its edge is found by bisection; the shipped functions are called as they stand.
constexpr int kRejDraws = 1 << 23;
enum { kRejEdgeA, kRejEdgeR0, kRejEdgeE, kRejEdgeE3, kRejEdgeQ, kRejEdgeXr, kRejEdges };

// smallest k in [0, 2^23] at which pred(k 2^-23) holds, for a predicate that is false, then true
template <typename Pred>
__device__ __forceinline__ int rej_first_true(Pred pred) {
  int lo = 0, hi = kRejDraws;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pred((float)mid * 0x1p-23f)) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// the predicate once more on either side of its edge: false below, true at it
template <typename Pred>
__device__ __forceinline__ bool rej_edge_holds(Pred pred, int edge) {
  if (edge > 0 && pred((float)(edge - 1) * 0x1p-23f)) return false;
  if (edge < kRejDraws && !pred((float)edge * 0x1p-23f)) return false;
  return true;
}

template <int DIM>
__global__ __launch_bounds__(256) void wos_rejection_selftest_kernel(const DevParams prm, const float* __restrict__ Rs,
                                                                     const float* __restrict__ lams,
                                                                     const float* __restrict__ xs, int64_t n,
                                                                     int32_t* __restrict__ edges,
                                                                     float* __restrict__ vals,
                                                                     int32_t* __restrict__ flags) {
  // the bound table in LDS, as stage_rej_jump stages it for every kernel that samples
  for (int i = threadIdx.x; i < 2 * kRejTabBins; i += blockDim.x) s_rej_tab[i] = prm.rej_tab[i];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float zero[DIM] = {};
  Gfn<DIM> g;
  g.init(true, lams[i]);
  g.update_ball(zero, Rs[i], false);
  // the preamble of sample_volume / sample_volume_wave (wos_device.h), restated
  const float R = g.R, lam = g.lambda, sl = g.sqrtLambda;
  const float a = DIM == 2 ? 2.2f : 2.0f, b = DIM == 2 ? 0.6f : 0.5f;
  const float bound = R <= lam ? smax(smax(a / R, a / lam), smax(b * __builtin_sqrtf(R), b * sl))
                               : smax(smin(a / R, a / lam), smin(b * __builtin_sqrtf(R), b * sl));
  const float nrm = g.norm();
  const float rho = g.A0 / g.A1;
  const float invNB = 1.0f / (nrm * bound);
  const float quick = rej_quick_bound<DIM>(prm, g.R, g.muR, g.sqrtLambda, invNB);
  // the 3D own generation's folded constants (sample_volume_wave, phase A)
  const float xabs = 1e-6f * g.R * invNB;
  const float kz = g.sqrtLambda * -1.44269502f, kb = invNB * 1.001f;
  const float r = xs[i] * R;

  // the callers take the 2D fast test only below mu R = 80
  const bool fast = DIM == 3 || g.muR < 80.0f;
  const auto fast_decide = [&](float u) {
    if (!fast) return -1;
    if constexpr (DIM == 2) return rej_fast_decide(u, r, sl, rho, invNB);
    else return rej_fast_decide3(u, r, sl, rho, invNB);
  };
  const auto not_fast_accept = [&](float u) { return fast_decide(u) != 1; };
  const auto fast_reject = [&](float u) { return fast_decide(u) == 0; };
  // the exact test of sample_volume
  const auto not_exact_accept = [&](float u) {
    g.r = r;
    const float p = g.evaluate() / nrm;
    const float pdfRadius = p / pdf_sphere_uniform<DIM>(g.r);
    return !(u < pdfRadius / bound);
  };
  const auto not_exact3_accept = [&](float u) {
    if constexpr (DIM == 3) return rej_exact_decide3(u, r, g.R, sl, g.A0, g.A1, nrm, bound) != 1;
    else return not_exact_accept(u);
  };
  const auto quick_reject = [&](float u) { return u > quick; };
  const auto x_reject = [&](float u) {
    if constexpr (DIM == 3) return rej_xreject3(u, r, kz, kb, xabs);
    else return false;
  };

  int32_t e[kRejEdges];
  e[kRejEdgeA] = rej_first_true(not_fast_accept);
  e[kRejEdgeR0] = rej_first_true(fast_reject);
  e[kRejEdgeE] = rej_first_true(not_exact_accept);
  e[kRejEdgeE3] = rej_first_true(not_exact3_accept);
  e[kRejEdgeQ] = rej_first_true(quick_reject);
  e[kRejEdgeXr] = rej_first_true(x_reject);
  int32_t f = 0;
  if (!rej_edge_holds(not_fast_accept, e[kRejEdgeA])) f |= 1 << kRejEdgeA;
  if (!rej_edge_holds(fast_reject, e[kRejEdgeR0])) f |= 1 << kRejEdgeR0;
  if (!rej_edge_holds(not_exact_accept, e[kRejEdgeE])) f |= 1 << kRejEdgeE;
  if (!rej_edge_holds(not_exact3_accept, e[kRejEdgeE3])) f |= 1 << kRejEdgeE3;
  if (!rej_edge_holds(quick_reject, e[kRejEdgeQ])) f |= 1 << kRejEdgeQ;
  if (!rej_edge_holds(x_reject, e[kRejEdgeXr])) f |= 1 << kRejEdgeXr;
  for (int k = 0; k < kRejEdges; k++) edges[i * kRejEdges + k] = e[k];
  vals[i * 3 + 0] = nrm;
  vals[i * 3 + 1] = bound;
  vals[i * 3 + 2] = invNB;
  flags[i] = f;
}

hipError_t launch_rejection_selftest(int dim, const float* rej_tab, const float* R, const float* lambda, const float* x,
                                     int64_t n, int32_t* edges, float* vals, int32_t* flags, hipStream_t s) {
  DevParams prm{};
  prm.rej_tab = rej_tab;
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (dim == 2)
    hipLaunchKernelGGL(wos_rejection_selftest_kernel<2>, dim3(grid), dim3(256), 0, s, prm, R, lambda, x, n, edges, vals, flags);
  else
    hipLaunchKernelGGL(wos_rejection_selftest_kernel<3>, dim3(grid), dim3(256), 0, s, prm, R, lambda, x, n, edges, vals, flags);
  return hipGetLastError();
}

}  // namespace wos
