// wos_selftest.hip -- device probes of the first-ball kernel's stratified sampler
// (wos_selftest_lhs, wos_selftest_lhs_permute, wos_selftest_lhs_plan; include/wos.h).
// The probes call build_lhs, lhs_permute_reg and lhs_permute of wos_device.h themselves, on
// the LDS layout wos_first_ball_kernel gives one wave, so a test can pin every regime of the
// sampler against the oracle's sequential loop without a full solve.  And a probe of the rejection
// sampler's decision functions (wos_selftest_rejection): the edge of each one over every draw a
// stream can produce; and a probe of the
// Green's-function members of the ball (wos_selftest_gfn); and a probe of the source sample
// (wos_selftest_sample_volume): sample_volume_wave under chosen lane masks beside the sequential
// sample_volume.  A translation unit of its own: what a unit instantiates changes its
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

// ---- the SIMD a wave runs on (hw_simd_id, the walk kernel's pinned express placement) ----
// One kBlock-thread block: out[w] the field as the walk kernel reads it, out[kBlock / kWave + w] the whole
// hardware id register, so the field's position can be confirmed on the device.
__global__ __launch_bounds__(kBlock) void wos_simd_id_selftest_kernel(uint32_t* __restrict__ out) {
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    out[w] = hw_simd_id();
    out[kBlock / kWave + w] = __builtin_amdgcn_s_getreg(kHwRegHwId | (31 << 11));
  }
}

hipError_t launch_simd_id_selftest(uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(wos_simd_id_selftest_kernel, dim3(1), dim3(kBlock), 0, s, out);
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

// ---- the Green's-function members of the ball (wos_selftest_gfn) ----------------------------------
// One lane per item: the ball as a solve builds it (init, update_ball), r, yVol and ySurf set as
// sample_volume and the surface sample set them, then every member function as shipped.  The probe
// adds no arithmetic to them.  MODE 0 harmonic, 1 Yukawa reference semantics, 2 the robust kernels'
// instantiation with `robust` set.
template <int DIM, int MODE>
__global__ __launch_bounds__(256) void wos_gfn_selftest_kernel(const float* __restrict__ items, int64_t n,
                                                               float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* it = items + i * WOS_GFN_ITEM;
  float* o = out + i * WOS_GFN_OUT;
  float c[DIM], dir[DIM], x[DIM], y[DIM];
  for (int k = 0; k < DIM; k++) { c[k] = it[3 + k]; dir[k] = it[6 + k]; x[k] = it[9 + k]; y[k] = it[12 + k]; }
  Gfn<DIM, MODE == 2> g;
  g.muR = g.A0 = g.A1 = g.B0 = g.B1 = 0.0f;
  g.init(MODE != 0, it[1]);
  g.update_ball(c, it[0], MODE == 2);
  g.r = it[2];
  for (int k = 0; k < DIM; k++) { g.yVol[k] = g.c[k] + g.r * dir[k]; g.ySurf[k] = g.c[k] + g.R * dir[k]; }
  float res[WOS_GFN_OUT] = {};
  const bool members = g.yukawa == 1 || (g.yukawa == kYukScaled && DIM == 2);
  if (members) { res[0] = g.A0; res[1] = g.A1; res[2] = g.B0; res[3] = g.B1; }
  if (g.yukawa) res[4] = g.muR;
  res[5] = (float)g.yukawa;
  res[6] = g.evaluate();
  res[7] = g.gradient_norm();
  res[8] = g.poisson_kernel();
  res[9] = g.norm();
  g.poisson_kernel_gradient(res + 10);
  res[13] = g.dir_sampled_poisson_kernel(g.yVol);
  res[14] = g.evaluate_xy(x, y);
  if constexpr (DIM == 2 && MODE != 0) {
    if (g.yukawa == 1) {
      // the fused forms, fed as the first-ball kernel feeds them
      double i0, k0, i1, k1;
      bessel_ik<true, true>((double)(g.r * g.sqrtLambda), &i0, &k0, &i1, &k1);
      res[15] = g.evaluate_k0i0(k0, i0);
      res[16] = g.gradient_norm_k1i1(k1, i1);
      // set_ball on the members the point-setup kernel stores (its own update_ball)
      Gfn<2> gp;
      gp.init(true, it[1]);
      gp.update_ball(c, it[0], false);
      const float pb[4] = {gp.A0, gp.A1, gp.B0, gp.B1};
      Gfn<2> gs;
      gs.init(true, it[1]);
      gs.set_ball(c, it[0], pb);
      res[17] = gs.A0; res[18] = gs.A1; res[19] = gs.B0; res[20] = gs.B1; res[21] = gs.muR;
    }
  }
  res[22] = pdf_sphere_uniform<DIM>(g.r);
  g.gradient(res + 23);
  // [26..31] belong to the free-space probe (wos_bvc.hip)
  for (int k = 0; k < 26; k++) o[k] = res[k];
}

hipError_t launch_gfn_selftest(int dim, int mode, const float* items, int64_t n, float* out, hipStream_t s) {
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
#define WOS_GFN_LAUNCH(D, M) hipLaunchKernelGGL((wos_gfn_selftest_kernel<D, M>), grid, blk, 0, s, items, n, out)
  if (dim == 2) {
    if (mode == 0) WOS_GFN_LAUNCH(2, 0); else if (mode == 1) WOS_GFN_LAUNCH(2, 1); else WOS_GFN_LAUNCH(2, 2);
  } else {
    if (mode == 0) WOS_GFN_LAUNCH(3, 0); else if (mode == 1) WOS_GFN_LAUNCH(3, 1); else WOS_GFN_LAUNCH(3, 2);
  }
#undef WOS_GFN_LAUNCH
  return hipGetLastError();
}

// ---- the walk step's geometry queries (wos_selftest_geometry) ------------------------------------
// One workgroup stages the geometry as the walk kernel does; wave w of the grid takes lane mask w,
// its set lanes the next items in order, and every lane calls the wave-cooperative query convergently
// (clear lanes with active / query / want false), as walk_iteration calls it.  Beside it each set lane
// runs the plain sequential scan and the per-lane culled form, and every shortcut next to the exact
// test over every primitive, candidate and group of the scene (the soundness word and the counts).
// The branch tag restates the shipped function's own regime choice from the same wave-uniform values.
namespace {

// the ancestors of group g in tree T accept (ok(box)) -- the tree scans descend through them
template <class Ok>
__device__ __forceinline__ bool geo_tree_path_ok(const DevTree& T, int g, Ok ok) {
  bool all = true;
  for (int L = 1; L <= T.levels; L++) all = all && ok(tree_node(T, L, g >> (3 * L)));
  return all;
}

__device__ __forceinline__ void geo_count(uint32_t* c, bool fired, int slot) { c[slot + (fired ? 0 : 1)]++; }

template <int DIM, bool GG>
__device__ __forceinline__ void geo_ray(const DevScene& sc, const LGeom& G, bool on, const float* it, RayLDS<DIM>* L,
                                        int lane, float* out, int32_t* tag, uint32_t* snd, uint32_t* cnt) {
  constexpr int PS = Layout<DIM>::prim;
  const int np = sc.n_prims, ng = sc.n_pgroups;
  float o[DIM], dir[DIM], tmax = 0.0f;
  for (int k = 0; k < DIM; k++) { o[k] = 0.0f; dir[k] = 1.0f; }
  if (on) {
    for (int k = 0; k < DIM; k++) { o[k] = it[k]; dir[k] = it[DIM + k]; }
    tmax = it[2 * DIM];
  }
  Hit h[3];
  bool f[3] = {false, false, false};
  if (on) {
    f[0] = ray_hit_scan<DIM>(G.prim, np, o, dir, tmax, &h[0]);
    f[1] = ray_hit<DIM>(G, np, ng, o, dir, tmax, &h[1]);
  }
  f[2] = ray_hit_wave<DIM, GG>(G, sc, on, o, dir, tmax, &h[2], L, lane);
  // ray_hit_wave's regime
  const uint64_t nmask = __ballot(on && np > 0);
  const bool tree = GG && sc.ptree.levels > 0, lone = (nmask & (nmask - 1)) == 0;
  const int t = nmask == 0 ? WOS_GEO_RAY_NONE
                : (!tree && np <= (DIM == 2 ? kRayScanMax2 : kRayScanMax3) && !lone) ? WOS_GEO_RAY_LANE_SCAN
                : (!tree && lone) ? WOS_GEO_RAY_SOLO : (tree ? WOS_GEO_RAY_TREE : WOS_GEO_RAY_LIST);
  if (!on) return;
  *tag = t;
  for (int q = 0; q < 3; q++) {
    float* r = out + q * WOS_GEO_OUT;
    r[0] = f[q] ? 1.0f : 0.0f;
    if (f[q]) {
      r[1] = h[q].d;
      for (int k = 0; k < DIM; k++) { r[2 + k] = h[q].p[k]; r[5 + k] = h[q].n[k]; }
    }
  }
  float inv[DIM];
  for (int k = 0; k < DIM; k++) inv[k] = __builtin_amdgcn_rcpf(dir[k]);
  uint32_t s = 0;
  for (int gi = 0; gi < ng; gi++) {
    bool any = false;
    const int p1 = (gi + 1) * kGroup < np ? (gi + 1) * kGroup : np;
    for (int p = gi * kGroup; p < p1; p++) {
      const float* P = G.prim + p * PS;
      float rt = tmax;
      Hit hh;
      const bool exact = ray_prim_exact<DIM>(P, o, dir, rt, &hh);
      const bool pass = ray_prim_prefilter<DIM>(P, o, dir, tmax);
      geo_count(cnt, !pass, WOS_GEO_C_PREFILTER);
      if (!pass && exact) s |= WOS_GEO_S_RAY_PREFILTER;
      any = any || exact;
    }
    const bool maybe = ray_box_maybe<DIM>(G.pgroup + gi * kGroupStride, o, inv, tmax);
    geo_count(cnt, !maybe, WOS_GEO_C_RAY_BOX);
    const bool path = !tree || geo_tree_path_ok(sc.ptree, gi, [&](const float* B) { return ray_box_maybe<DIM>(B, o, inv, tmax); });
    if (any && !(maybe && path)) s |= WOS_GEO_S_RAY_BOX;
  }
  *snd = s;
}

template <int DIM, bool GG>
__device__ __forceinline__ void geo_star(const DevScene& sc, const DevParams& prm, const LGeom& G, bool on,
                                         const float* it, StarLDS<DIM>* L, int lane, float* out, int32_t* tag,
                                         uint32_t* snd, uint32_t* cnt) {
  constexpr int SS = Layout<DIM>::sil;
  const int ns = sc.n_sil, nsg = sc.n_sgroups;
  const float minR = prm.min_star_radius, prec = prm.silhouette_precision;
  float x[DIM], maxR = 0.0f;
  bool flipOrient = false;
  for (int k = 0; k < DIM; k++) x[k] = 0.0f;
  if (on) {
    for (int k = 0; k < DIM; k++) x[k] = it[k];
    maxR = it[DIM];
    flipOrient = it[DIM + 1] != 0.0f;
  }
  const bool flip = !flipOrient;  // computeStarRadius passes !flipNormalOrientation
  const float r2_0 = maxR < kFltMax ? maxR * maxR : kFltMax, minR2 = minR * minR;
  const bool need = on && !(minR > maxR) && sc.n_prims > 0 && !(minR2 >= r2_0);
  // the exact distance and view of candidate s (the sequential loop's own arithmetic)
  const auto cand = [&](int s, float* view) {
    const float* S = G.sil + s * SS;
    if constexpr (DIM == 2) {
      view[0] = x[0] - S[0]; view[1] = x[1] - S[1];
      return __builtin_sqrtf(view[0] * view[0] + view[1] * view[1]);
    } else {
      float pt[3], t;
      const float d = cp_segment<3>(S, S + 3, x, pt, &t);
      for (int k = 0; k < 3; k++) view[k] = x[k] - pt[k];
      return d;
    }
  };
  const auto is_sil = [&](int s, const float* view, float d) {
    const float* S = G.sil + s * SS;
    return (DIM == 2 ? S[6] : S[12]) != 0.0f ? true : is_silhouette<DIM>(S, view, d, flip, prec);
  };
  float r[3] = {0.0f, 0.0f, 0.0f};
  int winner = -1;
  if (on) {
    // computeStarRadius as the oracle runs it: every candidate in index order, no cull
    if (minR > maxR) {
      r[0] = maxR;
    } else {
      r[0] = smax(maxR, minR);
      if (need) {
        float r2 = r2_0, best = 0.0f;
        for (int s = 0; s < ns; s++) {
          float view[DIM];
          const float d = cand(s, view), d2 = d * d;
          if (d2 > r2) continue;
          if (is_sil(s, view, d) && d2 <= r2) {
            r2 = d2; best = d; winner = s;
            if (minR2 >= r2) break;
          }
        }
        if (winner >= 0) r[0] = smax(best, minR);
      }
    }
    r[1] = star_radius<DIM>(G, ns, nsg, sc.n_prims, x, minR, maxR, prec, flipOrient);
  }
  r[2] = star_radius_wave<DIM, GG>(G, sc, prm, on, x, maxR, flipOrient, L, lane);
  // star_radius_wave's regime
  const int cell = (need && G.sgrid != nullptr) ? star_cell<DIM>(sc, x) : -1;
  const bool use_cell = cell >= 0;
  const uint64_t nmask = __ballot(need), cmask = __ballot(use_cell);
  const bool tree = GG && sc.stree.levels > 0, lone = (nmask & (nmask - 1)) == 0;
  int t = !need ? WOS_GEO_STAR_NONE
          : (lone && use_cell) ? WOS_GEO_STAR_SOLO_CELL
          : use_cell ? WOS_GEO_STAR_CELL_LISTS : (tree ? WOS_GEO_STAR_TREE : WOS_GEO_STAR_GROUPS);
  if (need && cmask != 0 && cmask != nmask) t |= WOS_GEO_STAR_MIXED;
  if (!on) return;
  *tag = t;
  for (int q = 0; q < 3; q++) out[q * WOS_GEO_OUT] = r[q];
  if (!need) return;
  uint32_t sd = 0;
  for (int gi = 0; gi < nsg; gi++) {
    bool any = false;
    const int s1 = (gi + 1) * kGroup < ns ? (gi + 1) * kGroup : ns;
    for (int s = gi * kGroup; s < s1; s++) {
      const float* S = G.sil + s * SS;
      float view[DIM];
      const float d = cand(s, view);
      const bool in_ball = d * d <= r2_0, sil = is_sil(s, view, d);
      any = any || (in_ball && sil);
      bool early;
      int cls = 2;
      if constexpr (DIM == 2) {
        const float d2raw = view[0] * view[0] + view[1] * view[1];
        early = d2raw > r2_0 * 1.000001f;
        if (S[6] == 0.0f) {
          cls = silhouette_class2(S, view, d2raw, flip, prec);
          cnt[WOS_GEO_C_CLASS + cls]++;
          if ((cls == 0 && sil) || (cls == 1 && !sil)) sd |= WOS_GEO_S_CLASS2;
        }
      } else {
        float e[3], hl[3];
        for (int k = 0; k < 3; k++) { e[k] = x[k] - 0.5f * (S[k] + S[3 + k]); hl[k] = 0.5f * (S[3 + k] - S[k]); }
        const float dm = __builtin_amdgcn_sqrtf(dotv<3>(e, e)), hr = __builtin_amdgcn_sqrtf(dotv<3>(hl, hl));
        const float lo = dm - hr;
        early = lo > 0.0f && lo * lo > r2_0 * 1.0001f + 1e-6f * dm * dm;
      }
      geo_count(cnt, early, WOS_GEO_C_STAR_EARLY);
      // the early-outs as restated above, and as star_candidate itself applies them: it must not
      // turn down a candidate the exact test accepts (silhouette_class2's 0 is judged above)
      float d2c;
      const bool shipped = star_candidate<DIM>(G, s, x, r2_0, flip, prec, &d2c);
      if ((early && in_ball) || (in_ball && sil && !shipped && cls != 0)) sd |= WOS_GEO_S_STAR_EARLY;
    }
    const float* B = G.sgroup + gi * kSGroupStride;
    const bool maybe = ball_box_maybe<DIM>(B, x, r2_0), culled = cone_culled<DIM>(B, x, prec);
    geo_count(cnt, !maybe, WOS_GEO_C_BALL_BOX);
    geo_count(cnt, culled, WOS_GEO_C_CONE);
    const bool path = !tree || geo_tree_path_ok(sc.stree, gi, [&](const float* N) { return ball_box_maybe<DIM>(N, x, r2_0); });
    if (any && !(maybe && path)) sd |= WOS_GEO_S_BALL_BOX;
    if (any && culled) sd |= WOS_GEO_S_CONE;
  }
  if (use_cell) {
    const uint16_t* off = reinterpret_cast<const uint16_t*>(G.sgrid);
    const uint8_t* lst = reinterpret_cast<const uint8_t*>(G.sgrid + G.sgrid_off_words);
    const int cb = off[cell], ce = off[cell + 1];
    bool held = winner < 0;
    for (int k = cb; k < ce; k++) held = held || (int)lst[k] == winner;
    cnt[WOS_GEO_C_CELL_LEN] = (uint32_t)(ce - cb);
    if (!held) sd |= WOS_GEO_S_STAR_CELL;
  }
  *snd = sd;
}

template <int DIM>
__device__ __forceinline__ void geo_dirichlet(const DevScene& sc, const LGeom& G, bool on, const float* it, int lane,
                                              float* out, int32_t* tag, uint32_t* snd, uint32_t* cnt) {
  constexpr int PS = Layout<DIM>::prim;
  const int nd = sc.n_dprims, ng = sc.n_dgroups;
  float x[DIM];
  for (int k = 0; k < DIM; k++) x[k] = on ? it[k] : 0.0f;
  float d[3] = {0.0f, 0.0f, 0.0f}, proj[2][DIM];
  int winner = -1;
  float wd2 = kFltMax;
  if (on) {
    d[0] = dirichlet_dist_lane<DIM>(sc, x);
    // projectToDirichlet: the same `<=` scan, keeping the closest point
    for (int k = 0; k < DIM; k++) proj[0][k] = proj[1][k] = x[k];
    for (int p = 0; p < nd; p++) {
      float pt[DIM], t0, t1;
      const float dp = cp_prim<DIM>(G.dprim + p * PS, x, pt, &t0, &t1);
      if (dp * dp <= wd2) {
        wd2 = dp * dp; winner = p;
        for (int k = 0; k < DIM; k++) proj[0][k] = pt[k];
      }
    }
    d[1] = dirichlet_dist_culled<DIM, true>(sc, G.dprim, G.dgroup, x, proj[1]);
  }
  dirichlet_dist_step<DIM>(sc, G, on, x, d[2], lane);
  // dirichlet_dist_step's regime
  int t = WOS_GEO_DIR_NONE;
  int cell = -1;
  if (nd > 0) {
    if (DIM == 2 && sc.dgrid != nullptr) {
      int c = 0;
      bool inside = true;
      for (int k = 1; k >= 0 && inside; k--) {
        const int nk = sc.dgrid_n[k];
        const float v = (x[k] - sc.dgrid_min[k]) * sc.dgrid_inv[k];
        if (!(v >= 0.0f && v < (float)nk)) { inside = false; break; }
        int i = (int)v;
        if (i > nk - 1) i = nk - 1;
        c = c * nk + i;
      }
      cell = inside ? c : -1;
      t = inside ? WOS_GEO_DIR_GRID : WOS_GEO_DIR_GRID_MISS;
    } else {
      const uint64_t m = __ballot(on);
      t = (m & (m - 1)) == 0 ? WOS_GEO_DIR_SOLO : (sc.dtree.levels > 0 ? WOS_GEO_DIR_TREE : WOS_GEO_DIR_CULLED);
    }
  }
  if (!on) return;
  *tag = t;
  for (int q = 0; q < 3; q++) out[q * WOS_GEO_OUT] = d[q];
  for (int q = 0; q < 2; q++)
    for (int k = 0; k < DIM; k++) out[q * WOS_GEO_OUT + 1 + k] = proj[q][k];
  if (nd <= 0) return;
  uint32_t s = 0;
  for (int gi = 0; gi < ng; gi++) {
    const float* B = G.dgroup + gi * kGroupStride;
    // the bound lies below the computed distance of every member, so a group the scans skip
    // (bound above the running minimum) never holds the winner
    const float lb = box_dist2<DIM>(B, x);
    const int p1 = (gi + 1) * kGroup < nd ? (gi + 1) * kGroup : nd;
    for (int p = gi * kGroup; p < p1; p++) {
      float pt[DIM], t0, t1;
      const float dp = cp_prim<DIM>(G.dprim + p * PS, x, pt, &t0, &t1);
      bool below = !(lb > dp * dp);
      for (int Lv = 1; Lv <= sc.dtree.levels; Lv++)
        below = below && !(box_dist2<DIM>(tree_node(sc.dtree, Lv, gi >> (3 * Lv)), x) > dp * dp);
      if (!below) s |= WOS_GEO_S_DIR_BOX;
    }
    geo_count(cnt, lb > wd2, WOS_GEO_C_DIR_BOX);
  }
  if (cell >= 0) {
    const uint32_t b = sc.dgrid[cell], e = sc.dgrid[cell + 1];
    const uint16_t* lst = reinterpret_cast<const uint16_t*>(sc.dgrid + sc.dgrid_off_words);
    bool held = false;
    for (uint32_t i = b; i < e; i++) held = held || (int)lst[i] == winner;
    cnt[WOS_GEO_C_CELL_LEN] = e - b;
    if (!held) s |= WOS_GEO_S_DIR_CELL;
  }
  *snd = s;
}

template <int DIM, bool GG, int KIND>
__global__ __launch_bounds__(kBlock) void wos_geometry_selftest_kernel(const DevScene sc, const DevParams prm,
                                                                      const float* __restrict__ items,
                                                                      const unsigned long long* __restrict__ masks,
                                                                      const int32_t* __restrict__ first, int n_masks,
                                                                      int geom_floats, float* __restrict__ out,
                                                                      int32_t* __restrict__ tags,
                                                                      uint32_t* __restrict__ sound,
                                                                      uint32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float probe_smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const LGeom G = stage_geometry<DIM, GG>(sc, probe_smem, true);
  __syncthreads();
  // per-wave scratch shared by the star and ray queries, as the walk kernel lays it out
  const int wave_u = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  char* wscratch = reinterpret_cast<char*>(probe_smem + geom_floats) + wave_u * walk_scratch_bytes<DIM>();
  const int w = (int)blockIdx.x * (kBlock / kWave) + wave_u;
  if (w >= n_masks) return;  // wave-uniform; no block barrier follows
  const unsigned long long mask = masks[w];
  const bool on = ((mask >> lane) & 1ull) != 0;
  const int64_t i = (int64_t)first[w] + __popcll(mask & ((1ull << lane) - 1ull));
  constexpr int IW = KIND == WOS_GEO_RAY ? 2 * DIM + 1 : (KIND == WOS_GEO_STAR ? DIM + 2 : DIM);
  const float* it = items + (on ? i : 0) * IW;
  float res[3 * WOS_GEO_OUT] = {};
  uint32_t cnt[WOS_GEO_COUNTS] = {};
  int32_t tag = 0;
  uint32_t snd = 0;
  if constexpr (KIND == WOS_GEO_RAY)
    geo_ray<DIM, GG>(sc, G, on, it, reinterpret_cast<RayLDS<DIM>*>(wscratch), lane, res, &tag, &snd, cnt);
  else if constexpr (KIND == WOS_GEO_STAR)
    geo_star<DIM, GG>(sc, prm, G, on, it, reinterpret_cast<StarLDS<DIM>*>(wscratch), lane, res, &tag, &snd, cnt);
  else
    geo_dirichlet<DIM>(sc, G, on, it, lane, res, &tag, &snd, cnt);
  if (!on) return;
  for (int k = 0; k < 3 * WOS_GEO_OUT; k++) out[i * 3 * WOS_GEO_OUT + k] = res[k];
  for (int k = 0; k < WOS_GEO_COUNTS; k++) counts[i * WOS_GEO_COUNTS + k] = cnt[k];
  tags[i] = tag;
  sound[i] = snd;
}

template <int DIM, bool GG>
void launch_geometry_kind(int kind, const DevScene& sc, const DevParams& prm, const float* items,
                          const unsigned long long* masks, const int32_t* first, int n_masks, size_t shmem,
                          int geom_floats, float* out, int32_t* tags, uint32_t* sound, uint32_t* counts, hipStream_t s) {
  const dim3 grid((n_masks + kBlock / kWave - 1) / (kBlock / kWave)), blk(kBlock);
  if (kind == WOS_GEO_RAY)
    hipLaunchKernelGGL((wos_geometry_selftest_kernel<DIM, GG, WOS_GEO_RAY>), grid, blk, shmem, s, sc, prm, items, masks,
                       first, n_masks, geom_floats, out, tags, sound, counts);
  else if (kind == WOS_GEO_STAR)
    hipLaunchKernelGGL((wos_geometry_selftest_kernel<DIM, GG, WOS_GEO_STAR>), grid, blk, shmem, s, sc, prm, items, masks,
                       first, n_masks, geom_floats, out, tags, sound, counts);
  else
    hipLaunchKernelGGL((wos_geometry_selftest_kernel<DIM, GG, WOS_GEO_DIRICHLET>), grid, blk, shmem, s, sc, prm, items,
                       masks, first, n_masks, geom_floats, out, tags, sound, counts);
}

}  // namespace

hipError_t launch_geometry_selftest(int dim, int kind, const DevScene& sc, const DevParams& prm, const float* items,
                                    const unsigned long long* masks, const int32_t* first, int n_masks, size_t shmem,
                                    int geom_floats, float* out, int32_t* tags, uint32_t* sound, uint32_t* counts,
                                    hipStream_t s) {
  if (dim == 2 && sc.geom_global)
    launch_geometry_kind<2, true>(kind, sc, prm, items, masks, first, n_masks, shmem, geom_floats, out, tags, sound, counts, s);
  else if (dim == 2)
    launch_geometry_kind<2, false>(kind, sc, prm, items, masks, first, n_masks, shmem, geom_floats, out, tags, sound, counts, s);
  else if (sc.geom_global)
    launch_geometry_kind<3, true>(kind, sc, prm, items, masks, first, n_masks, shmem, geom_floats, out, tags, sound, counts, s);
  else
    launch_geometry_kind<3, false>(kind, sc, prm, items, masks, first, n_masks, shmem, geom_floats, out, tags, sound, counts, s);
  return hipGetLastError();
}

// ---- the source sample (wos_selftest_sample_volume) ----------------------------------------------
// Workgroups of kBlock threads stage the jump constants and the bound table as every kernel that
// samples does (stage_rej_jump) and give each wave a RejLDS; wave w of the grid takes lane mask w, its
// set lanes the next items in order.  Every lane builds a ball as a solve builds it (init,
// update_ball) -- clear lanes a ball that would sample if `active` were not honoured -- and calls
// sample_volume_wave convergently, clear lanes with active false, as walk_iteration and first_balls
// call it.  Beside it each set lane runs the sequential sample_volume from a copy of the same ball
// and stream.  The regime tag restates sample_volume_wave's own choice from the same wave-uniform
// values; the canary words compare what a call had no business touching, bit for bit.
namespace {

template <int DIM, bool RB>
__device__ __forceinline__ bool sv_same_ball(const Gfn<DIM, RB>& a, const Gfn<DIM, RB>& b) {
  bool same = a.yukawa == b.yukawa;
  const auto eq = [](float x, float y) { return __float_as_uint(x) == __float_as_uint(y); };
  for (int k = 0; k < DIM; k++) same = same && eq(a.c[k], b.c[k]) && eq(a.yVol[k], b.yVol[k]) && eq(a.ySurf[k], b.ySurf[k]);
  return same && eq(a.R, b.R) && eq(a.r, b.r) && eq(a.lambda, b.lambda) && eq(a.sqrtLambda, b.sqrtLambda) &&
         eq(a.muR, b.muR) && eq(a.A0, b.A0) && eq(a.A1, b.A1) && eq(a.B0, b.B0) && eq(a.B1, b.B1);
}

template <int DIM, bool RB, bool FB>
__global__ __launch_bounds__(kBlock) void wos_sample_volume_selftest_kernel(
    const DevParams prm, int need_pdf, const float* __restrict__ items, const uint32_t* __restrict__ seeds,
    const unsigned long long* __restrict__ masks, const int32_t* __restrict__ first, int n_masks,
    float* __restrict__ out, unsigned long long* __restrict__ state, uint32_t* __restrict__ iters,
    int32_t* __restrict__ tags, uint32_t* __restrict__ canary) {
  __shared__ RejLDS rej[kBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1);
  stage_rej_jump(prm);
  __syncthreads();
  const int wave_u = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int w = (int)blockIdx.x * (kBlock / kWave) + wave_u;
  if (w >= n_masks) return;  // wave-uniform; no block barrier follows
  const unsigned long long mask = masks[w];
  const bool on = ((mask >> lane) & 1ull) != 0;
  const int64_t i = (int64_t)first[w] + __popcll(mask & ((1ull << lane) - 1ull));
  // clear lanes: a Yukawa ball on the fast path of either dimension, and a live stream
  float R = 0.5f, lam = 50.0f, c[DIM], dir[DIM];
  bool yuk = true;
  uint32_t seed = 0x9E3779B9u + (uint32_t)lane;
  for (int k = 0; k < DIM; k++) { c[k] = 0.25f * (float)(k + 1); dir[k] = k == 0 ? 1.0f : 0.0f; }
  if (on) {
    const float* it = items + i * WOS_SV_ITEM;
    R = it[0]; lam = it[1]; yuk = it[2] != 0.0f; seed = seeds[i];
    for (int k = 0; k < DIM; k++) { c[k] = it[3 + k]; dir[k] = it[6 + k]; }
  }
  Gfn<DIM, RB> g;
  g.muR = g.A0 = g.A1 = g.B0 = g.B1 = 0.0f;
  g.init(yuk, lam);
  g.update_ball(c, R, RB);
  Pcg32 s;
  s.seed((uint64_t)seed);
  const float pdf0 = -1234.5f;  // the canary value of pdf and out
  const Gfn<DIM, RB> g0 = g;
  const Pcg32 s0 = s;

  // the sequential form first, on copies (it shares nothing with the wave form but the staged tables)
  Gfn<DIM, RB> gq = g0;
  Pcg32 sq = s0;
  float pdfq = pdf0, outq[DIM];
  uint32_t itq = 0;
  for (int k = 0; k < DIM; k++) outq[k] = pdf0;
  if (on) sample_volume<DIM>(prm, gq, dir, sq, &pdfq, outq, &itq, need_pdf != 0);

  float pdfw = pdf0, outw[DIM];
  uint32_t itw = 0;
  for (int k = 0; k < DIM; k++) outw[k] = pdf0;
  // a lane publishes its stream in the wave's scratch only when it enters a cooperative generation:
  // the one trace of the regime the function itself leaves (no stream starts at the mark: 2^-64)
  constexpr unsigned long long kUnpublished = 0xFFFFFFFFFFFFFFFFull;
  rej[wave_u].s0[lane] = kUnpublished;
  wave_sync();
  sample_volume_wave<DIM, RB, FB>(prm, on, g, dir, s, &pdfw, outw, &itw, need_pdf != 0, &rej[wave_u], lane);
  wave_sync();
  const bool published = rej[wave_u].s0[lane] != kUnpublished;

  // sample_volume_wave's regime
  const bool coop = on && g0.yukawa && (DIM == 3 ? !g0.scaled() : g0.muR < 80.0f);
  const int nc = __popcll(__ballot(coop));
  const bool dense = WOS_REJ_OWN != 0 && kRejOwnD<DIM, FB> > 0 && nc >= kRejOwnMin;
  const int tag = !coop ? WOS_SV_FALLBACK
                  : nc == 1 ? WOS_SV_SOLO
                  : !dense ? WOS_SV_SPARSE
                  : ((int)itw <= kRejOwnD<DIM, FB> ? WOS_SV_DENSE_OWN : WOS_SV_DENSE_COOP);

  uint32_t cw = 0;
  const bool pdf_same = __float_as_uint(pdfw) == __float_as_uint(pdf0);
  if (!on) {
    if (!sv_same_ball<DIM, RB>(g, g0)) cw |= WOS_SV_CANARY_BALL;
    if (s.state != s0.state) cw |= WOS_SV_CANARY_STREAM;
    if (!pdf_same) cw |= WOS_SV_CANARY_PDF;
    for (int k = 0; k < DIM; k++)
      if (__float_as_uint(outw[k]) != __float_as_uint(pdf0)) cw |= WOS_SV_CANARY_OUT;
    if (itw != 0u) cw |= WOS_SV_CANARY_ITERS;
  } else if (!need_pdf && !pdf_same) {
    cw |= WOS_SV_CANARY_PDF;
  }
  canary[(int64_t)w * kWave + lane] = cw;
  if (!on) return;
  float* o = out + i * 2 * WOS_SV_OUT;
  for (int k = 0; k < 2 * WOS_SV_OUT; k++) o[k] = 0.0f;
  o[0] = g.r; o[1] = pdfw;
  o[WOS_SV_OUT + 0] = gq.r; o[WOS_SV_OUT + 1] = pdfq;
  for (int k = 0; k < DIM; k++) { o[2 + k] = outw[k]; o[WOS_SV_OUT + 2 + k] = outq[k]; }
  state[i * 2 + 0] = s.state; state[i * 2 + 1] = sq.state;
  iters[i * 2 + 0] = itw; iters[i * 2 + 1] = itq;
  tags[i] = tag | (published ? WOS_SV_PUBLISHED : 0);
}

template <int DIM, bool RB, bool FB>
void launch_sample_volume_variant(const DevParams& prm, int need_pdf, const float* items, const uint32_t* seeds,
                                  const unsigned long long* masks, const int32_t* first, int n_masks, float* out,
                                  unsigned long long* state, uint32_t* iters, int32_t* tags, uint32_t* canary,
                                  hipStream_t s) {
  const dim3 grid((n_masks + kBlock / kWave - 1) / (kBlock / kWave)), blk(kBlock);
  hipLaunchKernelGGL((wos_sample_volume_selftest_kernel<DIM, RB, FB>), grid, blk, 0, s, prm, need_pdf, items, seeds,
                     masks, first, n_masks, out, state, iters, tags, canary);
}

}  // namespace

hipError_t launch_sample_volume_selftest(int dim, bool rb, bool fb, const DevParams& prm, int need_pdf,
                                         const float* items, const uint32_t* seeds, const unsigned long long* masks,
                                         const int32_t* first, int n_masks, float* out, unsigned long long* state,
                                         uint32_t* iters, int32_t* tags, uint32_t* canary, hipStream_t s) {
#define WOS_SV_LAUNCH(D, R, F) \
  launch_sample_volume_variant<D, R, F>(prm, need_pdf, items, seeds, masks, first, n_masks, out, state, iters, tags, canary, s)
  if (dim == 2) {
    if (rb) { if (fb) WOS_SV_LAUNCH(2, true, true); else WOS_SV_LAUNCH(2, true, false); }
    else { if (fb) WOS_SV_LAUNCH(2, false, true); else WOS_SV_LAUNCH(2, false, false); }
  } else {
    if (rb) { if (fb) WOS_SV_LAUNCH(3, true, true); else WOS_SV_LAUNCH(3, true, false); }
    else { if (fb) WOS_SV_LAUNCH(3, false, true); else WOS_SV_LAUNCH(3, false, false); }
  }
#undef WOS_SV_LAUNCH
  return hipGetLastError();
}

// the sampler's schedule constants for dim and the first-ball (fb) or walk instantiation
void sample_volume_plan(int dim, bool fb, int32_t* out) {
  out[0] = kWave;
  out[1] = dim == 2 ? kRejBmin<2, false> : (fb ? kRejBmin<3, true> : kRejBmin<3, false>);
  out[2] = kRejBcap;
  out[3] = WOS_REJ_OWN != 0 ? (dim == 2 ? kRejOwnD<2, false> : (fb ? kRejOwnD<3, true> : kRejOwnD<3, false>)) : 0;
  out[4] = kRejOwnMin;
  out[5] = WOS_REJ_JUMP_LDS > 0 ? kRejJumpLds : 0;
  out[6] = kRejMax;
  out[7] = kBlock;
}

}  // namespace wos
