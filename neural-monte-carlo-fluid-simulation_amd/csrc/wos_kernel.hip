// wos_kernel.hip -- gfx950 walk-on-stars solve: the kernel instantiations and their
// host launchers (device code in wos_device.h).
//
// One projection = wos_point_setup_kernel, the walk-queue order (wos_lpt_scatter_kernel),
// wos_first_ball_kernel, the persistent wos_walk_kernel and wos_fold_kernel (statistics
// + masked outputs), all on the caller's stream.
//
// The first-ball and walk kernels are instantiated in five translation units (this one:
// one channel, reference float semantics; wos_channels.hip, wos_robust.hip,
// wos_channels_rb.hip, wos_bvc.hip).  Which one a solve runs is a KernelVariant
// (wos_variant.h); launch_first_balls, launch_walks and occupancy_blocks_per_cu here ask
// the units for its kernel (wos_select.h) and launch or query through that pointer.
#include "wos_device.h"
#include <algorithm>
#include "wos_launch.h"
#include "wos_select.h"

namespace wos {

// ---- walk-queue order: the permutation, buckets in descending cost order ----
// One launch: every block derives the bucket offsets from the final counts
// hist[0, kCostBuckets) itself (exclusive sums in descending bucket order), counts its
// points per bucket in LDS, reserves one range per bucket with an atomic on the fill
// cursors hist[kCostBuckets + b] (zeroed with the counts), then places its points.
// Order inside a bucket is immaterial: results do not depend on it.
__global__ __launch_bounds__(256) void wos_lpt_scatter_kernel(const DevTasks tk, int64_t n) {
  __shared__ uint32_t cnt[kCostBuckets], base[kCostBuckets], off[kCostBuckets];
  if (threadIdx.x < kCostBuckets) {
    cnt[threadIdx.x] = 0u;
    // offset of bucket b = points in buckets above b
    uint32_t acc = 0;
    for (int b = kCostBuckets - 1; b > (int)threadIdx.x; b--) acc += tk.hist[b];
    off[threadIdx.x] = acc;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int b = 0;
  uint32_t local = 0;
  if (i < n) {
    b = (tk.pstate[i] >> 8) & (kCostBuckets - 1);
    local = atomicAdd(&cnt[b], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kCostBuckets && cnt[threadIdx.x])
    base[threadIdx.x] = off[threadIdx.x] + atomicAdd(&tk.hist[kCostBuckets + threadIdx.x], cnt[threadIdx.x]);
  __syncthreads();
  if (i < n) tk.perm[base[b] + local] = (uint32_t)i;
}

// This unit's first-ball and walk kernels (wos_select.h): one channel, reference float
// semantics.  Walks <DIM, GG> with the Neumann term and Neumann-inert; 2D with LDS geometry
// also tail-spreading (DevParams::tail_spread).
#define UNIT_FIRST_BALLS(X) X(2, false, 1) X(3, false, 1)
#define UNIT_WALKS(X)                         \
  X(2, false, false, false, true, false, 1)   \
  X(2, false, false, false, false, false, 1)  \
  X(2, true, false, false, true, false, 1)    \
  X(2, true, false, false, false, false, 1)   \
  X(2, false, false, false, true, true, 1)    \
  X(2, false, false, false, false, true, 1)   \
  X(3, false, false, false, true, false, 1)   \
  X(3, false, false, false, false, false, 1)  \
  X(3, true, false, false, true, false, 1)    \
  X(3, true, false, false, false, false, 1)
UNIT_FIRST_BALLS(WOS_FIRST_BALL_INSTANTIATE)
template __global__ void wos_point_setup_kernel<2>(const DevScene, const DevParams, const float*, int64_t,
                                                   const DevTasks, unsigned long long*);
template __global__ void wos_point_setup_kernel<3>(const DevScene, const DevParams, const float*, int64_t,
                                                   const DevTasks, unsigned long long*);
UNIT_WALKS(WOS_WALK_INSTANTIATE)
UnitKernels unit_kernels_plain(const KernelVariant& v) {
  UnitKernels k;
  UNIT_FIRST_BALLS(WOS_FIRST_BALL_SELECT)
  UNIT_WALKS(WOS_WALK_SELECT)
  return k;
}
template __global__ void wos_fold_kernel<2>(const DevParams, const DevTasks, int64_t, float*, float*, int32_t*,
                                            int32_t*);
template __global__ void wos_fold_kernel<3>(const DevParams, const DevTasks, int64_t, float*, float*, int32_t*,
                                            int32_t*);
template __global__ void wos_fold4_kernel<3>(const DevParams, const DevTasks, int64_t, float*, float*, int32_t*,
                                             int32_t*, float*, float*);
template __global__ void wos_fold4_kernel<2>(const DevParams, const DevTasks, int64_t, float*, float*, int32_t*,
                                             int32_t*, float*, float*);
// the same with the per-point variances (wos_solve_var)
template __global__ void wos_fold4_kernel<3, true>(const DevParams, const DevTasks, int64_t, float*, float*,
                                                   int32_t*, int32_t*, float*, float*);
template __global__ void wos_fold4_kernel<2, true>(const DevParams, const DevTasks, int64_t, float*, float*,
                                                   int32_t*, int32_t*, float*, float*);

// math self-test kernel (parity of the deterministic math with the CPU oracle)
__global__ void wos_math_selftest_kernel(int which, const double* x, double* out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = x[i], r = 0.0;
  switch (which) {
    case 0: r = dexp(v); break;
    case 1: r = dlog(v); break;
    case 2: { double s, c; dsincos(v, &s, &c); r = s; } break;
    case 3: { double s, c; dsincos(v, &s, &c); r = c; } break;
    case 4: r = datan(v); break;
    case 5: r = __builtin_sqrt(v); break;
    case 6: r = bessi0(v); break;
    case 7: r = bessi1(v); break;
    case 8: r = bessk0(v); break;
    case 9: r = bessk1(v); break;
    case 10: r = (double)fexp((float)v); break;
    case 11: r = (double)flog((float)v); break;
    case 12: r = (double)fsin((float)v); break;
    case 13: r = (double)fcos((float)v); break;
    case 14: r = (double)fcbrt((float)v); break;
    case 15: r = (double)__builtin_sqrtf((float)v); break;
    case 16: r = (double)i0_fast((float)v); break;
    case 17: r = (double)k0_fast((float)v); break;
    // the fused evaluator of the kernels (bessel_ik) must equal 6..9
    case 18: { double a, b; bessel_ik<true, false>(v, &r, &a, nullptr, nullptr); (void)b; } break;
    case 19: { double a; bessel_ik<false, true>(v, nullptr, nullptr, &r, &a); } break;
    case 20: { double a; bessel_ik<true, false>(v, &a, &r, nullptr, nullptr); } break;
    case 21: { double a; bessel_ik<false, true>(v, nullptr, nullptr, &a, &r); } break;
    case 22: { double a, b, c; bessel_ik<true, true>(v, &a, &r, &b, &c); } break;
    case 23: { double a, b, c; bessel_ik<true, true>(v, &a, &b, &c, &r); } break;
    // the fused float pair of the rejection fast path (k0i0_fast): 24 I0, 25 K0
    case 24: { float k, i; k0i0_fast((float)v, &k, &i); r = (double)i; } break;
    case 25: { float k, i; k0i0_fast((float)v, &k, &i); r = (double)k; } break;
    default: r = __builtin_nan("");
  }
  out[i] = r;
}


// ---------------------------------------------------------------------------
// host-side launchers (called from wos_capi_*.cpp)
// ---------------------------------------------------------------------------
// the kernels of a variant: every unit is asked, the one that owns an instantiation answers
static UnitKernels kernels_of(const KernelVariant& v) {
  UnitKernels k;
  for (UnitKernels (*unit)(const KernelVariant&) : {unit_kernels_plain, unit_kernels_channels, unit_kernels_robust,
                                                    unit_kernels_channels_rb, unit_kernels_bstart}) {
    const UnitKernels u = unit(v);
    if (u.first_ball) k.first_ball = u.first_ball;
    if (u.walk) k.walk = u.walk;
  }
  return k;
}

hipError_t launch_first_balls(const KernelVariant& v, const DevScene& sc, const DevParams& prm, const float* pts,
                              int64_t n, int64_t base, int64_t stride, const DevTasks& tk,
                              unsigned long long* counters, unsigned int* work, int grid, size_t shmem, int lhs_floats,
                              hipStream_t s) {
  const FirstBallKernel kernel = kernels_of(v).first_ball;
  if (!kernel) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), shmem, s, sc, prm, pts, n, base, stride, tk, counters, work,
                     lhs_floats);
  return hipGetLastError();
}

hipError_t launch_point_setup(int dim, const DevScene& sc, const DevParams& prm, const float* pts, int64_t n,
                              const DevTasks& tk, hipStream_t s, unsigned long long* cksum) {
  const int grid = (int)((n * kSetupLanes + 255) / 256);
  if (grid < 1) return hipSuccess;
  if (dim == 2) hipLaunchKernelGGL(wos_point_setup_kernel<2>, dim3(grid), dim3(256), 0, s, sc, prm, pts, n, tk, cksum);
  else hipLaunchKernelGGL(wos_point_setup_kernel<3>, dim3(grid), dim3(256), 0, s, sc, prm, pts, n, tk, cksum);
  return hipGetLastError();
}

// ---- length hints: the express list (wos_scene.h H_*; DESIGN.md, Length hints) ----
// One block.  The list the last hinted walk kernel left holds (task, steps) of its long walks.  If the
// host's key matched (use) and the points are the ones the list was collected on (the point-setup
// checksums agree), the entries of >= express_min steps become the express list, longest first (a
// counting sort by steps; the order inside a step count is immaterial), each with its bit in the
// task bitmap and its point flagged in pstate (after point setup rewrote it).  The bits of the
// previous express list are cleared first, so the bitmap is never swept.  Then the list, the claim
// counters and the checksum are reset for the walk kernel that follows.
// The layout (express_slot, wos_scene.h): the entries of >= solo_min steps (0: none) are the solo tier,
// a prefix of the histogram; at most max_claims claims in all, so that one round of the walk grid's
// express waves hands out the whole list: the solo tier is cut to max_claims entries, then the list to
// what the claims left over hold.
// The kernel sits between point setup and the first balls, and its time is global-memory round trips:
// a thread reads its entries kHintBatch at a time (the loads of a batch are independent, then those of
// their points' states), and keeps which of them go express as a bit each, so the second pass reads
// the list alone.
constexpr int kHintBatch = 8;
static_assert((uint64_t)kHintListMax <= 64ull * kHintBins, "a thread's entries: a bit each of a 64-bit mask");
__global__ __launch_bounds__(kHintBins) void wos_hint_build_kernel(uint32_t* __restrict__ hc, int use,
                                                                   uint32_t express_min, uint32_t epw, uint32_t cap,
                                                                   uint32_t max_claims, uint32_t solo_min, const DevTasks tk) {
  __shared__ uint32_t s_bin[kHintBins], s_wave[kHintBins / kWave], s_nsolo;
  const int tid = threadIdx.x;
  uint32_t* const express = *reinterpret_cast<uint32_t* const*>(hc + H_EXPRESS);
  uint32_t* const bits = *reinterpret_cast<uint32_t* const*>(hc + H_BITS);
  const uint2* const list = *reinterpret_cast<const uint2* const*>(hc + H_LIST);
  const unsigned long long ck_cur = *reinterpret_cast<const unsigned long long*>(hc + H_CK_CUR);
  const unsigned long long ck_list = *reinterpret_cast<const unsigned long long*>(hc + H_CK_LIST);
  const uint32_t n_old = hc[H_NEXPRESS];
  const uint32_t n = hc[H_NLIST] < hc[H_CAP] ? hc[H_NLIST] : hc[H_CAP];
  // (a list that overflowed is a sample of walks that are the bulk, not the tail: no express list)
  const bool ok = use != 0 && ck_cur == ck_list && hc[H_NLIST] <= hc[H_CAP];
  const uint32_t T = (uint32_t)tk.T, wpp = (uint32_t)tk.wpp;
  for (uint32_t i0 = tid; i0 < n_old; i0 += kHintBatch * kHintBins) {
    uint32_t t[kHintBatch];
    for (int k = 0; k < kHintBatch; k++) t[k] = i0 + k * kHintBins < n_old ? express[i0 + k * kHintBins] : kExpressNone;
    for (int k = 0; k < kHintBatch; k++)
      if (t[k] != kExpressNone) atomicAnd(&bits[t[k] >> 5], ~(1u << (t[k] & 31u)));
  }
  s_bin[tid] = 0u;
  if (tid == 0) s_nsolo = 0u;
  __syncthreads();
  // bin 0: the longest
  const auto bin_of = [](const uint32_t steps) -> uint32_t {
    return (uint32_t)kHintBins - 1u - (steps < (uint32_t)kHintBins - 1u ? steps : (uint32_t)kHintBins - 1u);
  };
  // an entry goes express: long enough, a task of this batch, its point estimated.  Bit k of `go`:
  // the thread's entry tid + k kHintBins does.
  uint64_t go = 0ull;
  if (ok)
    for (uint32_t k0 = 0; (uint32_t)tid + k0 * kHintBins < n; k0 += kHintBatch) {
      uint2 e[kHintBatch];
      bool cand[kHintBatch];
      int32_t ps[kHintBatch];
      for (int k = 0; k < kHintBatch; k++) {
        const uint32_t i = (uint32_t)tid + (k0 + k) * kHintBins;
        e[k] = i < n ? list[i] : make_uint2(0u, 0u);
        cand[k] = i < n && e[k].y >= express_min && e[k].x < T;
      }
      for (int k = 0; k < kHintBatch; k++) ps[k] = cand[k] ? tk.pstate[e[k].x / wpp] : 0;
      for (int k = 0; k < kHintBatch; k++)
        if (ps[k] & kPtEstimate) {
          go |= 1ull << (k0 + k);
          atomicAdd(&s_bin[bin_of(e[k].y)], 1u);
        }
    }
  __syncthreads();
  // exclusive scan of the bins: inside each wave by shuffles, then the waves' totals
  const int lane = tid & (kWave - 1), wv = tid / kWave;
  const uint32_t mine = s_bin[tid];
  uint32_t inc = mine;
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t v = (uint32_t)__shfl_up((int)inc, off);
    if (lane >= off) inc += v;
  }
  if (lane == kWave - 1) s_wave[wv] = inc;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int w = 0; w < kHintBins / kWave; w++) {
    if (w < wv) before += s_wave[w];
    total += s_wave[w];
  }
  s_bin[tid] = before + inc - mine;  // the bin's fill cursor
  // the solo tier: the bins of >= solo_min steps (solo_min < kHintBins: wos_set_express_layout)
  if (solo_min > 0u && (uint32_t)tid == bin_of(solo_min)) s_nsolo = before + inc;
  __syncthreads();
  // (the longest of them: express waves are for the few walks that outlast the bulk)
  const uint32_t n_solo = s_nsolo < max_claims ? s_nsolo : max_claims;
  const uint64_t room = (uint64_t)n_solo + (uint64_t)(max_claims - n_solo) * epw;
  const uint32_t nx = ok ? ((uint64_t)total < room ? total : (uint32_t)room) : 0u;
  for (uint32_t k0 = 0; k0 < 64u && (go >> k0) != 0ull; k0 += kHintBatch) {
    uint2 e[kHintBatch];
    for (int k = 0; k < kHintBatch; k++)
      e[k] = ((go >> (k0 + k)) & 1ull) ? list[(uint32_t)tid + (k0 + k) * kHintBins] : make_uint2(0u, 0u);
    for (int k = 0; k < kHintBatch; k++) {
      if (!((go >> (k0 + k)) & 1ull)) continue;
      const uint32_t pos = atomicAdd(&s_bin[bin_of(e[k].y)], 1u);
      if (pos >= nx) continue;
      express[pos] = e[k].x;
      atomicOr(&bits[e[k].x >> 5], 1u << (e[k].x & 31u));
      atomicOr(&tk.pstate[e[k].x / wpp], kPtExpress);
    }
  }
  // (no barrier before these stores: every thread took what it reads of hc -- H_NLIST, H_CAP, H_NEXPRESS, the
  // checksums and the list pointers -- into registers before the first __syncthreads, and nothing above re-reads hc)
  if (tid == 0) {
    const uint32_t ns = n_solo < nx ? n_solo : nx;
    hc[H_NEXPRESS] = nx;
    hc[H_EPW] = epw;
    hc[H_NSOLO] = ns;
    hc[H_XG] = express_claims_below(nx, ns, epw);
    hc[H_CAP] = cap;
    hc[H_CLAIMED] = 0u;
    hc[H_NLIST] = 0u;
    hc[H_XCLAIM] = 0u;
    *reinterpret_cast<unsigned long long*>(hc + H_CK_LIST) = ck_cur;
    *reinterpret_cast<unsigned long long*>(hc + H_CK_CUR) = 0ull;
  }
}

hipError_t launch_hint_build(uint32_t* hc, int use, uint32_t express_min, uint32_t express_per_wave, uint32_t cap,
                             uint32_t max_claims, uint32_t solo_min, const DevTasks& tk, hipStream_t s) {
  hipLaunchKernelGGL(wos_hint_build_kernel, dim3(1), dim3(kHintBins), 0, s, hc, use, express_min, express_per_wave, cap,
                     max_claims, solo_min, tk);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void wos_zero_kernel(unsigned long long* a, int n64, uint32_t* b, int n32) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, di = gridDim.x * blockDim.x;
  for (int i = i0; i < n64; i += di) a[i] = 0ull;
  for (int i = i0; i < n32; i += di) b[i] = 0u;
}

hipError_t launch_zero(unsigned long long* a, int n64, uint32_t* b, int n32, hipStream_t s) {
  // one block per 1024 u64 (the grid-wide spreading control words can be ~10^4)
  const int grid = std::max(1, std::min(32, (std::max(n64, n32 / 2) + 1023) / 1024));
  hipLaunchKernelGGL(wos_zero_kernel, dim3(grid), dim3(256), 0, s, a, n64, b, n32);
  return hipGetLastError();
}

hipError_t launch_lpt_order(const DevTasks& tk, int64_t n, hipStream_t s) {
  const int grid = (int)((n + 255) / 256);
  if (grid > 0) hipLaunchKernelGGL(wos_lpt_scatter_kernel, dim3(grid), dim3(256), 0, s, tk, n);
  return hipGetLastError();
}

hipError_t launch_walks(const KernelVariant& v, const DevScene& sc, const DevParams& prm, const DevTasks& tk,
                        int64_t base, int64_t stride, unsigned long long* counters, unsigned int* tqueue, int grid,
                        size_t shmem, int geom_floats, hipStream_t s) {
  const WalkKernel kernel = kernels_of(v).walk;
  if (!kernel) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), shmem, s, sc, prm, tk, base, stride, counters, tqueue,
                     geom_floats);
  return hipGetLastError();
}

hipError_t launch_fold(int dim, const DevParams& prm, const DevTasks& tk, int64_t n, float* p, float* g,
                       int32_t* nest, int32_t* steps, float* p_var, float* g_var, hipStream_t s) {
  // the quad fold (pipelined staging), both dimensions: profiles/r5zm_ab_fold_pipe.log, r5zn_ab_fold4_2d.log
  if (tk.deriv == nullptr) {
    const int g4 = (int)((n + kFold4Points - 1) / kFold4Points);
    if (g4 < 1) return hipSuccess;
    const dim3 blk(4 * kFold4Points);
    if (p_var || g_var) {  // the variance instantiation only when a variance is asked for
      if (dim == 3)
        hipLaunchKernelGGL((wos_fold4_kernel<3, true>), dim3(g4), blk, 0, s, prm, tk, n, p, g, nest, steps, p_var, g_var);
      else
        hipLaunchKernelGGL((wos_fold4_kernel<2, true>), dim3(g4), blk, 0, s, prm, tk, n, p, g, nest, steps, p_var, g_var);
    } else if (dim == 3) {
      hipLaunchKernelGGL((wos_fold4_kernel<3>), dim3(g4), blk, 0, s, prm, tk, n, p, g, nest, steps, nullptr, nullptr);
    } else {
      hipLaunchKernelGGL((wos_fold4_kernel<2>), dim3(g4), blk, 0, s, prm, tk, n, p, g, nest, steps, nullptr, nullptr);
    }
    return hipGetLastError();
  }
  if (p_var || g_var) return hipErrorInvalidValue;  // the derivative fold carries no variance
  const int grid = (int)((n + kFoldPoints - 1) / kFoldPoints);
  if (grid < 1) return hipSuccess;
  if (dim == 2)
    hipLaunchKernelGGL(wos_fold_kernel<2>, dim3(grid), dim3(kFoldPoints), 0, s, prm, tk, n, p, g, nest, steps);
  else
    hipLaunchKernelGGL(wos_fold_kernel<3>, dim3(grid), dim3(kFoldPoints), 0, s, prm, tk, n, p, g, nest, steps);
  return hipGetLastError();
}

// P points' stratified samples and partners (fb_points_per_wave), then the sampler / shuffle scratch
size_t first_ball_wave_lds_bytes(int lhs_floats, int n_pairs) {
  const int P = fb_points_per_wave(n_pairs);
  return (size_t)2 * P * lhs_floats * sizeof(float) + fb_union_bytes(P * lhs_floats, 2 * n_pairs);
}

int first_ball_points_per_wave(int n_pairs) { return fb_points_per_wave(n_pairs); }

size_t walk_wave_lds_bytes(int dim) { return dim == 2 ? walk_scratch_bytes<2>() : walk_scratch_bytes<3>(); }

// residency of the very kernel the launchers above run for v (the instantiations differ in
// registers and static LDS)
hipError_t occupancy_blocks_per_cu(const KernelVariant& v, int which, size_t shmem, int* blocks) {
  const UnitKernels k = kernels_of(v);
  const void* kernel = which == 0 ? (const void*)k.first_ball : which == 1 ? (const void*)k.walk : nullptr;
  if (!kernel) return hipErrorInvalidValue;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, kernel, kBlock, shmem);
}

void diag_dump(const char* tag) {
  diag_print(tag, HIP_SYMBOL(g_diag));
#if WOS_TIMELINE
  // the walk kernel's live lanes over time (bins of 2^kTlShift ticks of the 100 MHz clock)
  static unsigned long long tl[1 + TL_NUM * kTlBins];
  hipMemcpyFromSymbol(tl, HIP_SYMBOL(g_tl), sizeof(tl));
  const double bt = (double)(1u << kTlShift);
  int last = 0;
  for (int b = 0; b < kTlBins; b++)
    if (tl[1 + TL_WAVE * kTlBins + b]) last = b;
  fprintf(stderr, "[timeline %s] bin_us %.2f (bin: busy waves, live lanes, lanes/busy wave, tasks handed out, walks finished)\n",
          tag, bt / 100.0);
  for (int b = 0; b <= last; b++) {
    const double w = tl[1 + TL_WAVE * kTlBins + b] / bt, l = tl[1 + TL_LANE * kTlBins + b] / bt;
    fprintf(stderr, "[timeline %s] %3d %8.1f %9.1f %6.2f %9llu %9llu\n", tag, b, w, l, w > 0 ? l / w : 0.0,
            tl[1 + TL_START * kTlBins + b], tl[1 + TL_FIN * kTlBins + b]);
  }
  static unsigned long long z[1 + TL_NUM * kTlBins];
  hipMemcpyToSymbol(HIP_SYMBOL(g_tl), z, sizeof(z));
#endif
}

// g_diag is per translation unit: `sym` is the calling unit's copy
void diag_print(const char* tag, const void* sym) {
#if WOS_DIAG
  unsigned long long d[D_NUM];
  hipMemcpyFromSymbol(d, sym, sizeof(d));
  fprintf(stderr, "[diag %s] iters %llu lanes/iter %.2f  cycles/iter: step %.0f star %.0f ray %.0f sample %.0f loop %.0f  ray_overflow %llu\n",
          tag, d[D_ITERS], (double)d[D_LANES] / (double)(d[D_ITERS] ? d[D_ITERS] : 1),
          (double)d[D_STEP] / d[D_ITERS], (double)d[D_STAR] / d[D_ITERS], (double)d[D_RAY] / d[D_ITERS],
          (double)d[D_SAMPLE] / d[D_ITERS], (double)d[D_LOOP] / d[D_ITERS], d[D_RAYOVF]);
  const double fp = (double)(d[D_FB_PTS] ? d[D_FB_PTS] : 1);
  fprintf(stderr, "[diag %s] first-ball: points %llu cycles/point: setup %.0f lhs %.0f balls %.0f total %.0f\n", tag,
          d[D_FB_PTS], d[D_FB_SETUP] / fp, d[D_FB_LHS] / fp, d[D_FB_BALLS] / fp, d[D_FB_TOTAL] / fp);
  fprintf(stderr, "[diag %s] first-ball parts cycles/point: ball update %.0f  sample (member a) %.0f  member a %.0f  member b %.0f  stores %.0f\n",
          tag, d[D_FB_UPD] / fp, d[D_FB_SMP] / fp, d[D_FB_MA] / fp, d[D_FB_MB] / fp, d[D_FB_ST] / fp);
  fprintf(stderr, "[diag %s] first-ball source samples: rejection iterations per point: sum over lanes %.1f, max over lanes %.1f\n",
          tag, d[D_FB_ITSUM] / fp, d[D_FB_ITMAX] / fp);
  fprintf(stderr, "[diag %s] step parts cycles/iter: mid (ball update) %.0f  end %.0f  tail %.0f\n", tag,
          (double)d[D_MID] / (d[D_ITERS] ? d[D_ITERS] : 1), (double)d[D_END] / (d[D_ITERS] ? d[D_ITERS] : 1),
          (double)d[D_TAIL] / (d[D_ITERS] ? d[D_ITERS] : 1));
  fprintf(stderr, "[diag %s] rejection: calls %llu, lanes/call %.1f, generations/call %.2f, items/call %.1f, quick-rejected %.1f%%, undecided %.3f%%\n",
          tag, d[D_RCALLS], (double)d[D_RLANES] / (d[D_RCALLS] ? d[D_RCALLS] : 1), (double)d[D_RGENS] / (d[D_RCALLS] ? d[D_RCALLS] : 1),
          (double)d[D_RITEMS] / (d[D_RCALLS] ? d[D_RCALLS] : 1), 100.0 * d[D_RQUICK] / (d[D_RITEMS] ? d[D_RITEMS] : 1),
          100.0 * d[D_RUND] / (d[D_RITEMS] ? d[D_RITEMS] : 1));
  fprintf(stderr, "[diag %s] max cycles/point (first balls) %llu, longest walk %llu steps, longest walk-kernel wave %llu cycles\n",
          tag, d[D_FB_MAX], d[D_WMAXLEN], d[D_WAVEMAX]);
  fprintf(stderr, "[diag %s] star calls %llu: groups visited/call %.2f, candidates/call %.2f, exact/call %.2f\n", tag,
          d[D_SCALLS], (double)d[D_SGVISIT] / d[D_SCALLS], (double)d[D_SCAND] / d[D_SCALLS],
          (double)d[D_SEXACT] / d[D_SCALLS]);
  fprintf(stderr, "[diag %s] after the queue ran dry: %llu iterations (%.1f%%), lanes/iter %.2f, %.1f%% of loop cycles\n",
          tag, d[D_XITERS], 100.0 * d[D_XITERS] / (d[D_ITERS] ? d[D_ITERS] : 1),
          (double)d[D_XLANES] / (d[D_XITERS] ? d[D_XITERS] : 1), 100.0 * d[D_XLOOP] / (d[D_LOOP] ? d[D_LOOP] : 1));
  fprintf(stderr, "[diag %s] express waves: %llu iterations, lanes/iter %.2f, cycles/iter (loop) %.0f\n", tag, d[D_E_ITERS],
          (double)d[D_E_LANES] / (d[D_E_ITERS] ? d[D_E_ITERS] : 1), (double)d[D_E_LOOP] / (d[D_E_ITERS] ? d[D_E_ITERS] : 1));
  static const char* const kLive[3] = {"1 live walk", "2-4 live walks", ">4 live walks"};
  for (int b = 0; b < 6; b++)
    fprintf(stderr, "[diag %s] express waves, %s, bulk queue %s: %llu iterations, cycles/iter (loop) %.0f\n", tag, kLive[b / 2],
            (b & 1) ? "dry" : "dealing", d[D_EB_ITERS + b], (double)d[D_EB_LOOP + b] / (d[D_EB_ITERS + b] ? d[D_EB_ITERS + b] : 1));
  const double li = (double)(d[D_L_ITERS] ? d[D_L_ITERS] : 1);
  fprintf(stderr, "[diag %s] <=2 live lanes: %llu iterations, cycles/iter: loop %.0f step %.0f star %.0f (cell %.0f prefix %.0f "
                  "window %.0f final %.0f) mid %.0f ray %.0f end %.0f sample %.0f tail %.0f\n",
          tag, d[D_L_ITERS], d[D_L_LOOP] / li, d[D_L_STEP] / li, d[D_L_STAR] / li, d[D_L_S_CELL] / li, d[D_L_S_PFX] / li,
          d[D_L_S_WIN] / li, d[D_L_S_FIN] / li, d[D_L_MID] / li, d[D_L_RAY] / li, d[D_L_END] / li, d[D_L_SAMPLE] / li,
          d[D_L_TAIL] / li);
  fprintf(stderr, "[diag %s] <=2 live lanes star detail: prologue %.0f  list build+sync %.0f  star total (in-function) %.0f\n", tag,
          d[D_L_S_PRE] / li, d[D_L_S_BUILD] / li, d[D_L_S_POST] / li);
  unsigned long long z[D_NUM] = {};
  hipMemcpyToSymbol(sym, z, sizeof(z));
#else
  (void)tag;
  (void)sym;
#endif
}

hipError_t launch_math_selftest(int which, const double* x, double* out, int64_t n, hipStream_t s) {
  int grid = (int)((n + 255) / 256);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(wos_math_selftest_kernel, dim3(grid), dim3(256), 0, s, which, x, out, n);
  return hipGetLastError();
}

}  // namespace wos

