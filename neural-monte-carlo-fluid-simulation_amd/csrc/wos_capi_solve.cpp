// wos_capi_solve.cpp -- the solve pipeline behind wos_solve / wos_solve_var / wos_solve_channels:
// what a solve's kernels are launched with (walk_layout, solve_plan, solve_grids), the pieces the
// walk tape's recording shares (batches, batch_head, fold_channels), and solve_locked, which boundary
// value caching also runs for its Dirichlet samples.
#include "wos_capi.h"

namespace wos::capi {

int walk_layout(wos_scene* s, const wos_solver_params* prm, WalkLayout& L) {
  Geom& geom = *s->geom;
  const wos::HostScene& host = geom.host;
  const int dim = host.dim;
  const int PS = dim == 2 ? wos::kPrimStride2 : wos::kPrimStride3;
  const int SS = dim == 2 ? wos::kSilStride2 : wos::kSilStride3;
  const int primAl = (host.n_prims * PS + 3) & ~3;
  const int silAl = (host.n_sil * SS + 3) & ~3;
  L.geom_floats = primAl + silAl + wos::kGroupStride * host.n_pgroups + wos::kSGroupStride * host.n_sgroups;
  // the walk kernel also stages the star-radius grid (after the silhouette groups)
  wos::DevScene& dsc = L.dsc;
  dsc = s->dev;
  dsc.sgrid = nullptr;
  dsc.sgrid_words = dsc.sgrid_off_words = 0;
  if (!(prm->schedule & WOS_SCHED_NO_STAR_GRID) && host.n_sil > 0) {
    const Geom::Grid* gr = nullptr;
    WOS_TRY(star_grid(geom, prm->silhouette_precision, prm->min_star_radius, &gr));
    if (gr->ok) {
      dsc.sgrid = gr->d;
      dsc.sgrid_words = (int32_t)gr->grid.words.size();
      dsc.sgrid_off_words = gr->grid.off_words;
      for (int k = 0; k < 3; k++) {
        dsc.sgrid_n[k] = gr->grid.n[k];
        dsc.sgrid_min[k] = gr->grid.gmin[k];
        dsc.sgrid_inv[k] = gr->grid.inv[k];
      }
    }
  }
  // the Dirichlet-distance cell grid (global memory)
  dsc.dgrid = nullptr;
  if (!(prm->schedule & WOS_SCHED_NO_DIR_GRID) && host.dim == 2 && host.n_dprims > 0) {
    bool ok = false;
    WOS_TRY(dir_grid(geom, &ok));
    if (ok) {
      dsc.dgrid = geom.d_dgrid;
      dsc.dgrid_off_words = geom.dgrid.off_words;
      for (int k = 0; k < 2; k++) {
        dsc.dgrid_n[k] = geom.dgrid.n[k];
        dsc.dgrid_min[k] = geom.dgrid.gmin[k];
        dsc.dgrid_inv[k] = geom.dgrid.inv[k];
      }
    }
  }
  // ... and the Dirichlet primitives with their culling boxes (after the grid)
  const int dir_floats = ((host.n_dprims * PS + 3) & ~3) + wos::kGroupStride * host.n_dgroups;
  L.geom_floats_walk = L.geom_floats + ((dsc.sgrid_words + 3) & ~3) + dir_floats;
  L.shmem_walk = (size_t)L.geom_floats_walk * sizeof(float) + wos::kWavesPerBlockHost * wos::walk_wave_lds_bytes(dim);
  if (dsc.sgrid != nullptr && L.shmem_walk > kLdsDynamicMax) {  // no room: the group scan alone
    dsc.sgrid = nullptr;
    dsc.sgrid_words = dsc.sgrid_off_words = 0;
    L.geom_floats_walk = L.geom_floats + dir_floats;
    L.shmem_walk =
        (size_t)L.geom_floats_walk * sizeof(float) + wos::kWavesPerBlockHost * wos::walk_wave_lds_bytes(dim);
  }
  return WOS_OK;
}

wos::DevParams dev_params(const wos_solver_params* prm) {
  wos::DevParams dp{};
  const bool anti = !prm->disable_gradient_antithetic_variates;
  dp.n_walks = prm->n_walks;
  dp.n_anti = anti ? 2 : 1;
  dp.n_pairs = anti ? std::max(1, prm->n_walks / 2) : prm->n_walks;
  dp.max_walk_length = prm->max_walk_length;
  dp.steps_before_tikhonov = prm->steps_before_tikhonov;
  dp.steps_before_maximal_spheres = prm->steps_before_maximal_spheres;
  dp.epsilon_shell = prm->epsilon_shell;
  dp.min_star_radius = prm->min_star_radius;
  dp.silhouette_precision = prm->silhouette_precision;
  dp.rr_threshold = prm->russian_roulette_threshold;
  dp.boundary_distance_mask = prm->boundary_distance_mask;
  dp.use_cv = !prm->disable_gradient_control_variates;
  dp.use_cosine = prm->use_cosine_sampling;
  dp.ignore_dirichlet = prm->ignore_dirichlet;
  dp.ignore_neumann = prm->ignore_neumann;
  dp.ignore_source = prm->ignore_source;
  dp.robust = prm->robust_float != 0;
  dp.seed = prm->seed;
  return dp;
}

int check_params(const std::string& fn, const wos_solver_params* prm) {
  if (prm->n_walks < 1) return fail(WOS_E_INVALID, fn + ": nWalks must be >= 1");
  if (prm->max_walk_length < 0) return fail(WOS_E_INVALID, fn + ": maxWalkLength must be >= 0");
  if (!(prm->epsilon_shell >= 0.0f) || !(prm->min_star_radius >= 0.0f) || !(prm->silhouette_precision >= 0.0f))
    return fail(WOS_E_INVALID, fn + ": negative tolerance");
  return WOS_OK;
}

#ifndef WOS_LHS_JUMP_STAGE
#define WOS_LHS_JUMP_STAGE 1
#endif

int solve_plan(DevCtx& c, wos_scene* s, const wos_solver_params* prm, const SolveExtra& ex, bool record, SolvePlan& P) {
  Geom& geom = *s->geom;
  const wos::HostScene& host = geom.host;
  const int dim = host.dim;
  wos::DevParams& dp = P.dp;
  dp = dev_params(prm);
  dp.force_estimate = ex.force_estimate ? 1 : 0;
  dp.wave_prio = ex.wave_prio;
  {
    // diagonal draws + shuffle draws of the stratified samples
    const int k_needed = 2 * (2 * dp.n_pairs) * (dim - 1);
    WOS_TRY(ensure_jump(c, k_needed));
    dp.jump = c.d_jump;
    dp.n_jump = c.n_jump;
    dp.rej_tab = c.d_rejtab;
  }

  // LDS: the walk kernel's staged geometry; per wave, the first-ball kernel's stratified
  // samples and their shuffle partners
  WalkLayout wl;
  WOS_TRY(walk_layout(s, prm, wl));
  wos::DevScene& dsc = P.dsc;
  dsc = wl.dsc;
  P.geom_floats_walk = wl.geom_floats_walk;
  P.shmem_walk = wl.shmem_walk;
  P.lhs_floats = ((2 * dp.n_pairs * (dim - 1)) + 3) & ~3;
  // the first-ball kernel stages no geometry (the point-setup kernel did the queries)
  P.shmem_fb = wos::kWavesPerBlockHost * wos::first_ball_wave_lds_bytes(P.lhs_floats, dp.n_pairs);
  P.shmem_fb_run = P.shmem_fb;  // + the staged jump constants (dp.lhs_jump_n), decided in solve_grids
  // scenes beyond the LDS budget (or WOS_SCHED_GEOM_GLOBAL): geometry read from global
  // memory through L2, LDS for the per-wave scratch only
  wos::DevScene& dfb = P.dfb;
  dfb = s->dev;
  // the first-ball kernel's walk-start Dirichlet distances read the cell grid too (global memory)
  dfb.dgrid = dsc.dgrid;
  dfb.dgrid_off_words = dsc.dgrid_off_words;
  for (int k = 0; k < 2; k++) {
    dfb.dgrid_n[k] = dsc.dgrid_n[k];
    dfb.dgrid_min[k] = dsc.dgrid_min[k];
    dfb.dgrid_inv[k] = dsc.dgrid_inv[k];
  }
  // (only the walk kernel stages geometry, so only its LDS decides)
  if ((prm->schedule & WOS_SCHED_GEOM_GLOBAL) || P.shmem_walk > kLdsDynamicMax) {
    dfb.geom_global = 1;
    dsc.geom_global = 1;
    P.geom_floats_walk = 0;
    P.shmem_walk = wos::kWavesPerBlockHost * wos::walk_wave_lds_bytes(dim);
  }
  if (P.shmem_fb > kLdsDynamicMax)
    return fail(WOS_E_CAPACITY, "wos_solve: nWalks exceed the LDS budget of the first-ball kernel (" +
                                    std::to_string(P.shmem_fb) + " bytes of stratified samples per block)");
  if (P.shmem_walk > kLdsDynamicMax)
    return fail(WOS_E_CAPACITY, "wos_solve: the walk kernel's per-wave scratch exceeds the LDS budget (" +
                                    std::to_string(P.shmem_walk) + " bytes)");

  P.wpp = (int64_t)dp.n_pairs * dp.n_anti;
  // The Neumann term (h == 0) is +0 at every step unless a ball's float members overflow
  // (mu R > 85 is the kernels' gate).  In a watertight single-sided scene every estimated
  // point and walk lies inside the boundary's bounding box, so R < its diagonal: below
  // the gate the walk kernel runs without the term's code (bit-identical results;
  // WOS_SCHED_FULL_NEUMANN keeps the full kernel).
  {
    double diag2 = 0.0;
    for (int k = 0; k < 3; k++) diag2 += (double)host.ext[k] * host.ext[k];
    const double mu_r = std::sqrt(std::max(0.0, (double)s->dev.absorption)) * std::sqrt(diag2) * 1.01;
    // (image-valued h makes the term non-zero at every step: never inert)
    dp.neumann_inert = (!dp.robust && s->dev.watertight && !s->dev.double_sided && mu_r < 80.0 && !s->dev.nimg &&
                        !(prm->schedule & WOS_SCHED_FULL_NEUMANN)) ? 1 : 0;
  }
  // Walks handed to idle sibling waves once the queue is dry (the walk kernel's SPR
  // instantiation): 2D scenes with LDS geometry (karman -4 %, its stride-8 shard -13 %,
  // config C neutral); 3D pays more for the extra live state than its short tails return
  // (profiles/r4zc_*, r4ze_*)
  dp.tail_spread = (dim == 2 && !dp.robust && !dsc.geom_global && !(prm->schedule & WOS_SCHED_NO_TAIL_SPREAD)) ? 1 : 0;
#ifdef WOS_ACCT_NOSPREAD
  dp.tail_spread = 0;  // HBM-accounting build: the walk kernel without tail spreading (no scratch)
#endif
  if (record) {
    dp.neumann_inert = 0;
    dp.tail_spread = 0;
    dsc.n_channels = 1;
    dfb.n_channels = 1;
  }
  // the first-ball and walk instantiations of this solve: launched and sized through the same key
  P.kv = wos::kernel_variant(dim, dsc, dp, false);
  return WOS_OK;
}

int solve_grids(DevCtx& c, int dim, int64_t chunk, bool record, SolvePlan& P) {
  wos::DevParams& dp = P.dp;
  const bool gg = P.dsc.geom_global != 0;
  const auto occupancy = [&](int which, size_t shmem, int* blocks) {
    return record ? wos::occupancy_rec_blocks_per_cu(dim, gg, which, shmem, blocks)
                  : wos::occupancy_blocks_per_cu(P.kv, which, shmem, blocks);
  };
  HIP_TRY(occupancy(0, P.shmem_fb, &P.bpc_fb));
  // the stratified samples' jump constants in LDS, unless they cost the first-ball kernel a block per CU
  const int jn = std::min(2 * (2 * dp.n_pairs) * (dim - 1), wos::kLhsJumpMax);
  const size_t shmem_j = P.shmem_fb + (size_t)jn * 2 * sizeof(uint64_t);
  int bpc_j = 0;
  if (jn > 0 && shmem_j <= kLdsDynamicMax) HIP_TRY(occupancy(0, shmem_j, &bpc_j));
  if (WOS_LHS_JUMP_STAGE && jn > 0 && bpc_j >= P.bpc_fb) {
    dp.lhs_jump_n = jn;
    P.shmem_fb_run = shmem_j;
  }
  const int64_t fb_waves = (chunk + wos::first_ball_points_per_wave(dp.n_pairs) - 1) / wos::first_ball_points_per_wave(dp.n_pairs);
  P.grid_fb = (int)std::min<int64_t>((fb_waves + wos::kWavesPerBlockHost - 1) / wos::kWavesPerBlockHost,
                                     (int64_t)std::max(1, P.bpc_fb) * std::max(1, c.num_cus));
  // of the walk instantiation launch_walks runs for kv (tail spreading has its own LDS and state)
  HIP_TRY(occupancy(1, P.shmem_walk, &P.bpc_walk));
  P.grid_walk = std::max(1, P.bpc_walk) * std::max(1, c.num_cus);
  return WOS_OK;
}

Batches batches(int64_t n, int64_t wpp) {
  Batches b;
  b.chunk = std::max<int64_t>(1, std::min<int64_t>(n, g_max_batch_tasks.load() / wpp));
  b.n_chunks = n > 0 ? (n + b.chunk - 1) / b.chunk : 0;
  return b;
}

int batch_head(DevCtx& c, int dim, const SolvePlan& P, int64_t k, const float* d_pts, int64_t nb,
               const wos::DevTasks& tk, hipEvent_t after_zero, hipStream_t st, unsigned long long* cksum) {
  HIP_TRY(wos::launch_zero(k == 0 ? c.d_counters : c.d_counters + wos::kNumCounters,
                           k == 0 ? wos::kNumCounterSlots : wos::kNumCounterSlots - wos::kNumCounters,
                           tk.hist, 2 * wos::kCostBuckets, st));
  if (after_zero) HIP_TRY(hipEventRecord(after_zero, st));
  HIP_TRY(wos::launch_point_setup(dim, P.dfb, P.dp, d_pts, nb, tk, st, cksum));
  HIP_TRY(wos::launch_lpt_order(tk, nb, st));
  return WOS_OK;
}

int fold_channels(int dim, const wos::DevParams& dp, const wos::DevTasks& tk, int C, int64_t nb, int64_t b0,
                  int64_t n, const SolveOut& out, hipStream_t st) {
  for (int ch = 0; ch < C; ch++) {
    wos::DevTasks tkc = tk;
    tkc.total = tk.total + (int64_t)ch * tk.T;
    tkc.first = tk.first + (int64_t)ch * tk.T;
    const int64_t o1 = (int64_t)ch * n + b0, od = ((int64_t)ch * n + b0) * dim;
    HIP_TRY(wos::launch_fold(dim, dp, tkc, nb, out.p + o1, out.grad + od,
                             (out.n_est && ch == 0) ? out.n_est + b0 : nullptr,
                             (out.steps && ch == 0) ? out.steps + b0 : nullptr, out.p_var ? out.p_var + o1 : nullptr,
                             out.grad_var ? out.grad_var + od : nullptr, st));
  }
  return WOS_OK;
}

int solve_locked(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                 int64_t index_stride, float* p, float* grad, int32_t* n_est, int32_t* steps, wos_stats* stats,
                 void* stream, uint32_t flags, const SolveExtra& ex) {
  const int dim = s->geom->host.dim;
  hipStream_t st = (hipStream_t)stream;
  DevCtx& c = g_ctx[s->device];
  WOS_TRY(ctx_ready(c, s->device));

  // the kernels' parameters, scene views and LDS layout of this solve
  SolvePlan plan;
  WOS_TRY(solve_plan(c, s, prm, ex, false, plan));
  wos::DevParams& dp = plan.dp;

  // the shared workspace may still be in use by a solve enqueued on another stream
  HIP_TRY(ctx_order(c, st));

  const bool dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  const int C = ex.channels;  // outputs [C][n] / [C][n*dim]: the staging holds C * n points
  OutStage out;
  WOS_TRY(stage_outputs(c, SolveOut{p, grad, n_est, steps, ex.p_var, ex.grad_var}, dev_ptrs, n, C, dim, out));
  const float* d_pts = pts;
  if (out.staged) {
    HIP_TRY(hipMemcpyAsync(c.d_pts, pts, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, st));
    d_pts = c.d_pts;
  }

  const int64_t wpp = plan.wpp;
  const Batches bt = batches(n, wpp);
  if (n > 0) {
    WOS_TRY(ensure_tasks(c, dim, bt.chunk * wpp, bt.chunk, C));
    WOS_TRY(solve_grids(c, dim, bt.chunk, false, plan));
  }
  // Length hints: the plain 2D one-channel solve in one batch (the other kernels carry none of it).
  // The list this solve's walk kernel leaves serves the next solve of the same key; the one in the
  // workspace is used if it was left under this solve's key.
  const bool hinted = dim == 2 && !dp.robust && dp.neumann_inert && C == 1 && bt.n_chunks == 1 && !ex.ddir &&
                      !ex.deriv && !(prm->schedule & WOS_SCHED_NO_LENGTH_HINTS);
  uint32_t* hc = nullptr;
  uint32_t hint_word = 0;
  bool hint_use = false;
  HintTuning ht{};
  HintKey hint_key;
  if (hinted) {
    {
      std::lock_guard<std::mutex> lk(g_hint_mu);
      ht = g_hint_tuning;
    }
    WOS_TRY(ensure_hints(c, bt.chunk * wpp, &hc));
    HintKey& key = hint_key;
    key.dim = dim; key.wpp = (int32_t)wpp; key.n_walks = dp.n_walks; key.n_anti = dp.n_anti;
    key.n = n; key.index_base = index_base; key.index_stride = index_stride;
    key.seed = dp.seed; key.geometry = s->geom->content_id;
    key.max_walk_length = dp.max_walk_length; key.steps_before_tikhonov = dp.steps_before_tikhonov;
    key.steps_before_maximal_spheres = dp.steps_before_maximal_spheres;
    key.use_cosine = dp.use_cosine; key.ignore_dirichlet = dp.ignore_dirichlet;
    key.ignore_neumann = dp.ignore_neumann; key.ignore_source = dp.ignore_source;
    key.force_estimate = dp.force_estimate;
    key.watertight = s->dev.watertight; key.double_sided = s->dev.double_sided;
    key.epsilon_shell = dp.epsilon_shell; key.min_star_radius = dp.min_star_radius;
    key.silhouette_precision = dp.silhouette_precision; key.rr_threshold = dp.rr_threshold;
    key.absorption = s->dev.absorption;
    hint_use = c.hint_key_valid && key == c.hint_key;
    // the list belongs to nobody until this solve's walk kernel, which refills it, is enqueued
    c.hint_key_valid = false;
    hint_word = wos::kHintCollect | (hint_use ? wos::kHintUse : 0u) | ((uint32_t)ht.priority << wos::kHintPrioShift) |
                (ht.stripe ? wos::kHintStripe : 0u) | (ht.placement ? wos::kHintPinned : 0u) |
                ((uint32_t)ht.hint_min << wos::kHintMinShift);
  }
  if (n > 0) c.hint_last = hinted;
  StatSlot* slot = nullptr;
  WOS_TRY(slot_open(c, st, 4 * bt.n_chunks, bt.n_chunks, plan.shape(), &slot));
  StatSlot& q = *slot;
  if (bt.n_chunks == 0) HIP_TRY(wos::launch_zero(c.d_counters, wos::kNumCounterSlots, nullptr, 0, st));
  for (int64_t k = 0; k < bt.n_chunks; k++) {
    const int64_t b0 = k * bt.chunk;
    hipEvent_t* ev = &q.bev[4 * k];
    const int64_t nb = std::min(bt.chunk, n - b0);
    wos::DevTasks tk = task_view(c, dim, nb * wpp, (int32_t)wpp, C);
    tk.ddir = ex.ddir ? ex.ddir + b0 * dim : nullptr;
    tk.deriv = ex.deriv ? ex.deriv + b0 : nullptr;
    const int64_t bbase = index_base + b0 * index_stride;
    unsigned int* q_points = (unsigned int*)(c.d_counters + wos::kNumCounters);
    unsigned int* q_tasks = (unsigned int*)(c.d_counters + wos::kTaskQueueSlot0);
    const int walk_grid = (int)std::min<int64_t>(plan.grid_walk, (tk.T + 63) / 64);
    tk.hint = hint_word;
    WOS_TRY(batch_head(c, dim, plan, k, d_pts + b0 * dim, nb, tk, ev[0], st,
                       hinted ? (unsigned long long*)(hc + wos::H_CK_CUR) : nullptr));
    // at most one claim per workgroup of the walk grid: where more walks than that are "long", they are
    // the bulk, and sparse waves would only cost throughput
    if (hinted)
      HIP_TRY(wos::launch_hint_build(hc, hint_use ? 1 : 0, (uint32_t)ht.express_min, (uint32_t)ht.express_per_wave,
                                     (uint32_t)ht.capacity, (uint32_t)walk_grid, (uint32_t)ht.solo_min, tk,
                                     st));
    HIP_TRY(wos::launch_first_balls(plan.kv, plan.dfb, dp, d_pts + b0 * dim, nb, bbase, index_stride, tk,
                                    c.d_counters, q_points, plan.grid_fb, plan.shmem_fb_run, plan.lhs_floats, st));
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(wos::launch_walks(plan.kv, plan.dsc, dp, tk, bbase, index_stride, c.d_counters, q_tasks, walk_grid,
                              plan.shmem_walk, plan.geom_floats_walk, st));
    if (hinted) {
      c.hint_key = hint_key;
      c.hint_key_valid = true;
    }
    HIP_TRY(hipEventRecord(ev[2], st));
    WOS_TRY(fold_channels(dim, dp, tk, C, nb, b0, n, out.dev, st));
    HIP_TRY(hipEventRecord(ev[3], st));
  }
  WOS_TRY(slot_close(q, c.d_counters, st));
  WOS_TRY(copy_back(out, st));
  const bool async = (flags & WOS_ASYNC) && dev_ptrs;
  WOS_TRY(slot_finish(c, q, st, async, stats));
  if (!async) wos::diag_dump(dim == 2 ? "2d" : "3d");  // DIAG builds only
  return WOS_OK;
}

// the argument checks of every solve entry point; n_channels 0: wos_solve / wos_solve_var,
// which refuse a scene that holds several channels
static int solve_checked(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                         int64_t index_stride, int32_t n_channels, float* p, float* grad, float* p_var,
                         float* grad_var, int32_t* n_est, int32_t* steps, wos_stats* stats, void* stream,
                         uint32_t flags) {
  if (!s || !prm) return fail(WOS_E_INVALID, "wos_solve: null scene/params");
  if (n < 0) return fail(WOS_E_INVALID, "wos_solve: negative point count");
  if (n > 0 && (!pts || !p || !grad)) return fail(WOS_E_INVALID, "wos_solve: null point/output buffer");
  if (n >= (int64_t)0xFFFFFFF0LL) return fail(WOS_E_INVALID, "wos_solve: too many points for one call");
  WOS_TRY(check_params("wos_solve", prm));
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  if (n_channels == 0 && s->dev.n_channels > 1)
    return fail(WOS_E_INVALID, "wos_solve: the scene holds " + std::to_string(s->dev.n_channels) +
                                   " source channels; use wos_solve_channels (or wos_scene_set_source for one)");
  if (n_channels != 0 && n_channels != s->dev.n_channels)
    return fail(WOS_E_INVALID, "wos_solve_channels: n_channels " + std::to_string(n_channels) +
                                   " differs from the scene's " + std::to_string(s->dev.n_channels));
  SolveExtra ex;
  ex.p_var = p_var;
  ex.grad_var = grad_var;
  ex.channels = s->dev.n_channels;
  return solve_locked(s, prm, pts, n, index_base, index_stride, p, grad, n_est, steps, stats, stream, flags, ex);
}

}  // namespace wos::capi

using namespace wos::capi;

extern "C" {

void wos_default_params(wos_solver_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  // defaults of runWalkOnStars_sampled (demo.cpp:121-137) and grid.h:159
  p->n_walks = 128;
  p->max_walk_length = 1024;
  p->steps_before_tikhonov = 1024;
  p->steps_before_maximal_spheres = 1024;
  p->epsilon_shell = 1e-3f;
  p->min_star_radius = 1e-3f;
  p->silhouette_precision = 1e-3f;
  p->russian_roulette_threshold = 0.0f;
  p->boundary_distance_mask = 0.0f;
  p->seed = 0x5EED0001ULL;
}

int wos_solve_var(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                  int64_t index_stride, float* p, float* grad, float* p_var, float* grad_var, int32_t* n_est,
                  int32_t* steps, wos_stats* stats, void* stream, uint32_t flags) {
  return solve_checked(s, prm, pts, n, index_base, index_stride, 0, p, grad, p_var, grad_var, n_est, steps, stats,
                       stream, flags);
}

int wos_solve_channels(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                       int64_t index_stride, int32_t n_channels, float* p, float* grad, float* p_var,
                       float* grad_var, int32_t* n_est, int32_t* steps, wos_stats* stats, void* stream,
                       uint32_t flags) {
  if (n_channels < 1 || n_channels > WOS_MAX_CHANNELS)
    return fail(WOS_E_INVALID, "wos_solve_channels: n_channels must be 1.." + std::to_string(WOS_MAX_CHANNELS) +
                                   ", got " + std::to_string(n_channels));
  return solve_checked(s, prm, pts, n, index_base, index_stride, n_channels, p, grad, p_var, grad_var, n_est, steps,
                       stats, stream, flags);
}

int wos_solve(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
              int64_t index_stride, float* p, float* grad, int32_t* n_est, int32_t* steps, wos_stats* stats,
              void* stream, uint32_t flags) {
  return wos_solve_var(s, prm, pts, n, index_base, index_stride, p, grad, nullptr, nullptr, n_est, steps, stats,
                       stream, flags);
}

}  // extern "C"
