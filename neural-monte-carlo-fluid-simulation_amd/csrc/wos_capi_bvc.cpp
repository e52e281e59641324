// wos_capi_bvc.cpp -- boundary value caching (wos_bvc, include/wos.h; kernels in wos_bvc.hip, the
// host sampler in wos_bvc_host.cpp): three independent walk sets on three streams, then the splat.
#include "wos_capi.h"

using namespace wos::capi;

// Stream priorities of boundary value caching's walk sets: the Dirichlet samples' solve and
// the Neumann samples' walks feed the splat (high), the near-boundary walks do not (low).
static int bvc_priority(bool high) {
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return 0;
  return high ? greatest : least;
}

// a side workspace's stream, event and counters (created on first use)
static int side_ready(TaskWs& w, int priority) {
  if (!w.stream) HIP_TRY(hipStreamCreateWithPriority(&w.stream, hipStreamNonBlocking, priority));
  if (!w.done) HIP_TRY(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
  if (!w.counters) HIP_TRY(hipMalloc((void**)&w.counters, wos::kNumCounterSlots * sizeof(unsigned long long)));
  return WOS_OK;
}

extern "C" {

void wos_default_bvc_params(wos_bvc_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  // defaults of runBoundaryValueCaching (demo.cpp:274-290)
  p->n_walks_solution = 128;
  p->n_walks_gradient = 640;
  p->boundary_cache_size = 1024;
  p->domain_cache_size = 1024;
  p->grid_res = 0;
  p->normal_offset = 5.0f * 1e-3f;
  p->radius_clamp = 1e-3f;
  p->kernel_regularization = 0.0f;
}

int wos_bvc(wos_scene* s, const wos_solver_params* prm, const wos_bvc_params* bp, float* solution, float* grad,
            float* samples, int64_t samples_capacity, int64_t* counts, wos_stats* stats) {
  if (!s || !prm || !bp || !solution || !grad) return fail(WOS_E_INVALID, "wos_bvc: null argument");
  if (bp->grid_res < 1) return fail(WOS_E_INVALID, "wos_bvc: gridRes must be >= 1");
  if (bp->n_walks_solution < 1) return fail(WOS_E_INVALID, "wos_bvc: nWalksForCachedSolutionEstimates must be >= 1");
  if (bp->boundary_cache_size < 0 || bp->domain_cache_size < 0) return fail(WOS_E_INVALID, "wos_bvc: negative cache size");
  if (prm->max_walk_length < 0) return fail(WOS_E_INVALID, "wos_bvc: maxWalkLength must be >= 0");
  {
    // both extents 0: the scene's bounding box; else both finite and > 0 (and a finite corner)
    const float* gb = bp->grid_box;
    const bool unset = gb[2] == 0.0f && gb[3] == 0.0f;
    const bool valid = std::isfinite(gb[0]) && std::isfinite(gb[1]) && std::isfinite(gb[2]) && std::isfinite(gb[3]) &&
                       gb[2] > 0.0f && gb[3] > 0.0f;
    if (!unset && !valid)
      return fail(WOS_E_INVALID, "wos_bvc: grid_box needs both extents 0 (the scene's box) or both finite and > 0");
  }
  std::lock_guard<std::mutex> lock(s->mu);
  if (s->dev.n_channels > 1)
    return fail(WOS_E_INVALID, "wos_bvc: the scene holds " + std::to_string(s->dev.n_channels) +
                                   " source channels; boundary value caching is single-channel");
  Geom& geom = *s->geom;
  const wos::HostScene& host = geom.host;
  if (host.dim != 2) return fail(WOS_E_INVALID, "wos_bvc: boundary value caching is 2D (the reference exports it from the 2D module only)");
  if (host.n_prims + host.n_dprims <= 0) return fail(WOS_E_INVALID, "wos_bvc: scene has no boundary");
  const bool has_dir = host.n_dprims > 0;
  if (has_dir && bp->n_walks_gradient < 1)
    return fail(WOS_E_INVALID, "wos_bvc: nWalksForCachedGradientEstimates must be >= 1");
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  WOS_TRY(ctx_ready(c, s->device));
  hipStream_t st = nullptr;
  HIP_TRY(ctx_order(c, st));
  HIP_TRY(hipStreamSynchronize(st));

  // ---- host: boundary samples (Neumann then Dirichlet segments), domain candidates,
  // evaluation grid (over grid_box, else the scene's bounding box)
  wos::BvcSampling smp;
  std::string err;
  const float pmin[2] = {host.pmin[0], host.pmin[1]}, pmax[2] = {host.pmax[0], host.pmax[1]};
  if (!wos::bvc_generate_samples(geom.v.data(), (int)(geom.v.size() / 2), geom.ix.data(), (int)(geom.ix.size() / 2),
                                 geom.dv.data(), (int)(geom.dv.size() / 2), geom.dix.data(),
                                 (int)(geom.dix.size() / 2), pmin, pmax, geom.double_sided != 0,
                                 bp->boundary_cache_size, bp->domain_cache_size, bp->normal_offset,
                                 prm->ignore_source != 0, prm->seed, smp, err))
    return fail(WOS_E_INVALID, "wos_bvc: " + err);
  float gmin[2] = {pmin[0], pmin[1]}, gext[2] = {pmax[0] - pmin[0], pmax[1] - pmin[1]};
  if (bp->grid_box[2] > 0.0f && bp->grid_box[3] > 0.0f) {
    gmin[0] = bp->grid_box[0]; gmin[1] = bp->grid_box[1];
    gext[0] = bp->grid_box[2]; gext[1] = bp->grid_box[3];
  }
  std::vector<float> ept;
  wos::bvc_evaluation_grid(bp->grid_res, gmin, gext, ept);
  const int64_t nb = (int64_t)smp.aligned.size();
  const int64_t nd = (int64_t)(smp.dcand.size() / 2);
  const int64_t ne = (int64_t)bp->grid_res * bp->grid_res;
  // runs of consecutive boundary samples of one type (the sampler emits a cache's Neumann
  // samples before its Dirichlet ones): [begin, end), Dirichlet?
  struct Run { int64_t b0, b1; bool dir; };
  std::vector<Run> runs;
  for (int64_t i = 0; i < nb; i++) {
    const bool d = smp.dirichlet[i] != 0;
    if (runs.empty() || runs.back().dir != d || runs.back().b1 != i) runs.push_back({i, i + 1, d});
    else runs.back().b1 = i + 1;
  }
  // BoundarySampler::computeEstimates (boundary_sampler.h:154-166): a Dirichlet sample's
  // derivative is along its normal, reversed for normal-aligned samples of double-sided scenes
  std::vector<float> ddir_h(2 * nb, 0.0f);
  for (int64_t i = 0; i < nb; i++) {
    const float sg = (geom.double_sided && smp.aligned[i]) ? -1.0f : 1.0f;
    ddir_h[2 * i] = smp.bnrm[2 * i] * sg;
    ddir_h[2 * i + 1] = smp.bnrm[2 * i + 1] * sg;
  }

  // ---- device buffers (freed on every exit)
  DevBufs B;
  float *d_bpt, *d_bnrm, *d_bdd, *d_bsol, *d_bdn, *d_ddir, *d_dc, *d_dsrc, *d_ept, *d_edd, *d_end, *d_sol, *d_grad;
  int32_t *d_bnest, *d_din, *d_ein;
  uint8_t* d_al;
  HIP_TRY(B.get(&d_bpt, 2 * nb)); HIP_TRY(B.get(&d_bnrm, 2 * nb)); HIP_TRY(B.get(&d_bdd, nb));
  HIP_TRY(B.get(&d_bsol, nb)); HIP_TRY(B.get(&d_bdn, nb)); HIP_TRY(B.get(&d_ddir, 2 * nb));
  float* d_dgrad;  // the Dirichlet samples' gradient (unused output of the solve)
  HIP_TRY(B.get(&d_bnest, nb)); HIP_TRY(B.get(&d_al, nb)); HIP_TRY(B.get(&d_dgrad, 2 * nb));
  HIP_TRY(B.get(&d_dc, 2 * nd)); HIP_TRY(B.get(&d_din, nd)); HIP_TRY(B.get(&d_dsrc, nd));
  HIP_TRY(B.get(&d_ept, 2 * ne)); HIP_TRY(B.get(&d_edd, ne)); HIP_TRY(B.get(&d_end, ne)); HIP_TRY(B.get(&d_ein, ne));
  HIP_TRY(B.get(&d_sol, ne)); HIP_TRY(B.get(&d_grad, 2 * ne));
  if (nb > 0) {
    HIP_TRY(hipMemcpy(d_bpt, smp.bpt.data(), 2 * nb * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_bnrm, smp.bnrm.data(), 2 * nb * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_al, smp.aligned.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ddir, ddir_h.data(), 2 * nb * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d_bdn, 0, nb * sizeof(float), st));
  }
  if (nd > 0) HIP_TRY(hipMemcpy(d_dc, smp.dcand.data(), 2 * nd * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_ept, ept.data(), 2 * ne * sizeof(float), hipMemcpyHostToDevice));

  // one batch timed by four events of its own; the shape is known once the walks are laid out
  StatSlot* slot = nullptr;
  WOS_TRY(slot_open(c, st, 4, 1, RunShape{}, &slot));
  StatSlot& q = *slot;
  HIP_TRY(hipEventRecord(q.bev[0], st));
  const wos::DevScene& sc0 = s->dev;
  HIP_TRY(wos::launch_bvc_point_info(sc0, d_bpt, nb, d_bdd, nullptr, nullptr, nullptr, st));
  HIP_TRY(wos::launch_bvc_point_info(sc0, d_dc, nd, nullptr, nullptr, d_din, d_dsrc, st));
  HIP_TRY(wos::launch_bvc_point_info(sc0, d_ept, ne, d_edd, d_end, d_ein, nullptr, st));
  // the splat's packed point list; the outputs of every other point are 0
  uint32_t *d_slist = nullptr, *d_scount = nullptr;
  HIP_TRY(B.get(&d_slist, ne)); HIP_TRY(B.get(&d_scount, 1));
  HIP_TRY(hipMemsetAsync(d_scount, 0, sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_sol, 0, ne * sizeof(float), st));
  HIP_TRY(hipMemsetAsync(d_grad, 0, 2 * ne * sizeof(float), st));
  HIP_TRY(wos::launch_bvc_splat_list(d_edd, d_end, d_ein, ne, bp->normal_offset, prm->boundary_distance_mask,
                                     geom.double_sided, d_slist, d_scount, st));
  // the cache size is known once the domain candidates' inside test is: a samples buffer
  // too small for it fails here, before the walks, with counts[] filled for a retry
  // (one host round trip: the inside test and source of the domain candidates, the
  // evaluation points' Dirichlet distances)
  std::vector<float> dsrc(nd), edd_h(has_dir ? ne : 0);
  std::vector<int32_t> din(nd);
  if (nd > 0) {
    HIP_TRY(hipMemcpyAsync(din.data(), d_din, nd * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dsrc.data(), d_dsrc, nd * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  if (has_dir) HIP_TRY(hipMemcpyAsync(edd_h.data(), d_edd, ne * sizeof(float), hipMemcpyDeviceToHost, st));
  if (nd > 0 || has_dir) HIP_TRY(hipStreamSynchronize(st));
  std::vector<uint8_t> dkeep(nd);
  int64_t nd_keep = 0;
  for (int64_t i = 0; i < nd; i++) {
    const float x = smp.dcand[2 * i], y = smp.dcand[2 * i + 1];
    // insideSolveRegion (demo.cpp:302-304): the inside test, or the bounding box if double-sided
    dkeep[i] = geom.double_sided ? (x >= pmin[0] && y >= pmin[1] && x <= pmax[0] && y <= pmax[1]) : din[i] != 0;
    nd_keep += dkeep[i];
  }
  if (samples && samples_capacity < nb + nd_keep) {
    if (counts) { counts[0] = smp.nb_main; counts[1] = smp.nb_aligned; counts[2] = nd_keep; counts[3] = nb + nd_keep; }
    HIP_TRY(hipStreamSynchronize(st));
    c.inflight = false;
    q.ticket = 0;  // the slot holds no finished solve: wos_solve_stats on it reports an unknown ticket
    return fail(WOS_E_CAPACITY, "wos_bvc: samples buffer holds " + std::to_string(samples_capacity) + " of " +
                                    std::to_string(nb + nd_keep) + " samples (counts[3])");
  }
  // evaluation points within normalOffset of the Dirichlet boundary (splatter.h:160-196)
  std::vector<int64_t> near_idx;
  std::vector<float> near_pt;
  if (has_dir) {
    for (int64_t i = 0; i < ne; i++)
      if (edd_h[i] < bp->normal_offset) {
        near_idx.push_back(i);
        near_pt.push_back(ept[2 * i]);
        near_pt.push_back(ept[2 * i + 1]);
      }
  }
  const int64_t nn = (int64_t)near_idx.size();
  float *d_npt = nullptr, *d_ndd = nullptr, *d_nsol = nullptr;
  int32_t* d_nnest = nullptr;
  HIP_TRY(B.get(&d_npt, 2 * nn)); HIP_TRY(B.get(&d_ndd, nn)); HIP_TRY(B.get(&d_nsol, nn)); HIP_TRY(B.get(&d_nnest, nn));
  if (nn > 0) {
    std::vector<float> ndd(nn);
    for (int64_t k = 0; k < nn; k++) ndd[k] = edd_h[near_idx[k]];
    HIP_TRY(hipMemcpy(d_npt, near_pt.data(), 2 * nn * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ndd, ndd.data(), nn * sizeof(float), hipMemcpyHostToDevice));
  }

  // ---- the cache (splatter order): boundary samples (value = the solution, filled in on the
  // device once their walks are done; the Neumann value 0: pde.neumann, scene.h:176-181;
  // Dirichlet samples also their normal derivative), then the domain samples inside the
  // solve region (value = the source)
  std::vector<float> recs;
  recs.reserve((size_t)(nb + nd_keep) * wos::kBvcRec);
  for (int64_t i = 0; i < nb; i++) {
    const bool al = smp.aligned[i] != 0, dir = smp.dirichlet[i] != 0;
    const int kind = dir ? (al ? wos::kBvcDirichletAligned : wos::kBvcDirichlet) : (al ? wos::kBvcAligned : wos::kBvcBoundary);
    const float r[wos::kBvcRec] = {smp.bpt[2 * i], smp.bpt[2 * i + 1], smp.bnrm[2 * i], smp.bnrm[2 * i + 1],
                                   al ? smp.pdf_aligned : smp.pdf_main, 0.0f, 0.0f, (float)kind};
    recs.insert(recs.end(), r, r + wos::kBvcRec);
  }
  for (int64_t i = 0; i < nd; i++) {
    if (!dkeep[i]) continue;
    const float r[wos::kBvcRec] = {smp.dcand[2 * i], smp.dcand[2 * i + 1], 0.0f, 0.0f, smp.pdf_domain, dsrc[i], 0.0f,
                                   (float)wos::kBvcDomain};
    recs.insert(recs.end(), r, r + wos::kBvcRec);
  }
  const int64_t nd_kept = nd_keep;
  const int64_t nrec = nb + nd_kept;
  float *d_recs = nullptr, *d_state = nullptr;
  HIP_TRY(B.get(&d_recs, (size_t)nrec * wos::kBvcRec));
  HIP_TRY(B.get(&d_state, (size_t)18 * ne));
  if (nrec > 0) HIP_TRY(hipMemcpy(d_recs, recs.data(), recs.size() * sizeof(float), hipMemcpyHostToDevice));

  // ---- Three independent walk sets, on three streams (their tails overlap the others' bulk):
  //   bvc_dir            the Dirichlet samples' estimateSolutionAndGradient along the normal
  //                      (nWalksForCachedGradientEstimates, keyed by the sample index) on the
  //                      solve pipeline, solution and derivative unmasked;
  //   side[0]            estimateSolution walks (walk_on_stars.h:353-464) of the Neumann
  //                      boundary samples (nWalksForCachedSolutionEstimates, seed tag 6) and
  //                      the finite-difference Dirichlet samples (nWalksForCachedGradient-
  //                      Estimates, tag 8);
  //   side[1]            estimateSolution walks of the evaluation points near the Dirichlet
  //                      boundary (nWalksForCachedSolutionEstimates, tag 7, keyed by rank).
  // Every allocation (layout grids, jump table, workspaces) happens before the first launch:
  // hipFree / hipMalloc would serialise the streams.
  WalkLayout wl;
  wos_solver_params wp0 = *prm;
  WOS_TRY(walk_layout(s, &wp0, wl));
  wos::DevScene dsc = wl.dsc;
  if ((prm->schedule & WOS_SCHED_GEOM_GLOBAL) || wl.shmem_walk > kLdsDynamicMax) {
    dsc.geom_global = 1;
    wl.geom_floats_walk = 0;
    wl.shmem_walk = wos::kWavesPerBlockHost * wos::walk_wave_lds_bytes(2);
  }
  const bool dir_solve = has_dir && !bp->use_finite_differences;
  wos_solver_params gp = *prm;
  gp.n_walks = bp->n_walks_gradient;
  gp.boundary_distance_mask = 0.0f;
  {
    // the Dirichlet solves' stratified-sample draws (solve_locked) bound the table from above
    WOS_TRY(ensure_jump(c, std::max(4096, 4 * std::max(1, bp->n_walks_gradient))));
  }
  int64_t side_tasks[kSideWs] = {0, 0}, side_points[kSideWs] = {0, 0};
  const int64_t max_batch = g_max_batch_tasks.load();
  for (const Run& r : runs) {
    const int64_t m = r.b1 - r.b0;
    if (!r.dir || bp->use_finite_differences) {
      const int64_t w = r.dir ? bp->n_walks_gradient : bp->n_walks_solution;
      if (m * w > max_batch) return fail(WOS_E_CAPACITY, "wos_bvc: samples x nWalks exceed one task batch");
      side_tasks[0] = std::max(side_tasks[0], m * w);
      side_points[0] = std::max(side_points[0], m);
    } else if (dir_solve) {
      const int64_t wpp = gp.disable_gradient_antithetic_variates ? gp.n_walks : 2 * std::max(1, gp.n_walks / 2);
      const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(m, max_batch / wpp));
      WOS_TRY(ensure_tasks(c, 2, chunk * wpp, chunk));
    }
  }
  if (nn * bp->n_walks_solution > max_batch)
    return fail(WOS_E_CAPACITY, "wos_bvc: samples x nWalks exceed one task batch");
  side_tasks[1] = nn * bp->n_walks_solution;
  side_points[1] = nn;
  for (int k = 0; k < kSideWs; k++) {
    TaskWs& w = c.side[k];
    WOS_TRY(side_ready(w, bvc_priority(k == 0)));
    WOS_TRY(ensure_tasks_in(w.tasks, w.task_cap, w.pstate, w.pstate_cap, 2, side_tasks[k], side_points[k]));
  }
  if (!c.bvc_dir) HIP_TRY(hipStreamCreateWithPriority(&c.bvc_dir, hipStreamNonBlocking, bvc_priority(true)));
  if (!c.bvc_dir_done) HIP_TRY(hipEventCreateWithFlags(&c.bvc_dir_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(q.bev[1], st));
  HIP_TRY(hipStreamWaitEvent(c.bvc_dir, q.bev[1], 0));
  for (TaskWs& w : c.side) {
    HIP_TRY(hipStreamWaitEvent(w.stream, q.bev[1], 0));
    HIP_TRY(wos::launch_zero(w.counters, wos::kNumCounterSlots, nullptr, 0, w.stream));
  }

  std::vector<uint64_t> dtickets;
  if (dir_solve) {
    SolveExtra ex;
    ex.force_estimate = true;
    ex.wave_prio = 2;
    for (const Run& r : runs) {
      if (!r.dir) continue;
      ex.ddir = d_ddir + 2 * r.b0;
      ex.deriv = d_bdn + r.b0;
      wos_stats rs{};
      WOS_TRY(solve_locked(s, &gp, d_bpt + 2 * r.b0, r.b1 - r.b0, r.b0, 1, d_bsol + r.b0, d_dgrad, d_bnest + r.b0,
                           nullptr, &rs, c.bvc_dir, WOS_PTRS_DEVICE | WOS_ASYNC, ex));
      dtickets.push_back(rs.ticket);
    }
  }
  HIP_TRY(hipEventRecord(c.bvc_dir_done, c.bvc_dir));

  bool first_walk[kSideWs] = {true, true};
  auto walks = [&](int k, const float* pts_d, const float* nrm_d, const uint8_t* al_d, const float* dd_d, int64_t np_,
                   int64_t base, int n_walks, int on_neumann, uint32_t tag, float* sol_d, int32_t* nest_d) -> int {
    if (np_ <= 0) return WOS_OK;
    TaskWs& w = c.side[k];
    wos_solver_params wp = *prm;
    wp.n_walks = n_walks;
    wp.disable_gradient_antithetic_variates = 1;  // one walk per task, no pairs
    wos::DevParams dp = dev_params(&wp);
    dp.jump = c.d_jump;
    dp.n_jump = c.n_jump;
    dp.rej_tab = c.d_rejtab;
    // the Neumann samples' harmonic walks run longest (reflecting, up to maxWalkLength): top
    // issue priority; the near-boundary walks feed nothing downstream: none
    dp.wave_prio = k == 0 ? 3 : 0;
    const int64_t wpp = n_walks;
    wos::DevTasks tk = task_view_in(w.tasks, w.pstate, w.pstate_cap, 2, np_ * wpp, (int32_t)wpp);
    tk.n0 = tk.bdir;
    tk.r0 = tk.first;
    tk.sflags = reinterpret_cast<uint32_t*>(tk.sdir);
    // the walk queue's counters start at 0 for every launch
    if (!first_walk[k])
      HIP_TRY(wos::launch_zero(w.counters + wos::kNumCounters, wos::kNumCounterSlots - wos::kNumCounters, nullptr, 0,
                               w.stream));
    first_walk[k] = false;
    HIP_TRY(wos::launch_bvc_start(dsc, dp, pts_d, nrm_d, al_d, dd_d, np_, tk, on_neumann, tag, w.stream));
    int bpc = 0;
    const wos::KernelVariant kv = wos::kernel_variant(2, dsc, dp, true);
    HIP_TRY(wos::occupancy_blocks_per_cu(kv, 1, wl.shmem_walk, &bpc));
    const int grid = (int)std::min<int64_t>((int64_t)std::max(1, bpc) * std::max(1, c.num_cus), (tk.T + 63) / 64);
    unsigned int* q_tasks = (unsigned int*)(w.counters + wos::kTaskQueueSlot0);
    HIP_TRY(wos::launch_walks(kv, dsc, dp, tk, base, 1, w.counters, q_tasks, grid, wl.shmem_walk,
                              wl.geom_floats_walk, w.stream));
    HIP_TRY(wos::launch_bvc_fold(tk, np_, sol_d, nest_d, w.stream));
    q.shape.bpc_walk = bpc;
    return WOS_OK;
  };
  for (const Run& r : runs) {
    const int64_t m = r.b1 - r.b0;
    if (!r.dir)
      WOS_TRY(walks(0, d_bpt + 2 * r.b0, d_bnrm + 2 * r.b0, d_al + r.b0, d_bdd + r.b0, m, r.b0, bp->n_walks_solution, 1,
                    6u, d_bsol + r.b0, d_bnest + r.b0));
    else if (bp->use_finite_differences)
      WOS_TRY(walks(0, d_bpt + 2 * r.b0, d_bnrm + 2 * r.b0, d_al + r.b0, d_bdd + r.b0, m, r.b0, bp->n_walks_gradient, 0,
                    8u, d_bsol + r.b0, d_bnest + r.b0));
    if (r.dir && bp->use_finite_differences)
      HIP_TRY(wos::launch_bvc_fd(s->dev, d_bpt + 2 * r.b0, d_bsol + r.b0, m, d_bdn + r.b0, c.side[0].stream));
  }
  WOS_TRY(walks(1, d_npt, nullptr, nullptr, d_ndd, nn, 0, bp->n_walks_solution, 0, 7u, d_nsol, d_nnest));
  // no first-ball kernel; the walk kernel's residency is the last walk set's
  q.shape = RunShape{0, q.shape.bpc_walk, (int32_t)wl.shmem_walk, dsc.sgrid != nullptr, dsc.geom_global,
                     dsc.dgrid != nullptr};

  // ---- the splat in two launches over the cache order: the records whose values side[0]
  // estimates (the Neumann samples before the first Dirichlet sample of the solve; all the
  // boundary samples without one) as soon as side[0]'s walks are done, beside the
  // Dirichlet solve; then the rest on the call's stream, continuing the same statistics
  int64_t p1 = nb;
  if (dir_solve)
    for (int64_t i = 0; i < nb; i++)
      if (smp.dirichlet[i]) { p1 = i; break; }
  const float ab = s->dev.absorption;
  const bool part1 = p1 > 0, part1_last = p1 == nrec;
  if (part1) {
    HIP_TRY(wos::launch_bvc_fill(d_recs, 0, p1, d_bsol, d_bdn, s->dev, prm->ignore_neumann, c.side[0].stream));
    HIP_TRY(wos::launch_bvc_splat(d_recs, 0, (int)p1, 1, part1_last ? 1 : 0, d_state, d_slist, d_scount, d_ept, ne,
                                  ab, bp->radius_clamp, bp->kernel_regularization, d_sol, d_grad, c.side[0].stream));
  }
  for (TaskWs& w : c.side) HIP_TRY(hipEventRecord(w.done, w.stream));
  HIP_TRY(hipStreamWaitEvent(st, c.bvc_dir_done, 0));
  HIP_TRY(hipStreamWaitEvent(st, c.side[0].done, 0));
  HIP_TRY(hipEventRecord(q.bev[2], st));
  if (!(part1 && part1_last)) {
    HIP_TRY(wos::launch_bvc_fill(d_recs, p1, nb, d_bsol, d_bdn, s->dev, prm->ignore_neumann, st));
    HIP_TRY(wos::launch_bvc_splat(d_recs, part1 ? (int)p1 : 0, (int)nrec, part1 ? 0 : 1, 1, d_state, d_slist,
                                  d_scount, d_ept, ne, ab, bp->radius_clamp, bp->kernel_regularization, d_sol,
                                  d_grad, st));
  }
  std::vector<float> nsol(nn);
  HIP_TRY(hipStreamWaitEvent(st, c.side[1].done, 0));
  HIP_TRY(hipEventRecord(q.bev[3], st));
  // the walk counters of both side workspaces (summed below); the Dirichlet solves' own
  // counters are in their stat slots
  std::vector<unsigned long long> cnt1(wos::kNumCounters);
  WOS_TRY(slot_close(q, c.side[0].counters, st));
  HIP_TRY(hipMemcpyAsync(cnt1.data(), c.side[1].counters, wos::kNumCounters * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, st));
  if (nn > 0) HIP_TRY(hipMemcpyAsync(nsol.data(), d_nsol, nn * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(solution, d_sol, ne * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(grad, d_grad, 2 * ne * sizeof(float), hipMemcpyDeviceToHost, st));
  if (samples && nrec > 0)  // the cache with its estimated values
    HIP_TRY(hipMemcpyAsync(recs.data(), d_recs, recs.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  std::vector<float> end_h(nn > 0 ? ne : 0);
  std::vector<int32_t> ein_h(nn > 0 ? ne : 0);
  if (nn > 0) {
    HIP_TRY(hipMemcpyAsync(end_h.data(), d_end, ne * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ein_h.data(), d_ein, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  // always synchronous (st has waited for the three walk sets): nothing is left in flight
  HIP_TRY(hipEventRecord(q.done, st));
  HIP_TRY(hipStreamSynchronize(st));
  c.inflight = false;
  for (int k = 0; k < wos::kNumCounters; k++) q.h_cnt[k] += cnt1[k];
  wos::diag_dump("bvc");  // DIAG builds only
  wos::diag_dump_bstart("bvc-bstart");
  // the pointwise estimates near the Dirichlet boundary replace the (unsplatted) points'
  // statistics: solution = the estimate, gradient 0 (evalPt.reset, splatter.h:186-192),
  // then saveEvaluationGrid's mask (grid.h:404-408)
  for (int64_t k = 0; k < nn; k++) {
    const int64_t i = near_idx[k];
    const bool masked = (ein_h[i] == 0 && !geom.double_sided) ||
                        std::min(std::fabs(edd_h[i]), std::fabs(end_h[i])) < prm->boundary_distance_mask;
    solution[i] = masked ? 0.0f : nsol[k];
  }
  if (counts) { counts[0] = smp.nb_main; counts[1] = smp.nb_aligned; counts[2] = nd_kept; counts[3] = nrec; }
  if (stats) {
    WOS_TRY(fill_stats(q, stats));
    // the Dirichlet solves ran inside this call's span: their counters, not their times
    for (uint64_t t : dtickets) {
      const StatSlot& dq = c.slot[t % kStatSlots];
      if (dq.ticket != t) continue;
      wos_stats rs{};
      WOS_TRY(fill_stats(dq, &rs));
      stats_add_counters(stats, rs);
    }
    stats->points_estimated = (uint64_t)nb;  // the cached boundary samples, whoever estimated them
  }
  if (samples && nrec > 0) {
    if (samples_capacity < nrec)
      return fail(WOS_E_CAPACITY, "wos_bvc: samples buffer holds " + std::to_string(samples_capacity) + " of " +
                                      std::to_string(nrec) + " samples (counts[3])");
    std::memcpy(samples, recs.data(), recs.size() * sizeof(float));
  }
  return WOS_OK;
}

}  // extern "C"
