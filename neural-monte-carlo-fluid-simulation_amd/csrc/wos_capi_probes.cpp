// wos_capi_probes.cpp -- the self-test probes of the solve's kernels (wos_selftest_*, kernels in
// wos_selftest.hip): they need neither a scene's workspace nor the device context, and each call owns
// what it allocates.  The two SIREN probes are with their kernels' host half, wos_capi_siren.cpp.
// wos_selftest_geometry alone takes a scene: it plans it as a solve does (solve_plan) and launches
// its own kernel on that plan, touching nothing of the shared workspace.
#include "wos_capi.h"

using namespace wos::capi;

extern "C" {

int wos_selftest_math(int32_t which, const double* x, double* out, int64_t n, int32_t device) {
  if (!x || !out || n < 0) return fail(WOS_E_INVALID, "wos_selftest_math: bad argument");
  if (n == 0) return WOS_OK;
  HIP_TRY(hipSetDevice(device));
  double *dx = nullptr, *dy = nullptr;
  HIP_TRY(hipMalloc((void**)&dx, n * sizeof(double)));
  hipError_t e = hipMalloc((void**)&dy, n * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(dx, x, n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = wos::launch_math_selftest(which, dx, dy, n, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dy, n * sizeof(double), hipMemcpyDeviceToHost);
  hipFree(dx);
  hipFree(dy);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, std::string("wos_selftest_math: ") + hipGetErrorString(e));
  return WOS_OK;
}

int wos_selftest_simd_ids(int32_t device, uint32_t* out) {
  if (!out) return fail(WOS_E_INVALID, "wos_selftest_simd_ids: null output");
  constexpr int kWords = 2 * 4;  // (wos_selftest.hip: two words per wave of a 256-thread block)
  HIP_TRY(hipSetDevice(device));
  uint32_t* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, kWords * sizeof(uint32_t)));
  hipError_t e = wos::launch_simd_id_selftest(d, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d, kWords * sizeof(uint32_t), hipMemcpyDeviceToHost);
  hipFree(d);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, std::string("wos_selftest_simd_ids: ") + hipGetErrorString(e));
  return WOS_OK;
}

int wos_selftest_lhs(uint64_t key, const int64_t* gidx, int64_t n, int32_t n_pairs, int32_t dim, int32_t jump_lds,
                     float* out, int32_t device) {
  if (!gidx || !out || n < 0 || n > (1 << 20) || n_pairs < 1 || n_pairs > (1 << 14) || (dim != 2 && dim != 3))
    return fail(WOS_E_INVALID, "wos_selftest_lhs: bad argument");
  if (n == 0) return WOS_OK;
  // diagonal draws + shuffle draws, a table of exactly that many jump constants
  const int draws = 2 * (2 * n_pairs) * (dim - 1);
  const int jn = jump_lds ? std::min(draws, wos::kLhsJumpMax) : 0;
  // (the probe launches without raising the kernel's dynamic LDS limit)
  if (wos::lhs_selftest_lds_bytes(n_pairs, dim, jn) > 64 * 1024)
    return fail(WOS_E_CAPACITY, "wos_selftest_lhs: n_pairs exceed the probe's LDS");
  std::vector<uint64_t> t(2 * (size_t)draws);
  uint64_t A = 1u, Cc = 0u;
  for (int k = 0; k < draws; k++) {
    t[2 * k] = A; t[2 * k + 1] = Cc;
    A = A * wos::kPcgMult;
    Cc = Cc * wos::kPcgMult + wos::kPcgInc;
  }
  const size_t nout = (size_t)n * 2 * n_pairs * (dim - 1);
  HIP_TRY(hipSetDevice(device));
  uint64_t* dj = nullptr;
  long long* di = nullptr;
  float* dout = nullptr;
  hipError_t e = hipMalloc((void**)&dj, t.size() * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc((void**)&di, n * sizeof(long long));
  if (e == hipSuccess) e = hipMalloc((void**)&dout, nout * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(dj, t.data(), t.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(di, gidx, n * sizeof(long long), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    wos::DevParams dp{};
    dp.n_pairs = n_pairs;
    dp.n_walks = 2 * n_pairs;
    dp.n_anti = 2;
    dp.seed = key;
    dp.jump = dj;
    dp.n_jump = draws;
    dp.lhs_jump_n = jn;
    e = wos::launch_lhs_selftest(dim, dp, di, (int)n, dout, nullptr);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, nout * sizeof(float), hipMemcpyDeviceToHost);
  hipFree(dj);
  hipFree(di);
  hipFree(dout);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, std::string("wos_selftest_lhs: ") + hipGetErrorString(e));
  return WOS_OK;
}

int wos_selftest_lhs_permute(int32_t impl, const int32_t* partner, const float* values, int32_t nstrat, int32_t sd,
                             int32_t slots, int32_t count, float* out, int32_t device) {
  const int max_strata = wos::lhs_permute_selftest_max_strata(impl), cap = wos::lhs_permute_selftest_slots(impl);
  const bool packed = impl == WOS_LHS_PACK_R1 || impl == WOS_LHS_PACK_R2;
  if (!partner || !values || !out || count < 0 || count > (1 << 16))
    return fail(WOS_E_INVALID, "wos_selftest_lhs_permute: bad argument");
  if (max_strata == 0) return fail(WOS_E_INVALID, "wos_selftest_lhs_permute: unknown impl");
  if (nstrat < 1 || nstrat > max_strata)
    return fail(WOS_E_INVALID, "wos_selftest_lhs_permute: nstrat does not fit impl " + std::to_string(impl) + " (at most " +
                                   std::to_string(max_strata) + ")");
  if (sd < 1 || sd > 2 || (packed && sd != 2) || slots < 1 || slots > cap)
    return fail(WOS_E_INVALID, "wos_selftest_lhs_permute: sd or slots do not fit impl " + std::to_string(impl));
  if (count == 0) return WOS_OK;
  const size_t per = (size_t)cap * nstrat * sd, total = per * count;
  // the swap partner of step j is one of j .. nstrat - 1 (every slot's table is loaded)
  for (size_t k = 0; k < total; k++) {
    const int j = (int)(k % nstrat);
    if (partner[k] < j || partner[k] >= nstrat)
      return fail(WOS_E_INVALID, "wos_selftest_lhs_permute: partner out of range at " + std::to_string(k));
  }
  HIP_TRY(hipSetDevice(device));
  int* dp = nullptr;
  float *dv = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc((void**)&dp, total * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&dv, total * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&dout, total * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(dp, partner, total * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dv, values, total * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = wos::launch_lhs_permute_selftest(impl, dp, dv, nstrat, sd, slots, count, dout, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, total * sizeof(float), hipMemcpyDeviceToHost);
  hipFree(dp);
  hipFree(dv);
  hipFree(dout);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, std::string("wos_selftest_lhs_permute: ") + hipGetErrorString(e));
  return WOS_OK;
}

int wos_selftest_lhs_plan(int32_t n_pairs, int32_t dim, int32_t* out) {
  if (!out || n_pairs < 1 || n_pairs > (1 << 20) || (dim != 2 && dim != 3))
    return fail(WOS_E_INVALID, "wos_selftest_lhs_plan: bad argument");
  wos::lhs_plan(n_pairs, dim, out);
  out[6] = (int32_t)kLdsDynamicMax;
  return WOS_OK;
}

int wos_selftest_rejection(int32_t dim, const float* R, const float* lambda, const float* x, int64_t n, int32_t* edges,
                           float* vals, int32_t* flags, int32_t device) {
  if (!R || !lambda || !x || !edges || !vals || !flags || n < 0 || n > (1LL << 26) || (dim != 2 && dim != 3))
    return fail(WOS_E_INVALID, "wos_selftest_rejection: bad argument");
  if (n == 0) return WOS_OK;
  const std::vector<float>& tab = rejection_tables();
  const size_t N = (size_t)n;
  HIP_TRY(hipSetDevice(device));
  DevBufs tmp;
  float *d_tab = nullptr, *d_R = nullptr, *d_lam = nullptr, *d_x = nullptr, *d_vals = nullptr;
  int32_t *d_edges = nullptr, *d_flags = nullptr;
  HIP_TRY(tmp.get(&d_tab, tab.size()));
  HIP_TRY(tmp.get(&d_R, N));
  HIP_TRY(tmp.get(&d_lam, N));
  HIP_TRY(tmp.get(&d_x, N));
  HIP_TRY(tmp.get(&d_edges, N * 6));
  HIP_TRY(tmp.get(&d_vals, N * 3));
  HIP_TRY(tmp.get(&d_flags, N));
  HIP_TRY(hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_R, R, N * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_lam, lambda, N * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_x, x, N * 4, hipMemcpyHostToDevice));
  HIP_TRY(wos::launch_rejection_selftest(dim, d_tab, d_R, d_lam, d_x, n, d_edges, d_vals, d_flags, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(edges, d_edges, N * 6 * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(vals, d_vals, N * 3 * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(flags, d_flags, N * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

int wos_selftest_gfn(int32_t dim, int32_t mode, const float* items, int64_t n, float* out, int32_t device) {
  static_assert(WOS_GFN_ITEM == wos::kGfnItem && WOS_GFN_OUT == wos::kGfnOut, "include/wos.h and wos_launch.h agree");
  if (!items || !out || n < 0 || n > (1LL << 24) || (dim != 2 && dim != 3))
    return fail(WOS_E_INVALID, "wos_selftest_gfn: bad argument");
  if (mode != WOS_GFN_HARMONIC && mode != WOS_GFN_YUKAWA && mode != WOS_GFN_ROBUST)
    return fail(WOS_E_INVALID, "wos_selftest_gfn: mode must be WOS_GFN_HARMONIC (0), WOS_GFN_YUKAWA (1) or "
                               "WOS_GFN_ROBUST (2), got " + std::to_string(mode));
  if (n == 0) return WOS_OK;
  const size_t N = (size_t)n;
  HIP_TRY(hipSetDevice(device));
  DevBufs tmp;
  float *d_items = nullptr, *d_out = nullptr;
  HIP_TRY(tmp.get(&d_items, N * WOS_GFN_ITEM));
  HIP_TRY(tmp.get(&d_out, N * WOS_GFN_OUT));
  HIP_TRY(hipMemcpy(d_items, items, N * WOS_GFN_ITEM * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_out, 0, N * WOS_GFN_OUT * 4));
  HIP_TRY(wos::launch_gfn_selftest(dim, mode, d_items, n, d_out, nullptr));
  if (dim == 2) HIP_TRY(wos::launch_freespace_selftest(d_items, n, mode != WOS_GFN_HARMONIC, d_out, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_out, N * WOS_GFN_OUT * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

int wos_selftest_geometry(wos_scene* s, uint32_t schedule, float min_star_radius, float silhouette_precision,
                          int32_t kind, const float* items, int64_t n, const uint64_t* masks, int32_t n_masks,
                          float* out, int32_t* tags, uint32_t* sound, uint32_t* counts, int32_t* plan) {
  if (!s || !items || !masks || !out || !tags || !sound || !counts)
    return fail(WOS_E_INVALID, "wos_selftest_geometry: null argument");
  if (kind != WOS_GEO_RAY && kind != WOS_GEO_STAR && kind != WOS_GEO_DIRICHLET)
    return fail(WOS_E_INVALID, "wos_selftest_geometry: kind must be WOS_GEO_RAY (0), WOS_GEO_STAR (1) or "
                               "WOS_GEO_DIRICHLET (2), got " + std::to_string(kind));
  if (n < 0 || n > (1 << 20) || n_masks < 0 || n_masks > (1 << 20))
    return fail(WOS_E_INVALID, "wos_selftest_geometry: bad item or mask count");
  const wos::HostScene& host = s->geom->host;
  const int dim = host.dim;
  if (kind == WOS_GEO_DIRICHLET && host.n_dprims <= 0)
    return fail(WOS_E_INVALID, "wos_selftest_geometry: the scene holds no Dirichlet boundary");
  // the first item of every wave; the masks hold exactly the n items
  std::vector<int32_t> first((size_t)n_masks);
  int64_t bits = 0;
  for (int32_t w = 0; w < n_masks; w++) {
    first[w] = (int32_t)std::min<int64_t>(bits, n);
    bits += __builtin_popcountll(masks[w]);
  }
  if (bits != n)
    return fail(WOS_E_INVALID, "wos_selftest_geometry: the masks' set bits sum to " + std::to_string(bits) +
                                   ", not to n = " + std::to_string(n));
  wos_solver_params prm;
  wos_default_params(&prm);
  prm.schedule = schedule;
  prm.min_star_radius = min_star_radius;
  prm.silhouette_precision = silhouette_precision;
  WOS_TRY(check_params("wos_selftest_geometry", &prm));
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  WOS_TRY(ctx_ready(c, s->device));
  // the scene as a solve's walk kernel sees it
  SolvePlan P;
  WOS_TRY(solve_plan(c, s, &prm, SolveExtra{}, false, P));
  if (plan) {
    plan[0] = P.dsc.geom_global;
    plan[1] = P.dsc.sgrid != nullptr;
    plan[2] = P.dsc.dgrid != nullptr;
    plan[3] = (int32_t)P.shmem_walk;
    plan[4] = P.dsc.ptree.levels;
    plan[5] = P.dsc.stree.levels;
    plan[6] = P.dsc.dtree.levels;
    plan[7] = P.dsc.n_sil;
  }
  if (n == 0) return WOS_OK;
  const size_t N = (size_t)n;
  const size_t iw = kind == WOS_GEO_RAY ? 2 * dim + 1 : (kind == WOS_GEO_STAR ? dim + 2 : dim);
  DevBufs tmp;
  float *d_items = nullptr, *d_out = nullptr;
  unsigned long long* d_masks = nullptr;
  int32_t *d_first = nullptr, *d_tags = nullptr;
  uint32_t *d_sound = nullptr, *d_counts = nullptr;
  HIP_TRY(tmp.get(&d_items, N * iw));
  HIP_TRY(tmp.get(&d_masks, (size_t)n_masks));
  HIP_TRY(tmp.get(&d_first, (size_t)n_masks));
  HIP_TRY(tmp.get(&d_out, N * 3 * WOS_GEO_OUT));
  HIP_TRY(tmp.get(&d_tags, N));
  HIP_TRY(tmp.get(&d_sound, N));
  HIP_TRY(tmp.get(&d_counts, N * WOS_GEO_COUNTS));
  HIP_TRY(hipMemcpy(d_items, items, N * iw * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_masks, masks, (size_t)n_masks * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_first, first.data(), (size_t)n_masks * 4, hipMemcpyHostToDevice));
  HIP_TRY(wos::launch_geometry_selftest(dim, kind, P.dsc, P.dp, d_items, d_masks, d_first, n_masks, P.shmem_walk,
                                        P.geom_floats_walk, d_out, d_tags, d_sound, d_counts, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_out, N * 3 * WOS_GEO_OUT * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tags, d_tags, N * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sound, d_sound, N * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(counts, d_counts, N * WOS_GEO_COUNTS * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

int wos_selftest_sample_volume(int32_t dim, uint32_t variant, int32_t need_pdf, const float* items,
                               const uint32_t* seeds, int64_t n, const uint64_t* masks, int32_t n_masks, float* out,
                               uint64_t* state, uint32_t* iters, int32_t* tags, uint32_t* canary, int32_t* plan,
                               int32_t device) {
  if (!items || !seeds || !masks || !out || !state || !iters || !tags || !canary)
    return fail(WOS_E_INVALID, "wos_selftest_sample_volume: null argument");
  if (dim != 2 && dim != 3) return fail(WOS_E_INVALID, "wos_selftest_sample_volume: dim must be 2 or 3");
  if (variant & ~(WOS_SV_FB | WOS_SV_RB))
    return fail(WOS_E_INVALID, "wos_selftest_sample_volume: variant holds bits beyond WOS_SV_FB | WOS_SV_RB");
  if (n < 0 || n > (1 << 20) || n_masks < 0 || n_masks > (1 << 20))
    return fail(WOS_E_INVALID, "wos_selftest_sample_volume: bad item or mask count");
  // the first item of every wave; the masks name no item beyond the n given
  std::vector<int32_t> first((size_t)n_masks);
  int64_t bits = 0;
  for (int32_t w = 0; w < n_masks; w++) {
    first[w] = (int32_t)std::min<int64_t>(bits, n);
    bits += __builtin_popcountll(masks[w]);
  }
  if (bits > n)
    return fail(WOS_E_INVALID, "wos_selftest_sample_volume: the masks' set bits sum to " + std::to_string(bits) +
                                   ", more than n = " + std::to_string(n));
  const bool fb = (variant & WOS_SV_FB) != 0, rb = (variant & WOS_SV_RB) != 0;
  if (plan) wos::sample_volume_plan(dim, fb, plan);
  if (n == 0 || n_masks == 0) return WOS_OK;
  if (device < 0 || device >= kMaxDevices) return fail(WOS_E_INVALID, "wos_selftest_sample_volume: no such device");
  HIP_TRY(hipSetDevice(device));
  DevCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lk(c.mu);
  WOS_TRY(ctx_ready(c, device));
  // the jump table and the bound table of a solve's DevParams
  WOS_TRY(ensure_jump(c, 4096));
  wos::DevParams dp{};
  dp.jump = c.d_jump;
  dp.n_jump = c.n_jump;
  dp.rej_tab = c.d_rejtab;
  dp.robust = rb ? 1 : 0;
  const size_t N = (size_t)n, W = (size_t)n_masks;
  DevBufs tmp;
  float *d_items = nullptr, *d_out = nullptr;
  uint32_t *d_seeds = nullptr, *d_iters = nullptr, *d_canary = nullptr;
  unsigned long long *d_masks = nullptr, *d_state = nullptr;
  int32_t *d_first = nullptr, *d_tags = nullptr;
  HIP_TRY(tmp.get(&d_items, N * WOS_SV_ITEM));
  HIP_TRY(tmp.get(&d_seeds, N));
  HIP_TRY(tmp.get(&d_masks, W));
  HIP_TRY(tmp.get(&d_first, W));
  HIP_TRY(tmp.get(&d_out, N * 2 * WOS_SV_OUT));
  HIP_TRY(tmp.get(&d_state, N * 2));
  HIP_TRY(tmp.get(&d_iters, N * 2));
  HIP_TRY(tmp.get(&d_tags, N));
  HIP_TRY(tmp.get(&d_canary, W * 64));
  HIP_TRY(hipMemcpy(d_items, items, N * WOS_SV_ITEM * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_seeds, seeds, N * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_masks, masks, W * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_first, first.data(), W * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_out, 0, N * 2 * WOS_SV_OUT * 4));
  HIP_TRY(hipMemset(d_state, 0, N * 2 * 8));
  HIP_TRY(hipMemset(d_iters, 0, N * 2 * 4));
  HIP_TRY(hipMemset(d_tags, 0, N * 4));
  HIP_TRY(hipMemset(d_canary, 0, W * 64 * 4));
  HIP_TRY(wos::launch_sample_volume_selftest(dim, rb, fb, dp, need_pdf != 0, d_items, d_seeds, d_masks, d_first,
                                             n_masks, d_out, d_state, d_iters, d_tags, d_canary, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_out, N * 2 * WOS_SV_OUT * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(state, d_state, N * 2 * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(iters, d_iters, N * 2 * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tags, d_tags, N * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(canary, d_canary, W * 64 * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

int wos_selftest_tape_rowsum(const uint32_t* row, int64_t n_rows, const uint32_t* id, const float* w, const float* a,
                             const float* c, int64_t n_tasks, int32_t n_channels, float* out, int32_t* tile_terms,
                             int32_t device) {
  if (tile_terms) *tile_terms = wos::kTapeIndexTile;
  if (!row || !id || !w || !a || !c || !out) return fail(WOS_E_INVALID, "wos_selftest_tape_rowsum: null argument");
  if (n_rows < 1 || n_rows >= 0xFFFFFFFFLL || n_tasks < 1 || n_tasks > (1LL << 30) || n_channels < 1 ||
      n_channels > wos::kMaxChannels || row[0] != 0)
    return fail(WOS_E_INVALID, "wos_selftest_tape_rowsum: bad argument");
  for (int64_t r = 0; r < n_rows; r++)
    if (row[r + 1] < row[r]) return fail(WOS_E_INVALID, "wos_selftest_tape_rowsum: row offsets decrease at " + std::to_string(r));
  const uint32_t n_terms = row[n_rows];
  std::vector<uint32_t> cell(n_terms);
  for (int64_t r = 0; r < n_rows; r++)
    for (uint32_t i = row[r]; i < row[r + 1]; i++) cell[i] = (uint32_t)r;
  for (uint32_t i = 0; i < n_terms; i++)
    if ((int64_t)(id[i] & 0x7FFFFFFFu) >= n_tasks)
      return fail(WOS_E_INVALID, "wos_selftest_tape_rowsum: id out of range at " + std::to_string(i));
  HIP_TRY(hipSetDevice(device));
  DevBufs tmp;
  uint32_t *d_row = nullptr, *d_cell = nullptr, *d_id = nullptr;
  float *d_w = nullptr, *d_part = nullptr, *d_a = nullptr, *d_c = nullptr, *d_out = nullptr;
  const size_t ct = (size_t)n_channels * n_tasks, co = (size_t)n_channels * n_rows;
  HIP_TRY(tmp.get(&d_row, (size_t)n_rows + 1));
  HIP_TRY(tmp.get(&d_cell, n_terms));
  HIP_TRY(tmp.get(&d_id, n_terms));
  HIP_TRY(tmp.get(&d_w, n_terms));
  HIP_TRY(tmp.get(&d_part, (size_t)wos::tape_index_tiles(n_terms) * 2 * wos::kMaxChannels));
  HIP_TRY(tmp.get(&d_a, ct));
  HIP_TRY(tmp.get(&d_c, ct));
  HIP_TRY(tmp.get(&d_out, co));
  HIP_TRY(hipMemcpy(d_row, row, ((size_t)n_rows + 1) * 4, hipMemcpyHostToDevice));
  if (n_terms > 0) {
    HIP_TRY(hipMemcpy(d_cell, cell.data(), (size_t)n_terms * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_id, id, (size_t)n_terms * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_w, w, (size_t)n_terms * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(d_a, a, ct * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_c, c, ct * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_out, 0, co * 4));
  const wos::DevTapeIndex ix{d_row, d_cell, d_id, d_w, d_part, n_terms};
  HIP_TRY(wos::launch_tape_rowsum(ix, n_rows, n_channels, n_tasks, d_a, d_c, d_out, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_out, co * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

}  // extern "C"
