// wos_capi_probes.cpp -- entry points that need neither a scene's workspace nor the device context:
// the self-test probes (wos_selftest_*, kernels in wos_selftest.hip) and the fused SIREN
// (wos_siren_eval, wos_siren.hip; wos_siren_vjp, wos_siren_vjp.hip; wos_siren_fit, wos_siren_fit.hip;
// wos_adam_step, wos_siren_fit_run and wos_siren_fit_run_batches, wos_siren_train.hip).  Each call owns what it allocates.
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

// ---- fused SIREN (wos_siren.hip) -------------------------------------------------------------
static int siren_shape_check(const std::string& fn, int32_t d_in, int32_t hidden) {
  if (d_in != 2 && d_in != 3) return fail(WOS_E_INVALID, fn + ": d_in must be 2 or 3, got " + std::to_string(d_in));
  if (hidden < 32 || hidden > wos::kSirenMaxHidden || hidden % 32 != 0)
    return fail(WOS_E_INVALID, fn + ": hidden must be a multiple of 32 in 32.." + std::to_string(wos::kSirenMaxHidden) +
                                   ", got " + std::to_string(hidden));
  return WOS_OK;
}

// the envelope of both entry points: shape, omega and the pointer arrays
static int siren_net_check(const std::string& fn, const wos_siren_net* net) {
  if (!net) return fail(WOS_E_INVALID, fn + ": null net");
  if (int rc = siren_shape_check(fn, net->d_in, net->hidden)) return rc;
  if (net->d_out < 1 || net->d_out > 3)
    return fail(WOS_E_INVALID, fn + ": d_out must be 1..3, got " + std::to_string(net->d_out));
  if (net->n_hidden_layers < 0 || net->n_hidden_layers > wos::kSirenMaxHiddenLayers)
    return fail(WOS_E_INVALID, fn + ": n_hidden_layers must be 0.." + std::to_string(wos::kSirenMaxHiddenLayers) +
                                   ", got " + std::to_string(net->n_hidden_layers));
  if (!std::isfinite(net->omega)) return fail(WOS_E_INVALID, fn + ": omega must be finite");
  const int NL = net->n_hidden_layers + 2;
  if (!net->weights || !net->biases) return fail(WOS_E_INVALID, fn + ": null weights or biases array");
  for (int l = 0; l < NL; l++)
    if (!net->weights[l] || !net->biases[l])
      return fail(WOS_E_INVALID, fn + ": null weights or biases pointer of layer " + std::to_string(l));
  return WOS_OK;
}

// No scene, no workspace, no lock: the call owns what it allocates.  Device pointers: the packed
// weights are a stream-ordered allocation, so WOS_ASYNC needs no host wait to free them.  Host
// pointers: one staging allocation, freed after the call's own synchronise.
int wos_siren_eval(const wos_siren_net* net, const float* pts, int64_t n, float* u, float* jac, float* div,
                   uint32_t flags, int32_t device, void* stream) {
  const std::string fn = "wos_siren_eval";
  if (int rc = siren_net_check(fn, net)) return rc;
  const int D = net->d_in, DO = net->d_out, H = net->hidden, L = net->n_hidden_layers, NL = L + 2;
  if (!u && !jac && !div) return fail(WOS_E_INVALID, fn + ": no output requested (u, jac and div are all null)");
  if (div && DO != D)
    return fail(WOS_E_INVALID, fn + ": div needs d_out == d_in, got d_out " + std::to_string(DO) + ", d_in " +
                                   std::to_string(D));
  if (n < 0) return fail(WOS_E_INVALID, fn + ": negative point count");
  if (n > (int64_t)0x7FFFFFFF * wos::kSirenTile) return fail(WOS_E_INVALID, fn + ": too many points for one call");
  if (n == 0) return WOS_OK;
  if (!pts) return fail(WOS_E_INVALID, fn + ": null point buffer");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  wos::SirenNet dn{};
  dn.d_in = D;
  dn.d_out = DO;
  dn.H = H;
  dn.L = L;
  dn.omega = net->omega;
  const size_t pack_n = wos::siren_pack_floats(H, L);
  if (flags & WOS_PTRS_DEVICE) {
    for (int l = 0; l < NL; l++) { dn.w[l] = net->weights[l]; dn.b[l] = net->biases[l]; }
    float* packed = nullptr;
    if (pack_n > 0) HIP_TRY(hipMallocAsync((void**)&packed, pack_n * sizeof(float), st));
    hipError_t e = wos::launch_siren_pack(dn, packed, st);
    if (e == hipSuccess) e = wos::launch_siren_eval(dn, packed, pts, n, u, jac, div, st);
    if (packed) {
      const hipError_t e2 = hipFreeAsync(packed, st);
      if (e == hipSuccess) e = e2;
    }
    if (e == hipSuccess && !(flags & WOS_ASYNC)) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
    return WOS_OK;
  }
  // one temporary: packed | weights and biases layer by layer | pts | u | jac | div (floats)
  const size_t N = (size_t)n;
  size_t o_w[wos::kSirenMaxLayers], o_b[wos::kSirenMaxLayers], n_w[wos::kSirenMaxLayers], n_b[wos::kSirenMaxLayers];
  size_t off = pack_n;
  for (int l = 0; l < NL; l++) {
    n_b[l] = l == NL - 1 ? (size_t)DO : (size_t)H;
    n_w[l] = n_b[l] * (l == 0 ? (size_t)D : (size_t)H);
    o_w[l] = off;
    off += n_w[l];
    o_b[l] = off;
    off += n_b[l];
  }
  const size_t o_pts = off, o_u = o_pts + N * D, o_j = o_u + (u ? N * DO : 0), o_d = o_j + (jac ? N * DO * D : 0),
               total = o_d + (div ? N : 0);
  float* tmp = nullptr;
  if (hipMalloc((void**)&tmp, total * sizeof(float)) != hipSuccess)
    return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string(total * sizeof(float)) + " bytes of staging");
  const auto run = [&]() -> hipError_t {
    hipError_t e;
    for (int l = 0; l < NL; l++) {
      if ((e = hipMemcpyAsync(tmp + o_w[l], net->weights[l], n_w[l] * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess)
        return e;
      if ((e = hipMemcpyAsync(tmp + o_b[l], net->biases[l], n_b[l] * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess)
        return e;
      dn.w[l] = tmp + o_w[l];
      dn.b[l] = tmp + o_b[l];
    }
    if ((e = hipMemcpyAsync(tmp + o_pts, pts, N * D * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
    if ((e = wos::launch_siren_pack(dn, tmp, st)) != hipSuccess) return e;
    if ((e = wos::launch_siren_eval(dn, tmp, tmp + o_pts, n, u ? tmp + o_u : nullptr, jac ? tmp + o_j : nullptr,
                                    div ? tmp + o_d : nullptr, st)) != hipSuccess)
      return e;
    if (u && (e = hipMemcpyAsync(u, tmp + o_u, N * DO * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if (jac && (e = hipMemcpyAsync(jac, tmp + o_j, N * DO * D * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess)
      return e;
    if (div && (e = hipMemcpyAsync(div, tmp + o_d, N * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    return hipStreamSynchronize(st);
  };
  const hipError_t e = run();
  if (e != hipSuccess) hipStreamSynchronize(st);  // nothing may still use tmp when it is freed
  hipFree(tmp);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
  return WOS_OK;
}

int wos_selftest_siren_layer(int32_t hidden, int32_t d_in, int64_t n_points, const float* W, const float* b,
                             const float* X, float* Z, int32_t device) {
  const std::string fn = "wos_selftest_siren_layer";
  if (int rc = siren_shape_check(fn, d_in, hidden)) return rc;
  if (!W || !b || !X || !Z) return fail(WOS_E_INVALID, fn + ": null argument");
  if (n_points < 1 || n_points > (1LL << 20)) return fail(WOS_E_INVALID, fn + ": n_points must be 1..2^20");
  HIP_TRY(hipSetDevice(device));
  DevBufs tmp;
  const size_t hh = (size_t)hidden * hidden, nx = (size_t)n_points * (1 + d_in) * hidden;
  float *d_W = nullptr, *d_b = nullptr, *d_pack = nullptr, *d_X = nullptr, *d_Z = nullptr;
  HIP_TRY(tmp.get(&d_W, hh));
  HIP_TRY(tmp.get(&d_b, (size_t)hidden));
  HIP_TRY(tmp.get(&d_pack, hh));
  HIP_TRY(tmp.get(&d_X, nx));
  HIP_TRY(tmp.get(&d_Z, nx));
  HIP_TRY(hipMemcpy(d_W, W, hh * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_b, b, (size_t)hidden * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_X, X, nx * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_Z, 0, nx * 4));
  HIP_TRY(wos::launch_siren_layer_selftest(hidden, d_in, n_points, d_W, d_b, d_pack, d_X, d_Z, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(Z, d_Z, nx * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

// ---- fused SIREN backward (wos_siren_vjp.hip) ------------------------------------------------
constexpr size_t kSirenVjpDefaultStash = (size_t)256 << 20;  // the stash's cap when workspace_bytes is 0

// One temporary per call: packed | packedT | H zeros | the plan's work; with host pointers also
// the staged network, points, cotangents and gradients.  Stream-ordered with device pointers.
int wos_siren_vjp(const wos_siren_net* net, const float* pts, int64_t n, const float* g_u, const float* g_jac,
                  const float* g_div, float* const* grad_weights, float* const* grad_biases, size_t workspace_bytes,
                  uint32_t flags, int32_t device, void* stream) {
  const std::string fn = "wos_siren_vjp";
  if (int rc = siren_net_check(fn, net)) return rc;
  const int D = net->d_in, DO = net->d_out, H = net->hidden, L = net->n_hidden_layers, NL = L + 2;
  if (!g_u && !g_jac && !g_div)
    return fail(WOS_E_INVALID, fn + ": no cotangent given (g_u, g_jac and g_div are all null)");
  if (g_div && DO != D)
    return fail(WOS_E_INVALID, fn + ": g_div needs d_out == d_in, got d_out " + std::to_string(DO) + ", d_in " +
                                   std::to_string(D));
  if (!grad_weights || !grad_biases) return fail(WOS_E_INVALID, fn + ": null grad_weights or grad_biases array");
  for (int l = 0; l < NL; l++)
    if (!grad_weights[l] || !grad_biases[l])
      return fail(WOS_E_INVALID, fn + ": null grad_weights or grad_biases pointer of layer " + std::to_string(l));
  if (n < 0) return fail(WOS_E_INVALID, fn + ": n is negative");
  if (n > (int64_t)0x7FFFFFFF * wos::kSirenTile) return fail(WOS_E_INVALID, fn + ": n: too many points for one call");
  const size_t tile_bytes = wos::siren_vjp_stash_floats_per_tile(D, H, L) * sizeof(float);
  if (workspace_bytes != 0 && workspace_bytes < tile_bytes)
    return fail(WOS_E_CAPACITY, fn + ": workspace_bytes " + std::to_string(workspace_bytes) +
                                    " cannot hold one tile's stash of " + std::to_string(tile_bytes) + " bytes");
  if (n > 0 && !pts) return fail(WOS_E_INVALID, fn + ": null point buffer");
  size_t n_w[wos::kSirenMaxLayers], n_b[wos::kSirenMaxLayers];
  for (int l = 0; l < NL; l++) {
    n_b[l] = l == NL - 1 ? (size_t)DO : (size_t)H;
    n_w[l] = n_b[l] * (l == 0 ? (size_t)D : (size_t)H);
  }
  const bool dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  if (n == 0 && !dev_ptrs) {
    for (int l = 0; l < NL; l++) {
      std::fill(grad_weights[l], grad_weights[l] + n_w[l], 0.0f);
      std::fill(grad_biases[l], grad_biases[l] + n_b[l], 0.0f);
    }
    return WOS_OK;
  }
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  wos::SirenNet dn{};
  dn.d_in = D;
  dn.d_out = DO;
  dn.H = H;
  dn.L = L;
  dn.omega = net->omega;
  wos::SirenGrads dg{};
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int per_cu = std::max<int>(1, (int)(kLdsDynamicMax / wos::siren_vjp_tile_lds_bytes(D, H)));
  const wos::SirenVjpPlan plan =
      wos::siren_vjp_plan(dn, n, workspace_bytes ? workspace_bytes : kSirenVjpDefaultStash, cus * per_cu);
  const size_t pack_n = wos::siren_pack_floats(H, L);
  const size_t o_packT = pack_n, o_zero = 2 * pack_n, o_work = o_zero + (size_t)H, dev_total = o_work + plan.total();
  const auto run = [&](float* tmp, const float* d_pts, const float* d_gu, const float* d_gj, const float* d_gd) -> hipError_t {
    if (n == 0) return wos::launch_siren_vjp(dn, nullptr, nullptr, nullptr, nullptr, 0, d_gu, d_gj, d_gd, dg, plan, nullptr, st);
    hipError_t e;
    if ((e = hipMemsetAsync(tmp + o_zero, 0, (size_t)H * sizeof(float), st)) != hipSuccess) return e;
    if ((e = wos::launch_siren_pack(dn, tmp, st)) != hipSuccess) return e;
    if ((e = wos::launch_siren_pack_transposed(dn, tmp + o_packT, st)) != hipSuccess) return e;
    return wos::launch_siren_vjp(dn, tmp, tmp + o_packT, tmp + o_zero, d_pts, n, d_gu, d_gj, d_gd, dg, plan, tmp + o_work, st);
  };
  if (dev_ptrs) {
    for (int l = 0; l < NL; l++) {
      dn.w[l] = net->weights[l];
      dn.b[l] = net->biases[l];
      dg.w[l] = grad_weights[l];
      dg.b[l] = grad_biases[l];
    }
    float* tmp = nullptr;
    if (n > 0 && hipMallocAsync((void**)&tmp, dev_total * sizeof(float), st) != hipSuccess)
      return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string(dev_total * sizeof(float)) + " bytes of workspace");
    hipError_t e = run(tmp, pts, g_u, g_jac, g_div);
    if (tmp) {
      const hipError_t e2 = hipFreeAsync(tmp, st);
      if (e == hipSuccess) e = e2;
    }
    if (e == hipSuccess && !(flags & WOS_ASYNC)) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
    return WOS_OK;
  }
  // host pointers: ... | weights, biases and their gradients layer by layer | pts | g_u | g_jac | g_div
  const size_t N = (size_t)n;
  size_t o_w[wos::kSirenMaxLayers], o_b[wos::kSirenMaxLayers], o_gw[wos::kSirenMaxLayers], o_gb[wos::kSirenMaxLayers];
  size_t off = dev_total;
  for (int l = 0; l < NL; l++) {
    o_w[l] = off;
    off += n_w[l];
    o_b[l] = off;
    off += n_b[l];
    o_gw[l] = off;
    off += n_w[l];
    o_gb[l] = off;
    off += n_b[l];
  }
  const size_t o_pts = off, o_u = o_pts + N * D, o_j = o_u + (g_u ? N * DO : 0), o_d = o_j + (g_jac ? N * DO * D : 0),
               total = o_d + (g_div ? N : 0);
  float* tmp = nullptr;
  if (hipMalloc((void**)&tmp, total * sizeof(float)) != hipSuccess)
    return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string(total * sizeof(float)) + " bytes of staging");
  const auto staged = [&]() -> hipError_t {
    hipError_t e;
    const auto up = [&](size_t o, const float* src, size_t count) {
      return hipMemcpyAsync(tmp + o, src, count * sizeof(float), hipMemcpyHostToDevice, st);
    };
    for (int l = 0; l < NL; l++) {
      if ((e = up(o_w[l], net->weights[l], n_w[l])) != hipSuccess) return e;
      if ((e = up(o_b[l], net->biases[l], n_b[l])) != hipSuccess) return e;
      dn.w[l] = tmp + o_w[l];
      dn.b[l] = tmp + o_b[l];
      dg.w[l] = tmp + o_gw[l];
      dg.b[l] = tmp + o_gb[l];
    }
    if ((e = up(o_pts, pts, N * D)) != hipSuccess) return e;
    if (g_u && (e = up(o_u, g_u, N * DO)) != hipSuccess) return e;
    if (g_jac && (e = up(o_j, g_jac, N * DO * D)) != hipSuccess) return e;
    if (g_div && (e = up(o_d, g_div, N)) != hipSuccess) return e;
    if ((e = run(tmp, tmp + o_pts, g_u ? tmp + o_u : nullptr, g_jac ? tmp + o_j : nullptr, g_div ? tmp + o_d : nullptr)) !=
        hipSuccess)
      return e;
    for (int l = 0; l < NL; l++) {
      if ((e = hipMemcpyAsync(grad_weights[l], dg.w[l], n_w[l] * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return e;
      if ((e = hipMemcpyAsync(grad_biases[l], dg.b[l], n_b[l] * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return e;
    }
    return hipStreamSynchronize(st);
  };
  const hipError_t e = staged();
  if (e != hipSuccess) hipStreamSynchronize(st);  // nothing may still use tmp when it is freed
  hipFree(tmp);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
  return WOS_OK;
}

// ---- fused SIREN fit step (wos_siren_fit.hip) ------------------------------------------------
// One temporary per call: packed | packedT | H zeros | the plan's work (loss only: packed | the
// tiles' sums); with host pointers also the staged network, points, target, scale, loss and
// gradients.  Stream-ordered with device pointers.
int wos_siren_fit(const wos_siren_net* net, const float* pts, int64_t n, const float* target, const float* scale,
                  float* loss, float* const* grad_weights, float* const* grad_biases, size_t workspace_bytes,
                  uint32_t flags, int32_t device, void* stream) {
  const std::string fn = "wos_siren_fit";
  if (int rc = siren_net_check(fn, net)) return rc;
  const int D = net->d_in, DO = net->d_out, H = net->hidden, L = net->n_hidden_layers, NL = L + 2;
  if (!loss) return fail(WOS_E_INVALID, fn + ": null loss");
  if (!target) return fail(WOS_E_INVALID, fn + ": null target");
  if ((grad_weights == nullptr) != (grad_biases == nullptr))
    return fail(WOS_E_INVALID, fn + ": exactly one of grad_weights and grad_biases is null (both null: the loss alone)");
  const bool grads = grad_weights != nullptr;
  if (grads)
    for (int l = 0; l < NL; l++)
      if (!grad_weights[l] || !grad_biases[l])
        return fail(WOS_E_INVALID, fn + ": null grad_weights or grad_biases pointer of layer " + std::to_string(l));
  if (n <= 0) return fail(WOS_E_INVALID, fn + ": n must be positive (a mean over nothing), got " + std::to_string(n));
  if (n > (int64_t)0x7FFFFFFF * wos::kSirenTile) return fail(WOS_E_INVALID, fn + ": n: too many points for one call");
  const size_t tile_bytes = wos::siren_fit_stash_floats_per_tile(H, L) * sizeof(float);
  if (workspace_bytes != 0 && workspace_bytes < tile_bytes)
    return fail(WOS_E_CAPACITY, fn + ": workspace_bytes " + std::to_string(workspace_bytes) +
                                    " cannot hold one tile's stash of " + std::to_string(tile_bytes) + " bytes");
  if (!pts) return fail(WOS_E_INVALID, fn + ": null point buffer");
  size_t n_w[wos::kSirenMaxLayers], n_b[wos::kSirenMaxLayers];
  for (int l = 0; l < NL; l++) {
    n_b[l] = l == NL - 1 ? (size_t)DO : (size_t)H;
    n_w[l] = n_b[l] * (l == 0 ? (size_t)D : (size_t)H);
  }
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  wos::SirenNet dn{};
  dn.d_in = D;
  dn.d_out = DO;
  dn.H = H;
  dn.L = L;
  dn.omega = net->omega;
  wos::SirenGrads dg{};
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int per_cu = std::max<int>(1, (int)(kLdsDynamicMax / wos::siren_fit_tile_lds_bytes(D, H)));
  const wos::SirenFitPlan plan =
      wos::siren_fit_plan(dn, n, workspace_bytes ? workspace_bytes : kSirenVjpDefaultStash, cus * per_cu);
  const size_t pack_n = wos::siren_pack_floats(H, L);
  const size_t o_packT = pack_n, o_zero = 2 * pack_n, o_work = grads ? o_zero + (size_t)H : pack_n,
               dev_total = o_work + plan.total(grads);
  const auto run = [&](float* tmp, const float* d_pts, const float* d_target, const float* d_scale, float* d_loss) -> hipError_t {
    hipError_t e;
    if ((e = wos::launch_siren_pack(dn, tmp, st)) != hipSuccess) return e;
    if (!grads)
      return wos::launch_siren_fit(dn, tmp, nullptr, nullptr, d_pts, n, d_target, d_scale, d_loss, nullptr, plan, tmp + o_work, st);
    if ((e = hipMemsetAsync(tmp + o_zero, 0, (size_t)H * sizeof(float), st)) != hipSuccess) return e;
    if ((e = wos::launch_siren_pack_transposed(dn, tmp + o_packT, st)) != hipSuccess) return e;
    return wos::launch_siren_fit(dn, tmp, tmp + o_packT, tmp + o_zero, d_pts, n, d_target, d_scale, d_loss, &dg, plan,
                                 tmp + o_work, st);
  };
  if (flags & WOS_PTRS_DEVICE) {
    for (int l = 0; l < NL; l++) {
      dn.w[l] = net->weights[l];
      dn.b[l] = net->biases[l];
      if (grads) {
        dg.w[l] = grad_weights[l];
        dg.b[l] = grad_biases[l];
      }
    }
    float* tmp = nullptr;
    if (hipMallocAsync((void**)&tmp, dev_total * sizeof(float), st) != hipSuccess)
      return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string(dev_total * sizeof(float)) + " bytes of workspace");
    hipError_t e = run(tmp, pts, target, scale, loss);
    const hipError_t e2 = hipFreeAsync(tmp, st);
    if (e == hipSuccess) e = e2;
    if (e == hipSuccess && !(flags & WOS_ASYNC)) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
    return WOS_OK;
  }
  // host pointers: ... | weights, biases and their gradients layer by layer | pts | target | scale | loss
  const size_t N = (size_t)n;
  size_t o_w[wos::kSirenMaxLayers], o_b[wos::kSirenMaxLayers], o_gw[wos::kSirenMaxLayers], o_gb[wos::kSirenMaxLayers];
  size_t off = dev_total;
  for (int l = 0; l < NL; l++) {
    o_w[l] = off;
    off += n_w[l];
    o_b[l] = off;
    off += n_b[l];
    o_gw[l] = off;
    off += grads ? n_w[l] : 0;
    o_gb[l] = off;
    off += grads ? n_b[l] : 0;
  }
  const size_t o_pts = off, o_t = o_pts + N * D, o_s = o_t + N * DO, o_loss = o_s + (scale ? N * DO : 0), total = o_loss + 1;
  float* tmp = nullptr;
  if (hipMalloc((void**)&tmp, total * sizeof(float)) != hipSuccess)
    return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string(total * sizeof(float)) + " bytes of staging");
  const auto staged = [&]() -> hipError_t {
    hipError_t e;
    const auto up = [&](size_t o, const float* src, size_t count) {
      return hipMemcpyAsync(tmp + o, src, count * sizeof(float), hipMemcpyHostToDevice, st);
    };
    for (int l = 0; l < NL; l++) {
      if ((e = up(o_w[l], net->weights[l], n_w[l])) != hipSuccess) return e;
      if ((e = up(o_b[l], net->biases[l], n_b[l])) != hipSuccess) return e;
      dn.w[l] = tmp + o_w[l];
      dn.b[l] = tmp + o_b[l];
      dg.w[l] = tmp + o_gw[l];
      dg.b[l] = tmp + o_gb[l];
    }
    if ((e = up(o_pts, pts, N * D)) != hipSuccess) return e;
    if ((e = up(o_t, target, N * DO)) != hipSuccess) return e;
    if (scale && (e = up(o_s, scale, N * DO)) != hipSuccess) return e;
    if ((e = run(tmp, tmp + o_pts, tmp + o_t, scale ? tmp + o_s : nullptr, tmp + o_loss)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(loss, tmp + o_loss, sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    for (int l = 0; grads && l < NL; l++) {
      if ((e = hipMemcpyAsync(grad_weights[l], dg.w[l], n_w[l] * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return e;
      if ((e = hipMemcpyAsync(grad_biases[l], dg.b[l], n_b[l] * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess)
        return e;
    }
    return hipStreamSynchronize(st);
  };
  const hipError_t e = staged();
  if (e != hipSuccess) hipStreamSynchronize(st);  // nothing may still use tmp when it is freed
  hipFree(tmp);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
  return WOS_OK;
}

int wos_selftest_siren_vjp_layer(int32_t hidden, int32_t d_in, int64_t n_points, const float* W, const float* dZ,
                                 const float* X, float* dX, float* dW, int32_t device) {
  const std::string fn = "wos_selftest_siren_vjp_layer";
  if (int rc = siren_shape_check(fn, d_in, hidden)) return rc;
  if (!W || !dZ || !X || !dX || !dW) return fail(WOS_E_INVALID, fn + ": null argument");
  if (n_points < 1 || n_points > (1LL << 16)) return fail(WOS_E_INVALID, fn + ": n_points must be 1..2^16");
  HIP_TRY(hipSetDevice(device));
  DevBufs tmp;
  const size_t hh = (size_t)hidden * hidden, nx = (size_t)n_points * (1 + d_in) * hidden;
  float *d_W = nullptr, *d_zero = nullptr, *d_pack = nullptr, *d_dZ = nullptr, *d_X = nullptr, *d_dX = nullptr,
        *d_dW = nullptr, *d_work = nullptr;
  HIP_TRY(tmp.get(&d_W, hh));
  HIP_TRY(tmp.get(&d_zero, (size_t)hidden));
  HIP_TRY(tmp.get(&d_pack, hh));
  HIP_TRY(tmp.get(&d_dZ, nx));
  HIP_TRY(tmp.get(&d_X, nx));
  HIP_TRY(tmp.get(&d_dX, nx));
  HIP_TRY(tmp.get(&d_dW, hh));
  HIP_TRY(tmp.get(&d_work, wos::siren_vjp_layer_selftest_floats(hidden, d_in, n_points)));
  HIP_TRY(hipMemcpy(d_W, W, hh * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_zero, 0, (size_t)hidden * 4));
  HIP_TRY(hipMemcpy(d_dZ, dZ, nx * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_X, X, nx * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_dX, 0, nx * 4));
  HIP_TRY(hipMemset(d_dW, 0, hh * 4));
  HIP_TRY(wos::launch_siren_vjp_layer_selftest(hidden, d_in, n_points, d_W, d_pack, d_zero, d_dZ, d_X, d_dX, d_dW, d_work,
                                               nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(dX, d_dX, nx * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(dW, d_dW, hh * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

// ---- fused Adam step and the device-resident fit loop (wos_siren_train.hip) --------------------
static_assert(wos::kAdamMaxTensors == 20, "include/wos.h documents n_tensors as 1..20");
static_assert(sizeof(wos_adam_params) == 5 * sizeof(double), "wos_adam_params is five doubles (wos_amd/_lib.py AdamParams)");
static_assert(sizeof(wos::AdamSegs) + sizeof(wos::AdamScalars) + 4 * sizeof(void*) <= 4096,
              "adam_update_kernel's arguments, the segment table included, fit the kernel argument segment");
static int adam_params_check(const std::string& fn, const wos_adam_params* opt) {
  if (!opt) return fail(WOS_E_INVALID, fn + ": null opt");
  if (!std::isfinite(opt->lr)) return fail(WOS_E_INVALID, fn + ": lr must be finite");
  if (!(opt->beta1 >= 0.0 && opt->beta1 < 1.0))
    return fail(WOS_E_INVALID, fn + ": beta1 must be in [0, 1), got " + std::to_string(opt->beta1));
  if (!(opt->beta2 >= 0.0 && opt->beta2 < 1.0))
    return fail(WOS_E_INVALID, fn + ": beta2 must be in [0, 1), got " + std::to_string(opt->beta2));
  if (!(opt->eps >= 0.0) || !std::isfinite(opt->eps))
    return fail(WOS_E_INVALID, fn + ": eps must be finite and >= 0, got " + std::to_string(opt->eps));
  if (!std::isfinite(opt->max_grad_norm)) return fail(WOS_E_INVALID, fn + ": max_grad_norm must be finite");
  return WOS_OK;
}

// the step's five scalars in double from the double parameters, each rounded to float once
static wos::AdamScalars adam_scalars(const wos_adam_params& o, int64_t step) {
  wos::AdamScalars s{};
  s.b2 = (float)o.beta2;
  s.omb1 = (float)(1.0 - o.beta1);
  s.omb2 = (float)(1.0 - o.beta2);
  s.bc2 = (float)std::sqrt(1.0 - std::pow(o.beta2, (double)step));
  s.ss = (float)(o.lr / (1.0 - std::pow(o.beta1, (double)step)));
  s.eps = (float)o.eps;
  s.max_norm = (float)o.max_grad_norm;
  return s;
}

// Device pointers: stream-ordered, one float of scratch only when clipping without grad_norm.
// Host pointers: one staging allocation -- params | grads | exp_avg | exp_avg_sq | norm.
int wos_adam_step(int32_t n_tensors, const int64_t* counts, float* const* params, const float* const* grads,
                  float* exp_avg, float* exp_avg_sq, int64_t step, const wos_adam_params* opt, float* grad_norm,
                  uint32_t flags, int32_t device, void* stream) {
  const std::string fn = "wos_adam_step";
  if (n_tensors < 1 || n_tensors > wos::kAdamMaxTensors)
    return fail(WOS_E_INVALID, fn + ": n_tensors must be 1.." + std::to_string(wos::kAdamMaxTensors) + ", got " +
                                   std::to_string(n_tensors));
  if (!counts) return fail(WOS_E_INVALID, fn + ": null counts");
  if (!params) return fail(WOS_E_INVALID, fn + ": null params array");
  if (!grads) return fail(WOS_E_INVALID, fn + ": null grads array");
  if (!exp_avg) return fail(WOS_E_INVALID, fn + ": null exp_avg");
  if (!exp_avg_sq) return fail(WOS_E_INVALID, fn + ": null exp_avg_sq");
  wos::AdamSegs segs{};
  segs.n = n_tensors;
  int64_t total = 0;
  for (int k = 0; k < n_tensors; k++) {
    if (counts[k] <= 0 || counts[k] > (int64_t)1 << 40)
      return fail(WOS_E_INVALID, fn + ": counts[" + std::to_string(k) + "] must be positive (at most 2^40), got " +
                                     std::to_string(counts[k]));
    if (!params[k]) return fail(WOS_E_INVALID, fn + ": null params pointer of tensor " + std::to_string(k));
    if (!grads[k]) return fail(WOS_E_INVALID, fn + ": null grads pointer of tensor " + std::to_string(k));
    total += counts[k];
    segs.end[k] = total;
  }
  if (step < 1) return fail(WOS_E_INVALID, fn + ": step must be >= 1 (the step being taken), got " + std::to_string(step));
  if (int rc = adam_params_check(fn, opt)) return rc;
  const bool clip = opt->max_grad_norm > 0.0;
  const wos::AdamScalars sc = adam_scalars(*opt, step);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const auto run = [&](float* m, float* v, float* norm) -> hipError_t {
    hipError_t e;
    if (clip && (e = wos::launch_adam_norm(segs, norm, st)) != hipSuccess) return e;
    return wos::launch_adam_update(segs, m, v, sc, clip ? norm : nullptr, nullptr, st);
  };
  if (flags & WOS_PTRS_DEVICE) {
    for (int k = 0; k < n_tensors; k++) {
      segs.p[k] = params[k];
      segs.g[k] = grads[k];
    }
    float* scratch = nullptr;
    if (clip && !grad_norm && hipMallocAsync((void**)&scratch, sizeof(float), st) != hipSuccess)
      return fail(WOS_E_NOMEM, fn + ": cannot allocate the norm's scratch word");
    hipError_t e = run(exp_avg, exp_avg_sq, grad_norm ? grad_norm : scratch);
    if (scratch) {
      const hipError_t e2 = hipFreeAsync(scratch, st);
      if (e == hipSuccess) e = e2;
    }
    if (e == hipSuccess && !(flags & WOS_ASYNC)) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
    return WOS_OK;
  }
  const size_t T = (size_t)total, o_g = T, o_m = 2 * T, o_v = 3 * T, o_norm = 4 * T;
  float* tmp = nullptr;
  if (hipMalloc((void**)&tmp, (o_norm + 1) * sizeof(float)) != hipSuccess)
    return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string((o_norm + 1) * sizeof(float)) + " bytes of staging");
  const auto staged = [&]() -> hipError_t {
    hipError_t e;
    const auto up = [&](size_t o, const float* src, size_t count) {
      return hipMemcpyAsync(tmp + o, src, count * sizeof(float), hipMemcpyHostToDevice, st);
    };
    for (int k = 0; k < n_tensors; k++) {
      const size_t at = (size_t)(segs.end[k] - counts[k]);
      if ((e = up(at, params[k], (size_t)counts[k])) != hipSuccess) return e;
      if ((e = up(o_g + at, grads[k], (size_t)counts[k])) != hipSuccess) return e;
      segs.p[k] = tmp + at;
      segs.g[k] = tmp + o_g + at;
    }
    if ((e = up(o_m, exp_avg, T)) != hipSuccess) return e;
    if ((e = up(o_v, exp_avg_sq, T)) != hipSuccess) return e;
    if ((e = run(tmp + o_m, tmp + o_v, tmp + o_norm)) != hipSuccess) return e;
    const auto down = [&](float* dst, size_t o, size_t count) {
      return hipMemcpyAsync(dst, tmp + o, count * sizeof(float), hipMemcpyDeviceToHost, st);
    };
    for (int k = 0; k < n_tensors; k++)
      if ((e = down(params[k], (size_t)(segs.end[k] - counts[k]), (size_t)counts[k])) != hipSuccess) return e;
    if ((e = down(exp_avg, o_m, T)) != hipSuccess) return e;
    if ((e = down(exp_avg_sq, o_v, T)) != hipSuccess) return e;
    if (clip && grad_norm && (e = down(grad_norm, o_norm, 1)) != hipSuccess) return e;
    return hipStreamSynchronize(st);
  };
  const hipError_t e = staged();
  if (e != hipSuccess) hipStreamSynchronize(st);  // nothing may still use tmp when it is freed
  hipFree(tmp);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
  return WOS_OK;
}

// The two fit loops' tensors: the network's own weights and biases for the fit step, and for the Adam
// step the same tensors, weights, then biases, with their gradients in one flat buffer `g` in that order.
static void fit_run_bind(const wos_siren_net* net, float* g, wos::SirenNet& dn, wos::AdamSegs& segs, wos::SirenGrads& dg) {
  const int D = net->d_in, DO = net->d_out, H = net->hidden, NL = net->n_hidden_layers + 2;
  segs.n = 2 * NL;
  size_t at = 0;
  for (int k = 0; k < 2 * NL; k++) {
    const int l = k < NL ? k : k - NL;
    const size_t rows = l == NL - 1 ? (size_t)DO : (size_t)H, count = k < NL ? rows * (l == 0 ? (size_t)D : (size_t)H) : rows;
    segs.p[k] = const_cast<float*>(k < NL ? net->weights[l] : net->biases[l]);
    segs.g[k] = g + at;
    (k < NL ? dg.w[l] : dg.b[l]) = g + at;
    at += count;
    segs.end[k] = (int64_t)at;
  }
  for (int l = 0; l < NL; l++) {
    dn.w[l] = net->weights[l];
    dn.b[l] = net->biases[l];
  }
}

// One iteration of either loop on n contiguous rows: wos_siren_fit's launches (both packs, the zero
// fill, the fit step with `plan`; the loss to state[1]) and wos_adam_step's (the norm to state[2] when
// clipping; the update, a no-op once state[0] is set).
static hipError_t fit_run_step(const wos::SirenNet& dn, float* tmp, size_t o_packT, size_t o_zero, size_t o_work,
                               const float* pts, int64_t n, const float* target, const float* scale,
                               const wos::SirenFitPlan& plan, const wos::SirenGrads& dg, const wos::AdamSegs& segs,
                               float* exp_avg, float* exp_avg_sq, const wos::AdamScalars& sc, bool clip, int* state,
                               hipStream_t st) {
  float *loss = (float*)state + 1, *norm = (float*)state + 2;
  hipError_t e;
  if ((e = wos::launch_siren_pack(dn, tmp, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(tmp + o_zero, 0, (size_t)dn.H * sizeof(float), st)) != hipSuccess) return e;
  if ((e = wos::launch_siren_pack_transposed(dn, tmp + o_packT, st)) != hipSuccess) return e;
  if ((e = wos::launch_siren_fit(dn, tmp, tmp + o_packT, tmp + o_zero, pts, n, target, scale, loss, &dg, plan, tmp + o_work,
                                 st)) != hipSuccess)
    return e;
  if (clip && (e = wos::launch_adam_norm(segs, norm, st)) != hipSuccess) return e;
  return wos::launch_adam_update(segs, exp_avg, exp_avg_sq, sc, clip ? norm : nullptr, state, st);
}

// One stream-ordered temporary per run: packed | packedT | H zeros | the plan's work (wos_siren_fit's
// layout), then the batch's points, target and scale, the flat gradients (weights, then biases: the
// order of exp_avg) and the state words [stop flag, loss, norm], each on a 256-byte boundary.
int wos_siren_fit_run(const wos_siren_net* net, const float* pool_pts, const float* pool_target, const float* pool_scale,
                      int64_t n_pool, const int64_t* idx, int64_t n_iters, int64_t batch, float* exp_avg,
                      float* exp_avg_sq, int64_t step0, const wos_adam_params* opt, float stop_loss, int32_t check_every,
                      float* losses, int64_t* status, size_t workspace_bytes, uint32_t flags, int32_t device,
                      void* stream) {
  const std::string fn = "wos_siren_fit_run";
  if (int rc = siren_net_check(fn, net)) return rc;
  const int D = net->d_in, DO = net->d_out, H = net->hidden, L = net->n_hidden_layers, NL = L + 2;
  if (!(flags & WOS_PTRS_DEVICE)) return fail(WOS_E_INVALID, fn + ": flags: device pointers only (WOS_PTRS_DEVICE)");
  if (check_every < 0) return fail(WOS_E_INVALID, fn + ": check_every must be >= 0, got " + std::to_string(check_every));
  if ((flags & WOS_ASYNC) && check_every > 0)
    return fail(WOS_E_INVALID, fn + ": check_every > 0 synchronises with the host and cannot be WOS_ASYNC");
  if (n_iters <= 0) return fail(WOS_E_INVALID, fn + ": n_iters must be positive, got " + std::to_string(n_iters));
  if (batch <= 0) return fail(WOS_E_INVALID, fn + ": batch must be positive, got " + std::to_string(batch));
  if (n_pool <= 0) return fail(WOS_E_INVALID, fn + ": n_pool must be positive, got " + std::to_string(n_pool));
  if (batch > (int64_t)0x7FFFFFFF * wos::kSirenTile) return fail(WOS_E_INVALID, fn + ": batch: too many points for one step");
  if (n_iters > (int64_t)1 << 40) return fail(WOS_E_INVALID, fn + ": n_iters: too many iterations for one call");
  if (step0 < 0) return fail(WOS_E_INVALID, fn + ": step0 must be >= 0, got " + std::to_string(step0));
  if (!pool_pts) return fail(WOS_E_INVALID, fn + ": null pool_pts");
  if (!pool_target) return fail(WOS_E_INVALID, fn + ": null pool_target");
  if (!idx) return fail(WOS_E_INVALID, fn + ": null idx");
  if (!losses) return fail(WOS_E_INVALID, fn + ": null losses");
  if (!status) return fail(WOS_E_INVALID, fn + ": null status");
  if (!exp_avg) return fail(WOS_E_INVALID, fn + ": null exp_avg");
  if (!exp_avg_sq) return fail(WOS_E_INVALID, fn + ": null exp_avg_sq");
  if (std::isnan(stop_loss)) return fail(WOS_E_INVALID, fn + ": stop_loss is NaN (negative: never stop)");
  if (int rc = adam_params_check(fn, opt)) return rc;
  const size_t tile_bytes = wos::siren_fit_stash_floats_per_tile(H, L) * sizeof(float);
  if (workspace_bytes != 0 && workspace_bytes < tile_bytes)
    return fail(WOS_E_CAPACITY, fn + ": workspace_bytes " + std::to_string(workspace_bytes) +
                                    " cannot hold one tile's stash of " + std::to_string(tile_bytes) + " bytes");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  wos::SirenNet dn{};
  dn.d_in = D;
  dn.d_out = DO;
  dn.H = H;
  dn.L = L;
  dn.omega = net->omega;
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int per_cu = std::max<int>(1, (int)(kLdsDynamicMax / wos::siren_fit_tile_lds_bytes(D, H)));
  const wos::SirenFitPlan plan =
      wos::siren_fit_plan(dn, batch, workspace_bytes ? workspace_bytes : kSirenVjpDefaultStash, cus * per_cu);
  const auto pad = [](size_t floats) { return (floats + 63) / 64 * 64; };
  const size_t pack_n = wos::siren_pack_floats(H, L), B = (size_t)batch;
  size_t n_par = 0;
  for (int l = 0; l < NL; l++) n_par += (l == NL - 1 ? (size_t)DO : (size_t)H) * ((l == 0 ? (size_t)D : (size_t)H) + 1);
  const size_t o_packT = pack_n, o_zero = 2 * pack_n, o_work = o_zero + (size_t)H, o_pts = pad(o_work + plan.total(true)),
               o_t = o_pts + pad(B * D), o_s = o_t + pad(B * DO), o_g = o_s + (pool_scale ? pad(B * DO) : 0),
               o_state = o_g + pad(n_par), total = o_state + 64;
  wos::AdamSegs segs{};
  wos::SirenGrads dg{};
  float* tmp = nullptr;
  if (hipMallocAsync((void**)&tmp, total * sizeof(float), st) != hipSuccess)
    return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string(total * sizeof(float)) + " bytes of workspace");
  fit_run_bind(net, tmp + o_g, dn, segs, dg);
  int* state = (int*)(tmp + o_state);
  float *b_pts = tmp + o_pts,*b_t = tmp + o_t, *b_s = pool_scale ? tmp + o_s : nullptr;
  const bool clip = opt->max_grad_norm > 0.0;
  int stopped = 0;  // the flag as last read on the host (check_every > 0)
  const auto run = [&]() -> hipError_t {
    hipError_t e;
    if ((e = hipMemsetAsync(state, 0, 64 * sizeof(float), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st)) != hipSuccess) return e;
    if ((e = hipMemsetD32Async((hipDeviceptr_t)losses, 0x7FC00000, (size_t)n_iters, st)) != hipSuccess) return e;
    int64_t pending = -1;  // the iteration whose commit has not been enqueued yet
    for (int64_t i = 0; i < n_iters; i++) {
      if ((e = wos::launch_fit_run_gather(D, DO, pool_pts, pool_target, pool_scale, n_pool, idx + i * batch, batch, b_pts,
                                          b_t, b_s, state, pending, stop_loss, losses, status, st)) != hipSuccess)
        return e;
      if ((e = fit_run_step(dn, tmp, o_packT, o_zero, o_work, b_pts, batch, b_t, b_s, plan, dg, segs, exp_avg, exp_avg_sq,
                            adam_scalars(*opt, step0 + i + 1), clip, state, st)) != hipSuccess)
        return e;
      pending = i;
      if (check_every > 0 && (i + 1) % check_every == 0 && i + 1 < n_iters) {
        if ((e = wos::launch_fit_run_commit(state, i, stop_loss, losses, status, st)) != hipSuccess) return e;
        pending = -1;
        if ((e = hipMemcpyAsync(&stopped, state, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        if (stopped) break;
      }
    }
    if (pending >= 0) return wos::launch_fit_run_commit(state, pending, stop_loss, losses, status, st);
    return hipSuccess;
  };
  hipError_t e = run();
  const hipError_t e2 = hipFreeAsync(tmp, st);
  if (e == hipSuccess) e = e2;
  int64_t bad = 0;
  if (e == hipSuccess && !(flags & WOS_ASYNC)) {
    e = hipMemcpyAsync(&bad, status + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
  if (bad != 0)
    return fail(WOS_E_INVALID, fn + ": idx: " + std::to_string(bad) + " indices outside [0, n_pool) were clamped (status[1])");
  return WOS_OK;
}

// wos_siren_fit_run without a pool: iteration i's rows offsets[i] .. offsets[i + 1] - 1 are read in
// place, with wos_siren_fit's plan for that many rows.  One stream-ordered temporary per run: packed |
// packedT | H zeros | the largest plan's work, then the flat gradients and the state words.  The
// commit that the gather carries there is a launch of its own here, between two iterations.
int wos_siren_fit_run_batches(const wos_siren_net* net, const float* pts, const float* target, const float* scale,
                              const int64_t* offsets, int64_t n_iters, float* exp_avg, float* exp_avg_sq, int64_t step0,
                              const wos_adam_params* opt, float stop_loss, int32_t check_every, float* losses,
                              int64_t* status, size_t workspace_bytes, uint32_t flags, int32_t device, void* stream) {
  const std::string fn = "wos_siren_fit_run_batches";
  if (int rc = siren_net_check(fn, net)) return rc;
  const int D = net->d_in, DO = net->d_out, H = net->hidden, L = net->n_hidden_layers, NL = L + 2;
  if (!(flags & WOS_PTRS_DEVICE)) return fail(WOS_E_INVALID, fn + ": flags: device pointers only (WOS_PTRS_DEVICE)");
  if (check_every < 0) return fail(WOS_E_INVALID, fn + ": check_every must be >= 0, got " + std::to_string(check_every));
  if ((flags & WOS_ASYNC) && check_every > 0)
    return fail(WOS_E_INVALID, fn + ": check_every > 0 synchronises with the host and cannot be WOS_ASYNC");
  if (n_iters <= 0) return fail(WOS_E_INVALID, fn + ": n_iters must be positive, got " + std::to_string(n_iters));
  if (n_iters > (int64_t)1 << 40) return fail(WOS_E_INVALID, fn + ": n_iters: too many iterations for one call");
  if (step0 < 0) return fail(WOS_E_INVALID, fn + ": step0 must be >= 0, got " + std::to_string(step0));
  if (!pts) return fail(WOS_E_INVALID, fn + ": null pts");
  if (!target) return fail(WOS_E_INVALID, fn + ": null target");
  if (!offsets) return fail(WOS_E_INVALID, fn + ": null offsets");
  if (!losses) return fail(WOS_E_INVALID, fn + ": null losses");
  if (!status) return fail(WOS_E_INVALID, fn + ": null status");
  if (!exp_avg) return fail(WOS_E_INVALID, fn + ": null exp_avg");
  if (!exp_avg_sq) return fail(WOS_E_INVALID, fn + ": null exp_avg_sq");
  if (std::isnan(stop_loss)) return fail(WOS_E_INVALID, fn + ": stop_loss is NaN (negative: never stop)");
  if (int rc = adam_params_check(fn, opt)) return rc;
  if (offsets[0] < 0) return fail(WOS_E_INVALID, fn + ": offsets[0] must be >= 0, got " + std::to_string(offsets[0]));
  for (int64_t i = 0; i < n_iters; i++) {
    if (offsets[i + 1] <= offsets[i])
      return fail(WOS_E_INVALID, fn + ": offsets must be strictly increasing: iteration " + std::to_string(i) + " has no rows (" +
                                     std::to_string(offsets[i]) + " to " + std::to_string(offsets[i + 1]) +
                                     "), and its loss is a mean over nothing");
    if (offsets[i + 1] - offsets[i] > (int64_t)0x7FFFFFFF * wos::kSirenTile)
      return fail(WOS_E_INVALID, fn + ": offsets: too many points for one step in iteration " + std::to_string(i));
  }
  const size_t tile_bytes = wos::siren_fit_stash_floats_per_tile(H, L) * sizeof(float);
  if (workspace_bytes != 0 && workspace_bytes < tile_bytes)
    return fail(WOS_E_CAPACITY, fn + ": workspace_bytes " + std::to_string(workspace_bytes) +
                                    " cannot hold one tile's stash of " + std::to_string(tile_bytes) + " bytes");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  wos::SirenNet dn{};
  dn.d_in = D;
  dn.d_out = DO;
  dn.H = H;
  dn.L = L;
  dn.omega = net->omega;
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int per_cu = std::max<int>(1, (int)(kLdsDynamicMax / wos::siren_fit_tile_lds_bytes(D, H)));
  const auto plan_of = [&](int64_t i) {  // wos_siren_fit's plan for iteration i's rows
    return wos::siren_fit_plan(dn, offsets[i + 1] - offsets[i], workspace_bytes ? workspace_bytes : kSirenVjpDefaultStash,
                               cus * per_cu);
  };
  size_t work = 0;
  for (int64_t i = 0; i < n_iters; i++) work = std::max(work, plan_of(i).total(true));
  const auto pad = [](size_t floats) { return (floats + 63) / 64 * 64; };
  const size_t pack_n = wos::siren_pack_floats(H, L);
  size_t n_par = 0;
  for (int l = 0; l < NL; l++) n_par += (l == NL - 1 ? (size_t)DO : (size_t)H) * ((l == 0 ? (size_t)D : (size_t)H) + 1);
  const size_t o_packT = pack_n, o_zero = 2 * pack_n, o_work = o_zero + (size_t)H, o_g = pad(o_work + work),
               o_state = o_g + pad(n_par), total = o_state + 64;
  wos::AdamSegs segs{};
  wos::SirenGrads dg{};
  float* tmp = nullptr;
  if (hipMallocAsync((void**)&tmp, total * sizeof(float), st) != hipSuccess)
    return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string(total * sizeof(float)) + " bytes of workspace");
  fit_run_bind(net, tmp + o_g, dn, segs, dg);
  int* state = (int*)(tmp + o_state);
  const bool clip = opt->max_grad_norm > 0.0;
  int stopped = 0;  // the flag as last read on the host (check_every > 0)
  const auto run = [&]() -> hipError_t {
    hipError_t e;
    if ((e = hipMemsetAsync(state, 0, 64 * sizeof(float), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st)) != hipSuccess) return e;
    if ((e = hipMemsetD32Async((hipDeviceptr_t)losses, 0x7FC00000, (size_t)n_iters, st)) != hipSuccess) return e;
    int64_t pending = -1;  // the iteration whose commit has not been enqueued yet
    for (int64_t i = 0; i < n_iters; i++) {
      if (pending >= 0 && (e = wos::launch_fit_run_commit(state, pending, stop_loss, losses, status, st)) != hipSuccess)
        return e;
      const int64_t row = offsets[i];
      if ((e = fit_run_step(dn, tmp, o_packT, o_zero, o_work, pts + row * D, offsets[i + 1] - row, target + row * DO,
                            scale ? scale + row * DO : nullptr, plan_of(i), dg, segs, exp_avg, exp_avg_sq,
                            adam_scalars(*opt, step0 + i + 1), clip, state, st)) != hipSuccess)
        return e;
      pending = i;
      if (check_every > 0 && (i + 1) % check_every == 0 && i + 1 < n_iters) {
        if ((e = wos::launch_fit_run_commit(state, i, stop_loss, losses, status, st)) != hipSuccess) return e;
        pending = -1;
        if ((e = hipMemcpyAsync(&stopped, state, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        if (stopped) break;
      }
    }
    if (pending >= 0) return wos::launch_fit_run_commit(state, pending, stop_loss, losses, status, st);
    return hipSuccess;
  };
  hipError_t e = run();
  const hipError_t e2 = hipFreeAsync(tmp, st);
  if (e == hipSuccess) e = e2;
  if (e == hipSuccess && !(flags & WOS_ASYNC)) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
  return WOS_OK;
}

}  // extern "C"
