// wos_capi_siren.cpp -- the host half of the fused SIREN: wos_siren_eval (wos_siren.hip), wos_siren_vjp
// (wos_siren_vjp.hip), wos_siren_fit (wos_siren_fit.hip), wos_adam_step, wos_siren_fit_run and
// wos_siren_fit_run_batches (wos_siren_train.hip), and the two SIREN self-test probes.  No scene, no
// workspace, no lock: each call owns the one temporary it allocates (with_tmp).
#include "wos_capi.h"

using namespace wos::capi;

// ---- the envelope ------------------------------------------------------------------------------
static int siren_shape_check(const std::string& fn, int32_t d_in, int32_t hidden) {
  if (d_in != 2 && d_in != 3) return fail(WOS_E_INVALID, fn + ": d_in must be 2 or 3, got " + std::to_string(d_in));
  if (hidden < 32 || hidden > wos::kSirenMaxHidden || hidden % 32 != 0)
    return fail(WOS_E_INVALID, fn + ": hidden must be a multiple of 32 in 32.." + std::to_string(wos::kSirenMaxHidden) +
                                   ", got " + std::to_string(hidden));
  return WOS_OK;
}

// the envelope of every entry point: shape, omega and the pointer arrays
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

static int grad_ptrs_check(const std::string& fn, float* const* gw, float* const* gb, int NL) {
  for (int l = 0; l < NL; l++)
    if (!gw[l] || !gb[l])
      return fail(WOS_E_INVALID, fn + ": null grad_weights or grad_biases pointer of layer " + std::to_string(l));
  return WOS_OK;
}

static int stash_cap_check(const std::string& fn, size_t workspace_bytes, size_t tile_bytes) {
  if (workspace_bytes != 0 && workspace_bytes < tile_bytes)
    return fail(WOS_E_CAPACITY, fn + ": workspace_bytes " + std::to_string(workspace_bytes) +
                                    " cannot hold one tile's stash of " + std::to_string(tile_bytes) + " bytes");
  return WOS_OK;
}

// floats per row of a fit's scale: d_out, or with WOS_FIT_SCALE_MATRIX d_out * d_out
static int scale_width(uint32_t flags, int d_out) { return (flags & WOS_FIT_SCALE_MATRIX) ? d_out * d_out : d_out; }

// ---- the network as the launchers take it --------------------------------------------------------
// wos_siren_net -> wos::SirenNet without layer pointers
static wos::SirenNet net_view(const wos_siren_net* net) {
  wos::SirenNet dn{};
  dn.d_in = net->d_in;
  dn.d_out = net->d_out;
  dn.H = net->hidden;
  dn.L = net->n_hidden_layers;
  dn.omega = net->omega;
  return dn;
}

// elements of every layer's weight and bias; returns their sum, the network's parameters
static size_t layer_counts(const wos_siren_net* net, size_t* n_w, size_t* n_b) {
  const int NL = net->n_hidden_layers + 2;
  size_t n_par = 0;
  for (int l = 0; l < NL; l++) {
    n_b[l] = l == NL - 1 ? (size_t)net->d_out : (size_t)net->hidden;
    n_w[l] = n_b[l] * (l == 0 ? (size_t)net->d_in : (size_t)net->hidden);
    n_par += n_w[l] + n_b[l];
  }
  return n_par;
}

// device pointers: the caller's own layers (and gradients, gw non-null)
static void bind_layers(const wos_siren_net* net, float* const* gw, float* const* gb, wos::SirenNet& dn, wos::SirenGrads& dg) {
  for (int l = 0; l < dn.L + 2; l++) {
    dn.w[l] = net->weights[l];
    dn.b[l] = net->biases[l];
    if (gw) {
      dg.w[l] = gw[l];
      dg.b[l] = gb[l];
    }
  }
}

// what siren_vjp_plan and siren_fit_plan take beside the net and n: the stash's cap (256 MiB when
// workspace_bytes is 0) and the tile workgroups that `device` holds at once
struct PlanArgs {
  size_t stash_cap;
  int resident;
};
static int plan_args(int32_t device, size_t workspace_bytes, size_t tile_lds_bytes, PlanArgs* out) {
  constexpr size_t kSirenVjpDefaultStash = (size_t)256 << 20;
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int per_cu = std::max<int>(1, (int)(kLdsDynamicMax / tile_lds_bytes));
  *out = {workspace_bytes ? workspace_bytes : kSirenVjpDefaultStash, cus * per_cu};
  return WOS_OK;
}

// The device half of every temporary: packed | packedT | H zeros | work; without the transposed copy
// (the forward, the loss alone) packed | work.  The kernels read the packed copies with 16-byte loads.
struct DevTmp {
  size_t o_packT, o_zero, o_work, floats;
  DevTmp(const wos::SirenNet& dn, bool transposed, size_t work) {
    const size_t pack_n = wos::siren_pack_floats(dn.H, dn.L);
    o_packT = pack_n;
    o_zero = 2 * pack_n;
    o_work = transposed ? o_zero + (size_t)dn.H : pack_n;
    floats = o_work + work;
  }
};

// the fragment-ordered copy of the hidden weights and, for a backward, the H zeros and the copy of W^T:
// for E members in the same three launches, member e's copies e * member_stride floats further on
// (the zeros are member 0's, and every member reads them)
static hipError_t enqueue_packs(const wos::SirenNets& nets, int E, float* tmp, const DevTmp& lay, size_t member_stride,
                                bool transposed, hipStream_t st) {
  hipError_t e;
  if ((e = wos::launch_siren_pack_members(nets, E, tmp, member_stride, st)) != hipSuccess || !transposed) return e;
  if ((e = hipMemsetAsync(tmp + lay.o_zero, 0, (size_t)nets.v[0].H * sizeof(float), st)) != hipSuccess) return e;
  return wos::launch_siren_pack_transposed_members(nets, E, tmp + lay.o_packT, member_stride, st);
}
static hipError_t enqueue_packs(const wos::SirenNet& dn, float* tmp, const DevTmp& lay, bool transposed, hipStream_t st) {
  wos::SirenNets nets{};
  nets.v[0] = dn;
  return enqueue_packs(nets, 1, tmp, lay, 0, transposed, st);
}

// ---- the call protocol ---------------------------------------------------------------------------
// A call's one temporary, handed out front to back.  up / down are the staged half's copies; the
// first error sticks and turns the later ones into no-ops, so a body tests `e` once after its uploads.
struct Tmp {
  float* base = nullptr;
  size_t floats = 0, used = 0;
  hipStream_t st = nullptr;
  hipError_t e = hipSuccess;
  float* take(size_t count) {
    if (used + count > floats) e = hipErrorInvalidValue;  // (the caller's sum of its takes is wrong)
    float* at = base + used;
    used += count;
    return at;
  }
  float* put(float* at, const float* src, size_t count) {
    if (e == hipSuccess) e = hipMemcpyAsync(at, src, count * sizeof(float), hipMemcpyHostToDevice, st);
    return at;
  }
  float* up(const float* src, size_t count) { return put(take(count), src, count); }
  void down(float* dst, const float* at, size_t count) {
    if (e == hipSuccess) e = hipMemcpyAsync(dst, at, count * sizeof(float), hipMemcpyDeviceToHost, st);
  }
};

// Runs body(Tmp&) inside a temporary of `floats` floats (0: none is allocated).  Stream-ordered
// (device pointers): the free is enqueued behind the body, so WOS_ASYNC needs no host wait.  Staged
// (host pointers): one hipMalloc, freed after the call's own synchronise.
template <class Body>
static int with_tmp(const std::string& fn, size_t floats, bool staged, uint32_t flags, hipStream_t st, Body&& body) {
  Tmp t;
  t.floats = floats;
  t.st = st;
  const size_t bytes = floats * sizeof(float);
  if (floats > 0 && (staged ? hipMalloc((void**)&t.base, bytes) : hipMallocAsync((void**)&t.base, bytes, st)) != hipSuccess)
    return fail(WOS_E_NOMEM, fn + ": cannot allocate " + std::to_string(bytes) + " bytes of " + (staged ? "staging" : "workspace"));
  hipError_t e = body(t);
  if (staged) {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) hipStreamSynchronize(st);  // nothing may still use the temporary when it is freed
    hipFree(t.base);
  } else {
    if (t.base) {
      const hipError_t e2 = hipFreeAsync(t.base, st);
      if (e == hipSuccess) e = e2;
    }
    if (e == hipSuccess && !(flags & WOS_ASYNC)) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) return fail(WOS_E_DEVICE, fn + ": " + hipGetErrorString(e));
  return WOS_OK;
}

// host pointers: the layers uploaded one after the other, each followed by room for its gradients (grads)
static void stage_net(Tmp& t, const wos_siren_net* net, const size_t* n_w, const size_t* n_b, bool grads, wos::SirenNet& dn,
                      wos::SirenGrads& dg) {
  for (int l = 0; l < dn.L + 2; l++) {
    dn.w[l] = t.up(net->weights[l], n_w[l]);
    dn.b[l] = t.up(net->biases[l], n_b[l]);
    if (grads) {
      dg.w[l] = t.take(n_w[l]);
      dg.b[l] = t.take(n_b[l]);
    }
  }
}

static void download_grads(Tmp& t, const wos::SirenGrads& dg, float* const* gw, float* const* gb, const size_t* n_w,
                           const size_t* n_b, int NL) {
  for (int l = 0; l < NL; l++) {
    t.down(gw[l], dg.w[l], n_w[l]);
    t.down(gb[l], dg.b[l], n_b[l]);
  }
}

extern "C" {

// ---- fused SIREN (wos_siren.hip) -------------------------------------------------------------
// The temporary: packed; with host pointers also the staged network, pts, u, jac and div.
int wos_siren_eval(const wos_siren_net* net, const float* pts, int64_t n, float* u, float* jac, float* div,
                   uint32_t flags, int32_t device, void* stream) {
  const std::string fn = "wos_siren_eval";
  if (int rc = siren_net_check(fn, net)) return rc;
  const int D = net->d_in, DO = net->d_out;
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
  wos::SirenNet dn = net_view(net);
  wos::SirenGrads dg{};
  size_t n_w[wos::kSirenMaxLayers], n_b[wos::kSirenMaxLayers];
  const size_t n_par = layer_counts(net, n_w, n_b), N = (size_t)n, nu = u ? N * DO : 0, nj = jac ? N * DO * D : 0,
               nd = div ? N : 0;
  const DevTmp lay(dn, false, 0);
  const bool dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  return with_tmp(fn, lay.floats + (dev_ptrs ? 0 : n_par + N * D + nu + nj + nd), !dev_ptrs, flags, st, [&](Tmp& t) -> hipError_t {
    float* tmp = t.take(lay.floats);
    const float* d_pts = pts;
    float *d_u = u, *d_j = jac, *d_d = div;
    if (dev_ptrs) {
      bind_layers(net, nullptr, nullptr, dn, dg);
    } else {
      stage_net(t, net, n_w, n_b, false, dn, dg);
      d_pts = t.up(pts, N * D);
      d_u = u ? t.take(nu) : nullptr;
      d_j = jac ? t.take(nj) : nullptr;
      d_d = div ? t.take(nd) : nullptr;
      if (t.e != hipSuccess) return t.e;
    }
    hipError_t e;
    if ((e = enqueue_packs(dn, tmp, lay, false, st)) != hipSuccess) return e;
    if ((e = wos::launch_siren_eval(dn, tmp, d_pts, n, d_u, d_j, d_d, st)) != hipSuccess || dev_ptrs) return e;
    if (u) t.down(u, d_u, nu);
    if (jac) t.down(jac, d_j, nj);
    if (div) t.down(div, d_d, nd);
    return t.e;
  });
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
// The temporary: packed | packedT | H zeros | the plan's work; with host pointers also the staged
// network with its gradients, points and cotangents.
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
  WOS_TRY(grad_ptrs_check(fn, grad_weights, grad_biases, NL));
  if (n < 0) return fail(WOS_E_INVALID, fn + ": n is negative");
  if (n > (int64_t)0x7FFFFFFF * wos::kSirenTile) return fail(WOS_E_INVALID, fn + ": n: too many points for one call");
  WOS_TRY(stash_cap_check(fn, workspace_bytes, wos::siren_vjp_stash_floats_per_tile(D, H, L) * sizeof(float)));
  if (n > 0 && !pts) return fail(WOS_E_INVALID, fn + ": null point buffer");
  size_t n_w[wos::kSirenMaxLayers], n_b[wos::kSirenMaxLayers];
  const size_t n_par = layer_counts(net, n_w, n_b);
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
  wos::SirenNet dn = net_view(net);
  wos::SirenGrads dg{};
  PlanArgs pa;
  WOS_TRY(plan_args(device, workspace_bytes, wos::siren_vjp_tile_lds_bytes(D, H), &pa));
  const wos::SirenVjpPlan plan = wos::siren_vjp_plan(dn, n, pa.stash_cap, pa.resident);
  const DevTmp lay(dn, true, plan.total());
  const size_t N = (size_t)n, nu = g_u ? N * DO : 0, nj = g_jac ? N * DO * D : 0, nd = g_div ? N : 0,
               dev_floats = n > 0 ? lay.floats : 0;  // no points: the kernel only zeroes the gradients
  return with_tmp(fn, dev_floats + (dev_ptrs ? 0 : 2 * n_par + N * D + nu + nj + nd), !dev_ptrs, flags, st, [&](Tmp& t) -> hipError_t {
    float* tmp = t.take(dev_floats);
    const float *d_pts = pts, *d_gu = g_u, *d_gj = g_jac, *d_gd = g_div;
    if (dev_ptrs) {
      bind_layers(net, grad_weights, grad_biases, dn, dg);
    } else {
      stage_net(t, net, n_w, n_b, true, dn, dg);
      d_pts = t.up(pts, N * D);
      if (g_u) d_gu = t.up(g_u, nu);
      if (g_jac) d_gj = t.up(g_jac, nj);
      if (g_div) d_gd = t.up(g_div, nd);
      if (t.e != hipSuccess) return t.e;
    }
    if (n == 0) return wos::launch_siren_vjp(dn, nullptr, nullptr, nullptr, nullptr, 0, d_gu, d_gj, d_gd, dg, plan, nullptr, st);
    hipError_t e;
    if ((e = enqueue_packs(dn, tmp, lay, true, st)) != hipSuccess) return e;
    if ((e = wos::launch_siren_vjp(dn, tmp, tmp + lay.o_packT, tmp + lay.o_zero, d_pts, n, d_gu, d_gj, d_gd, dg, plan,
                                   tmp + lay.o_work, st)) != hipSuccess || dev_ptrs)
      return e;
    download_grads(t, dg, grad_weights, grad_biases, n_w, n_b, NL);
    return t.e;
  });
}

// ---- fused SIREN fit step (wos_siren_fit.hip) ------------------------------------------------
// The temporary: packed | packedT | H zeros | the plan's work (loss only: packed | the tiles' sums);
// with host pointers also the staged network with its gradients, points, target, scale and loss.
int wos_siren_fit(const wos_siren_net* net, const float* pts, int64_t n, const float* target, const float* scale,
                  float* loss, float* const* grad_weights, float* const* grad_biases, size_t workspace_bytes,
                  uint32_t flags, int32_t device, void* stream) {
  const std::string fn = "wos_siren_fit";
  if (int rc = siren_net_check(fn, net)) return rc;
  const int D = net->d_in, DO = net->d_out, H = net->hidden, L = net->n_hidden_layers, NL = L + 2;
  if (!loss) return fail(WOS_E_INVALID, fn + ": null loss");
  if (!target) return fail(WOS_E_INVALID, fn + ": null target");
  if ((flags & WOS_FIT_SCALE_MATRIX) && !scale)
    return fail(WOS_E_INVALID, fn + ": null scale with WOS_FIT_SCALE_MATRIX (the flag says how scale is laid out)");
  if ((grad_weights == nullptr) != (grad_biases == nullptr))
    return fail(WOS_E_INVALID, fn + ": exactly one of grad_weights and grad_biases is null (both null: the loss alone)");
  const bool grads = grad_weights != nullptr;
  if (grads) WOS_TRY(grad_ptrs_check(fn, grad_weights, grad_biases, NL));
  if (n <= 0) return fail(WOS_E_INVALID, fn + ": n must be positive (a mean over nothing), got " + std::to_string(n));
  if (n > (int64_t)0x7FFFFFFF * wos::kSirenTile) return fail(WOS_E_INVALID, fn + ": n: too many points for one call");
  WOS_TRY(stash_cap_check(fn, workspace_bytes, wos::siren_fit_stash_floats_per_tile(H, L) * sizeof(float)));
  if (!pts) return fail(WOS_E_INVALID, fn + ": null point buffer");
  size_t n_w[wos::kSirenMaxLayers], n_b[wos::kSirenMaxLayers];
  const size_t n_par = layer_counts(net, n_w, n_b);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  wos::SirenNet dn = net_view(net);
  wos::SirenGrads dg{};
  PlanArgs pa;
  WOS_TRY(plan_args(device, workspace_bytes, wos::siren_fit_tile_lds_bytes(D, H), &pa));
  const wos::SirenFitPlan plan = wos::siren_fit_plan(dn, n, pa.stash_cap, pa.resident);
  const DevTmp lay(dn, grads, plan.total(grads));
  const int SW = scale_width(flags, DO);
  const size_t N = (size_t)n, ns = scale ? N * SW : 0;
  const bool dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  return with_tmp(fn, lay.floats + (dev_ptrs ? 0 : (grads ? 2 : 1) * n_par + N * D + N * DO + ns + 1), !dev_ptrs, flags, st,
                  [&](Tmp& t) -> hipError_t {
    float* tmp = t.take(lay.floats);
    const float *d_pts = pts, *d_target = target, *d_scale = scale;
    float* d_loss = loss;
    if (dev_ptrs) {
      bind_layers(net, grad_weights, grad_biases, dn, dg);
    } else {
      stage_net(t, net, n_w, n_b, grads, dn, dg);
      d_pts = t.up(pts, N * D);
      d_target = t.up(target, N * DO);
      if (scale) d_scale = t.up(scale, ns);
      d_loss = t.take(1);
      if (t.e != hipSuccess) return t.e;
    }
    hipError_t e;
    if ((e = enqueue_packs(dn, tmp, lay, grads, st)) != hipSuccess) return e;
    if ((e = wos::launch_siren_fit(dn, tmp, grads ? tmp + lay.o_packT : nullptr, grads ? tmp + lay.o_zero : nullptr, d_pts, n,
                                   d_target, d_scale, SW, d_loss, grads ? &dg : nullptr, plan, tmp + lay.o_work, st)) != hipSuccess ||
        dev_ptrs)
      return e;
    t.down(loss, d_loss, 1);
    if (grads) download_grads(t, dg, grad_weights, grad_biases, n_w, n_b, NL);
    return t.e;
  });
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

}  // extern "C"

// ---- fused Adam step and the device-resident fit loops (wos_siren_train.hip) ---------------------
static_assert(wos::kAdamMaxTensors == 20, "include/wos.h documents n_tensors as 1..20");
static_assert(sizeof(wos_adam_params) == 5 * sizeof(double), "wos_adam_params is five doubles (wos_amd/_lib.py AdamParams)");
static_assert(sizeof(wos::AdamMembers) + sizeof(wos::AdamScalars) + 2 * sizeof(void*) <= 4096,
              "adam_update_kernel's arguments, every member's segment table included, fit the kernel argument segment");
static_assert(sizeof(wos::SirenNets) + sizeof(wos::SirenMemberRows) + 16 * sizeof(void*) <= 4096,
              "siren_fit_tile_kernel's arguments, every member's network included, fit the kernel argument segment");
static_assert(wos::kSirenMaxMembers == WOS_MAX_CHANNELS, "an ensemble is as wide as a multi-channel solve");
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

// Device pointers: one float of scratch, and only when clipping without grad_norm.  Host pointers:
// params | grads | exp_avg | exp_avg_sq | norm.
extern "C" int wos_adam_step(int32_t n_tensors, const int64_t* counts, float* const* params, const float* const* grads,
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
  const bool clip = opt->max_grad_norm > 0.0, dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  const wos::AdamScalars sc = adam_scalars(*opt, step);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const size_t T = (size_t)total;
  return with_tmp(fn, dev_ptrs ? (clip && !grad_norm ? 1 : 0) : 4 * T + 1, !dev_ptrs, flags, st, [&](Tmp& t) -> hipError_t {
    float *m = exp_avg, *v = exp_avg_sq, *norm = grad_norm ? grad_norm : t.base;
    float *p0 = dev_ptrs ? nullptr : t.take(T), *g0 = dev_ptrs ? nullptr : t.take(T);
    for (int k = 0; k < n_tensors; k++) {
      const size_t at = (size_t)(segs.end[k] - counts[k]), count = (size_t)counts[k];
      segs.p[k] = dev_ptrs ? params[k] : t.put(p0 + at, params[k], count);
      segs.g[k] = dev_ptrs ? grads[k] : t.put(g0 + at, grads[k], count);
    }
    if (!dev_ptrs) {
      m = t.up(exp_avg, T);
      v = t.up(exp_avg_sq, T);
      norm = t.take(1);
      if (t.e != hipSuccess) return t.e;
    }
    hipError_t e;
    if (clip && (e = wos::launch_adam_norm(segs, norm, st)) != hipSuccess) return e;
    if ((e = wos::launch_adam_update(segs, m, v, sc, clip ? norm : nullptr, nullptr, st)) != hipSuccess || dev_ptrs) return e;
    for (int k = 0; k < n_tensors; k++) t.down(params[k], segs.p[k], (size_t)counts[k]);
    t.down(exp_avg, m, T);
    t.down(exp_avg_sq, v, T);
    if (clip && grad_norm) t.down(grad_norm, norm, 1);
    return t.e;
  });
}

// The two fit loops' tensors: the network's own weights and biases for the fit step, and for the Adam
// step the same tensors, weights, then biases, with their gradients in one flat buffer `g` in that order.
static void fit_run_bind(const wos_siren_net* net, float* g, wos::SirenNet& dn, wos::AdamSegs& segs, wos::SirenGrads& dg) {
  const int NL = net->n_hidden_layers + 2;
  size_t n_w[wos::kSirenMaxLayers], n_b[wos::kSirenMaxLayers];
  layer_counts(net, n_w, n_b);
  segs.n = 2 * NL;
  size_t at = 0;
  for (int k = 0; k < 2 * NL; k++) {
    const int l = k < NL ? k : k - NL;
    segs.p[k] = const_cast<float*>(k < NL ? net->weights[l] : net->biases[l]);
    segs.g[k] = g + at;
    (k < NL ? dg.w[l] : dg.b[l]) = g + at;
    at += k < NL ? n_w[l] : n_b[l];
    segs.end[k] = (int64_t)at;
  }
  bind_layers(net, nullptr, nullptr, dn, dg);
}

// the rows of one iteration, contiguous on the device: the points, which the members share, and each
// member's target and scale
struct FitRows {
  const float* pts;
  wos::SirenMemberRows m;
};

// What a loop's members keep in its temporary, member e at + e * stride: the device half of a fit step
// (`member`: packed | packedT | H zeros | work), the flat gradients (`grad`) and, kFitStateWords apart,
// the state words.
struct FitStrides {
  size_t member, grad;
};

// One iteration of either loop on n contiguous rows, every launch covering the E members:
// wos_siren_fit's launches (both packs, the zero fill, the fit step with `plan`; the loss to state[1])
// and wos_adam_step's (the norm to state[2] when clipping; the update, a no-op for a member whose
// state[0] is set).  dg: member 0's gradients.
static hipError_t fit_run_step(const wos::SirenNets& nets, int E, float* tmp, const DevTmp& lay, const FitStrides& stride,
                               const FitRows& r, int64_t n, const wos::SirenFitPlan& plan, const wos::SirenGrads& dg,
                               const wos::AdamMembers& adam, const wos::AdamScalars& sc, bool clip, int* state,
                               hipStream_t st) {
  float *loss = (float*)state + 1, *norm = (float*)state + 2;
  hipError_t e;
  if ((e = enqueue_packs(nets, E, tmp, lay, stride.member, true, st)) != hipSuccess) return e;
  if ((e = wos::launch_siren_fit_members(nets, E, tmp, tmp + lay.o_packT, tmp + lay.o_zero, r.pts, n, r.m, loss,
                                         wos::kFitStateWords, &dg, stride.grad, plan, tmp + lay.o_work, stride.member, st)) !=
      hipSuccess)
    return e;
  if (clip && (e = wos::launch_adam_norm_members(adam, E, norm, st)) != hipSuccess) return e;
  return wos::launch_adam_update_members(adam, E, sc, clip ? norm : nullptr, state, st);
}

// what the two loops take alike: n_members networks of one shape, each with its moments, its row of
// `losses` and its pair of `status`.  ensemble: the caller is an _ensemble entry point, whose
// refusals name the member.
struct FitRun {
  bool ensemble;
  int32_t n_members;
  const wos_siren_net* nets;
  int64_t n_iters;
  float* const* exp_avg;
  float* const* exp_avg_sq;
  int64_t step0;
  const wos_adam_params* opt;
  float stop_loss;
  int32_t check_every;
  float* losses;
  int64_t* status;
  size_t workspace_bytes;
  uint32_t flags;
  int32_t device;
  hipStream_t st;
};
struct NamedPtr {
  std::string name;
  const void* p;
};
static size_t pad64(size_t floats) { return (floats + 63) / 64 * 64; }  // to a 256-byte boundary
static std::string of_member(const FitRun& a, int e) { return a.ensemble ? " of member " + std::to_string(e) : ""; }

// The members' networks: the envelope of each, then one shape for all.  The first refusal of the
// loops, as siren_net_check is of the single-network entry points.
static int fit_run_nets_check(const std::string& fn, const FitRun& a) {
  if (!a.ensemble) return siren_net_check(fn, a.nets);
  if (a.n_members < 1 || a.n_members > wos::kSirenMaxMembers)
    return fail(WOS_E_INVALID, fn + ": n_members must be 1.." + std::to_string(wos::kSirenMaxMembers) + ", got " +
                                   std::to_string(a.n_members));
  if (!a.nets) return fail(WOS_E_INVALID, fn + ": null nets");
  for (int e = 0; e < a.n_members; e++)
    if (int rc = siren_net_check(fn + ": member " + std::to_string(e), &a.nets[e])) return rc;
  const wos_siren_net& n0 = a.nets[0];
  for (int e = 1; e < a.n_members; e++) {
    const wos_siren_net& ne = a.nets[e];
    const auto differs = [&](const char* field, const std::string& mine, const std::string& first) {
      return fail(WOS_E_INVALID, fn + ": member " + std::to_string(e) + ": " + field + " is " + mine + ", member 0's " + first +
                                     " (the members of an ensemble have one shape)");
    };
    if (ne.d_in != n0.d_in) return differs("d_in", std::to_string(ne.d_in), std::to_string(n0.d_in));
    if (ne.d_out != n0.d_out) return differs("d_out", std::to_string(ne.d_out), std::to_string(n0.d_out));
    if (ne.hidden != n0.hidden) return differs("hidden", std::to_string(ne.hidden), std::to_string(n0.hidden));
    if (ne.n_hidden_layers != n0.n_hidden_layers)
      return differs("n_hidden_layers", std::to_string(ne.n_hidden_layers), std::to_string(n0.n_hidden_layers));
    if (ne.omega != n0.omega) return differs("omega", std::to_string(ne.omega), std::to_string(n0.omega));
  }
  return WOS_OK;
}

// no two members train the same tensor or keep their moments in the same buffer
static int fit_run_alias_check(const std::string& fn, const FitRun& a) {
  const int NL = a.nets[0].n_hidden_layers + 2;
  for (int e = 1; e < a.n_members; e++)
    for (int f = 0; f < e; f++) {
      const std::string pair = ": members " + std::to_string(f) + " and " + std::to_string(e) + " share ";
      for (int l = 0; l < NL; l++)
        for (int m = 0; m < NL; m++) {
          if (a.nets[e].weights[l] == a.nets[f].weights[m])
            return fail(WOS_E_INVALID, fn + pair + "a weights pointer (layers " + std::to_string(m) + " and " + std::to_string(l) + ")");
          if (a.nets[e].biases[l] == a.nets[f].biases[m])
            return fail(WOS_E_INVALID, fn + pair + "a biases pointer (layers " + std::to_string(m) + " and " + std::to_string(l) + ")");
        }
      if (a.exp_avg[e] == a.exp_avg[f]) return fail(WOS_E_INVALID, fn + pair + "an exp_avg buffer");
      if (a.exp_avg_sq[e] == a.exp_avg_sq[f]) return fail(WOS_E_INVALID, fn + pair + "an exp_avg_sq buffer");
      if (a.exp_avg[e] == a.exp_avg_sq[f] || a.exp_avg_sq[e] == a.exp_avg[f])
        return fail(WOS_E_INVALID, fn + pair + "a moment buffer (one's exp_avg is the other's exp_avg_sq)");
    }
  return WOS_OK;
}

// Both loops, for one network and for an ensemble.  One stream-ordered temporary per run: per member
// packed | packedT | H zeros | the largest plan's work (wos_siren_fit's layout), then `gathered` floats
// of the caller's own, per member the flat gradients (weights, then biases: the order of exp_avg) and
// per member the state words [stop flag, loss, norm], each on a 256-byte boundary.  sizes_check and
// rows_check: the caller's own refusals, at their places among the shared ones; `in`: its input
// arrays.  n_of(i): the rows of iteration i.  feed(i, pending, gathered, state, rows): where they lie,
// after enqueuing what brings them there and the commit of iteration `pending` (-1: none is due).
// clamped non-null: status[1] as read back after a blocking run.
template <class Sizes, class Rows, class NOf, class Feed>
static int fit_run_loop(const std::string& fn, const FitRun& a, const std::vector<NamedPtr>& in, Sizes&& sizes_check,
                        Rows&& rows_check, size_t gathered, NOf&& n_of, Feed&& feed, int64_t* clamped) {
  const int E = a.n_members;
  const wos_siren_net* net = a.nets;  // member 0: every member has its shape
  const int D = net->d_in, H = net->hidden, L = net->n_hidden_layers;
  const int64_t n_iters = a.n_iters;
  hipStream_t st = a.st;
  if (!(a.flags & WOS_PTRS_DEVICE)) return fail(WOS_E_INVALID, fn + ": flags: device pointers only (WOS_PTRS_DEVICE)");
  if (a.check_every < 0) return fail(WOS_E_INVALID, fn + ": check_every must be >= 0, got " + std::to_string(a.check_every));
  if ((a.flags & WOS_ASYNC) && a.check_every > 0)
    return fail(WOS_E_INVALID, fn + ": check_every > 0 synchronises with the host and cannot be WOS_ASYNC");
  if (n_iters <= 0) return fail(WOS_E_INVALID, fn + ": n_iters must be positive, got " + std::to_string(n_iters));
  WOS_TRY(sizes_check());
  if (n_iters > (int64_t)1 << 40) return fail(WOS_E_INVALID, fn + ": n_iters: too many iterations for one call");
  if (a.step0 < 0) return fail(WOS_E_INVALID, fn + ": step0 must be >= 0, got " + std::to_string(a.step0));
  for (const NamedPtr& q : in)
    if (!q.p) return fail(WOS_E_INVALID, fn + ": null " + q.name);
  if (!a.losses) return fail(WOS_E_INVALID, fn + ": null losses");
  if (!a.status) return fail(WOS_E_INVALID, fn + ": null status");
  if (!a.exp_avg) return fail(WOS_E_INVALID, fn + ": null exp_avg");
  if (!a.exp_avg_sq) return fail(WOS_E_INVALID, fn + ": null exp_avg_sq");
  for (int e = 0; e < E; e++) {
    if (!a.exp_avg[e]) return fail(WOS_E_INVALID, fn + ": null exp_avg" + of_member(a, e));
    if (!a.exp_avg_sq[e]) return fail(WOS_E_INVALID, fn + ": null exp_avg_sq" + of_member(a, e));
  }
  if (std::isnan(a.stop_loss)) return fail(WOS_E_INVALID, fn + ": stop_loss is NaN (negative: never stop)");
  if (int rc = adam_params_check(fn, a.opt)) return rc;
  WOS_TRY(rows_check());
  WOS_TRY(fit_run_alias_check(fn, a));
  WOS_TRY(stash_cap_check(fn, a.workspace_bytes, wos::siren_fit_stash_floats_per_tile(H, L) * sizeof(float)));
  const int32_t device = a.device;
  HIP_TRY(hipSetDevice(device));
  wos::SirenNet dn = net_view(net);
  PlanArgs pa;
  WOS_TRY(plan_args(device, a.workspace_bytes, wos::siren_fit_tile_lds_bytes(D, H), &pa));
  wos::SirenFitPlan plan{};
  int64_t plan_n = -1;
  const auto plan_of = [&](int64_t n) -> const wos::SirenFitPlan& {  // wos_siren_fit's plan for n rows, per member
    if (n != plan_n) plan = wos::siren_fit_plan(dn, n, pa.stash_cap, pa.resident);
    plan_n = n;
    return plan;
  };
  size_t work = 0;
  for (int64_t i = 0; i < n_iters; i++) work = std::max(work, plan_of(n_of(i)).total(true));
  const DevTmp lay(dn, true, work);
  size_t n_w[wos::kSirenMaxLayers], n_b[wos::kSirenMaxLayers];
  const FitStrides stride{pad64(lay.floats), pad64(layer_counts(net, n_w, n_b))};
  const size_t o_own = E * stride.member, o_g = o_own + gathered, o_state = o_g + E * stride.grad;
  const bool clip = a.opt->max_grad_norm > 0.0, blocking = !(a.flags & WOS_ASYNC);
  return with_tmp(fn, o_state + (size_t)E * wos::kFitStateWords, false, a.flags, st, [&](Tmp& t) -> hipError_t {
    float* tmp = t.base;
    wos::SirenNets nets{};
    wos::AdamMembers adam{};
    wos::SirenGrads dg{};  // member 0's: member e's lie e * stride.grad further on
    for (int e = E - 1; e >= 0; e--) {
      nets.v[e] = dn;
      fit_run_bind(&a.nets[e], tmp + o_g + e * stride.grad, nets.v[e], adam.segs[e], dg);
      adam.exp_avg[e] = a.exp_avg[e];
      adam.exp_avg_sq[e] = a.exp_avg_sq[e];
    }
    int* state = (int*)(tmp + o_state);
    const auto commit = [&](int64_t i) {
      return wos::launch_fit_run_commit_members(E, state, i, a.stop_loss, a.losses, n_iters, a.status, st);
    };
    hipError_t e;
    if ((e = hipMemsetAsync(state, 0, (size_t)E * wos::kFitStateWords * sizeof(float), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.status, 0, (size_t)E * 2 * sizeof(int64_t), st)) != hipSuccess) return e;
    if ((e = hipMemsetD32Async((hipDeviceptr_t)a.losses, 0x7FC00000, (size_t)E * n_iters, st)) != hipSuccess) return e;
    int flags[wos::kSirenMaxMembers * wos::kFitStateWords] = {};  // the state words as last read on the host (check_every > 0)
    bool stopped = false;                                         // every member's flag was set then
    int64_t pending = -1;                                         // the iteration whose commit has not been enqueued yet
    for (int64_t i = 0; i < n_iters && !stopped; i++) {
      FitRows r{};
      if ((e = feed(i, pending, tmp + o_own, state, r)) != hipSuccess) return e;
      const int64_t n = n_of(i);
      if ((e = fit_run_step(nets, E, tmp, lay, stride, r, n, plan_of(n), dg, adam, adam_scalars(*a.opt, a.step0 + i + 1), clip,
                            state, st)) != hipSuccess)
        return e;
      pending = i;
      if (a.check_every > 0 && (i + 1) % a.check_every == 0 && i + 1 < n_iters) {
        if ((e = commit(i)) != hipSuccess) return e;
        pending = -1;
        const size_t words = (size_t)(E - 1) * wos::kFitStateWords + 1;
        if ((e = hipMemcpyAsync(flags, state, words * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        stopped = true;
        for (int m = 0; m < E; m++) stopped = stopped && flags[m * wos::kFitStateWords] != 0;
      }
    }
    if (pending >= 0 && (e = commit(pending)) != hipSuccess) return e;
    if (clamped && blocking) return hipMemcpyAsync(clamped, a.status + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st);
    return hipSuccess;
  });
}

// The pool form for one network and for an ensemble.  Iteration i gathers the rows idx[i * batch ..]
// of the pool into the temporary (the shared points, then per member target | scale); the gather
// carries the commit of the iteration before.
static int fit_run_pool(const std::string& fn, const FitRun& a, const float* pool_pts, const float* const* pool_target,
                        const float* const* pool_scale, int64_t n_pool, const int64_t* idx, int64_t batch) {
  if (int rc = fit_run_nets_check(fn, a)) return rc;
  const int E = a.n_members, D = a.nets[0].d_in, DO = a.nets[0].d_out;
  std::vector<NamedPtr> in{{"pool_pts", pool_pts}, {"pool_target", pool_target}};
  wos::FitPools pools{};
  bool scaled = false;
  for (int e = 0; e < E && pool_target; e++) {
    in.push_back({"pool_target" + of_member(a, e), pool_target[e]});
    pools.target[e] = pool_target[e];
    pools.scale[e] = pool_scale ? pool_scale[e] : nullptr;
    scaled = scaled || pools.scale[e];
  }
  in.push_back({"idx", idx});
  if ((a.flags & WOS_FIT_SCALE_MATRIX) && !scaled)
    return fail(WOS_E_INVALID, fn + ": null pool_scale with WOS_FIT_SCALE_MATRIX (the flag says how pool_scale is laid out)");
  pools.scale_width = scale_width(a.flags, DO);
  const size_t B = (size_t)batch, g_pts = pad64(B * D), g_t = pad64(B * DO), g_s = scaled ? pad64(B * pools.scale_width) : 0,
               g_rows = g_t + g_s;
  int64_t bad = 0;
  const int rc = fit_run_loop(
      fn, a, in,
      [&]() -> int {
        if (batch <= 0) return fail(WOS_E_INVALID, fn + ": batch must be positive, got " + std::to_string(batch));
        if (n_pool <= 0) return fail(WOS_E_INVALID, fn + ": n_pool must be positive, got " + std::to_string(n_pool));
        if (batch > (int64_t)0x7FFFFFFF * wos::kSirenTile)
          return fail(WOS_E_INVALID, fn + ": batch: too many points for one step");
        return WOS_OK;
      },
      [] { return WOS_OK; }, g_pts + E * g_rows, [&](int64_t) { return batch; },
      [&](int64_t i, int64_t pending, float* own, int* state, FitRows& r) {
        float *b_pts = own, *b_t = own + g_pts, *b_s = scaled ? b_t + g_t : nullptr;
        r.pts = b_pts;
        for (int e = 0; e < E; e++) {
          r.m.target[e] = b_t + e * g_rows;
          r.m.scale[e] = pools.scale[e] ? b_s + e * g_rows : nullptr;
        }
        r.m.scale_width = pools.scale_width;
        return wos::launch_fit_run_gather_members(D, DO, E, pool_pts, pools, n_pool, idx + i * batch, batch, b_pts, b_t, b_s,
                                                  g_rows, state, pending, a.stop_loss, a.losses, a.n_iters, a.status, a.st);
      },
      &bad);
  if (rc == WOS_OK && bad != 0)
    return fail(WOS_E_INVALID, fn + ": idx: " + std::to_string(bad) + " indices outside [0, n_pool) were clamped (status[1])");
  return rc;
}

// The form without a pool: iteration i's rows offsets[i] .. offsets[i + 1] - 1 are read in place, with
// wos_siren_fit's plan for that many rows.  The commit that the gather carries there is a launch of
// its own here, between two iterations.
static int fit_run_rows(const std::string& fn, const FitRun& a, const float* pts, const float* const* target,
                        const float* const* scale, const int64_t* offsets) {
  if (int rc = fit_run_nets_check(fn, a)) return rc;
  const int E = a.n_members, D = a.nets[0].d_in, DO = a.nets[0].d_out;
  const int64_t n_iters = a.n_iters;
  std::vector<NamedPtr> in{{"pts", pts}, {"target", target}};
  for (int e = 0; e < E && target; e++) in.push_back({"target" + of_member(a, e), target[e]});
  in.push_back({"offsets", offsets});
  const int SW = scale_width(a.flags, DO);
  if (a.flags & WOS_FIT_SCALE_MATRIX) {
    bool scaled = false;
    for (int e = 0; e < E && scale; e++) scaled = scaled || scale[e];
    if (!scaled) return fail(WOS_E_INVALID, fn + ": null scale with WOS_FIT_SCALE_MATRIX (the flag says how scale is laid out)");
  }
  return fit_run_loop(
      fn, a, in, [] { return WOS_OK; },
      [&]() -> int {
        if (offsets[0] < 0) return fail(WOS_E_INVALID, fn + ": offsets[0] must be >= 0, got " + std::to_string(offsets[0]));
        for (int64_t i = 0; i < n_iters; i++) {
          if (offsets[i + 1] <= offsets[i])
            return fail(WOS_E_INVALID, fn + ": offsets must be strictly increasing: iteration " + std::to_string(i) +
                                           " has no rows (" + std::to_string(offsets[i]) + " to " +
                                           std::to_string(offsets[i + 1]) + "), and its loss is a mean over nothing");
          if (offsets[i + 1] - offsets[i] > (int64_t)0x7FFFFFFF * wos::kSirenTile)
            return fail(WOS_E_INVALID, fn + ": offsets: too many points for one step in iteration " + std::to_string(i));
        }
        return WOS_OK;
      },
      0, [&](int64_t i) { return offsets[i + 1] - offsets[i]; },
      [&](int64_t i, int64_t pending, float*, int* state, FitRows& r) {
        const int64_t row = offsets[i];
        r.pts = pts + row * D;
        for (int e = 0; e < E; e++) {
          r.m.target[e] = target[e] + row * DO;
          r.m.scale[e] = scale && scale[e] ? scale[e] + row * SW : nullptr;
        }
        r.m.scale_width = SW;
        return pending >= 0 ? wos::launch_fit_run_commit_members(E, state, pending, a.stop_loss, a.losses, n_iters, a.status, a.st)
                            : hipSuccess;
      },
      nullptr);
}

extern "C" {

int wos_siren_fit_run(const wos_siren_net* net, const float* pool_pts, const float* pool_target, const float* pool_scale,
                      int64_t n_pool, const int64_t* idx, int64_t n_iters, int64_t batch, float* exp_avg,
                      float* exp_avg_sq, int64_t step0, const wos_adam_params* opt, float stop_loss, int32_t check_every,
                      float* losses, int64_t* status, size_t workspace_bytes, uint32_t flags, int32_t device,
                      void* stream) {
  const FitRun a{false, 1, net, n_iters, &exp_avg, &exp_avg_sq, step0, opt, stop_loss, check_every, losses, status,
                 workspace_bytes, flags, device, (hipStream_t)stream};
  return fit_run_pool("wos_siren_fit_run", a, pool_pts, &pool_target, &pool_scale, n_pool, idx, batch);
}

int wos_siren_fit_run_batches(const wos_siren_net* net, const float* pts, const float* target, const float* scale,
                              const int64_t* offsets, int64_t n_iters, float* exp_avg, float* exp_avg_sq, int64_t step0,
                              const wos_adam_params* opt, float stop_loss, int32_t check_every, float* losses,
                              int64_t* status, size_t workspace_bytes, uint32_t flags, int32_t device, void* stream) {
  const FitRun a{false, 1, net, n_iters, &exp_avg, &exp_avg_sq, step0, opt, stop_loss, check_every, losses, status,
                 workspace_bytes, flags, device, (hipStream_t)stream};
  return fit_run_rows("wos_siren_fit_run_batches", a, pts, &target, &scale, offsets);
}

// The two loops for n_members networks of one shape on the same points, index draw or row offsets,
// optimiser parameters and step0: every launch of an iteration covers all members, and member e ends
// with the bits of the single-network call on its own arguments.
int wos_siren_fit_run_ensemble(int32_t n_members, const wos_siren_net* nets, const float* pool_pts,
                               const float* const* pool_target, const float* const* pool_scale, int64_t n_pool,
                               const int64_t* idx, int64_t n_iters, int64_t batch, float* const* exp_avg,
                               float* const* exp_avg_sq, int64_t step0, const wos_adam_params* opt, float stop_loss,
                               int32_t check_every, float* losses, int64_t* status, size_t workspace_bytes, uint32_t flags,
                               int32_t device, void* stream) {
  const FitRun a{true, n_members, nets, n_iters, exp_avg, exp_avg_sq, step0, opt, stop_loss, check_every, losses, status,
                 workspace_bytes, flags, device, (hipStream_t)stream};
  return fit_run_pool("wos_siren_fit_run_ensemble", a, pool_pts, pool_target, pool_scale, n_pool, idx, batch);
}

int wos_siren_fit_run_batches_ensemble(int32_t n_members, const wos_siren_net* nets, const float* pts,
                                       const float* const* target, const float* const* scale, const int64_t* offsets,
                                       int64_t n_iters, float* const* exp_avg, float* const* exp_avg_sq, int64_t step0,
                                       const wos_adam_params* opt, float stop_loss, int32_t check_every, float* losses,
                                       int64_t* status, size_t workspace_bytes, uint32_t flags, int32_t device,
                                       void* stream) {
  const FitRun a{true, n_members, nets, n_iters, exp_avg, exp_avg_sq, step0, opt, stop_loss, check_every, losses, status,
                 workspace_bytes, flags, device, (hipStream_t)stream};
  return fit_run_rows("wos_siren_fit_run_batches_ensemble", a, pts, target, scale, offsets);
}

}  // extern "C"
