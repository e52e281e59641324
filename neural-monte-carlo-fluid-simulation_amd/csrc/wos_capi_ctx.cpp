// wos_capi_ctx.cpp -- the per-device context behind include/wos.h: its lifecycle, the grow-only
// workspaces, the stat slots and the enqueue protocol every run on the shared workspace follows
// (wos_capi.h), wos_stats, and the entry points that touch nothing else.
#include "wos_capi.h"

namespace wos::capi {

thread_local std::string g_err;
DevCtx g_ctx[kMaxDevices];

// walk tasks per batch: 2^28 tasks = 16 GB of workspace at most (60 B per task, sized for 3D), 5.6 % of a
// MI355X's 288 GB -- config E (2^31 walks) runs in 8 batches, D (2^27) and each rank's share of an 8-GPU
// E in one.  Fewer batches, fewer ramp-downs of the persistent kernels: against 2^24 (round 5) C 12.8 ->
// 11.6 ms, D 26.0 -> 24.0 ms, E 420 -> 376 ms, first balls of E 127 -> 102 ms, bit-exact
// (profiles/r6c_ab_batch.log; 2^26 / 2^27 in between).  A smaller solve allocates only what it uses.
#ifndef WOS_BATCH_LOG2
#define WOS_BATCH_LOG2 28
#endif
static_assert(WOS_BATCH_LOG2 <= 30, "task indices carry a flag in bit 31 (wos_walk_kernel hand-out)");
constexpr int64_t kDefaultBatchTasks = (int64_t)1 << WOS_BATCH_LOG2;
std::atomic<int64_t> g_max_batch_tasks{kDefaultBatchTasks};

// Length hints (Length hints): walks of >= hint_min steps are listed, those of >=
// express_min steps start first in the next solve, express_per_wave to a wave at issue priority `priority`.
// Express layout: walks of >= solo_min steps a wave each (0: none), the others striped or in blocks, the
// express wave rotating (0) or pinned to the workgroup's lowest SIMD (1).
constexpr HintTuning kDefaultHintTuning = {24, 32, 16, (int32_t)wos::kHintListMax, 0, 64, 0, 0};
std::mutex g_hint_mu;
HintTuning g_hint_tuning = kDefaultHintTuning;

bool HintKey::operator==(const HintKey& o) const {
  return dim == o.dim && wpp == o.wpp && n_walks == o.n_walks && n_anti == o.n_anti && n == o.n &&
         index_base == o.index_base && index_stride == o.index_stride && seed == o.seed && geometry == o.geometry &&
         max_walk_length == o.max_walk_length && steps_before_tikhonov == o.steps_before_tikhonov &&
         steps_before_maximal_spheres == o.steps_before_maximal_spheres && use_cosine == o.use_cosine &&
         ignore_dirichlet == o.ignore_dirichlet && ignore_neumann == o.ignore_neumann &&
         ignore_source == o.ignore_source && force_estimate == o.force_estimate && watertight == o.watertight &&
         double_sided == o.double_sided && epsilon_shell == o.epsilon_shell && min_star_radius == o.min_star_radius &&
         silhouette_precision == o.silhouette_precision && rr_threshold == o.rr_threshold && absorption == o.absorption;
}

static void ctx_free(DevCtx& c) {
  hipFree(c.d_pts); hipFree(c.d_p); hipFree(c.d_g); hipFree(c.d_nest); hipFree(c.d_steps);
  hipFree(c.d_pvar); hipFree(c.d_gvar);
  c.d_pvar = c.d_gvar = nullptr;
  c.ws_var_points = 0;
  hipFree(c.d_jump); hipFree(c.d_tasks); hipFree(c.d_pstate); hipFree(c.d_counters); hipFree(c.d_rejtab);
  c.d_rejtab = nullptr;
  hipFree(c.d_hint_list); hipFree(c.d_hint_express); hipFree(c.d_hint_bits);
  c.d_hint_list = nullptr; c.d_hint_express = nullptr; c.d_hint_bits = nullptr;
  c.hint_bits_tasks = 0;
  c.hint_key_valid = false;
  c.hint_last = false;
  for (StatSlot& q : c.slot) {
    if (q.ev0) hipEventDestroy(q.ev0);
    if (q.ev1) hipEventDestroy(q.ev1);
    if (q.done) hipEventDestroy(q.done);
    for (hipEvent_t e : q.bev) hipEventDestroy(e);
    if (q.h_cnt) hipHostFree(q.h_cnt);
    q = StatSlot{};
  }
  if (c.done) hipEventDestroy(c.done);
  if (c.bvc_dir_done) hipEventDestroy(c.bvc_dir_done);
  if (c.bvc_dir) hipStreamDestroy(c.bvc_dir);
  c.bvc_dir_done = nullptr;
  c.bvc_dir = nullptr;
  for (TaskWs& w : c.side) {
    hipFree(w.tasks); hipFree(w.pstate); hipFree(w.counters);
    if (w.done) hipEventDestroy(w.done);
    if (w.stream) hipStreamDestroy(w.stream);
    w = TaskWs{};
  }
  c.d_pts = c.d_p = c.d_g = nullptr;
  c.d_nest = c.d_steps = nullptr;
  c.ws_points = 0;
  c.d_jump = nullptr; c.n_jump = 0;
  c.d_tasks = nullptr; c.task_cap = 0;
  c.d_pstate = nullptr; c.pstate_cap = 0;
  c.d_counters = nullptr;
  c.done = nullptr;
  c.last_stream = nullptr;
  c.inflight = false;
  c.ready = false;
}

// the rejection bound tables (host, computed once per process)
const std::vector<float>& rejection_tables() {
  static std::once_flag once;
  // [2D bound | 3D bound] (DevParams::rej_tab)
  static std::vector<float> t(2 * wos::kRejTabBins);
  std::call_once(once, [] {
    wos::rejection_bound_table(2, t.data());
    wos::rejection_bound_table(3, t.data() + wos::kRejTabBins);
  });
  return t;
}

int ctx_ready(DevCtx& c, int device) {
  if (c.ready) return WOS_OK;
  {
    const std::vector<float>& t = rejection_tables();
    HIP_TRY(hipMalloc((void**)&c.d_rejtab, t.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(c.d_rejtab, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceGetAttribute(&c.num_cus, hipDeviceAttributeMultiprocessorCount, device));
  HIP_TRY(hipMalloc((void**)&c.d_counters, wos::kMainCounterSlots * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(c.d_counters, 0, wos::kMainCounterSlots * sizeof(unsigned long long)));
  for (StatSlot& q : c.slot) {
    HIP_TRY(hipHostMalloc((void**)&q.h_cnt, wos::kNumCounters * sizeof(unsigned long long)));
    HIP_TRY(hipEventCreate(&q.ev0));
    HIP_TRY(hipEventCreate(&q.ev1));
    HIP_TRY(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
  }
  HIP_TRY(hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
  c.ready = true;
  return WOS_OK;
}

hipError_t ctx_order(DevCtx& c, hipStream_t st) {
  if (c.inflight && c.last_stream != st && c.done) return hipStreamWaitEvent(st, c.done, 0);
  return hipSuccess;
}

int ctx_mark(DevCtx& c, hipStream_t st) {
  HIP_TRY(hipEventRecord(c.done, st));
  c.last_stream = st;
  return WOS_OK;
}

// ---- workspaces ---------------------------------------------------------------
int ensure_workspace(DevCtx& c, int dim, size_t npts) {
  if (npts <= c.ws_points) return WOS_OK;
  hipFree(c.d_pts); hipFree(c.d_p); hipFree(c.d_g); hipFree(c.d_nest); hipFree(c.d_steps);
  c.d_pts = c.d_p = c.d_g = nullptr; c.d_nest = c.d_steps = nullptr; c.ws_points = 0;
  const size_t cap = npts + npts / 4 + 1024;
  HIP_TRY(hipMalloc((void**)&c.d_pts, cap * 3 * sizeof(float)));  // either dimension
  HIP_TRY(hipMalloc((void**)&c.d_p, cap * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&c.d_g, cap * 3 * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&c.d_nest, cap * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&c.d_steps, cap * sizeof(int32_t)));
  (void)dim;
  c.ws_points = cap;
  return WOS_OK;
}

// the variance staging buffers, apart from the rest so a plain wos_solve allocates what it always did
static int ensure_var_workspace(DevCtx& c, size_t npts) {
  if (npts <= c.ws_var_points) return WOS_OK;
  hipFree(c.d_pvar); hipFree(c.d_gvar);
  c.d_pvar = c.d_gvar = nullptr; c.ws_var_points = 0;
  const size_t cap = npts + npts / 4 + 1024;
  HIP_TRY(hipMalloc((void**)&c.d_pvar, cap * sizeof(float)));
  HIP_TRY(hipMalloc((void**)&c.d_gvar, cap * 3 * sizeof(float)));  // either dimension
  c.ws_var_points = cap;
  return WOS_OK;
}

int ensure_tasks_in(float*& d_tasks, int64_t& task_cap, int32_t*& d_pstate, int64_t& pstate_cap, int dim,
                    int64_t tasks, int64_t points, int channels) {
  // sized for 3D records so either dimension fits; task_cap counts one-channel tasks (tf floats),
  // so a batch with several channels asks for its float count in those units
  const int tf = std::max(wos::task_floats(dim), wos::task_floats(3));
  const int tfc = std::max(wos::task_floats(dim, channels), wos::task_floats(3, channels));
  if (channels > 1) tasks = (tasks * tfc + tf - 1) / tf;
  if (tasks > task_cap) {
    hipFree(d_tasks);
    d_tasks = nullptr; task_cap = 0;
    HIP_TRY(hipMalloc((void**)&d_tasks, (size_t)tasks * tf * sizeof(float)));
    task_cap = tasks;
  }
  if (points > pstate_cap) {
    hipFree(d_pstate);
    d_pstate = nullptr; pstate_cap = 0;
    HIP_TRY(hipMalloc((void**)&d_pstate, ((size_t)7 * points + 2 * wos::kCostBuckets) * sizeof(int32_t)));
    pstate_cap = points;
  }
  return WOS_OK;
}

int ensure_tasks(DevCtx& c, int dim, int64_t tasks, int64_t points, int channels) {
  return ensure_tasks_in(c.d_tasks, c.task_cap, c.d_pstate, c.pstate_cap, dim, tasks, points, channels);
}

wos::DevTasks task_view_in(float* d_tasks, int32_t* d_pstate, int64_t pstate_cap, int dim, int64_t T, int32_t wpp,
                           int channels) {
  wos::DevTasks tk{};
  float* f = d_tasks;
  tk.pt = f; f += dim * T;
  tk.thr = f; f += T;
  tk.tsrc = f; f += channels * T;
  tk.dd = f; f += T;
  tk.first = f; f += channels * T;
  tk.bdir = f; f += dim * T;
  tk.sdir = f; f += dim * T;
  tk.total = f; f += channels * T;
  tk.code = (uint32_t*)f;
  tk.pstate = d_pstate;
  tk.perm = (uint32_t*)(d_pstate + pstate_cap);
  tk.prad = (float*)(d_pstate + 2 * pstate_cap);
  tk.hist = (uint32_t*)(d_pstate + 3 * pstate_cap);
  tk.pball = (float*)(d_pstate + 3 * pstate_cap + 2 * wos::kCostBuckets);
  tk.pball_stride = pstate_cap;
  tk.T = T;
  tk.wpp = wpp;
  return tk;
}

wos::DevTasks task_view(DevCtx& c, int dim, int64_t T, int32_t wpp, int channels) {
  return task_view_in(c.d_tasks, c.d_pstate, c.pstate_cap, dim, T, wpp, channels);
}

int ensure_hints(DevCtx& c, int64_t tasks, uint32_t** hc_out) {
  uint32_t* const hc = (uint32_t*)(c.d_counters + wos::kNumCounterSlots);
  *hc_out = hc;
  if (c.d_hint_list && tasks <= c.hint_bits_tasks) return WOS_OK;
  // (re)built from nothing: the lists, a zeroed bitmap and control block, no key.  Blocking, like
  // every growth of the workspace (hipFree waits for the device).
  hipFree(c.d_hint_list); hipFree(c.d_hint_express); hipFree(c.d_hint_bits);
  c.d_hint_list = nullptr; c.d_hint_express = nullptr; c.d_hint_bits = nullptr;
  c.hint_bits_tasks = 0;
  c.hint_key_valid = false;
  const size_t words = (size_t)((tasks + 31) / 32);
  HIP_TRY(hipMalloc(&c.d_hint_list, (size_t)wos::kHintListMax * 2 * sizeof(uint32_t)));
  HIP_TRY(hipMalloc((void**)&c.d_hint_express, (size_t)wos::kHintListMax * sizeof(uint32_t)));
  HIP_TRY(hipMalloc((void**)&c.d_hint_bits, words * sizeof(uint32_t)));
  HIP_TRY(hipMemset(c.d_hint_bits, 0, words * sizeof(uint32_t)));
  uint32_t h[wos::H_WORDS] = {};
  const auto put = [&](int at, const void* p) { std::memcpy(h + at, &p, sizeof(p)); };
  put(wos::H_LIST, c.d_hint_list);
  put(wos::H_EXPRESS, c.d_hint_express);
  put(wos::H_BITS, c.d_hint_bits);
  HIP_TRY(hipMemcpy(hc, h, sizeof(h), hipMemcpyHostToDevice));
  c.hint_bits_tasks = tasks;
  return WOS_OK;
}

int ensure_jump(DevCtx& c, int k_needed) {
  if (k_needed <= c.n_jump) return WOS_OK;
  // >= 2 * 1000 + 2: the wave-cooperative rejection sampler jumps up to 1000 iterations ahead
  const int cap = std::max(k_needed, 4096);
  std::vector<uint64_t> t(2 * (size_t)cap);
  uint64_t A = 1u, Cc = 0u;
  for (int k = 0; k < cap; k++) {
    t[2 * k] = A; t[2 * k + 1] = Cc;
    A = A * wos::kPcgMult;
    Cc = Cc * wos::kPcgMult + wos::kPcgInc;
  }
  hipFree(c.d_jump);
  c.d_jump = nullptr; c.n_jump = 0;
  HIP_TRY(hipMalloc((void**)&c.d_jump, t.size() * sizeof(uint64_t)));
  HIP_TRY(hipMemcpy(c.d_jump, t.data(), t.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  c.n_jump = cap;
  return WOS_OK;
}

// ---- host-pointer staging of a solve's outputs -------------------------------------
int stage_outputs(DevCtx& c, const SolveOut& caller, bool dev_ptrs, int64_t n, int C, int dim, OutStage& o) {
  o.dev = o.host = caller;
  o.n = (size_t)std::max<int64_t>(n, 0);
  o.C = C;
  o.dim = dim;
  o.staged = !dev_ptrs && n > 0;
  if (!o.staged) return WOS_OK;
  WOS_TRY(ensure_workspace(c, dim, o.n * C));
  o.dev.p = c.d_p; o.dev.grad = c.d_g;
  o.dev.n_est = caller.n_est ? c.d_nest : nullptr;
  o.dev.steps = caller.steps ? c.d_steps : nullptr;
  if (caller.p_var || caller.grad_var) {
    WOS_TRY(ensure_var_workspace(c, o.n * C));
    o.dev.p_var = caller.p_var ? c.d_pvar : nullptr;
    o.dev.grad_var = caller.grad_var ? c.d_gvar : nullptr;
  }
  return WOS_OK;
}

int copy_back(const OutStage& o, hipStream_t st) {
  if (!o.staged) return WOS_OK;
  const size_t n = o.n, nc = o.n * o.C;
  const SolveOut &h = o.host, &d = o.dev;
  HIP_TRY(hipMemcpyAsync(h.p, d.p, nc * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h.grad, d.grad, nc * o.dim * sizeof(float), hipMemcpyDeviceToHost, st));
  if (h.n_est) HIP_TRY(hipMemcpyAsync(h.n_est, d.n_est, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (h.steps) HIP_TRY(hipMemcpyAsync(h.steps, d.steps, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (h.p_var) HIP_TRY(hipMemcpyAsync(h.p_var, d.p_var, nc * sizeof(float), hipMemcpyDeviceToHost, st));
  if (h.grad_var)
    HIP_TRY(hipMemcpyAsync(h.grad_var, d.grad_var, nc * o.dim * sizeof(float), hipMemcpyDeviceToHost, st));
  return WOS_OK;
}

// ---- the enqueue protocol --------------------------------------------------------
int slot_open(DevCtx& c, hipStream_t st, int64_t n_events, int64_t n_batches, const RunShape& shape, StatSlot** out) {
  const uint64_t ticket = c.next_ticket++;
  StatSlot& q = c.slot[ticket % kStatSlots];
  while ((int64_t)q.bev.size() < n_events) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    q.bev.push_back(e);
  }
  q.ticket = ticket;
  q.n_batches = n_batches;
  q.shape = shape;
  HIP_TRY(hipEventRecord(q.ev0, st));
  *out = &q;
  return WOS_OK;
}

int slot_close(StatSlot& q, const unsigned long long* d_cnt, hipStream_t st) {
  HIP_TRY(hipEventRecord(q.ev1, st));
  HIP_TRY(hipMemcpyAsync(q.h_cnt, d_cnt, wos::kNumCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  return WOS_OK;
}

int slot_finish(DevCtx& c, StatSlot& q, hipStream_t st, bool async, wos_stats* stats) {
  HIP_TRY(hipEventRecord(q.done, st));
  WOS_TRY(ctx_mark(c, st));
  c.inflight = true;
  if (async) {
    if (stats) {
      *stats = wos_stats{};
      stats->ticket = q.ticket;
    }
    return WOS_OK;
  }
  HIP_TRY(hipStreamSynchronize(st));
  c.inflight = false;
  return stats ? fill_stats(q, stats) : WOS_OK;
}

// ---- wos_stats -----------------------------------------------------------------------
void stats_from(const unsigned long long* cnt, const RunShape& shape, wos_stats* stats) {
  *stats = wos_stats{};
  stats->walk_steps = cnt[0];
  stats->wasted_steps = cnt[1];
  stats->walks_recorded = cnt[2];
  stats->walks_escaped = cnt[3];
  stats->walks_max_length = cnt[4];
  stats->walks_rr = cnt[5];
  stats->walks_dirichlet = cnt[6];
  stats->points_estimated = cnt[7];
  stats->rejection_iters = cnt[8];
  stats->first_ball_blocks_per_cu = shape.bpc_fb;
  stats->walk_blocks_per_cu = shape.bpc_walk;
  stats->walk_lds_bytes = shape.walk_lds;
  stats->star_grid = shape.star_grid;
  stats->geom_global = shape.geom_global;
  stats->dir_grid = shape.dir_grid;
}

void stats_add_counters(wos_stats* into, const wos_stats& from) {
  into->walk_steps += from.walk_steps; into->wasted_steps += from.wasted_steps;
  into->walks_recorded += from.walks_recorded; into->walks_escaped += from.walks_escaped;
  into->walks_max_length += from.walks_max_length; into->walks_rr += from.walks_rr;
  into->walks_dirichlet += from.walks_dirichlet; into->points_estimated += from.points_estimated;
  into->rejection_iters += from.rejection_iters;
}

int fill_stats(const StatSlot& q, wos_stats* stats) {
  stats_from(q.h_cnt, q.shape, stats);
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, q.ev0, q.ev1));
  stats->kernel_ms = ms;
  stats->walk_launches = (uint64_t)q.n_batches;
  for (int64_t b = 0; b < q.n_batches; b++) {
    const hipEvent_t* ev = &q.bev[4 * b];
    float a = 0.0f, w = 0.0f, f = 0.0f;
    HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&w, ev[1], ev[2]));
    HIP_TRY(hipEventElapsedTime(&f, ev[2], ev[3]));
    stats->first_ball_ms += a; stats->walk_ms += w; stats->fold_ms += f;
  }
  stats->ticket = q.ticket;
  return WOS_OK;
}

}  // namespace wos::capi

using namespace wos::capi;

extern "C" {

const char* wos_last_error(void) { return g_err.c_str(); }
int32_t wos_abi_version(void) { return WOS_ABI_VERSION; }

int32_t wos_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int64_t wos_set_max_batch_tasks(int64_t max_tasks) {
  const int64_t v = max_tasks <= 0 ? kDefaultBatchTasks
                                   : std::min<int64_t>(std::max<int64_t>(max_tasks, (int64_t)1 << 16), (int64_t)1 << 30);
  return g_max_batch_tasks.exchange(v);
}

void wos_set_length_hints(int32_t hint_min, int32_t express_min, int32_t express_per_wave, int32_t capacity,
                          int32_t priority) {
  std::lock_guard<std::mutex> lk(g_hint_mu);
  const HintTuning& d = kDefaultHintTuning;
  HintTuning& t = g_hint_tuning;
  t.hint_min = hint_min < 0 ? d.hint_min : std::min(std::max(hint_min, 1), (int32_t)wos::kHintMinMask);
  t.express_min = express_min < 0 ? d.express_min : std::max(express_min, 1);
  t.express_per_wave = express_per_wave < 0 ? d.express_per_wave : std::min(std::max(express_per_wave, 1), 64);
  t.capacity = capacity < 0 ? d.capacity : std::min(std::max(capacity, 1), (int32_t)wos::kHintListMax);
  t.priority = priority < 0 ? d.priority : std::min(priority, 3);
}

void wos_set_express_layout(int32_t solo_min, int32_t stripe, int32_t placement) {
  std::lock_guard<std::mutex> lk(g_hint_mu);
  const HintTuning& d = kDefaultHintTuning;
  HintTuning& t = g_hint_tuning;
  t.solo_min = solo_min < 0 ? d.solo_min : std::min(solo_min, wos::kHintBins - 1);
  t.stripe = stripe < 0 ? d.stripe : std::min(stripe, 1);
  t.placement = placement < 0 ? d.placement : std::min(placement, 1);
}

void wos_get_express_layout(int32_t* out) {
  if (!out) return;
  std::lock_guard<std::mutex> lk(g_hint_mu);
  out[0] = g_hint_tuning.solo_min;
  out[1] = g_hint_tuning.stripe;
  out[2] = g_hint_tuning.placement;
}

int64_t wos_selftest_express_slot(uint32_t nx, uint32_t express_per_wave, int32_t stripe, uint32_t* out, int64_t rows) {
  int64_t r = 0;
  for (uint32_t n_solo = 0; n_solo <= nx; n_solo++)
    for (uint32_t c = 0; c < nx + 2u; c++)
      for (uint32_t j = 0; j < express_per_wave + 2u; j++) {
        const uint32_t e = wos::express_slot(c, j, nx, n_solo, express_per_wave, stripe != 0 ? 1u : 0u);
        if (e == wos::kExpressNone) continue;
        if (out && r < rows) {
          out[4 * r] = n_solo; out[4 * r + 1] = c; out[4 * r + 2] = j; out[4 * r + 3] = e;
        }
        r++;
      }
  return r;
}

int32_t wos_selftest_hint_key(int32_t field) {
  HintKey a, b;
  int k = 0;
  bool hit = false;
  const auto bump = [&](auto& v) {
    if (k++ == field) { v = v + 1; hit = true; }
  };
  bump(b.dim); bump(b.wpp); bump(b.n_walks); bump(b.n_anti); bump(b.n); bump(b.index_base); bump(b.index_stride);
  bump(b.seed); bump(b.geometry); bump(b.max_walk_length); bump(b.steps_before_tikhonov);
  bump(b.steps_before_maximal_spheres); bump(b.use_cosine); bump(b.ignore_dirichlet); bump(b.ignore_neumann);
  bump(b.ignore_source); bump(b.force_estimate); bump(b.watertight); bump(b.double_sided); bump(b.epsilon_shell);
  bump(b.min_star_radius); bump(b.silhouette_precision); bump(b.rr_threshold); bump(b.absorption);
  static_assert(sizeof(HintKey) == 4 * 4 + 3 * 8 + 2 * 8 + 10 * 4 + 5 * 4 + 4, "a new HintKey field: compare it, bump it here");
  if (field < 0 || !hit) return -1;
  return a == b ? 0 : 1;
}

int wos_length_hint_stats(int32_t device, int64_t* out) {
  if (!out) return fail(WOS_E_INVALID, "wos_length_hint_stats: null output");
  for (int k = 0; k < 4; k++) out[k] = 0;
  if (device < 0 || device >= kMaxDevices) return fail(WOS_E_INVALID, "wos_length_hint_stats: no such device");
  DevCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lk(c.mu);
  if (!c.ready || !c.hint_last || !c.d_hint_list) return WOS_OK;
  HIP_TRY(hipSetDevice(device));
  if (c.inflight) HIP_TRY(hipEventSynchronize(c.done));
  uint32_t h[wos::H_WORDS];
  HIP_TRY(hipMemcpy(h, c.d_counters + wos::kNumCounterSlots, sizeof(h), hipMemcpyDeviceToHost));
  out[0] = h[wos::H_CLAIMED];
  out[1] = h[wos::H_NLIST] > h[wos::H_CAP] ? h[wos::H_NLIST] - h[wos::H_CAP] : 0;
  out[2] = std::min(h[wos::H_NLIST], h[wos::H_CAP]);
  out[3] = h[wos::H_NEXPRESS];
  return WOS_OK;
}

int wos_express_layout_stats(int32_t device, int64_t* out) {
  if (!out) return fail(WOS_E_INVALID, "wos_express_layout_stats: null output");
  for (int k = 0; k < 2; k++) out[k] = 0;
  if (device < 0 || device >= kMaxDevices) return fail(WOS_E_INVALID, "wos_express_layout_stats: no such device");
  DevCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lk(c.mu);
  if (!c.ready || !c.hint_last || !c.d_hint_list) return WOS_OK;
  HIP_TRY(hipSetDevice(device));
  if (c.inflight) HIP_TRY(hipEventSynchronize(c.done));
  uint32_t h[wos::H_WORDS];
  HIP_TRY(hipMemcpy(h, c.d_counters + wos::kNumCounterSlots, sizeof(h), hipMemcpyDeviceToHost));
  out[0] = h[wos::H_NSOLO];
  out[1] = h[wos::H_XG];
  return WOS_OK;
}

int wos_release_caches(int32_t device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
  for (int dv = 0; dv < std::min(ndev, kMaxDevices); dv++) {
    if (device >= 0 && dv != device) continue;
    DevCtx& c = g_ctx[dv];
    std::unique_lock<std::mutex> lk(c.mu);
    // the slot events may be awaited by wos_solve_stats outside the lock
    c.no_waiters.wait(lk, [&] { return c.stat_waiters == 0; });
    if (!c.ready) continue;
    HIP_TRY(hipSetDevice(dv));
    HIP_TRY(hipDeviceSynchronize());
    ctx_free(c);
  }
  geom_cache_drop(device);
  return WOS_OK;
}

int wos_solve_stats(wos_scene* s, uint64_t ticket, wos_stats* stats) {
  if (!s || !stats) return fail(WOS_E_INVALID, "wos_solve_stats: null scene/stats");
  const auto unknown = [&] {
    return fail(WOS_E_INVALID, "wos_solve_stats: unknown ticket (more than " + std::to_string(kStatSlots) +
                                   " solves were enqueued on this device after it)");
  };
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  hipEvent_t done = nullptr;
  {
    // only the ticket check and the event handle under the locks: waiting here would
    // stall every other enqueuer on the device behind this solve
    std::lock_guard<std::mutex> lock(s->mu);
    std::lock_guard<std::mutex> lk(c.mu);
    StatSlot& q = c.slot[ticket % kStatSlots];
    if (ticket == 0 || q.ticket != ticket) return unknown();
    done = q.done;
    c.stat_waiters++;
  }
  const hipError_t e = hipEventSynchronize(done);
  std::lock_guard<std::mutex> lock(s->mu);
  std::lock_guard<std::mutex> lk(c.mu);
  if (--c.stat_waiters == 0) c.no_waiters.notify_all();
  if (e != hipSuccess) return fail(WOS_E_DEVICE, std::string("wos_solve_stats: ") + hipGetErrorString(e));
  StatSlot& q = c.slot[ticket % kStatSlots];
  // the slot was recycled by a later solve while we waited (its event re-recorded)
  if (q.ticket != ticket) return unknown();
  HIP_TRY(hipEventSynchronize(q.done));
  return fill_stats(q, stats);
}

}  // extern "C"
