// wos_capi_tape.cpp -- the walk tape (include/wos.h; kernels in wos_tape.hip, wos_tape_index.hip):
// record a solve's walks once, replay them per source, their adjoint, and the cell-sorted index.
// One segment per batch of points.  Per task (T = points * walks per point), one allocation:
//   float  bdir[dim][T] sdir[dim][T] gnorm[T] thr_end[T] term[T] tneu[T]
//   u32    code[T] cell0[T] cnt[T] slot[T + 1]      i32 pstate[points]
// = 8 (dim + 4) bytes per walk (2D 48, 3D 56), and per entry slot 12 bytes: cell, pThr, pNrm.
#include "wos_capi.h"

using namespace wos::capi;

struct TapeSeg {
  int64_t nb = 0, T = 0;  // points, tasks
  uint64_t slots = 0;
  void* buf = nullptr;    // the per-task arrays
  void* ebuf = nullptr;   // the entry slots
  wos::DevTape tp{};
  uint32_t* code = nullptr;
  float* bdir = nullptr;
  float* sdir = nullptr;
  int32_t* pstate = nullptr;
};

// a segment's cell-sorted index (wos_tape_index_build), one allocation:
//   u32 row[cells + 1] cell[n_terms] id[n_terms]   float w[n_terms]   float part[tiles][2][kMaxChannels]
struct TapeIndexSeg {
  void* buf = nullptr;
  wos::DevTapeIndex ix{};
  int64_t bytes = 0, max_row = 0;
};

struct TapeIndex {
  std::vector<TapeIndexSeg> seg;
  int64_t bytes = 0, n_terms = 0, max_row = 0;
  ~TapeIndex() { for (TapeIndexSeg& g : seg) hipFree(g.buf); }
};

struct wos_tape {
  int device = 0;
  std::shared_ptr<Geom> geom;  // kept alive: the tape outlives caches and, harmlessly, its scene
  uint64_t scene_serial = 0;
  int dim = 0;
  int32_t sdims[3] = {0, 0, 0};
  wos::DevParams dp{};         // what the fold reads, and ignore_source
  int64_t n = 0, wpp = 0;
  std::vector<TapeSeg> seg;
  unsigned long long* d_cnt = nullptr;  // the recorded walks' counters (kNumCounters), copied into every replay's stats
  uint32_t* d_flag = nullptr;           // DevTape::overflow
  int64_t n_entries = 0, max_entries = 0, bytes = 0;
  RunShape shape;                    // of the recording's kernels: what every replay's stats report
  std::unique_ptr<TapeIndex> index;  // null until wos_tape_index_build
  ~wos_tape() {
    hipSetDevice(device);
    index.reset();
    for (TapeSeg& g : seg) { hipFree(g.buf); hipFree(g.ebuf); }
    hipFree(d_cnt);
    hipFree(d_flag);
  }
};

static size_t tape_task_bytes(int dim, int64_t T, int64_t nb) {
  return ((size_t)(2 * dim + 4) * T + (size_t)3 * T + (size_t)(T + 1) + (size_t)nb) * 4;
}

// the views into a segment's per-task allocation
static void tape_seg_views(TapeSeg& g, int dim, uint32_t* flag) {
  const int64_t T = g.T;
  float* f = (float*)g.buf;
  g.bdir = f; f += dim * T;
  g.sdir = f; f += dim * T;
  g.tp.gnorm = f; f += T;
  g.tp.thr_end = f; f += T;
  g.tp.term = f; f += T;
  g.tp.tneu = f; f += T;
  uint32_t* u = (uint32_t*)f;
  g.code = u; u += T;
  g.tp.cell0 = u; u += T;
  g.tp.cnt = u; u += T;
  g.tp.slot = u; u += T + 1;
  g.pstate = (int32_t*)u;
  g.tp.overflow = flag;
}

// the scene a replay or an adjoint runs on is the recorded one, with as many channels as the caller
// says and the recorded grid (need_grid: a tape recorded with a null source is refused); s->mu held
static int tape_check_scene(const std::string& fn, const wos_tape* tape, const wos_scene* s, int32_t n_channels,
                            bool need_grid = false) {
  if (s->serial != tape->scene_serial)
    return fail(WOS_E_INVALID, fn + ": the tape was recorded on another scene");
  if (n_channels != s->dev.n_channels)
    return fail(WOS_E_INVALID, fn + ": n_channels " + std::to_string(n_channels) +
                                   " differs from the scene's " + std::to_string(s->dev.n_channels));
  if (need_grid && tape->sdims[0] == 0)
    return fail(WOS_E_INVALID, fn + ": the tape was recorded with a null source (no grid to differentiate)");
  for (int k = 0; k < 3; k++)
    if ((s->dev.source ? s->dev.sdims[k] : 0) != tape->sdims[k])
      return fail(WOS_E_INVALID, fn + ": the scene's source dims differ from the recorded ones "
                                 "(the tape stores grid cells)");
  return WOS_OK;
}

// the replay's and the adjoint's transient [C][T] arrays: the head of the task workspace
static int tape_ensure_tasks(DevCtx& c, const wos_tape* tape, int C) {
  int64_t maxT = 0;
  for (const TapeSeg& g : tape->seg) maxT = std::max(maxT, g.T);
  return maxT > 0 ? ensure_tasks(c, tape->dim, maxT, 0, C) : WOS_OK;
}

extern "C" {

int wos_tape_record(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                    int64_t index_stride, int64_t max_bytes, wos_tape** out, wos_stats* stats, void* stream,
                    uint32_t flags) {
  if (!s || !prm || !out) return fail(WOS_E_INVALID, "wos_tape_record: null scene/params/out");
  *out = nullptr;
  if (n < 0) return fail(WOS_E_INVALID, "wos_tape_record: negative point count");
  if (n > 0 && !pts) return fail(WOS_E_INVALID, "wos_tape_record: null point buffer");
  if (n >= (int64_t)0xFFFFFFF0LL) return fail(WOS_E_INVALID, "wos_tape_record: too many points for one call");
  WOS_TRY(check_params("wos_tape_record", prm));
  if (prm->robust_float)
    return fail(WOS_E_INVALID, "wos_tape_record: robust_float walks are not recorded (reference float semantics only)");
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  WOS_TRY(ctx_ready(c, s->device));
  const int dim = s->geom->host.dim;
  hipStream_t st = (hipStream_t)stream;
  SolvePlan plan;
  WOS_TRY(solve_plan(c, s, prm, SolveExtra{}, true, plan));
  wos::DevParams& dp = plan.dp;
  HIP_TRY(ctx_order(c, st));
  const float* d_pts = pts;
  if (!(flags & WOS_PTRS_DEVICE) && n > 0) {
    WOS_TRY(ensure_workspace(c, dim, (size_t)n));
    HIP_TRY(hipMemcpyAsync(c.d_pts, pts, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, st));
    d_pts = c.d_pts;
  }
  const int64_t wpp = plan.wpp;
  const Batches bt = batches(n, wpp);
  DevBufs tmp;  // the recording pass's own counters and queues; the scan's block sums
  unsigned long long* d_cnt2 = nullptr;
  unsigned long long* d_bsum = nullptr;
  if (n > 0) {
    WOS_TRY(ensure_tasks(c, dim, bt.chunk * wpp, bt.chunk, 1));
    WOS_TRY(solve_grids(c, dim, bt.chunk, true, plan));
    HIP_TRY(tmp.get(&d_cnt2, (size_t)wos::kNumCounterSlots));
    HIP_TRY(tmp.get(&d_bsum, (size_t)wos::tape_slot_blocks(bt.chunk * wpp) + 1));
  }

  std::unique_ptr<wos_tape> tape(new wos_tape());
  tape->device = s->device;
  tape->geom = s->geom;
  tape->scene_serial = s->serial;
  tape->dim = dim;
  for (int k = 0; k < 3; k++) tape->sdims[k] = s->dev.source ? s->dev.sdims[k] : 0;
  tape->dp = dp;
  tape->dp.jump = nullptr;
  tape->dp.rej_tab = nullptr;
  tape->n = n;
  tape->wpp = wpp;
  tape->shape = plan.shape();
  HIP_TRY(hipMalloc((void**)&tape->d_cnt, (wos::kNumCounters + 2) * sizeof(unsigned long long)));
  HIP_TRY(hipMalloc((void**)&tape->d_flag, sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(tape->d_cnt, 0, (wos::kNumCounters + 2) * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(tape->d_flag, 0, sizeof(uint32_t), st));
  tape->bytes = (int64_t)((wos::kNumCounters + 2) * sizeof(unsigned long long) + sizeof(uint32_t));
  unsigned long long* d_stat = tape->d_cnt + wos::kNumCounters;  // entries written: sum, longest walk
  const auto over_cap = [&](int64_t bytes) {
    return fail(WOS_E_CAPACITY, "wos_tape_record: the tape needs more than " + std::to_string(bytes) +
                                    " bytes, max_bytes is " + std::to_string(max_bytes));
  };

  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  HIP_TRY(hipEventCreate(&ev0));
  struct EvGuard { hipEvent_t& a; hipEvent_t& b; ~EvGuard() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); } } evg{ev0, ev1};
  HIP_TRY(hipEventCreate(&ev1));
  HIP_TRY(hipEventRecord(ev0, st));
  if (bt.n_chunks == 0) HIP_TRY(wos::launch_zero(c.d_counters, wos::kNumCounterSlots, nullptr, 0, st));
  tape->seg.reserve((size_t)bt.n_chunks);
  for (int64_t k = 0; k < bt.n_chunks; k++) {
    const int64_t b0 = k * bt.chunk;
    const int64_t nb = std::min(bt.chunk, n - b0);
    tape->seg.emplace_back();
    TapeSeg& g = tape->seg.back();
    g.nb = nb;
    g.T = nb * wpp;
    const size_t tb = tape_task_bytes(dim, g.T, nb);
    if (max_bytes > 0 && tape->bytes + (int64_t)tb > max_bytes) return over_cap(tape->bytes + (int64_t)tb);
    HIP_TRY(hipMalloc(&g.buf, tb));
    tape->bytes += (int64_t)tb;
    tape_seg_views(g, dim, tape->d_flag);
    // the batch as a solve lays it out; the first balls' records go to the tape at once
    wos::DevTasks tk = task_view(c, dim, g.T, (int32_t)wpp, 1);
    wos::DevTasks tkr = tk;
    tkr.bdir = g.bdir;
    tkr.sdir = g.sdir;
    const int64_t bbase = index_base + b0 * index_stride;
    unsigned long long* qslot = c.d_counters + wos::kNumCounters;
    const int walk_grid = (int)std::min<int64_t>(plan.grid_walk, (g.T + 63) / 64);
    WOS_TRY(batch_head(c, dim, plan, k, d_pts + b0 * dim, nb, tk, nullptr, st));
    HIP_TRY(wos::launch_first_balls_rec(dim, plan.dfb, dp, d_pts + b0 * dim, nb, bbase, index_stride, tkr, g.tp,
                                        c.d_counters, (unsigned int*)qslot, plan.grid_fb, plan.shmem_fb_run,
                                        plan.lhs_floats, st));
    // pass 1, the plain walk kernel: its codes bound every walk's entries (its totals, from a
    // zero first-ball source, are not used); its counters are the recording's
    HIP_TRY(hipMemsetAsync(tk.tsrc, 0, (size_t)g.T * sizeof(float), st));
    HIP_TRY(wos::launch_walks(plan.kv, plan.dsc, dp, tk, bbase, index_stride, c.d_counters,
                              (unsigned int*)(c.d_counters + wos::kTaskQueueSlot0), walk_grid, plan.shmem_walk,
                              plan.geom_floats_walk, st));
    HIP_TRY(wos::launch_tape_slots(tk.code, g.T, (uint32_t*)g.tp.slot, d_bsum, st));
    unsigned long long slots = 0;
    HIP_TRY(hipMemcpyAsync(&slots, d_bsum + wos::tape_slot_blocks(g.T), sizeof(slots), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (slots >= (1ull << 31))
      return fail(WOS_E_CAPACITY, "wos_tape_record: a batch's walks need " + std::to_string(slots) +
                                      " entry slots (32-bit slot indices); lower wos_set_max_batch_tasks");
    g.slots = slots;
    const size_t eb = (size_t)std::max<unsigned long long>(slots, 1) * 12;
    if (max_bytes > 0 && tape->bytes + (int64_t)eb > max_bytes) return over_cap(tape->bytes + (int64_t)eb);
    HIP_TRY(hipMalloc(&g.ebuf, eb));
    tape->bytes += (int64_t)eb;
    g.tp.e_cell = (uint32_t*)g.ebuf;
    g.tp.e_thr = (float*)g.ebuf + std::max<unsigned long long>(slots, 1);
    g.tp.e_nrm = g.tp.e_thr + std::max<unsigned long long>(slots, 1);
    HIP_TRY(hipMemsetAsync(g.ebuf, 0, eb, st));  // slots a walk leaves unused read as cell 0
    // pass 2, the same walks again (deterministic), recording into their slots
    tkr.code = g.code;
    HIP_TRY(wos::launch_zero(d_cnt2, wos::kNumCounterSlots, nullptr, 0, st));
    HIP_TRY(wos::launch_walks_rec(dim, plan.dsc.geom_global != 0, plan.dsc, dp, tkr, g.tp, bbase, index_stride, d_cnt2,
                                  (unsigned int*)(d_cnt2 + wos::kTaskQueueSlot0), walk_grid, plan.shmem_walk,
                                  plan.geom_floats_walk, st));
    HIP_TRY(hipMemcpyAsync(g.pstate, tk.pstate, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(wos::launch_tape_stats(g.code, g.tp.cnt, g.T, d_stat, st));
  }
  HIP_TRY(hipMemcpyAsync(tape->d_cnt, c.d_counters, wos::kNumCounters * sizeof(unsigned long long),
                         hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipEventRecord(ev1, st));
  unsigned long long h_cnt[wos::kNumCounters + 2] = {};
  uint32_t h_flag = 0;
  HIP_TRY(hipMemcpyAsync(h_cnt, tape->d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&h_flag, tape->d_flag, sizeof(h_flag), hipMemcpyDeviceToHost, st));
  WOS_TRY(ctx_mark(c, st));
  HIP_TRY(hipStreamSynchronize(st));
  c.inflight = false;
  if (h_flag)
    return fail(WOS_E_DEVICE, "wos_tape_record: a walk outgrew the slots sized for it; the tape is discarded");
  tape->n_entries = (int64_t)h_cnt[wos::kNumCounters];
  tape->max_entries = (int64_t)h_cnt[wos::kNumCounters + 1];
  if (stats) {  // blocking, no slot: no ticket, no per-kernel times; both walk passes count as launches
    stats_from(h_cnt, tape->shape, stats);
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    stats->kernel_ms = ms;
    stats->walk_launches = (uint64_t)(2 * bt.n_chunks);
  }
  *out = tape.release();
  return WOS_OK;
}

int wos_tape_solve(wos_tape* tape, wos_scene* s, int32_t n_channels, float* p, float* grad, float* p_var,
                   float* grad_var, int32_t* n_est, int32_t* steps, wos_stats* stats, void* stream, uint32_t flags) {
  if (!tape || !s) return fail(WOS_E_INVALID, "wos_tape_solve: null tape/scene");
  const int64_t n = tape->n;
  const int dim = tape->dim;
  if (n > 0 && (!p || !grad)) return fail(WOS_E_INVALID, "wos_tape_solve: null output buffer");
  std::lock_guard<std::mutex> lock(s->mu);
  WOS_TRY(tape_check_scene("wos_tape_solve", tape, s, n_channels));
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  WOS_TRY(ctx_ready(c, s->device));
  hipStream_t st = (hipStream_t)stream;
  // the shared workspace, and the source a wos_scene_set_source* on another stream may still write
  HIP_TRY(ctx_order(c, st));
  const int C = n_channels;
  const bool dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  OutStage out;
  WOS_TRY(stage_outputs(c, SolveOut{p, grad, n_est, steps, p_var, grad_var}, dev_ptrs, n, C, dim, out));
  WOS_TRY(tape_ensure_tasks(c, tape, C));
  const int64_t n_chunks = (int64_t)tape->seg.size();
  StatSlot* slot = nullptr;
  WOS_TRY(slot_open(c, st, 4 * n_chunks, n_chunks, tape->shape, &slot));
  StatSlot& q = *slot;
  int64_t b0 = 0;
  for (int64_t k = 0; k < n_chunks; k++) {
    const TapeSeg& g = tape->seg[(size_t)k];
    hipEvent_t* ev = &q.bev[4 * k];
    wos::DevTasks tk{};  // the solve's fold, unchanged, on the replayed totals
    tk.total = c.d_tasks;
    tk.first = c.d_tasks + (int64_t)C * g.T;
    tk.code = g.code;
    tk.bdir = g.bdir;
    tk.sdir = g.sdir;
    tk.pstate = g.pstate;
    tk.T = g.T;
    tk.wpp = (int32_t)tape->wpp;
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(hipEventRecord(ev[1], st));  // no first balls: walk_ms is the replay kernel
    HIP_TRY(wos::launch_tape_replay(g.tp, g.code, s->dev, tape->dp.ignore_source, g.T, tk.total, tk.first, st));
    HIP_TRY(hipEventRecord(ev[2], st));
    WOS_TRY(fold_channels(dim, tape->dp, tk, C, g.nb, b0, n, out.dev, st));
    HIP_TRY(hipEventRecord(ev[3], st));
    b0 += g.nb;
  }
  WOS_TRY(slot_close(q, tape->d_cnt, st));
  WOS_TRY(copy_back(out, st));
  return slot_finish(c, q, st, (flags & WOS_ASYNC) && dev_ptrs, stats);
}

// wos_tape_vjp (indexed = false: the scatter's float atomics) and wos_tape_vjp_indexed (the index's
// ordered sums) differ in the kernel that follows the adjoint fold; fn: the name errors carry
static int tape_vjp(const std::string& fn, bool indexed, wos_tape* tape, wos_scene* s, int32_t n_channels,
                    const float* grad_p, const float* grad_grad, float* grad_source, wos_stats* stats, void* stream,
                    uint32_t flags) {
  if (!tape || !s) return fail(WOS_E_INVALID, fn + ": null tape/scene");
  if (!grad_p && !grad_grad) return fail(WOS_E_INVALID, fn + ": both upstream gradients are null");
  if (!grad_source) return fail(WOS_E_INVALID, fn + ": null output buffer");
  const int64_t n = tape->n;
  const int dim = tape->dim;
  std::lock_guard<std::mutex> lock(s->mu);
  WOS_TRY(tape_check_scene(fn, tape, s, n_channels, true));
  int64_t cells = 1;
  for (int k = 0; k < dim; k++) cells *= tape->sdims[k];
  if (cells < 1 || cells > 0xFFFFFFFFLL) return fail(WOS_E_INVALID, fn + ": source grid too large");
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  if (indexed && !tape->index)
    return fail(WOS_E_INVALID, fn + ": the tape has no index (wos_tape_index_build)");
  WOS_TRY(ctx_ready(c, s->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(ctx_order(c, st));  // the shared workspace
  const int C = n_channels;
  const bool dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  const float* d_up = grad_p;
  const float* d_ug = grad_grad;
  float* d_out = grad_source;
  DevBufs tmp;  // host pointers: the device copy of the result
  if (!dev_ptrs) {
    if (n > 0) {
      WOS_TRY(ensure_workspace(c, dim, (size_t)n * C));
      if (grad_p) {
        HIP_TRY(hipMemcpyAsync(c.d_p, grad_p, (size_t)n * C * sizeof(float), hipMemcpyHostToDevice, st));
        d_up = c.d_p;
      }
      if (grad_grad) {
        HIP_TRY(hipMemcpyAsync(c.d_g, grad_grad, (size_t)n * C * dim * sizeof(float), hipMemcpyHostToDevice, st));
        d_ug = c.d_g;
      }
    }
    HIP_TRY(tmp.get(&d_out, (size_t)cells * C));
  }
  // a / c [C][T]: the head of the task workspace, where the replay keeps total / first
  WOS_TRY(tape_ensure_tasks(c, tape, C));
  const bool run = !tape->dp.ignore_source;  // ignoreSource: the map does not depend on the grid
  const int64_t n_chunks = run ? (int64_t)tape->seg.size() : 0;
  // per segment two batches: the adjoint fold (fold_ms), then the scatter or the sum (walk_ms)
  StatSlot* slot = nullptr;
  WOS_TRY(slot_open(c, st, 8 * n_chunks, 2 * n_chunks, tape->shape, &slot));
  StatSlot& q = *slot;
  HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)cells * C * sizeof(float), st));
  int64_t b0 = 0;
  for (int64_t k = 0; k < n_chunks; k++) {
    const TapeSeg& g = tape->seg[(size_t)k];
    hipEvent_t* ev = &q.bev[8 * k];
    float* a = c.d_tasks;
    float* cc = c.d_tasks + (int64_t)C * g.T;
    for (int e = 0; e < 3; e++) HIP_TRY(hipEventRecord(ev[e], st));
    HIP_TRY(wos::launch_tape_adjoint_fold(dim, tape->dp, g.code, g.bdir, g.sdir, g.pstate, g.nb, g.T, (int)tape->wpp, C,
                                          d_up ? d_up + b0 : nullptr, d_ug ? d_ug + b0 * dim : nullptr, n, a, cc, st));
    HIP_TRY(hipEventRecord(ev[3], st));
    HIP_TRY(hipEventRecord(ev[4], st));
    HIP_TRY(hipEventRecord(ev[5], st));
    if (indexed)
      HIP_TRY(wos::launch_tape_rowsum(tape->index->seg[(size_t)k].ix, cells, C, g.T, a, cc, d_out, st));
    else
      HIP_TRY(wos::launch_tape_scatter(g.tp, g.code, cells, C, g.T, a, cc, d_out, st));
    HIP_TRY(hipEventRecord(ev[6], st));
    HIP_TRY(hipEventRecord(ev[7], st));
    b0 += g.nb;
  }
  WOS_TRY(slot_close(q, tape->d_cnt, st));
  if (!dev_ptrs)
    HIP_TRY(hipMemcpyAsync(grad_source, d_out, (size_t)cells * C * sizeof(float), hipMemcpyDeviceToHost, st));
  return slot_finish(c, q, st, (flags & WOS_ASYNC) && dev_ptrs, stats);
}

int wos_tape_vjp(wos_tape* tape, wos_scene* s, int32_t n_channels, const float* grad_p, const float* grad_grad,
                 float* grad_source, wos_stats* stats, void* stream, uint32_t flags) {
  return tape_vjp("wos_tape_vjp", false, tape, s, n_channels, grad_p, grad_grad, grad_source, stats, stream, flags);
}

int wos_tape_vjp_indexed(wos_tape* tape, wos_scene* s, int32_t n_channels, const float* grad_p,
                         const float* grad_grad, float* grad_source, wos_stats* stats, void* stream, uint32_t flags) {
  return tape_vjp("wos_tape_vjp_indexed", true, tape, s, n_channels, grad_p, grad_grad, grad_source, stats, stream,
                  flags);
}

int wos_tape_read(const wos_tape* tape, int32_t segment, int32_t field, int64_t offset, int64_t count, void* dst) {
  if (!tape || !dst) return fail(WOS_E_INVALID, "wos_tape_read: null argument");
  if (segment < 0 || segment >= (int32_t)tape->seg.size())
    return fail(WOS_E_INVALID, "wos_tape_read: segment " + std::to_string(segment) + " of " +
                                   std::to_string(tape->seg.size()));
  const TapeSeg& g = tape->seg[(size_t)segment];
  const int64_t T = g.T, dim = tape->dim;
  const void* src = nullptr;
  int64_t len = 0;
  switch (field) {
    case WOS_TAPE_CODE: src = g.code; len = T; break;
    case WOS_TAPE_CNT: src = g.tp.cnt; len = T; break;
    case WOS_TAPE_SLOT: src = g.tp.slot; len = T + 1; break;
    case WOS_TAPE_CELL0: src = g.tp.cell0; len = T; break;
    case WOS_TAPE_GNORM: src = g.tp.gnorm; len = T; break;
    case WOS_TAPE_THR_END: src = g.tp.thr_end; len = T; break;
    case WOS_TAPE_TERM: src = g.tp.term; len = T; break;
    case WOS_TAPE_TNEU: src = g.tp.tneu; len = T; break;
    case WOS_TAPE_BDIR: src = g.bdir; len = dim * T; break;
    case WOS_TAPE_SDIR: src = g.sdir; len = dim * T; break;
    case WOS_TAPE_E_CELL: src = g.tp.e_cell; len = (int64_t)g.slots; break;
    case WOS_TAPE_E_THR: src = g.tp.e_thr; len = (int64_t)g.slots; break;
    case WOS_TAPE_E_NRM: src = g.tp.e_nrm; len = (int64_t)g.slots; break;
    case WOS_TAPE_PSTATE: src = g.pstate; len = g.nb; break;
    case WOS_TAPE_SEGMENT_POINTS: len = 1; break;
    default: return fail(WOS_E_INVALID, "wos_tape_read: unknown field " + std::to_string(field));
  }
  if (offset < 0 || count < 0 || offset > len || count > len - offset)
    return fail(WOS_E_INVALID, "wos_tape_read: [" + std::to_string(offset) + ", +" + std::to_string(count) +
                                   ") is outside the field's " + std::to_string(len) + " elements");
  if (field == WOS_TAPE_SEGMENT_POINTS) {
    if (count == 1) *(int64_t*)dst = g.nb;
    return WOS_OK;
  }
  if (count == 0) return WOS_OK;
  HIP_TRY(hipSetDevice(tape->device));
  // the tape is written once, by the blocking wos_tape_record
  HIP_TRY(hipMemcpy(dst, (const char*)src + offset * 4, (size_t)count * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

int wos_tape_get_info(const wos_tape* tape, wos_tape_info* info) {
  if (!tape || !info) return fail(WOS_E_INVALID, "wos_tape_get_info: null argument");
  *info = wos_tape_info{};
  info->dim = tape->dim;
  info->n_walks = tape->dp.n_walks;
  for (int k = 0; k < 3; k++) info->source_dims[k] = tape->sdims[k];
  info->device = tape->device;
  info->n_points = tape->n;
  info->n_tasks = tape->n * tape->wpp;
  info->n_entries = tape->n_entries;
  info->max_entries_per_walk = tape->max_entries;
  info->bytes = tape->bytes;
  info->replay_chunk_entries = wos::kTapeChunk;
  return WOS_OK;
}

static int64_t tape_cells(const wos_tape* tape) {
  int64_t cells = 1;
  for (int k = 0; k < tape->dim; k++) cells *= tape->sdims[k];
  return cells;
}

int wos_tape_index_build(wos_tape* tape, int64_t max_bytes) {
  if (!tape) return fail(WOS_E_INVALID, "wos_tape_index_build: null tape");
  if (tape->sdims[0] == 0)
    return fail(WOS_E_INVALID, "wos_tape_index_build: the tape was recorded with a null source (no grid to index)");
  const int64_t cells = tape_cells(tape);
  if (cells < 1 || cells >= 0xFFFFFFFFLL) return fail(WOS_E_INVALID, "wos_tape_index_build: source grid too large");
  HIP_TRY(hipSetDevice(tape->device));
  DevCtx& c = g_ctx[tape->device];
  std::lock_guard<std::mutex> lk(c.mu);
  if (tape->index) return WOS_OK;
  int bits = 1;  // of the keys 0 .. cells - 1; the absent key's low bits, all ones, sort behind them
  while ((1ull << bits) < (uint64_t)cells + 1) bits++;
  const hipStream_t st = nullptr;
  std::unique_ptr<TapeIndex> index(new TapeIndex());
  auto over_cap = [&](int64_t need) {
    return fail(WOS_E_CAPACITY, "wos_tape_index_build: the index and its sort need more than " + std::to_string(need) +
                                    " bytes, max_bytes is " + std::to_string(max_bytes));
  };
  for (const TapeSeg& g : tape->seg) {
    // with ignoreSource recorded no term depends on the grid: an empty index
    const int64_t N = tape->dp.ignore_source ? 0 : g.T + (int64_t)g.slots;
    if (N >= 0xFFFFFFFFLL)
      return fail(WOS_E_CAPACITY, "wos_tape_index_build: a segment of " + std::to_string(N) +
                                      " terms (at most 2^32 - 2); record in smaller batches (wos_set_max_batch_tasks)");
    DevBufs tmp;  // the sort's scratch
    uint32_t *key_in = nullptr, *key_out = nullptr, *d_terms = nullptr;
    unsigned long long *val_in = nullptr, *val_out = nullptr;
    char* sort_tmp = nullptr;
    size_t sort_bytes = 0;
    uint32_t n_terms = 0;
    int64_t scratch = 0;
    if (N > 0) {
      HIP_TRY(wos::tape_index_sort(nullptr, &sort_bytes, key_in, key_out, val_in, val_out, N, bits, st));
      scratch = N * 24 + (int64_t)sort_bytes + 4;
      if (max_bytes > 0 && index->bytes + scratch + (cells + 1) * 4 > max_bytes)
        return over_cap(index->bytes + scratch + (cells + 1) * 4);
      HIP_TRY(tmp.get(&key_in, (size_t)N));
      HIP_TRY(tmp.get(&key_out, (size_t)N));
      HIP_TRY(tmp.get(&val_in, (size_t)N));
      HIP_TRY(tmp.get(&val_out, (size_t)N));
      HIP_TRY(tmp.get(&sort_tmp, sort_bytes));
      HIP_TRY(tmp.get(&d_terms, 1));
      HIP_TRY(wos::launch_tape_index_enum(g.tp, g.code, g.T, (int64_t)g.slots, cells, key_in, val_in, st));
      HIP_TRY(wos::tape_index_sort(sort_tmp, &sort_bytes, key_in, key_out, val_in, val_out, N, bits, st));
      HIP_TRY(wos::launch_tape_index_count(key_out, N, d_terms, st));
      HIP_TRY(hipMemcpyAsync(&n_terms, d_terms, sizeof(n_terms), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    const int64_t tiles = wos::tape_index_tiles(n_terms);
    const int64_t bytes = ((cells + 1) + 3 * (int64_t)n_terms + tiles * 2 * wos::kMaxChannels) * 4;
    if (max_bytes > 0 && index->bytes + scratch + bytes > max_bytes) return over_cap(index->bytes + scratch + bytes);
    index->seg.emplace_back();
    TapeIndexSeg& x = index->seg.back();
    HIP_TRY(hipMalloc(&x.buf, (size_t)bytes));
    x.bytes = bytes;
    index->bytes += bytes;
    uint32_t* u = (uint32_t*)x.buf;
    uint32_t* row = u; u += cells + 1;
    uint32_t* cell = u; u += n_terms;
    uint32_t* id = u; u += n_terms;
    float* w = (float*)u; u += n_terms;
    x.ix = wos::DevTapeIndex{row, cell, id, w, (float*)u, n_terms};
    if (n_terms > 0)
      HIP_TRY(wos::launch_tape_index_finish(key_out, val_out, n_terms, cells, row, cell, id, w, st));
    else
      HIP_TRY(hipMemsetAsync(row, 0, (size_t)(cells + 1) * 4, st));
    std::vector<uint32_t> h_row((size_t)cells + 1);
    HIP_TRY(hipMemcpyAsync(h_row.data(), row, h_row.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t r = 0; r < cells; r++) x.max_row = std::max<int64_t>(x.max_row, (int64_t)h_row[r + 1] - h_row[r]);
    index->n_terms += n_terms;
    index->max_row = std::max(index->max_row, x.max_row);
  }
  tape->index = std::move(index);
  return WOS_OK;
}

int wos_tape_index_get_info(const wos_tape* tape, wos_tape_index_info* info) {
  if (!tape || !info) return fail(WOS_E_INVALID, "wos_tape_index_get_info: null argument");
  *info = wos_tape_index_info{};
  info->n_cells = tape->sdims[0] == 0 ? 0 : tape_cells(tape);
  info->tile_terms = wos::kTapeIndexTile;
  std::lock_guard<std::mutex> lk(g_ctx[tape->device].mu);
  if (!tape->index) return WOS_OK;
  info->built = 1;
  info->n_segments = (int32_t)tape->index->seg.size();
  info->n_terms = tape->index->n_terms;
  info->max_terms_per_cell = tape->index->max_row;
  info->bytes = tape->index->bytes;
  return WOS_OK;
}

int wos_tape_index_read(const wos_tape* tape, int32_t segment, int32_t field, int64_t offset, int64_t count,
                        void* dst) {
  if (!tape || !dst) return fail(WOS_E_INVALID, "wos_tape_index_read: null argument");
  std::lock_guard<std::mutex> lk(g_ctx[tape->device].mu);
  if (!tape->index) return fail(WOS_E_INVALID, "wos_tape_index_read: the tape has no index (wos_tape_index_build)");
  if (segment < 0 || segment >= (int32_t)tape->index->seg.size())
    return fail(WOS_E_INVALID, "wos_tape_index_read: segment " + std::to_string(segment) + " of " +
                                   std::to_string(tape->index->seg.size()));
  const wos::DevTapeIndex& ix = tape->index->seg[(size_t)segment].ix;
  const void* src = nullptr;
  int64_t len = ix.n_terms;
  switch (field) {
    case WOS_TAPE_INDEX_ROW: src = ix.row; len = tape_cells(tape) + 1; break;
    case WOS_TAPE_INDEX_ID: src = ix.id; break;
    case WOS_TAPE_INDEX_W: src = ix.w; break;
    case WOS_TAPE_INDEX_CELL: src = ix.cell; break;
    default: return fail(WOS_E_INVALID, "wos_tape_index_read: unknown field " + std::to_string(field));
  }
  if (offset < 0 || count < 0 || offset > len || count > len - offset)
    return fail(WOS_E_INVALID, "wos_tape_index_read: [" + std::to_string(offset) + ", +" + std::to_string(count) +
                                   ") is outside the field's " + std::to_string(len) + " elements");
  if (count == 0) return WOS_OK;
  HIP_TRY(hipSetDevice(tape->device));
  // the index is written once, by the blocking wos_tape_index_build
  HIP_TRY(hipMemcpy(dst, (const char*)src + offset * 4, (size_t)count * 4, hipMemcpyDeviceToHost));
  return WOS_OK;
}

int wos_tape_destroy(wos_tape* tape) {
  if (!tape) return WOS_OK;
  {
    // a replay enqueued with WOS_ASYNC may still read the tape
    DevCtx& c = g_ctx[tape->device];
    std::lock_guard<std::mutex> lk(c.mu);
    hipSetDevice(tape->device);
    if (c.ready && c.inflight && c.done) hipEventSynchronize(c.done);
  }
  delete tape;
  return WOS_OK;
}

}  // extern "C"
