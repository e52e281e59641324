// wos_capi.h -- what the host units behind include/wos.h share (internal, not installed):
//   wos_capi_ctx.cpp     the per-device context, its workspaces, the stat slots and the enqueue protocol
//   wos_capi_scene.cpp   the geometry cache, meshes, scenes, geometry queries
//   wos_capi_solve.cpp   the solve pipeline (wos_solve*)
//   wos_capi_tape.cpp    the walk tape, its index, replay and adjoint
//   wos_capi_bvc.cpp     boundary value caching
//   wos_capi_probes.cpp  the self-test probes of the solve's kernels
//   wos_capi_siren.cpp   the fused SIREN: forward, backward, fit step, Adam step, the two fit loops, its probes
//
// Device memory lives at three levels, sized for a time-stepper that builds a
// new Scene(sceneConfig, div) for every projection (model_split.py:191):
//   * per device (DevCtx, kept for the process): the solve workspace -- walk
//     tasks, per-point state, PCG32 jump table, counters, staging buffers for
//     host pointers, timing events.  Shared by every scene on the device, so a
//     fresh scene costs no workspace allocation;
//   * per geometry (Geom, shared by content, the 8 most recent kept after their
//     last scene is gone): the prepared boundary records and the star-radius
//     grids built for it, so re-creating a scene on the same boundary skips the
//     preparation and the upload;
//   * per scene: the source grid (replaceable in place, wos_scene_set_source).
// Errors are reported as status codes + wos_last_error(), never by aborting the
// process (the reference aborts: config.h:8-11, scene.h:106-109).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/wos.h"
#include "wos_bvc.h"
#include "wos_detmath.h"
#include "wos_host_scene.h"
#include "wos_launch.h"
#include "wos_siren.h"

namespace wos::capi {

extern thread_local std::string g_err;  // wos_last_error

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) return fail(WOS_E_DEVICE, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// a step that has already reported its failure (fail): pass its status up
#define WOS_TRY(expr)                  \
  do {                                 \
    int _rc = (expr);                  \
    if (_rc != WOS_OK) return _rc;     \
  } while (0)

template <typename T>
hipError_t upload(T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  if (src.empty()) return hipSuccess;
  hipError_t e = hipMalloc((void**)dst, src.size() * sizeof(T));
  if (e != hipSuccess) { *dst = nullptr; return e; }
  e = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) {  // no half-initialised buffer is ever handed out
    hipFree(*dst);
    *dst = nullptr;
  }
  return e;
}

// device allocations of one call, freed on every exit path
struct DevBufs {
  std::vector<void*> p;
  ~DevBufs() { for (void* q : p) hipFree(q); }
  template <typename T>
  hipError_t get(T** out, size_t n) {
    *out = nullptr;
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(1, n) * sizeof(T));
    if (e == hipSuccess) { p.push_back(q); *out = (T*)q; }
    return e;
  }
};

// ---- per-device solve workspace ---------------------------------------------
// Occupancy and LDS layout of a run's kernels, as wos_stats reports them: decided by the solve's
// plan (SolvePlan::shape), kept by the tape for its replays, held by the stat slot until read.
struct RunShape {
  int32_t bpc_fb = 0, bpc_walk = 0, walk_lds = 0, star_grid = 0, geom_global = 0, dir_grid = 0;
};

// Timing events + a pinned copy of the counters of one enqueued solve, so a solve
// enqueued with WOS_ASYNC can report its statistics later (wos_solve_stats) while
// the next solves are already queued behind it.
struct StatSlot {
  uint64_t ticket = 0;                  // 0: empty
  unsigned long long* h_cnt = nullptr;  // pinned host copy of the kNumCounters counters
  hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
  std::vector<hipEvent_t> bev;          // per-chunk kernel boundary events (4 per chunk), grow-only
  int64_t n_batches = 0;
  RunShape shape;
};
constexpr int kStatSlots = 16;

// A walk-task workspace with its own counters and non-blocking stream: boundary value
// caching runs its independent walk sets (the boundary samples' walks, the walks of the
// evaluation points near the Dirichlet boundary) beside the Dirichlet samples' solve on
// the call's stream, so one set's long tail overlaps the others' bulk.
struct TaskWs {
  float* tasks = nullptr;
  int64_t task_cap = 0;
  int32_t* pstate = nullptr;
  int64_t pstate_cap = 0;
  unsigned long long* counters = nullptr;  // kNumCounterSlots
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
};
constexpr int kSideWs = 2;

// Everything that decides a solve's walks (not its values): the length hints a solve leaves are used
// by the next one only if the keys are equal field for field (Length hints).  The point
// coordinates are guarded on the device (the point-setup checksum).
struct HintKey {
  int32_t dim = 0, wpp = 0, n_walks = 0, n_anti = 0;
  int64_t n = 0, index_base = 0, index_stride = 0;
  uint64_t seed = 0, geometry = 0;  // Geom::content_id
  int32_t max_walk_length = 0, steps_before_tikhonov = 0, steps_before_maximal_spheres = 0;
  int32_t use_cosine = 0, ignore_dirichlet = 0, ignore_neumann = 0, ignore_source = 0, force_estimate = 0;
  int32_t watertight = 0, double_sided = 0;
  float epsilon_shell = 0, min_star_radius = 0, silhouette_precision = 0, rr_threshold = 0, absorption = 0;
  bool operator==(const HintKey& o) const;
};
// the tunables of the length hints (wos_set_length_hints) and of the express layout (wos_set_express_layout)
struct HintTuning {
  int32_t hint_min, express_min, express_per_wave, capacity, priority;
  int32_t solo_min, stripe, placement;
};
extern std::mutex g_hint_mu;
extern HintTuning g_hint_tuning;

struct DevCtx {
  std::mutex mu;  // one solve at a time per device (the workspace is shared)
  bool ready = false;
  int num_cus = 0;
  float* d_pts = nullptr;
  float* d_p = nullptr;
  float* d_g = nullptr;
  int32_t* d_nest = nullptr;
  int32_t* d_steps = nullptr;
  size_t ws_points = 0;
  float* d_pvar = nullptr;     // staging of wos_solve_var's host outputs (only once one is asked for)
  float* d_gvar = nullptr;
  size_t ws_var_points = 0;
  uint64_t* d_jump = nullptr;  // PCG32 jump-ahead table (A_k, C_k), grow-only
  int n_jump = 0;
  float* d_tasks = nullptr;    // walk-task workspace (DevTasks arrays), grow-only
  int64_t task_cap = 0;
  int32_t* d_pstate = nullptr; // per-point state + queue permutation of one batch, then bucket counters
  int64_t pstate_cap = 0;
  unsigned long long* d_counters = nullptr;  // kNumCounters u64 + work counters (kMainCounterSlots)
  StatSlot slot[kStatSlots];   // ring indexed by ticket % kStatSlots
  uint64_t next_ticket = 1;
  hipEvent_t done = nullptr;   // end of the last enqueued solve
  hipStream_t last_stream = nullptr;
  bool inflight = false;       // a solve may still run on last_stream
  float* d_rejtab = nullptr;   // rejection bound table, 2D then 3D (DevParams::rej_tab)
  int stat_waiters = 0;        // wos_solve_stats calls waiting on a slot's event without the lock
  std::condition_variable no_waiters;
  // length hints: the device lists behind d_counters' control block, and what the list in it belongs to
  void* d_hint_list = nullptr;        // uint2 [kHintListMax]
  uint32_t* d_hint_express = nullptr; // [kHintListMax]
  uint32_t* d_hint_bits = nullptr;    // one bit per task of the workspace
  int64_t hint_bits_tasks = 0;
  HintKey hint_key;
  bool hint_key_valid = false;
  bool hint_last = false;             // the last solve on the workspace ran with hints (collecting at least)
  TaskWs side[kSideWs];        // boundary value caching's side-stream workspaces (lazy)
  hipStream_t bvc_dir = nullptr;  // boundary value caching: the Dirichlet samples' solve (lazy)
  hipEvent_t bvc_dir_done = nullptr;
};

constexpr int kMaxDevices = 64;
extern DevCtx g_ctx[kMaxDevices];  // never destroyed: the HIP runtime may be gone at process exit
extern std::atomic<int64_t> g_max_batch_tasks;  // wos_set_max_batch_tasks

// caller holds c.mu and has selected the device
int ctx_ready(DevCtx& c, int device);
// order `st` after the last solve enqueued on another stream (the workspace and,
// for set_source, the source grid may still be in use there)
hipError_t ctx_order(DevCtx& c, hipStream_t st);
// `st` now holds the last work enqueued on the shared workspace: c.done, c.last_stream
int ctx_mark(DevCtx& c, hipStream_t st);

int ensure_workspace(DevCtx& c, int dim, size_t npts);
int ensure_tasks_in(float*& d_tasks, int64_t& task_cap, int32_t*& d_pstate, int64_t& pstate_cap, int dim,
                    int64_t tasks, int64_t points, int channels = 1);
int ensure_tasks(DevCtx& c, int dim, int64_t tasks, int64_t points, int channels = 1);
// SoA views into a task workspace for a chunk of T tasks
// (channels: the [C][T] arrays tsrc, first and total of a solve with several source channels)
wos::DevTasks task_view_in(float* d_tasks, int32_t* d_pstate, int64_t pstate_cap, int dim, int64_t T, int32_t wpp,
                           int channels = 1);
wos::DevTasks task_view(DevCtx& c, int dim, int64_t T, int32_t wpp, int channels = 1);
// state_k = A_k * state_0 + C_k for the PCG32 LCG (multiplier kPcgMult, increment kPcgInc)
int ensure_jump(DevCtx& c, int k_needed);
// the length hints' lists for a batch of `tasks` tasks; *hc: the control block
int ensure_hints(DevCtx& c, int64_t tasks, uint32_t** hc);
// the rejection bound tables [2D | 3D] of DevParams::rej_tab (host, computed once per process)
const std::vector<float>& rejection_tables();

// ---- the enqueue protocol of everything that runs on the shared workspace (Boundary) ----
// 1. the next ticket's slot for n_batches batches timed by n_events boundary events (q.bev), holding
//    `shape`; records ev0 on st
int slot_open(DevCtx& c, hipStream_t st, int64_t n_events, int64_t n_batches, const RunShape& shape, StatSlot** out);
// 2. the end of the timed span: ev1, then the kNumCounters counters at d_cnt to the pinned slot
int slot_close(StatSlot& q, const unsigned long long* d_cnt, hipStream_t st);
// 3. after the caller's own copies back: q.done and c.done on st, the context marked in flight; then
//    async: stats hold the ticket alone; else st is synchronised and stats filled (stats may be null)
int slot_finish(DevCtx& c, StatSlot& q, hipStream_t st, bool async, wos_stats* stats);

// counters (kNumCounters, the kernels' order) and shape of a run -> a zeroed wos_stats
void stats_from(const unsigned long long* cnt, const RunShape& shape, wos_stats* stats);
// the nine counters of `from` added to `into`
void stats_add_counters(wos_stats* into, const wos_stats& from);
// statistics of the solve held by slot q (its done event has completed)
int fill_stats(const StatSlot& q, wos_stats* stats);

// A solve's outputs as its kernels see them: the caller's own pointers (WOS_PTRS_DEVICE), else the
// context's staging buffers, copied back once the kernels are enqueued.  [C][n] / [C][n * dim];
// n_est and steps [n]; optional ones null.
struct SolveOut {
  float* p = nullptr;
  float* grad = nullptr;
  int32_t* n_est = nullptr;
  int32_t* steps = nullptr;
  float* p_var = nullptr;
  float* grad_var = nullptr;
};
struct OutStage {
  SolveOut dev, host;  // host: the caller's; dev == host unless staged
  size_t n = 0;
  int C = 1, dim = 2;
  bool staged = false;
};
// grows the staging for C * n points (the variance staging only once a variance is asked for)
int stage_outputs(DevCtx& c, const SolveOut& caller, bool dev_ptrs, int64_t n, int C, int dim, OutStage& o);
int copy_back(const OutStage& o, hipStream_t st);

// ---- prepared geometry, shared by content -----------------------------------
struct Geom {
  int device = 0;
  int dim = 2, double_sided = 0;
  std::vector<float> v, dv;  // the key: exactly the inputs of prepare_scene
  uint64_t content_id = 0;   // a hash of the key (length hints: the geometry's identity across Geom objects)
  std::vector<int32_t> ix, dix;
  wos::HostScene host;
  float *d_prim = nullptr, *d_paux = nullptr, *d_sil = nullptr, *d_dprim = nullptr, *d_dpaux = nullptr;
  float *d_pgroup = nullptr, *d_sgroup = nullptr, *d_dgroup = nullptr;
  float *d_ptree = nullptr, *d_stree = nullptr, *d_dtree = nullptr;
  float* d_nbox = nullptr;  // fcpw's Neumann BVH (stochastic boundary sample)
  int32_t *d_nchild = nullptr, *d_nref = nullptr;
  std::mutex mu;  // star grids
  struct Grid {
    float prec, min_r;
    bool ok;
    wos::StarGrid grid;
    uint32_t* d = nullptr;
  };
  std::list<Grid> grids;  // stable addresses (a solve keeps a pointer)
  // the Dirichlet-distance cell grid (geometry only: built once, on first use)
  bool dgrid_built = false, dgrid_ok = false;
  wos::DirGrid dgrid;
  uint32_t* d_dgrid = nullptr;
  ~Geom();
};

// the star grid of `g` for the solver's silhouette precision and minR (built once)
int star_grid(Geom& g, float prec, float min_r, const Geom::Grid** out);
int dir_grid(Geom& g, bool* ok);
// wos_release_caches: forget the cached geometries of `device` (< 0: of every device)
void geom_cache_drop(int device);

// dynamic LDS a workgroup may use: 160 KB per CU minus the kernels' static LDS
// (rejection jump table 2 KB, counters, histogram)
constexpr size_t kLdsDynamicMax = 160 * 1024 - 4096;

}  // namespace wos::capi

struct wos_scene {
  int device = 0;
  uint64_t serial = 0;  // process-unique, never reused (an address can be)
  std::shared_ptr<wos::capi::Geom> geom;
  wos::DevScene dev{};
  float* d_source = nullptr;
  size_t source_cap = 0;  // floats
  float* d_planar = nullptr;  // staging of a host source with several channels, before the texel pack
  size_t planar_cap = 0;      // floats
  float g_dirichlet = 0.0f;   // wos_scene_desc.dirichlet_value (per-channel constants may replace dev's)
  float* d_dimg = nullptr;  // image-valued Dirichlet data (wos_scene_desc.dirichlet_image)
  float* d_nimg = nullptr;  // image-valued Neumann data (wos_scene_desc.neumann_image)
  std::mutex mu;          // solve vs set_source on the same scene
};

namespace wos::capi {

// ---- the solve pipeline (wos_capi_solve.cpp) ---------------------------------
// The walk kernel's LDS image for a solve on `s`: staged geometry, the star-radius
// grid of the solver's precision / minR (if it fits), the Dirichlet primitives.
struct WalkLayout {
  wos::DevScene dsc;          // the scene with its star grid (or none)
  int geom_floats = 0;        // Neumann records + culling boxes
  int geom_floats_walk = 0;   // + the star grid + the Dirichlet records (the walk kernel)
  size_t shmem_walk = 0;      // dynamic LDS of a walk-kernel workgroup
};
int walk_layout(wos_scene* s, const wos_solver_params* prm, WalkLayout& L);

// DevParams of a solve (walk_on_stars.h WalkSettings from the solver keys)
wos::DevParams dev_params(const wos_solver_params* prm);
// the refusals of solver parameters no kernel can run, under the entry point's name
int check_params(const std::string& fn, const wos_solver_params* prm);

// what a solve needs beyond wos_solve's arguments (BVC's Dirichlet samples): per point the
// direction of the derivative [n][dim] and the derivative out [n] (device pointers), and
// estimation at every point regardless of the inside test
struct SolveExtra {
  const float* ddir = nullptr;
  float* deriv = nullptr;
  bool force_estimate = false;
  int wave_prio = 0;  // the walk / fold kernels' waves at this issue priority (0..3)
  // wos_solve_var: the variances out (host or device pointers like p and grad; null: not asked for)
  float* p_var = nullptr;
  float* grad_var = nullptr;
  // wos_solve_channels: the scene's source channels; every output is channel-major ([C][n], [C][n*dim])
  int channels = 1;
};

// What a solve's kernels are launched with: decided from the scene and the parameters alone
// (solve_plan), then sized for a batch of `chunk` points (solve_grids).  record: the walk
// tape's recording kernels (wos_tape.hip) -- one channel, full Neumann term, no tail spreading.
struct SolvePlan {
  wos::DevParams dp{};
  wos::DevScene dsc{}, dfb{};  // the scene as the walk / the first-ball kernel sees it
  int geom_floats_walk = 0, lhs_floats = 0;
  size_t shmem_walk = 0, shmem_fb = 0, shmem_fb_run = 0;
  int64_t wpp = 0;
  wos::KernelVariant kv{};
  int grid_fb = 0, grid_walk = 0, bpc_fb = 0, bpc_walk = 0;
  RunShape shape() const {
    return {bpc_fb, bpc_walk, (int32_t)shmem_walk, dsc.sgrid != nullptr, dsc.geom_global, dsc.dgrid != nullptr};
  }
};
int solve_plan(DevCtx& c, wos_scene* s, const wos_solver_params* prm, const SolveExtra& ex, bool record, SolvePlan& P);
// grids and residency for batches of `chunk` points (record: of the recording kernels)
int solve_grids(DevCtx& c, int dim, int64_t chunk, bool record, SolvePlan& P);

// Points are solved in batches whose walk tasks fit the task workspace (g_max_batch_tasks).
struct Batches {
  int64_t chunk = 1, n_chunks = 0;  // points per batch, batches
};
Batches batches(int64_t n, int64_t wpp);
// The head of batch `k`, nb points at d_pts: one launch zeroes the counters (first batch: all of
// them; later ones: the queues) and the bucket histogram -- instead of two or three memset
// dispatches; after_zero (or null) is recorded; then the point setup and the LPT order.
// cksum (or null): the point setup adds the points' checksum there (length hints).
int batch_head(DevCtx& c, int dim, const SolvePlan& P, int64_t k, const float* d_pts, int64_t nb,
               const wos::DevTasks& tk, hipEvent_t after_zero, hipStream_t st, unsigned long long* cksum = nullptr);
// One fold per channel of the batch of nb points at b0 of n: only total and first ([C][T] in tk) differ,
// code / bdir / sdir are the walks'.  Outputs channel-major; n_est and steps from channel 0 alone.
int fold_channels(int dim, const wos::DevParams& dp, const wos::DevTasks& tk, int C, int64_t nb, int64_t b0,
                  int64_t n, const SolveOut& out, hipStream_t st);

// wos_solve with the scene's and the device context's locks held
int solve_locked(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                 int64_t index_stride, float* p, float* grad, int32_t* n_est, int32_t* steps, wos_stats* stats,
                 void* stream, uint32_t flags, const SolveExtra& ex);

}  // namespace wos::capi
