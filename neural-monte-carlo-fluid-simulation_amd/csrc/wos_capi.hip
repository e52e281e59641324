// wos_capi.hip -- the extern "C" boundary declared in include/wos.h.
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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <list>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <condition_variable>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/wos.h"
#include "wos_bvc.h"
#include "wos_detmath.h"
#include "wos_host_scene.h"
#include "wos_launch.h"
#include "wos_siren.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) return fail(WOS_E_DEVICE, std::string(#expr ": ") + hipGetErrorString(_e)); \
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

// ---- per-device solve workspace ---------------------------------------------
// Timing events + a pinned copy of the counters of one enqueued solve, so a solve
// enqueued with WOS_ASYNC can report its statistics later (wos_solve_stats) while
// the next solves are already queued behind it.
struct StatSlot {
  uint64_t ticket = 0;                  // 0: empty
  unsigned long long* h_cnt = nullptr;  // pinned host copy of the kNumCounters counters
  hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
  std::vector<hipEvent_t> bev;          // per-chunk kernel boundary events (4 per chunk), grow-only
  int64_t n_batches = 0;
  int32_t bpc_fb = 0, bpc_walk = 0, walk_lds = 0, star_grid = 0, geom_global = 0, dir_grid = 0;
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
  TaskWs side[kSideWs];        // boundary value caching's side-stream workspaces (lazy)
  hipStream_t bvc_dir = nullptr;  // boundary value caching: the Dirichlet samples' solve (lazy)
  hipEvent_t bvc_dir_done = nullptr;
};

constexpr int kMaxDevices = 64;
DevCtx g_ctx[kMaxDevices];  // never destroyed: the HIP runtime may be gone at process exit

void ctx_free(DevCtx& c) {
  hipFree(c.d_pts); hipFree(c.d_p); hipFree(c.d_g); hipFree(c.d_nest); hipFree(c.d_steps);
  hipFree(c.d_pvar); hipFree(c.d_gvar);
  c.d_pvar = c.d_gvar = nullptr;
  c.ws_var_points = 0;
  hipFree(c.d_jump); hipFree(c.d_tasks); hipFree(c.d_pstate); hipFree(c.d_counters); hipFree(c.d_rejtab);
  c.d_rejtab = nullptr;
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

// caller holds c.mu and has selected the device
int ctx_ready(DevCtx& c, int device) {
  if (c.ready) return WOS_OK;
  {
    const std::vector<float>& t = rejection_tables();
    HIP_TRY(hipMalloc((void**)&c.d_rejtab, t.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(c.d_rejtab, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceGetAttribute(&c.num_cus, hipDeviceAttributeMultiprocessorCount, device));
  HIP_TRY(hipMalloc((void**)&c.d_counters, wos::kMainCounterSlots * sizeof(unsigned long long)));
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

// order `st` after the last solve enqueued on another stream (the workspace and,
// for set_source, the source grid may still be in use there)
hipError_t ctx_order(DevCtx& c, hipStream_t st) {
  if (c.inflight && c.last_stream != st && c.done) return hipStreamWaitEvent(st, c.done, 0);
  return hipSuccess;
}

// ---- prepared geometry, shared by content -----------------------------------
struct Geom {
  int device = 0;
  int dim = 2, double_sided = 0;
  std::vector<float> v, dv;  // the key: exactly the inputs of prepare_scene
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
  ~Geom() {
    hipSetDevice(device);
    // a wos_scene_query enqueued with WOS_ASYNC may still read these records: it is ordered against
    // nothing but its stream, and wos_scene_destroy waits for solves only
    hipDeviceSynchronize();
    hipFree(d_prim); hipFree(d_paux); hipFree(d_sil); hipFree(d_dprim); hipFree(d_dpaux);
    hipFree(d_pgroup); hipFree(d_sgroup); hipFree(d_dgroup);
    hipFree(d_ptree); hipFree(d_stree); hipFree(d_dtree);
    hipFree(d_nbox); hipFree(d_nchild); hipFree(d_nref);
    for (Grid& g : grids) hipFree(g.d);
    hipFree(d_dgrid);
  }
};

std::mutex g_geom_mu;
// most recent first; heap-held and never destroyed (no hipFree during static teardown)
std::vector<std::shared_ptr<Geom>>& g_geom_lru = *new std::vector<std::shared_ptr<Geom>>();
constexpr size_t kGeomCacheSize = 8;

template <typename T>
bool same(const std::vector<T>& a, const T* b, int n) {
  return a.size() == (size_t)n && (n == 0 || std::memcmp(a.data(), b, (size_t)n * sizeof(T)) == 0);
}

bool geom_matches(const Geom& g, const wos_scene_desc* d, int device) {
  const int dim = d->dim;
  return g.device == device && g.dim == dim && g.double_sided == d->is_double_sided &&
         same(g.v, d->vertices, d->n_vertices * dim) && same(g.ix, d->prims, d->n_prims * dim) &&
         same(g.dv, d->dvertices, d->n_dvertices * dim) && same(g.dix, d->dprims, d->n_dprims * dim);
}

// the prepared geometry of `d` on `device`: from the cache, else prepared + uploaded
int geom_get(const wos_scene_desc* d, int device, std::shared_ptr<Geom>& out) {
  {
    std::lock_guard<std::mutex> lk(g_geom_mu);
    for (size_t i = 0; i < g_geom_lru.size(); i++)
      if (geom_matches(*g_geom_lru[i], d, device)) {
        out = g_geom_lru[i];
        std::rotate(g_geom_lru.begin(), g_geom_lru.begin() + i, g_geom_lru.begin() + i + 1);
        return WOS_OK;
      }
  }
  auto g = std::make_shared<Geom>();
  const int dim = d->dim;
  g->device = device;
  g->dim = dim;
  g->double_sided = d->is_double_sided;
  if (d->n_vertices > 0) g->v.assign(d->vertices, d->vertices + (size_t)d->n_vertices * dim);
  if (d->n_prims > 0) g->ix.assign(d->prims, d->prims + (size_t)d->n_prims * dim);
  if (d->n_dvertices > 0) g->dv.assign(d->dvertices, d->dvertices + (size_t)d->n_dvertices * dim);
  if (d->n_dprims > 0) g->dix.assign(d->dprims, d->dprims + (size_t)d->n_dprims * dim);
  wos::HostSceneInput in;
  in.dim = dim;
  in.vertices = d->vertices; in.prims = d->prims; in.n_vertices = d->n_vertices; in.n_prims = d->n_prims;
  in.dvertices = d->dvertices; in.dprims = d->dprims; in.n_dvertices = d->n_dvertices; in.n_dprims = d->n_dprims;
  in.is_double_sided = d->is_double_sided;
  std::string err;
  if (!wos::prepare_scene(in, g->host, err)) return fail(WOS_E_INVALID, "wos_scene_create: " + err);
  HIP_TRY(upload(&g->d_prim, g->host.prim));
  HIP_TRY(upload(&g->d_paux, g->host.paux));
  HIP_TRY(upload(&g->d_sil, g->host.sil));
  HIP_TRY(upload(&g->d_dprim, g->host.dprim));
  HIP_TRY(upload(&g->d_dpaux, g->host.dpaux));
  HIP_TRY(upload(&g->d_pgroup, g->host.pgroup));
  HIP_TRY(upload(&g->d_dgroup, g->host.dgroup));
  HIP_TRY(upload(&g->d_sgroup, g->host.sgroup));
  HIP_TRY(upload(&g->d_ptree, g->host.ptree.node));
  HIP_TRY(upload(&g->d_stree, g->host.stree.node));
  HIP_TRY(upload(&g->d_dtree, g->host.dtree.node));
  HIP_TRY(upload(&g->d_nbox, g->host.nbvh.box));
  HIP_TRY(upload(&g->d_nchild, g->host.nbvh.child));
  HIP_TRY(upload(&g->d_nref, g->host.nbvh.ref));
  {
    std::lock_guard<std::mutex> lk(g_geom_mu);
    g_geom_lru.insert(g_geom_lru.begin(), g);
    if (g_geom_lru.size() > kGeomCacheSize) g_geom_lru.pop_back();
  }
  out = g;
  return WOS_OK;
}

// LDS budget of the star-radius grid (staged by every walk-kernel workgroup)
constexpr size_t kStarGridBudget = 16 * 1024;

// dynamic LDS a workgroup may use: 160 KB per CU minus the kernels' static LDS
// (rejection jump table 2 KB, counters, histogram)
constexpr size_t kLdsDynamicMax = 160 * 1024 - 4096;

// the star grid of `g` for the solver's silhouette precision and minR (built once)
int star_grid(Geom& g, float prec, float min_r, const Geom::Grid** out) {
  std::lock_guard<std::mutex> lk(g.mu);
  for (const Geom::Grid& x : g.grids)
    if (x.prec == prec && x.min_r == min_r) { *out = &x; return WOS_OK; }
  Geom::Grid x{prec, min_r, false, {}, nullptr};
  // cached (ok or not) only once its upload has succeeded: a failed upload is reported and
  // the next solve builds the grid again
  if (wos::build_star_grid(g.host, prec, min_r, kStarGridBudget, x.grid)) {
    HIP_TRY(upload(&x.d, x.grid.words));
    x.ok = true;
  }
  g.grids.push_back(std::move(x));
  *out = &g.grids.back();
  return WOS_OK;
}

int dir_grid(Geom& g, bool* ok) {
  std::lock_guard<std::mutex> lk(g.mu);
  if (!g.dgrid_built) {
    // built / ok only once the upload has succeeded (upload leaves d_dgrid null on failure),
    // so no later solve reads a half-initialised grid
    const bool have = wos::build_dirichlet_grid(g.host, g.dgrid);
    if (have) HIP_TRY(upload(&g.d_dgrid, g.dgrid.words));
    g.dgrid_ok = have;
    g.dgrid_built = true;
  }
  *ok = g.dgrid_ok;
  return WOS_OK;
}

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
std::atomic<int64_t> g_max_batch_tasks{kDefaultBatchTasks};  // wos_set_max_batch_tasks
std::atomic<uint64_t> g_scene_serial{0};  // wos_scene::serial: what a walk tape knows its scene by

}  // namespace

struct wos_scene {
  int device = 0;
  uint64_t serial = 0;  // process-unique, never reused (an address can be)
  std::shared_ptr<Geom> geom;
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

extern "C" {

const char* wos_last_error(void) { return g_err.c_str(); }
int32_t wos_abi_version(void) { return WOS_ABI_VERSION; }

int32_t wos_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int wos_load_obj(const char* path, int32_t dim, int32_t flip_orientation, int32_t normalize, wos_mesh* out) {
  if (!path || !out) return fail(WOS_E_INVALID, "wos_load_obj: null argument");
  if (dim != 2 && dim != 3) return fail(WOS_E_INVALID, "wos_load_obj: dim must be 2 or 3");
  std::vector<float> v;
  std::vector<int32_t> ix;
  std::string err;
  if (!wos::load_obj(path, dim, flip_orientation != 0, normalize != 0, v, ix, err))
    return fail(err.rfind("Error opening", 0) == 0 ? WOS_E_IO : WOS_E_INVALID, err);
  out->dim = dim;
  out->n_vertices = (int32_t)(v.size() / dim);
  out->n_prims = (int32_t)(ix.size() / dim);
  out->vertices = (float*)std::malloc(std::max<size_t>(1, v.size()) * sizeof(float));
  out->prims = (int32_t*)std::malloc(std::max<size_t>(1, ix.size()) * sizeof(int32_t));
  if (!out->vertices || !out->prims) return fail(WOS_E_NOMEM, "wos_load_obj: out of memory");
  if (!v.empty()) std::memcpy(out->vertices, v.data(), v.size() * sizeof(float));
  if (!ix.empty()) std::memcpy(out->prims, ix.data(), ix.size() * sizeof(int32_t));
  return WOS_OK;
}

void wos_mesh_free(wos_mesh* mesh) {
  if (!mesh) return;
  std::free(mesh->vertices);
  std::free(mesh->prims);
  mesh->vertices = nullptr;
  mesh->prims = nullptr;
  mesh->n_vertices = mesh->n_prims = 0;
}

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

static int check_source_dims(int dim, const int32_t* dims, size_t* nsrc) {
  const int nsd = dim == 2 ? 2 : 3;
  size_t n = 1;
  for (int k = 0; k < nsd; k++) {
    if (dims[k] <= 0) return fail(WOS_E_INVALID, "bad source dims");
    n *= (size_t)dims[k];
  }
  *nsrc = n;
  return WOS_OK;
}

int wos_scene_create(const wos_scene_desc* d, int32_t device, wos_scene** out) {
  if (!d || !out) return fail(WOS_E_INVALID, "wos_scene_create: null argument");
  *out = nullptr;
  if (d->dim != 2 && d->dim != 3) return fail(WOS_E_INVALID, "wos_scene_create: dim must be 2 or 3");
  size_t nsrc = 0;
  if (d->source && check_source_dims(d->dim, d->source_dims, &nsrc) != WOS_OK)
    return fail(WOS_E_INVALID, "wos_scene_create: bad source dims");
  if (!(d->absorption >= 0.0f)) return fail(WOS_E_INVALID, "wos_scene_create: absorption must be >= 0");
  size_t ndimg = 0;
  if (d->dirichlet_image) {
    if (d->dim != 2) return fail(WOS_E_INVALID, "wos_scene_create: dirichlet_image is 2D only");
    if (d->dirichlet_image_dims[0] < 1 || d->dirichlet_image_dims[1] < 1 ||
        (int64_t)d->dirichlet_image_dims[0] * d->dirichlet_image_dims[1] > (int64_t)1 << 28)
      return fail(WOS_E_INVALID, "wos_scene_create: bad dirichlet_image dims");
    if (!(d->dirichlet_image_box[2] > 0.0f) || !(d->dirichlet_image_box[3] > 0.0f))
      return fail(WOS_E_INVALID, "wos_scene_create: dirichlet_image_box extent must be > 0");
    ndimg = (size_t)d->dirichlet_image_dims[0] * d->dirichlet_image_dims[1];
  }
  size_t nnimg = 0;
  if (d->neumann_image) {
    if (d->dim != 2) return fail(WOS_E_INVALID, "wos_scene_create: neumann_image is 2D only");
    if (d->neumann_image_dims[0] < 1 || d->neumann_image_dims[1] < 1 ||
        (int64_t)d->neumann_image_dims[0] * d->neumann_image_dims[1] > (int64_t)1 << 28)
      return fail(WOS_E_INVALID, "wos_scene_create: bad neumann_image dims");
    const float* nb = d->neumann_image_box;
    if (!std::isfinite(nb[0]) || !std::isfinite(nb[1]) || !(nb[2] > 0.0f) || !(nb[3] > 0.0f) ||
        !std::isfinite(nb[2]) || !std::isfinite(nb[3]))
      return fail(WOS_E_INVALID, "wos_scene_create: neumann_image_box needs a finite corner and extents > 0");
    nnimg = (size_t)d->neumann_image_dims[0] * d->neumann_image_dims[1];
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(WOS_E_DEVICE, "wos_scene_create: no HIP device available");
  if (device < 0 || device >= ndev || device >= kMaxDevices)
    return fail(WOS_E_INVALID, "wos_scene_create: device index out of range");
  HIP_TRY(hipSetDevice(device));
  std::shared_ptr<Geom> geom;
  int rc = geom_get(d, device, geom);
  if (rc != WOS_OK) return rc;
  auto* s = new wos_scene();
  s->device = device;
  s->geom = geom;
  s->serial = g_scene_serial.fetch_add(1) + 1;
  if (d->source) {
    hipError_t e = hipMalloc((void**)&s->d_source, nsrc * sizeof(float));
    if (e == hipSuccess)
      e = hipMemcpy(s->d_source, d->source, nsrc * sizeof(float),
                    d->source_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      hipFree(s->d_source);
      delete s;
      return fail(WOS_E_DEVICE, std::string("wos_scene_create: ") + hipGetErrorString(e));
    }
    s->source_cap = nsrc;
  }
  if (ndimg) {
    hipError_t e = hipMalloc((void**)&s->d_dimg, ndimg * sizeof(float));
    if (e == hipSuccess)
      e = hipMemcpy(s->d_dimg, d->dirichlet_image, ndimg * sizeof(float),
                    d->dirichlet_image_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      hipFree(s->d_dimg);
      hipFree(s->d_source);
      delete s;
      return fail(WOS_E_DEVICE, std::string("wos_scene_create: ") + hipGetErrorString(e));
    }
  }
  if (nnimg) {
    hipError_t e = hipMalloc((void**)&s->d_nimg, nnimg * sizeof(float));
    if (e == hipSuccess)
      e = hipMemcpy(s->d_nimg, d->neumann_image, nnimg * sizeof(float),
                    d->neumann_image_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      hipFree(s->d_nimg);
      hipFree(s->d_dimg);
      hipFree(s->d_source);
      delete s;
      return fail(WOS_E_DEVICE, std::string("wos_scene_create: ") + hipGetErrorString(e));
    }
  }
  const wos::HostScene& h = geom->host;
  wos::DevScene& ds = s->dev;
  ds.dim = d->dim;
  ds.n_prims = h.n_prims;
  ds.n_sil = h.n_sil;
  ds.n_dprims = h.n_dprims;
  ds.prim = geom->d_prim; ds.paux = geom->d_paux; ds.sil = geom->d_sil;
  ds.dprim = geom->d_dprim; ds.dpaux = geom->d_dpaux;
  ds.source = s->d_source;
  ds.pgroup = geom->d_pgroup; ds.sgroup = geom->d_sgroup; ds.dgroup = geom->d_dgroup;
  ds.n_pgroups = h.n_pgroups; ds.n_sgroups = h.n_sgroups; ds.n_dgroups = h.n_dgroups;
  auto tree = [](const wos::HostTree& ht, const float* dnode) {
    wos::DevTree t{};
    t.node = dnode;
    t.levels = ht.levels;
    for (int l = 0; l <= wos::kTreeLevels; l++) { t.n[l] = ht.n[l]; t.off[l] = ht.off[l]; }
    return t;
  };
  ds.ptree = tree(h.ptree, geom->d_ptree);
  ds.stree = tree(h.stree, geom->d_stree);
  ds.dtree = tree(h.dtree, geom->d_dtree);
  ds.nbvh_box = geom->d_nbox;
  ds.nbvh_child = geom->d_nchild;
  ds.nbvh_ref = geom->d_nref;
  ds.nbvh_branch = h.nbvh.branch;
  const int nsd = d->dim == 2 ? 2 : 3;
  for (int k = 0; k < 3; k++) {
    ds.sdims[k] = d->source ? (k < nsd ? d->source_dims[k] : 1) : 0;
    ds.pmin[k] = h.pmin[k]; ds.pmax[k] = h.pmax[k]; ds.ext[k] = h.ext[k];
  }
  ds.absorption = d->absorption;
  ds.g_dirichlet = d->dirichlet_value;
  s->g_dirichlet = d->dirichlet_value;
  ds.n_channels = 1;
  for (int c = 0; c < wos::kMaxChannels; c++) ds.g_ch[c] = d->dirichlet_value;
  ds.dimg = s->d_dimg;
  for (int k = 0; k < 2; k++) ds.ddims[k] = ndimg ? d->dirichlet_image_dims[k] : 0;
  for (int k = 0; k < 4; k++) ds.dbox[k] = ndimg ? d->dirichlet_image_box[k] : 0.0f;
  ds.nimg = s->d_nimg;
  for (int k = 0; k < 2; k++) ds.ndims[k] = nnimg ? d->neumann_image_dims[k] : 0;
  for (int k = 0; k < 4; k++) ds.nbox[k] = nnimg ? d->neumann_image_box[k] : 0.0f;
  ds.watertight = d->is_watertight;
  ds.double_sided = d->is_double_sided;
  *out = s;
  return WOS_OK;
}

int wos_scene_set_source(wos_scene* s, const float* source, const int32_t* dims, int32_t on_device, void* stream) {
  if (!s || !source || !dims) return fail(WOS_E_INVALID, "wos_scene_set_source: null argument");
  size_t nsrc = 0;
  if (check_source_dims(s->dev.dim, dims, &nsrc) != WOS_OK) return fail(WOS_E_INVALID, "wos_scene_set_source: bad source dims");
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  DevCtx& c = g_ctx[s->device];
  {
    std::lock_guard<std::mutex> lk(c.mu);
    HIP_TRY(ctx_order(c, st));  // a solve on another stream may still read the old grid
  }
  if (nsrc > s->source_cap) {
    HIP_TRY(hipStreamSynchronize(st));
    hipFree(s->d_source);
    s->d_source = nullptr;
    s->source_cap = 0;
    HIP_TRY(hipMalloc((void**)&s->d_source, nsrc * sizeof(float)));
    s->source_cap = nsrc;
  }
  HIP_TRY(hipMemcpyAsync(s->d_source, source, nsrc * sizeof(float),
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  const int nsd = s->dev.dim == 2 ? 2 : 3;
  s->dev.source = s->d_source;
  for (int k = 0; k < 3; k++) s->dev.sdims[k] = k < nsd ? dims[k] : 1;
  // back to one channel with the scene's own Dirichlet data
  s->dev.n_channels = 1;
  s->dev.g_dirichlet = s->g_dirichlet;
  for (int c = 0; c < wos::kMaxChannels; c++) s->dev.g_ch[c] = s->g_dirichlet;
  return WOS_OK;
}

int wos_scene_set_source_channels(wos_scene* s, const float* source, int32_t n_channels, const int32_t* dims,
                                  const float* dirichlet_values, int32_t on_device, void* stream) {
  if (!s || !source || !dims) return fail(WOS_E_INVALID, "wos_scene_set_source_channels: null argument");
  if (n_channels < 1 || n_channels > WOS_MAX_CHANNELS)
    return fail(WOS_E_INVALID, "wos_scene_set_source_channels: n_channels must be 1.." + std::to_string(WOS_MAX_CHANNELS) +
                                   ", got " + std::to_string(n_channels));
  if (dirichlet_values && s->d_dimg)
    return fail(WOS_E_INVALID, "wos_scene_set_source_channels: per-channel dirichlet_values cannot be combined with "
                               "the scene's Dirichlet image (image-valued data is shared by the channels)");
  if (n_channels == 1) {  // today's plain copy
    int rc = wos_scene_set_source(s, source, dims, on_device, stream);
    if (rc != WOS_OK) return rc;
    if (dirichlet_values) {
      std::lock_guard<std::mutex> lock(s->mu);
      s->dev.g_dirichlet = dirichlet_values[0];
      for (int c = 0; c < wos::kMaxChannels; c++) s->dev.g_ch[c] = dirichlet_values[0];
    }
    return WOS_OK;
  }
  size_t cells = 0;
  if (check_source_dims(s->dev.dim, dims, &cells) != WOS_OK)
    return fail(WOS_E_INVALID, "wos_scene_set_source_channels: bad source dims");
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  DevCtx& c = g_ctx[s->device];
  {
    std::lock_guard<std::mutex> lk(c.mu);
    HIP_TRY(ctx_order(c, st));  // a solve on another stream may still read the old grid
  }
  const size_t ntex = cells * wos::kMaxChannels, nplanar = cells * (size_t)n_channels;
  if (ntex > s->source_cap || (!on_device && nplanar > s->planar_cap)) HIP_TRY(hipStreamSynchronize(st));
  if (ntex > s->source_cap) {
    hipFree(s->d_source);
    s->d_source = nullptr;
    s->source_cap = 0;
    s->dev.source = nullptr;
    HIP_TRY(hipMalloc((void**)&s->d_source, ntex * sizeof(float)));
    s->source_cap = ntex;
  }
  const float* planar = source;
  if (!on_device) {
    if (nplanar > s->planar_cap) {
      hipFree(s->d_planar);
      s->d_planar = nullptr;
      s->planar_cap = 0;
      HIP_TRY(hipMalloc((void**)&s->d_planar, nplanar * sizeof(float)));
      s->planar_cap = nplanar;
    }
    HIP_TRY(hipMemcpyAsync(s->d_planar, source, nplanar * sizeof(float), hipMemcpyHostToDevice, st));
    planar = s->d_planar;
  }
  HIP_TRY(wos::launch_source_pack(planar, s->d_source, (int64_t)cells, n_channels, st));
  const int nsd = s->dev.dim == 2 ? 2 : 3;
  s->dev.source = s->d_source;
  for (int k = 0; k < 3; k++) s->dev.sdims[k] = k < nsd ? dims[k] : 1;
  s->dev.n_channels = n_channels;
  s->dev.g_dirichlet = s->g_dirichlet;
  for (int ch = 0; ch < wos::kMaxChannels; ch++)
    s->dev.g_ch[ch] = (dirichlet_values && ch < n_channels) ? dirichlet_values[ch] : s->g_dirichlet;
  return WOS_OK;
}

int32_t wos_scene_channels(const wos_scene* s) { return s ? s->dev.n_channels : 0; }

int wos_scene_destroy(wos_scene* s) {
  if (!s) return WOS_OK;
  {
    std::lock_guard<std::mutex> lock(s->mu);
    hipSetDevice(s->device);
    DevCtx& c = g_ctx[s->device];
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.inflight) hipEventSynchronize(c.done);  // an async solve may still read the source
    hipFree(s->d_source);
    hipFree(s->d_planar);
    hipFree(s->d_dimg);
    hipFree(s->d_nimg);
  }
  delete s;
  return WOS_OK;
}

int64_t wos_set_max_batch_tasks(int64_t max_tasks) {
  const int64_t v = max_tasks <= 0 ? kDefaultBatchTasks
                                   : std::min<int64_t>(std::max<int64_t>(max_tasks, (int64_t)1 << 16), (int64_t)1 << 30);
  return g_max_batch_tasks.exchange(v);
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
  std::lock_guard<std::mutex> lk(g_geom_mu);
  if (device < 0) {
    g_geom_lru.clear();
  } else {
    g_geom_lru.erase(std::remove_if(g_geom_lru.begin(), g_geom_lru.end(),
                                    [&](const std::shared_ptr<Geom>& g) { return g->device == device; }),
                     g_geom_lru.end());
  }
  return WOS_OK;
}

int wos_scene_get_info(const wos_scene* s, wos_scene_info* info) {
  if (!s || !info) return fail(WOS_E_INVALID, "wos_scene_get_info: null argument");
  const wos::HostScene& h = s->geom->host;
  info->dim = h.dim;
  info->n_prims = h.n_prims;
  info->n_silhouettes = h.n_sil;
  info->n_dprims = h.n_dprims;
  info->device = s->device;
  for (int k = 0; k < 3; k++) { info->bbox_min[k] = h.pmin[k]; info->bbox_max[k] = h.pmax[k]; }
  return WOS_OK;
}

// Geometry queries (wos_query.hip).  Reads the prepared geometry only: no device-context lock,
// no workspace, no ordering against solves on other streams.  Host pointers are staged through
// one allocation of the call's own, freed before it returns.
int wos_scene_query(wos_scene* s, int32_t which, float boundary_distance_mask, const float* pts, int64_t n,
                    float* dist, float* signed_dist, float* closest, int32_t* state, void* stream, uint32_t flags) {
  if (!s) return fail(WOS_E_INVALID, "wos_scene_query: null scene");
  if (which != WOS_QUERY_NEUMANN && which != WOS_QUERY_DIRICHLET)
    return fail(WOS_E_INVALID, "wos_scene_query: which must be WOS_QUERY_NEUMANN (0) or WOS_QUERY_DIRICHLET (1), got " +
                                   std::to_string(which));
  if (!dist && !signed_dist && !closest && !state)
    return fail(WOS_E_INVALID, "wos_scene_query: no output requested (dist, signed_dist, closest and state are all null)");
  if (n < 0) return fail(WOS_E_INVALID, "wos_scene_query: negative point count");
  if (n >= (int64_t)0xFFFFFFF0LL) return fail(WOS_E_INVALID, "wos_scene_query: too many points for one call");
  const wos::HostScene& host = s->geom->host;
  const int dim = host.dim;
  if ((dist || signed_dist || closest) && (which == WOS_QUERY_NEUMANN ? host.n_prims : host.n_dprims) <= 0)
    return fail(WOS_E_INVALID, std::string("wos_scene_query: the scene holds no ") +
                                   (which == WOS_QUERY_NEUMANN ? "Neumann" : "Dirichlet") +
                                   " boundary (dist, signed_dist and closest need one; state alone does not)");
  if (n == 0) return WOS_OK;
  if (!pts) return fail(WOS_E_INVALID, "wos_scene_query: null point buffer");
  wos::DevScene dsc;
  {
    std::lock_guard<std::mutex> lock(s->mu);  // set_source rewrites the source fields of s->dev
    dsc = s->dev;
  }
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  if (flags & WOS_PTRS_DEVICE) {
    HIP_TRY(wos::launch_point_query(dim, dsc, which, boundary_distance_mask, pts, n, dist, signed_dist, closest,
                                    state, st));
    if (!(flags & WOS_ASYNC)) HIP_TRY(hipStreamSynchronize(st));
    return WOS_OK;
  }
  // one temporary: pts [n][dim] | dist [n] | signed_dist [n] | closest [n][dim] | state [n], 4-byte elements
  const size_t N = (size_t)n;
  const size_t o_dist = N * dim, o_sd = o_dist + (dist ? N : 0), o_cl = o_sd + (signed_dist ? N : 0),
               o_st = o_cl + (closest ? N * dim : 0), total = o_st + (state ? N : 0);
  float* tmp = nullptr;
  if (hipMalloc((void**)&tmp, total * sizeof(float)) != hipSuccess)
    return fail(WOS_E_NOMEM, "wos_scene_query: cannot allocate " + std::to_string(total * sizeof(float)) +
                                 " bytes of staging");
  const auto run = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(tmp, pts, N * dim * sizeof(float), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    e = wos::launch_point_query(dim, dsc, which, boundary_distance_mask, tmp, n, dist ? tmp + o_dist : nullptr,
                                signed_dist ? tmp + o_sd : nullptr, closest ? tmp + o_cl : nullptr,
                                state ? (int32_t*)(tmp + o_st) : nullptr, st);
    if (e != hipSuccess) return e;
    if (dist && (e = hipMemcpyAsync(dist, tmp + o_dist, N * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess)
      return e;
    if (signed_dist &&
        (e = hipMemcpyAsync(signed_dist, tmp + o_sd, N * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess)
      return e;
    if (closest &&
        (e = hipMemcpyAsync(closest, tmp + o_cl, N * dim * sizeof(float), hipMemcpyDeviceToHost, st)) != hipSuccess)
      return e;
    if (state && (e = hipMemcpyAsync(state, tmp + o_st, N * sizeof(int32_t), hipMemcpyDeviceToHost, st)) != hipSuccess)
      return e;
    return hipStreamSynchronize(st);
  };
  const hipError_t e = run();
  if (e != hipSuccess) hipStreamSynchronize(st);  // nothing may still use tmp when it is freed
  hipFree(tmp);
  if (e != hipSuccess) return fail(WOS_E_DEVICE, std::string("wos_scene_query: ") + hipGetErrorString(e));
  return WOS_OK;
}

}  // extern "C"

namespace {

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
int ensure_var_workspace(DevCtx& c, size_t npts) {
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
                    int64_t tasks, int64_t points, int channels = 1) {
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

int ensure_tasks(DevCtx& c, int dim, int64_t tasks, int64_t points, int channels = 1) {
  return ensure_tasks_in(c.d_tasks, c.task_cap, c.d_pstate, c.pstate_cap, dim, tasks, points, channels);
}

// SoA views into a task workspace for a chunk of T tasks
// (channels: the [C][T] arrays tsrc, first and total of a solve with several source channels)
wos::DevTasks task_view_in(float* d_tasks, int32_t* d_pstate, int64_t pstate_cap, int dim, int64_t T, int32_t wpp,
                           int channels = 1) {
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

wos::DevTasks task_view(DevCtx& c, int dim, int64_t T, int32_t wpp, int channels = 1) {
  return task_view_in(c.d_tasks, c.d_pstate, c.pstate_cap, dim, T, wpp, channels);
}

// Stream priorities of boundary value caching's walk sets: the Dirichlet samples' solve and
// the Neumann samples' walks feed the splat (high), the near-boundary walks do not (low).

int bvc_priority(bool high) {
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return 0;
  return high ? greatest : least;
}

// a side workspace's stream, event and counters (created on first use)
int side_ready(TaskWs& w, int priority) {
  if (!w.stream) HIP_TRY(hipStreamCreateWithPriority(&w.stream, hipStreamNonBlocking, priority));
  if (!w.done) HIP_TRY(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
  if (!w.counters) HIP_TRY(hipMalloc((void**)&w.counters, wos::kNumCounterSlots * sizeof(unsigned long long)));
  return WOS_OK;
}

// state_k = A_k * state_0 + C_k for the PCG32 LCG (multiplier kPcgMult, increment kPcgInc)
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

// statistics of the solve held by slot q (its done event has completed)
int fill_stats(const StatSlot& q, wos_stats* stats) {
  *stats = wos_stats{};
  const unsigned long long* cnt = q.h_cnt;
  stats->walk_steps = cnt[0];
  stats->wasted_steps = cnt[1];
  stats->walks_recorded = cnt[2];
  stats->walks_escaped = cnt[3];
  stats->walks_max_length = cnt[4];
  stats->walks_rr = cnt[5];
  stats->walks_dirichlet = cnt[6];
  stats->points_estimated = cnt[7];
  stats->rejection_iters = cnt[8];
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
  stats->first_ball_blocks_per_cu = q.bpc_fb;
  stats->walk_blocks_per_cu = q.bpc_walk;
  stats->walk_lds_bytes = q.walk_lds;
  stats->star_grid = q.star_grid;
  stats->geom_global = q.geom_global;
  stats->dir_grid = q.dir_grid;
  stats->ticket = q.ticket;
  return WOS_OK;
}

// The walk kernel's LDS image for a solve on `s`: staged geometry, the star-radius
// grid of the solver's precision / minR (if it fits), the Dirichlet primitives.
struct WalkLayout {
  wos::DevScene dsc;          // the scene with its star grid (or none)
  int geom_floats = 0;        // Neumann records + culling boxes
  int geom_floats_walk = 0;   // + the star grid + the Dirichlet records (the walk kernel)
  size_t shmem_walk = 0;      // dynamic LDS of a walk-kernel workgroup
};

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
    int rc = star_grid(geom, prm->silhouette_precision, prm->min_star_radius, &gr);
    if (rc != WOS_OK) return rc;
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
    int rc = dir_grid(geom, &ok);
    if (rc != WOS_OK) return rc;
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

// DevParams of a solve (walk_on_stars.h WalkSettings from the solver keys)
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

int solve_locked(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                 int64_t index_stride, float* p, float* grad, int32_t* n_est, int32_t* steps, wos_stats* stats,
                 void* stream, uint32_t flags, const SolveExtra& ex);
int solve_checked(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                  int64_t index_stride, int32_t n_channels, float* p, float* grad, float* p_var, float* grad_var,
                  int32_t* n_est, int32_t* steps, wos_stats* stats, void* stream, uint32_t flags);

}  // namespace

extern "C" {

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

}  // extern "C"

namespace {

// the argument checks of every solve entry point; n_channels 0: wos_solve / wos_solve_var,
// which refuse a scene that holds several channels
int solve_checked(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                  int64_t index_stride, int32_t n_channels, float* p, float* grad, float* p_var, float* grad_var,
                  int32_t* n_est, int32_t* steps, wos_stats* stats, void* stream, uint32_t flags) {
  if (!s || !prm) return fail(WOS_E_INVALID, "wos_solve: null scene/params");
  if (n < 0) return fail(WOS_E_INVALID, "wos_solve: negative point count");
  if (n > 0 && (!pts || !p || !grad)) return fail(WOS_E_INVALID, "wos_solve: null point/output buffer");
  if (n >= (int64_t)0xFFFFFFF0LL) return fail(WOS_E_INVALID, "wos_solve: too many points for one call");
  if (prm->n_walks < 1) return fail(WOS_E_INVALID, "wos_solve: nWalks must be >= 1");
  if (prm->max_walk_length < 0) return fail(WOS_E_INVALID, "wos_solve: maxWalkLength must be >= 0");
  if (!(prm->epsilon_shell >= 0.0f) || !(prm->min_star_radius >= 0.0f) || !(prm->silhouette_precision >= 0.0f))
    return fail(WOS_E_INVALID, "wos_solve: negative tolerance");
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

}  // namespace

extern "C" {

int wos_solve(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
              int64_t index_stride, float* p, float* grad, int32_t* n_est, int32_t* steps, wos_stats* stats,
              void* stream, uint32_t flags) {
  return wos_solve_var(s, prm, pts, n, index_base, index_stride, p, grad, nullptr, nullptr, n_est, steps, stats,
                       stream, flags);
}

}  // extern "C"

namespace {

// What a solve's kernels are launched with: decided from the scene and the parameters alone
// (solve_plan), then sized for a batch of `chunk` points (solve_grids).  record: the walk
// tape's recording kernels (wos_tape.hip) -- one channel, full Neumann term, no tail spreading.
#ifndef WOS_LHS_JUMP_STAGE
#define WOS_LHS_JUMP_STAGE 1
#endif
struct SolvePlan {
  wos::DevParams dp{};
  wos::DevScene dsc{}, dfb{};  // the scene as the walk / the first-ball kernel sees it
  int geom_floats_walk = 0, lhs_floats = 0;
  size_t shmem_walk = 0, shmem_fb = 0, shmem_fb_run = 0;
  int64_t wpp = 0;
  wos::KernelVariant kv{};
  int grid_fb = 0, grid_walk = 0, bpc_fb = 0, bpc_walk = 0;
};

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
    int rc = ensure_jump(c, k_needed);
    if (rc != WOS_OK) return rc;
    dp.jump = c.d_jump;
    dp.n_jump = c.n_jump;
    dp.rej_tab = c.d_rejtab;
  }

  // LDS: the walk kernel's staged geometry; per wave, the first-ball kernel's stratified
  // samples and their shuffle partners
  WalkLayout wl;
  {
    int rc = walk_layout(s, prm, wl);
    if (rc != WOS_OK) return rc;
  }
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

// grids and residency for batches of `chunk` points (record: of the recording kernels)
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

// wos_solve with the scene's and the device context's locks held
int solve_locked(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                 int64_t index_stride, float* p, float* grad, int32_t* n_est, int32_t* steps, wos_stats* stats,
                 void* stream, uint32_t flags, const SolveExtra& ex) {
  Geom& geom = *s->geom;
  const wos::HostScene& host = geom.host;
  const int dim = host.dim;
  hipStream_t st = (hipStream_t)stream;
  DevCtx& c = g_ctx[s->device];
  {
    int rc = ctx_ready(c, s->device);
    if (rc != WOS_OK) return rc;
  }

  // the kernels' parameters, scene views and LDS layout of this solve
  SolvePlan plan;
  {
    int rc = solve_plan(c, s, prm, ex, false, plan);
    if (rc != WOS_OK) return rc;
  }
  wos::DevParams& dp = plan.dp;
  const wos::DevScene& dsc = plan.dsc;
  const wos::DevScene& dfb = plan.dfb;
  const int geom_floats_walk = plan.geom_floats_walk, lhs_floats = plan.lhs_floats;
  const size_t shmem_walk = plan.shmem_walk;
  const wos::KernelVariant kv = plan.kv;

  // the shared workspace may still be in use by a solve enqueued on another stream
  HIP_TRY(ctx_order(c, st));

  const float* d_pts = pts;
  float* d_p = p;
  float* d_g = grad;
  int32_t* d_nest = n_est;
  int32_t* d_steps = steps;
  float* d_pvar = ex.p_var;
  float* d_gvar = ex.grad_var;
  const bool dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  const int C = ex.channels;  // outputs [C][n] / [C][n*dim]: the staging holds C * n points
  if (!dev_ptrs && n > 0) {
    int rc = ensure_workspace(c, dim, (size_t)n * C);
    if (rc != WOS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c.d_pts, pts, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, st));
    d_pts = c.d_pts; d_p = c.d_p; d_g = c.d_g;
    d_nest = n_est ? c.d_nest : nullptr;
    d_steps = steps ? c.d_steps : nullptr;
    if (ex.p_var || ex.grad_var) {
      rc = ensure_var_workspace(c, (size_t)n * C);
      if (rc != WOS_OK) return rc;
      d_pvar = ex.p_var ? c.d_pvar : nullptr;
      d_gvar = ex.grad_var ? c.d_gvar : nullptr;
    }
  }

  // Points are solved in chunks whose walk tasks fit the task workspace.
  const int64_t wpp = (int64_t)dp.n_pairs * dp.n_anti;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, g_max_batch_tasks.load() / wpp));
  const int64_t n_chunks = n > 0 ? (n + chunk - 1) / chunk : 0;
  if (n > 0) {
    int rc = ensure_tasks(c, dim, chunk * wpp, chunk, C);
    if (rc != WOS_OK) return rc;
    rc = solve_grids(c, dim, chunk, false, plan);
    if (rc != WOS_OK) return rc;
  }
  const int grid_fb = plan.grid_fb, grid_walk = plan.grid_walk, bpc_fb = plan.bpc_fb, bpc_walk = plan.bpc_walk;
  const size_t shmem_fb_run = plan.shmem_fb_run;
  const uint64_t ticket = c.next_ticket++;
  StatSlot& q = c.slot[ticket % kStatSlots];
  while ((int64_t)q.bev.size() < 4 * n_chunks) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    q.bev.push_back(e);
  }
  q.ticket = ticket;
  q.n_batches = n_chunks;
  q.bpc_fb = bpc_fb;
  q.bpc_walk = bpc_walk;
  q.walk_lds = (int32_t)shmem_walk;
  q.star_grid = dsc.sgrid != nullptr;
  q.geom_global = dsc.geom_global;
  q.dir_grid = dsc.dgrid != nullptr;
  HIP_TRY(hipEventRecord(q.ev0, st));
  if (n_chunks == 0) HIP_TRY(wos::launch_zero(c.d_counters, wos::kMainCounterSlots, nullptr, 0, st));
  for (int64_t k = 0; k < n_chunks; k++) {
    const int64_t b0 = k * chunk;
    hipEvent_t* ev = &q.bev[4 * k];
    const int64_t nb = std::min(chunk, n - b0);
    wos::DevTasks tk = task_view(c, dim, nb * wpp, (int32_t)wpp, C);
    tk.ddir = ex.ddir ? ex.ddir + b0 * dim : nullptr;
    tk.deriv = ex.deriv ? ex.deriv + b0 : nullptr;
    const int64_t bbase = index_base + b0 * index_stride;
    unsigned long long* qslot = c.d_counters + wos::kNumCounters;
    unsigned int* q_points = (unsigned int*)qslot;
    unsigned int* q_tasks = (unsigned int*)(c.d_counters + wos::kTaskQueueSlot0);
    const int walk_grid = (int)std::min<int64_t>(grid_walk, (tk.T + 63) / 64);
    // one launch zeroes the counters (first chunk: all of them; later chunks: the queues) and
    // the bucket histogram -- instead of two or three memset dispatches
    HIP_TRY(wos::launch_zero(k == 0 ? c.d_counters : qslot,
                             k == 0 ? wos::kNumCounterSlots : wos::kNumCounterSlots - wos::kNumCounters,
                             tk.hist, 2 * wos::kCostBuckets, st));
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(wos::launch_point_setup(dim, dfb, dp, d_pts + b0 * dim, nb, tk, st));
    HIP_TRY(wos::launch_lpt_order(tk, nb, st));
    HIP_TRY(wos::launch_first_balls(kv, dfb, dp, d_pts + b0 * dim, nb, bbase, index_stride, tk, c.d_counters,
                                    q_points, grid_fb, shmem_fb_run, lhs_floats, st));
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(wos::launch_walks(kv, dsc, dp, tk, bbase, index_stride, c.d_counters, q_tasks, walk_grid,
                              shmem_walk, geom_floats_walk, st));
    HIP_TRY(hipEventRecord(ev[2], st));
    // one fold per channel: only total and first differ, code / bdir / sdir are the walks'
    for (int ch = 0; ch < C; ch++) {
      wos::DevTasks tkc = tk;
      tkc.total = tk.total + (int64_t)ch * tk.T;
      tkc.first = tk.first + (int64_t)ch * tk.T;
      const int64_t o1 = (int64_t)ch * n + b0, od = ((int64_t)ch * n + b0) * dim;
      HIP_TRY(wos::launch_fold(dim, dp, tkc, nb, d_p + o1, d_g + od, (d_nest && ch == 0) ? d_nest + b0 : nullptr,
                               (d_steps && ch == 0) ? d_steps + b0 : nullptr, d_pvar ? d_pvar + o1 : nullptr,
                               d_gvar ? d_gvar + od : nullptr, st));
    }
    HIP_TRY(hipEventRecord(ev[3], st));
  }
  HIP_TRY(hipEventRecord(q.ev1, st));
  HIP_TRY(hipMemcpyAsync(q.h_cnt, c.d_counters, wos::kNumCounters * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, st));
  if (!dev_ptrs && n > 0) {
    HIP_TRY(hipMemcpyAsync(p, d_p, (size_t)n * C * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(grad, d_g, (size_t)n * C * dim * sizeof(float), hipMemcpyDeviceToHost, st));
    if (n_est) HIP_TRY(hipMemcpyAsync(n_est, d_nest, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (steps) HIP_TRY(hipMemcpyAsync(steps, d_steps, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (ex.p_var)
      HIP_TRY(hipMemcpyAsync(ex.p_var, d_pvar, (size_t)n * C * sizeof(float), hipMemcpyDeviceToHost, st));
    if (ex.grad_var)
      HIP_TRY(hipMemcpyAsync(ex.grad_var, d_gvar, (size_t)n * C * dim * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipEventRecord(q.done, st));
  HIP_TRY(hipEventRecord(c.done, st));
  c.last_stream = st;
  c.inflight = true;
  if ((flags & WOS_ASYNC) && dev_ptrs) {
    if (stats) {
      *stats = wos_stats{};
      stats->ticket = ticket;
    }
    return WOS_OK;
  }
  HIP_TRY(hipStreamSynchronize(st));
  c.inflight = false;
  wos::diag_dump(dim == 2 ? "2d" : "3d");
  if (stats) {
    int rc = fill_stats(q, stats);
    if (rc != WOS_OK) return rc;
  }
  return WOS_OK;
}

}  // namespace

extern "C" {

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

// ---- walk tape (include/wos.h; kernels in wos_tape.hip) ----------------------------------
// One segment per batch of points.  Per task (T = points * walks per point), one allocation:
//   float  bdir[dim][T] sdir[dim][T] gnorm[T] thr_end[T] term[T] tneu[T]
//   u32    code[T] cell0[T] cnt[T] slot[T + 1]      i32 pstate[points]
// = 8 (dim + 4) bytes per walk (2D 48, 3D 56), and per entry slot 12 bytes: cell, pThr, pNrm.
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
  int32_t bpc_fb = 0, bpc_walk = 0, walk_lds = 0, star_grid = 0, geom_global = 0, dir_grid = 0;
  std::unique_ptr<TapeIndex> index;  // null until wos_tape_index_build
  ~wos_tape() {
    hipSetDevice(device);
    index.reset();
    for (TapeSeg& g : seg) { hipFree(g.buf); hipFree(g.ebuf); }
    hipFree(d_cnt);
    hipFree(d_flag);
  }
};

namespace {

size_t tape_task_bytes(int dim, int64_t T, int64_t nb) {
  return ((size_t)(2 * dim + 4) * T + (size_t)3 * T + (size_t)(T + 1) + (size_t)nb) * 4;
}

// the views into a segment's per-task allocation
void tape_seg_views(TapeSeg& g, int dim, uint32_t* flag) {
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

}  // namespace

extern "C" {

int wos_tape_record(wos_scene* s, const wos_solver_params* prm, const float* pts, int64_t n, int64_t index_base,
                    int64_t index_stride, int64_t max_bytes, wos_tape** out, wos_stats* stats, void* stream,
                    uint32_t flags) {
  if (!s || !prm || !out) return fail(WOS_E_INVALID, "wos_tape_record: null scene/params/out");
  *out = nullptr;
  if (n < 0) return fail(WOS_E_INVALID, "wos_tape_record: negative point count");
  if (n > 0 && !pts) return fail(WOS_E_INVALID, "wos_tape_record: null point buffer");
  if (n >= (int64_t)0xFFFFFFF0LL) return fail(WOS_E_INVALID, "wos_tape_record: too many points for one call");
  if (prm->n_walks < 1) return fail(WOS_E_INVALID, "wos_tape_record: nWalks must be >= 1");
  if (prm->max_walk_length < 0) return fail(WOS_E_INVALID, "wos_tape_record: maxWalkLength must be >= 0");
  if (!(prm->epsilon_shell >= 0.0f) || !(prm->min_star_radius >= 0.0f) || !(prm->silhouette_precision >= 0.0f))
    return fail(WOS_E_INVALID, "wos_tape_record: negative tolerance");
  if (prm->robust_float)
    return fail(WOS_E_INVALID, "wos_tape_record: robust_float walks are not recorded (reference float semantics only)");
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  {
    int rc = ctx_ready(c, s->device);
    if (rc != WOS_OK) return rc;
  }
  const int dim = s->geom->host.dim;
  hipStream_t st = (hipStream_t)stream;
  SolvePlan plan;
  {
    int rc = solve_plan(c, s, prm, SolveExtra{}, true, plan);
    if (rc != WOS_OK) return rc;
  }
  wos::DevParams& dp = plan.dp;
  HIP_TRY(ctx_order(c, st));
  const float* d_pts = pts;
  if (!(flags & WOS_PTRS_DEVICE) && n > 0) {
    int rc = ensure_workspace(c, dim, (size_t)n);
    if (rc != WOS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c.d_pts, pts, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, st));
    d_pts = c.d_pts;
  }
  const int64_t wpp = plan.wpp;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, g_max_batch_tasks.load() / wpp));
  const int64_t n_chunks = n > 0 ? (n + chunk - 1) / chunk : 0;
  DevBufs tmp;  // the recording pass's own counters and queues; the scan's block sums
  unsigned long long* d_cnt2 = nullptr;
  unsigned long long* d_bsum = nullptr;
  if (n > 0) {
    int rc = ensure_tasks(c, dim, chunk * wpp, chunk, 1);
    if (rc != WOS_OK) return rc;
    rc = solve_grids(c, dim, chunk, true, plan);
    if (rc != WOS_OK) return rc;
    HIP_TRY(tmp.get(&d_cnt2, (size_t)wos::kNumCounterSlots));
    HIP_TRY(tmp.get(&d_bsum, (size_t)wos::tape_slot_blocks(chunk * wpp) + 1));
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
  tape->bpc_fb = plan.bpc_fb;
  tape->bpc_walk = plan.bpc_walk;
  tape->walk_lds = (int32_t)plan.shmem_walk;
  tape->star_grid = plan.dsc.sgrid != nullptr;
  tape->geom_global = plan.dsc.geom_global;
  tape->dir_grid = plan.dsc.dgrid != nullptr;
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
  if (n_chunks == 0) HIP_TRY(wos::launch_zero(c.d_counters, wos::kMainCounterSlots, nullptr, 0, st));
  tape->seg.reserve((size_t)n_chunks);
  for (int64_t k = 0; k < n_chunks; k++) {
    const int64_t b0 = k * chunk;
    const int64_t nb = std::min(chunk, n - b0);
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
    HIP_TRY(wos::launch_zero(k == 0 ? c.d_counters : qslot,
                             k == 0 ? wos::kNumCounterSlots : wos::kNumCounterSlots - wos::kNumCounters,
                             tk.hist, 2 * wos::kCostBuckets, st));
    HIP_TRY(wos::launch_point_setup(dim, plan.dfb, dp, d_pts + b0 * dim, nb, tk, st));
    HIP_TRY(wos::launch_lpt_order(tk, nb, st));
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
  HIP_TRY(hipEventRecord(c.done, st));
  c.last_stream = st;
  HIP_TRY(hipStreamSynchronize(st));
  c.inflight = false;
  if (h_flag)
    return fail(WOS_E_DEVICE, "wos_tape_record: a walk outgrew the slots sized for it; the tape is discarded");
  tape->n_entries = (int64_t)h_cnt[wos::kNumCounters];
  tape->max_entries = (int64_t)h_cnt[wos::kNumCounters + 1];
  if (stats) {
    *stats = wos_stats{};
    stats->walk_steps = h_cnt[0];
    stats->wasted_steps = h_cnt[1];
    stats->walks_recorded = h_cnt[2];
    stats->walks_escaped = h_cnt[3];
    stats->walks_max_length = h_cnt[4];
    stats->walks_rr = h_cnt[5];
    stats->walks_dirichlet = h_cnt[6];
    stats->points_estimated = h_cnt[7];
    stats->rejection_iters = h_cnt[8];
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    stats->kernel_ms = ms;
    stats->walk_launches = (uint64_t)(2 * n_chunks);
    stats->first_ball_blocks_per_cu = tape->bpc_fb;
    stats->walk_blocks_per_cu = tape->bpc_walk;
    stats->walk_lds_bytes = tape->walk_lds;
    stats->star_grid = tape->star_grid;
    stats->geom_global = tape->geom_global;
    stats->dir_grid = tape->dir_grid;
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
  if (s->serial != tape->scene_serial)
    return fail(WOS_E_INVALID, "wos_tape_solve: the tape was recorded on another scene");
  if (n_channels != s->dev.n_channels)
    return fail(WOS_E_INVALID, "wos_tape_solve: n_channels " + std::to_string(n_channels) +
                                   " differs from the scene's " + std::to_string(s->dev.n_channels));
  for (int k = 0; k < 3; k++)
    if ((s->dev.source ? s->dev.sdims[k] : 0) != tape->sdims[k])
      return fail(WOS_E_INVALID, "wos_tape_solve: the scene's source dims differ from the recorded ones "
                                 "(the tape stores grid cells)");
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  {
    int rc = ctx_ready(c, s->device);
    if (rc != WOS_OK) return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  // the shared workspace, and the source a wos_scene_set_source* on another stream may still write
  HIP_TRY(ctx_order(c, st));
  const int C = n_channels;
  float* d_p = p;
  float* d_g = grad;
  int32_t* d_nest = n_est;
  int32_t* d_steps = steps;
  float* d_pvar = p_var;
  float* d_gvar = grad_var;
  const bool dev_ptrs = (flags & WOS_PTRS_DEVICE) != 0;
  if (!dev_ptrs && n > 0) {
    int rc = ensure_workspace(c, dim, (size_t)n * C);
    if (rc != WOS_OK) return rc;
    d_p = c.d_p; d_g = c.d_g;
    d_nest = n_est ? c.d_nest : nullptr;
    d_steps = steps ? c.d_steps : nullptr;
    if (p_var || grad_var) {
      rc = ensure_var_workspace(c, (size_t)n * C);
      if (rc != WOS_OK) return rc;
      d_pvar = p_var ? c.d_pvar : nullptr;
      d_gvar = grad_var ? c.d_gvar : nullptr;
    }
  }
  // the replay's transient total / first [C][T]: the head of the task workspace
  int64_t maxT = 0;
  for (const TapeSeg& g : tape->seg) maxT = std::max(maxT, g.T);
  if (maxT > 0) {
    int rc = ensure_tasks(c, dim, maxT, 0, C);
    if (rc != WOS_OK) return rc;
  }
  const int64_t n_chunks = (int64_t)tape->seg.size();
  const uint64_t ticket = c.next_ticket++;
  StatSlot& q = c.slot[ticket % kStatSlots];
  while ((int64_t)q.bev.size() < 4 * n_chunks) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    q.bev.push_back(e);
  }
  q.ticket = ticket;
  q.n_batches = n_chunks;
  q.bpc_fb = tape->bpc_fb;
  q.bpc_walk = tape->bpc_walk;
  q.walk_lds = tape->walk_lds;
  q.star_grid = tape->star_grid;
  q.geom_global = tape->geom_global;
  q.dir_grid = tape->dir_grid;
  HIP_TRY(hipEventRecord(q.ev0, st));
  int64_t b0 = 0;
  for (int64_t k = 0; k < n_chunks; k++) {
    const TapeSeg& g = tape->seg[(size_t)k];
    hipEvent_t* ev = &q.bev[4 * k];
    float* total = c.d_tasks;
    float* first = c.d_tasks + (int64_t)C * g.T;
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(hipEventRecord(ev[1], st));  // no first balls: walk_ms is the replay kernel
    HIP_TRY(wos::launch_tape_replay(g.tp, g.code, s->dev, tape->dp.ignore_source, g.T, total, first, st));
    HIP_TRY(hipEventRecord(ev[2], st));
    wos::DevTasks tk{};
    tk.code = g.code;
    tk.bdir = g.bdir;
    tk.sdir = g.sdir;
    tk.pstate = g.pstate;
    tk.T = g.T;
    tk.wpp = (int32_t)tape->wpp;
    for (int ch = 0; ch < C; ch++) {  // the solve's fold, unchanged, on the replayed totals
      wos::DevTasks tkc = tk;
      tkc.total = total + (int64_t)ch * g.T;
      tkc.first = first + (int64_t)ch * g.T;
      const int64_t o1 = (int64_t)ch * n + b0, od = ((int64_t)ch * n + b0) * dim;
      HIP_TRY(wos::launch_fold(dim, tape->dp, tkc, g.nb, d_p + o1, d_g + od, (d_nest && ch == 0) ? d_nest + b0 : nullptr,
                               (d_steps && ch == 0) ? d_steps + b0 : nullptr, d_pvar ? d_pvar + o1 : nullptr,
                               d_gvar ? d_gvar + od : nullptr, st));
    }
    HIP_TRY(hipEventRecord(ev[3], st));
    b0 += g.nb;
  }
  HIP_TRY(hipEventRecord(q.ev1, st));
  HIP_TRY(hipMemcpyAsync(q.h_cnt, tape->d_cnt, wos::kNumCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                         st));
  if (!dev_ptrs && n > 0) {
    HIP_TRY(hipMemcpyAsync(p, d_p, (size_t)n * C * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(grad, d_g, (size_t)n * C * dim * sizeof(float), hipMemcpyDeviceToHost, st));
    if (n_est) HIP_TRY(hipMemcpyAsync(n_est, d_nest, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (steps) HIP_TRY(hipMemcpyAsync(steps, d_steps, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (p_var) HIP_TRY(hipMemcpyAsync(p_var, d_pvar, (size_t)n * C * sizeof(float), hipMemcpyDeviceToHost, st));
    if (grad_var)
      HIP_TRY(hipMemcpyAsync(grad_var, d_gvar, (size_t)n * C * dim * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipEventRecord(q.done, st));
  HIP_TRY(hipEventRecord(c.done, st));
  c.last_stream = st;
  c.inflight = true;
  if ((flags & WOS_ASYNC) && dev_ptrs) {
    if (stats) {
      *stats = wos_stats{};
      stats->ticket = ticket;
    }
    return WOS_OK;
  }
  HIP_TRY(hipStreamSynchronize(st));
  c.inflight = false;
  if (stats) {
    int rc = fill_stats(q, stats);
    if (rc != WOS_OK) return rc;
  }
  return WOS_OK;
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
  if (s->serial != tape->scene_serial)
    return fail(WOS_E_INVALID, fn + ": the tape was recorded on another scene");
  if (n_channels != s->dev.n_channels)
    return fail(WOS_E_INVALID, fn + ": n_channels " + std::to_string(n_channels) +
                                   " differs from the scene's " + std::to_string(s->dev.n_channels));
  if (tape->sdims[0] == 0)
    return fail(WOS_E_INVALID, fn + ": the tape was recorded with a null source (no grid to differentiate)");
  for (int k = 0; k < 3; k++)
    if ((s->dev.source ? s->dev.sdims[k] : 0) != tape->sdims[k])
      return fail(WOS_E_INVALID, fn + ": the scene's source dims differ from the recorded ones "
                                 "(the tape stores grid cells)");
  int64_t cells = 1;
  for (int k = 0; k < dim; k++) cells *= tape->sdims[k];
  if (cells < 1 || cells > 0xFFFFFFFFLL) return fail(WOS_E_INVALID, fn + ": source grid too large");
  HIP_TRY(hipSetDevice(s->device));
  DevCtx& c = g_ctx[s->device];
  std::lock_guard<std::mutex> lk(c.mu);
  if (indexed && !tape->index)
    return fail(WOS_E_INVALID, fn + ": the tape has no index (wos_tape_index_build)");
  {
    int rc = ctx_ready(c, s->device);
    if (rc != WOS_OK) return rc;
  }
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
      int rc = ensure_workspace(c, dim, (size_t)n * C);
      if (rc != WOS_OK) return rc;
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
  int64_t maxT = 0;
  for (const TapeSeg& g : tape->seg) maxT = std::max(maxT, g.T);
  if (maxT > 0) {
    int rc = ensure_tasks(c, dim, maxT, 0, C);
    if (rc != WOS_OK) return rc;
  }
  const bool run = !tape->dp.ignore_source;  // ignoreSource: the map does not depend on the grid
  const int64_t n_chunks = run ? (int64_t)tape->seg.size() : 0;
  const uint64_t ticket = c.next_ticket++;
  StatSlot& q = c.slot[ticket % kStatSlots];
  while ((int64_t)q.bev.size() < 8 * n_chunks) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    q.bev.push_back(e);
  }
  q.ticket = ticket;
  q.n_batches = 2 * n_chunks;  // per segment: the adjoint fold (fold_ms), then the scatter or the sum (walk_ms)
  q.bpc_fb = tape->bpc_fb;
  q.bpc_walk = tape->bpc_walk;
  q.walk_lds = tape->walk_lds;
  q.star_grid = tape->star_grid;
  q.geom_global = tape->geom_global;
  q.dir_grid = tape->dir_grid;
  HIP_TRY(hipEventRecord(q.ev0, st));
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
  HIP_TRY(hipEventRecord(q.ev1, st));
  HIP_TRY(hipMemcpyAsync(q.h_cnt, tape->d_cnt, wos::kNumCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                         st));
  if (!dev_ptrs)
    HIP_TRY(hipMemcpyAsync(grad_source, d_out, (size_t)cells * C * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(q.done, st));
  HIP_TRY(hipEventRecord(c.done, st));
  c.last_stream = st;
  c.inflight = true;
  if ((flags & WOS_ASYNC) && dev_ptrs) {
    if (stats) {
      *stats = wos_stats{};
      stats->ticket = ticket;
    }
    return WOS_OK;
  }
  HIP_TRY(hipStreamSynchronize(st));
  c.inflight = false;
  if (stats) {
    int rc = fill_stats(q, stats);
    if (rc != WOS_OK) return rc;
  }
  return WOS_OK;
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
  {
    int rc = ctx_ready(c, s->device);
    if (rc != WOS_OK) return rc;
  }
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

  const uint64_t ticket = c.next_ticket++;
  StatSlot& q = c.slot[ticket % kStatSlots];
  while (q.bev.size() < 4) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    q.bev.push_back(e);
  }
  q.ticket = ticket;
  q.n_batches = 1;
  q.bpc_fb = 0;
  q.bpc_walk = 0;
  HIP_TRY(hipEventRecord(q.ev0, st));
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
  {
    int rc = walk_layout(s, &wp0, wl);
    if (rc != WOS_OK) return rc;
  }
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
    int rc = ensure_jump(c, std::max(4096, 4 * std::max(1, bp->n_walks_gradient)));
    if (rc != WOS_OK) return rc;
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
      int rc = ensure_tasks(c, 2, chunk * wpp, chunk);
      if (rc != WOS_OK) return rc;
    }
  }
  if (nn * bp->n_walks_solution > max_batch)
    return fail(WOS_E_CAPACITY, "wos_bvc: samples x nWalks exceed one task batch");
  side_tasks[1] = nn * bp->n_walks_solution;
  side_points[1] = nn;
  for (int k = 0; k < kSideWs; k++) {
    TaskWs& w = c.side[k];
    int rc = side_ready(w, bvc_priority(k == 0));
    if (rc == WOS_OK) rc = ensure_tasks_in(w.tasks, w.task_cap, w.pstate, w.pstate_cap, 2, side_tasks[k], side_points[k]);
    if (rc != WOS_OK) return rc;
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
      int rc = solve_locked(s, &gp, d_bpt + 2 * r.b0, r.b1 - r.b0, r.b0, 1, d_bsol + r.b0, d_dgrad, d_bnest + r.b0,
                            nullptr, &rs, c.bvc_dir, WOS_PTRS_DEVICE | WOS_ASYNC, ex);
      if (rc != WOS_OK) return rc;
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
    q.bpc_walk = bpc;
    return WOS_OK;
  };
  for (const Run& r : runs) {
    const int64_t m = r.b1 - r.b0;
    int rc = WOS_OK;
    if (!r.dir)
      rc = walks(0, d_bpt + 2 * r.b0, d_bnrm + 2 * r.b0, d_al + r.b0, d_bdd + r.b0, m, r.b0, bp->n_walks_solution, 1,
                 6u, d_bsol + r.b0, d_bnest + r.b0);
    else if (bp->use_finite_differences)
      rc = walks(0, d_bpt + 2 * r.b0, d_bnrm + 2 * r.b0, d_al + r.b0, d_bdd + r.b0, m, r.b0, bp->n_walks_gradient, 0,
                 8u, d_bsol + r.b0, d_bnest + r.b0);
    if (rc != WOS_OK) return rc;
    if (r.dir && bp->use_finite_differences)
      HIP_TRY(wos::launch_bvc_fd(s->dev, d_bpt + 2 * r.b0, d_bsol + r.b0, m, d_bdn + r.b0, c.side[0].stream));
  }
  {
    int rc = walks(1, d_npt, nullptr, nullptr, d_ndd, nn, 0, bp->n_walks_solution, 0, 7u, d_nsol, d_nnest);
    if (rc != WOS_OK) return rc;
  }
  q.walk_lds = (int32_t)wl.shmem_walk;
  q.star_grid = dsc.sgrid != nullptr;
  q.geom_global = dsc.geom_global;
  q.dir_grid = dsc.dgrid != nullptr;

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
  HIP_TRY(hipEventRecord(q.ev1, st));
  // the walk counters of both side workspaces (summed below); the Dirichlet solves' own
  // counters are in their stat slots
  std::vector<unsigned long long> cnt1(wos::kNumCounters);
  HIP_TRY(hipMemcpyAsync(q.h_cnt, c.side[0].counters, wos::kNumCounters * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, st));
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
    int rc = fill_stats(q, stats);
    if (rc != WOS_OK) return rc;
    stats->points_estimated = (uint64_t)nb;
    // the Dirichlet solves ran inside this call's span: their counters, not their times
    for (uint64_t t : dtickets) {
      const StatSlot& dq = c.slot[t % kStatSlots];
      if (dq.ticket != t) continue;
      wos_stats rs{};
      rc = fill_stats(dq, &rs);
      if (rc != WOS_OK) return rc;
      stats->walk_steps += rs.walk_steps; stats->wasted_steps += rs.wasted_steps;
      stats->walks_recorded += rs.walks_recorded; stats->walks_escaped += rs.walks_escaped;
      stats->walks_max_length += rs.walks_max_length; stats->walks_rr += rs.walks_rr;
      stats->walks_dirichlet += rs.walks_dirichlet; stats->rejection_iters += rs.rejection_iters;
    }
  }
  if (samples && nrec > 0) {
    if (samples_capacity < nrec)
      return fail(WOS_E_CAPACITY, "wos_bvc: samples buffer holds " + std::to_string(samples_capacity) + " of " +
                                      std::to_string(nrec) + " samples (counts[3])");
    std::memcpy(samples, recs.data(), recs.size() * sizeof(float));
  }
  return WOS_OK;
}

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

// No scene, no workspace, no lock: the call owns what it allocates.  Device pointers: the packed
// weights are a stream-ordered allocation, so WOS_ASYNC needs no host wait to free them.  Host
// pointers: one staging allocation, freed after the call's own synchronise.
int wos_siren_eval(const wos_siren_net* net, const float* pts, int64_t n, float* u, float* jac, float* div,
                   uint32_t flags, int32_t device, void* stream) {
  const std::string fn = "wos_siren_eval";
  if (!net) return fail(WOS_E_INVALID, fn + ": null net");
  if (int rc = siren_shape_check(fn, net->d_in, net->hidden)) return rc;
  if (net->d_out < 1 || net->d_out > 3)
    return fail(WOS_E_INVALID, fn + ": d_out must be 1..3, got " + std::to_string(net->d_out));
  if (net->n_hidden_layers < 0 || net->n_hidden_layers > wos::kSirenMaxHiddenLayers)
    return fail(WOS_E_INVALID, fn + ": n_hidden_layers must be 0.." + std::to_string(wos::kSirenMaxHiddenLayers) +
                                   ", got " + std::to_string(net->n_hidden_layers));
  if (!std::isfinite(net->omega)) return fail(WOS_E_INVALID, fn + ": omega must be finite");
  const int D = net->d_in, DO = net->d_out, H = net->hidden, L = net->n_hidden_layers, NL = L + 2;
  if (!net->weights || !net->biases) return fail(WOS_E_INVALID, fn + ": null weights or biases array");
  for (int l = 0; l < NL; l++)
    if (!net->weights[l] || !net->biases[l])
      return fail(WOS_E_INVALID, fn + ": null weights or biases pointer of layer " + std::to_string(l));
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

}  // extern "C"
