// wos_capi_scene.cpp -- the prepared-geometry cache, meshes, scenes and their source grids,
// geometry queries (include/wos.h; kernels in wos_query.hip, the source pack in wos_channels.hip).
#include "wos_capi.h"

namespace wos::capi {

Geom::~Geom() {
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

static std::mutex g_geom_mu;
// most recent first; heap-held and never destroyed (no hipFree during static teardown)
static std::vector<std::shared_ptr<Geom>>& g_geom_lru = *new std::vector<std::shared_ptr<Geom>>();
constexpr size_t kGeomCacheSize = 8;
static std::atomic<uint64_t> g_scene_serial{0};  // wos_scene::serial: what a walk tape knows its scene by

template <typename T>
static bool same(const std::vector<T>& a, const T* b, int n) {
  return a.size() == (size_t)n && (n == 0 || std::memcmp(a.data(), b, (size_t)n * sizeof(T)) == 0);
}

static bool geom_matches(const Geom& g, const wos_scene_desc* d, int device) {
  const int dim = d->dim;
  return g.device == device && g.dim == dim && g.double_sided == d->is_double_sided &&
         same(g.v, d->vertices, d->n_vertices * dim) && same(g.ix, d->prims, d->n_prims * dim) &&
         same(g.dv, d->dvertices, d->n_dvertices * dim) && same(g.dix, d->dprims, d->n_dprims * dim);
}

// the prepared geometry of `d` on `device`: from the cache, else prepared + uploaded
static int geom_get(const wos_scene_desc* d, int device, std::shared_ptr<Geom>& out) {
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
  {
    // FNV-1a over the key
    uint64_t h = 0xCBF29CE484222325ull;
    const auto mix = [&](const void* p, size_t bytes) {
      const unsigned char* b = (const unsigned char*)p;
      for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    };
    const int32_t head[2] = {dim, d->is_double_sided};
    mix(head, sizeof(head));
    mix(g->v.data(), g->v.size() * sizeof(float));
    mix(g->ix.data(), g->ix.size() * sizeof(int32_t));
    mix(g->dv.data(), g->dv.size() * sizeof(float));
    mix(g->dix.data(), g->dix.size() * sizeof(int32_t));
    g->content_id = h;
  }
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

void geom_cache_drop(int device) {
  std::lock_guard<std::mutex> lk(g_geom_mu);
  if (device < 0) {
    g_geom_lru.clear();
  } else {
    g_geom_lru.erase(std::remove_if(g_geom_lru.begin(), g_geom_lru.end(),
                                    [&](const std::shared_ptr<Geom>& g) { return g->device == device; }),
                     g_geom_lru.end());
  }
}

// LDS budget of the star-radius grid (staged by every walk-kernel workgroup)
constexpr size_t kStarGridBudget = 16 * 1024;

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

// what a set_source leaves in the scene: the grid's dims, n_channels source channels, and the scene's own
// Dirichlet constant for every channel but those dirichlet_values (or null) names
static void source_installed(wos_scene* s, const int32_t* dims, int n_channels, const float* dirichlet_values) {
  const int nsd = s->dev.dim == 2 ? 2 : 3;
  s->dev.source = s->d_source;
  for (int k = 0; k < 3; k++) s->dev.sdims[k] = k < nsd ? dims[k] : 1;
  s->dev.n_channels = n_channels;
  s->dev.g_dirichlet = s->g_dirichlet;
  for (int ch = 0; ch < wos::kMaxChannels; ch++)
    s->dev.g_ch[ch] = (dirichlet_values && ch < n_channels) ? dirichlet_values[ch] : s->g_dirichlet;
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

}  // namespace wos::capi

using namespace wos::capi;

extern "C" {

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
  WOS_TRY(geom_get(d, device, geom));
  auto* s = new wos_scene();
  s->device = device;
  s->geom = geom;
  s->serial = g_scene_serial.fetch_add(1) + 1;
  // the scene's own copies of the description's arrays (host or device); a failure leaves nothing behind
  const auto copy_in = [&](float** dst, const void* src, size_t count, int on_device) -> int {
    hipError_t e = hipMalloc((void**)dst, count * sizeof(float));
    if (e == hipSuccess)
      e = hipMemcpy(*dst, src, count * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e == hipSuccess) return WOS_OK;
    hipFree(s->d_nimg);
    hipFree(s->d_dimg);
    hipFree(s->d_source);
    delete s;
    return fail(WOS_E_DEVICE, std::string("wos_scene_create: ") + hipGetErrorString(e));
  };
  if (d->source) {
    WOS_TRY(copy_in(&s->d_source, d->source, nsrc, d->source_on_device));
    s->source_cap = nsrc;
  }
  if (ndimg) WOS_TRY(copy_in(&s->d_dimg, d->dirichlet_image, ndimg, d->dirichlet_image_on_device));
  if (nnimg) WOS_TRY(copy_in(&s->d_nimg, d->neumann_image, nnimg, d->neumann_image_on_device));
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
  source_installed(s, dims, 1, nullptr);  // back to one channel with the scene's own Dirichlet data
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
    WOS_TRY(wos_scene_set_source(s, source, dims, on_device, stream));
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
  source_installed(s, dims, n_channels, dirichlet_values);
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
