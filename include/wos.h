/*
 * wos.h -- C ABI of the MI355X walk-on-stars pressure-projection engine.
 *
 * This is the drop-in boundary for the one hot path of
 * Pranav-Jain/Neural-Monte-Carlo-Fluid-Simulation: the zombie / zombie3d WoSt
 * estimator behind the pybind11 module `zombie_bindings`
 * (bindings/zombie/demo/demo.cpp:393-401, bindings/zombie3d/demo/demo.cpp:119-125).
 * Plain pointers and sizes only; no torch / STL types cross this boundary.
 *
 * Every function returns WOS_OK (0) or a negative WOS_E* status; the message of
 * the last failure on the calling thread is available from wos_last_error()
 * (the reference aborts the interpreter instead: config.h:8-11, scene.h:106-109).
 */
#ifndef WOS_H
#define WOS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WOS_ABI_VERSION 10

enum {
    WOS_OK = 0,
    WOS_E_INVALID = -1,     /* bad argument / config value            */
    WOS_E_IO = -2,          /* file missing / unreadable               */
    WOS_E_DEVICE = -3,      /* HIP runtime error                       */
    WOS_E_CAPACITY = -4,    /* scene too large for the LDS-staged path */
    WOS_E_NOMEM = -5
};

/* flags for wos_solve */
#define WOS_PTRS_DEVICE 0x1u   /* pts/p/grad/n_est/steps are device pointers on the scene's device */
#define WOS_ASYNC       0x2u   /* with WOS_PTRS_DEVICE: enqueue on `stream` and return; only
                                  stats->ticket is filled (read the rest with wos_solve_stats) */
/* flag for wos_siren_fit, wos_siren_fit_run, wos_siren_fit_run_batches and the two _ensemble loops
 * (added within ABI 10; a library older than this flag ignores the bit and reads `scale` as
 * [rows][d_out], so a caller that sets it needs a library that knows it) */
#define WOS_FIT_SCALE_MATRIX 0x4u /* scale / pool_scale / every non-NULL entry of the ensemble arrays is a
                                     row-major d_out x d_out matrix per row: [rows][d_out][d_out] */

/* A boundary mesh: 2D line segments (dim=2) or 3D triangles (dim=3). */
typedef struct wos_mesh {
    int32_t dim;
    int32_t n_vertices;
    int32_t n_prims;
    float *vertices;          /* n_vertices * dim */
    int32_t *prims;           /* n_prims * dim (0-based vertex indices) */
} wos_mesh;

/* Replaces Scene::loadOBJ (bindings/zombie/demo/scene.h:104-145, 2D `v`/`l`
 * lines, flipOrientation swaps segment ends, normalizeDomain recentres) and
 * zombie::loadSurfaceMesh<3> (include/zombie/utils/fcpw_scene_loader.h:47-73).
 * Arrays are malloc'd; release with wos_mesh_free. */
int wos_load_obj(const char *path, int32_t dim, int32_t flip_orientation,
                 int32_t normalize, wos_mesh *out);
void wos_mesh_free(wos_mesh *mesh);

typedef struct wos_scene_desc {
    int32_t dim;                     /* 2 or 3 */
    const float *vertices;           /* Neumann boundary (the reference's OBJ "boundary") */
    const int32_t *prims;
    int32_t n_vertices, n_prims;
    const float *dvertices;          /* optional Dirichlet boundary (empty in the reference) */
    const int32_t *dprims;
    int32_t n_dvertices, n_dprims;
    float dirichlet_value;           /* constant g on the Dirichlet boundary */
    float absorption;                /* scene.absorptionCoeff (lambda) */
    int32_t is_watertight;           /* scene.isWatertight */
    int32_t is_double_sided;         /* scene.isDoubleSided */
    const float *source;             /* -div(u) grid: 2D [H][W] (rows ~ y); 3D [X][Y][Z] */
    int32_t source_dims[3];
    int32_t source_on_device;        /* source is a device pointer (copied d2d) */
    /* optional image-valued Dirichlet data (2D, ABI 8), replacing dirichlet_value: g at a walk's
       projection x onto the Dirichlet boundary is Image::get((x - x0) / ex, (y - y0) / ey)
       (setTerminalContribution walk_on_stars.h:331-351 -> projectToDirichlet
       fcpw_scene_loader.h:345-364 -> the upstream demo's pde.dirichlet, scene.h:202-207 commented
       in the fork: x0, y0 = bbox.pMin, ex = ey = bbox.extent().maxCoeff(); image.h:53-58) */
    const float *dirichlet_image;    /* [H][W] row-major, row ~ y; NULL: constant dirichlet_value */
    int32_t dirichlet_image_dims[2]; /* H, W */
    float dirichlet_image_box[4];    /* x0, y0, ex, ey: the rectangle the image covers */
    int32_t dirichlet_image_on_device;
    /* optional image-valued Neumann data h (2D, ABI 9): pde.neumann at a boundary sample y is
       Image::get((y - x0) / ex, (y - y0) / ey) (the upstream demo's pde.neumann, scene.h:175-181
       commented in the fork: uv = (x - bbox.pMin) / bbox.extent(); image.h:53-58).  It enters the
       walk's Neumann term throughput * alpha * G * h / pdf at every step (walk_on_stars.h:212-260)
       and a BVC Neumann sample's normal derivative (boundary_sampler.h:126-133).  NULL: h = 0,
       the reference's pde.neumann (scene.h:176-181, scene_3d.h:108-111) */
    const float *neumann_image;      /* [H][W] row-major, row ~ y */
    int32_t neumann_image_dims[2];   /* H, W */
    float neumann_image_box[4];      /* x0, y0, ex, ey */
    int32_t neumann_image_on_device;
} wos_scene_desc;

typedef struct wos_scene wos_scene;

/* Replaces Scene::Scene(json, mat) (scene.h:54-77) / Scene(json, mat3d)
 * (scene_3d.h:22-40): normals, silhouettes (fcpw.inl:224-353, sbvh.inl:313-436),
 * padded bbox, then uploads geometry + source to `device`. */
int wos_scene_create(const wos_scene_desc *desc, int32_t device, wos_scene **out);
int wos_scene_destroy(wos_scene *scene);

/* Replaces the source grid (-div u) of an existing scene.  The reference rebuilds
 * the whole scene every projection to change only this (model_split.py:185-191,
 * Scene(sceneConfig, div) -> scene.h:54-77 / scene_3d.h:22-40); here geometry
 * stays resident.  dims as wos_scene_desc.source_dims; `on_device`: `source` is
 * a device pointer on the scene's device.  The copy is ordered on `stream`
 * (hipStream_t, NULL = null stream) after any solve still running on another
 * stream. */
int wos_scene_set_source(wos_scene *scene, const float *source, const int32_t *dims,
                         int32_t on_device, void *stream);

/* Several source fields on one set of walks (added within ABI 10: new entry points only).  The
 * reference's estimator is generic in its value type (WalkOnStars<T, DIM>, PDE<T, DIM>,
 * walk_on_stars.h:32-50, pde.h:14-27); a walk itself never looks at the source, so up to
 * WOS_MAX_CHANNELS right-hand sides on one geometry -- the components of a vector-valued solve, the
 * members of an ensemble -- share every walk (common random numbers) for little more than the price
 * of one.  Contract: channel c of wos_solve_channels equals, bit for bit, wos_solve_var on the same
 * scene with source c and the constant Dirichlet value g_c.
 *   source            planar [C][H][W] (2D) or [C][X][Y][Z] (3D); dims as wos_scene_set_source
 *   dirichlet_values  host array of C constants g_c, or NULL: every channel uses the scene's
 *                     Dirichlet data.  Image-valued Dirichlet and Neumann data stay scalar and apply
 *                     to every channel; non-NULL dirichlet_values on a scene with a Dirichlet image
 *                     is WOS_E_INVALID
 *   n_channels        1..WOS_MAX_CHANNELS, else WOS_E_INVALID
 * The planar input is packed into one 16-byte texel per grid cell by a kernel on `stream`, ordered
 * like wos_scene_set_source's copy (one channel: that copy).  wos_scene_set_source returns the
 * scene to one channel and to its own Dirichlet data.  While a scene holds more than one channel,
 * wos_solve, wos_solve_var and wos_bvc return WOS_E_INVALID (they never solve channel 0 silently). */
#define WOS_MAX_CHANNELS 4
int wos_scene_set_source_channels(wos_scene *scene, const float *source, int32_t n_channels,
                                  const int32_t *dims, const float *dirichlet_values,
                                  int32_t on_device, void *stream);
int32_t wos_scene_channels(const wos_scene *scene);   /* source channels the scene holds (>= 1) */

/* Scenes share a per-device solve workspace and a cache of prepared geometries
 * (keyed by content), so the reference's per-step Scene(...) costs neither a
 * workspace allocation nor a re-preparation.  This releases both for `device`
 * (-1: every device); live scenes stay valid and the next solve reallocates. */
int wos_release_caches(int32_t device);

/* Walk tasks per batch (ABI 10).  A solve runs its points in batches of at most this many walk
 * tasks (the per-device workspace holds one batch: 60 B per task, plus 12 B for every source
 * channel beyond the first -- 60 + 12 (C - 1), wos_solve_channels); default 2^28 = 16 GB at most,
 * sized for a 288 GB MI355X (fewer batches, fewer ramp-downs of the persistent kernels).  A
 * caller that shares the GPU with other work can cap it.  max_tasks <= 0: the default; else
 * clamped to [2^16, 2^30].  Returns the previous value.  Results do not depend on it. */
int64_t wos_set_max_batch_tasks(int64_t max_tasks);

/* Length hints (additive, ABI 10).  A solve's walks do not depend on the source, so a time-stepper
 * that solves the same points on the same boundary every step repeats them step for step.  A plain
 * 2D one-channel solve that runs in one batch lists its walks of >= hint_min steps in the per-device
 * workspace; the next such solve with the same walks (same geometry content, absorption, point count
 * and coordinates, index_base / index_stride, seed and walk-relevant solver parameters; a fresh
 * wos_scene on the same geometry qualifies) starts those of >= express_min steps first, longest
 * first, express_per_wave to a wave that takes nothing else until they have ended, at issue priority
 * `priority` (0..3).  Scheduling only: results are bit-identical with and without, a stale or foreign
 * list is never used, and the first solve of a point set runs as it always did.  capacity: entries
 * of the list (at most 65536; walks beyond it are counted, not listed, and a list that overflowed
 * is not used at all: where that many walks are long they are the bulk, not the tail).  The express
 * list holds at most express_per_wave walks per workgroup of the walk kernel's grid, the longest.
 * Hinted are the plain solves (wos_solve, wos_solve_var) of 2D one-channel scenes whose Neumann term
 * is provably inert (watertight, single-sided, no Neumann image; not WOS_SCHED_FULL_NEUMANN); robust_float,
 * several channels, 3D, solves that split into batches, the tape and wos_bvc run as they always did.
 * A negative argument selects that value's default.  Takes effect with the next solve.  WOS_SCHED_NO_LENGTH_HINTS switches both the
 * listing and the use off for a solve; wos_release_caches drops the list.
 * wos_length_hint_stats: of the last solve on `device`, after waiting for it: out[0] express walks
 * started, out[1] walks the list had no room for, out[2] walks listed, out[3] entries of the express
 * list it ran with (all 0 if that solve ran without hints).
 * wos_selftest_hint_key: host only.  1 if two hint keys that differ in field `field` alone compare
 * unequal, 0 if they compare equal, -1 past the last field. */
void wos_set_length_hints(int32_t hint_min, int32_t express_min, int32_t express_per_wave, int32_t capacity,
                          int32_t priority);
int wos_length_hint_stats(int32_t device, int64_t *out);
int32_t wos_selftest_hint_key(int32_t field);

/* Express layout (additive, ABI 10): which wave starts which walk of the express list.  Scheduling
 * only, like the hints themselves.  solo_min: the express walks of >= solo_min steps get a wave
 * each (0: none do; at most 1023).  The walks below go express_per_wave to a wave: stripe 0 in
 * contiguous blocks of the list, which is sorted longest first, so a wave's walks are of nearly one
 * length; stripe 1 one walk of each length band, so the wave thins out as its short walks end.
 * placement 0: a workgroup's express wave is wave (workgroup index mod 4); 1: the first of its
 * waves on the lowest-numbered SIMD the workgroup occupies.  The express list holds at most as
 * many walks as one claim per workgroup of the walk kernel's grid covers: the solo tier is cut to
 * that first, then the list.  A negative argument selects that value's default; values are
 * clamped, never refused.  wos_get_express_layout: out[0..2] the three values in force.
 * wos_express_layout_stats: of the last solve on `device`, after waiting for it: out[0] the entries
 * of its solo tier, out[1] the claims its other express entries went to (both 0 if that solve ran
 * without hints); with wos_length_hint_stats' out[3] entries, out[1] = ceil((out[3] - out[0]) /
 * express_per_wave).
 * wos_selftest_express_slot: host only.  The layout's table for a list of nx entries, for every
 * solo tier n_solo in 0..nx: a row (n_solo, claim, j, entry) in out (4 words each, at most `rows`
 * of them written) for every claim in 0..nx+1 and j in 0..express_per_wave+1 that holds an entry;
 * returns the number of rows there are.
 * wos_selftest_simd_ids: of one 256-thread workgroup, out[w] the SIMD wave w ran on as the walk
 * kernel reads it, out[4 + w] the wave's whole hardware id register. */
void wos_set_express_layout(int32_t solo_min, int32_t stripe, int32_t placement);
void wos_get_express_layout(int32_t *out);
int wos_express_layout_stats(int32_t device, int64_t *out);
int64_t wos_selftest_express_slot(uint32_t nx, uint32_t express_per_wave, int32_t stripe, uint32_t *out, int64_t rows);
int wos_selftest_simd_ids(int32_t device, uint32_t *out);

typedef struct wos_scene_info {
    int32_t dim, n_prims, n_silhouettes, n_dprims, device;
    float bbox_min[3], bbox_max[3];
} wos_scene_info;
int wos_scene_get_info(const wos_scene *scene, wos_scene_info *info);

/* ---- Geometry queries: distance, side and solve state of points, on the device ----------
 * What a solve's point setup computes for every query point before it walks (added within
 * ABI 10: a new entry point only), for callers that need it outside a solve: the time-stepper's
 * obstacle SDF (the reference's obs_sdf_func, src/2d/models/base.py:239-241, 352-358, which for
 * a mesh goes through the host: obstacle_function, src/2d/sources.py:102-119) and an inside /
 * mask test that agrees with the solver's own.  For n points pts[n*dim], each output optional
 * (NULL), all four NULL being WOS_E_INVALID:
 *   dist[n]         distance to boundary `which` (WOS_QUERY_NEUMANN: the scene's boundary mesh;
 *                   WOS_QUERY_DIRICHLET: its optional Dirichlet mesh)
 *   signed_dist[n]  the solver's signed distance: +dist on the side the primitive's normal at
 *                   the closest point faces, -dist on the other -- negative on the domain side
 *   closest[n*dim]  the closest point on that boundary (the last primitive among exact ties)
 *   state[n]        bit 0 estimated, bit 1 p masked, bit 2 grad masked -- WOS_TAPE_PSTATE's bits,
 *                   what a solve with output.boundaryDistanceMask = boundary_distance_mask gives
 *                   the point -- and bit 3 insideDomain (fcpw_scene_loader.h:642-648).  It always
 *                   takes both boundaries as the solver does (without Dirichlet geometry the far
 *                   corner of the bounding box) and does not depend on `which`.
 * The values are the solve's own device functions': bit for bit what wos_solve decides.
 * WOS_E_INVALID: `which` out of range; dist, signed_dist or closest asked of a boundary the scene
 * does not hold (state alone needs none).  n == 0 succeeds without a launch.  Pointers are host
 * pointers (blocking; staged through temporaries of the call's own) or, with WOS_PTRS_DEVICE,
 * device pointers on the scene's device; WOS_ASYNC as in wos_solve: with WOS_PTRS_DEVICE it
 * enqueues on `stream` and returns, without it (host pointers) the flag is ignored and the call
 * blocks.  The call reads geometry only: it is ordered against nothing but `stream`, may run
 * beside solves on other streams, and leaves the solve workspace and the source alone.
 * Lifetime of an enqueued query: it reads the scene's prepared geometry, which outlives
 * wos_scene_destroy and wos_release_caches until the device has finished with it (it is released
 * only after a device synchronise), so destroying the scene behind a pending query is safe; pts
 * and the output buffers are the caller's and must stay valid until `stream` has run the query. */
enum { WOS_QUERY_NEUMANN = 0, WOS_QUERY_DIRICHLET = 1 };
int wos_scene_query(wos_scene *scene, int32_t which, float boundary_distance_mask,
                    const float *pts, int64_t n,
                    float *dist, float *signed_dist, float *closest /* [n][dim] */, int32_t *state,
                    void *stream, uint32_t flags);

/* Solver / output settings: the keys runWalkOnStars_sampled reads
 * (demo.cpp:121-137) plus output.boundaryDistanceMask (grid.h:159) and the
 * counter-based RNG key that replaces the clock seeds. */
typedef struct wos_solver_params {
    int32_t n_walks;                        /* nWalks (128) */
    int32_t max_walk_length;                /* maxWalkLength (1024) */
    int32_t steps_before_tikhonov;          /* setpsBeforeApplyingTikhonov (maxWalkLength) */
    int32_t steps_before_maximal_spheres;   /* setpsBeforeUsingMaximalSpheres (maxWalkLength) */
    float epsilon_shell;                    /* epsilonShell (1e-3) */
    float min_star_radius;                  /* minStarRadius (1e-3) */
    float silhouette_precision;             /* silhouettePrecision (1e-3) */
    float russian_roulette_threshold;       /* russianRouletteThreshold (0) */
    float boundary_distance_mask;           /* output.boundaryDistanceMask (0) */
    int32_t disable_gradient_control_variates;
    int32_t disable_gradient_antithetic_variates;
    int32_t use_cosine_sampling;            /* useCosineSamplingForDirectionalDerivatives */
    int32_t ignore_dirichlet;
    int32_t ignore_neumann;
    int32_t ignore_source;
    uint64_t seed;                          /* RNG key */
    int32_t robust_float;                   /* 0 (default): the reference's float Bessel members, which
                                               overflow to NaN for 2D Yukawa balls with mu R > ~92
                                               (distributions.h:585-587,695); 1: balls with mu R > 80 use
                                               exponentially scaled Bessels and ratios (finite, correct) --
                                               identical to mode 0 on every ball with mu R <= 80 */
    uint32_t schedule;                      /* WOS_SCHED_* bits: how the solve is scheduled on the GPU,
                                               never what it computes (results are bit-identical) */
} wos_solver_params;

/* wos_solver_params.schedule (no reference analogue; 0 = the engine's choice) */
#define WOS_SCHED_GEOM_GLOBAL   0x1u  /* read the geometry records through L2 even when they fit LDS */
#define WOS_SCHED_FULL_NEUMANN  0x2u  /* keep the walk kernel's Neumann term even when it is provably +0 */
#define WOS_SCHED_NO_STAR_GRID  0x4u  /* no star-radius cell grid: the cooperative group scan alone */
#define WOS_SCHED_NO_DIR_GRID   0x8u  /* no Dirichlet-distance cell grid (2D): the culled scans alone */
#define WOS_SCHED_NO_TAIL_SPREAD 0x10u /* no hand-over of walks to idle sibling waves once the queue is dry */
#define WOS_SCHED_NO_GRID_SPREAD 0x20u /* reserved, no effect: grid-wide hand-over was measured slower than the
                                          in-workgroup one and removed (the bit stays defined so callers still build) */
#define WOS_SCHED_NO_LENGTH_HINTS (0x40u) /* neither list this solve's long walks nor start known-long walks first
                                           (wos_set_length_hints) */

void wos_default_params(wos_solver_params *p);

typedef struct wos_stats {
    uint64_t walk_steps;        /* ball steps of recorded walks (first ball + walk() iterations) */
    uint64_t wasted_steps;      /* ball steps of dropped walks (escaped / over max length) */
    uint64_t walks_recorded;
    uint64_t walks_escaped;
    uint64_t walks_max_length;
    uint64_t walks_rr;
    uint64_t walks_dirichlet;
    uint64_t points_estimated;
    uint64_t rejection_iters;
    double kernel_ms;           /* device time of the whole solve: all batches, all kernels (HIP events) */
    double first_ball_ms;       /* of which: point setup + first balls (wos_first_ball_kernel) */
    double walk_ms;             /* of which: the walks (wos_walk_kernel) -- the dominant kernel */
    double fold_ms;             /* of which: statistics + masked outputs (wos_fold_kernel) */
    uint64_t walk_launches;     /* walk-kernel launches (one per batch of points) */
    int32_t first_ball_blocks_per_cu;  /* occupancy of the launches (256-thread workgroups per CU) */
    int32_t walk_blocks_per_cu;
    int32_t walk_lds_bytes;     /* dynamic LDS per walk-kernel workgroup */
    int32_t star_grid;          /* 1: the star-radius cell grid was used */
    int32_t geom_global;        /* 1: geometry read from global memory (too large for LDS) */
    int32_t dir_grid;                       /* the walk kernel used the Dirichlet-distance cell grid (2D) */
    uint64_t ticket;            /* id of this solve on its device (for wos_solve_stats) */
} wos_stats;

/* Replaces runWalkOnStars_sampled (demo.cpp:119-205) / runWalkOnStars_3d
 * (zombie3d/demo/demo.cpp:15-116) for n query points pts[n*dim]:
 *   p[n]          masked pressure    (grid.h:155-179)
 *   grad[n*dim]   masked gradient    (grid.h:207-237)
 *   n_est[n]      recorded walks per point (optional, may be NULL)
 *   steps[n]      ball steps per point incl. wasted (optional, may be NULL)
 * The RNG of point i is keyed by the global index index_base + i*index_stride,
 * so sharding the points across GPUs does not change any result.
 * `stream` is a hipStream_t (NULL = the device's null stream). */
int wos_solve(wos_scene *scene, const wos_solver_params *params,
              const float *pts, int64_t n, int64_t index_base, int64_t index_stride,
              float *p, float *grad, int32_t *n_est, int32_t *steps,
              wos_stats *stats, void *stream, uint32_t flags);

/* wos_solve with the estimator's error bars (added within ABI 10: a new entry point, no struct or
 * existing signature changes, so the version number stays): the reference keeps them on the same Welford
 * pass as the means (SampleStatistics::update, walk_on_stars.h:863-868) and so does the fold kernel.
 *   p_var[n]         getEstimatedSolutionVariance, solutionM2 / max(1, nSolutionEstimates - 1)
 *   grad_var[n*dim]  getEstimatedGradientVariance, gradientM2[k] / max(1, nGradientEstimates - 1)
 *                    (walk_on_stars.h:811-831; both counts are n_est here)
 * Each may be NULL.  They are the per-walk sample variances of the point's walk contributions, in
 * walk order, bit for bit the reference's float operations.  Masking rule: a variance is masked
 * exactly like its mean -- p_var[i] is 0 wherever the distance mask or the domain test zeroes p[i]
 * (grid.h:155-179), grad_var[i*dim+k] is 0 wherever grad[i*dim+k] is zeroed (grid.h:207-237), and
 * both are 0 for points that are not estimated (n_est 0).  With one recorded walk M2 is 0.
 * Pointers follow `flags` like p and grad (host, or WOS_PTRS_DEVICE with or without WOS_ASYNC).
 * wos_solve is this call with both NULL: the same kernels, results and timings as before. */
int wos_solve_var(wos_scene *scene, const wos_solver_params *params,
                  const float *pts, int64_t n, int64_t index_base, int64_t index_stride,
                  float *p, float *grad, float *p_var, float *grad_var, int32_t *n_est, int32_t *steps,
                  wos_stats *stats, void *stream, uint32_t flags);

/* wos_solve_var on a scene with n_channels source channels (wos_scene_set_source_channels; n_channels
 * must equal wos_scene_channels, else WOS_E_INVALID).  Outputs are channel-major:
 *   p[C][n], grad[C][n*dim], and the optional p_var[C][n], grad_var[C][n*dim];
 *   n_est[n], steps[n] are the walks' and therefore shared by the channels.
 * Masks, points that are not estimated and the variance masking rule apply to each channel as in
 * wos_solve_var; wos_stats counts the walks once.  Host pointers, WOS_PTRS_DEVICE and WOS_ASYNC
 * work as there, batches included.  With one channel this is wos_solve_var. */
int wos_solve_channels(wos_scene *scene, const wos_solver_params *params,
                       const float *pts, int64_t n, int64_t index_base, int64_t index_stride,
                       int32_t n_channels, float *p, float *grad, float *p_var, float *grad_var,
                       int32_t *n_est, int32_t *steps, wos_stats *stats, void *stream, uint32_t flags);

/* Boundary value caching: the reference's `bvc(scene, solver, output)`
 * (bindings/zombie/demo/demo.cpp:265-363, exported at :396), replaced here.
 * Solver keys as for wos_solve plus the BVC keys demo.cpp:269-290 reads. */
typedef struct wos_bvc_params {
    int32_t n_walks_solution;       /* nWalksForCachedSolutionEstimates (128) */
    int32_t n_walks_gradient;       /* nWalksForCachedGradientEstimates (640): Dirichlet samples only */
    int32_t boundary_cache_size;    /* boundaryCacheSize (1024) */
    int32_t domain_cache_size;      /* domainCacheSize (1024) */
    int32_t grid_res;               /* output.gridRes (required) */
    int32_t use_finite_differences; /* useFiniteDifferencesForBoundaryDerivatives (Dirichlet samples only) */
    float normal_offset;            /* normalOffsetForCachedDirichletSamples (5 epsilonShell) */
    float radius_clamp;             /* radiusClampForKernels (1e-3) */
    float kernel_regularization;    /* regularizationForKernels (0) */
    float grid_box[4];              /* evaluation grid x0, y0, ex, ey (ABI 8; extent 0: the scene's
                                       bounding box -- createEvaluationGrid(bbox.pMin, bbox.pMax),
                                       demo.cpp:311, grid.h:352-368) */
} wos_bvc_params;

void wos_default_bvc_params(wos_bvc_params *p);

/* runBoundaryValueCaching (demo.cpp:265-363) on a 2D scene, blocking, host buffers:
 *   solution[g*g], grad[g*g*2]  the evaluation grid (point (i, j) at index i*g + j,
 *                               x = i/g * extent + box min over grid_box, grid.h:352-368),
 *                               masked as saveEvaluationGrid does (grid.h:393-409);
 *   samples[k*8] (optional)     the cached samples [x y nx ny pdf value dn/dn kind], kind 0
 *                               Neumann boundary, 1 Neumann normal-aligned, 2 domain (value =
 *                               the source), 3 Dirichlet boundary, 4 Dirichlet normal-aligned
 *                               (the sample normalOffset inside the boundary, value = the
 *                               estimated solution, dn/dn its estimated normal derivative),
 *                               if samples_capacity holds them (else WOS_E_CAPACITY);
 *   counts[4] (optional)        boundary, normal-aligned, domain samples, total.
 * Boundary samples cover the Neumann and the Dirichlet segments (boundary_sampler.h:87-412);
 * evaluation points within normalOffset of the Dirichlet boundary take a pointwise
 * estimateSolution (splatter.h:160-196).  3D scenes return WOS_E_INVALID (zombie3d exports no
 * bvc).  The three walk sets (Dirichlet samples, Neumann samples, near-boundary points) run
 * on three streams at once; stats: kernel_ms the whole call, first_ball_ms the point
 * queries, walk_ms until the cache is complete, fold_ms the splat and the near-boundary
 * walks still running beside it. */
int wos_bvc(wos_scene *scene, const wos_solver_params *params, const wos_bvc_params *bvc,
            float *solution, float *grad, float *samples, int64_t samples_capacity, int64_t *counts,
            wos_stats *stats);

/* Statistics of an earlier solve on the scene's device, by stats->ticket: waits for
 * that solve to finish, then fills *stats.  A time-stepper can enqueue the projection
 * (WOS_ASYNC) and keep queueing device work behind it, as the reference's caller does
 * with its training loop after wost() (model_split.py:272-283).  The last 16 solves
 * per device are held; older tickets return WOS_E_INVALID.  No reference analogue. */
int wos_solve_stats(wos_scene *scene, uint64_t ticket, wos_stats *stats);

/* ---- Walk tape: a solve's walks recorded once, replayed for every new source ----------
 * A walk never looks at the source grid: radii, directions, source sample points, throughput,
 * roulette and the recorded / dropped decision follow from geometry, lambda and the key alone.
 * A tape keeps, for fixed (scene, params, pts, index_base, index_stride), everything about the
 * walks but the source values: per walk the first ball's Green's function norm and source cell,
 * one entry (cell, throughput, norm; 12 bytes) per step that samples inside the star, and the
 * finish (code, throughput, Dirichlet term, Neumann total).  wos_tape_solve then redoes only the
 * source products and sums for the scene's current source grid and runs the ordinary fold: bit
 * for bit what wos_solve_channels (one channel: wos_solve_var) would return now for the recorded
 * points, indices and parameters -- p, grad, p_var, grad_var, n_est and steps -- at the cost of
 * streaming the tape.  The noise is frozen exactly as a fixed `seed` freezes it: re-record with a
 * new key for fresh noise.  No reference analogue.
 *
 * wos_tape_record  blocking; pts host or WOS_PTRS_DEVICE (the only flag read).  Costs about two
 *                  solves: a plain walk pass sizes every walk's slots, the recording pass fills
 *                  them.  Batches follow wos_set_max_batch_tasks (one segment per batch; results
 *                  do not depend on it).  max_bytes <= 0: no cap; a tape that would be larger
 *                  returns WOS_E_CAPACITY and keeps nothing.  stats: the recorded walks' counters
 *                  and the recording's device time.  robust_float = 1 and parameters wos_solve
 *                  refuses are WOS_E_INVALID.  The scene may hold several channels: the tape does
 *                  not depend on their count.
 * wos_tape_solve   outputs, pointers, flags (WOS_ASYNC included), ticket and stream ordering as
 *                  wos_solve_channels; n_channels must equal wos_scene_channels(scene).  Reads the
 *                  scene's current source (ordered after a wos_scene_set_source* on another
 *                  stream).  WOS_E_INVALID: another scene than the recorded one (by a process-unique
 *                  serial, not the address), source dims other than the recorded ones (the tape
 *                  stores cell indices), n_channels mismatch.  stats: the walk counters are the
 *                  recorded ones; kernel_ms, walk_ms (the replay kernel) and fold_ms this call's.
 * wos_tape_destroy frees the tape (valid after wos_release_caches and after the scene is gone:
 *                  the tape shares the geometry and owns its device memory). */
typedef struct wos_tape wos_tape;
typedef struct wos_tape_info {
    int32_t dim, n_walks, source_dims[3], device;
    int64_t n_points, n_tasks, n_entries, max_entries_per_walk, bytes;
    int32_t replay_chunk_entries;   /* entries the replay kernel stages per wave and pass */
} wos_tape_info;
int wos_tape_record(wos_scene *scene, const wos_solver_params *params, const float *pts, int64_t n,
                    int64_t index_base, int64_t index_stride, int64_t max_bytes,
                    wos_tape **out, wos_stats *stats, void *stream, uint32_t flags);
int wos_tape_solve(wos_tape *tape, wos_scene *scene, int32_t n_channels,
                   float *p, float *grad, float *p_var, float *grad_var,
                   int32_t *n_est, int32_t *steps, wos_stats *stats, void *stream, uint32_t flags);
int wos_tape_get_info(const wos_tape *tape, wos_tape_info *info);
int wos_tape_destroy(wos_tape *tape);

/* ---- Walk tape adjoint: the gradient of a loss with respect to the source grid ------------
 * wos_tape_solve is an affine map from the source grid to (p, grad p).  wos_tape_vjp applies
 * its transpose: grad_source[c][cell] = sum_i grad_p[c][i] dp_i/df[cell]
 * + sum_ik grad_grad[c][i][k] dg_ik/df[cell], on the recorded walks, for every channel on its own
 * plane.  The map is affine, so the result depends neither on the scene's current source values
 * nor on the channels' Dirichlet constants.  Upstream values of outputs the forward masks, and of
 * points it does not estimate, are read as 0.  The sums are float atomics: two calls may differ in
 * the last bits (wos_tape_vjp_indexed below sums in a fixed order instead).  With ignoreSource
 * recorded the result is exactly 0.
 *
 * wos_tape_vjp   grad_p [C][n] and grad_grad [C][n][dim] as wos_tape_solve lays out p and grad;
 *                one of them may be NULL (zeros), both NULL is WOS_E_INVALID.  grad_source
 *                [C][cells], planar in the layout wos_scene_set_source_channels takes, is
 *                overwritten.  Scene, n_channels and source dims are checked as wos_tape_solve
 *                checks them; a tape recorded with a null source is WOS_E_INVALID.  Pointers,
 *                flags (WOS_PTRS_DEVICE, WOS_ASYNC), ticket and stream ordering as wos_tape_solve.
 *                stats: the recorded walks' counters; kernel_ms this call's, fold_ms the adjoint
 *                fold, walk_ms the scatter, walk_launches two per segment.
 * wos_tape_read  blocking diagnostic copy-out of `count` elements from `offset` of one array of
 *                one segment (one segment per recorded batch), so that the operator can be
 *                restated on the host.  Elements are 4 bytes: float, or uint32 (code, cnt, slot,
 *                cell0, cell) / int32 (pstate).  Per task [n_tasks of the segment]: code, cnt
 *                (entries | bit 31), cell0, gnorm, thr_end, term, tneu; slot [n_tasks + 1]; bdir,
 *                sdir [dim][n_tasks]; per entry slot [slot[n_tasks]]: cell, thr, nrm; per point:
 *                pstate (bit 0 estimated, bit 1 p masked, bit 2 grad masked).
 *                WOS_TAPE_SEGMENT_POINTS reads nothing from the device: dst receives one int64,
 *                the segment's point count (offset 0, count 1).  A segment, field, offset or
 *                count out of range is WOS_E_INVALID. */
typedef enum wos_tape_field {
    WOS_TAPE_CODE = 0, WOS_TAPE_CNT = 1, WOS_TAPE_SLOT = 2, WOS_TAPE_CELL0 = 3, WOS_TAPE_GNORM = 4,
    WOS_TAPE_THR_END = 5, WOS_TAPE_TERM = 6, WOS_TAPE_TNEU = 7, WOS_TAPE_BDIR = 8, WOS_TAPE_SDIR = 9,
    WOS_TAPE_E_CELL = 10, WOS_TAPE_E_THR = 11, WOS_TAPE_E_NRM = 12, WOS_TAPE_PSTATE = 13,
    WOS_TAPE_SEGMENT_POINTS = 14
} wos_tape_field;
int wos_tape_vjp(wos_tape *tape, wos_scene *scene, int32_t n_channels,
                 const float *grad_p, const float *grad_grad, float *grad_source,
                 wos_stats *stats, void *stream, uint32_t flags);
int wos_tape_read(const wos_tape *tape, int32_t segment, int32_t field, int64_t offset, int64_t count,
                  void *dst);

/* ---- Walk tape adjoint, indexed: the same gradient, bit for bit reproducible ---------------
 * The terms wos_tape_vjp adds per segment, in their canonical order: first the first-ball terms
 * (cell0[t], id = t | 0x80000000, w = gnorm[t]) of every recorded task t = 0 .. T - 1 with
 * cell0[t] < cells, then the entry terms (cell[e], id = t, w = fl(thr[e] nrm[e])) of every filled
 * slot e = 0 .. slot[T] - 1 with cell[e] < cells (filled: e in [slot[t], slot[t] + min(cnt[t]
 * without bit 31, slot[t + 1] - slot[t])) of a recorded task t).  The index of a segment is this
 * list stably sorted by cell: row offsets [cells + 1] and, per term, cell, id and w (12 bytes).
 * Bit 31 of id selects c_j instead of a_j.  The tape owns one index per segment; it is a pure
 * function of the tape.  wos_tape_vjp_indexed sums the terms of every cell in an order that
 * depends on the row offsets and on tile_terms alone -- not on n_channels, the stream or
 * timing -- without atomics, so two calls agree in every bit (csrc/wos_tape_index.hip states the
 * order).  Segments are added in segment order: a tape recorded in other batches has another
 * (equally fixed) order.
 *
 * wos_tape_index_build     blocking, idempotent (a second call returns WOS_OK and does nothing).
 *                          max_bytes <= 0: no cap; else the cap of the call's peak device
 *                          allocation, the index plus the sort's scratch: over it the call
 *                          returns WOS_E_CAPACITY, keeps nothing and leaves the tape as it was.
 *                          A tape recorded with a null source is WOS_E_INVALID, a grid of
 *                          0xFFFFFFFF cells or more too.  With ignoreSource recorded the index is
 *                          empty.  The index survives wos_release_caches; wos_tape_destroy frees
 *                          it.  wos_tape_get_info's bytes do not count it.
 * wos_tape_index_get_info  built 0 / 1; n_terms over all segments; max_terms_per_cell the longest
 *                          row of any segment; bytes the index's device memory; tile_terms the
 *                          tile constant of the sum (set whether built or not).
 * wos_tape_index_read      blocking diagnostic copy-out as wos_tape_read's: row [n_cells + 1]
 *                          uint32, cell and id [row[n_cells]] uint32, w float.  WOS_E_INVALID
 *                          before the build.
 * wos_tape_vjp_indexed     parameters, checks, pointers, flags, ticket and stats as wos_tape_vjp;
 *                          fold_ms the adjoint fold, walk_ms the sum kernels.  WOS_E_INVALID if the
 *                          index is not built. */
typedef enum wos_tape_index_field {
    WOS_TAPE_INDEX_ROW = 0, WOS_TAPE_INDEX_ID = 1, WOS_TAPE_INDEX_W = 2, WOS_TAPE_INDEX_CELL = 3
} wos_tape_index_field;
typedef struct wos_tape_index_info {
    int32_t built, n_segments;
    int64_t n_terms, n_cells, max_terms_per_cell, bytes;
    int32_t tile_terms;
} wos_tape_index_info;
int wos_tape_index_build(wos_tape *tape, int64_t max_bytes);
int wos_tape_index_get_info(const wos_tape *tape, wos_tape_index_info *info);
int wos_tape_index_read(const wos_tape *tape, int32_t segment, int32_t field, int64_t offset, int64_t count,
                        void *dst);
int wos_tape_vjp_indexed(wos_tape *tape, wos_scene *scene, int32_t n_channels,
                         const float *grad_p, const float *grad_grad, float *grad_source,
                         wos_stats *stats, void *stream, uint32_t flags);

/* Device self-test of the deterministic math used by the kernel (for the
 * GPU-vs-oracle parity tests): which = 0 exp, 1 log, 2 sin, 3 cos, 4 atan,
 * 5 sqrt, 6 bessi0, 7 bessi1, 8 bessk0, 9 bessk1 (double); 10 expf, 11 logf,
 * 12 sinf, 13 cosf, 14 cbrtf (float in, float out widened to double); 15 sqrtf,
 * 16 i0_fast, 17 k0_fast, 18-23 the fused double evaluator, 24/25 I0/K0 of the fused
 * float pair of the rejection fast path. */
int wos_selftest_math(int32_t which, const double *x, double *out, int64_t n, int32_t device);

/* Device self-tests of the first-ball kernel's stratified sampler (generateStratifiedSamples,
 * sampling.h:435-457), for the GPU-vs-oracle tests.  They run the kernel's own device
 * functions on the LDS layout the kernel gives a wave.
 *
 * wos_selftest_lhs: the 2 n_pairs (dim - 1) stratified samples of each of the n point indices
 * gidx (seed key `key`, the per-point stream of tag 0), out [n][2 n_pairs][dim - 1].  One wave
 * builds the samples of plan[0] consecutive indices, as the kernel builds a pack of points.
 * jump_lds = 1 stages the first min(draws, 512) jump constants in LDS as a solve does,
 * 0 stages none (every draw reads the global table).
 *
 * wos_selftest_lhs_permute: runs one shuffle implementation on `count` caller-supplied tables.
 * A table holds WOS_LHS_PACK_R1 ? 2 : 1 slots of values [nstrat][sd] and partners [sd][nstrat]
 * (partner[i][j] in [j, nstrat)); `slots` of them are shuffled (the rest must come back as
 * given), out like values.  An impl whose registers / scratch nstrat does not fit, sd outside
 * 1..2 (the packed forms: 2) or a partner out of range is WOS_E_INVALID.
 *
 * wos_selftest_lhs_plan (host only, no device): what the kernels' constants select for
 * n_pairs and dim -- out[0] points per wave, [1] 1 if one pass shuffles every slot and
 * dimension (the packed forms), [2] the shuffle (WOS_LHS_*), [3] passes of the pair loop,
 * [4] jump constants 0 all staged in LDS, 1 LDS then the global table, [5] LDS bytes per wave,
 * [6] the dynamic LDS budget in bytes (a solve needs 4 x [5] <= [6]), [7] point packs per
 * queue grab, [8] 64-stratum chunks of the register / LDS shuffle (0: serial); out holds 9. */
#define WOS_LHS_REG1 0     /* lhs_permute_reg, one 64-lane chunk (nstrat <= 64) */
#define WOS_LHS_REG2 1     /* lhs_permute_reg, two chunks (nstrat <= 128) */
#define WOS_LHS_LDS 2      /* lhs_permute, pointer jumping in LDS (nstrat <= 256) */
#define WOS_LHS_PACK_R1 3  /* lhs_permute_reg<2, 1, 4>: up to 2 slots x 2 dimensions at once */
#define WOS_LHS_PACK_R2 4  /* lhs_permute_reg<2, 2, 2>: 1 slot x 2 dimensions at once */
#define WOS_LHS_SERIAL 5   /* lane 0's loop (plan only) */
int wos_selftest_lhs(uint64_t key, const int64_t *gidx, int64_t n, int32_t n_pairs, int32_t dim,
                     int32_t jump_lds, float *out, int32_t device);
int wos_selftest_lhs_permute(int32_t impl, const int32_t *partner, const float *values, int32_t nstrat,
                             int32_t sd, int32_t slots, int32_t count, float *out, int32_t device);
int wos_selftest_lhs_plan(int32_t n_pairs, int32_t dim, int32_t *out);

/* Device self-test of the Yukawa rejection sampler's decision functions (rejectionSampleGreensFn,
 * distributions.h:362-383), for the GPU tests (added within ABI 10: a new entry point only;
 * csrc/wos_selftest.hip).  Item i is the ball of radius R[i] with absorption lambda[i] and the
 * radius draw r = x[i] R[i]; `dim` holds for the call.  The kernel builds the ball and the
 * sampler's per-ball constants as a solve does and calls the shipped functions.  The u draws a
 * stream can produce are u_k = k 2^-23, k = 0 .. 2^23 - 1; each test is a prefix or a suffix of
 * them, so its edge describes its decision at every draw.  edges[i][6], 2^23 meaning "none":
 *   [0] a   draws the certified float test accepts (a prefix; 2D: none decided once mu R >= 80)
 *   [1] r0  first draw the certified float test rejects (a suffix)
 *   [2] e   draws the exact test of the sequential loop accepts
 *   [3] e3  the same for the cooperative sampler's exact 3D test (2D: e)
 *   [4] q   first draw the per-ball certain reject takes (closed form and tabulated bound)
 *   [5] xr  first draw the radius-dependent certain reject takes (3D; 2D: none)
 * The shortcuts are sound iff a <= e <= min(r0, q, xr).  vals[i][3] = the ball's norm, the
 * sampler's bound and 1 / (norm bound) as the kernels form them.  flags[i] bit j is set when test j
 * is not false below its edge and true at it.  n = 0 succeeds; a null pointer, n < 0 or dim
 * outside 2..3 is WOS_E_INVALID. */
int wos_selftest_rejection(int32_t dim, const float *R, const float *lambda, const float *x, int64_t n,
                           int32_t *edges, float *vals, int32_t *flags, int32_t device);

/* Device self-test of the Green's-function members of the ball (Gfn, csrc/wos_device.h;
 * distributions.h:273-832) and of the splat's 2D free-space functions (FreeSpace2, csrc/wos_bvc.hip;
 * distributions.h:85-119, 168-219), for the GPU tests (added within ABI 10: a new entry point only;
 * kernels in csrc/wos_selftest.hip and csrc/wos_bvc.hip).  One lane per item builds the ball as a
 * solve does (init, update_ball), sets r, yVol = c + r dir and ySurf = c + R dir as sample_volume
 * and the surface sample set them, and calls every member as shipped.  mode: WOS_GFN_HARMONIC,
 * WOS_GFN_YUKAWA (reference semantics) or WOS_GFN_ROBUST (the robust kernels' instantiation with
 * `robust` set: scaled members above mu R = 80).  items[n][WOS_GFN_ITEM]:
 *   [0] R  [1] lambda  [2] r  [3..5] c  [6..8] dir (unit)  [9..11] x  [12..14] y
 *   [15..16] n (2D unit normal of the free-space functions)  [17] the splat's radius clamp
 * out[n][WOS_GFN_OUT], slots that do not apply 0:
 *   [0..3] A0 A1 B0 B1 after update_ball (2D K0 I0 K1 I1, 3D exp sinh K32 I32 at mu R; the scaled
 *          ke0 ie0 ke1 ie1 in 2D scaled balls, none in 3D scaled balls)  [4] mu R
 *   [5] the ball's tag (0 harmonic, 1 Yukawa, 2 Yukawa with scaled members)
 *   [6] evaluate  [7] gradient_norm  [8] poisson_kernel  [9] norm  [10..12] poisson_kernel_gradient
 *   [13] dir_sampled_poisson_kernel(yVol)  [14] evaluate_xy(x, y)
 *   [15] evaluate_k0i0  [16] gradient_norm_k1i1, both from one bessel_ik<true, true> at mu r as the
 *          first-ball kernel feeds them (2D, tag 1)
 *   [17..21] A0 A1 B0 B1 mu R after set_ball on the four values the point-setup kernel stores
 *          (2D, tag 1)
 *   [22] pdf_sphere_uniform(r)  [23..25] gradient
 *   [26] free-space G(x, y)  [27..28] grad G  [29] P  [30..31] grad P at r = max(clamp, |y - x|),
 *          harmonic in mode 0 and Yukawa otherwise (2D)
 * n = 0 succeeds without a launch.  A null pointer, n < 0, dim outside 2..3 or an unknown mode is
 * WOS_E_INVALID. */
enum { WOS_GFN_HARMONIC = 0, WOS_GFN_YUKAWA = 1, WOS_GFN_ROBUST = 2 };
#define WOS_GFN_ITEM 20
#define WOS_GFN_OUT 32
int wos_selftest_gfn(int32_t dim, int32_t mode, const float *items, int64_t n, float *out, int32_t device);

/* Device self-test of the three geometry queries of a walk step -- the first ray hit, the star
 * radius and the distance to the Dirichlet boundary -- for the GPU tests (added within ABI 10: a new
 * entry point only; csrc/wos_selftest.hip).  The scene is planned exactly as wos_solve plans it under
 * `schedule`, min_star_radius and silhouette_precision (LDS or global geometry, star grid, Dirichlet
 * grid, the three hierarchies), workgroups of four waves stage the geometry as the walk kernel does,
 * and wave w takes the 64-bit lane mask masks[w]: its set lanes take the next items in order, and
 * every lane calls the wave-cooperative query with active / query / want false on clear lanes, as
 * the walk step calls it.  The set bits of all n_masks masks must sum to n.
 *   kind                 items[n][.]
 *   WOS_GEO_RAY          origin[dim], direction[dim], tmax
 *   WOS_GEO_STAR         x[dim], maxR, flip (0 or 1: computeStarRadius's flipNormalOrientation)
 *   WOS_GEO_DIRICHLET    x[dim]
 * out[n][3][WOS_GEO_OUT]: form 0 the plain sequential scan with no cull, form 1 the per-lane culled
 * form (ray_hit, star_radius, dirichlet_dist_culled), form 2 the wave-cooperative form as shipped
 * (ray_hit_wave, star_radius_wave, dirichlet_dist_step).  Ray: [0] 1.0 if hit, and where hit [1] d,
 * [2..] p, [5..] unit normal (zeros otherwise).  Star: [0] the radius.  Dirichlet: [0] the distance,
 * [1..] projectToDirichlet's point (forms 0 and 1; form 2 computes none).
 * tags[n]: the regime form 2 took for the item's wave (WOS_GEO_RAY_*, WOS_GEO_STAR_*, WOS_GEO_DIR_*).
 * sound[n]: bit WOS_GEO_S_* is set when that shortcut said "certainly reject" where the exact test
 * accepts, over every primitive, candidate and group of the scene for the item (each judged against
 * tmax / maxR alone); all zero means every shortcut kept its promise.  counts[n][WOS_GEO_COUNTS]:
 * how often each shortcut fired (slot WOS_GEO_C_x) and declined (slot WOS_GEO_C_x + 1), how often
 * silhouette_class2 returned 0, 1, 2 (WOS_GEO_C_CLASS + 0..2), and the length of the item's cell list.
 * plan[8] (may be NULL): geom_global, star grid present, Dirichlet grid present, dynamic LDS bytes,
 * the levels of the primitive, silhouette and Dirichlet group hierarchies, silhouette candidates.
 * n = 0 succeeds without a launch.  A null argument, an unknown kind, a Dirichlet query on a scene
 * without Dirichlet geometry or masks whose set bits do not sum to n are WOS_E_INVALID. */
enum { WOS_GEO_RAY = 0, WOS_GEO_STAR = 1, WOS_GEO_DIRICHLET = 2 };
#define WOS_GEO_OUT 8
#define WOS_GEO_COUNTS 16
enum { WOS_GEO_RAY_NONE = 0,   /* no lane of the wave queries */
       WOS_GEO_RAY_LANE_SCAN,  /* few primitives, two or more lanes: each lane scans them all */
       WOS_GEO_RAY_SOLO,       /* one querying lane: groups and primitives over the lanes, DPP minima */
       WOS_GEO_RAY_LIST,       /* the cooperative LDS list over the flat group scan */
       WOS_GEO_RAY_TREE };     /* the same list over the primitive-group hierarchy */
enum { WOS_GEO_STAR_NONE = 0,    /* decided without a scan (minR > maxR, minR >= maxR, no primitives) */
       WOS_GEO_STAR_SOLO_CELL,   /* one querying lane inside the star grid */
       WOS_GEO_STAR_CELL_LISTS,  /* the windowed cell lists */
       WOS_GEO_STAR_GROUPS,      /* the flat silhouette-group scan */
       WOS_GEO_STAR_TREE,        /* the scan over the silhouette-group hierarchy */
       WOS_GEO_STAR_MIXED = 0x100 }; /* or-ed in: the wave mixes lanes inside and outside the grid */
enum { WOS_GEO_DIR_NONE = 0, WOS_GEO_DIR_GRID, /* the Dirichlet cell grid */
       WOS_GEO_DIR_GRID_MISS,                  /* outside the grid: the culled scan */
       WOS_GEO_DIR_SOLO, WOS_GEO_DIR_CULLED,   /* one wanting lane; the culled flat scan */
       WOS_GEO_DIR_TREE };                     /* the culled scan over the Dirichlet-group hierarchy */
#define WOS_GEO_S_RAY_BOX 0x1u        /* ray_box_maybe (a group or a hierarchy node above it) */
#define WOS_GEO_S_RAY_PREFILTER 0x2u  /* ray_prim_prefilter against ray_prim_exact */
#define WOS_GEO_S_BALL_BOX 0x4u       /* ball_box_maybe over a group holding an accepted candidate */
#define WOS_GEO_S_CONE 0x8u           /* cone_culled over such a group */
#define WOS_GEO_S_CLASS2 0x10u        /* silhouette_class2's 0 / 1 against is_silhouette */
#define WOS_GEO_S_STAR_EARLY 0x20u    /* star_candidate's distance early-outs against d^2 <= r2 */
#define WOS_GEO_S_STAR_CELL 0x40u     /* the star grid's cell list lacks the exact scan's winner */
#define WOS_GEO_S_DIR_BOX 0x80u       /* a Dirichlet box bound above a member's computed d^2 */
#define WOS_GEO_S_DIR_CELL 0x100u     /* the Dirichlet grid's cell list lacks the winning segment */
enum { WOS_GEO_C_RAY_BOX = 0, WOS_GEO_C_PREFILTER = 2, WOS_GEO_C_BALL_BOX = 4, WOS_GEO_C_CONE = 6,
       WOS_GEO_C_STAR_EARLY = 8, WOS_GEO_C_DIR_BOX = 10, WOS_GEO_C_CLASS = 12, WOS_GEO_C_CELL_LEN = 15 };
int wos_selftest_geometry(wos_scene *s, uint32_t schedule, float min_star_radius, float silhouette_precision,
                          int32_t kind, const float *items, int64_t n, const uint64_t *masks, int32_t n_masks,
                          float *out, int32_t *tags, uint32_t *sound, uint32_t *counts, int32_t *plan);

/* Device self-test of the source sample of a walk step and of a first ball -- sample_volume_wave,
 * the wave-cooperative rejection sampler, beside the sequential loop sample_volume it promises to
 * reproduce -- for the GPU tests (added within ABI 10: a new entry point only; csrc/wos_selftest.hip).
 * Workgroups of four waves stage the context's PCG32 jump table and the bound table as every kernel
 * that samples stages them and give each wave its own LDS scratch; wave w takes the 64-bit lane mask
 * masks[w], its set lanes take the next items in order, and every lane calls sample_volume_wave with
 * `active` false on clear lanes, as the walk step and the first balls call it.  Clear lanes hold a
 * ball and a stream that would sample if `active` were not honoured.
 *   dim      2 or 3
 *   variant  WOS_SV_FB: the first-ball kernel's instantiation (its block sizes and own generation)
 *            WOS_SV_RB: the robust kernels' Gfn with `robust` set (scaled balls above mu R = 80)
 *   need_pdf 0 or 1, as the caller passes it (the walk step 0, the first balls 1)
 *   items[n][WOS_SV_ITEM]  [0] R  [1] lambda  [2] yukawa (0 or 1)  [3..5] c  [6..8] dir (unit)
 *   seeds[n]  the 32-bit stream seed; the stream is seeded as the walk seeds its own (Pcg32::seed)
 * The ball is built as a solve builds it (init, update_ball).  Per item, two results: form 0 the
 * cooperative form as shipped, form 1 the sequential sample_volume from a copy of the same ball and
 * stream.  out[n][2][WOS_SV_OUT]: [0] g.r after the clamps  [1] pdf  [2..4] out.  state[n][2]: the
 * stream state after the call.  iters[n][2]: the iterations the call added.
 * tags[n]: the regime the cooperative form took for the item (WOS_SV_*), restated from the same
 * wave-uniform values, with WOS_SV_PUBLISHED or-ed in when the lane wrote its stream to the wave's
 * scratch -- which the function does on entering a cooperative generation and nowhere else, so the
 * bit is set on sparse lanes and on dense lanes that continued, and clear on the others.
 * canary[n_masks][64], one word per lane: on a clear lane the bits WOS_SV_CANARY_* of what the call
 * changed of that lane's ball, stream, pdf, out or iteration count; on a set lane WOS_SV_CANARY_PDF
 * when need_pdf is 0 and pdf was written all the same.
 * plan[8] (may be NULL): the wave size, the minimum and maximum iterations per lane and generation,
 * the iterations of the own generation (0: none), the sampling lanes it needs, the iterations whose
 * jump constants are staged in LDS, the iteration limit and the workgroup size, for `dim` and variant.
 * n = 0 succeeds without a launch.  A null pointer, n < 0, dim outside 2..3, an unknown variant bit
 * or more set mask bits than items are WOS_E_INVALID. */
#define WOS_SV_FB 0x1u
#define WOS_SV_RB 0x2u
#define WOS_SV_ITEM 9
#define WOS_SV_OUT 5
enum { WOS_SV_FALLBACK = 0,  /* off the fast path: the sequential loop (harmonic, 2D mu R >= 80, 3D scaled) */
       WOS_SV_SOLO,          /* the wave's one sampling lane */
       WOS_SV_SPARSE,        /* cooperative generations from iteration 0 */
       WOS_SV_DENSE_OWN,     /* dense wave, accepted inside the own generation */
       WOS_SV_DENSE_COOP,    /* dense wave, continued cooperatively after it */
       WOS_SV_PUBLISHED = 0x100 }; /* or-ed in: the lane published its stream for a cooperative generation */
#define WOS_SV_CANARY_BALL 0x1u
#define WOS_SV_CANARY_STREAM 0x2u
#define WOS_SV_CANARY_PDF 0x4u
#define WOS_SV_CANARY_OUT 0x8u
#define WOS_SV_CANARY_ITERS 0x10u
int wos_selftest_sample_volume(int32_t dim, uint32_t variant, int32_t need_pdf, const float *items,
                               const uint32_t *seeds, int64_t n, const uint64_t *masks, int32_t n_masks,
                               float *out, uint64_t *state, uint32_t *iters, int32_t *tags, uint32_t *canary,
                               int32_t *plan, int32_t device);

/* Device self-test of the indexed adjoint's sum kernels (csrc/wos_tape_index.hip) on a
 * caller-supplied index, without a scene: row [n_rows + 1] (row[0] = 0, non-decreasing), id and
 * w [row[n_rows]] (id & 0x7FFFFFFF < n_tasks; bit 31: take c), a and c [n_channels][n_tasks],
 * n_channels 1 .. 4.  out [n_channels][n_rows] = the per-row sums, from zero;
 * *tile_terms (may be NULL) = the tile constant.  Anything else is WOS_E_INVALID. */
int wos_selftest_tape_rowsum(const uint32_t *row, int64_t n_rows, const uint32_t *id, const float *w,
                             const float *a, const float *c, int64_t n_tasks, int32_t n_channels,
                             float *out, int32_t *tile_terms, int32_t device);

/* ---- Fused SIREN: value, input Jacobian and divergence of the velocity network ---------------
 * The reference's MLP with sine (src/2d/models/networks.py:25-68): Linear(d_in, hidden),
 * sin(omega .), n_hidden_layers x [Linear(hidden, hidden), sin(omega .)], Linear(hidden, d_out),
 * every layer with bias -- evaluated in forward mode in one kernel (added within ABI 10: new entry
 * points only; csrc/wos_siren.hip).  It replaces the autograd divergence behind get_divergence
 * (model_split.py:230-236, diff_ops.py:45-51): no activation leaves the chip.  For n points
 * pts[n*d_in], each output optional (NULL), all three NULL being WOS_E_INVALID:
 *   u[n*d_out]         the network's value
 *   jac[n*d_out*d_in]  jac[(p*d_out + i)*d_in + k] = d u_i / d x_k
 *   div[n]             (jac[0][0] + jac[1][1]) + jac[2][2], added in f32 in that order; needs
 *                      d_out == d_in
 * Envelope: d_in 2 or 3, d_out 1..3, hidden a multiple of 32 in 32..256, n_hidden_layers 0..8,
 * omega finite; anything else is WOS_E_INVALID with a message naming the field.  weights and biases
 * are host arrays of n_hidden_layers + 2 pointers, torch's layout: weights[l] [out][in] row-major.
 * All arithmetic is f32 in a fixed order (DESIGN.md "Fused SIREN source"): a point's outputs are the
 * same bits whatever n is, wherever the point sits in pts, whichever outputs are requested and from
 * run to run.  Pointer rules are wos_scene_query's: pts, u, jac, div and every weights[l] / biases[l]
 * are host pointers (the call stages them and blocks) or, with WOS_PTRS_DEVICE, device pointers on
 * `device`; with WOS_PTRS_DEVICE | WOS_ASYNC the call enqueues on `stream` and returns, and the
 * buffers must stay valid until `stream` has run it.  n == 0 succeeds without a launch. */
typedef struct wos_siren_net {
    int32_t d_in, d_out, hidden, n_hidden_layers;
    float omega;
    const float *const *weights;   /* n_hidden_layers + 2 pointers */
    const float *const *biases;    /* n_hidden_layers + 2 pointers */
} wos_siren_net;
int wos_siren_eval(const wos_siren_net *net, const float *pts, int64_t n,
                   float *u, float *jac, float *div,
                   uint32_t flags, int32_t device, void *stream);

/* Device self-test of wos_siren_eval's hidden-layer product (the kernel's own device function on
 * its own LDS layout), host pointers, blocking: for n_points points carrying 1 + d_in columns of
 * `hidden` floats, X [n_points][1 + d_in][hidden], the pre-activations Z of the same shape:
 * Z[p][0] = W X[p][0] + b and Z[p][s] = W X[p][s] for s > 0, W [hidden][hidden] row-major.
 * hidden and d_in as wos_siren_eval; n_points >= 1. */
int wos_selftest_siren_layer(int32_t hidden, int32_t d_in, int64_t n_points, const float *W, const float *b,
                             const float *X, float *Z, int32_t device);

/* ---- Fused SIREN backward: gradients of (u, jac, div) with respect to the weights -------------
 * The vector-Jacobian product of wos_siren_eval's three outputs with the cotangents g_u[n*d_out],
 * g_jac[n*d_out*d_in] and g_div[n] (each may be NULL and counts as zero; all three NULL is
 * WOS_E_INVALID, as is g_div with d_out != d_in), summed over the n points (added within ABI 10:
 * new entry points only; csrc/wos_siren_vjp.hip, DESIGN.md "Fused SIREN backward"):
 *   grad_weights[l], grad_biases[l]   l = 0 .. n_hidden_layers + 1, the shapes of net's weights[l]
 *                                     and biases[l]; written, not accumulated
 * i.e. the gradient of  sum_p (g_u . u + g_jac . jac + g_div div)  with the seeds
 * Jb[i][k] = g_jac[i][k] + g_div [i == k].  There is no gradient with respect to the points or omega.
 * The forward is recomputed by wos_siren_eval's own code (the same pre-activation bits, OCML
 * sincosf); all arithmetic is f32.  The points are walked in chunks of whole 32-point tiles; per
 * chunk the layers' columns are stashed in a temporary of at most workspace_bytes (0: 256 MiB),
 * (2 n_hidden_layers + 1) * hidden * (1 + d_in) * 4 bytes per point; a non-zero workspace_bytes
 * that cannot hold one tile is WOS_E_CAPACITY.  The per-slice and per-tile partial sums come on top
 * (up to about a quarter of the stash).  Sums run in a fixed order without atomics: the same call with the same
 * n and workspace_bytes returns the same bits; different n or workspace_bytes may differ in the last
 * bits.  Envelope and pointer rules are wos_siren_eval's: host pointers (staged, blocking),
 * WOS_PTRS_DEVICE, or WOS_PTRS_DEVICE | WOS_ASYNC on `stream`; grad_weights and grad_biases are
 * host arrays of pointers like net's.  n == 0 writes zeros; n < 0 or a NULL gradient pointer is
 * WOS_E_INVALID. */
int wos_siren_vjp(const wos_siren_net *net, const float *pts, int64_t n,
                  const float *g_u, const float *g_jac, const float *g_div,
                  float *const *grad_weights, float *const *grad_biases,
                  size_t workspace_bytes,
                  uint32_t flags, int32_t device, void *stream);

/* Device self-test of wos_siren_vjp's two hidden-layer products, host pointers, blocking; dZ, X and
 * dX are [n_points][1 + d_in][hidden], W and dW [hidden][hidden] row-major:
 *   dX[p][s] = W^T dZ[p][s]             the transposed fragment-ordered copy of W through the
 *                                       forward's own product
 *   dW = sum over p, s of dZ[p][s] X[p][s]^T   the weight-gradient kernel with its split-K
 *                                       reduction; the padding columns of the last tile hold ones
 *                                       and must not count
 * hidden and d_in as wos_siren_eval; n_points 1 .. 65536. */
int wos_selftest_siren_vjp_layer(int32_t hidden, int32_t d_in, int64_t n_points,
                                 const float *W, const float *dZ, const float *X,
                                 float *dX, float *dW, int32_t device);

/* ---- Fused SIREN fit step: regression loss of the value and its weight gradients --------------
 * One iteration of the time-stepper's velocity fits (_advect_velocity, _project_velocity:
 * src/2d/models/model_split.py:88-120, 274-283) without its optimiser step (added within ABI 10: a
 * new entry point only; csrc/wos_siren_fit.hip, DESIGN.md "Fused SIREN fit step"):
 *   loss[0] = 1 / (n d_out) * sum_p sum_i (scale[p][i] u_i(x_p) - target[p][i])^2
 *   grad_weights[l], grad_biases[l]   its gradient, l = 0 .. n_hidden_layers + 1, the shapes of net's
 *                                     weights[l] and biases[l]; written, not accumulated
 * target[n*d_out]; scale[n*d_out] or NULL (= 1): a wrap u = s(x) * N(x) + c(x) that is diagonal-affine
 * in the network's output is scale = s with c folded into the target.  grad_weights and grad_biases
 * both NULL: the loss alone, with no backward sweep and no stash, the same bits as the full call's
 * loss.  Exactly one of them NULL, a NULL entry in either, a NULL loss or target and n <= 0 (a mean
 * over nothing) are WOS_E_INVALID.  u is wos_siren_eval's value chain (the same bits); all arithmetic
 * is f32: r = fma(scale, u, -target), the seed d loss / d u = (scale (r + r)) (1 / (n d_out)), the sum
 * of r r in a fixed blocked order divided once by n d_out.  The points are walked in chunks of whole
 * 32-point tiles; per chunk the layers' pre-activations are stashed in a temporary of at most
 * workspace_bytes (0: 256 MiB), (2 n_hidden_layers + 1) * hidden * 4 bytes per point; a non-zero
 * workspace_bytes that cannot hold one tile is WOS_E_CAPACITY.  No atomics: the same call with the
 * same n and workspace_bytes returns the same bits in loss and in every gradient.  Envelope and
 * pointer rules are wos_siren_vjp's: host pointers (staged, blocking), WOS_PTRS_DEVICE, or
 * WOS_PTRS_DEVICE | WOS_ASYNC on `stream`; loss is a pointer of the same kind as pts.  There is no
 * gradient with respect to the points, scale, target or omega.
 * WOS_FIT_SCALE_MATRIX: scale is S[n*d_out*d_out], a row-major matrix per point, for a wrap
 * u = S(x) N(x) + c(x) that mixes the network's components (a free-slip wall, u = (I - (1 - w) n n^T) N):
 *   loss[0] = 1 / (n d_out) * sum_p sum_i ((S[p] u(x_p))_i - target[p][i])^2
 * with r_i = -target_i, then r_i = fma(S[i][m], u_m, r_i) for m = 0 .. d_out - 1 in order, and the seed
 * d loss / d u_m = acc (1 / (n d_out)), g_i = r_i + r_i, acc = S[0][m] g_0 (a rounded product), then
 * acc = fma(S[i][m], g_i, acc) for i = 1 .. d_out - 1; everything else as above.  A matrix whose
 * off-diagonal entries are exact zeros gives, for finite u, the values of the call without the flag on
 * its diagonal (only the sign of an exact zero may differ).  The flag with a NULL scale is
 * WOS_E_INVALID, naming scale.  Without the flag nothing changes. */
int wos_siren_fit(const wos_siren_net *net, const float *pts, int64_t n,
                  const float *target, const float *scale, float *loss,
                  float *const *grad_weights, float *const *grad_biases,
                  size_t workspace_bytes,
                  uint32_t flags, int32_t device, void *stream);

/* ---- Fused Adam step: clip_grad_norm_ and torch.optim.Adam.step() in one call -----------------
 * The optimiser of the velocity fits (update_network, src/2d/models/base.py:130-152), for any list
 * of float tensors (added within ABI 10: new entry points only; csrc/wos_siren_train.hip, DESIGN.md
 * "Fused Adam step and the device-resident fit loop").  n_tensors is 1..20; counts, params and grads
 * are host arrays of n_tensors entries; exp_avg and exp_avg_sq are single flat buffers of sum(counts)
 * floats in the order of params; step >= 1 is the step being taken.  Torch's single-tensor Adam with
 * amsgrad, weight decay and maximize off, f32 with one operation per rounding; from the double
 * parameters the host computes, each rounded to float once, b2 = beta2, omb1 = 1 - beta1,
 * omb2 = 1 - beta2, bc2 = sqrt(1 - beta2^step), ss = lr / (1 - beta1^step); per element
 *   g' = g * c                        (only when clipping)
 *   m' = m + omb1 * (g' - m)
 *   v' = v * b2 + (omb2 * g') * g'
 *   p' = p - ss * (m' / (sqrtf(v') / bc2 + eps))
 * max_grad_norm > 0 clips: norm = sqrtf(sum g^2), one workgroup of 256 threads summing in a fixed
 * order over the flat order of the tensors, c = min(max_grad_norm / (norm + 1e-6f), 1); grad_norm
 * (may be NULL) then receives the unclipped norm.  max_grad_norm <= 0: no norm is computed, grad_norm
 * is not written.  grads are read, never written (torch's clip scales them in place; this does not).
 * No atomics: the same call gives the same bits.  Subnormal inputs and intermediates are kept (IEEE
 * gradual underflow, nothing is flushed to zero).
 * Non-finite gradients behave as clip_grad_norm_ (error_if_nonfinite off) followed by Adam.step() do;
 * nothing is detected or refused.  c is torch.clamp(max = 1) of the quotient, which keeps a NaN: when
 * clipping, one NaN gradient makes the norm, c, and so every parameter and both moments of every
 * tensor NaN; one infinite gradient makes the norm inf and c = 0, so that element goes NaN and every
 * other one takes the step of a zero gradient.  Without clipping only the element's own p, m and v
 * are touched (NaN for a NaN gradient; m = v = inf and p = NaN for an infinite one).  In
 * wos_siren_fit_run a NaN loss is not <= stop_loss and never stops the run: losses[i] stays NaN from
 * there on and, when clipping, the whole network is NaN after that iteration's step.
 * Pointer rules are wos_siren_fit's: params[k], grads[k], exp_avg, exp_avg_sq and grad_norm are host
 * pointers (staged, blocking), WOS_PTRS_DEVICE, or WOS_PTRS_DEVICE | WOS_ASYNC on `stream`.
 * WOS_E_INVALID, naming the field, before any device work: a NULL pointer or entry, n_tensors out of
 * range, a count <= 0, step < 1, a non-finite lr, beta1 or beta2 outside [0, 1), eps < 0 or not
 * finite, a non-finite max_grad_norm. */
typedef struct wos_adam_params {      /* doubles, as torch.optim.Adam holds them */
    double lr, beta1, beta2, eps;
    double max_grad_norm;             /* <= 0: no clipping (the reference's default, grad_clip = -1) */
} wos_adam_params;
int wos_adam_step(int32_t n_tensors, const int64_t *counts,
                  float *const *params, const float *const *grads,
                  float *exp_avg, float *exp_avg_sq,
                  int64_t step, const wos_adam_params *opt, float *grad_norm,
                  uint32_t flags, int32_t device, void *stream);

/* ---- Device-resident fit loop: n_iters iterations of gather -> fit step -> Adam step ----------
 * The projection fit's training loop (_project_velocity, model_split.py:274-283, in _training_loop,
 * base.py:130-152) on a fixed pool of samples: pool_pts[n_pool*d_in], pool_target[n_pool*d_out],
 * pool_scale[n_pool*d_out] or NULL, idx[n_iters*batch].  Iteration i gathers the rows idx[i][j] of the
 * three pool arrays into a contiguous batch, runs wos_siren_fit's step on it (n = batch, the same
 * workspace_bytes and chunking; the loss to losses[i]) and then wos_adam_step with
 * step = step0 + i + 1 over weights[0..], biases[0..] -- exp_avg and exp_avg_sq are flat in that
 * order.  Bit for bit, in the loss, every parameter and both moments, iteration i is those calls
 * made separately.
 * THIS ENTRY POINT WRITES THROUGH net->weights[l] AND net->biases[l]: the network is updated in
 * place (wos_siren_fit_run_batches below is the only other one that does).
 * Device pointers only: without WOS_PTRS_DEVICE the call is WOS_E_INVALID.  One stream-ordered
 * temporary per call holds the packed weights, the batch, the gradients and the fit step's work.
 * An index outside [0, n_pool) is clamped (no out-of-bounds read) and counted in status[1]; a
 * blocking call that ends with status[1] != 0 returns WOS_E_INVALID.
 * Early stop (the reference's `if early_stop and loss <= 1.1e-10: break` after update_network):
 * stop_loss < 0 never stops.  Otherwise iteration i's update is applied; then, in stream order, a
 * sticky device flag is set when losses[i] <= stop_loss, and every later iteration's Adam step and
 * loss write are no-ops.  losses is filled with NaN at the start, so losses[j] is NaN from the stop
 * on; status[0] is the number of iterations applied.  check_every = 0 enqueues all n_iters
 * iterations without a host synchronisation; check_every = c > 0 (blocking calls only: with
 * WOS_ASYNC it is WOS_E_INVALID) synchronises after every c iterations, reads the flag and stops
 * enqueuing.  The results are the same bits either way.  With check_every = 0 a stop does not shorten
 * the call: every remaining iteration still runs its gather, both packs, the fit step and the norm
 * kernel, only the Adam update and the loss write being switched off; a caller that expects early
 * stops sets check_every.
 * WOS_E_INVALID: n_iters, batch or n_pool <= 0, step0 < 0, a NULL idx, losses, status, pool_pts or
 * pool_target, a NaN stop_loss, wos_adam_step's parameter rules, wos_siren_eval's envelope.
 * A non-zero workspace_bytes below one tile is WOS_E_CAPACITY, as in wos_siren_fit.
 * WOS_FIT_SCALE_MATRIX: pool_scale is [n_pool*d_out*d_out], the gather copies rows of d_out * d_out
 * floats and the step is wos_siren_fit's with the flag; with a NULL pool_scale it is WOS_E_INVALID,
 * naming pool_scale. */
int wos_siren_fit_run(const wos_siren_net *net,
                      const float *pool_pts, const float *pool_target, const float *pool_scale, int64_t n_pool,
                      const int64_t *idx, int64_t n_iters, int64_t batch,
                      float *exp_avg, float *exp_avg_sq, int64_t step0, const wos_adam_params *opt,
                      float stop_loss, int32_t check_every,
                      float *losses, int64_t *status,
                      size_t workspace_bytes, uint32_t flags, int32_t device, void *stream);

/* ---- Device-resident fit loop over ragged batches read in place -------------------------------
 * The advection fit's training loop (_advect_velocity, model_split.py:88-120, in _training_loop,
 * base.py:130-152), whose points are new every iteration and, where samples inside an obstacle are
 * dropped (base.py:239-241), of another count every iteration (added within ABI 10: a new entry point
 * only; DESIGN.md "Device-resident advection fit").  pts[total*d_in], target[total*d_out] and
 * scale[total*d_out] or NULL hold the rows of all iterations one after the other; offsets is a HOST
 * array of n_iters + 1 row offsets, offsets[0] >= 0 (it need not be 0) and strictly increasing.
 * Iteration i is wos_siren_fit's step on the n_i = offsets[i+1] - offsets[i] rows from offsets[i] on,
 * read in place (no gather, no copy; a batch's first row needs no more than a float's alignment),
 * with wos_siren_fit's own chunking for n = n_i and the same workspace_bytes, the loss, a mean over
 * n_i d_out, to losses[i]; then wos_adam_step with step = step0 + i + 1.  Bit for bit, in the loss,
 * every parameter and both moments, iteration i is
 *   wos_siren_fit(net, pts + offsets[i]*d_in, n_i, target + offsets[i]*d_out,
 *                 scale ? scale + offsets[i]*d_out : NULL, ...) and wos_adam_step(...)
 * made separately.  THE NETWORK IS UPDATED IN PLACE through net->weights[l] and net->biases[l], as
 * in wos_siren_fit_run.  Device pointers only (offsets excepted).  One stream-ordered temporary per
 * call holds the packed weights, the gradients and the fit step's work, sized for the largest n_i.
 * Early stop, losses (NaN from the stop on), check_every and status[0] are wos_siren_fit_run's;
 * status[1] is always 0: there is no index to clamp.
 * WOS_E_INVALID, naming the field, before any device work: n_iters <= 0, step0 < 0, a NULL pts,
 * target, offsets, losses, status, exp_avg or exp_avg_sq, offsets[0] < 0, an iteration without rows
 * (offsets[i+1] <= offsets[i]: a mean over nothing; the iteration is named), a NaN stop_loss,
 * check_every < 0 or check_every > 0 with WOS_ASYNC, wos_adam_step's parameter rules,
 * wos_siren_eval's envelope.  A non-zero workspace_bytes below one tile is WOS_E_CAPACITY.
 * WOS_FIT_SCALE_MATRIX: scale is [total*d_out*d_out], iteration i reads it from
 * scale + offsets[i]*d_out*d_out on, and the step is wos_siren_fit's with the flag; with a NULL scale
 * it is WOS_E_INVALID, naming scale. */
int wos_siren_fit_run_batches(const wos_siren_net *net,
                              const float *pts, const float *target, const float *scale,
                              const int64_t *offsets, int64_t n_iters,
                              float *exp_avg, float *exp_avg_sq, int64_t step0, const wos_adam_params *opt,
                              float stop_loss, int32_t check_every,
                              float *losses, int64_t *status,
                              size_t workspace_bytes, uint32_t flags, int32_t device, void *stream);

/* ---- Ensemble fit loops: up to WOS_MAX_CHANNELS networks trained in one device loop ------------
 * The two loops above for n_members = 1..WOS_MAX_CHANNELS networks of one shape, the members of an
 * ensemble on one obstacle mesh after a multi-channel solve (added within ABI 10: new entry points
 * only; DESIGN.md "Ensemble fit loops").  nets[n_members]; pool_target / target, pool_scale / scale,
 * exp_avg and exp_avg_sq are HOST arrays of n_members device pointers (pool_scale / scale may be
 * NULL, or hold NULL entries: that member has no scale); losses[n_members][n_iters] and
 * status[n_members][2] are device arrays, member-major.
 * Shared by the members: the points, the index draw `idx` or the row offsets, opt and step0 -- common
 * random numbers, as the walks of the multi-channel solve are.  A member's own: its network, targets
 * and scales, both moments, its row of losses and its status pair.
 * Every launch of an iteration covers all members (an iteration stays eleven launches).  Bit for bit,
 * member e's losses, every parameter and both moments are those of wos_siren_fit_run /
 * wos_siren_fit_run_batches called on member e's arguments alone; workspace_bytes counts per member,
 * and the call's one stream-ordered temporary is n_members times as large.
 * Early stop: the stop flag is sticky per member; a stopped member's later updates and loss writes
 * are no-ops while the others go on, and check_every = c stops enqueuing once every member's flag is
 * set.  status[e][1] counts the clamped indices of the shared draw (the same number for every e).
 * WOS_E_INVALID, naming the field and the member, before any device work and writing nothing:
 * n_members outside 1..WOS_MAX_CHANNELS, members that differ in d_in, d_out, hidden,
 * n_hidden_layers or omega, two members sharing a weights or biases pointer or a moment buffer, a
 * NULL entry of nets' arrays, pool_target / target, exp_avg or exp_avg_sq, and every refusal of the
 * single-network entry points.
 * WOS_FIT_SCALE_MATRIX covers every member that has a scale: each non-NULL entry of pool_scale / scale
 * is [rows][d_out][d_out]; a NULL entry is still the identity (the unscaled step's bits).  The flag
 * with a NULL array, or with every entry NULL, is WOS_E_INVALID, naming pool_scale / scale. */
int wos_siren_fit_run_ensemble(int32_t n_members, const wos_siren_net *nets,
                               const float *pool_pts, const float *const *pool_target,
                               const float *const *pool_scale, int64_t n_pool,
                               const int64_t *idx, int64_t n_iters, int64_t batch,
                               float *const *exp_avg, float *const *exp_avg_sq, int64_t step0,
                               const wos_adam_params *opt, float stop_loss, int32_t check_every,
                               float *losses, int64_t *status,
                               size_t workspace_bytes, uint32_t flags, int32_t device, void *stream);

int wos_siren_fit_run_batches_ensemble(int32_t n_members, const wos_siren_net *nets,
                                       const float *pts, const float *const *target, const float *const *scale,
                                       const int64_t *offsets, int64_t n_iters,
                                       float *const *exp_avg, float *const *exp_avg_sq, int64_t step0,
                                       const wos_adam_params *opt, float stop_loss, int32_t check_every,
                                       float *losses, int64_t *status,
                                       size_t workspace_bytes, uint32_t flags, int32_t device, void *stream);

const char *wos_last_error(void);
int32_t wos_abi_version(void);
int32_t wos_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* WOS_H */
