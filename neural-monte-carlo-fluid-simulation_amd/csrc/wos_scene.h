// wos_scene.h -- scene and solver-parameter layouts shared by the host-side scene
// preparation (wos_scene.cpp) and the gfx950 kernels (wos_kernel.hip).
//
// HBM layout (all float32, structure-of-records, 16-byte aligned):
//   prim  : Neumann primitives, packed per primitive
//           2D  [pa.x pa.y v.x v.y], v = pb - pa               (4 floats)
//           3D  [pa.xyz pb.xyz pc.xyz]                         (9 floats)
//   paux  : per-primitive normals used only by signed-distance queries
//           2D  [na.xy nb.xy nseg.xy]  (vertex normals at the ends + segment normal)
//           3D  [na nb nc | e0 e1 e2 | nface]  (vertex, edge, face normals; 21 floats)
//   sil   : silhouette candidates (vertices in 2D, edges in 3D)
//           2D  [p.xy n0.xy n1.xy miss pad]                    (8 floats)
//           3D  [pa.xyz pb.xyz n0.xyz n1.xyz miss pad pad pad] (16 floats)
//   dprim/dpaux : same as prim/paux for the (optional) Dirichlet boundary
//   source: the -div(u) grid, row-major; 2D (H rows ~ y, W cols ~ x), 3D (X,Y,Z);
//           with n_channels > 1 texel-interleaved, [cell][kMaxChannels] (unused channels +0)
//   pgroup/sgroup: padded boxes of kGroup consecutive prims / silhouettes
//           (8 / 16 floats, see kSGroupStride), used only to skip whole groups
//
// The Neumann prim + sil arrays are staged into LDS by every workgroup.
#pragma once
#include <stdint.h>

namespace wos {

constexpr int kPrimStride2 = 4, kPrimStride3 = 9;
constexpr int kAuxStride2 = 6, kAuxStride3 = 21;
constexpr int kSilStride2 = 8, kSilStride3 = 16;
// most source channels of one solve (WOS_MAX_CHANNELS): one 16-byte texel per grid cell
constexpr int kMaxChannels = 4;
// culling groups: kGroup consecutive primitives (or silhouette candidates) share
// one padded bounding box record [min.xyz pad max.xyz pad]; silhouette groups add
// a bounding sphere and the cone of their adjacent normals:
//   [min.xyz sin(alpha) | max.xyz cos(alpha) | c.xyz rho | axis.xyz nocull]
constexpr int kGroup = 8, kGroupStride = 8, kSGroupStride = 16;

// Bounding-volume hierarchy over a group array (the role of fcpw's 8-wide MBVH,
// mbvh.inl:702-818, for meshes far beyond the reference's): an implicit 8-ary tree
// whose level-0 nodes are the groups and whose node (L, i), L >= 1, bounds the
// groups [i 8^L, (i+1) 8^L) with the union of their padded boxes ([min pad | max pad],
// kGroupStride floats).  Levels are built until at most 8 nodes remain; scenes with
// at most kTreeMinGroups groups get none (levels = 0: the flat group scan).
constexpr int kTreeLevels = 8;
constexpr int kTreeMinGroups = 64;
struct DevTree {
  const float* node;           // level L's boxes at node + off[L] * kGroupStride (L >= 1)
  int32_t levels;              // 0: no tree
  int32_t n[kTreeLevels + 1];  // n[0] = groups, n[L] = nodes of level L
  int32_t off[kTreeLevels + 1];
};

template <int DIM> struct Layout;
template <> struct Layout<2> {
  static constexpr int prim = kPrimStride2, aux = kAuxStride2, sil = kSilStride2;
};
template <> struct Layout<3> {
  static constexpr int prim = kPrimStride3, aux = kAuxStride3, sil = kSilStride3;
};

struct DevScene {
  int32_t dim;
  int32_t n_prims, n_sil, n_dprims;
  const float* prim;
  const float* paux;
  const float* sil;
  const float* dprim;
  const float* dpaux;
  const float* source;
  const float* pgroup;   // n_pgroups boxes over consecutive Neumann primitives
  const float* sgroup;   // n_sgroups boxes over consecutive silhouette candidates
  const float* dgroup;   // n_dgroups boxes over consecutive Dirichlet primitives
  int32_t n_pgroups, n_sgroups, n_dgroups;
  DevTree ptree, stree, dtree;  // hierarchies over pgroup / sgroup / dgroup
  // fcpw's wide BVH over the Neumann primitives (wos_host_scene.h HostFcpwBvh), read
  // from global memory by the stochastic boundary sample; nullptr without Neumann prims
  const float* nbvh_box;
  const int32_t* nbvh_child;
  const int32_t* nbvh_ref;
  int32_t nbvh_branch;
  // 1: the kernels read the geometry records from global memory (L2) instead of
  // staging them in LDS -- scenes too large for the LDS budget (set per solve)
  int32_t geom_global;
  int32_t sdims[3];
  float pmin[3], pmax[3], ext[3];
  float absorption;
  float g_dirichlet;
  // image-valued Dirichlet data (wos_scene_desc.dirichlet_image; nullptr: g_dirichlet):
  // [ddims[0]][ddims[1]] over the rectangle dbox = (x0, y0, ex, ey)
  const float* dimg;
  int32_t ddims[2];
  float dbox[4];
  // image-valued Neumann data h (wos_scene_desc.neumann_image; nullptr: h = 0, the reference's):
  // [ndims[0]][ndims[1]] over the rectangle nbox = (x0, y0, ex, ey)
  const float* nimg;
  int32_t ndims[2];
  float nbox[4];
  int32_t watertight;
  int32_t double_sided;
  // star-radius cell grid (wos_host_scene.h StarGrid; nullptr: none): u16 cell
  // offsets then u8 candidate lists, staged into LDS by the walk kernel
  const uint32_t* sgrid;
  int32_t sgrid_words, sgrid_off_words;
  int32_t sgrid_n[3];
  float sgrid_min[3], sgrid_inv[3];
  // Dirichlet-distance cell grid (2D; wos_host_scene.h DirGrid; nullptr: none), global
  // memory: u32 cell offsets then u16 segment indices
  const uint32_t* dgrid;
  int32_t dgrid_off_words;
  int32_t dgrid_n[2];
  float dgrid_min[2], dgrid_inv[2];
  // source channels (wos_scene_set_source_channels; 1: the plain grid) and channel c's
  // Dirichlet constant (g_dirichlet unless given per channel; unused with dimg)
  int32_t n_channels;
  float g_ch[kMaxChannels];
};

struct DevParams {
  int32_t n_walks;          // as configured (nWalks)
  int32_t n_pairs;          // walks per antithetic iteration set (nWalks/2 or nWalks)
  int32_t n_anti;           // 2 with antithetic variates, else 1
  int32_t max_walk_length;
  int32_t steps_before_tikhonov;
  int32_t steps_before_maximal_spheres;
  float epsilon_shell;
  float min_star_radius;
  float silhouette_precision;
  float rr_threshold;
  float boundary_distance_mask;
  int32_t use_cv;
  int32_t use_cosine;
  int32_t ignore_dirichlet;
  int32_t ignore_neumann;
  int32_t ignore_source;
  int32_t robust;           // wos_solver_params.robust_float (Gfn::scaled)
  int32_t neumann_inert;    // 1: no ball can reach the float-overflow regime (walk kernel without the Neumann term)
  int32_t force_estimate;   // 1: estimate every point, inside the domain or not (BVC's Dirichlet samples:
                            // BoundarySampler::computeEstimates solves at every sample, boundary_sampler.h:125-166)
  int32_t tail_spread;      // 1: the walk kernel instantiation that hands walks to idle sibling waves
  int32_t wave_prio;        // 0..3: the walk / fold kernels' waves issue at this priority (s_setprio) --
                            // boundary value caching's concurrent walk sets, longest chain highest
  uint64_t seed;
  // PCG32 jump-ahead table: jump[2k], jump[2k+1] = (A_k, C_k) with
  // state_k = A_k * state_0 + C_k (mod 2^64); lets the lanes of a wave draw the
  // per-point stratified samples in parallel.  n_jump entries.
  const uint64_t* jump;
  int32_t n_jump;
  // entries of jump staged in the first-ball kernel's LDS (its stratified-sample draws; 0: none)
  int32_t lhs_jump_n;
  // certain-reject bounds of the Yukawa rejection threshold by bin of s = mu R
  // (wos_host_scene.h rejection_bound_table), kRejTabBins floats; nullptr: none
  const float* rej_tab;
};

// bins of the rejection bound table: bin = floor(kRejTabScale * sqrt(mu R))
// the walk kernel's task-queue counters (wos_launch.h kTaskQueueSlot0): at most
// kMaxTaskQueues, kTaskQueueStride u32 words (64 B) apart
constexpr int kMaxTaskQueues = 32;
constexpr unsigned int kTaskQueueStride = 16;
constexpr int kRejTabBins = 96;
// most jump constants the first-ball kernel stages in LDS (16 B each)
constexpr int kLhsJumpMax = 512;
constexpr float kRejTabScale = 8.0f;

// Walk-task workspace of one batch of points, SoA over T = n_points * wpp tasks
// (task t = point * wpp + pair * n_anti + member).  Written by the first-ball
// kernel, advanced by the walk kernel, folded by the statistics kernel.
struct DevTasks {
  float* pt;        // [DIM][T] walk start: the first ball's boundary sample
  float* thr;       // [T] throughput after the first ball
  float* tsrc;      // [C][T] source contribution of the first ball (C = DevScene::n_channels)
  float* dd;        // [T] Dirichlet distance at pt
  float* first;     // [C][T] record: first-ball source value (control variate)
  float* bdir;      // [DIM][T] record: boundary gradient direction
  float* sdir;      // [DIM][T] record: source gradient direction
  float* total;     // [C][T] record: walk total
  uint32_t* code;   // [T] record: (steps << 1) | recorded
  int32_t* pstate;  // [n] bit0 estimated, bit1 mask p, bit2 mask grad p, bits 8..12 cost bucket
  uint32_t* perm;   // [n] walk-queue order of the points (longest expected walks first)
  uint32_t* hist;   // [2 * kCostBuckets] bucket counts, then running bucket offsets
  float* prad;      // [n] first-ball radius 0.99 min(dDist, nDist) (point-setup kernel -> presorted first balls)
  int64_t T;
  int32_t wpp;      // walks per point = n_pairs * n_anti
  // length hints of the plain 2D walk kernels (kHint*, below), in the padding that followed wpp, so the
  // layout every other kernel sees is unchanged; 0: neither collect nor use
  uint32_t hint;
  // Boundary-start walks (estimateSolution, walk_on_stars.h:353-464; boundary value
  // caching): per task the start normal [DIM][T], the first sphere radius [T] and
  // bit 0 "starts on the Neumann boundary" [T].  They alias the first-ball record
  // arrays (bdir, first, sdir), which such walks do not use; nullptr otherwise.
  float* n0;
  float* r0;
  uint32_t* sflags;
  // [4][pball_stride] per point: the 2D Yukawa first ball's Bessel members K0 I0 K1 I1 at
  // mu R (Gfn::update_ball), written by the point-setup kernel (one lane per point) for the
  // reference-semantics first-ball kernel; nullptr: the first-ball kernel evaluates them
  float* pball;
  int64_t pball_stride;
  // per point [n][DIM] SampleEstimationData::directionForDerivative (nullptr: (1, 0[, 0]),
  // walk_on_stars.h:665-666) and the estimated directional derivative out [n]
  // (getEstimatedDerivative, :843-846; nullptr: not computed) -- BVC's Dirichlet samples
  const float* ddir;
  float* deriv;
};

// ---- length hints (Length hints) ----
// The walks of a solve do not depend on the source, so a time-stepper's next projection repeats
// them step for step.  The plain 2D walk kernel lists the walks that took >= hint_min steps; the
// next solve of the same walks starts those of >= express_min steps first, longest first, in
// waves that hold nothing else ("express").  A scheduling hint only: results do not depend on it.
// DevTasks::hint: bit 0 collect, bit 1 use the express list, bits 2-3 the express waves' issue
// priority, bit 4 striped claims, bit 5 pinned placement (express layout, below), bits 8-23 hint_min.
constexpr uint32_t kHintCollect = 1u, kHintUse = 2u, kHintStripe = 16u, kHintPinned = 32u;
constexpr int kHintBins = 1024;  // the build kernel's histogram by steps (its block size): solo_min < kHintBins
constexpr int kHintPrioShift = 2, kHintMinShift = 8;
constexpr uint32_t kHintMinMask = 0xFFFFu;
constexpr int32_t kPtExpress = 1 << 16;    // pstate: some walk of the point is express-owned
constexpr uint32_t kHintListMax = 1u << 16;  // entries of the collection list (and of the express list)
// the control block's first word, counted from the walk kernel's task queues (its `tqueue`)
constexpr int kHintBlockWord = kMaxTaskQueues * (int)kTaskQueueStride;
// The control block: u32 words that follow the main solve's counter slots (kNumCounterSlots u64 after
// `counters`).  The two atomics of the walk kernel sit on lines of their own.
enum {
  H_NLIST = 0,      // walks offered to the list by the running walk kernel (may exceed H_CAP)
  H_XCLAIM = 16,    // claims handed out (express_slot, below)
  H_NEXPRESS = 32,  // entries of the express list
  H_EPW,            // express walks a claim below the solo tier holds
  H_CAP,            // capacity of the list in use (<= kHintListMax)
  H_CLAIMED,        // express walks started by the last hinted walk kernel
  H_NSOLO,          // entries of the solo tier: the first H_NSOLO of the list, a claim each
  H_XG,             // claims below the solo tier: ceil((H_NEXPRESS - H_NSOLO) / H_EPW)
  H_CK_CUR = 48,    // u64: checksum of the points of the running solve (point setup)
  H_CK_LIST = 50,   // u64: ... of the solve that filled the list
  H_LIST = 52,      // u64: uint2* (task, steps)
  H_EXPRESS = 54,   // u64: uint32_t* tasks, longest first
  H_BITS = 56,      // u64: uint32_t* one bit per task: express-owned
  H_WORDS = 64
};

// ---- express layout: which entries of the express list (longest first) a claim holds ----
// The first n_solo entries, the longest walks, are a claim each: a wave of their own.  The m = nx -
// n_solo entries below go to G = ceil(m / epw) claims of up to epw: striped, claim n_solo + i holds
// the entries n_solo + i + j G (one of each length band, so the wave thins out as the short ones
// end); unstriped, the contiguous block n_solo + i epw + j.  Entry j of claim c, or kExpressNone;
// a claim's entries are j = 0, 1, ... without a gap, and every entry of [0, nx) belongs to exactly
// one (claim, j) (tests/test_express_layout_cpu.py walks the whole table).
constexpr uint32_t kExpressNone = 0xFFFFFFFFu;
#ifdef __HIP__
#define WOS_HOST_DEVICE __host__ __device__
#else  // (a host compiler reads this header too: wos_variant.h)
#define WOS_HOST_DEVICE
#endif
WOS_HOST_DEVICE inline uint32_t express_claims_below(uint32_t nx, uint32_t n_solo, uint32_t epw) {
  return epw > 0u && nx > n_solo ? (nx - n_solo + epw - 1u) / epw : 0u;
}
// (G: express_claims_below(nx, n_solo, epw), which the build kernel leaves in H_XG)
WOS_HOST_DEVICE inline uint32_t express_slot_g(uint32_t c, uint32_t j, uint32_t nx, uint32_t n_solo, uint32_t epw,
                                                   uint32_t stripe, uint32_t G) {
  if (c < n_solo) return j == 0u && c < nx ? c : kExpressNone;
  const uint32_t i = c - n_solo;
  if (i >= G || j >= epw) return kExpressNone;
  const uint32_t e = n_solo + (stripe ? i + j * G : i * epw + j);  // (nx <= kHintListMax, epw <= 64: no overflow)
  return e < nx ? e : kExpressNone;
}
WOS_HOST_DEVICE inline uint32_t express_slot(uint32_t c, uint32_t j, uint32_t nx, uint32_t n_solo, uint32_t epw,
                                                 uint32_t stripe) {
  return express_slot_g(c, j, nx, n_solo, epw, stripe, express_claims_below(nx, n_solo, epw));
}

// What a recording pass (wos_tape.hip) keeps of a batch's walks instead of their source-dependent
// values, so that wos_tape_replay_kernel can redo totalSource and the walk total for any source
// grid.  Per task [T]; entries SoA over the batch's entry slots.  Task t owns the slots
// [slot[t], slot[t + 1]) (an exclusive scan of an upper bound of its entries, slot[T] = all).
struct DevTape {
  float* gnorm;          // [T] first ball: the Green's function norm of its source sample
  uint32_t* cell0;       // [T] first ball: the source grid cell of its source sample
  const uint32_t* slot;  // [T + 1] first entry slot of task t
  uint32_t* cnt;         // [T] entries written | bit 31: Dirichlet end with the constant g (walk_finish own_g)
  float* thr_end;        // [T] final throughput
  float* term;           // [T] terminal contribution g (0 without one)
  float* tneu;           // [T] totalNeumann
  uint32_t* e_cell;      // [slots] source grid cell of a step's source sample, in step order
  float* e_thr;          // [slots] throughput before the step (pThr)
  float* e_nrm;          // [slots] Green's function norm of the step's ball (pNrm)
  uint32_t* overflow;    // [1] set when a recorded walk had more entries than slots (the tape is discarded)
};
constexpr uint32_t kTapeOwnG = 0x80000000u;
// entries the replay kernel stages per wave and pass (one per lane)
constexpr int kTapeChunk = 64;

// floats per task: start state pt[DIM] thr tsrc dd, record first bdir[DIM] sdir[DIM] total code;
// every source channel beyond the first adds its own tsrc, first and total
constexpr int task_floats(int dim, int channels = 1) { return 3 * dim + 6 + 3 * (channels - 1); }
constexpr int kCostBuckets = 32;

}  // namespace wos
