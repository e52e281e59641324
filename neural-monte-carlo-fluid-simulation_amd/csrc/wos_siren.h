// wos_siren.h -- host interface of the fused SIREN value / Jacobian / divergence kernel
// (wos_siren.hip).  Its own header: the five solve kernel units do not see it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace wos {

constexpr int kSirenTile = 32;          // points per workgroup: one 32-column MFMA tile per carried column
constexpr int kSirenMaxHidden = 256;    // H: a multiple of 32 in 32 .. 256
constexpr int kSirenMaxHiddenLayers = 8;                        // L
constexpr int kSirenMaxLayers = kSirenMaxHiddenLayers + 2;      // Linear layers: L + 2

// Device pointers of one network, torch layout: w[l] [out][in] row-major, b[l] [out];
// l = 0 the first layer, 1 .. L the hidden ones, L + 1 the output layer.
struct SirenNet {
  int d_in, d_out, H, L;
  float omega;
  const float* w[kSirenMaxLayers];
  const float* b[kSirenMaxLayers];
};

// An ensemble: up to kSirenMaxMembers networks of one shape trained side by side.  A launch with a
// member axis carries every member's own pointers in its arguments (about 740 bytes of SirenNet);
// what the members keep in the call's temporary lies a fixed stride apart, member e at + e * stride.
constexpr int kSirenMaxMembers = 4;
struct SirenNets {
  SirenNet v[kSirenMaxMembers];
};
// the rows of one fit step per member: target [n][d_out] and scale (null: 1), [n][scale_width] with
// scale_width = d_out (a factor per component; 0 stands for it) or d_out * d_out (a row-major matrix
// per point); one width for every member that has a scale
struct SirenMemberRows {
  const float* target[kSirenMaxMembers];
  const float* scale[kSirenMaxMembers];
  int scale_width;
};

// floats of the fragment-ordered copy of the L hidden weight matrices (0 for L = 0)
inline size_t siren_pack_floats(int H, int L) { return (size_t)L * H * H; }

// Rewrites hidden layer l's W [H][H] as packed[l][r][q][lane][e] = W[32 r + (lane & 31)][8 q + 2 e + (lane >> 5)]:
// the A operand of k-step 4 q + e of row tile r, one 16-byte load per lane and four k-steps.
hipError_t launch_siren_pack(const SirenNet& net, float* packed, hipStream_t s);
// The same for members 0 .. E - 1 in one launch: member e's copy at packed + e * member_stride.
hipError_t launch_siren_pack_members(const SirenNets& nets, int E, float* packed, size_t member_stride, hipStream_t s);

// u [n][d_out], jac [n][d_out][d_in], div [n]: each may be null.  packed: launch_siren_pack's.
hipError_t launch_siren_eval(const SirenNet& net, const float* packed, const float* pts, int64_t n, float* u,
                             float* jac, float* div, hipStream_t s);

// The hidden-layer GEMM of launch_siren_eval alone (the same device function): Z[p][0] = W X[p][0] + b,
// Z[p][s] = W X[p][s] for s = 1 .. d_in; X and Z [n][1 + d_in][H]; packed: H * H floats of scratch.
hipError_t launch_siren_layer_selftest(int H, int d_in, int64_t n, const float* W, const float* b, float* packed,
                                       const float* X, float* Z, hipStream_t s);

// The same kernel on weights that are already fragment-ordered (launch_siren_pack's layout, or
// launch_siren_pack_transposed's for Z = W^T X).
hipError_t launch_siren_layer_packed(int H, int d_in, int64_t n, const float* packed, const float* b, const float* X,
                                     float* Z, hipStream_t s);

// ---- backward (wos_siren_vjp.hip) --------------------------------------------------------------
// packedT[l][r][q][lane][e] = W[8 q + 2 e + (lane >> 5)][32 r + (lane & 31)]: launch_siren_pack's copy of W^T.
hipError_t launch_siren_pack_transposed(const SirenNet& net, float* packedT, hipStream_t s);
hipError_t launch_siren_pack_transposed_members(const SirenNets& nets, int E, float* packedT, size_t member_stride,
                                                hipStream_t s);

// Gradient pointers of one network, shapes of SirenNet's w and b.
struct SirenGrads {
  float* w[kSirenMaxLayers];
  float* b[kSirenMaxLayers];
};

// The backward's temporaries for chunks of `tiles` 32-point tiles, in floats.
struct SirenVjpPlan {
  int tiles;         // tiles per chunk
  int slices;        // split-K slices of the weight-gradient kernel per chunk
  size_t stash;      // (2 L + 1) H C 32 floats per tile: X_0 .. X_L (first the pre-activations) and dZ_1 .. dZ_L
  size_t tile_part;  // per-tile partials of dWo, dbo, db_0 .. db_L and dW0
  size_t slice_part; // per-slice partials of dW_1 .. dW_L
  size_t total() const { return stash + tile_part + slice_part; }
};
inline size_t siren_vjp_stash_floats_per_tile(int d_in, int H, int L) { return (size_t)(2 * L + 1) * H * (1 + d_in) * kSirenTile; }
inline size_t siren_vjp_tile_part_floats(const SirenNet& net) {
  return (size_t)net.d_out * net.H + net.d_out + (size_t)(net.L + 1) * net.H + (size_t)net.H * net.d_in;
}
constexpr int kSirenWgradSliceBlocks = 16;  // 32-column blocks of K per split-K slice
// resident_tiles: how many tile workgroups the device holds at once (0: unknown); when the points
// need several chunks, a chunk is a whole multiple of it, so that no chunk ends in a thin round.
SirenVjpPlan siren_vjp_plan(const SirenNet& net, int64_t n, size_t stash_cap_bytes, int resident_tiles);
size_t siren_vjp_tile_lds_bytes(int d_in, int H);  // dynamic LDS of one tile workgroup

// grads = the vector-Jacobian product of (u, J, div) with (g_u, g_jac, g_div), each may be null,
// summed over the n points; written, not accumulated.  packed / packedT: the two fragment-ordered
// copies; zeros: H zero floats; work: plan.total() floats.  The same n and plan give the same bits.
hipError_t launch_siren_vjp(const SirenNet& net, const float* packed, const float* packedT, const float* zeros,
                            const float* pts, int64_t n, const float* g_u, const float* g_jac, const float* g_div,
                            const SirenGrads& grads, const SirenVjpPlan& plan, float* work, hipStream_t s);

// The backward's two generic launches, shared with the fit step (wos_siren_fit.hip).
// A row of partials is cut into segments, each with its own destination: dst[k] receives the
// elements [end[k - 1], end[k]) of the row.
constexpr int kReduceSegs = 12;
static_assert(kReduceSegs >= kSirenMaxHiddenLayers + 4,
              "the tiles' partials are cut into L + 4 segments: dWo, dbo, db_0 .. db_L, dW0");
struct SirenReduceSegs {
  int n;
  int end[kReduceSegs];
  float* dst[kReduceSegs];
};
// dst(e) = (accumulate ? dst(e) : 0) + sum over i < n_part of part[i * stride + e], in an order
// that depends on n_part alone.
hipError_t siren_reduce(const float* part, int n_part, size_t stride, const SirenReduceSegs& segs, bool accumulate,
                        hipStream_t s);
// E members in one launch: member e reads part + e * part_member_stride and writes dst[k] + e * dst_member_stride.
hipError_t siren_reduce_members(const float* part, int n_part, size_t stride, const SirenReduceSegs& segs, bool accumulate,
                                int E, size_t part_member_stride, size_t dst_member_stride, hipStream_t s);
// part[slice][l] [H][H] = dZ_l X_{l-1}^T over the slice's column blocks: ds, xs [L][tiles][H][C * 32]
// (layer_stride apart), C columns per point, columns of points past n_valid masked.
hipError_t siren_wgrad(const float* ds, const float* xs, size_t layer_stride, int H, int C, int tiles, int64_t n_valid,
                       float* part, int L, hipStream_t s);
// E members in one launch (grid z = member * L + layer): member e's ds, xs and part at + e * member_stride.
hipError_t siren_wgrad_members(const float* ds, const float* xs, size_t layer_stride, int H, int C, int tiles,
                               int64_t n_valid, float* part, int L, int E, size_t member_stride, hipStream_t s);

// wos_selftest_siren_vjp_layer's device half: dX = W^T dZ from the transposed pack and
// siren_hidden_gemm, dW = sum dZ X^T from the weight-gradient kernel and its reduction.  dZ, X, dX
// [n][1 + d_in][H]; packedT, zeros as above; work: siren_vjp_layer_selftest_floats(H, d_in, n).
size_t siren_vjp_layer_selftest_floats(int H, int d_in, int64_t n);
hipError_t launch_siren_vjp_layer_selftest(int H, int d_in, int64_t n, const float* W, float* packedT, const float* zeros,
                                           const float* dZ, const float* X, float* dX, float* dW, float* work,
                                           hipStream_t s);

// ---- fit step (wos_siren_fit.hip) --------------------------------------------------------------
// The fit step's temporaries for chunks of `tiles` 32-point tiles, in floats.  One column per point.
struct SirenFitPlan {
  int tiles;          // tiles per chunk
  int slices;         // split-K slices of the weight-gradient kernel per chunk
  size_t stash;       // (2 L + 1) H 32 floats per tile: z_0 .. z_L (then a_0 .. a_{L-1}) and dz_1 .. dz_L
  size_t tile_part;   // per-tile partials of dWo, dbo, db_0 .. db_L and dW0 (the backward's layout)
  size_t slice_part;  // per-slice partials of dW_1 .. dW_L
  size_t loss_part;   // per-tile sums of squared residuals
  size_t total(bool grads) const { return grads ? stash + tile_part + slice_part + loss_part : loss_part; }
};
inline size_t siren_fit_stash_floats_per_tile(int H, int L) { return (size_t)(2 * L + 1) * H * kSirenTile; }
// The chunking follows from the stash's cap whether or not gradients are asked for: the loss-only
// call sums in the full call's order.
SirenFitPlan siren_fit_plan(const SirenNet& net, int64_t n, size_t stash_cap_bytes, int resident_tiles);
size_t siren_fit_tile_lds_bytes(int d_in, int H);  // dynamic LDS of one tile workgroup

// loss[0] = 1 / (n d_out) sum (scale u - target)^2 (scale null: 1) and, with grads non-null, its
// gradient (written, not accumulated).  scale_width: SirenMemberRows'; with d_out * d_out the
// residual is S u - target and the seed S^T (2 r) / (n d_out).  grads null: the loss alone -- packedT, zeros may be null,
// work holds plan.total(false) floats.  n >= 1.  The same n and plan give the same bits.
hipError_t launch_siren_fit(const SirenNet& net, const float* packed, const float* packedT, const float* zeros,
                            const float* pts, int64_t n, const float* target, const float* scale, int scale_width,
                            float* loss, const SirenGrads* grads, const SirenFitPlan& plan, float* work, hipStream_t s);
// The same step for members 0 .. E - 1 on the same points, each launch covering all of them: member e
// does exactly what launch_siren_fit does on nets.v[e] and its rows.  packed, packedT and work are
// member 0's, member e's lie e * member_stride floats further on; `zeros` is shared.  loss: member e's
// at loss + e * loss_stride.  grads: member 0's, each pointer of member e's grad_stride floats further on.
hipError_t launch_siren_fit_members(const SirenNets& nets, int E, const float* packed, const float* packedT,
                                    const float* zeros, const float* pts, int64_t n, const SirenMemberRows& rows,
                                    float* loss, size_t loss_stride, const SirenGrads* grads, size_t grad_stride,
                                    const SirenFitPlan& plan, float* work, size_t member_stride, hipStream_t s);

// ---- optimiser step and the device-resident fit loop (wos_siren_train.hip) ----------------------
// The tensors of one Adam step in their flat order: tensor k holds the elements [end[k - 1], end[k])
// of exp_avg and exp_avg_sq, its parameters at p[k] and its gradients at g[k].
constexpr int kAdamMaxTensors = 20;
static_assert(kAdamMaxTensors == 2 * kSirenMaxLayers, "wos_siren_fit_run steps a weight and a bias per Linear layer");
struct AdamSegs {
  int n;
  int64_t end[kAdamMaxTensors];
  float* p[kAdamMaxTensors];
  const float* g[kAdamMaxTensors];
};
// The step's scalars, each rounded once from double: beta2, 1 - beta1, 1 - beta2, sqrt(1 - beta2^step),
// lr / (1 - beta1^step), eps, max_grad_norm.
struct AdamScalars {
  float b2, omb1, omb2, bc2, ss, eps, max_norm;
};
// One Adam step per member: its tensors and its two moment buffers.
struct AdamMembers {
  AdamSegs segs[kSirenMaxMembers];
  float* exp_avg[kSirenMaxMembers];
  float* exp_avg_sq[kSirenMaxMembers];
};
// A fit loop's state words, kFitStateWords per member: [0] the sticky stop flag, [1] the bits of the
// iteration's loss, [2] the gradient norm.
constexpr int kFitStateWords = 64;
// norm[0] = the L2 norm of all gradients, one workgroup, a fixed order.
hipError_t launch_adam_norm(const AdamSegs& segs, float* norm, hipStream_t s);
// One workgroup per member: member e's norm to norm[e * kFitStateWords].
hipError_t launch_adam_norm_members(const AdamMembers& m, int E, float* norm, hipStream_t s);
// norm non-null: the gradients count as g * min(max_norm / (norm[0] + 1e-6f), 1).  stop non-null and
// stop[0] != 0: nothing is written.
hipError_t launch_adam_update(const AdamSegs& segs, float* exp_avg, float* exp_avg_sq, const AdamScalars& sc,
                              const float* norm, const int* stop, hipStream_t s);
// All members in one launch: member e's norm and stop words lie e * kFitStateWords further on.
hipError_t launch_adam_update_members(const AdamMembers& m, int E, const AdamScalars& sc, const float* norm,
                                      const int* stop, hipStream_t s);
// wos_siren_fit_run's state: state[0] the sticky stop flag, state[1] the bits of the iteration's loss.
// The gather copies rows idx[0 .. batch) of the pool arrays (pool_scale and scale may be null; their
// rows are scale_width floats, 0: d_out) into pts / target / scale, clamping and counting (status[1]) an index outside [0, n_pool), and commits
// iteration prev >= 0 first: unless stopped, losses[prev] = the loss, status[0] = prev + 1, and the
// flag is set when stop_loss >= 0 and the loss <= stop_loss.  launch_fit_run_commit: the commit alone.
hipError_t launch_fit_run_gather(int d_in, int d_out, const float* pool_pts, const float* pool_target,
                                 const float* pool_scale, int scale_width, int64_t n_pool, const int64_t* idx,
                                 int64_t batch, float* pts, float* target, float* scale, int* state, int64_t prev, float stop_loss, float* losses,
                                 int64_t* status, hipStream_t s);
hipError_t launch_fit_run_commit(int* state, int64_t iter, float stop_loss, float* losses, int64_t* status,
                                 hipStream_t s);
// The same for E members that share the pool's points and the index draw.  Member e gathers its own
// pool_target[e] / pool_scale[e] (a null entry: no scale; rows of scale_width floats, 0: d_out) into
// target / scale + e * rows_stride and
// commits into state + e * kFitStateWords, losses + e * losses_stride and status + 2 e; member 0
// writes the shared pts.
struct FitPools {
  const float* target[kSirenMaxMembers];
  const float* scale[kSirenMaxMembers];
  int scale_width;
};
hipError_t launch_fit_run_gather_members(int d_in, int d_out, int E, const float* pool_pts, const FitPools& pools,
                                         int64_t n_pool, const int64_t* idx, int64_t batch, float* pts, float* target,
                                         float* scale, size_t rows_stride, int* state, int64_t prev, float stop_loss,
                                         float* losses, int64_t losses_stride, int64_t* status, hipStream_t s);
hipError_t launch_fit_run_commit_members(int E, int* state, int64_t iter, float stop_loss, float* losses,
                                         int64_t losses_stride, int64_t* status, hipStream_t s);

}  // namespace wos
