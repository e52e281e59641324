// wos_siren_train.hip -- the optimiser step of the velocity fits and the two small kernels that let
// K iterations of gather -> fit step -> Adam step run back to back on one stream (wos_adam_step,
// wos_siren_fit_run; DESIGN.md "Fused Adam step and the device-resident fit loop").
//
// Adam is torch's single-tensor form (lerp_, mul_().addcmul_(), sqrt() / bc2 + eps, addcdiv_) with
// amsgrad, weight decay and maximize off: f32, one operation per rounding (-ffp-contract=off), the
// five step scalars rounded once from double on the host.  clip_grad_norm_'s norm is one workgroup's
// sum in a fixed order, so the same call gives the same bits.  The gradients are read, never written.
//
// Every kernel here has a member axis (wos_siren_fit_run_ensemble; DESIGN.md "Ensemble fit loops"): a
// launch covers the E <= kSirenMaxMembers networks of an ensemble, each block working on its member's
// own tensors exactly as the single-network launch, E = 1, does.
#include "wos_siren.h"

namespace wos {

// S = sum g^2 over the flat order of the tensors: thread t chains acc = acc + g[e] * g[e] over
// e = t, t + 256, ... (the product rounded, then the sum), the 256 chains' sums pairwise (t, t + 128),
// (t, t + 64), ... -- siren_fit_loss_kernel's shape.  norm[0] = sqrtf(S).  One workgroup per member:
// its norm goes to norm[blockIdx.x * kFitStateWords].
__global__ __launch_bounds__(256) void adam_norm_kernel(const AdamMembers members, float* __restrict__ norm) {
  __shared__ float sm[256];
  const AdamSegs& segs = members.segs[blockIdx.x];
  norm += blockIdx.x * kFitStateWords;
  const int tid = threadIdx.x;
  float acc = 0.0f;
  for (int k = 0; k < segs.n; k++) {  // a thread's elements of tensor k follow its elements of tensor k - 1
    const int64_t begin = k == 0 ? 0 : segs.end[k - 1], count = segs.end[k] - begin;
    const float* __restrict__ g = segs.g[k];
    const int64_t first = (int64_t)((tid - begin) & 255);  // the least e - begin >= 0 with e = tid (mod 256)
#pragma unroll 8
    for (int64_t i = first; i < count; i += 256) {
      const float x = g[i];
      const float sq = x * x;
      acc = acc + sq;
    }
  }
  sm[tid] = acc;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) sm[tid] = sm[tid] + sm[tid + w];
    __syncthreads();
  }
  if (tid == 0) norm[0] = sqrtf(sm[0]);
}

// One launch over all tensors; element e of the flat order belongs to the tensor k with
// end[k - 1] <= e < end[k].  norm null: no clipping and no multiply.  stop non-null and set: a no-op.
// Grid y is the member: its tensors and moments from `members`, its norm and stop words
// blockIdx.y * kFitStateWords further on.
__global__ __launch_bounds__(256) void adam_update_kernel(const AdamMembers members, const AdamScalars sc,
                                                         const float* __restrict__ norm,
                                                         const int* __restrict__ stop) {
  const int member = blockIdx.y;
  const AdamSegs& segs = members.segs[member];
  float* __restrict__ m_all = members.exp_avg[member];
  float* __restrict__ v_all = members.exp_avg_sq[member];
  if (norm) norm += member * kFitStateWords;
  if (stop && stop[member * kFitStateWords] != 0) return;
  const int64_t total = segs.end[segs.n - 1];
  float c = 1.0f;
  if (norm) {
    const float den = norm[0] + 1e-6f;
    const float q = sc.max_norm / den;
    c = q >= 1.0f ? 1.0f : q;  // torch.clamp(max = 1): a NaN norm gives a NaN coefficient, and every element goes NaN
  }
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    int k = 0;
#pragma unroll
    for (int j = 0; j < kAdamMaxTensors - 1; j++) k += (j < segs.n - 1 && e >= segs.end[j]) ? 1 : 0;
    const int64_t at = e - (k == 0 ? 0 : segs.end[k - 1]);
    float g = segs.g[k][at];
    if (norm) g = g * c;
    const float m0 = m_all[e], v0 = v_all[e];
    const float dm = g - m0;
    const float wm = sc.omb1 * dm;
    const float m1 = m0 + wm;
    const float vb = v0 * sc.b2;
    const float og = sc.omb2 * g;
    const float ogg = og * g;
    const float v1 = vb + ogg;
    const float root = sqrtf(v1);
    const float rb = root / sc.bc2;
    const float den = rb + sc.eps;
    const float ratio = m1 / den;
    const float upd = sc.ss * ratio;
    float* p = segs.p[k] + at;
    p[0] = p[0] - upd;
    m_all[e] = m1;
    v_all[e] = v1;
  }
}

// The previous iteration's book-keeping, in stream order after its Adam step: unless the run has
// stopped, its loss is published, it counts as applied, and the run stops from here on when the
// loss is at or below stop_loss (stop_loss < 0: never).  state: [0] the sticky stop flag, [1] the
// fit step's loss.
__device__ __forceinline__ void fit_run_commit(int* state, int64_t iter, float stop_loss, float* losses,
                                               long long* status) {
  if (state[0] != 0) return;
  const float loss = __int_as_float(state[1]);
  losses[iter] = loss;
  status[0] = iter + 1;
  if (stop_loss >= 0.0f && loss <= stop_loss) state[0] = 1;
}

// thread e commits member e: its state words, its row of losses and its status pair
__global__ void fit_run_commit_kernel(int n_members, int* state, int64_t iter, float stop_loss, float* losses,
                                      int64_t losses_stride, long long* status) {
  const int e = threadIdx.x;
  if (blockIdx.x == 0 && e < n_members)
    fit_run_commit(state + e * kFitStateWords, iter, stop_loss, losses + e * losses_stride, status + 2 * e);
}

// Rows idx[j] of the pool into the batch buffers; an index outside [0, n_pool) is clamped and
// counted in status[1].  Thread 0 also commits iteration `prev` (prev < 0: nothing to commit).
// Grid y is the member: it gathers its own pool's target and scale into target / scale +
// member * rows_stride and commits its own state, losses and status; the points are shared, and
// member 0 writes them.
template <int D>
__global__ __launch_bounds__(256) void fit_run_gather_kernel(const float* __restrict__ pool_pts, const FitPools pools,
                                                            int64_t n_pool, const long long* __restrict__ idx,
                                                            int64_t batch, int d_out, float* __restrict__ pts,
                                                            float* __restrict__ target, float* __restrict__ scale,
                                                            size_t rows_stride, int* state, int64_t prev,
                                                            float stop_loss, float* losses, int64_t losses_stride,
                                                            long long* status) {
  const int member = blockIdx.y;
  const float* __restrict__ pool_target = pools.target[member];
  const float* __restrict__ pool_scale = pools.scale[member];
  target += member * rows_stride;
  scale += member * rows_stride;
  status += 2 * member;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j == 0 && prev >= 0)
    fit_run_commit(state + member * kFitStateWords, prev, stop_loss, losses + member * losses_stride, status);
  if (j >= batch) return;
  long long r = idx[j];
  if (r < 0 || r >= n_pool) {
    atomicAdd((unsigned long long*)&status[1], 1ull);
    r = r < 0 ? 0 : n_pool - 1;
  }
  if (member == 0) {
#pragma unroll
    for (int k = 0; k < D; k++) pts[j * D + k] = pool_pts[r * D + k];
  }
  for (int i = 0; i < d_out; i++) target[j * d_out + i] = pool_target[r * d_out + i];
  if (pool_scale) {
    const int sw = pools.scale_width ? pools.scale_width : d_out;  // a factor per component, or a matrix per point
    for (int i = 0; i < sw; i++) scale[j * sw + i] = pool_scale[r * sw + i];
  }
}

hipError_t launch_adam_norm_members(const AdamMembers& m, int E, float* norm, hipStream_t s) {
  hipLaunchKernelGGL(adam_norm_kernel, dim3(E), dim3(256), 0, s, m, norm);
  return hipGetLastError();
}

hipError_t launch_adam_update_members(const AdamMembers& m, int E, const AdamScalars& sc, const float* norm,
                                      const int* stop, hipStream_t s) {
  const AdamSegs& segs = m.segs[0];  // every member's tensors have member 0's counts
  const int64_t total = segs.end[segs.n - 1], blocks = (total + 255) / 256;
  const unsigned grid = (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));  // grid-stride past 2^28 elements
  hipLaunchKernelGGL(adam_update_kernel, dim3(grid, E), dim3(256), 0, s, m, sc, norm, stop);
  return hipGetLastError();
}

hipError_t launch_adam_norm(const AdamSegs& segs, float* norm, hipStream_t s) {
  AdamMembers m{};
  m.segs[0] = segs;
  return launch_adam_norm_members(m, 1, norm, s);
}

hipError_t launch_adam_update(const AdamSegs& segs, float* exp_avg, float* exp_avg_sq, const AdamScalars& sc,
                              const float* norm, const int* stop, hipStream_t s) {
  AdamMembers m{};
  m.segs[0] = segs;
  m.exp_avg[0] = exp_avg;
  m.exp_avg_sq[0] = exp_avg_sq;
  return launch_adam_update_members(m, 1, sc, norm, stop, s);
}

hipError_t launch_fit_run_gather_members(int d_in, int d_out, int E, const float* pool_pts, const FitPools& pools,
                                         int64_t n_pool, const int64_t* idx, int64_t batch, float* pts, float* target,
                                         float* scale, size_t rows_stride, int* state, int64_t prev, float stop_loss,
                                         float* losses, int64_t losses_stride, int64_t* status, hipStream_t s) {
  const dim3 grid((unsigned)((batch + 255) / 256), E);
  if (d_in == 2)
    hipLaunchKernelGGL(fit_run_gather_kernel<2>, grid, dim3(256), 0, s, pool_pts, pools, n_pool, (const long long*)idx,
                       batch, d_out, pts, target, scale, rows_stride, state, prev, stop_loss, losses, losses_stride,
                       (long long*)status);
  else
    hipLaunchKernelGGL(fit_run_gather_kernel<3>, grid, dim3(256), 0, s, pool_pts, pools, n_pool, (const long long*)idx,
                       batch, d_out, pts, target, scale, rows_stride, state, prev, stop_loss, losses, losses_stride,
                       (long long*)status);
  return hipGetLastError();
}

hipError_t launch_fit_run_gather(int d_in, int d_out, const float* pool_pts, const float* pool_target,
                                 const float* pool_scale, int scale_width, int64_t n_pool, const int64_t* idx,
                                 int64_t batch, float* pts, float* target, float* scale, int* state, int64_t prev,
                                 float stop_loss, float* losses, int64_t* status, hipStream_t s) {
  FitPools pools{};
  pools.target[0] = pool_target;
  pools.scale[0] = pool_scale;
  pools.scale_width = scale_width;
  return launch_fit_run_gather_members(d_in, d_out, 1, pool_pts, pools, n_pool, idx, batch, pts, target, scale, 0, state, prev,
                                       stop_loss, losses, 0, status, s);
}

hipError_t launch_fit_run_commit_members(int E, int* state, int64_t iter, float stop_loss, float* losses,
                                         int64_t losses_stride, int64_t* status, hipStream_t s) {
  hipLaunchKernelGGL(fit_run_commit_kernel, dim3(1), dim3(64), 0, s, E, state, iter, stop_loss, losses, losses_stride,
                     (long long*)status);
  return hipGetLastError();
}

hipError_t launch_fit_run_commit(int* state, int64_t iter, float stop_loss, float* losses, int64_t* status,
                                 hipStream_t s) {
  return launch_fit_run_commit_members(1, state, iter, stop_loss, losses, 0, status, s);
}

}  // namespace wos
