// wos_siren.hip -- fused SIREN value, input Jacobian and divergence (wos_siren_eval).
//
// The reference's MLP with sine (src/2d/models/networks.py:25-68): Linear(d_in, H), sin(w .),
// L x [Linear(H, H), sin(w .)], Linear(H, d_out).  Forward mode: every point carries C = 1 + d_in
// columns through the net, its activation a and the tangents t_k = da/dx_k, so one pass gives
// u, J = du/dx and div u = trace J, and no activation leaves the chip.
//
// Layout.  A workgroup of 4 waves owns a tile of 32 points.  The tile's columns live in LDS as
// X[H][C * 32] (column s * 32 + j: carried column s of point j).  A hidden layer is Z = W X on
// v_mfma_f32_32x32x2_f32: wave w owns the row tiles r = w, w + 4 (32 output rows each) for all C
// column tiles, i.e. up to 2 x 4 accumulators of 16 registers.  Per k-step (two k values) the B
// operand of column tile c is one ds_read_b32, X[2 step + (lane >> 5)][32 c + (lane & 31)] -- the
// two wave halves read two rows, each 32 consecutive banks: conflict free -- and the A operand comes
// from the fragment-ordered copy of W that siren_pack_kernel writes once per call, 16 bytes per
// lane and four k-steps, prefetched one group ahead.  After a barrier (every wave has read X) the
// epilogue is lane-local: value and tangents of (row, point) sit in the same register of the same
// lane of the C accumulators.  The lane parks them at their own places in X and one rolled loop
// rereads them and writes the sin / cos products over them: one copy of the sin / cos code instead
// of 32 unrolled ones, and no dynamically indexed register array (no scratch).
//
// Arithmetic (f32, fixed order; DESIGN.md "Fused SIREN source"):
//   layer 0   z = fma(W0[r][d-1], x[d-1], ... fma(W0[r][0], x[0], b0[r]))
//   hidden    z = the MFMA's own chain over k = 0, 1, ..., H - 1 in that order, started from 0,
//             then the bias: fma(W[r][H-1], a[H-1], ... fma(W[r][0], a[0], 0)) + b[r]; the tangent
//             columns the same chain without the bias
//   both      wz = w * z, (s, c) = sincosf(wz), a = s, oc = w * c, t_k = oc * (W0[r][k] | Z_k)   (OCML; the
//             value-only kernel drops c)
//   output    u_i = (fma chain over h = 0 .. H - 1 started from 0) + b_out[i]; J[i][k] the chain alone
//   div       (J[0][0] + J[1][1]) + J[2][2]
// A point's columns never meet another point's, so its outputs do not depend on n, on its place
// in the batch or on which outputs were asked for (the value-only kernel carries one column and
// runs the same chains).
#include "wos_siren_device.h"

namespace wos {

// grid y: the member, whose copy lies blockIdx.y * member_stride floats into `packed`
__global__ __launch_bounds__(256) void siren_pack_kernel(const SirenNets nets, float* __restrict__ packed,
                                                        size_t member_stride) {
  const SirenNet& net = nets.v[blockIdx.y];
  packed += blockIdx.y * member_stride;
  const int H = net.H, Q = H >> 3;
  const size_t per = (size_t)H * H, total = per * net.L;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(idx / per);
    const int rem = (int)(idx - (size_t)l * per);
    const int e = rem & 3, lane = (rem >> 2) & 63, rq = rem >> 8;
    const int q = rq % Q, r = rq / Q;
    const int row = r * 32 + (lane & 31), k = 8 * q + 2 * e + (lane >> 5);
    packed[idx] = net.w[1 + l][(size_t)row * H + k];
  }
}

// D = d_in; TAN: carry the tangent columns (C = 1 + D) or the value alone (C = 1);
// RT: row tiles per wave, 1 for H <= 128, 2 above.
template <int D, bool TAN, int RT>
__global__ __launch_bounds__(256) void siren_eval_kernel(const SirenNet net, const float4* __restrict__ packed,
                                                        const float* __restrict__ pts, int64_t n,
                                                        float* __restrict__ u, float* __restrict__ jac,
                                                        float* __restrict__ div) {
  constexpr int C = TAN ? 1 + D : 1, cols = C * 32;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int H = net.H, L = net.L, DO = net.d_out;
  const float omega = net.omega;
  float* Xl = s_mem;              // [H][cols]
  float* Ol = s_mem + H * cols;   // [d_out][cols]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = tid & 31;
  const int64_t base = (int64_t)blockIdx.x * kSirenTile;

  {  // layer 0 on the VALU (K = d_in); a point past n computes on x = 0 and is never stored
    const int64_t p = base + j;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; k++) x[k] = p < n ? pts[p * D + k] : 0.0f;
    const float* W0 = net.w[0];
    const float* b0 = net.b[0];
    for (int row = tid >> 5; row < H; row += 8) {
      float w[D];
      float z = b0[row];
#pragma unroll
      for (int k = 0; k < D; k++) {
        w[k] = W0[row * D + k];
        z = fmaf(w[k], x[k], z);
      }
      const float wz = omega * z;
      float sn, cs;
      sincosf(wz, &sn, &cs);  // the value-only kernel too: the same sine by construction
      Xl[row * cols + j] = sn;
      if (TAN) {
        const float oc = omega * cs;
#pragma unroll
        for (int k = 0; k < D; k++) Xl[row * cols + (1 + k) * 32 + j] = oc * w[k];
      }
    }
  }
  __syncthreads();

  const int R = H >> 5, Q = H >> 3;
  for (int l = 0; l < L; l++) {
    f32x16 acc[RT][C];
    const bool busy = wave < R;  // wave-uniform: with H < 128 the waves past H / 32 own no row tile
    if (busy) siren_hidden_gemm<C, RT>(packed + (size_t)l * R * Q * 64, net.b[1 + l], Xl, H, wave, lane, acc);
    __syncthreads();  // every wave has read X: the layer is written back in place
    if (busy) {
      // the pre-activations go to their own places in X first (static register indices), then one
      // rolled loop turns them into sin / cos products: each lane rereads only what it wrote
#pragma unroll
      for (int i = 0; i < RT; i++) {
        const int r = wave + 4 * i;
        if (r < R) {
#pragma unroll
          for (int reg = 0; reg < 16; reg++) {
            float* xo = Xl + (r * 32 + siren_acc_row(reg, lane)) * cols + j;
#pragma unroll
            for (int c = 0; c < C; c++) xo[c * 32] = acc[i][c][reg];
          }
        }
      }
      for (int t = 0; t < RT * 16; t++) {
        const int r = wave + 4 * (t >> 4);
        if (r >= R) break;
        float* xo = Xl + (r * 32 + siren_acc_row(t & 15, lane)) * cols + j;
        const float wz = omega * xo[0];
        float sn, cs;
        sincosf(wz, &sn, &cs);
        xo[0] = sn;
        if (TAN) {
          const float oc = omega * cs;
#pragma unroll
          for (int c = 1; c < C; c++) xo[c * 32] = oc * xo[c * 32];
        }
      }
    }
    __syncthreads();
  }

  {  // output layer: d_out x cols dot products of length H, one per thread and pass
    const float* Wo = net.w[L + 1];
    const float* bo = net.b[L + 1];
    for (int item = tid; item < DO * cols; item += 256) {
      const int i = item / cols, col = item - i * cols;
      const float* wr = Wo + i * H;
      float s = 0.0f;
      for (int h = 0; h < H; h++) s = fmaf(wr[h], Xl[h * cols + col], s);
      Ol[item] = col < 32 ? s + bo[i] : s;
    }
  }
  __syncthreads();

  if (tid < 32) {
    const int64_t p = base + tid;
    if (p < n) {
      if (u)
        for (int i = 0; i < DO; i++) u[p * DO + i] = Ol[i * cols + tid];
      if (TAN) {
        if (jac)
          for (int i = 0; i < DO; i++)
#pragma unroll
            for (int k = 0; k < D; k++) jac[(p * DO + i) * D + k] = Ol[i * cols + (1 + k) * 32 + tid];
        if (div) {  // the host admits div only with d_out == d_in
          float dv = Ol[0 * cols + 1 * 32 + tid] + Ol[1 * cols + 2 * 32 + tid];
          if (D == 3) dv = dv + Ol[2 * cols + 3 * 32 + tid];
          div[p] = dv;
        }
      }
    }
  }
}

// wos_selftest_siren_layer: siren_hidden_gemm on caller-supplied columns, pre-activations out
template <int D, int RT>
__global__ __launch_bounds__(256) void siren_layer_selftest_kernel(int H, const float4* __restrict__ packed,
                                                                  const float* __restrict__ bias,
                                                                  const float* __restrict__ X, int64_t n,
                                                                  float* __restrict__ Z) {
  constexpr int C = 1 + D, cols = C * 32;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  float* Xl = s_mem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = tid & 31;
  const int64_t base = (int64_t)blockIdx.x * kSirenTile;
  for (int item = tid; item < H * cols; item += 256) {  // item = (point, column, h), h fastest as in X
    const int h = item % H, pc = item / H, c = pc % C, pj = pc / C;
    const int64_t p = base + pj;
    Xl[h * cols + c * 32 + pj] = p < n ? X[(p * C + c) * H + h] : 0.0f;
  }
  __syncthreads();
  const int R = H >> 5;
  if (wave >= R) return;
  f32x16 acc[RT][C];
  siren_hidden_gemm<C, RT>(packed, bias, Xl, H, wave, lane, acc);
  const int64_t p = base + j;
  if (p >= n) return;
#pragma unroll
  for (int i = 0; i < RT; i++) {
    const int r = wave + 4 * i;
    if (r < R) {
#pragma unroll
      for (int reg = 0; reg < 16; reg++)
#pragma unroll
        for (int c = 0; c < C; c++) Z[(p * C + c) * H + r * 32 + siren_acc_row(reg, lane)] = acc[i][c][reg];
    }
  }
}

hipError_t launch_siren_pack_members(const SirenNets& nets, int E, float* packed, size_t member_stride, hipStream_t s) {
  const size_t total = siren_pack_floats(nets.v[0].H, nets.v[0].L);
  if (total == 0) return hipSuccess;
  const unsigned grid = (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(siren_pack_kernel, dim3(grid, E), dim3(256), 0, s, nets, packed, member_stride);
  return hipGetLastError();
}

hipError_t launch_siren_pack(const SirenNet& net, float* packed, hipStream_t s) {
  SirenNets nets{};
  nets.v[0] = net;
  return launch_siren_pack_members(nets, 1, packed, 0, s);
}

template <int D, bool TAN, int RT>
static hipError_t siren_eval_launch(const SirenNet& net, const float* packed, const float* pts, int64_t n, float* u,
                                    float* jac, float* div, hipStream_t s) {
  constexpr int cols = (TAN ? 1 + D : 1) * 32;
  const size_t lds = (size_t)(net.H + net.d_out) * cols * sizeof(float);
  const int64_t grid = (n + kSirenTile - 1) / kSirenTile;
  hipLaunchKernelGGL((siren_eval_kernel<D, TAN, RT>), dim3((unsigned)grid), dim3(256), lds, s, net,
                     (const float4*)packed, pts, n, u, jac, div);
  return hipGetLastError();
}

hipError_t launch_siren_eval(const SirenNet& net, const float* packed, const float* pts, int64_t n, float* u,
                             float* jac, float* div, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if ((n + kSirenTile - 1) / kSirenTile > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  const bool tan = jac != nullptr || div != nullptr, two = net.H > 128;
  const int sel = (net.d_in == 3 ? 4 : 0) | (tan ? 2 : 0) | (two ? 1 : 0);
  switch (sel) {
    case 0: return siren_eval_launch<2, false, 1>(net, packed, pts, n, u, jac, div, s);
    case 1: return siren_eval_launch<2, false, 2>(net, packed, pts, n, u, jac, div, s);
    case 2: return siren_eval_launch<2, true, 1>(net, packed, pts, n, u, jac, div, s);
    case 3: return siren_eval_launch<2, true, 2>(net, packed, pts, n, u, jac, div, s);
    case 4: return siren_eval_launch<3, false, 1>(net, packed, pts, n, u, jac, div, s);
    case 5: return siren_eval_launch<3, false, 2>(net, packed, pts, n, u, jac, div, s);
    case 6: return siren_eval_launch<3, true, 1>(net, packed, pts, n, u, jac, div, s);
    default: return siren_eval_launch<3, true, 2>(net, packed, pts, n, u, jac, div, s);
  }
}

template <int D, int RT>
static hipError_t siren_layer_launch(int H, const float* packed, const float* b, const float* X, int64_t n, float* Z,
                                     hipStream_t s) {
  const size_t lds = (size_t)H * (1 + D) * 32 * sizeof(float);
  const int64_t grid = (n + kSirenTile - 1) / kSirenTile;
  hipLaunchKernelGGL((siren_layer_selftest_kernel<D, RT>), dim3((unsigned)grid), dim3(256), lds, s, H,
                     (const float4*)packed, b, X, n, Z);
  return hipGetLastError();
}

hipError_t launch_siren_layer_selftest(int H, int d_in, int64_t n, const float* W, const float* b, float* packed,
                                       const float* X, float* Z, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  SirenNet net{};
  net.d_in = d_in;
  net.H = H;
  net.L = 1;
  net.w[1] = W;
  hipError_t e = launch_siren_pack(net, packed, s);
  if (e != hipSuccess) return e;
  return launch_siren_layer_packed(H, d_in, n, packed, b, X, Z, s);
}

hipError_t launch_siren_layer_packed(int H, int d_in, int64_t n, const float* packed, const float* b, const float* X,
                                     float* Z, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (d_in == 2)
    return H > 128 ? siren_layer_launch<2, 2>(H, packed, b, X, n, Z, s) : siren_layer_launch<2, 1>(H, packed, b, X, n, Z, s);
  return H > 128 ? siren_layer_launch<3, 2>(H, packed, b, X, n, Z, s) : siren_layer_launch<3, 1>(H, packed, b, X, n, Z, s);
}

}  // namespace wos
