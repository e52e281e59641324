// wos_siren_vjp.hip -- fused SIREN backward (wos_siren_vjp): the vector-Jacobian product of the
// network's value u, input Jacobian J and divergence with respect to every weight and bias.
//
// Contract (DESIGN.md "Fused SIREN backward").  With the forward's columns per point -- in sine layer
// l the pre-activations z, Z_k, (s, c) = sincosf(w z), a = s, t_k = w c Z_k -- and the seeds
// ub = g_u, Jb[i][k] = g_J[i][k] + g_div [i == k]:
//   output   dWo[i][h] = sum_p (ub_i a[h] + sum_k Jb_ik t_k[h]),  dbo = sum_p ub,
//            da = Wo^T ub,  dt_k = Wo^T Jb[:, k]
//   sine     dZ_k = w c dt_k,  dz = w c da - w^2 s sum_k dt_k Z_k
//   hidden   dW = sum_p (dz a_prev^T + sum_k dZ_k t_prev,k^T),  db = sum_p dz,
//            da_prev = W^T dz,  dt_prev,k = W^T dZ_k
//   layer 0  dW0[r][k] = sum_p (dz[r] x_k + dZ_k[r]),  db0 = sum_p dz
//
// Layout.  The points go in chunks of whole 32-point tiles whose stash fits the workspace.  Per
// chunk, siren_vjp_tile_kernel (the forward's workgroup: 4 waves, one tile, X[H][C * 32] in LDS)
// re-runs the forward with the forward's own code and stores every layer's pre-activation columns
// to the stash, then sweeps back: it reloads a layer's z, Z_k, repeats sincosf on the same bits,
// forms dz, dZ_k in place in LDS, stores them for the weight-gradient kernel, overwrites the
// stashed pre-activations with the layer's outputs a, t_k (the other operand of the next layer's
// weight gradient) and takes dX_prev = W^T dZ with siren_hidden_gemm on the transposed
// fragment-ordered copy of W.  The output layer and layer 0 are VALU code like their forward twins
// and leave per-tile partials, as do the bias gradients.  siren_wgrad_kernel then forms
// dW_l = dZ_l X_{l-1}^T on v_mfma_f32_32x32x2_f32, one 128 x 128 output tile and one K slice of 16
// column blocks per workgroup, and siren_reduce_kernel adds the slices' and the tiles' partials in
// a fixed blocked order, chunk after chunk.  No atomics: the same n and chunk size give the same bits.
//
// A point past n has zero seeds, so every dz, dZ_k of its column is a zero (its forward columns,
// computed on x = 0, are finite); the weight-gradient kernel masks those columns on load as well.
#include "wos_siren_device.h"

namespace wos {

// grid y: the member, as in siren_pack_kernel
__global__ __launch_bounds__(256) void siren_pack_transposed_kernel(const SirenNets nets, float* __restrict__ packed,
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
    packed[idx] = net.w[1 + l][(size_t)k * H + row];
  }
}

// xs: [L + 1][T][H][cols], ds: [L][T][H][cols] (layer_stride = T H cols); part: [tile][P]:
// dWo [d_out][H] | dbo [d_out] | db_0 .. db_L [H] each | dW0 [H][D]
template <int D, int RT>
__global__ __launch_bounds__(256) void siren_vjp_tile_kernel(const SirenNet net, const float4* __restrict__ packed,
                                                            const float4* __restrict__ packedT,
                                                            const float* __restrict__ zeros,
                                                            const float* __restrict__ pts, int64_t n,
                                                            const float* __restrict__ g_u,
                                                            const float* __restrict__ g_jac,
                                                            const float* __restrict__ g_div, float* __restrict__ xs,
                                                            float* __restrict__ ds, size_t layer_stride,
                                                            float* __restrict__ tile_part, int P) {
  constexpr int C = 1 + D, cols = C * 32;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int H = net.H, L = net.L, DO = net.d_out;
  const float omega = net.omega;
  float* Xl = s_mem;                  // [H][cols]
  float* Sl = s_mem + H * cols;       // [3][cols]: the seeds ub | Jb[:, 0] | ... per output row
  float* Pl = Sl + 3 * cols;          // [D][32]: the tile's points
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = tid & 31;
  const int64_t base = (int64_t)blockIdx.x * kSirenTile;
  const size_t tile_off = (size_t)blockIdx.x * H * cols;
  float* part = tile_part + (size_t)blockIdx.x * P;

  for (int item = tid; item < 3 * cols; item += 256) {  // seeds; a point past n contributes nothing
    const int i = item / cols, col = item - i * cols, s = col >> 5;
    const int64_t p = base + (col & 31);
    float v = 0.0f;
    if (p < n && i < DO) {
      if (s == 0) {
        if (g_u) v = g_u[p * DO + i];
      } else {
        if (g_jac) v = g_jac[(p * DO + i) * D + (s - 1)];
        if (g_div && i == s - 1) v = v + g_div[p];
      }
    }
    Sl[item] = v;
  }

  {  // layer 0, the forward's code; the pre-activation columns go to the stash
    const int64_t p = base + j;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; k++) x[k] = p < n ? pts[p * D + k] : 0.0f;
    if (tid < 32) {
#pragma unroll
      for (int k = 0; k < D; k++) Pl[k * 32 + j] = x[k];
    }
    const float* W0 = net.w[0];
    const float* b0 = net.b[0];
    float* zs = xs + tile_off;
    for (int row = tid >> 5; row < H; row += 8) {
      float w[D];
      float z = b0[row];
#pragma unroll
      for (int k = 0; k < D; k++) {
        w[k] = W0[row * D + k];
        z = fmaf(w[k], x[k], z);
      }
      zs[row * cols + j] = z;
      const float wz = omega * z;
      float sn, cs;
      sincosf(wz, &sn, &cs);
      Xl[row * cols + j] = sn;
      const float oc = omega * cs;
#pragma unroll
      for (int k = 0; k < D; k++) {
        zs[row * cols + (1 + k) * 32 + j] = w[k];
        Xl[row * cols + (1 + k) * 32 + j] = oc * w[k];
      }
    }
  }
  __syncthreads();

  const int R = H >> 5, Q = H >> 3;
  const bool busy = wave < R;  // wave-uniform: with H < 128 the waves past H / 32 own no row tile
  for (int l = 0; l < L; l++) {
    f32x16 acc[RT][C];
    if (busy) siren_hidden_gemm<C, RT>(packed + (size_t)l * R * Q * 64, net.b[1 + l], Xl, H, wave, lane, acc);
    __syncthreads();
    if (busy) {
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
      float* zs = xs + (size_t)(l + 1) * layer_stride + tile_off;
      for (int t = 0; t < RT * 16; t++) {
        const int r = wave + 4 * (t >> 4);
        if (r >= R) break;
        const int row = r * 32 + siren_acc_row(t & 15, lane);
        float* xo = Xl + row * cols + j;
        float* zo = zs + row * cols + j;
        const float z = xo[0];
        zo[0] = z;
        const float wz = omega * z;
        float sn, cs;
        sincosf(wz, &sn, &cs);
        xo[0] = sn;
        const float oc = omega * cs;
#pragma unroll
        for (int c = 1; c < C; c++) {
          const float zk = xo[c * 32];
          zo[c * 32] = zk;
          xo[c * 32] = oc * zk;
        }
      }
    }
    __syncthreads();
  }

  {  // output layer: dWo and dbo of this tile.  Row h starts its sum at column h mod cols, so that
     // the threads of a wave half read 32 different banks; the order is fixed all the same.
    for (int h = tid; h < H; h += 256) {
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
      int col = h % cols;
      for (int t = 0; t < cols; t++) {
        const float xv = Xl[h * cols + col];
        s0 = fmaf(Sl[col], xv, s0);
        s1 = fmaf(Sl[cols + col], xv, s1);
        s2 = fmaf(Sl[2 * cols + col], xv, s2);
        col = col + 1 == cols ? 0 : col + 1;
      }
      part[h] = s0;
      if (DO > 1) part[H + h] = s1;
      if (DO > 2) part[2 * H + h] = s2;
    }
    if (tid < DO) {
      float v[32];  // a plain sum of the cotangents: pairwise, (p, p + 16), then (p, p + 8), ...
#pragma unroll
      for (int t = 0; t < 32; t++) v[t] = Sl[tid * cols + t];
#pragma unroll
      for (int w = 16; w >= 1; w >>= 1)
#pragma unroll
        for (int t = 0; t < w; t++) v[t] = v[t] + v[t + w];
      part[DO * H + tid] = v[0];
    }
  }
  __syncthreads();
  {  // (da, dt_k) of the last sine layer = Wo^T seeds, over X
    const float* Wo = net.w[L + 1];
    for (int item = tid; item < H * cols; item += 256) {
      const int h = item / cols, col = item - h * cols;
      float v = Wo[h] * Sl[col];
      if (DO > 1) v = fmaf(Wo[H + h], Sl[cols + col], v);
      if (DO > 2) v = fmaf(Wo[2 * H + h], Sl[2 * cols + col], v);
      Xl[item] = v;
    }
  }
  __syncthreads();

  float* part_b = part + DO * H + DO;
  float* part_w0 = part_b + (L + 1) * H;
  const float om2 = omega * omega;
  for (int l = L; l >= 0; l--) {
    float* zs = xs + (size_t)l * layer_stride + tile_off;
    float* dst = l >= 1 ? ds + (size_t)(l - 1) * layer_stride + tile_off : nullptr;
    for (int item = tid; item < H * 32; item += 256) {  // (row, point): the point is tid & 31 throughout
      const int row = item >> 5;
      float* xo = Xl + row * cols + j;
      float* zo = zs + row * cols + j;
      const float wz = omega * zo[0];
      float sn, cs;
      sincosf(wz, &sn, &cs);
      const float oc = omega * cs;
      float zk[D], dt[D];
      float dot = 0.0f;
#pragma unroll
      for (int k = 0; k < D; k++) {
        zk[k] = zo[(1 + k) * 32];
        dt[k] = xo[(1 + k) * 32];
        dot = fmaf(dt[k], zk[k], dot);
      }
      const float dz = oc * xo[0] - (om2 * sn) * dot;
      xo[0] = dz;
      if (dst) dst[row * cols + j] = dz;
      if (l < L) zo[0] = sn;
#pragma unroll
      for (int k = 0; k < D; k++) {
        const float dzk = oc * dt[k];
        xo[(1 + k) * 32] = dzk;
        if (dst) dst[row * cols + (1 + k) * 32 + j] = dzk;
        if (l < L) zo[(1 + k) * 32] = oc * zk[k];
      }
    }
    __syncthreads();
    for (int r = tid; r < H; r += 256) {  // db_l, and dW0 at layer 0: sums over the tile's points
      float sb = 0.0f, sw[D];
#pragma unroll
      for (int k = 0; k < D; k++) sw[k] = 0.0f;
      for (int t = 0; t < 32; t++) {
        const int jj = (t + r) & 31;
        const float dz = Xl[r * cols + jj];
        sb = sb + dz;
        if (l == 0) {
#pragma unroll
          for (int k = 0; k < D; k++) sw[k] = sw[k] + fmaf(dz, Pl[k * 32 + jj], Xl[r * cols + (1 + k) * 32 + jj]);
        }
      }
      part_b[l * H + r] = sb;
      if (l == 0) {
#pragma unroll
        for (int k = 0; k < D; k++) part_w0[r * D + k] = sw[k];
      }
    }
    if (l == 0) break;
    f32x16 acc[RT][C];
    if (busy) siren_hidden_gemm<C, RT>(packedT + (size_t)(l - 1) * R * Q * 64, zeros, Xl, H, wave, lane, acc);
    __syncthreads();  // every wave has read dZ, and the partial sums above are done
    if (busy) {
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
    }
    __syncthreads();
  }
}

// dW = A B^T over K: A = ds + z * layer_stride, B = xs + z * layer_stride, both [T][H][cols] with
// K = (tile, column).  Workgroup (x: output tile of 128 x 128, y: slice of kSirenWgradSliceBlocks
// 32-column blocks, z: layer, and above it the member, whose ds, xs and part lie member_stride apart); wave (wr, wc) owns 64 x 64 of it as 2 x 2 MFMA tiles.  A block of
// K is staged in LDS as [128][33]: stored along K (32 banks a row), read down the rows at stride
// 33 (32 banks again).  Columns of points past n_valid are read as zero.
constexpr int kWgradTile = 128, kWgradPitch = 33;

__global__ __launch_bounds__(256) void siren_wgrad_kernel(const float* __restrict__ ds, const float* __restrict__ xs,
                                                         size_t layer_stride, int H, int C, int n_kb, int64_t n_valid,
                                                         float* __restrict__ part, int L, size_t member_stride) {
  __shared__ float As[kWgradTile * kWgradPitch];
  __shared__ float Bs[kWgradTile * kWgradPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = tid & 31, half = lane >> 5;
  const int TB = (H + kWgradTile - 1) / kWgradTile;
  const int tr = blockIdx.x / TB, tc = blockIdx.x - tr * TB;
  const int member = blockIdx.z / L, lz = blockIdx.z - member * L, cols = C * 32;  // grid z = member * L + layer
  const float* A = ds + member * member_stride + (size_t)lz * layer_stride;
  const float* B = xs + member * member_stride + (size_t)lz * layer_stride;
  const int wr = wave >> 1, wc = wave & 1;
  const int row0 = tr * kWgradTile + 64 * wr, col0 = tc * kWgradTile + 64 * wc;
  const bool busy = row0 < H && col0 < H;  // wave-uniform
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int reg = 0; reg < 16; reg++) acc[a][b][reg] = 0.0f;
  const int kb0 = blockIdx.y * kSirenWgradSliceBlocks, kb1 = min(n_kb, kb0 + kSirenWgradSliceBlocks);
  // a thread stages rows (tid >> 5) + 8 i of both operands; the next block's loads fly during the MFMAs
  float ra[16], rb[16];
  const auto fetch = [&](int kb) {
    const int t = kb / C, s = kb - t * C;
    const bool live = (int64_t)t * kSirenTile + j < n_valid;
    const size_t off = (size_t)t * H * cols + s * 32 + j;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int r = (tid >> 5) + 8 * i;
      const int ha = tr * kWgradTile + r, hb = tc * kWgradTile + r;
      ra[i] = live && ha < H ? A[off + (size_t)ha * cols] : 0.0f;
      rb[i] = hb < H ? B[off + (size_t)hb * cols] : 0.0f;
    }
  };
  if (kb0 < kb1) fetch(kb0);
  for (int kb = kb0; kb < kb1; kb++) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int r = (tid >> 5) + 8 * i;
      As[r * kWgradPitch + j] = ra[i];
      Bs[r * kWgradPitch + j] = rb[i];
    }
    __syncthreads();
    if (kb + 1 < kb1) fetch(kb + 1);
    if (busy) {
      const float* ap = As + (64 * wr + (lane & 31)) * kWgradPitch + half;
      const float* bp = Bs + (64 * wc + (lane & 31)) * kWgradPitch + half;
#pragma unroll 4
      for (int ks = 0; ks < 16; ks++) {
        const float a0 = ap[2 * ks], a1 = ap[32 * kWgradPitch + 2 * ks];
        const float b0 = bp[2 * ks], b1 = bp[32 * kWgradPitch + 2 * ks];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!busy) return;
  float* out = part + member * member_stride + ((size_t)blockIdx.y * L + lz) * H * H;
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const int col = col0 + 32 * b + (lane & 31);
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int row = row0 + 32 * a + siren_acc_row(reg, lane);
        if (row < H && col < H) out[(size_t)row * H + col] = acc[a][b][reg];
      }
    }
}

// dst(e) = (accumulate ? dst(e) : 0) + sum over i < n_part of part[i * stride + e].  Eight threads
// per element: thread y adds the partials i = y, y + 8, ... as a chain, then thread 0 adds the
// eight chains' sums in the order y = 0 .. 7.  The order depends on n_part alone.
__global__ __launch_bounds__(256) void siren_reduce_kernel(const float* __restrict__ part, int n_part, size_t stride,
                                                          const SirenReduceSegs segs, int count, int accumulate,
                                                          size_t part_member_stride, size_t dst_member_stride) {
  __shared__ float sm[8][33];
  part += blockIdx.y * part_member_stride;  // grid y: the member
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + tx;
  float s = 0.0f;
  if (e < count)
    for (int i = ty; i < n_part; i += 8) s = s + part[(size_t)i * stride + e];
  sm[ty][tx] = s;
  __syncthreads();
  if (ty != 0 || e >= count) return;
  float total = 0.0f;
#pragma unroll
  for (int y = 0; y < 8; y++) total = total + sm[y][tx];
  float* out = nullptr;
#pragma unroll
  for (int k = 0; k < kReduceSegs; k++) {
    const int begin = k == 0 ? 0 : segs.end[k - 1];
    if (k < segs.n && e >= begin && e < segs.end[k]) out = segs.dst[k] + blockIdx.y * dst_member_stride + (e - begin);
  }
  if (out) *out = accumulate ? *out + total : total;
}

// self-test: src [n][C][H] -> the stash image [T][H][cols]; columns past n are filled with ones, so
// the weight-gradient kernel's own masking is what keeps them out
__global__ __launch_bounds__(256) void siren_vjp_image_kernel(const float* __restrict__ src, int64_t n, int H, int C,
                                                             size_t total, float* __restrict__ img) {
  const int cols = C * 32;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int col = (int)(idx % cols);
    const size_t th = idx / cols;
    const int h = (int)(th % H);
    const int64_t p = (int64_t)(th / H) * kSirenTile + (col & 31);
    img[idx] = p < n ? src[((size_t)p * C + (col >> 5)) * H + h] : 1.0f;
  }
}

size_t siren_vjp_tile_lds_bytes(int d_in, int H) { return ((size_t)(H + 3) * (1 + d_in) * 32 + d_in * 32) * sizeof(float); }

hipError_t launch_siren_pack_transposed_members(const SirenNets& nets, int E, float* packedT, size_t member_stride,
                                                hipStream_t s) {
  const size_t total = siren_pack_floats(nets.v[0].H, nets.v[0].L);
  if (total == 0) return hipSuccess;
  const unsigned grid = (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(siren_pack_transposed_kernel, dim3(grid, E), dim3(256), 0, s, nets, packedT, member_stride);
  return hipGetLastError();
}

hipError_t launch_siren_pack_transposed(const SirenNet& net, float* packedT, hipStream_t s) {
  SirenNets nets{};
  nets.v[0] = net;
  return launch_siren_pack_transposed_members(nets, 1, packedT, 0, s);
}

SirenVjpPlan siren_vjp_plan(const SirenNet& net, int64_t n, size_t stash_cap_bytes, int resident_tiles) {
  SirenVjpPlan p{};
  const int C = 1 + net.d_in;
  const size_t per_tile = siren_vjp_stash_floats_per_tile(net.d_in, net.H, net.L);
  const int64_t tiles_all = (n + kSirenTile - 1) / kSirenTile;
  int64_t fit = (int64_t)(stash_cap_bytes / (per_tile * sizeof(float)));
  fit = fit < (1 << 20) ? fit : (1 << 20);  // T C and every launch's grid stay far inside an int
  p.tiles = (int)(tiles_all < fit ? tiles_all : fit);
  if (p.tiles < 1) return p;
  if (resident_tiles > 0 && p.tiles < tiles_all && p.tiles > resident_tiles)
    p.tiles -= p.tiles % resident_tiles;  // several chunks: each a whole number of rounds of resident workgroups
  p.slices = net.L > 0 ? (p.tiles * C + kSirenWgradSliceBlocks - 1) / kSirenWgradSliceBlocks : 0;
  p.stash = per_tile * p.tiles;
  p.tile_part = siren_vjp_tile_part_floats(net) * p.tiles;
  p.slice_part = (size_t)p.slices * net.L * net.H * net.H;
  return p;
}

hipError_t siren_reduce_members(const float* part, int n_part, size_t stride, const SirenReduceSegs& segs, bool accumulate,
                                int E, size_t part_member_stride, size_t dst_member_stride, hipStream_t s) {
  const int count = segs.end[segs.n - 1];
  hipLaunchKernelGGL(siren_reduce_kernel, dim3((unsigned)((count + 31) / 32), E), dim3(256), 0, s, part, n_part, stride,
                     segs, count, accumulate ? 1 : 0, part_member_stride, dst_member_stride);
  return hipGetLastError();
}

hipError_t siren_reduce(const float* part, int n_part, size_t stride, const SirenReduceSegs& segs, bool accumulate,
                        hipStream_t s) {
  return siren_reduce_members(part, n_part, stride, segs, accumulate, 1, 0, 0, s);
}

hipError_t siren_wgrad_members(const float* ds, const float* xs, size_t layer_stride, int H, int C, int tiles,
                               int64_t n_valid, float* part, int L, int E, size_t member_stride, hipStream_t s) {
  const int TB = (H + kWgradTile - 1) / kWgradTile, n_kb = tiles * C;
  const int slices = (n_kb + kSirenWgradSliceBlocks - 1) / kSirenWgradSliceBlocks;
  hipLaunchKernelGGL(siren_wgrad_kernel, dim3(TB * TB, slices, L * E), dim3(256), 0, s, ds, xs, layer_stride, H, C, n_kb,
                     n_valid, part, L, member_stride);
  return hipGetLastError();
}

hipError_t siren_wgrad(const float* ds, const float* xs, size_t layer_stride, int H, int C, int tiles, int64_t n_valid,
                       float* part, int L, hipStream_t s) {
  return siren_wgrad_members(ds, xs, layer_stride, H, C, tiles, n_valid, part, L, 1, 0, s);
}

template <int D, int RT>
static hipError_t siren_vjp_tile_launch(const SirenNet& net, const float* packed, const float* packedT,
                                        const float* zeros, const float* pts, int64_t n, const float* g_u,
                                        const float* g_jac, const float* g_div, float* xs, float* ds,
                                        size_t layer_stride, float* tile_part, int P, hipStream_t s) {
  const size_t lds = siren_vjp_tile_lds_bytes(D, net.H);
  const int64_t grid = (n + kSirenTile - 1) / kSirenTile;
  hipLaunchKernelGGL((siren_vjp_tile_kernel<D, RT>), dim3((unsigned)grid), dim3(256), lds, s, net,
                     (const float4*)packed, (const float4*)packedT, zeros, pts, n, g_u, g_jac, g_div, xs, ds,
                     layer_stride, tile_part, P);
  return hipGetLastError();
}

hipError_t launch_siren_vjp(const SirenNet& net, const float* packed, const float* packedT, const float* zeros,
                            const float* pts, int64_t n, const float* g_u, const float* g_jac, const float* g_div,
                            const SirenGrads& grads, const SirenVjpPlan& plan, float* work, hipStream_t s) {
  const int D = net.d_in, DO = net.d_out, H = net.H, L = net.L, C = 1 + D, cols = C * 32;
  hipError_t e;
  if (n <= 0) {  // an empty sum: zeros
    for (int l = 0; l < L + 2; l++) {
      const size_t nb = l == L + 1 ? (size_t)DO : (size_t)H, nw = nb * (l == 0 ? (size_t)D : (size_t)H);
      if ((e = hipMemsetAsync(grads.w[l], 0, nw * sizeof(float), s)) != hipSuccess) return e;
      if ((e = hipMemsetAsync(grads.b[l], 0, nb * sizeof(float), s)) != hipSuccess) return e;
    }
    return hipSuccess;
  }
  if (plan.tiles < 1) return hipErrorInvalidValue;
  const int T = plan.tiles, P = (int)siren_vjp_tile_part_floats(net);
  const size_t layer_stride = (size_t)T * H * cols;
  float* xs = work;
  float* ds = xs + (size_t)(L + 1) * layer_stride;
  float* tile_part = work + plan.stash;
  float* slice_part = tile_part + plan.tile_part;
  const int64_t per_chunk = (int64_t)T * kSirenTile;
  // the tiles' partials in the order of the tile kernel's layout, and the slices' by layer
  SirenReduceSegs tile_segs{}, slice_segs{};
  const auto seg = [](SirenReduceSegs& g, float* dst, int count) {
    g.end[g.n] = (g.n ? g.end[g.n - 1] : 0) + count;
    g.dst[g.n++] = dst;
  };
  seg(tile_segs, grads.w[L + 1], DO * H);
  seg(tile_segs, grads.b[L + 1], DO);
  for (int l = 0; l <= L; l++) seg(tile_segs, grads.b[l], H);
  seg(tile_segs, grads.w[0], H * D);
  for (int l = 0; l < L; l++) seg(slice_segs, grads.w[1 + l], H * H);
  for (int64_t base = 0; base < n; base += per_chunk) {
    const int64_t nc = n - base < per_chunk ? n - base : per_chunk;
    const int tiles = (int)((nc + kSirenTile - 1) / kSirenTile);
    const bool acc = base > 0;
    const float* cp = pts + base * D;
    const float* cu = g_u ? g_u + base * DO : nullptr;
    const float* cj = g_jac ? g_jac + base * DO * D : nullptr;
    const float* cd = g_div ? g_div + base : nullptr;
    if (D == 2)
      e = H > 128 ? siren_vjp_tile_launch<2, 2>(net, packed, packedT, zeros, cp, nc, cu, cj, cd, xs, ds, layer_stride, tile_part, P, s)
                  : siren_vjp_tile_launch<2, 1>(net, packed, packedT, zeros, cp, nc, cu, cj, cd, xs, ds, layer_stride, tile_part, P, s);
    else
      e = H > 128 ? siren_vjp_tile_launch<3, 2>(net, packed, packedT, zeros, cp, nc, cu, cj, cd, xs, ds, layer_stride, tile_part, P, s)
                  : siren_vjp_tile_launch<3, 1>(net, packed, packedT, zeros, cp, nc, cu, cj, cd, xs, ds, layer_stride, tile_part, P, s);
    if (e != hipSuccess) return e;
    if ((e = siren_reduce(tile_part, tiles, P, tile_segs, acc, s)) != hipSuccess) return e;
    if (L > 0) {
      if ((e = siren_wgrad(ds, xs, layer_stride, H, C, tiles, nc, slice_part, L, s)) != hipSuccess) return e;
      const int slices = (tiles * C + kSirenWgradSliceBlocks - 1) / kSirenWgradSliceBlocks;
      if ((e = siren_reduce(slice_part, slices, (size_t)L * H * H, slice_segs, acc, s)) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

size_t siren_vjp_layer_selftest_floats(int H, int d_in, int64_t n) {
  const size_t tiles = (size_t)((n + kSirenTile - 1) / kSirenTile), C = 1 + d_in;
  const size_t slices = (tiles * C + kSirenWgradSliceBlocks - 1) / kSirenWgradSliceBlocks;
  return 2 * tiles * H * C * 32 + slices * H * H;
}

hipError_t launch_siren_vjp_layer_selftest(int H, int d_in, int64_t n, const float* W, float* packedT, const float* zeros,
                                           const float* dZ, const float* X, float* dX, float* dW, float* work,
                                           hipStream_t s) {
  if (n <= 0) return hipSuccess;
  SirenNet net{};
  net.d_in = d_in;
  net.H = H;
  net.L = 1;
  net.w[1] = W;
  hipError_t e = launch_siren_pack_transposed(net, packedT, s);
  if (e != hipSuccess) return e;
  if ((e = launch_siren_layer_packed(H, d_in, n, packedT, zeros, dZ, dX, s)) != hipSuccess) return e;
  const int C = 1 + d_in, tiles = (int)((n + kSirenTile - 1) / kSirenTile);
  const size_t image = (size_t)tiles * H * C * 32;
  float* a_img = work;
  float* b_img = work + image;
  float* part = b_img + image;
  const unsigned grid = (unsigned)((image + 255) / 256 < 4096 ? (image + 255) / 256 : 4096);
  hipLaunchKernelGGL(siren_vjp_image_kernel, dim3(grid), dim3(256), 0, s, dZ, n, H, C, image, a_img);
  hipLaunchKernelGGL(siren_vjp_image_kernel, dim3(grid), dim3(256), 0, s, X, n, H, C, image, b_img);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = siren_wgrad(a_img, b_img, image, H, C, tiles, n, part, 1, s)) != hipSuccess) return e;
  const int slices = (tiles * C + kSirenWgradSliceBlocks - 1) / kSirenWgradSliceBlocks;
  SirenReduceSegs segs{};
  segs.n = 1;
  segs.end[0] = H * H;
  segs.dst[0] = dW;
  return siren_reduce(part, slices, (size_t)H * H, segs, false, s);
}

}  // namespace wos
