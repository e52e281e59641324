// wos_siren_fit.hip -- fused SIREN fit step (wos_siren_fit): the regression loss of the network's
// value against a fixed target and its gradient with respect to every weight and bias.
//
// Contract (DESIGN.md "Fused SIREN fit step").  With N = n d_out and, per point p and output i,
//   u       wos_siren_eval's value chain (the value-only kernel's code: the same bits)
//   r       = fma(scale, u, -target)                      (scale absent: 1, i.e. u - target rounded once)
//   ub      = (scale (r + r)) (1 / N)                     the seed d loss / d u, 1 / N rounded once on the host
//   loss    = (sum of r r) / N
// With a matrix wrap (MATRIX: scale is S [n][d_out][d_out], row-major) the two lines read
//   r_i     = -target_i, then r_i = fma(S[i][m], u_m, r_i) for m = 0 .. d_out - 1 in order
//   ub_m    = acc (1 / N) with g_i = r_i + r_i, acc = S[0][m] g_0 (rounded), then
//             acc = fma(S[i][m], g_i, acc) for i = 1 .. d_out - 1: the seed S^T (2 r) / N
// and everything from r and ub on is the same code.
// The gradients are the backward of wos_siren_vjp seeded with g_u = ub and no tangent columns:
//   output   dWo[i][h] = sum_p ub_i a[h],  dbo = sum_p ub,  da = Wo^T ub
//   sine     dz = (w c) da
//   hidden   dW = sum_p dz a_prev^T,  db = sum_p dz,  da_prev = W^T dz
//   layer 0  dW0[r][k] = sum_p dz[r] x_k,  db0 = sum_p dz
//
// Layout.  The points go in chunks of whole 32-point tiles whose stash fits the workspace.  Per
// chunk, siren_fit_tile_kernel (the forward's workgroup: 4 waves, one tile, one column per point,
// X[H][32] in LDS) runs the value-only forward with the forward's own code, stores every layer's
// pre-activation column to the stash, forms r and ub in LDS and writes the tile's sum of squares;
// the loss-only instantiation ends there and stores nothing else.  The other one sweeps back as
// siren_vjp_tile_kernel does: it reloads a layer's z, repeats sincosf on the same bits, forms dz in
// place in LDS, stores it for the weight-gradient kernel, overwrites the stashed z with the layer's
// output a and takes da_prev = W^T dz with siren_hidden_gemm<1, RT> on the transposed
// fragment-ordered copy of W.  The backward's siren_wgrad_kernel (C = 1) and siren_reduce_kernel
// finish the weight gradients; the tiles' sums of squares have a reduction of their own.  No
// atomics: the same n and chunk size give the same bits, in the loss and in every gradient.
//
// A point past n has r = ub = 0, so every dz of its column is a zero (its forward column, computed
// on x = 0, is finite); the weight-gradient kernel masks those columns on load as well.
#include "wos_siren_device.h"

namespace wos {

// xs: [L + 1][T][H][32], ds: [L][T][H][32] (layer_stride = T H 32); part: [tile][P], the backward's
// layout: dWo [d_out][H] | dbo [d_out] | db_0 .. db_L [H] each | dW0 [H][D]; loss_part: [tile].
// Grid y is the member: its network and rows come from the argument arrays, and its packed copies,
// stash and partials lie blockIdx.y * member_stride floats past member 0's.  The points and the
// zeros are shared.  MATRIX: a member's scale is [n][d_out][d_out]; a member without one takes the
// unscaled path, as in the other instantiation.
template <int D, int RT, bool GRADS, bool MATRIX>
__global__ __launch_bounds__(256) void siren_fit_tile_kernel(const SirenNets nets, const float4* __restrict__ packed,
                                                            const float4* __restrict__ packedT,
                                                            const float* __restrict__ zeros,
                                                            const float* __restrict__ pts, int64_t n,
                                                            const SirenMemberRows rows, float inv_count,
                                                            float* __restrict__ xs, float* __restrict__ ds,
                                                            size_t layer_stride, float* __restrict__ tile_part, int P,
                                                            float* __restrict__ loss_part, size_t member_stride) {
  constexpr int cols = 32;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int member = blockIdx.y;
  const SirenNet& net = nets.v[member];
  const float* __restrict__ target = rows.target[member];
  const float* __restrict__ scale = rows.scale[member];
  {  // (a stride that is a multiple of four floats: the packed copies are read as float4)
    const size_t off = member * member_stride;
    packed += off / 4;
    loss_part += off;
    if (GRADS) {
      packedT += off / 4;
      xs += off;
      ds += off;
      tile_part += off;
    }
  }
  const int H = net.H, L = net.L, DO = net.d_out;
  const float omega = net.omega;
  float* Xl = s_mem;             // [H][32]
  float* Sl = s_mem + H * cols;  // [3][32]: the seeds ub per output row
  float* Rl = Sl + 3 * cols;     // [3][32]: the residuals r
  float* Ql = Rl + 3 * cols;     // [32]: the points' squared residuals
  float* Pl = Ql + cols;         // [D][32]: the tile's points
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = tid & 31;
  const int64_t base = (int64_t)blockIdx.x * kSirenTile;
  const size_t tile_off = (size_t)blockIdx.x * H * cols;

  {  // layer 0, the forward's code; the pre-activation column goes to the stash
    const int64_t p = base + j;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; k++) x[k] = p < n ? pts[p * D + k] : 0.0f;
    if (GRADS && tid < 32) {
#pragma unroll
      for (int k = 0; k < D; k++) Pl[k * 32 + j] = x[k];
    }
    const float* W0 = net.w[0];
    const float* b0 = net.b[0];
    for (int row = tid >> 5; row < H; row += 8) {
      float z = b0[row];
#pragma unroll
      for (int k = 0; k < D; k++) z = fmaf(W0[row * D + k], x[k], z);
      if (GRADS) xs[tile_off + row * cols + j] = z;
      const float wz = omega * z;
      float sn, cs;
      sincosf(wz, &sn, &cs);
      Xl[row * cols + j] = sn;
    }
  }
  __syncthreads();

  const int R = H >> 5, Q = H >> 3;
  const bool busy = wave < R;  // wave-uniform: with H < 128 the waves past H / 32 own no row tile
  for (int l = 0; l < L; l++) {
    f32x16 acc[RT][1];
    if (busy) siren_hidden_gemm<1, RT>(packed + (size_t)l * R * Q * 64, net.b[1 + l], Xl, H, wave, lane, acc);
    __syncthreads();  // every wave has read X: the layer is written back in place
    if (busy) {
#pragma unroll
      for (int i = 0; i < RT; i++) {
        const int r = wave + 4 * i;
        if (r < R) {
#pragma unroll
          for (int reg = 0; reg < 16; reg++) Xl[(r * 32 + siren_acc_row(reg, lane)) * cols + j] = acc[i][0][reg];
        }
      }
      float* zs = xs + (size_t)(l + 1) * layer_stride + tile_off;
      for (int t = 0; t < RT * 16; t++) {
        const int r = wave + 4 * (t >> 4);
        if (r >= R) break;
        const int row = r * 32 + siren_acc_row(t & 15, lane);
        float* xo = Xl + row * cols + j;
        const float z = xo[0];
        if (GRADS) zs[row * cols + j] = z;
        const float wz = omega * z;
        float sn, cs;
        sincosf(wz, &sn, &cs);
        xo[0] = sn;
      }
    }
    __syncthreads();
  }

  {  // output layer, the forward's chain; the thread that holds u_i of a point forms its r and ub
    const float* Wo = net.w[L + 1];
    const float* bo = net.b[L + 1];
    const int i = tid >> 5;  // the output row of this thread, for tid < 3 * cols
    const int64_t p = base + j;
    const bool live = tid < 3 * cols && i < DO && p < n;
    float u = 0.0f;
    if (tid < 3 * cols && i < DO) {
      const float* wr = Wo + i * H;
      for (int h = 0; h < H; h++) u = fmaf(wr[h], Xl[h * cols + j], u);
      u = u + bo[i];
    }
    if (MATRIX && scale) {
      // a point's d_out values meet in LDS: u in the seeds' rows, then r in its own, then the seeds
      const float* S = scale + (p * DO + i) * DO;  // row i of the point's matrix (read when live)
      if (tid < 3 * cols) Sl[tid] = u;
      __syncthreads();
      float r = 0.0f;
      if (live) {
        r = -target[p * DO + i];
        for (int m = 0; m < DO; m++) r = fmaf(S[m], Sl[m * cols + j], r);
      }
      if (tid < 3 * cols) Rl[tid] = r;
      __syncthreads();  // every u has been read: the seeds' rows are free again
      float ub = 0.0f;
      if (live) {  // this thread's output is column i of S now: ub_i = (sum over k of S[k][i] (r_k + r_k)) / N
        const float* Sc = scale + p * DO * DO + i;
        const float g0 = Rl[j] + Rl[j];
        float acc = Sc[0] * g0;
        for (int k = 1; k < DO; k++) {
          const float g = Rl[k * cols + j] + Rl[k * cols + j];
          acc = fmaf(Sc[k * DO], g, acc);
        }
        ub = acc * inv_count;
      }
      if (tid < 3 * cols) Sl[tid] = ub;
    } else if (tid < 3 * cols) {
      float r = 0.0f, ub = 0.0f;
      if (live) {
        const float sc = scale ? scale[p * DO + i] : 1.0f;
        r = fmaf(sc, u, -target[p * DO + i]);
        ub = (sc * (r + r)) * inv_count;
      }
      Rl[tid] = r;
      Sl[tid] = ub;
    }
  }
  __syncthreads();

  if (tid < 32) {  // a point's squares, over i in order
    float q = Rl[tid] * Rl[tid];
    q = q + Rl[cols + tid] * Rl[cols + tid];
    q = q + Rl[2 * cols + tid] * Rl[2 * cols + tid];
    Ql[tid] = q;
  }
  float* part = tile_part + (size_t)blockIdx.x * P;
  if (GRADS) {  // dWo and dbo of this tile.  Row h starts its sum at column h mod 32, so that the threads
                // of a wave half read 32 different banks; the order is fixed all the same.
    for (int h = tid; h < H; h += 256) {
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
      int col = h & 31;
#pragma unroll 4
      for (int t = 0; t < cols; t++) {
        const float xv = Xl[h * cols + col];
        s0 = fmaf(Sl[col], xv, s0);
        s1 = fmaf(Sl[cols + col], xv, s1);
        s2 = fmaf(Sl[2 * cols + col], xv, s2);
        col = (col + 1) & 31;
      }
      part[h] = s0;
      if (DO > 1) part[H + h] = s1;
      if (DO > 2) part[2 * H + h] = s2;
    }
    if (tid < DO) {
      float v[32];  // a plain sum of the seeds: pairwise, (p, p + 16), then (p, p + 8), ...
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
  if (tid == 255) {  // the tile's sum of squares: pairwise over the points, (p, p + 16), then (p, p + 8), ...
    float v[32];
#pragma unroll
    for (int t = 0; t < 32; t++) v[t] = Ql[t];
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1)
#pragma unroll
      for (int t = 0; t < w; t++) v[t] = v[t] + v[t + w];
    loss_part[blockIdx.x] = v[0];
  }
  if (!GRADS) return;
  {  // da of the last sine layer = Wo^T ub, over X
    const float* Wo = net.w[L + 1];
    for (int item = tid; item < H * cols; item += 256) {
      const int h = item >> 5;
      float v = Wo[h] * Sl[j];
      if (DO > 1) v = fmaf(Wo[H + h], Sl[cols + j], v);
      if (DO > 2) v = fmaf(Wo[2 * H + h], Sl[2 * cols + j], v);
      Xl[item] = v;
    }
  }
  __syncthreads();

  float* part_b = part + DO * H + DO;
  float* part_w0 = part_b + (L + 1) * H;
  for (int l = L; l >= 0; l--) {
    float* zs = xs + (size_t)l * layer_stride + tile_off;
    float* dst = l >= 1 ? ds + (size_t)(l - 1) * layer_stride + tile_off : nullptr;
    for (int item = tid; item < H * cols; item += 256) {  // (row, point): the point is tid & 31 throughout
      const float wz = omega * zs[item];
      float sn, cs;
      sincosf(wz, &sn, &cs);
      const float dz = (omega * cs) * Xl[item];
      Xl[item] = dz;
      if (dst) dst[item] = dz;
      if (l < L) zs[item] = sn;  // the other operand of the next layer's weight gradient
    }
    __syncthreads();
    for (int r = tid; r < H; r += 256) {  // db_l, and dW0 at layer 0: sums over the tile's points
      float sb = 0.0f, sw[D];
#pragma unroll
      for (int k = 0; k < D; k++) sw[k] = 0.0f;
#pragma unroll 4
      for (int t = 0; t < 32; t++) {
        const int jj = (t + r) & 31;
        const float dz = Xl[r * cols + jj];
        sb = sb + dz;
        if (l == 0) {
#pragma unroll
          for (int k = 0; k < D; k++) sw[k] = fmaf(dz, Pl[k * 32 + jj], sw[k]);
        }
      }
      part_b[l * H + r] = sb;
      if (l == 0) {
#pragma unroll
        for (int k = 0; k < D; k++) part_w0[r * D + k] = sw[k];
      }
    }
    if (l == 0) break;
    f32x16 acc[RT][1];
    if (busy) siren_hidden_gemm<1, RT>(packedT + (size_t)(l - 1) * R * Q * 64, zeros, Xl, H, wave, lane, acc);
    __syncthreads();  // every wave has read dz, and the partial sums above are done
    if (busy) {
#pragma unroll
      for (int i = 0; i < RT; i++) {
        const int r = wave + 4 * i;
        if (r < R) {
#pragma unroll
          for (int reg = 0; reg < 16; reg++) Xl[(r * 32 + siren_acc_row(reg, lane)) * cols + j] = acc[i][0][reg];
        }
      }
    }
    __syncthreads();
  }
}

// loss = (first ? 0 : loss) + sum of part[0 .. n_part), divided by `count` after the last chunk;
// between chunks loss[0] holds the running sum of squares.  One workgroup: thread t adds the
// partials t, t + 256, ... as a chain, then the 256 chains' sums pairwise, (t, t + 128), (t, t + 64), ...
// One workgroup per member: its partials at part + e * part_stride, its loss at loss[e * loss_stride].
__global__ __launch_bounds__(256) void siren_fit_loss_kernel(const float* __restrict__ part, int n_part,
                                                            float* __restrict__ loss, float count, int first,
                                                            int last, size_t part_stride, size_t loss_stride) {
  __shared__ float sm[256];
  const int tid = threadIdx.x;
  part += blockIdx.x * part_stride;
  loss += blockIdx.x * loss_stride;
  float s = 0.0f;
  for (int i = tid; i < n_part; i += 256) s = s + part[i];
  sm[tid] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) sm[tid] = sm[tid] + sm[tid + w];
    __syncthreads();
  }
  if (tid != 0) return;
  const float total = first ? sm[0] : loss[0] + sm[0];
  loss[0] = last ? total / count : total;
}

size_t siren_fit_tile_lds_bytes(int d_in, int H) { return ((size_t)(H + 7) * 32 + d_in * 32) * sizeof(float); }

SirenFitPlan siren_fit_plan(const SirenNet& net, int64_t n, size_t stash_cap_bytes, int resident_tiles) {
  SirenFitPlan p{};
  const size_t per_tile = siren_fit_stash_floats_per_tile(net.H, net.L);
  const int64_t tiles_all = (n + kSirenTile - 1) / kSirenTile;
  int64_t fit = (int64_t)(stash_cap_bytes / (per_tile * sizeof(float)));
  fit = fit < (1 << 20) ? fit : (1 << 20);  // every launch's grid stays far inside an int
  p.tiles = (int)(tiles_all < fit ? tiles_all : fit);
  if (p.tiles < 1) return p;
  if (resident_tiles > 0 && p.tiles < tiles_all && p.tiles > resident_tiles)
    p.tiles -= p.tiles % resident_tiles;  // several chunks: each a whole number of rounds of resident workgroups
  p.slices = net.L > 0 ? (p.tiles + kSirenWgradSliceBlocks - 1) / kSirenWgradSliceBlocks : 0;
  p.stash = per_tile * p.tiles;
  p.tile_part = siren_vjp_tile_part_floats(net) * p.tiles;
  p.slice_part = (size_t)p.slices * net.L * net.H * net.H;
  p.loss_part = (size_t)p.tiles;
  return p;
}

// what one chunk's tile launch takes
struct FitTileArgs {
  const float *packed, *packedT, *zeros, *pts;
  int64_t n;
  SirenMemberRows rows;
  float inv_count;
  float *xs, *ds;
  size_t layer_stride;
  float* tile_part;
  int P;
  float* loss_part;
  size_t member_stride;
  bool matrix;  // rows.scale holds a d_out x d_out matrix per point
};

template <int D, int RT, bool GRADS, bool MATRIX>
static hipError_t siren_fit_tile_launch(const SirenNets& nets, int E, const FitTileArgs& a, hipStream_t s) {
  const size_t lds = siren_fit_tile_lds_bytes(D, nets.v[0].H);
  const int64_t grid = (a.n + kSirenTile - 1) / kSirenTile;
  hipLaunchKernelGGL((siren_fit_tile_kernel<D, RT, GRADS, MATRIX>), dim3((unsigned)grid, E), dim3(256), lds, s, nets,
                     (const float4*)a.packed, (const float4*)a.packedT, a.zeros, a.pts, a.n, a.rows, a.inv_count, a.xs,
                     a.ds, a.layer_stride, a.tile_part, a.P, a.loss_part, a.member_stride);
  return hipGetLastError();
}

template <int D, bool GRADS, bool MATRIX>
static hipError_t siren_fit_tile_rows(const SirenNets& nets, int E, const FitTileArgs& a, hipStream_t s) {
  return nets.v[0].H > 128 ? siren_fit_tile_launch<D, 2, GRADS, MATRIX>(nets, E, a, s)
                           : siren_fit_tile_launch<D, 1, GRADS, MATRIX>(nets, E, a, s);
}

template <bool GRADS>
static hipError_t siren_fit_tile_select(const SirenNets& nets, int E, const FitTileArgs& a, hipStream_t s) {
  if (nets.v[0].d_in == 2)
    return a.matrix ? siren_fit_tile_rows<2, GRADS, true>(nets, E, a, s) : siren_fit_tile_rows<2, GRADS, false>(nets, E, a, s);
  return a.matrix ? siren_fit_tile_rows<3, GRADS, true>(nets, E, a, s) : siren_fit_tile_rows<3, GRADS, false>(nets, E, a, s);
}

hipError_t launch_siren_fit_members(const SirenNets& nets, int E, const float* packed, const float* packedT,
                                    const float* zeros, const float* pts, int64_t n, const SirenMemberRows& rows,
                                    float* loss, size_t loss_stride, const SirenGrads* grads, size_t grad_stride,
                                    const SirenFitPlan& plan, float* work, size_t member_stride, hipStream_t s) {
  const SirenNet& net = nets.v[0];  // every member has its shape
  const int D = net.d_in, DO = net.d_out, H = net.H, L = net.L, cols = 32;
  if (n <= 0 || plan.tiles < 1 || E < 1 || E > kSirenMaxMembers) return hipErrorInvalidValue;
  // floats per row of a scale: d_out, or d_out * d_out for a matrix per point (0: d_out).  With
  // d_out = 1 the two are one layout and one arithmetic, and the diagonal kernel serves both.
  const int SW = rows.scale_width ? rows.scale_width : DO;
  if (SW != DO && SW != DO * DO) return hipErrorInvalidValue;
  hipError_t e;
  const int T = plan.tiles, P = (int)siren_vjp_tile_part_floats(net);
  const size_t layer_stride = (size_t)T * H * cols;
  // the whole call's count: a chunk's seeds and the last division see n, not the chunk
  const float count = (float)((double)n * DO), inv_count = 1.0f / count;
  float *xs = nullptr, *ds = nullptr, *tile_part = nullptr, *slice_part = nullptr, *loss_part = work;
  SirenReduceSegs tile_segs{}, slice_segs{};
  if (grads) {
    xs = work;
    ds = xs + (size_t)(L + 1) * layer_stride;
    tile_part = work + plan.stash;
    slice_part = tile_part + plan.tile_part;
    loss_part = slice_part + plan.slice_part;
    // the tiles' partials in the order of the tile kernel's layout, and the slices' by layer
    const auto seg = [](SirenReduceSegs& g, float* dst, int count) {
      g.end[g.n] = (g.n ? g.end[g.n - 1] : 0) + count;
      g.dst[g.n++] = dst;
    };
    seg(tile_segs, grads->w[L + 1], DO * H);
    seg(tile_segs, grads->b[L + 1], DO);
    for (int l = 0; l <= L; l++) seg(tile_segs, grads->b[l], H);
    seg(tile_segs, grads->w[0], H * D);
    for (int l = 0; l < L; l++) seg(slice_segs, grads->w[1 + l], H * H);
  }
  const int64_t per_chunk = (int64_t)T * kSirenTile;
  for (int64_t base = 0; base < n; base += per_chunk) {
    const int64_t nc = n - base < per_chunk ? n - base : per_chunk;
    const int tiles = (int)((nc + kSirenTile - 1) / kSirenTile);
    const bool acc = base > 0, last = base + per_chunk >= n;
    FitTileArgs a{};
    a.packed = packed;
    a.pts = pts + base * D;
    a.n = nc;
    for (int m = 0; m < E; m++) {
      a.rows.target[m] = rows.target[m] + base * DO;
      a.rows.scale[m] = rows.scale[m] ? rows.scale[m] + base * SW : nullptr;
    }
    a.rows.scale_width = SW;
    a.matrix = SW != DO;
    a.inv_count = inv_count;
    a.loss_part = loss_part;
    a.member_stride = member_stride;
    if (grads) {
      a.packedT = packedT;
      a.zeros = zeros;
      a.xs = xs;
      a.ds = ds;
      a.layer_stride = layer_stride;
      a.tile_part = tile_part;
      a.P = P;
    }
    e = grads ? siren_fit_tile_select<true>(nets, E, a, s) : siren_fit_tile_select<false>(nets, E, a, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(siren_fit_loss_kernel, dim3(E), dim3(256), 0, s, loss_part, tiles, loss, count, acc ? 0 : 1,
                       last ? 1 : 0, member_stride, loss_stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!grads) continue;
    if ((e = siren_reduce_members(tile_part, tiles, P, tile_segs, acc, E, member_stride, grad_stride, s)) != hipSuccess) return e;
    if (L > 0) {
      if ((e = siren_wgrad_members(ds, xs, layer_stride, H, 1, tiles, nc, slice_part, L, E, member_stride, s)) != hipSuccess)
        return e;
      const int slices = (tiles + kSirenWgradSliceBlocks - 1) / kSirenWgradSliceBlocks;
      if ((e = siren_reduce_members(slice_part, slices, (size_t)L * H * H, slice_segs, acc, E, member_stride, grad_stride, s)) !=
          hipSuccess)
        return e;
    }
  }
  return hipSuccess;
}

hipError_t launch_siren_fit(const SirenNet& net, const float* packed, const float* packedT, const float* zeros,
                            const float* pts, int64_t n, const float* target, const float* scale, int scale_width,
                            float* loss, const SirenGrads* grads, const SirenFitPlan& plan, float* work, hipStream_t s) {
  SirenNets nets{};
  nets.v[0] = net;
  SirenMemberRows rows{};
  rows.target[0] = target;
  rows.scale[0] = scale;
  rows.scale_width = scale_width;
  return launch_siren_fit_members(nets, 1, packed, packedT, zeros, pts, n, rows, loss, 0, grads, 0, plan, work, 0, s);
}

}  // namespace wos
