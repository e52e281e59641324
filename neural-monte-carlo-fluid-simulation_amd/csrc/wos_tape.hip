// wos_tape.hip -- the walk tape (wos_tape_record / wos_tape_solve): a solve's walks recorded
// once and replayed for every new source grid.
//
// A walk never looks at the source (wos_channels.hip), and the source enters a walk's total in
// three places only: the first ball (gnorm * texel), every step that samples inside the star
// (pThr * (pNrm * texel)) and the finish (throughput * g + totalNeumann + totalSource).  The
// recording instantiations of the first-ball and walk code (REC = true in wos_device.h:
// reference semantics, one channel, full Neumann term, no tail spreading) store the factors
// and the grid cell of every such product in a DevTape instead of loading the texel;
// wos_tape_replay_kernel repeats the products and sums for the scene's current source, per
// channel, in the walk's own order -- bit for bit the full solve -- and the ordinary fold
// follows on the replayed totals.
//
// A translation unit of its own: the five units of the solve are compiled as before.
#include "wos_device.h"
#include "wos_launch.h"
#include "wos_select.h"

namespace wos {

// ---- recording kernels: the bodies of wos_first_ball_kernel / wos_walk_kernel with REC = true.
// The arguments of the kernel they record come first (the walk body re-reads scene,
// parameters and tasks from the head of the kernarg segment), the tape last.
template <int DIM>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DIM == 2 ? WOS_FB_WAVES_PER_EU2 : WOS_FB_WAVES_PER_EU))) void wos_first_ball_rec_kernel(
    const DevScene sc, const DevParams prm, const float* __restrict__ pts, int64_t n, int64_t base, int64_t stride,
    const DevTasks tk, unsigned long long* __restrict__ counters, unsigned int* __restrict__ work, int lhs_floats,
    const DevTape tape_arg) {
  constexpr bool RB = false, REC = true;
  constexpr int NC = 1;
  const DevTape* const tape = &tape_arg;
#include "wos_first_ball_body.inc"
}

template <int DIM, bool GG>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DIM == 2 ? WOS_WALK_WAVES_PER_EU : WOS_WALK_WAVES_PER_EU3))) void wos_walk_rec_kernel(
    const DevScene sc_arg, const DevParams prm_arg, const DevTasks tk_arg, int64_t base, int64_t stride,
    unsigned long long* __restrict__ counters, unsigned int* __restrict__ tqueue, int geom_floats,
    const DevTape tape_arg) {
  constexpr bool BSTART = false, RB = false, NEU = true, SPR = false, REC = true;
  constexpr int NC = 1;
  const DevTape* const tape = &tape_arg;
#include "wos_walk_body.inc"
}

template __global__ void wos_first_ball_rec_kernel<2>(WOS_FIRST_BALL_PARAMS, const DevTape);
template __global__ void wos_first_ball_rec_kernel<3>(WOS_FIRST_BALL_PARAMS, const DevTape);
template __global__ void wos_walk_rec_kernel<2, false>(WOS_WALK_PARAMS, const DevTape);
template __global__ void wos_walk_rec_kernel<2, true>(WOS_WALK_PARAMS, const DevTape);
template __global__ void wos_walk_rec_kernel<3, false>(WOS_WALK_PARAMS, const DevTape);
template __global__ void wos_walk_rec_kernel<3, true>(WOS_WALK_PARAMS, const DevTape);

using FirstBallRecKernel = void (*)(WOS_FIRST_BALL_PARAMS, const DevTape);
using WalkRecKernel = void (*)(WOS_WALK_PARAMS, const DevTape);

static FirstBallRecKernel first_ball_rec_of(int dim) {
  return dim == 2 ? wos_first_ball_rec_kernel<2> : dim == 3 ? wos_first_ball_rec_kernel<3> : nullptr;
}
static WalkRecKernel walk_rec_of(int dim, bool gg) {
  if (dim == 2) return gg ? wos_walk_rec_kernel<2, true> : wos_walk_rec_kernel<2, false>;
  if (dim == 3) return gg ? wos_walk_rec_kernel<3, true> : wos_walk_rec_kernel<3, false>;
  return nullptr;
}

hipError_t launch_first_balls_rec(int dim, const DevScene& sc, const DevParams& prm, const float* pts, int64_t n,
                                  int64_t base, int64_t stride, const DevTasks& tk, const DevTape& tape,
                                  unsigned long long* counters, unsigned int* work, int grid, size_t shmem,
                                  int lhs_floats, hipStream_t s) {
  const FirstBallRecKernel kernel = first_ball_rec_of(dim);
  if (!kernel) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), shmem, s, sc, prm, pts, n, base, stride, tk, counters, work,
                     lhs_floats, tape);
  return hipGetLastError();
}

hipError_t launch_walks_rec(int dim, bool geom_global, const DevScene& sc, const DevParams& prm, const DevTasks& tk,
                            const DevTape& tape, int64_t base, int64_t stride, unsigned long long* counters,
                            unsigned int* tqueue, int grid, size_t shmem, int geom_floats, hipStream_t s) {
  const WalkRecKernel kernel = walk_rec_of(dim, geom_global);
  if (!kernel) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), shmem, s, sc, prm, tk, base, stride, counters, tqueue,
                     geom_floats, tape);
  return hipGetLastError();
}

hipError_t occupancy_rec_blocks_per_cu(int dim, bool geom_global, int which, size_t shmem, int* blocks) {
  const void* kernel = which == 0 ? (const void*)first_ball_rec_of(dim)
                                  : which == 1 ? (const void*)walk_rec_of(dim, geom_global) : nullptr;
  if (!kernel) return hipErrorInvalidValue;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, kernel, kBlock, shmem);
}

// ---- slot sizing: slot = exclusive scan, in task order, of an upper bound of every task's entries.
// A recorded walk of `steps` ball steps (the first ball included) has at most steps - 1 entries,
// a dropped walk keeps none.  Blocks of kSlotBlock tasks: block sums, one block scans them,
// then every block scans its own tasks from its offset.  slot[T] = the batch's slots.
constexpr int kSlotPer = 8, kSlotBlock = 256 * kSlotPer;

__device__ __forceinline__ uint32_t tape_cap_of(uint32_t code) { return (code & 1u) && (code >> 1) > 0u ? (code >> 1) - 1u : 0u; }

// exclusive scan of one value per thread over the block's 256 threads; *sum: the block's total
__device__ __forceinline__ unsigned long long block_excl_scan_256(unsigned long long v, unsigned long long* sh,
                                                                  unsigned long long* sum) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned long long a = tid >= off ? sh[tid - off] : 0ull;
    __syncthreads();
    sh[tid] += a;
    __syncthreads();
  }
  const unsigned long long incl = sh[tid];
  *sum = sh[255];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(256) void wos_tape_cap_sum_kernel(const uint32_t* __restrict__ code, int64_t T,
                                                               unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long sh[256];
  const int64_t b0 = (int64_t)blockIdx.x * kSlotBlock;
  unsigned long long v = 0ull;
  for (int j = 0; j < kSlotPer; j++) {
    const int64_t i = b0 + (int64_t)j * 256 + threadIdx.x;
    if (i < T) v += tape_cap_of(code[i]);
  }
  unsigned long long sum;
  block_excl_scan_256(v, sh, &sum);
  if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
}

// in place: bsum[b] -> sum of the blocks before b; bsum[nb] = the total
__global__ __launch_bounds__(256) void wos_tape_block_scan_kernel(unsigned long long* bsum, int64_t nb) {
  __shared__ unsigned long long sh[256];
  unsigned long long carry = 0ull;
  for (int64_t b0 = 0; b0 < nb; b0 += 256) {
    const int64_t i = b0 + threadIdx.x;
    const unsigned long long v = i < nb ? bsum[i] : 0ull;
    unsigned long long sum;
    const unsigned long long ex = block_excl_scan_256(v, sh, &sum);
    if (i < nb) bsum[i] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}

// slot[i] for i in [0, T]: thread tid owns the block's tasks [tid * kSlotPer, (tid + 1) * kSlotPer)
__global__ __launch_bounds__(256) void wos_tape_slot_kernel(const uint32_t* __restrict__ code, int64_t T,
                                                            const unsigned long long* __restrict__ bsum,
                                                            uint32_t* __restrict__ slot) {
  __shared__ unsigned long long sh[256];
  const int64_t i0 = (int64_t)blockIdx.x * kSlotBlock + (int64_t)threadIdx.x * kSlotPer;
  uint32_t cap[kSlotPer];
  unsigned long long v = 0ull;
  for (int j = 0; j < kSlotPer; j++) {
    cap[j] = i0 + j < T ? tape_cap_of(code[i0 + j]) : 0u;
    v += cap[j];
  }
  unsigned long long sum;
  unsigned long long at = bsum[blockIdx.x] + block_excl_scan_256(v, sh, &sum);
  for (int j = 0; j < kSlotPer; j++) {
    if (i0 + j <= T) slot[i0 + j] = (uint32_t)at;
    at += cap[j];
  }
}

hipError_t launch_tape_slots(const uint32_t* code, int64_t T, uint32_t* slot, unsigned long long* bsum, hipStream_t s) {
  const int64_t nb = tape_slot_blocks(T);
  if (nb > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wos_tape_cap_sum_kernel, dim3((unsigned)nb), dim3(256), 0, s, code, T, bsum);
  hipLaunchKernelGGL(wos_tape_block_scan_kernel, dim3(1), dim3(256), 0, s, bsum, nb);
  hipLaunchKernelGGL(wos_tape_slot_kernel, dim3((unsigned)nb), dim3(256), 0, s, code, T, (const unsigned long long*)bsum,
                     slot);
  return hipGetLastError();
}

// entries of the recorded walks: out[0] += their sum, out[1] = max(out[1], the longest)
__global__ __launch_bounds__(256) void wos_tape_stats_kernel(const uint32_t* __restrict__ code,
                                                             const uint32_t* __restrict__ cnt, int64_t T,
                                                             unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_sum, s_max;
  if (threadIdx.x == 0) { s_sum = 0ull; s_max = 0ull; }
  __syncthreads();
  unsigned long long sum = 0ull, mx = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T; i += (int64_t)gridDim.x * blockDim.x) {
    if (!(code[i] & 1u)) continue;
    const unsigned long long c = cnt[i] & ~kTapeOwnG;
    sum += c;
    mx = c > mx ? c : mx;
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off);
    const unsigned long long o = __shfl_xor(mx, off);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) { atomicAdd(&s_sum, sum); atomicMax(&s_max, mx); }
  __syncthreads();
  if (threadIdx.x == 0) { atomicAdd(&out[0], s_sum); atomicMax(&out[1], s_max); }
}

hipError_t launch_tape_stats(const uint32_t* code, const uint32_t* cnt, int64_t T, unsigned long long* out,
                             hipStream_t s) {
  if (T < 1) return hipSuccess;
  const int grid = (int)std::min<int64_t>((T + 255) / 256, 1024);
  hipLaunchKernelGGL(wos_tape_stats_kernel, dim3(grid), dim3(256), 0, s, code, cnt, T, out);
  return hipGetLastError();
}

// ---- replay ----------------------------------------------------------------------------
// One lane per task, a wave per 64 consecutive tasks.  Slots are a prefix sum in task order, so
// the wave's walks own one contiguous slot range: the wave streams it in chunks of kTapeChunk
// entries -- one entry per lane, coalesced 4-byte loads of cell, pThr and pNrm -- gathers the
// chunk's texels wave-wide and parks them with (pThr, pNrm) in its LDS slice; then every lane
// adds its own walk's entries of the chunk in step order.  A walk longer than a chunk and a
// group larger than the slice simply take more passes.  The float operations per walk and
// channel are the solve's, in its order (first_balls, flush_source, walk_finish):
//   first = gnorm * tex0;  tsrc = 0;  tsrc += 1 * first;
//   tsrc += pThr * (pNrm * tex)  per entry;
//   total = thrEnd * g + totalNeumann + tsrc.
template <int NC>
struct Texel { float v[NC]; };

template <int NC>
__device__ __forceinline__ Texel<NC> tape_texel(const float* __restrict__ source, uint32_t cells, uint32_t cell) {
  Texel<NC> r;
  for (int c = 0; c < NC; c++) r.v[c] = 0.0f;
  // a null source reads as 0 (source_value); a cell is never beyond the grid the tape was recorded on
  if (source == nullptr || cell >= cells) return r;
  if constexpr (NC == 1) {
    r.v[0] = source[cell];
  } else {
    static_assert(NC == 4, "one float4 texel per cell");
    const float4 q = reinterpret_cast<const float4*>(source)[cell];
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
  }
  return r;
}

struct TapeChannels { float g[kMaxChannels]; };

template <int NC>
__global__ __launch_bounds__(kBlock) void wos_tape_replay_kernel(const DevTape tp, const uint32_t* __restrict__ code,
                                                                 const float* __restrict__ source, uint32_t cells,
                                                                 int ignore_source, int n_channels,
                                                                 const TapeChannels gch, int64_t T,
                                                                 float* __restrict__ total, float* __restrict__ first) {
  __shared__ float s_thr[kBlock / kWave][kTapeChunk], s_nrm[kBlock / kWave][kTapeChunk];
  __shared__ float s_tex[kBlock / kWave][kTapeChunk * NC];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t - lane >= T) return;  // the whole wave is beyond the tasks
  const bool valid = t < T;
  const uint32_t cd = valid ? code[t] : 0u;
  const bool rec = (cd & 1u) != 0u;  // dropped walks and points without walks are skipped
  const uint32_t s0 = valid ? tp.slot[t] : 0u;
  const uint32_t cap = valid ? tp.slot[t + 1] - s0 : 0u;
  const uint32_t cw = rec ? tp.cnt[t] : 0u;
  const bool own_g = (cw & kTapeOwnG) != 0u;
  uint32_t n = cw & ~kTapeOwnG;
  n = n < cap ? n : cap;
  float tsrc[NC], fst[NC];
  for (int c = 0; c < NC; c++) { tsrc[c] = 0.0f; fst[c] = 0.0f; }
  if (rec && !ignore_source) {
    const float gnorm = tp.gnorm[t];
    const Texel<NC> x = tape_texel<NC>(source, cells, tp.cell0[t]);
    for (int c = 0; c < NC; c++) {
      fst[c] = gnorm * x.v[c];
      tsrc[c] += 1.0f * fst[c];
    }
  }
  // the wave's slot range: from its first task's slots to the last entry any of its walks wrote
  const uint32_t e0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s0);
  uint32_t e1 = rec ? s0 + n : e0;
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)e1, off);
    e1 = o > e1 ? o : e1;
  }
  for (uint32_t w0 = e0; w0 < e1; w0 += kTapeChunk) {
    const uint32_t e = w0 + (uint32_t)lane;
    if (e < e1) {
      const Texel<NC> x = tape_texel<NC>(source, cells, tp.e_cell[e]);
      s_thr[wave][lane] = tp.e_thr[e];
      s_nrm[wave][lane] = tp.e_nrm[e];
      for (int c = 0; c < NC; c++) s_tex[wave][lane * NC + c] = x.v[c];
    }
    wave_sync();
    const uint32_t lo = s0 > w0 ? s0 : w0;
    const uint32_t hi = s0 + n < w0 + kTapeChunk ? s0 + n : w0 + kTapeChunk;
    for (uint32_t j = lo; j < hi; j++) {
      const uint32_t k = j - w0;
      const float thr = s_thr[wave][k], nrm = s_nrm[wave][k];
      for (int c = 0; c < NC; c++) tsrc[c] += thr * (nrm * s_tex[wave][k * NC + c]);
    }
    wave_sync();
  }
  if (!rec) return;
  const float thr_end = tp.thr_end[t], term = tp.term[t], tneu = tp.tneu[t];
  for (int c = 0; c < NC; c++) {
    if (c >= n_channels) break;
    // several channels: channel c's Dirichlet constant where the walk ended on constant data (walk_finish)
    const float g = (NC > 1 && own_g) ? gch.g[c] : term;
    total[(int64_t)c * T + t] = thr_end * g + tneu + tsrc[c];
    first[(int64_t)c * T + t] = fst[c];
  }
}

template __global__ void wos_tape_replay_kernel<1>(const DevTape, const uint32_t*, const float*, uint32_t, int, int,
                                                   const TapeChannels, int64_t, float*, float*);
template __global__ void wos_tape_replay_kernel<kMaxChannels>(const DevTape, const uint32_t*, const float*, uint32_t,
                                                              int, int, const TapeChannels, int64_t, float*, float*);

hipError_t launch_tape_replay(const DevTape& tape, const uint32_t* code, const DevScene& sc, int ignore_source,
                              int64_t T, float* total, float* first, hipStream_t s) {
  if (T < 1) return hipSuccess;
  const int64_t grid = (T + kBlock - 1) / kBlock;
  if (grid > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  int64_t cells = 1;
  for (int k = 0; k < (sc.dim == 2 ? 2 : 3); k++) cells *= sc.sdims[k];
  if (cells < 0 || cells > 0xFFFFFFFFLL) return hipErrorInvalidValue;
  TapeChannels gch;
  for (int c = 0; c < kMaxChannels; c++) gch.g[c] = sc.g_ch[c];
  if (sc.n_channels > 1)
    hipLaunchKernelGGL(wos_tape_replay_kernel<kMaxChannels>, dim3((unsigned)grid), dim3(kBlock), 0, s, tape, code,
                       sc.source, (uint32_t)cells, ignore_source, sc.n_channels, gch, T, total, first);
  else
    hipLaunchKernelGGL(wos_tape_replay_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, s, tape, code, sc.source,
                       (uint32_t)cells, ignore_source, 1, gch, T, total, first);
  return hipGetLastError();
}

// ---- adjoint (wos_tape_vjp) ---------------------------------------------------------------
// Replay + fold are an affine map from the source grid to (p, grad p); these two kernels apply its
// transpose to an upstream (P, G).  With R the recorded records of a point, N = |R|, nb(j) the
// recorded walks before j's pair and cvb_j / cvs_j the averages of total / first over them
// (0 without control variates or with nb(j) = 0), the fold computes
//   p   = (1/N) sum_R total_j
//   g_k = (1/N) sum_R [(total_j - first_j - cvb_j) b_jk + (first_j - cvs_j) s_jk]
// so with B_j = sum_k G_k b_jk, S_j = sum_k G_k s_jk:
//   a_j = dL/dtotal_j          = (1/N) [P + B_j - cv sum_{r in R, pair(r) > pair(j)} B_r / nb(r)]
//   c_j = dL/dfirst_j + a_j    = (1/N) [S_j - cv sum_{r in R, pair(r) > pair(j)} S_r / nb(r)] + (a_j - B_j / N)
// (first enters total with weight 1), and the replay's transpose scatters
//   out[cell0_j] += c_j gnorm_j,   out[cell_e] += a_j (thr_e nrm_e)  for every entry e of walk j.
//
// wos_tape_adjoint_fold_kernel: quad lane ch of point pp runs channel ch's sweep -- forward over
// the codes for N, then backward over the records, pair by pair, carrying the two suffix sums.
// code, bdir and sdir come through LDS in chunks of kAdjChunk records as in the fold, a and c
// leave through LDS the same way.  The sums are kept in double and rounded once into a / c.
constexpr int kAdjPoints = 32;  // points per 128-thread block
constexpr int kAdjChunk = 16;

template <int DIM>
__global__ __launch_bounds__(4 * kAdjPoints) void wos_tape_adjoint_fold_kernel(
    const uint32_t* __restrict__ code, const float* __restrict__ bdir, const float* __restrict__ sdir,
    const int32_t* __restrict__ pstate, int64_t n, int64_t T, int wpp, int n_anti, int use_cv, int n_channels,
    const float* __restrict__ up_p, const float* __restrict__ up_g, int64_t up_stride, float* __restrict__ a_out,
    float* __restrict__ c_out) {
  constexpr int NF = 1 + 2 * DIM;  // code | bdir[DIM] | sdir[DIM]
  constexpr int CH = kAdjChunk, LD = CH + 1, NT = 4 * kAdjPoints;
  __shared__ float lds[NF][kAdjPoints][LD];
  __shared__ float s_out[2 * kMaxChannels][kAdjPoints][LD];
  __shared__ int s_n[kAdjPoints];
  const int tid = threadIdx.x;
  const int ch = tid & 3, pp = tid >> 2;
  const int64_t p0 = (int64_t)blockIdx.x * kAdjPoints;
  const int nb = (int)((n - p0) < kAdjPoints ? (n - p0) : kAdjPoints);
  const int64_t i = p0 + pp;
  const int ps = pp < nb ? pstate[i] : 0;
  const bool live = pp < nb && ch < n_channels && (ps & kPtEstimate) != 0;
  // N: the block's tasks are contiguous, [p0 * wpp, (p0 + nb) * wpp)
  if (tid < kAdjPoints) s_n[tid] = 0;
  __syncthreads();
  for (int e = tid; e < nb * wpp; e += NT)
    if (code[p0 * wpp + e] & 1u) atomicAdd(&s_n[e / wpp], 1);
  __syncthreads();
  const int N = s_n[pp];
  // upstream, read as 0 where the forward masks the output
  double P = 0.0, G[DIM];
  for (int k = 0; k < DIM; k++) G[k] = 0.0;
  if (live && N > 0) {
    if (up_p && !(ps & kPtMaskP)) P = (double)up_p[(int64_t)ch * up_stride + i];
    if (up_g && !(ps & kPtMaskG))
      for (int k = 0; k < DIM; k++) G[k] = (double)up_g[((int64_t)ch * up_stride + i) * DIM + k];
  }
  const double inv_n = N > 0 ? 1.0 / (double)N : 0.0;
  double suf_b = 0.0, suf_s = 0.0;    // sum over the recorded walks of later pairs of B_r / nb(r), S_r / nb(r)
  double pend_b = 0.0, pend_s = 0.0;  // the current pair's B_r, S_r
  int pend_n = 0, after = 0;          // recorded walks of the current pair, of later pairs
  const int last = ((wpp - 1) / CH) * CH;
  for (int c0 = last; c0 >= 0; c0 -= CH) {
    const int cnt = (wpp - c0) < CH ? (wpp - c0) : CH;
    for (int e = tid; e < nb * CH; e += NT) {
      const int q = e / CH, j = e - q * CH;
      if (j >= cnt) continue;
      const int64_t t = (p0 + q) * wpp + c0 + j;
      lds[0][q][j] = __uint_as_float(code[t]);
      for (int k = 0; k < DIM; k++) {
        lds[1 + k][q][j] = bdir[k * T + t];
        lds[1 + DIM + k][q][j] = sdir[k * T + t];
      }
    }
    __syncthreads();
    if (pp < nb && ch < n_channels) {
      for (int j = cnt - 1; j >= 0; j--) {
        float a = 0.0f, c = 0.0f;
        if (live && N > 0 && (__float_as_uint(lds[0][pp][j]) & 1u)) {
          double B = 0.0, S = 0.0;
          for (int k = 0; k < DIM; k++) {
            B += G[k] * (double)lds[1 + k][pp][j];
            S += G[k] * (double)lds[1 + DIM + k][pp][j];
          }
          const double ad = inv_n * (P + B - suf_b);
          a = (float)ad;
          c = (float)(inv_n * (S - suf_s) + (ad - B * inv_n));
          pend_b += B;
          pend_s += S;
          pend_n += 1;
        }
        s_out[ch][pp][j] = a;
        s_out[kMaxChannels + ch][pp][j] = c;
        if ((c0 + j) % n_anti == 0) {  // the pair is complete: it joins the suffix of the pairs before it
          const int nbef = N - after - pend_n;
          if (use_cv && nbef > 0) {
            suf_b += pend_b / (double)nbef;
            suf_s += pend_s / (double)nbef;
          }
          after += pend_n;
          pend_b = 0.0; pend_s = 0.0; pend_n = 0;
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < nb * CH; e += NT) {
      const int q = e / CH, j = e - q * CH;
      if (j >= cnt) continue;
      const int64_t t = (p0 + q) * wpp + c0 + j;
      for (int cc = 0; cc < n_channels; cc++) {
        a_out[(int64_t)cc * T + t] = s_out[cc][q][j];
        c_out[(int64_t)cc * T + t] = s_out[kMaxChannels + cc][q][j];
      }
    }
    // the next chunk's staging writes lds / s_out only after every thread has passed the barrier
    // above and finished this copy-out of its own elements; its readers wait at the next barrier
    __syncthreads();
  }
}

template __global__ void wos_tape_adjoint_fold_kernel<2>(const uint32_t*, const float*, const float*, const int32_t*,
                                                         int64_t, int64_t, int, int, int, int, const float*,
                                                         const float*, int64_t, float*, float*);
template __global__ void wos_tape_adjoint_fold_kernel<3>(const uint32_t*, const float*, const float*, const int32_t*,
                                                         int64_t, int64_t, int, int, int, int, const float*,
                                                         const float*, int64_t, float*, float*);

hipError_t launch_tape_adjoint_fold(int dim, const DevParams& prm, const uint32_t* code, const float* bdir,
                                    const float* sdir, const int32_t* pstate, int64_t n, int64_t T, int wpp,
                                    int n_channels, const float* up_p, const float* up_g, int64_t up_stride,
                                    float* a, float* c, hipStream_t s) {
  if (n < 1) return hipSuccess;
  if (n_channels < 1 || n_channels > kMaxChannels || (int64_t)kAdjPoints * wpp > 0x7FFFFFFFLL)
    return hipErrorInvalidValue;
  const int64_t grid = (n + kAdjPoints - 1) / kAdjPoints;
  if (grid > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  const int use_cv = prm.use_cv ? 1 : 0;
  if (dim == 2)
    hipLaunchKernelGGL(wos_tape_adjoint_fold_kernel<2>, dim3((unsigned)grid), dim3(4 * kAdjPoints), 0, s, code, bdir,
                       sdir, pstate, n, T, wpp, (int)prm.n_anti, use_cv, n_channels, up_p, up_g, up_stride, a, c);
  else if (dim == 3)
    hipLaunchKernelGGL(wos_tape_adjoint_fold_kernel<3>, dim3((unsigned)grid), dim3(4 * kAdjPoints), 0, s, code, bdir,
                       sdir, pstate, n, T, wpp, (int)prm.n_anti, use_cv, n_channels, up_p, up_g, up_stride, a, c);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// wos_tape_scatter_kernel: the replay with the read turned into a write.  One lane per task, a
// wave per 64 consecutive tasks, the wave's contiguous slot range in chunks of kTapeChunk.  Per
// chunk every lane writes its walk's a into the LDS slots of its own entries (slots no walk
// filled keep 0); then the lane that owns entry e loads cell, pThr and pNrm coalesced and adds
// a * (pThr * pNrm) to out[channel][cell] with the hardware float atomic (global_atomic_add_f32,
// no return value), runs of equal cells in adjacent lanes first summed in registers.  The
// task's lane adds the first-ball term c * gnorm at cell0.  out is planar [C][cells], the
// caller's layout.  The kernel is bound by the atomics' rate (19 - 20 G terms/s on B, C and D alike,
// hot cells or not: profiles/tape_vjp_timing.jsonl); the run pre-combine bought 1 - 7 %.
template <int NC>
__global__ __launch_bounds__(kBlock) void wos_tape_scatter_kernel(const DevTape tp, const uint32_t* __restrict__ code,
                                                                  uint32_t cells, int n_channels, int64_t T,
                                                                  const float* __restrict__ a_in,
                                                                  const float* __restrict__ c_in,
                                                                  float* __restrict__ out) {
  __shared__ float s_a[kBlock / kWave][kTapeChunk * NC];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t - lane >= T) return;  // the whole wave is beyond the tasks
  const bool valid = t < T;
  const uint32_t cd = valid ? code[t] : 0u;
  const bool rec = (cd & 1u) != 0u;
  const uint32_t s0 = valid ? tp.slot[t] : 0u;
  const uint32_t cap = valid ? tp.slot[t + 1] - s0 : 0u;
  uint32_t n = rec ? tp.cnt[t] & ~kTapeOwnG : 0u;
  n = n < cap ? n : cap;
  float a[NC];
  for (int c = 0; c < NC; c++) a[c] = 0.0f;
  if (rec) {
    const float gnorm = tp.gnorm[t];
    const uint32_t cell = tp.cell0[t];
    for (int c = 0; c < NC; c++) {
      if (c >= n_channels) break;
      a[c] = a_in[(int64_t)c * T + t];
      const float v = c_in[(int64_t)c * T + t] * gnorm;
      if (cell < cells && v != 0.0f) unsafeAtomicAdd(&out[(size_t)c * cells + cell], v);
    }
  }
  const uint32_t e0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s0);
  uint32_t e1 = rec ? s0 + n : e0;
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)e1, off);
    e1 = o > e1 ? o : e1;
  }
  for (uint32_t w0 = e0; w0 < e1; w0 += kTapeChunk) {
    for (int c = 0; c < NC; c++) s_a[wave][lane * NC + c] = 0.0f;
    wave_sync();
    const uint32_t lo = s0 > w0 ? s0 : w0;
    const uint32_t hi = s0 + n < w0 + kTapeChunk ? s0 + n : w0 + kTapeChunk;
    for (uint32_t j = lo; j < hi; j++) {
      const uint32_t k = j - w0;
      for (int c = 0; c < NC; c++) s_a[wave][k * NC + c] = a[c];
    }
    wave_sync();
    const uint32_t e = w0 + (uint32_t)lane;
    // consecutive steps of a walk often sample the same cell: a run of equal cells in adjacent
    // lanes is summed into its first lane (segmented suffix scan), one atomic per run
    uint32_t cell = 0xFFFFFFFFu;
    float v[NC];
    for (int c = 0; c < NC; c++) v[c] = 0.0f;
    if (e < e1) {
      cell = tp.e_cell[e];
      const float w = tp.e_thr[e] * tp.e_nrm[e];
      for (int c = 0; c < NC; c++) v[c] = s_a[wave][lane * NC + c] * w;
    }
    const uint32_t prev = (uint32_t)__shfl_up((int)cell, 1);
    const bool head = lane == 0 || prev != cell;
    const unsigned long long heads = __ballot(head);
    const int run = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));  // the run's first lane
    for (int off = 1; off < kWave; off <<= 1) {
      const int orun = __shfl_down(run, off);
      for (int c = 0; c < NC; c++) {
        const float o = __shfl_down(v[c], off);
        if (lane + off < kWave && orun == run) v[c] += o;
      }
    }
    if (head && cell < cells)
      for (int c = 0; c < NC; c++) {
        if (c >= n_channels) break;
        if (v[c] != 0.0f) unsafeAtomicAdd(&out[(size_t)c * cells + cell], v[c]);
      }
    wave_sync();
  }
}

template __global__ void wos_tape_scatter_kernel<1>(const DevTape, const uint32_t*, uint32_t, int, int64_t, const float*,
                                                    const float*, float*);
template __global__ void wos_tape_scatter_kernel<kMaxChannels>(const DevTape, const uint32_t*, uint32_t, int, int64_t,
                                                               const float*, const float*, float*);

hipError_t launch_tape_scatter(const DevTape& tape, const uint32_t* code, int64_t cells, int n_channels, int64_t T,
                               const float* a, const float* c, float* out, hipStream_t s) {
  if (T < 1) return hipSuccess;
  const int64_t grid = (T + kBlock - 1) / kBlock;
  if (grid > 0x7FFFFFFFLL || cells < 1 || cells > 0xFFFFFFFFLL || n_channels < 1 || n_channels > kMaxChannels)
    return hipErrorInvalidValue;
  if (n_channels > 1)
    hipLaunchKernelGGL(wos_tape_scatter_kernel<kMaxChannels>, dim3((unsigned)grid), dim3(kBlock), 0, s, tape, code,
                       (uint32_t)cells, n_channels, T, a, c, out);
  else
    hipLaunchKernelGGL(wos_tape_scatter_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, s, tape, code, (uint32_t)cells,
                       1, T, a, c, out);
  return hipGetLastError();
}

}  // namespace wos
