// wos_tape_index.hip -- the walk tape's cell-sorted index (wos_tape_index_build) and the
// atomic-free sum of the adjoint over it (wos_tape_vjp_indexed).
//
// The replay's transpose adds, per segment, one term per recorded first ball (c_j gnorm_j at
// cell0_j) and one per filled entry (a_j (thr_e nrm_e) at cell_e).  wos_tape_scatter_kernel adds
// them with float atomics, in whatever order the hardware serves them.  The index is that term
// list stably sorted by cell -- per term the cell, an id (the task; bit 31: take c_j, not a_j) and
// the weight w, per cell a row offset -- built once per tape: an enumeration kernel in the
// canonical order (first balls by task, then entries by slot), a stable radix sort over the
// bits of the cell (rocPRIM), row offsets from the sorted keys.
//
// wos_tape_rowsum_kernel then streams the terms once.  A wave owns one tile of kTapeIndexTile
// consecutive terms, whatever rows they belong to, so the work is balanced over terms and a row
// of ten thousand terms costs no more than ten tiles.  Rows inside a tile are written by that
// wave; a row that crosses tiles leaves one partial per tile, and wos_tape_rowsum_cross_kernel
// adds them in tile order.  No atomics: every cell has exactly one writer per segment.
//
// The order of the float additions, a pure function of the row offsets and kTapeIndexTile
// (tests/tape_index_model.py restates it):
//   1. v_i = fl(x_i w_i) per term, x = a or c of the term's task;
//   2. per chunk of 64 consecutive terms (chunks start at multiples of 64 of the segment's term
//      index): for off = 1, 2, 4, 8, 16, 32, every lane l with l + off < 64 whose term l + off
//      is of the same row does v_l = fl(v_l + v_{l + off}), all lanes at once from the values
//      of the step before; the first lane of a row's run then holds the piece (row, chunk);
//   3. per tile a row's pieces are added in chunk order, s = fl(s + piece);
//   4. a row's tile sums are added in tile order, s = fl(s + tile sum);
//   5. out[cell] = fl(out[cell] + s), segment after segment.
// All in float: a double partial would cost the streaming kernel twice the registers for bits
// the float atomic path never had either.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "wos_launch.h"

namespace wos {

namespace {
constexpr int kLanes = 64;
constexpr uint32_t kNoCell = 0xFFFFFFFFu;  // the key of an absent term: sorts behind every cell
constexpr uint32_t kTile = (uint32_t)kTapeIndexTile;
static_assert(kTapeIndexTile % kLanes == 0, "a tile is whole chunks");
}  // namespace

// ---- build ------------------------------------------------------------------------------
// Element i of the enumeration: i < T the first ball of task i, else entry slot i - T.  The
// slot's task is the last t with slot[t] <= e (tasks without slots repeat their neighbour's
// offset).  val = w's bits << 32 | id.
__global__ __launch_bounds__(256) void wos_tape_index_enum_kernel(const DevTape tp, const uint32_t* __restrict__ code,
                                                                  int64_t T, int64_t slots, uint32_t cells,
                                                                  uint32_t* __restrict__ key,
                                                                  unsigned long long* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T + slots) return;
  uint32_t k = kNoCell, id = 0u;
  float w = 0.0f;
  if (i < T) {
    if (code[i] & 1u) {
      const uint32_t cell = tp.cell0[i];
      if (cell < cells) { k = cell; id = (uint32_t)i | 0x80000000u; w = tp.gnorm[i]; }
    }
  } else {
    const uint32_t e = (uint32_t)(i - T);
    int64_t lo = 0, hi = T;  // slot[lo] <= e < slot[hi] (slot[0] = 0, slot[T] = slots)
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (tp.slot[mid] <= e) lo = mid; else hi = mid;
    }
    if (code[lo] & 1u) {
      const uint32_t s0 = tp.slot[lo], cap = tp.slot[lo + 1] - s0;
      uint32_t n = tp.cnt[lo] & ~kTapeOwnG;
      n = n < cap ? n : cap;
      if (e - s0 < n) {  // a slot the walk filled
        const uint32_t cell = tp.e_cell[e];
        if (cell < cells) { k = cell; id = (uint32_t)lo; w = tp.e_thr[e] * tp.e_nrm[e]; }
      }
    }
  }
  key[i] = k;
  val[i] = ((unsigned long long)__float_as_uint(w) << 32) | id;
}

// the sorted keys' terms: the position of the first absent one
__global__ __launch_bounds__(256) void wos_tape_index_count_kernel(const uint32_t* __restrict__ key, int64_t N,
                                                                   uint32_t* __restrict__ n_terms) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > N) return;
  const bool before = i == 0 || key[i - 1] != kNoCell;
  const bool here = i == N || key[i] == kNoCell;
  if (before && here) *n_terms = (uint32_t)i;
}

// cell / id / w of the sorted terms, and the row offsets: element i starts every row in
// (key[i - 1], key[i]]; i = n_terms closes the rows behind the last term, row[cells] = n_terms
__global__ __launch_bounds__(256) void wos_tape_index_finish_kernel(const uint32_t* __restrict__ key,
                                                                    const unsigned long long* __restrict__ val,
                                                                    uint32_t n_terms, uint32_t cells,
                                                                    uint32_t* __restrict__ row,
                                                                    uint32_t* __restrict__ cell,
                                                                    uint32_t* __restrict__ id, float* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > (int64_t)n_terms) return;
  if (i < (int64_t)n_terms) {
    const unsigned long long v = val[i];
    cell[i] = key[i];
    id[i] = (uint32_t)v;
    w[i] = __uint_as_float((uint32_t)(v >> 32));
  }
  const int64_t lo = i == 0 ? 0 : (int64_t)key[i - 1] + 1;
  const int64_t hi = i == (int64_t)n_terms ? (int64_t)cells : (int64_t)key[i];
  for (int64_t r = lo; r <= hi; r++) row[r] = (uint32_t)i;
}

hipError_t launch_tape_index_enum(const DevTape& tape, const uint32_t* code, int64_t T, int64_t slots, int64_t cells,
                                  uint32_t* key, unsigned long long* val, hipStream_t s) {
  const int64_t N = T + slots;
  if (N < 1) return hipSuccess;
  const int64_t grid = (N + 255) / 256;
  if (grid > 0x7FFFFFFFLL || cells < 1 || cells >= 0xFFFFFFFFLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wos_tape_index_enum_kernel, dim3((unsigned)grid), dim3(256), 0, s, tape, code, T, slots,
                     (uint32_t)cells, key, val);
  return hipGetLastError();
}

hipError_t tape_index_sort(void* temp, size_t* temp_bytes, const uint32_t* key_in, uint32_t* key_out,
                           const unsigned long long* val_in, unsigned long long* val_out, int64_t N, int bits,
                           hipStream_t s) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, key_in, key_out, val_in, val_out, (size_t)N, 0u, (unsigned)bits,
                                   s);
}

hipError_t launch_tape_index_count(const uint32_t* key, int64_t N, uint32_t* n_terms, hipStream_t s) {
  const int64_t grid = (N + 1 + 255) / 256;
  if (grid > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wos_tape_index_count_kernel, dim3((unsigned)grid), dim3(256), 0, s, key, N, n_terms);
  return hipGetLastError();
}

hipError_t launch_tape_index_finish(const uint32_t* key, const unsigned long long* val, uint32_t n_terms,
                                    int64_t cells, uint32_t* row, uint32_t* cell, uint32_t* id, float* w,
                                    hipStream_t s) {
  const int64_t grid = ((int64_t)n_terms + 1 + 255) / 256;
  if (grid > 0x7FFFFFFFLL || cells < 1 || cells >= 0xFFFFFFFFLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wos_tape_index_finish_kernel, dim3((unsigned)grid), dim3(256), 0, s, key, val, n_terms,
                     (uint32_t)cells, row, cell, id, w);
  return hipGetLastError();
}

// ---- sum --------------------------------------------------------------------------------
// One wave per tile, one term per lane and chunk.  The row still open at a chunk's end is carried
// (wave-uniform) into the next chunk; a closed row goes to out if the tile holds all of it, else
// to the tile's partial: part[tile][0] the row that began before the tile, [1] the one that
// began in it and goes on behind it.
template <int NC>
__global__ __launch_bounds__(256) void wos_tape_rowsum_kernel(const DevTapeIndex ix, uint32_t cells, int n_channels,
                                                              int64_t T, const float* __restrict__ a_in,
                                                              const float* __restrict__ c_in,
                                                              float* __restrict__ out) {
  const int lane = threadIdx.x & (kLanes - 1);
  const uint64_t tile = (uint64_t)blockIdx.x * (256 / kLanes) + threadIdx.x / kLanes;
  const uint64_t t0 = tile * kTile;
  if (t0 >= ix.n_terms) return;
  const uint64_t t1 = t0 + kTile < ix.n_terms ? t0 + kTile : ix.n_terms;

  auto emit = [&](uint32_t cell, const float* v) {
    if (cell >= cells) return;  // the padding behind the last term
    const uint64_t rs = ix.row[cell], re = ix.row[cell + 1];
    if (rs >= t0 && re <= t0 + kTile) {
      for (int c = 0; c < NC; c++) {
        if (c >= n_channels) break;
        const size_t o = (size_t)c * cells + cell;
        out[o] = out[o] + v[c];  // this wave is the cell's only writer
      }
    } else {
      float* p = ix.part + (tile * 2 + (rs < t0 ? 0 : 1)) * kMaxChannels;
      for (int c = 0; c < NC; c++) p[c] = v[c];
    }
  };

  bool carry_on = false;
  uint32_t carry_cell = kNoCell;
  float carry[NC];
  for (int c = 0; c < NC; c++) carry[c] = 0.0f;
  for (uint64_t b = t0; b < t1; b += kLanes) {
    const uint64_t i = b + lane;
    uint32_t cell = kNoCell;
    float v[NC];
    for (int c = 0; c < NC; c++) v[c] = 0.0f;
    if (i < ix.n_terms) {
      cell = ix.cell[i];
      const uint32_t id = ix.id[i];
      const float w = ix.w[i];
      const float* src = (id >> 31) ? c_in : a_in;
      const int64_t t = (int64_t)(id & 0x7FFFFFFFu);
      for (int c = 0; c < NC; c++) {
        if (c >= n_channels) break;
        v[c] = src[(int64_t)c * T + t] * w;
      }
    }
    for (int off = 1; off < kLanes; off <<= 1) {
      const uint32_t ocell = (uint32_t)__shfl_down((int)cell, off);
      const bool same = lane + off < kLanes && ocell == cell;
      for (int c = 0; c < NC; c++) {
        const float o = __shfl_down(v[c], off);
        if (same) v[c] = v[c] + o;
      }
    }
    const uint32_t prev = (uint32_t)__shfl_up((int)cell, 1);
    const bool head = lane == 0 || prev != cell;
    const int last = 63 - __builtin_clzll(__ballot(head));  // the first lane of the chunk's last run
    if (lane == 0 && carry_on) {
      if (cell == carry_cell) {
        for (int c = 0; c < NC; c++) v[c] = carry[c] + v[c];
      } else {
        emit(carry_cell, carry);
      }
    }
    if (head && lane != last) emit(cell, v);
    carry_cell = (uint32_t)__shfl((int)cell, last);
    for (int c = 0; c < NC; c++) carry[c] = __shfl(v[c], last);
    carry_on = true;
  }
  if (lane == 0 && carry_on) emit(carry_cell, carry);
}

template __global__ void wos_tape_rowsum_kernel<1>(const DevTapeIndex, uint32_t, int, int64_t, const float*,
                                                   const float*, float*);
template __global__ void wos_tape_rowsum_kernel<kMaxChannels>(const DevTapeIndex, uint32_t, int, int64_t, const float*,
                                                              const float*, float*);

// One thread per tile boundary b (at term b kTile): if a row crosses it and this is the first
// boundary the row crosses, the thread adds the row's partials in tile order and owns the cell.
__global__ __launch_bounds__(256) void wos_tape_rowsum_cross_kernel(const DevTapeIndex ix, uint32_t cells,
                                                                    int n_channels, float* __restrict__ out) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1;
  const uint64_t pos = b * kTile;
  if (pos >= ix.n_terms) return;
  const uint32_t cell = ix.cell[pos];
  if (cell >= cells || ix.cell[pos - 1] != cell) return;
  const uint64_t rs = ix.row[cell], re = ix.row[cell + 1];
  const uint64_t k0 = rs / kTile, k1 = (re - 1) / kTile;
  if (b != k0 + 1) return;
  for (int c = 0; c < n_channels; c++) {
    float acc = ix.part[(k0 * 2 + 1) * kMaxChannels + c];
    for (uint64_t k = k0 + 1; k <= k1; k++) acc = acc + ix.part[(k * 2 + 0) * kMaxChannels + c];
    const size_t o = (size_t)c * cells + cell;
    out[o] = out[o] + acc;
  }
}

hipError_t launch_tape_rowsum(const DevTapeIndex& ix, int64_t cells, int n_channels, int64_t T, const float* a,
                              const float* c, float* out, hipStream_t s) {
  if (ix.n_terms == 0) return hipSuccess;
  if (cells < 1 || cells >= 0xFFFFFFFFLL || n_channels < 1 || n_channels > kMaxChannels || T < 1)
    return hipErrorInvalidValue;
  const int64_t tiles = tape_index_tiles(ix.n_terms);
  const int64_t grid = (tiles + 3) / 4;
  if (n_channels > 1)
    hipLaunchKernelGGL(wos_tape_rowsum_kernel<kMaxChannels>, dim3((unsigned)grid), dim3(256), 0, s, ix, (uint32_t)cells,
                       n_channels, T, a, c, out);
  else
    hipLaunchKernelGGL(wos_tape_rowsum_kernel<1>, dim3((unsigned)grid), dim3(256), 0, s, ix, (uint32_t)cells, 1, T, a,
                       c, out);
  if (tiles > 1)
    hipLaunchKernelGGL(wos_tape_rowsum_cross_kernel, dim3((unsigned)((tiles - 1 + 255) / 256)), dim3(256), 0, s, ix,
                       (uint32_t)cells, n_channels, out);
  return hipGetLastError();
}

}  // namespace wos
