// wos_siren_device.h -- device pieces shared by the fused SIREN forward (wos_siren.hip) and its
// backward (wos_siren_vjp.hip): the accumulator lane map and the hidden-layer product.
#pragma once
#include "wos_siren.h"

namespace wos {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// row, within its 32-row tile, of accumulator register `reg` of `lane` (the column is lane & 31)
__device__ __forceinline__ int siren_acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// One hidden layer's pre-activations of this wave's row tiles r = wave + 4 i (i < RT), for the C
// column tiles of Xl [H][C * 32] (LDS): acc[i][0] = W X_0 + b, acc[i][c] = W X_c.  Wp: the layer's
// fragment-ordered weights (launch_siren_pack).  Every chain starts from 0 and the bias is added to
// the finished sum, one rounding: a chain started from the bias rounds each of its H partial sums at
// the bias's magnitude, which at small H is several times the sum's own.  Row tiles past H / 32
// compute a duplicate of the last one, which the caller drops.  No barrier inside.
template <int C, int RT>
__device__ __forceinline__ void siren_hidden_gemm(const float4* __restrict__ Wp, const float* __restrict__ bias,
                                                  const float* Xl, int H, int wave, int lane, f32x16 (&acc)[RT][C]) {
  constexpr int cols = C * 32;
  const int R = H >> 5, Q = H >> 3;
  const float4* wp[RT];
#pragma unroll
  for (int i = 0; i < RT; i++) {
    const int r = min(wave + 4 * i, R - 1);
    wp[i] = Wp + (size_t)r * Q * 64 + lane;
#pragma unroll
    for (int reg = 0; reg < 16; reg++)
#pragma unroll
      for (int c = 0; c < C; c++) acc[i][c][reg] = 0.0f;
  }
  const float* xb = Xl + (lane >> 5) * cols + (lane & 31);
  float4 a[RT];
#pragma unroll
  for (int i = 0; i < RT; i++) a[i] = wp[i][0];
  for (int q = 0; q < Q; q++) {
    float4 an[RT];
    const int qn = min(q + 1, Q - 1);
#pragma unroll
    for (int i = 0; i < RT; i++) an[i] = wp[i][(size_t)qn * 64];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      float bv[C];
#pragma unroll
      for (int c = 0; c < C; c++) bv[c] = xb[(8 * q + 2 * e) * cols + c * 32];
#pragma unroll
      for (int i = 0; i < RT; i++) {
        const float av = e == 0 ? a[i].x : e == 1 ? a[i].y : e == 2 ? a[i].z : a[i].w;
#pragma unroll
        for (int c = 0; c < C; c++) acc[i][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[c], acc[i][c], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < RT; i++) a[i] = an[i];
  }
  // the bias as one more k-step of column tile 0: A = (b[row], 0), B = (1, 0), so every element takes
  // fma(b[row], 1, z) = z + b[row], rounded once, and the second k adds an exact zero
  const float one = lane < 32 ? 1.0f : 0.0f;
#pragma unroll
  for (int i = 0; i < RT; i++) {
    const int r = min(wave + 4 * i, R - 1);
    const float bv = lane < 32 ? bias[r * 32 + lane] : 0.0f;
    acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv, one, acc[i][0], 0, 0, 0);
  }
}

}  // namespace wos
