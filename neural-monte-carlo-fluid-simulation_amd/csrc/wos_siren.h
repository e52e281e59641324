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

// floats of the fragment-ordered copy of the L hidden weight matrices (0 for L = 0)
inline size_t siren_pack_floats(int H, int L) { return (size_t)L * H * H; }

// Rewrites hidden layer l's W [H][H] as packed[l][r][q][lane][e] = W[32 r + (lane & 31)][8 q + 2 e + (lane >> 5)]:
// the A operand of k-step 4 q + e of row tile r, one 16-byte load per lane and four k-steps.
hipError_t launch_siren_pack(const SirenNet& net, float* packed, hipStream_t s);

// u [n][d_out], jac [n][d_out][d_in], div [n]: each may be null.  packed: launch_siren_pack's.
hipError_t launch_siren_eval(const SirenNet& net, const float* packed, const float* pts, int64_t n, float* u,
                             float* jac, float* div, hipStream_t s);

// The hidden-layer GEMM of launch_siren_eval alone (the same device function): Z[p][0] = W X[p][0] + b,
// Z[p][s] = W X[p][s] for s = 1 .. d_in; X and Z [n][1 + d_in][H]; packed: H * H floats of scratch.
hipError_t launch_siren_layer_selftest(int H, int d_in, int64_t n, const float* W, const float* b, float* packed,
                                       const float* X, float* Z, hipStream_t s);

}  // namespace wos
