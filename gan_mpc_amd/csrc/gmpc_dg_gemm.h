// The two-halves fp32 matrix-core GEMM of the row kernels: k_dyn_rows (gmpc_dyn_grads.hip) and k_cem_rollout
// (gmpc_cem.hip) include it.
#pragma once
#include "gmpc_launch.h"

#define GMPC_DG_THREADS 256
#define GMPC_DG_LDA 260          // LDS row stride of the row kernels' activations (widths <= 256, + 4)

// One 16 x 16 output tile per (wave, column tile) for each of the two row halves: rows 0..15 of the LDS operand are
// the primal rows (forward) / w deltas (backward) of the workgroup's 16 steps, rows 16..31 the tangent rows /
// lam deltas.  v_mfma_f32_16x16x4_f32: lane l supplies A[l & 15][k0 + (l >> 4)] and B[k0 + (l >> 4)][j0 + (l & 15)],
// and holds D[4 (l >> 4) + r][j0 + (l & 15)] in register r.  B is the layer's weight matrix ([K][N] row-major: W_l
// forward, W_l^T backward) read from global memory (L2-resident).  Widths up to 256: at most 16 column tiles, four
// per wave.
struct DgTiles {
  f32x4_t p[4], q[4];   // column tile c = wave + 4 i: primal / tangent half
};

__device__ __forceinline__ void dg_gemm(const float* A, int K, int N, const float* __restrict__ Wg, int wave,
                                        int lane, DgTiles& acc) {
  const int l16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc.p[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    acc.q[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const int nct = (N + 15) >> 4;
  // the column of each of this wave's tiles (past N: a valid column whose product is discarded)
  int col[4];
  bool on[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (wave + 4 * i) * 16 + l16;
    on[i] = wave + 4 * i < nct;
    col[i] = j < N ? j : N - 1;
  }
  const float* pa = A + l16 * GMPC_DG_LDA;
  const float* qa = A + (16 + l16) * GMPC_DG_LDA;
  int k0 = 0;
  for (; k0 + 8 <= K; k0 += 8) {
    float w0[4], w1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w0[i] = on[i] ? Wg[(size_t)(k0 + kq) * N + col[i]] : 0.f;
      w1[i] = on[i] ? Wg[(size_t)(k0 + 4 + kq) * N + col[i]] : 0.f;
    }
    const float a0 = pa[k0 + kq], b0 = qa[k0 + kq], a1 = pa[k0 + 4 + kq], b1 = qa[k0 + 4 + kq];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!on[i]) continue;
      acc.p[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w0[i], acc.p[i], 0, 0, 0);
      acc.q[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0, w0[i], acc.q[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!on[i]) continue;
      acc.p[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, w1[i], acc.p[i], 0, 0, 0);
      acc.q[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1, w1[i], acc.q[i], 0, 0, 0);
    }
  }
  for (; k0 < K; k0 += 4) {
    const int k = k0 + kq;
    const bool kin = k < K;
    float w0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w0[i] = on[i] && kin ? Wg[(size_t)k * N + col[i]] : 0.f;
    const float a0 = kin ? pa[k] : 0.f, b0 = kin ? qa[k] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!on[i]) continue;
      acc.p[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w0[i], acc.p[i], 0, 0, 0);
      acc.q[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0, w0[i], acc.q[i], 0, 0, 0);
    }
  }
  mfma_fence<false>(acc.p[0], acc.p[1], acc.p[2], acc.p[3], acc.q[0], acc.q[1], acc.q[2], acc.q[3]);
}
