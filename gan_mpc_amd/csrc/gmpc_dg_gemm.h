// The two-halves fp32 matrix-core GEMM of the row kernels: k_dyn_rows (gmpc_dyn_grads.hip) and k_cem_rollout
// (gmpc_cem.hip) include it.  Below it, its bf16 counterpart for the sampled rollouts in bf16 mode.
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

// ---- the bf16 counterpart (the sampled rollouts in bf16 mode) ----------------------------
// v_mfma_f32_16x16x32_bf16: lane l supplies A[l & 15][k0 + 8 (l >> 4) + j] and B[k0 + 8 (l >> 4) + j][j0 + (l & 15)],
// j = 0..7 (16 bytes each), and holds D as above -- the C/D layout does not depend on the operand type, so the
// accumulators are DgTiles again.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// Row stride of the bf16 operand block, in elements: 528 bytes = 33 sixteen-byte slots.  ds_read_b128 serves a wave in
// four groups of 16 lanes, each 8 rows at one kq and the other 8 rows at kq + 1 (lanes {0-3, 12-15, 20-27}, ...), on
// 16 slots of 16 bytes (bank = (byte / 4) mod 64).  A lane's slot is (33 row + 2 k0 / 16 + kq) mod 16 = (row + kq +
// const) mod 16: the 16 rows of one kq fall on 16 different slots, and a group meets itself in one slot only (row 12
// at kq against row 11 at kq + 1), 2 cycles for 1.  No linear stride does better: the 8 slots of the second half would
// have to be the complement of the first half's and its own shift by one.  A stride of 256 + 0 would put all 16 rows on
// one slot.
#define GMPC_DG_LDH 264
// The packed weight image of one layer ([K][N] fp32 -> bf16, K padded to Kp = 32 ceil(K / 32), N to Np = 16 ceil(N /
// 16), zeros in the padding): element (k, j) at ((k >> 3) Np + j) 8 + (k & 7), so the 8 k-consecutive values of a lane
// are one 16-byte load and the 16 lanes of a kq read 256 contiguous bytes.
__host__ __device__ __forceinline__ int dg_kp(int K) { return (K + 31) & ~31; }
__host__ __device__ __forceinline__ int dg_np(int N) { return (N + 15) & ~15; }

// The products of a wave with NT column tiles (tile i at wp + 64 i): one k-step of 32 per turn, the next turn's
// weights requested before this turn's products issue; no branch around a product.  The fence stands at the end of
// EVERY turn, over the tiles that took part: there the accumulators are tied in the registers the loop carries them
// in.  Behind the loop hipcc rearranges them for what follows (the switch's join) BEFORE a fence placed there, right
// behind the last product (seen for NT = 2 with any operand order).  The wait overlaps the turn's last products,
// which hold the matrix pipe that long anyway.
template <int NT>
__device__ __forceinline__ void dg_gemm_bf16_tiles(const bf16x8_t* pa, const bf16x8_t* qa, const bf16x8_t* wp, int Kp,
                                                   int Np, DgTiles& acc) {
  bf16x8_t wn[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) wn[i] = wp[64 * i];
  for (int k0 = 0; k0 < Kp; k0 += 32) {
    bf16x8_t w[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) w[i] = wn[i];
    if (k0 + 32 < Kp) {
      const bf16x8_t* nx = wp + (size_t)((k0 + 32) >> 3) * Np;
#pragma unroll
      for (int i = 0; i < NT; ++i) wn[i] = nx[64 * i];
    }
    const bf16x8_t a0 = pa[k0 >> 3], b0 = qa[k0 >> 3];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      acc.p[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, w[i], acc.p[i], 0, 0, 0);
      acc.q[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b0, w[i], acc.q[i], 0, 0, 0);
    }
    if constexpr (NT == 4)
      mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1], acc.p[2], acc.q[2], acc.p[3], acc.q[3]);
    if constexpr (NT == 3) mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1], acc.p[2], acc.q[2]);
    if constexpr (NT == 2) mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1]);
    if constexpr (NT == 1) mfma_fence<true>(acc.p[0], acc.q[0]);
  }
}

// acc = A[32][Kp] (bf16, LDS, row stride GMPC_DG_LDH; columns K .. Kp-1 zero) * the packed image Wp of [Kp][Np]
__device__ __forceinline__ void dg_gemm_bf16(const __bf16* A, int Kp, int Np, const __bf16* __restrict__ Wp, int wave,
                                             int lane, DgTiles& acc) {
  const int l16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc.p[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    acc.q[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  // the wave's tiles are wave, wave + 4, ...: the first nt of its four (through a scalar register: a uniform switch)
  const int wu = __builtin_amdgcn_readfirstlane(wave), nct = Np >> 4;
  const int nt = nct > wu ? (nct - wu + 3) >> 2 : 0;
  // this lane's 16 bytes of k-step 0 of the wave's first tile; a tile on: 64 slots, a k-step on: 4 Np slots
  const bf16x8_t* wp = reinterpret_cast<const bf16x8_t*>(Wp) + (size_t)kq * Np + wu * 16 + l16;
  const bf16x8_t* pa = reinterpret_cast<const bf16x8_t*>(A + l16 * GMPC_DG_LDH) + kq;
  const bf16x8_t* qa = reinterpret_cast<const bf16x8_t*>(A + (16 + l16) * GMPC_DG_LDH) + kq;
  switch (nt) {
    case 4: dg_gemm_bf16_tiles<4>(pa, qa, wp, Kp, Np, acc); break;
    case 3: dg_gemm_bf16_tiles<3>(pa, qa, wp, Kp, Np, acc); break;
    case 2: dg_gemm_bf16_tiles<2>(pa, qa, wp, Kp, Np, acc); break;
    case 1: dg_gemm_bf16_tiles<1>(pa, qa, wp, Kp, Np, acc); break;
    default: break;     // (no tile: the zeros above)
  }
}
