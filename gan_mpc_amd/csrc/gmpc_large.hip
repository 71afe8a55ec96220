// Large-state path (n > 64: BASELINE configs C4 Humanoid n=376, C5 synthetic n=1024).
//
// The value matrix P of the Riccati recursion no longer fits a CU's LDS (565 KB at n=376, 4.2 MB at
// n=1024), and the per-step LQR blocks cannot all be materialised either (AB is 15 GB
// per GPU at C4, 460 GB at C5).  The backward pass therefore runs STEP-MAJOR: for t = T-1 .. 0, for
// the whole batch at once,
//     [A_t | B_t]  <- MFMA Jacobian chain on the samples (b, t)          (k_linearize_mfma, strided)
//     [PA | PB] = P [A | B]                 batched fp32-MFMA GEMMs      (gmpc_bgemm.hip: k_bgemm_tn_lds / k_bgemm_tn)
//     [H | Gr]  = B^T [PA | PB]                                          (k_bgemm_tn)
//     gains K_t k_t, adjoint, value vector, V = H + G K / 2               (gmpc_big_step.hip: k_big_step)
//     T1 = A^T (PA) + K^T V + V^T K   one GEMM over two K-segments, only the blocks that touch the
//                                     upper triangle                     (k_bgemm_tn_lds)
//     P <- Q_t + T1 (upper triangle, mirrored)                           (k_big_pupdate)
// K^T V + V^T K = K^T H + H^T K + K^T G K are the cross terms of trajax' lqr_step value update; written
// as [K; V]^T [V; K] the product is symmetric term by term, so -- like A^T P A with a symmetric P -- its
// two triangles differ only by rounding and the lower one need not be computed (half of the second
// n^3 product of every step).  trajax symmetrises the sum explicitly; the mirror gives the same
// exactly symmetric P up to that rounding.
// Every product is written as  C = sum_k X[k][:]^T Y[k][:]  ("TN") with row-major operands, so row k
// of X / Y IS the MFMA A / B operand of k-step k and all global reads are coalesced; P's symmetry
// turns P A into that form (X = P).  Reference arithmetic: trajax lqr_step / tvlqr / adjoint.
#include <cstdlib>
#include <cstring>

#include "gmpc_launch.h"
#include "gmpc_riccati_parts.h"

// P = Q_t + T1 on the upper triangle, mirrored into the lower one: tile (I, J) with I <= J (64 x 64) is read
// row-wise once and written twice (the transposed copy through LDS), so every global access is
// coalesced and P comes out exactly symmetric.  T1's strictly lower blocks are never read.
#define GMPC_PU_TILE 64
__global__ __launch_bounds__(GMPC_THREADS) void k_big_pupdate(int n, int ng, int T, int t, const float* X,
                                                              const float* goal, const float* mpc_w,
                                                              const float* sbuf, const float* T1,
                                                              const int* active, float* P) {
  constexpr int TS = GMPC_PU_TILE;
  __shared__ float tA[TS][TS + 1], dI[TS], dJ[TS];
  // blockIdx.x enumerates the tile pairs I <= J only (row I holds nt - I of them): a workgroup that returns at once
  // still waits for its dispatch slot behind the ones before it
  const int nt_ = (n + TS - 1) / TS, b = blockIdx.z;
  int I = 0, J = blockIdx.x;
  while (J >= nt_ - I) { J -= nt_ - I; ++I; }
  J += I;
  if (active != nullptr && active[b] == 0) return;
  const int tx = threadIdx.x & (TS - 1), ty = threadIdx.x / TS;      // 64 columns x 4 rows per sweep
  const size_t o = (size_t)b * n * n;
  const size_t xb = ((size_t)b * (T + 1) + t) * n, gb = ((size_t)b * (T + 1) + t) * ng;
  if (threadIdx.x < TS) {
    const int i = I * TS + tx;
    dI[tx] = i < ng ? X[xb + i] - goal[gb + i] : 0.f;
  } else if (threadIdx.x < 2 * TS) {
    const int j = J * TS + tx;
    dJ[tx] = j < ng ? X[xb + j] - goal[gb + j] : 0.f;
  }
  __syncthreads();
  const float w1 = sigmoidf_(mpc_w[1]);
  const float s = sbuf[b];
  const float is = 1.f / s, is3 = 1.f / (s * s * s);
  constexpr int RS = GMPC_THREADS / TS;
  float tv[TS / RS];
  // all the tile's reads first (16 per thread in flight), then the stores
#pragma unroll
  for (int q = 0; q < TS / RS; ++q) {
    const int r = ty + RS * q, i = I * TS + r, j = J * TS + tx;
    // diagonal tiles: take the element of the upper triangle for both (i, j) and (j, i)
    const size_t src = i <= j ? (size_t)i * n + j : (size_t)j * n + i;
    tv[q] = (i < n && j < n) ? T1[o + src] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < TS / RS; ++q) {
    const int r = ty + RS * q, i = I * TS + r, j = J * TS + tx;
    float v = 0.f;
    if (i < n && j < n) {
      const float di = dI[r], dj = dJ[tx];
      v = w1 * ((i == j && i < ng ? is : 0.f) - di * dj * is3) + tv[q];
      P[o + (size_t)i * n + j] = v;
    }
    tA[r][tx] = v;
  }
  __syncthreads();
  if (I != J) {
#pragma unroll
    for (int q = 0; q < TS / RS; ++q) {
      const int r = ty + RS * q, i = J * TS + r, j = I * TS + tx;     // transposed tile
      if (i < n && j < n) P[o + (size_t)i * n + j] = tA[tx][r];
    }
  }
}

__global__ void k_big_init(int B, int n, int T, const float* QT, const float* qT, const int* active,
                           float* P, float* pvec, float* lam, float* adj, float* gn2, const float* lx) {
  const int b = blockIdx.y;
  if (active != nullptr && active[b] == 0) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n * n) P[(size_t)b * n * n + e] = QT[(size_t)b * n * n + e];
  if (e < n) {
    if (lx == nullptr) {
      const float q = qT[(size_t)b * n + e];
      pvec[(size_t)b * n + e] = q;
      lam[(size_t)b * n + e] = q;
      adj[((size_t)b * (T + 1) + T) * n + e] = q;
    } else {          // bilevel solve: value vector 0, loss adjoint d loss / d x_T
      pvec[(size_t)b * n + e] = 0.f;
      lam[(size_t)b * n + e] = lx[((size_t)b * (T + 1) + T) * n + e];
    }
  }
  if (e == 0) gn2[b] = 0.f;
}

// trajax continuation test (gmpc_ric_continue, as at the tail of k_riccati)
__global__ void k_big_cont(int B, int T, int m, const float* U, const float* gn2, const int* iters,
                           const float* obj, const float* alpha, const float* obj_step,
                           const float* U_step, gmpc_ilqr_opts opts, const int* active, int* cont) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (active != nullptr && active[b] == 0) return;
  float un2 = 0.f;
  for (int e = 0; e < T * m; ++e) { const float u = U[(size_t)b * T * m + e]; un2 = fmaf(u, u, un2); }
  cont[b] = gmpc_ric_continue(gn2[b], un2, b, obj, obj_step, U_step, iters, alpha, opts) ? 1 : 0;
}

// out[b][c][r] = in[b][r][c], 64 x 64 tiles through LDS
__global__ __launch_bounds__(GMPC_THREADS) void k_btranspose(int R, int C, const float* in, float* out,
                                                             const int* active) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z;
  if (active != nullptr && active[b] == 0) return;
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const float* src = in + (size_t)b * R * C;
  float* dst = out + (size_t)b * R * C;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int r = r0 + ty + 4 * q, c = c0 + tx;
    tile[ty + 4 * q][tx] = (r < R && c < C) ? src[(size_t)r * C + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = c0 + ty + 4 * q, r = r0 + tx;
    if (r < R && c < C) dst[(size_t)c * R + r] = tile[tx][ty + 4 * q];
  }
}
__global__ void k_add_identity(int n, int ld, const int* active, float* M) {
  const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (active != nullptr && active[b] == 0)) return;
  M[(size_t)b * n * ld + (size_t)i * ld + i] += 1.f;
}

// ------------------------------------------------------------------------------------------------
// forward tangent roll of the bilevel solve: dU_t = k_t + K_t dX_t ; dX_{t+1} = A_t dX_t + B_t dU_t
// (oracle hessian_solve, second loop).  One workgroup per trajectory and time step; [A|B] of the step
// comes from the same strided Jacobian chain as in the backward pass.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GMPC_THREADS) void k_big_fwd(int n, int m, int T, int t, const float* ABt,
                                                          const float* K, const float* k, float* Hout,
                                                          float* dX, const float* Vtb, const float* WL, int h) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* dx = reinterpret_cast<float*>(smem);   // n
  float* du = dx + n;                           // m
  float* zv = du + m;                           // h   V^T [dx; du]   (low-rank form)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nm = n + m;
  const size_t bt = (size_t)b * T + t;
  for (int i = tid; i < n; i += blockDim.x) dx[i] = t == 0 ? 0.f : dX[((size_t)b * (T + 1) + t) * n + i];
  __syncthreads();
  for (int j = wave; j < m; j += GMPC_THREADS / 64) {
    const float* Kr = K + (bt * m + j) * n;
    float v = 0.f;
    for (int i = lane; i < n; i += 64) v = fmaf(Kr[i], dx[i], v);
    v = wave_sum(v);
    if (lane == 0) { const float u = k[bt * m + j] + v; du[j] = u; Hout[bt * m + j] = u; }
  }
  if (t == 0)
    for (int i = tid; i < n; i += blockDim.x) dX[(size_t)b * (T + 1) * n + i] = 0.f;
  __syncthreads();
  if (Vtb != nullptr) {
    // dX' = dx + W_L^T (V^T [dx; du])
    const float* Vt = Vtb + (size_t)b * h * nm;
    for (int kk = wave; kk < h; kk += GMPC_THREADS / 64) {
      const float* row = Vt + (size_t)kk * nm;
      float v = 0.f;
      for (int c = lane; c < nm; c += 64) v = fmaf(row[c], c < n ? dx[c] : du[c - n], v);
      v = wave_sum(v);
      if (lane == 0) zv[kk] = v;
    }
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x) {
      float v = dx[i];
      for (int kk = 0; kk < h; ++kk) v = fmaf(WL[(size_t)kk * n + i], zv[kk], v);
      dX[((size_t)b * (T + 1) + t + 1) * n + i] = v;
    }
    return;
  }
  const float* AB = ABt + (size_t)b * n * nm;
  for (int i = wave; i < n; i += GMPC_THREADS / 64) {
    const float* row = AB + (size_t)i * nm;
    float v = 0.f;
    for (int c = lane; c < nm; c += 64) v = fmaf(row[c], c < n ? dx[c] : du[c - n], v);
    v = wave_sum(v);
    if (lane == 0) dX[((size_t)b * (T + 1) + t + 1) * n + i] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// Low-rank form of the per-step Jacobians.  For the relu MLP  J = W_L^T D_{L-2} W_{L-2}^T ... D_0 W_0^T, so
//   A_t = I + W_L^T Vx_t^T,   B_t = W_L^T Vu_t^T,   V_t^T = D_{L-2} W_{L-2}^T ... D_0 W_0^T   [h][n+m],
// with h the last hidden width and W_L^T shared by every sample.  When h < n / 2 (C5: 200 vs 1024) the n^3
// products of the Riccati step go through the factors:
//   W1 = W_L P                    [h][n]      2 h n^2
//   [PA | PB] = [P | 0] + W1^T V^T            2 n h (n+m)
//   W2 = W_L [PA | PB]            [h][n+m]    2 h n (n+m)
//   [H | G_r] = Vu W2             (thin)
//   T1 = PA + Vx W2 + K^T W                   2 n^2 h + 2 n^2 (2m)
// 8 n^2 h instead of 4 n^3 flops (2.56x fewer at C5), and V^T itself costs 2 h (sum h_l h_{l+1} + h (n+m))
// instead of the n-row chain.  V^T is built by masked products: S^T_{L-3}[k][j] = d_{L-3}[k] W_{L-2}[k][j]
// d_{L-2}[j] elementwise, S^T_{l-1} = rowmask_{l-1}(W_l S^T_l) and V^T = S_0 W_0^T as batched GEMMs.
// ------------------------------------------------------------------------------------------------
__global__ void k_mask_scale(int K, int N, const float* W, const uint32_t* maskK, const uint32_t* maskN,
                             long smask, float* out) {
  // out[b][k][j] = W[k][j] if bit k of maskK[b] (optional) and bit j of maskN[b] (optional) are set, else 0
  const int b = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)K * N) return;
  const int kk = (int)(e / N), j = (int)(e - (long)kk * N);
  bool on = true;
  if (maskK) on = on && ((maskK[(size_t)b * smask + (kk >> 5)] >> (kk & 31)) & 1u);
  if (maskN) on = on && ((maskN[(size_t)b * smask + (j >> 5)] >> (j & 31)) & 1u);
  out[(size_t)b * K * N + e] = on ? W[e] : 0.f;
}

// V_t^T for the B samples of step t into w.Vt
static void big_lowrank_factors(const BigWork& w, int B, const MlpDesc& dyn, const uint32_t* masks, int t,
                                const int* active, hipStream_t s) {
  const int L = dyn.L, T = w.T, nm = w.n + w.m, h = w.h, Lh = L - 1;
  const long smask = (long)T * Lh * GMPC_MW;
  auto mk = [&](int l) { return masks + ((size_t)t * Lh + l) * GMPC_MW; };   // + b * smask inside the kernels
  auto gemm = [&](int M, int N, int K, const float* X, long sx, int ldx, const float* Y, long sy, int ldy, float* C,
                  long sc, int ldc) { return bgemm_args(B, M, N, K, X, sx, ldx, Y, sy, ldy, C, sc, ldc, active); };
  if (L == 2) {          // one hidden layer: V^T = D_0 W_0^T
    const long cnt = (long)h * nm;
    hipLaunchKernelGGL(k_mask_scale, dim3((unsigned)((cnt + 255) / 256), B), dim3(256), 0, s, h, nm, dyn.WT[0], mk(0),
                       nullptr, smask, w.Vt);
    return;
  }
  // S^T_{L-3} [dims[L-2]][h]
  float* cur = w.Sa;
  float* nxt = w.Sb;
  {
    const int K = dyn.dims[L - 2];
    const long cnt = (long)K * h;
    hipLaunchKernelGGL(k_mask_scale, dim3((unsigned)((cnt + 255) / 256), B), dim3(256), 0, s, K, h, dyn.W[L - 2],
                       mk(L - 3), mk(L - 2), smask, cur);
  }
  for (int l = L - 3; l >= 1; --l) {
    // S^T_{l-1} [dims[l]][h] = rowmask_{l-1}( W_l S^T_l ):  X = WT[l] ([dims[l+1]][dims[l]], shared), Y = S^T_l
    BgemmArgs g = gemm(dyn.dims[l], h, dyn.dims[l + 1], dyn.WT[l], 0, dyn.dims[l], cur, (long)dyn.dims[l + 1] * h, h,
                       nxt, (long)dyn.dims[l] * h, h);
    g.rowmask = mk(l - 1); g.srm = smask;
    gmpc_launch_bgemm_tn(g, s);
    float* sw = cur; cur = nxt; nxt = sw;
  }
  // V^T [h][n+m] = S_0 W_0^T:  X = S^T_0 ([dims[1]][h]), Y = WT[0] ([dims[1]][n+m], shared)
  gmpc_launch_bgemm_tn(gemm(h, nm, dyn.dims[1], cur, (long)dyn.dims[1] * h, h, dyn.WT[0], 0, nm, w.Vt, (long)h * nm,
                            nm), s);
}

// MLP dynamics on the large-state path whose last hidden width is below n / 2 take the low-rank form (8 n^2 h instead
// of 4 n^3 flops per Riccati step); GMPC_BIG_DENSE=1 keeps the dense form (A/B timing).  Read when a ctx is created.
int gmpc_big_lowrank_h(const gmpc_shape* sh) {
  if (!(sh->n > 64 || sh->m > 32) || sh->dyn_lstm_features > 0) return 0;
  const int hl = sh->dyn_dims[sh->dyn_layers - 1];
  return 2 * hl < sh->n && getenv("GMPC_BIG_DENSE") == nullptr ? hl : 0;
}

// The Jacobians of step t for the B samples (b, t), enqueued on `s`: the low-rank form's factors V_t^T into w.Vt
// (MLP dynamics with w.h > 0; AB is not written), else [A_t | B_t] into AB -- from the LSTM variant's kernel (dl) or
// the MFMA chains (k_linearize_regs, else k_linearize_mfma).  Non-zero when no chain covers the shape.
static int big_step_jacobians(const BigWork& w, int B, const MlpDesc& dyn, const LinPad& lp, const uint32_t* masks,
                              const DynlDesc* dl, const float* X, const float* U, int t, const int* active,
                              float* AB, hipStream_t s) {
  const int n = w.n, m = w.m, T = w.T;
  const int fam = gmpc_linearize_family_of(true, w.h, dl != nullptr, B, n, m, dyn.L, dyn.dims, true);
  if (fam == LIN_DYNL) {
    gmpc_launch_dynl_jac(B, T, 1, t, *dl, X, U, active, AB, s);
  } else if (fam == LIN_LOWRANK) {
    big_lowrank_factors(w, B, dyn, masks, t, active, s);
  } else if (gmpc_launch_linearize_family(fam, B, T, n, m, dyn, lp, masks, active, AB, T, t, s) != 0) {
    return -1;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// host driver of one backward pass
// ------------------------------------------------------------------------------------------------
int gmpc_big_backward(const BigWork& w, int B, const MlpDesc& dyn, const LinPad& lp,
                      const uint32_t* masks, const float* X, const float* U, const float* goal,
                      const float* mpc_w, const float* QT, const float* qT, const int* active, float* K,
                      float* k, float* grad, float* adj, const float* lx, float* Bvec, hipStream_t s,
                      const DynlDesc* dl, const float* lam_sol, const float* lu) {
  // lam_sol (bilevel solve of the LSTM dynamics only): the adjoints of the rollout objective at the solution;
  // the step's curvature Phi = lam_{t+1} . d^2 f joins R, M^T (through [H | G_r]) and Q (through T1)
  const bool curv = dl != nullptr && lx != nullptr && lam_sol != nullptr && w.Phi != nullptr;
  // lx != null: the bilevel Hessian solve (k_big_step mode 1); grad / adj are not written then.  lu (mode 1 only,
  // may be null): d loss / d U of a loss that depends on the controls, the linear term of Bvec
  const int n = w.n, m = w.m, T = w.T, nm = n + m;
  const dim3 ge((n * n + 255) / 256, B);
  hipLaunchKernelGGL(k_big_init, ge, dim3(256), 0, s, B, n, T, QT, qT, active, w.P, w.pvec, w.lam, adj,
                     w.gn2, lx);
  const bool lowrank = w.h > 0 && dl == nullptr;
  const int h = lowrank ? w.h : 0;
  const long snn = (long)n * n, snm = (long)n * nm, smn = (long)m * n, smnm = (long)m * nm;
  auto gemm = [&](int M, int N, int Kk, const float* Xp, long sx, int ldx, const float* Yp, long sy, int ldy,
                  float* Cp, long sc, int ldc) {
    return bgemm_args(B, M, N, Kk, Xp, sx, ldx, Yp, sy, ldy, Cp, sc, ldc, active);
  };
  const int nt = (n + GMPC_PU_TILE - 1) / GMPC_PU_TILE;
  // (read per pass, not once: the tests compare the two forms of the gain solve inside one process)
  const char* sv_env = getenv("GMPC_BIG_SOLVE");
  const bool solve_valu = sv_env != nullptr && strcmp(sv_env, "valu") == 0;
  // One step ahead on a side stream (dense form): the Jacobians [A | B] of a step do not depend on P.  Step t's
  // are produced into copy t & 1 of the buffer while step t + 1's products run on the caller's stream -- the
  // Jacobian chain fills the matrix pipe under k_big_step, k_big_pupdate, the thin products and the transposes, which
  // leave it idle.  ev_ready[i]: copy i is written; ev_free[i]: the point of the caller's stream behind which copy i
  // may be overwritten.  (The low-rank form gains nothing from it: its factor GEMMs and k_big_step slow each other
  // down by what the overlap saves, C5 1.980 vs 1.984 s.)
  const bool pipe = !lowrank && dl == nullptr && w.side != nullptr && w.ABt2 != nullptr;
  float* const ABc[2] = {w.ABt, pipe ? w.ABt2 : w.ABt};
  int rc_side = 0;
  auto jacobians = [&](int t, hipStream_t st) {
    if (big_step_jacobians(w, B, dyn, lp, masks, dl, X, U, t, active, ABc[t & 1], st) != 0) rc_side = -1;
  };
  // event / wait failures: a missed wait would be a silent race on the Jacobian copies, so they end the pass; on any
  // error after the fork the caller's stream first joins the side stream (nothing is left in flight on it)
  auto ev = [&](hipError_t e) { if (e != hipSuccess) rc_side = -1; };
  auto bail = [&]() -> int {
    if (pipe) (void)hipStreamSynchronize(w.side);
    (void)hipGetLastError();
    return -1;
  };
  if (pipe) {
    ev(hipEventRecord(w.ev_start, s));                   // the side stream starts behind the caller's earlier work
    ev(hipStreamWaitEvent(w.side, w.ev_start, 0));
    jacobians(T - 1, w.side);
    ev(hipEventRecord(w.ev_ready[(T - 1) & 1], w.side));
  }
  for (int t = T - 1; t >= 0; --t) {
    const float* A = ABc[t & 1];
    const float* Bm = ABc[t & 1] + n;
    const long shn = (long)h * n, shnm = (long)h * nm;
    const float* WLT = lowrank ? dyn.WT[dyn.L - 1] : nullptr;     // [n][h]: W_L^T, the TN left operand of W_L (.)
    if (pipe) ev(hipStreamWaitEvent(s, w.ev_ready[t & 1], 0));
    else jacobians(t, s);     // (the LSTM variant's too: nothing is enqueued between here and [PA | PB])
    if (rc_side != 0) return bail();
    if (lowrank) {
      // the factors V_t^T (above), then the n^3 products through them (see big_lowrank_factors)
      // Y = W_L P, S = W_L P W_L^T = W_L Y^T, then with Z = Y + S Vx^T / 2:
      //     A^T P A = P + Vx Z + Z^T Vx^T            (T1 below: two K-segments of h rows, a third for K, V)
      //     [H | Gr] = B^T P [A | B] = Vu ([Y | 0] + S V^T) = Vu (2 [Z | S Vu^T / 2] - [Y | 0])
      // 2 h n^2 + 4 h^2 n + 2.2 n^2 h flops instead of the 7.1 n^2 h of [PA | PB] = P [A | B], W_L [PA | PB],
      // A^T (PA) written out (C5: 1.05 instead of 1.49 Gflop per trajectory and step)
      gmpc_launch_bgemm_tn(gemm(h, n, n, WLT, 0, h, w.P, snn, n, w.W1b, shn, n), s);            // Y = W_L P
      float* Yt = w.PAB;                                                                        // [n][h]
      hipLaunchKernelGGL(k_btranspose, dim3((n + 63) / 64, (h + 63) / 64, B), dim3(GMPC_THREADS), 0, s, h, n,
                         w.W1b, Yt, active);
      float* S = w.Sa;                                        // [h][h] (Sa / Sb are the factor products' scratch)
      const long shh = (long)h * h;
      gmpc_launch_bgemm_tn(gemm(h, h, n, WLT, 0, h, Yt, shn, h, S, shh, h), s);                 // S = W_L Y^T
      // W2b = S V^T / 2 + [Y | 0] = [Z | S Vu^T / 2]   (S symmetric up to rounding: S^T V^T is the TN form)
      BgemmArgs g2 = gemm(h, n, h, S, shh, h, w.Vt, shnm, nm, w.W2b, shnm, nm);
      g2.alpha = 0.5f; g2.E = w.W1b; g2.se = shn; g2.lde = n; g2.En = n;
      gmpc_launch_bgemm_tn(g2, s);
      BgemmArgs g3 = gemm(h, m, h, S, shh, h, w.Vt + n, shnm, nm, w.W2b + n, shnm, nm);
      g3.alpha = 0.5f;
      gmpc_launch_bgemm_tn(g3, s);
      BgemmArgs g4 = gemm(m, nm, h, w.Vt + n, shnm, nm, w.W2b, shnm, nm, w.HG, smnm, nm);       // 2 Vu W2b
      g4.alpha = 2.f;
      gmpc_launch_bgemm_tn(g4, s);
      BgemmArgs g5 = gemm(m, n, h, w.Vt + n, shnm, nm, w.W1b, shn, n, w.HG, smnm, nm);          // - Vu [Y | 0]
      g5.alpha = -1.f; g5.beta = 1.f;
      gmpc_launch_bgemm_tn(g5, s);
    } else {
    // [PA | PB] = P [A | B]   (P symmetric, so P = P^T is the "TN" left operand)
    gmpc_launch_bgemm_tn(gemm(n, n, n, w.P, snn, n, A, snm, nm, w.PAB, snm, nm), s);
    gmpc_launch_bgemm_tn(gemm(n, m, n, w.P, snn, n, Bm, snm, nm, w.PAB + n, snm, nm), s);
    // [H | Gr] = B^T [PA | PB]
    gmpc_launch_bgemm_tn(gemm(m, nm, n, Bm, snm, nm, w.PAB, snm, nm, w.HG, smnm, nm), s);
    // step t - 1's Jacobians start when step t reaches its stretch of kernels that leave the matrix pipe idle (the
    // thin products, k_big_step, ...): started at the top of the step they only shared the pipe with the step's
    // first big GEMM, both at half speed (kernel trace: linearize 0.66 ms beside PA 1.04 ms, then 0.36 ms of thin
    // products and k_big_step alone); behind the two thin products: started behind PA the chain stretched [H | G_r]
    // from 0.09 to 0.6 ms -- C4 98.8 / 100.3 / 98.0 ms for a start behind PA / PB / [H | G_r], 99.6 without the side
    // stream
    if (pipe && t > 0) {
      ev(hipEventRecord(w.ev_free[(t - 1) & 1], s));        // (the copy's last reader was step t + 1; this point is later)
      ev(hipStreamWaitEvent(w.side, w.ev_free[(t - 1) & 1], 0));
      jacobians(t - 1, w.side);
      ev(hipEventRecord(w.ev_ready[(t - 1) & 1], w.side));
    }
    }
    if (curv) {
      gmpc_launch_dynl_curv(B, T, 1, t, *dl, X, U, lam_sol, active, w.Phi, s);
      gmpc_launch_add_phi(B, n, m, w.Phi, w.HG, nullptr, s);
    }
    BigStepArgs a;
    a.Vt = lowrank ? w.Vt : nullptr; a.WL = lowrank ? dyn.W[dyn.L - 1] : nullptr; a.h = h;
    a.B = B; a.n = n; a.m = m; a.T = T; a.t = t;
    a.mode = lx != nullptr ? 1 : 0; a.lx = lx; a.lu = lx != nullptr ? lu : nullptr; a.Bvec = Bvec;
    a.X = X; a.U = U; a.goal = goal; a.ng = w.ng; a.mpc_w = mpc_w; a.ABt = A; a.HG = w.HG; a.KV = w.KV; a.VK = w.VK;
    a.pvec = w.pvec; a.lam = w.lam; a.sbuf = w.sbuf; a.gn2 = w.gn2; a.active = active;
    a.K = K; a.k = k; a.grad = grad; a.adj = adj;
    a.solve_valu = solve_valu ? 1 : 0;
    if (gmpc_launch_big_step(a, s) != 0) { bail(); return -2; }     // (its LDS does not fit: nothing launched)
    // T1 = A^T (PA) + [K; V]^T [V; K], upper blocks only   (low-rank form: P + Vx Z + Z^T Vx^T)
    BgemmArgs g = lowrank ? gemm(n, n, h, w.Vt, shnm, nm, w.W2b, shnm, nm, w.T1, snn, n)
                          : gemm(n, n, n, A, snm, nm, w.PAB, snm, nm, w.T1, snn, n);
    g.X2 = w.KV; g.sx2 = 2 * smn; g.ldx2 = n;
    g.Y2 = w.VK; g.sy2 = 2 * smn; g.ldy2 = n; g.K2 = 2 * m;
    if (lowrank) {
      g.E = w.P; g.se = snn; g.lde = n; g.En = n;
      g.X3 = w.W2b; g.sx3 = shnm; g.ldx3 = nm; g.Y3 = w.Vt; g.sy3 = shnm; g.ldy3 = nm; g.K3 = h;
    }
    g.upper_only = 1;
    gmpc_launch_bgemm_tn(g, s);
    if (curv) gmpc_launch_add_phi(B, n, m, w.Phi, nullptr, w.T1, s);
    hipLaunchKernelGGL(k_big_pupdate, dim3(nt * (nt + 1) / 2, 1, B), dim3(GMPC_THREADS), 0, s, n, w.ng > 0 ? w.ng : n, T, t, X,
                       goal, mpc_w,
                       w.sbuf, w.T1, active, w.P);
  }
  if (lowrank) {
    // keep the documented content of the step buffer: [A_0 | B_0] = [I | 0] + W_L^T V_0^T of the last step
    // processed (gmpc_debug_buffer 5, the `lqr` slot of the host mirror) -- one thin-K GEMM per pass
    const long shnm = (long)h * nm;
    gmpc_launch_bgemm_tn(gemm(n, nm, h, dyn.W[dyn.L - 1], 0, n, w.Vt, shnm, nm, w.ABt, snm, nm), s);
    hipLaunchKernelGGL(k_add_identity, dim3((n + 255) / 256, B), dim3(256), 0, s, n, nm, active, w.ABt);
  }
  return 0;
}

int gmpc_big_forward_tangent(const BigWork& w, int B, const MlpDesc& dyn, const LinPad& lp,
                             const uint32_t* masks, const float* K, const float* k, float* Hout, float* dX,
                             hipStream_t s, const DynlDesc* dl, const float* X, const float* U) {
  const int n = w.n, m = w.m, T = w.T;
  const bool lowrank = w.h > 0 && dl == nullptr;
  for (int t = 0; t < T; ++t) {
    if (big_step_jacobians(w, B, dyn, lp, masks, dl, X, U, t, nullptr, w.ABt, s) != 0) return -1;
    hipLaunchKernelGGL(k_big_fwd, dim3(B), dim3(GMPC_THREADS), (size_t)(n + m + (lowrank ? w.h : 0)) * sizeof(float),
                       s, n, m, T, t, w.ABt, K, k, Hout, dX, lowrank ? w.Vt : nullptr,
                       lowrank ? dyn.W[dyn.L - 1] : nullptr, lowrank ? w.h : 0);
  }
  return 0;
}

void gmpc_launch_big_cont(int B, int T, int m, const float* U, const float* gn2, const int* iters,
                          const float* obj, const float* alpha, const float* obj_step,
                          const float* U_step, const gmpc_ilqr_opts& opts, const int* active, int* cont,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_big_cont, dim3((B + 63) / 64), dim3(64), 0, s, B, T, m, U, gn2, iters, obj, alpha,
                     obj_step, U_step, opts, active, cont);
}
