// Gradient of an upper-level loss L(X*, U*) with respect to the relu-MLP dynamics' weights
// (gmpc_bilevel_grad_dynamics), from the state a preceding gmpc_bilevel_grad(_cotangent) leaves in the ctx:
// H = A^{-1} Bvec, its tangent roll dX, [A_t | B_t], QT and qT.  f(x, u) = x + MLP([x; u]):
//
//   dL/dtheta = dL/dtheta|_U - d/dtheta [ H . grad_U J ]   (H held fixed)
//             = sum_t  mu_{t+1} . f_theta - nu_{t+1} . f_theta - lam_{t+1} . d/dtheta (f_x dX_t + f_u H_t)
//
//   lam_T = qT,        lam_t = q_t + A_t^T lam_{t+1}        q_t = w1 d / s  (d = x_t[:ng] - g_t, s = sqrt(|d|^2 + a^2))
//   mu_T  = lx_T,      mu_t  = lx_t + A_t^T mu_{t+1}
//   nu_T  = QT dX_T,   nu_t  = Q_t dX_t + A_t^T nu_{t+1}      (the relu dynamics have no curvature: Phi = 0)
//
// Per step, with w = mu_{t+1} - nu_{t+1}: one MLP pass over the primal row a_0 = [x_t; u_t] and the tangent row
// a'_0 = [dX_t; H_t] (the primal's relu masks, no bias), backward passes of w and lam_{t+1} through the same masks:
//   gW_l = sum_{b,t} a_{l-1}^T delta_l(w) - a'_{l-1}^T delta_l(lam),   gb_l = sum_{b,t} delta_l(w).
// The residual x adds nothing to the parameter gradient.
//
//   k_dyn_adjoints  one workgroup per trajectory: the three backward sweeps -> w, lam planes [B][T][n]
//   k_dyn_rows      16 steps per workgroup on v_mfma_f32_16x16x4_f32: the layer inputs [a; -a'] and deltas
//                   [delta(w); delta(lam)] as 2 B T rows, whose column sums (k_wgrad*) are the weight gradient.
#include "gmpc_launch.h"

#include <cstring>

#define GMPC_DG_THREADS 256
#define GMPC_DG_CHUNK 8          // steps staged per chunk of the adjoint sweep (at most)
#define GMPC_DG_CHUNK_FLOATS 14336   // LDS budget of the staged steps (56 KB)
#define GMPC_DG_ROWS 16          // steps per workgroup of the row kernel (32 GEMM rows: primal + tangent)
#define GMPC_DG_LDA 260          // LDS row stride of the row kernel's activations (widths <= 256, + 4)

// ---- the three adjoint sweeps ---------------------------------------------------------------------------------
// n <= 64, m <= 32 ([A_t | B_t] is kept).  Wave 0 runs mu, wave 1 nu, wave 2 lam; lane c owns state c and holds its
// adjoint in a register (lanes >= n hold 0).  A_t^T v is an NMAX-term sum of LDS reads of column c of A_t times v_i
// broadcast with v_readlane.  Steps come in chunks of K (<= GMPC_DG_CHUNK): every thread loads the chunk into LDS,
// the waves run it backwards and park v_{t+1} in LDS, and the chunk's w / lam rows go out behind the barrier.
template <int NMAX>
__global__ __launch_bounds__(GMPC_DG_THREADS) void k_dyn_adjoints(int T, int n, int ng, int m, int K,
                                                                  const float* mpc_w,
                                                                  const float* X, const float* goal, const float* dX,
                                                                  const float* lx, const float* AB, const float* QT,
                                                                  const float* qT, float* wout, float* lout) {
  extern __shared__ __attribute__((aligned(16))) char smem_da[];
  const int nm = n + m, fa = n * nm;
  float* S = reinterpret_cast<float*>(smem_da);
  float* ABs = S;                    // [K][n][nm]
  float* LXs = ABs + K * fa;         // [K][n]
  float* DXs = LXs + K * n;          // [K][n]
  float* Xs = DXs + K * n;           // [K][n]
  float* Gs = Xs + K * n;            // [K][ng]
  float* Vs = Gs + K * ng;           // [3][K][64]: v_{t+1} of each sweep
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const int lc = lane < n ? lane : 0;
  const float al = GMPC_ALPHA;
  const float w1 = sigmoidf_(mpc_w[1]);
  const size_t xrow = (size_t)b * (T + 1), urow = (size_t)b * T;

  // ---- terminal values (dX_T through LDS for the QT product)
  if (tid < n) Xs[tid] = dX[(xrow + T) * n + tid];
  __syncthreads();
  float v_adj = 0.f;
  if (lane < n) {
    if (wave == 0) {
      v_adj = lx[(xrow + T) * n + lane];
    } else if (wave == 1) {
      const float* q = QT + ((size_t)b * n + lane) * n;
      float v = 0.f;
      for (int k = 0; k < n; ++k) v = fmaf(q[k], Xs[k], v);
      v_adj = v;
    } else if (wave == 2) {
      v_adj = qT[(size_t)b * n + lane];
    }
  }
  __syncthreads();

  auto atv = [&](const float* A, float v) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) acc = fmaf(A[(i < n ? i : n - 1) * nm + lc], __int_as_float(
                                                  __builtin_amdgcn_readlane(__float_as_int(v), i)), acc);
    return acc;
  };
  for (int tend = T; tend > 0; tend -= K) {
    const int t0 = tend - K > 0 ? tend - K : 0, kc = tend - t0;
    for (int e = tid; e < kc * fa; e += GMPC_DG_THREADS) ABs[e] = AB[(urow + t0) * fa + e];
    for (int e = tid; e < kc * n; e += GMPC_DG_THREADS) {
      LXs[e] = lx[(xrow + t0) * n + e];
      DXs[e] = dX[(xrow + t0) * n + e];
      Xs[e] = X[(xrow + t0) * n + e];
    }
    for (int e = tid; e < kc * ng; e += GMPC_DG_THREADS) Gs[e] = goal[(xrow + t0) * ng + e];
    __syncthreads();
    if (wave < 3) {
      float* vs = Vs + wave * K * 64;
      for (int k = kc - 1; k >= 0; --k) {
        vs[k * 64 + lane] = v_adj;          // v_{t0 + k + 1}
        float src = 0.f;                    // this sweep's source term at step t0 + k
        if (wave == 0) {
          src = LXs[k * n + lc];
        } else {
          // |d|^2 and d . dX over the goal columns: q_t = w1 d / s, Q_t dX_t = w1 (dX / s - d (d . dX) / s^3)
          const float cd = lane < ng ? Xs[k * n + lane] - Gs[k * ng + lane] : 0.f;
          const float dd = wave_sum(cd * cd);
          const float is = 1.f / sqrtf(dd + al * al);
          if (wave == 1) {
            const float cdx = lane < n ? DXs[k * n + lane] : 0.f;
            const float dxd = wave_sum(cd * cdx);
            src = lane < ng ? w1 * (cdx * is - cd * dxd * (is * is * is)) : 0.f;
          } else {
            src = lane < ng ? w1 * cd * is : 0.f;
          }
        }
        const float v = atv(ABs + k * fa, v_adj);
        v_adj = lane < n ? src + v : 0.f;
      }
    }
    __syncthreads();
    for (int e = tid; e < kc * n; e += GMPC_DG_THREADS) {
      const int k = e / n, i = e - k * n;
      wout[(urow + t0) * n + e] = Vs[k * 64 + i] - Vs[(K + k) * 64 + i];
      lout[(urow + t0) * n + e] = Vs[(2 * K + k) * 64 + i];
    }
    __syncthreads();
  }
}

// ---- the row kernel -------------------------------------------------------------------------------------------
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

// rows: B T steps, r = b T + t.  acts / dels: [2 rows][stride]; row r holds the primal layer inputs a_0 .. a_{L-1}
// and delta_1(w) .. delta_L(w), row rows + r the negated tangent inputs -a'_0 .. -a'_{L-1} and delta_1(lam) ..
// delta_L(lam).  lay: the column of a_l / delta_{l+1} in a row, and the row stride.
struct DgRowArgs {
  int rows, T, n, m;
  MlpDesc dyn;
  MlpRows lay;
  const float *X, *U, *dX, *H, *w, *lam;
  float *acts, *dels;
};

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_dyn_rows(DgRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_dr[];
  float* Ab = reinterpret_cast<float*>(smem_dr);                                  // [32][GMPC_DG_LDA]
  unsigned char* mk = reinterpret_cast<unsigned char*>(Ab + 32 * GMPC_DG_LDA);   // [L-1][16][256] relu masks
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, nm = n + m, L = a.dyn.L, T = a.T;
  const int r0 = blockIdx.x * GMPC_DG_ROWS;
  const size_t st = a.lay.stride, tro = (size_t)a.rows;   // the tangent row of step r is tro + r
  // ---- layer 0 inputs: [x_t; u_t] and [dX_t; H_t]
  for (int e = tid; e < GMPC_DG_ROWS * nm; e += GMPC_DG_THREADS) {
    const int i = e / nm, c = e - i * nm, r = r0 + i;
    float p = 0.f, q = 0.f;
    if (r < a.rows) {
      const int bb = r / T, t = r - bb * T;
      const size_t xr = (size_t)bb * (T + 1) + t;
      p = c < n ? a.X[xr * n + c] : a.U[(size_t)r * m + c - n];
      q = c < n ? a.dX[xr * n + c] : a.H[(size_t)r * m + c - n];
      a.acts[(size_t)r * st + c] = p;
      a.acts[(tro + r) * st + c] = -q;
    }
    Ab[i * GMPC_DG_LDA + c] = p;
    Ab[(16 + i) * GMPC_DG_LDA + c] = q;
  }
  __syncthreads();
  DgTiles acc;
  // ---- forward through the hidden layers (the output layer's value is not needed)
  for (int l = 0; l < L - 1; ++l) {
    const int K = a.dyn.dims[l], N = a.dyn.dims[l + 1];
    dg_gemm(Ab, K, N, a.dyn.W[l], wave, lane, acc);
    __syncthreads();   // every wave has read its operand rows
    const float* bias = a.dyn.b[l];
    unsigned char* ml = mk + l * GMPC_DG_ROWS * 256;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int j = (wave + 4 * ci) * 16 + l16;
      if (j >= N) continue;
      const float bj = bias[j];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int i = 4 * kq + rr, r = r0 + i;
        const float z = acc.p[ci][rr] + bj;
        const bool on = z > 0.f;
        const float p = on ? z : 0.f, q = on ? acc.q[ci][rr] : 0.f;
        Ab[i * GMPC_DG_LDA + j] = p;
        Ab[(16 + i) * GMPC_DG_LDA + j] = q;
        ml[i * 256 + j] = on ? 1 : 0;
        if (r < a.rows) {
          a.acts[(size_t)r * st + a.lay.aoff[l + 1] + j] = p;
          a.acts[(tro + r) * st + a.lay.aoff[l + 1] + j] = -q;
        }
      }
    }
    __syncthreads();
  }
  // ---- backward: delta_L = w_{t+1} (primal half) and lam_{t+1} (tangent half)
  for (int e = tid; e < GMPC_DG_ROWS * n; e += GMPC_DG_THREADS) {
    const int i = e / n, c = e - i * n, r = r0 + i;
    float p = 0.f, q = 0.f;
    if (r < a.rows) {
      p = a.w[(size_t)r * n + c];
      q = a.lam[(size_t)r * n + c];
      a.dels[(size_t)r * st + a.lay.doff[L - 1] + c] = p;
      a.dels[(tro + r) * st + a.lay.doff[L - 1] + c] = q;
    }
    Ab[i * GMPC_DG_LDA + c] = p;
    Ab[(16 + i) * GMPC_DG_LDA + c] = q;
  }
  __syncthreads();
  for (int l = L - 1; l >= 1; --l) {
    const int K = a.dyn.dims[l + 1], N = a.dyn.dims[l];   // delta_l = mask_l . (delta_{l+1} W_l^T)
    dg_gemm(Ab, K, N, a.dyn.WT[l], wave, lane, acc);
    __syncthreads();
    const unsigned char* ml = mk + (l - 1) * GMPC_DG_ROWS * 256;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int j = (wave + 4 * ci) * 16 + l16;
      if (j >= N) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int i = 4 * kq + rr, r = r0 + i;
        const bool on = ml[i * 256 + j] != 0;
        const float p = on ? acc.p[ci][rr] : 0.f, q = on ? acc.q[ci][rr] : 0.f;
        Ab[i * GMPC_DG_LDA + j] = p;
        Ab[(16 + i) * GMPC_DG_LDA + j] = q;
        if (r < a.rows) {
          a.dels[(size_t)r * st + a.lay.doff[l - 1] + j] = p;
          a.dels[(tro + r) * st + a.lay.doff[l - 1] + j] = q;
        }
      }
    }
    __syncthreads();
  }
}

// Host-side launchers ---------------------------------------------------------------------------
void gmpc_launch_dyn_adjoints(int B, int T, int n, int ng, int m, const float* mpc_w, const float* X,
                              const float* goal, const float* dX, const float* lx, const float* AB, const float* QT,
                              const float* qT, float* w, float* lam, hipStream_t s) {
  const int F = n * (n + m) + 3 * n + ng;
  int K = GMPC_DG_CHUNK_FLOATS / F;
  if (K > GMPC_DG_CHUNK) K = GMPC_DG_CHUNK;
  if (K > T) K = T;
  if (K < 1) K = 1;   // (n <= 64, m <= 32: F <= 6400)
  const size_t lds = ((size_t)K * F + 3 * (size_t)K * 64) * sizeof(float);
  if (n <= 32)
    hipLaunchKernelGGL(k_dyn_adjoints<32>, dim3(B), dim3(GMPC_DG_THREADS), lds, s, T, n, ng, m, K, mpc_w, X, goal,
                       dX, lx, AB, QT, qT, w, lam);
  else
    hipLaunchKernelGGL(k_dyn_adjoints<64>, dim3(B), dim3(GMPC_DG_THREADS), lds, s, T, n, ng, m, K, mpc_w, X, goal,
                       dX, lx, AB, QT, qT, w, lam);
}

int gmpc_launch_dyn_rows(int B, int T, int n, int m, const MlpDesc& dyn, const float* X, const float* U,
                         const float* dX, const float* H, const float* w, const float* lam, float* acts, float* dels,
                         const MlpRows& lay, hipStream_t s) {
  DgRowArgs a;
  memset(&a, 0, sizeof(a));
  for (int l = 0; l <= dyn.L; ++l)
    if (dyn.dims[l] > 256) return 1;
  a.rows = B * T; a.T = T; a.n = n; a.m = m; a.dyn = dyn; a.lay = lay;
  a.X = X; a.U = U; a.dX = dX; a.H = H; a.w = w; a.lam = lam; a.acts = acts; a.dels = dels;
  const size_t lds = 32 * GMPC_DG_LDA * sizeof(float) + (size_t)(dyn.L > 1 ? dyn.L - 1 : 1) * GMPC_DG_ROWS * 256;
  hipLaunchKernelGGL(k_dyn_rows, dim3((a.rows + GMPC_DG_ROWS - 1) / GMPC_DG_ROWS), dim3(GMPC_DG_THREADS), lds, s, a);
  return 0;
}
