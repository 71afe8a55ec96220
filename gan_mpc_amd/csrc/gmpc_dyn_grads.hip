// Gradient of an upper-level loss L(X*, U*) with respect to the relu-MLP dynamics' weights
// (gmpc_bilevel_grad_dynamics).  f(x, u) = x + MLP([x; u]):
//
//   dL/dtheta = dL/dtheta|_U - d/dtheta [ H . grad_U J ]   (H held fixed)
//             = sum_t  mu_{t+1} . f_theta - nu_{t+1} . f_theta - lam_{t+1} . d/dtheta (f_x dX_t + f_u H_t)
//
// The adjoints come from k_tail_adjoints (gmpc_tail_adjoints.hip) as the planes w = mu_{t+1} - nu_{t+1} and lam_{t+1}.
// Per step: one MLP pass over the primal row a_0 = [x_t; u_t] and the tangent row a'_0 = [dX_t; H_t] (the primal's
// relu masks, no bias), backward passes of w and lam_{t+1} through the same masks:
//   gW_l = sum_{b,t} a_{l-1}^T delta_l(w) - a'_{l-1}^T delta_l(lam),   gb_l = sum_{b,t} delta_l(w).
// The residual x adds nothing to the parameter gradient.
//
//   k_dyn_rows      16 steps per workgroup on v_mfma_f32_16x16x4_f32: the layer inputs [a; -a'] and deltas
//                   [delta(w); delta(lam)] as 2 B T rows, whose column sums (k_wgrad*) are the weight gradient.
#include "gmpc_dg_gemm.h"

#include <cstring>

#define GMPC_DG_ROWS 16          // steps per workgroup of the row kernel (32 GEMM rows: primal + tangent)

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

// Host-side launcher ----------------------------------------------------------------------------
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
