// Vector-Jacobian product of a plan's one-step ensemble disagreement (gmpc_ensemble_disagreement_vjp; DESIGN.md section
// 30): d[p][b][t] = |MLP_p(z_t) - MLP_0(z_t)|^2 at z_t = [x_t; u_t] of the nominal rollout X, under the weights
// w[p][b][t] = gd + gD.  X is given, so the local part is independent per (b, t) row; the part through the nominal
// rollout is section 29's sweep with P = 1 under gX = rx, launched by the entry point behind these kernels.
//
//   k_disvjp_rows    grid (tiles of 32 (b, t) rows, P + 1).  Plane p < P is member p, plane P the bound (nominal)
//                    network: the tile's rows go through ALL layers of the plane's network with k_ensvjp_rows' step
//                    arithmetic (dg_gemm, then max(v + b, 0)); the output o = acc + b goes to the plane's rows of `out`,
//                    the relu bits of every hidden unit to the plane's masks and, for a member whose weight gradients
//                    are wanted, the layer inputs to its acts rows (the last tile zeroes the member's pad rows).  One
//                    code path and one live tile; the nominal's forward is taken once per tile, not once per member.
//   k_disvjp_back    grid (tiles of 32 rows, P + 1).  Plane p < P: c^p = 2 w (o^p - o^0) from the two output planes, back
//                    through member p's masked W_l^T to q^p.  Plane P: c^N = -((c^0 + c^1) + ...) with the same
//                    operations per member, back through the nominal's masked W_l^T to q^N.  The deltas of every layer go
//                    to the plane's dels rows where weight gradients are wanted.
//   k_disvjp_reduce  r_t = (((q^0 + q^1) + ...) + q^{P-1}) + q^N per element, one fp32 addition each: the state part
//                    to rx [B][T+1][n] (row T zero), the control part to ru [B][T][m].
//   k_disvjp_add     out = x + y per element of rows of `width` floats `ld` apart: grad_U = ru + chain, and the nominal's
//                    local dels rows + the chain's, ahead of the one weight-gradient pass.
// Both networks' outputs come from the same instructions on the same operand rows, so a member whose layers equal the
// bound layers has o^p - o^0 == 0 exactly.  No atomics; every float a kernel reads was written earlier in the same call.
#include "gmpc_cem_rollout.h"

// the bits of one (plane, row, hidden layer): words [GMPC_MW], bit j & 31 of word j >> 5 = unit j is active
__device__ __forceinline__ size_t disvjp_mask_at(size_t p, size_t rows, size_t r, int Lh, int l) {
  return ((p * rows + r) * Lh + l) * GMPC_MW;
}

// c^p of (row r of problem b, output j): e = o^p - o^0, then (2 w) e -- every operation one IEEE fp32 operation
__device__ __forceinline__ float disvjp_c(const DisVjpArgs& a, size_t p, size_t R, size_t r, int b, int j) {
#pragma clang fp contract(off)
  float w;
  if (a.gd && a.gD)
    w = a.gd[p * R + r] + a.gD[p * a.B + b];
  else
    w = a.gd ? a.gd[p * R + r] : a.gD[p * a.B + b];
  const float e = a.out[(p * R + r) * a.n + j] - a.out[((size_t)a.P * R + r) * a.n + j];
  const float w2 = 2.f * w;
  return w2 * e;
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_disvjp_rows(DisVjpArgs a) {
  __shared__ __attribute__((aligned(16))) float Ab[GMPC_CEM_ROWS * GMPC_DG_LDA];   // the layer inputs of the 32 rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, T = a.T, L = a.dyn.L, Lh = L - 1;
  const int R = a.B * T;                         // the rows: r = b T + t
  const int r0 = blockIdx.x * GMPC_CEM_ROWS;
  const size_t p = blockIdx.y, st = a.dr.stride;
  const bool member = p < (size_t)a.P;
  float* acts = member && a.acts ? a.acts + p * a.rstride : nullptr;
  if (acts && blockIdx.x == gridDim.x - 1) {
    // the pad rows behind the member's B T rows (read, not used, by the weight-gradient GEMMs)
    float* dels = a.dels + p * a.rstride;
    const size_t o = (size_t)R * st;
    for (size_t e = tid; e < GMPC_WGRAD_PAD * st; e += GMPC_DG_THREADS) {
      acts[o + e] = 0.f;
      dels[o + e] = 0.f;
    }
  }
  // ---- layer 0 input [x_t; u_t] (rows past R: the last row again, nothing written for them)
  for (int e = tid; e < GMPC_CEM_ROWS * (n + m); e += GMPC_DG_THREADS) {
    const int i = e / (n + m), j = e - i * (n + m);
    const int r = min(r0 + i, R - 1), b = r / T, t = r - b * T;
    const float v = j < n ? a.X[((size_t)b * (T + 1) + t) * n + j] : a.U[(size_t)r * m + (j - n)];
    Ab[i * GMPC_DG_LDA + j] = v;
    if (acts && r0 + i < R) acts[(size_t)r * st + a.dr.aoff[0] + j] = v;
  }
  __syncthreads();
  DgTiles acc;
  for (int l = 0; l < L; ++l) {
    const int K = a.dyn.dims[l], Nl = a.dyn.dims[l + 1];
    const float* W = member ? a.dyn.W[l] + p * a.mstride : a.nom.W[l];
    const float* bias = member ? a.dyn.b[l] + p * a.mstride : a.nom.b[l];
    dg_gemm(Ab, K, Nl, W, wave, lane, acc);
    if (l == Lh) {
      // ---- the output o = acc + b of every live row
      float* out = a.out + p * (size_t)R * n;
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const int j = (wave + 4 * ci) * 16 + l16;
        if (j >= n) continue;
        const float bj = bias[j];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int ip = r0 + 4 * kq + rr, iq = ip + 16;
          if (ip < R) out[(size_t)ip * n + j] = acc.p[ci][rr] + bj;
          if (iq < R) out[(size_t)iq * n + j] = acc.q[ci][rr] + bj;
        }
      }
      break;
    }
    __syncthreads();   // every wave has read its operand rows
    cem_store_tiles(Ab, acc, Nl, wave, lane, [bias](float v, int j) { return fmaxf(v + bias[j], 0.f); });
    __syncthreads();
    // ---- the layer's relu bits: one thread per (row, word of 32 units)
    {
      const int i = tid >> 3, w = tid & 7;
      if (r0 + i < R) {
        const float* row = Ab + i * GMPC_DG_LDA + 32 * w;
        uint32_t bits = 0u;
        for (int k = 0; k < 32; ++k)
          if (32 * w + k < Nl && row[k] > 0.f) bits |= 1u << k;
        a.masks[disvjp_mask_at(p, R, r0 + i, Lh, l) + w] = bits;
      }
    }
    // ---- a_{l+1} of every live row
    if (acts) {
      const int ao = a.dr.aoff[l + 1];
      for (int e = tid; e < GMPC_CEM_ROWS * Nl; e += GMPC_DG_THREADS) {
        const int i = e / Nl, j = e - i * Nl;
        if (r0 + i < R) acts[(size_t)(r0 + i) * st + ao + j] = Ab[i * GMPC_DG_LDA + j];
      }
    }
    // (the next product reads Ab as it is; its barrier orders the next layer's stores behind these reads)
  }
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_disvjp_back(DisVjpArgs a) {
  __shared__ __attribute__((aligned(16))) float Ab[GMPC_CEM_ROWS * GMPC_DG_LDA];   // the deltas of the 32 rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, T = a.T, L = a.dyn.L, Lh = L - 1, P = a.P;
  const size_t R = (size_t)a.B * T, st = a.dr.stride;
  const int r0 = blockIdx.x * GMPC_CEM_ROWS;
  const size_t p = blockIdx.y;
  const bool member = p < (size_t)P;
  float* dels = member ? (a.dels ? a.dels + p * a.rstride : nullptr) : a.ndels;
  // ---- e_{L-1} = c of the plane: the output layer's delta rows and the first operand
  {
    const int dL = a.dr.doff[L - 1];
    for (int e = tid; e < GMPC_CEM_ROWS * n; e += GMPC_DG_THREADS) {
#pragma clang fp contract(off)
      const int i = e / n, j = e - i * n;
      const size_t r = min((size_t)(r0 + i), R - 1);
      const int b = (int)(r / T);
      float c;
      if (member) {
        c = disvjp_c(a, p, R, r, b, j);
      } else {
        float sum = disvjp_c(a, 0, R, r, b, j);
        for (int q = 1; q < P; ++q) sum = sum + disvjp_c(a, q, R, r, b, j);
        c = -sum;
      }
      Ab[i * GMPC_DG_LDA + j] = c;
      if (dels && (size_t)(r0 + i) < R) dels[r * st + dL + j] = c;
    }
  }
  __syncthreads();
  // the thread's 8 rows in the accumulator layout: half h, register rr -> operand row 16 h + 4 kq + rr
  size_t ri[2][4];
  bool ok[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const size_t r = (size_t)r0 + 16 * h + 4 * kq + rr;
      ok[h][rr] = r < R;
      ri[h][rr] = r < R ? r : R - 1;
    }
  DgTiles acc;
  for (int l = L - 1; l >= 1; --l) {
    const int K = a.dyn.dims[l + 1], Nl = a.dyn.dims[l];      // e_{l-1} = [z_{l-1} > 0] . (e_l W_l^T)
    dg_gemm(Ab, K, Nl, member ? a.dyn.WT[l] + p * a.mstride : a.nom.WT[l], wave, lane, acc);
    __syncthreads();
    const int dof = a.dr.doff[l - 1];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int j = (wave + 4 * ci) * 16 + l16;
      if (j >= Nl) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int i = 4 * kq + rr;
        const uint32_t mp = a.masks[disvjp_mask_at(p, R, ri[0][rr], Lh, l - 1) + (j >> 5)];
        const uint32_t mq = a.masks[disvjp_mask_at(p, R, ri[1][rr], Lh, l - 1) + (j >> 5)];
        const float dp = (mp >> (j & 31)) & 1u ? acc.p[ci][rr] : 0.f;
        const float dq = (mq >> (j & 31)) & 1u ? acc.q[ci][rr] : 0.f;
        Ab[i * GMPC_DG_LDA + j] = dp;
        Ab[(16 + i) * GMPC_DG_LDA + j] = dq;
        if (dels) {
          if (ok[0][rr]) dels[ri[0][rr] * st + dof + j] = dp;
          if (ok[1][rr]) dels[ri[1][rr] * st + dof + j] = dq;
        }
      }
    }
    __syncthreads();
  }
  // ---- q = e_0 W_0^T, [n + m] per row
  dg_gemm(Ab, a.dyn.dims[1], n + m, member ? a.dyn.WT[0] + p * a.mstride : a.nom.WT[0], wave, lane, acc);
  float* q = a.q + p * R * (size_t)(n + m);
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const int j = (wave + 4 * ci) * 16 + l16;
    if (j >= n + m) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      if (ok[0][rr]) q[ri[0][rr] * (n + m) + j] = acc.p[ci][rr];
      if (ok[1][rr]) q[ri[1][rr] * (n + m) + j] = acc.q[ci][rr];
    }
  }
}

// r_t = (((q^0 + q^1) + ...) + q^{P-1}) + q^N per element, every addition one IEEE fp32 operation (k_ensvjp_reduce's
// form): element i < B (T+1) n goes to rx (row T: zero), the R m elements behind them to ru.
__global__ __launch_bounds__(GMPC_THREADS) void k_disvjp_reduce(DisVjpArgs a) {
#pragma clang fp contract(off)
  const int n = a.n, m = a.m, T = a.T;
  const size_t R = (size_t)a.B * T, nx = (size_t)a.B * (T + 1) * n, plane = R * (size_t)(n + m);
  size_t i = (size_t)blockIdx.x * GMPC_THREADS + threadIdx.x;
  size_t src;
  float* dst;
  if (i < nx) {
    const size_t bt = i / n, b = bt / (T + 1), t = bt - b * (T + 1);
    dst = a.rx + i;
    if (t == (size_t)T) {
      *dst = 0.f;
      return;
    }
    src = (b * T + t) * (n + m) + (i - bt * n);
  } else {
    i -= nx;
    if (i >= R * m) return;
    const size_t r = i / m;
    dst = a.ru + i;
    src = r * (n + m) + n + (i - r * m);
  }
  float sum = a.q[src];
  for (int p = 1; p <= a.P; ++p) sum = sum + a.q[p * plane + src];
  *dst = sum;
}

// out[r][j] = x[r][j] + y[r][j], j < width, rows `ld` floats apart (out may be x or y)
__global__ __launch_bounds__(GMPC_THREADS) void k_disvjp_add(size_t rows, int width, size_t ld, const float* x,
                                                             const float* y, float* out) {
  const size_t i = (size_t)blockIdx.x * GMPC_THREADS + threadIdx.x;
  if (i >= rows * width) return;
  const size_t r = i / width, o = r * ld + (i - r * width);
  out[o] = x[o] + y[o];
}

// Host-side launchers ---------------------------------------------------------------------------
int gmpc_launch_dis_vjp_local(const DisVjpArgs& a, hipStream_t s) {
  for (int l = 0; l <= a.dyn.L; ++l)
    if (a.dyn.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return 1;
  if (a.n + a.m > GMPC_SAMPLED_MAX_WIDTH || a.B < 1 || a.T < 1 || a.P < 1 || a.P > GMPC_MAX_ENSEMBLE) return 1;
  if (!a.gd && !a.gD) return 1;
  if ((a.acts != nullptr) != (a.dels != nullptr)) return 1;
  if (!a.out || !a.q || !a.rx || !a.ru || (a.dyn.L > 1 && !a.masks)) return 1;
  const size_t R = (size_t)a.B * a.T;
  const dim3 grid((unsigned)((R + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS), a.P + 1);
  hipLaunchKernelGGL(k_disvjp_rows, grid, dim3(GMPC_DG_THREADS), 0, s, a);
  hipLaunchKernelGGL(k_disvjp_back, grid, dim3(GMPC_DG_THREADS), 0, s, a);
  const size_t total = (size_t)a.B * (a.T + 1) * a.n + R * a.m;
  hipLaunchKernelGGL(k_disvjp_reduce, dim3((unsigned)((total + GMPC_THREADS - 1) / GMPC_THREADS)), dim3(GMPC_THREADS),
                     0, s, a);
  return 0;
}

void gmpc_launch_dis_vjp_add(size_t rows, int width, size_t ld, const float* x, const float* y, float* out,
                             hipStream_t s) {
  const size_t total = rows * width;
  if (total == 0) return;
  hipLaunchKernelGGL(k_disvjp_add, dim3((unsigned)((total + GMPC_THREADS - 1) / GMPC_THREADS)), dim3(GMPC_THREADS), 0,
                     s, rows, width, ld, x, y, out);
}
