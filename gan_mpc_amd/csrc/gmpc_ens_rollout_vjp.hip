// Vector-Jacobian product of a plan's rollout and per-step costs under every member of a dynamics ensemble
// (gmpc_ensemble_rollout_vjp): the derivation of gmpc_rollout_vjp.hip (section 14) with
// f_p(x, u) = x + MLP_p([x; u]) at (X[p], U, goal) under (gX[p], gcost[p]), for the P members at once, on the fp32
// matrix instruction.
//
//   k_ensvjp_rows    grid (tiles of 32 (b, t) rows, P).  X is given, so the B T steps of a member are independent: each
//                    tile's rows go through member p's hidden layers with k_ens_rollout's step arithmetic (dg_gemm, then
//                    max(v + b, 0)), the relu bits of every hidden unit go to the call's masks (a unit is active iff its
//                    output is > 0, as in k_rvjp_sweep) and, when the members' weight gradients are wanted, the layer
//                    inputs to the member's acts rows.  The last tile zeroes the member's pad rows.
//   k_ensvjp_sweep   grid (tiles of 32 problems, P).  v_{t+1} of the 32 problems stays in registers in dg_gemm's
//                    accumulator layout.  First the terminal cost: the cost MLP forward and back at x_T (its rows go to
//                    acts2 / dels2, row p B + b); then t = T-1 .. 0: v_{t+1} through member p's W_l^T, masked, the stage
//                    terms in closed form with the row sums by cem_row8_sum.  Per step it writes member p's dL/dU_t,
//                    dL/dgoal_t and the dels rows, at the end dL/dx0 -- all per member, into the call workspace.
//   k_ensvjp_reduce  out = ((g^0 + g^1) + ...) + g^{P-1} per element: one fp32 addition per member in ascending p, no
//                    contraction, so P = 1 hands the member's value through bit for bit.
// The transposes of the members are k_dynfit_transpose's (gmpc_dynfit_rows.hip), the sums over rows the weight-gradient
// GEMMs of gmpc_wgrad.hip.  No atomics; every float a kernel reads was written earlier in the same call.
#include "gmpc_cem_rollout.h"

// the bits of one (row, step, hidden layer): words [GMPC_MW], bit j & 31 of word j >> 5 = unit j is active
__device__ __forceinline__ size_t ensvjp_mask_at(size_t p, size_t rows, size_t r, int Lh, int l) {
  return ((p * rows + r) * Lh + l) * GMPC_MW;
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_ensvjp_rows(EnsVjpArgs a) {
  __shared__ __attribute__((aligned(16))) float Ab[GMPC_CEM_ROWS * GMPC_DG_LDA];   // the layer inputs of the 32 rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = a.n, m = a.m, T = a.T, L = a.dyn.L, Lh = L - 1;
  const int R = a.B * T;                         // the member's rows: r = b T + t
  const int r0 = blockIdx.x * GMPC_CEM_ROWS;
  const size_t p = blockIdx.y, st = a.dr.stride;
  float* acts = a.acts ? a.acts + p * a.rstride : nullptr;
  if (acts && blockIdx.x == gridDim.x - 1) {
    // the pad rows behind the member's B T rows (read, not used, by the weight-gradient GEMMs)
    float* dels = a.dels + p * a.rstride;
    const size_t o = (size_t)R * st;
    for (size_t e = tid; e < GMPC_WGRAD_PAD * st; e += GMPC_DG_THREADS) {
      acts[o + e] = 0.f;
      dels[o + e] = 0.f;
    }
  }
  // ---- layer 0 input [x_t; u_t] of member p (rows past R: the last row again, nothing written for them)
  const float* Xp = a.X + p * a.B * (size_t)(T + 1) * n;
  for (int e = tid; e < GMPC_CEM_ROWS * (n + m); e += GMPC_DG_THREADS) {
    const int i = e / (n + m), j = e - i * (n + m);
    const int r = min(r0 + i, R - 1), b = r / T, t = r - b * T;
    const float v = j < n ? Xp[((size_t)b * (T + 1) + t) * n + j] : a.U[(size_t)r * m + (j - n)];
    Ab[i * GMPC_DG_LDA + j] = v;
    if (acts && r0 + i < R) acts[(size_t)r * st + a.dr.aoff[0] + j] = v;
  }
  __syncthreads();
  DgTiles acc;
  for (int l = 0; l < Lh; ++l) {
    const int K = a.dyn.dims[l], Nl = a.dyn.dims[l + 1];
    dg_gemm(Ab, K, Nl, a.dyn.W[l] + p * a.mstride, wave, lane, acc);
    __syncthreads();   // every wave has read its operand rows
    const float* bias = a.dyn.b[l] + p * a.mstride;
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
        a.masks[ensvjp_mask_at(p, R, r0 + i, Lh, l) + w] = bits;
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

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_ensvjp_sweep(EnsVjpArgs a) {
  __shared__ __attribute__((aligned(16))) float Ab[GMPC_CEM_ROWS * GMPC_DG_LDA];   // the deltas of the 32 rows
  __shared__ float s_gcx[GMPC_CEM_ROWS], s_gcu[GMPC_CEM_ROWS];   // gc_t w1 / s_t and gc_t w0 / r_t of a row
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, T = a.T, B = a.B, L = a.dyn.L, Lh = L - 1, Lc = a.cost.L - 1;
  const int b0 = blockIdx.x * GMPC_CEM_ROWS;     // row i of the tile is problem b0 + i
  const size_t p = blockIdx.y;
  const int rrow = tid >> 3, rc = tid & 7;       // the row whose sums this thread shares in, its lane of the row's 8
  const int last = B - 1;
  const int rb = min(b0 + rrow, last);
  const bool rlive = b0 + rrow < B;
  const bool gcon = a.gc != nullptr;
  const float al = GMPC_ALPHA;
  float w0 = 0.f, w1 = 0.f, w2 = 0.f;
  if (gcon) {
    w0 = sigmoidf_(a.mpc_w[0]); w1 = sigmoidf_(a.mpc_w[1]); w2 = sigmoidf_(a.mpc_w[2]);
  }
  const size_t xs = (size_t)(T + 1) * n;         // X / goal / gX floats per problem
  const float* Xp = a.X + p * B * xs;
  const float* gXp = a.gX ? a.gX + p * B * xs : nullptr;
  const float* gcp = gcon ? a.gc + p * B * (size_t)(T + 1) : nullptr;
  // The thread's 8 problems in the accumulator layout: half h (0: p, 1: q), register rr -> operand row 16 h + 4 kq + rr
  int bi[2][4];
  bool ok[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int b = b0 + 16 * h + 4 * kq + rr;
      ok[h][rr] = b < B;
      bi[h][rr] = b < B ? b : last;
    }
  float gm0 = 0.f, gm1 = 0.f, gm2 = 0.f;         // d/d mpc_w of row rrow (the same in its 8 lanes)
  DgTiles v, acc;                                 // v_{t+1} of the 32 problems; a product's output
  // ---- v_T = gX_T
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const int j = (wave + 4 * ci) * 16 + l16;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      v.p[ci][rr] = gXp && j < n ? gXp[(size_t)bi[0][rr] * xs + (size_t)T * n + j] : 0.f;
      v.q[ci][rr] = gXp && j < n ? gXp[(size_t)bi[1][rr] * xs + (size_t)T * n + j] : 0.f;
    }
  }
  // ---- terminal cost c_T = w2 |MLP_c(x_T)|^2: v_T += gc_T grad_x c_T
  if (gcon) {
    const size_t cst = a.cr.stride;
    float* cacts = a.cacts + p * B * cst;
    float* cdels = a.cdels + p * B * cst;
    for (int e = tid; e < GMPC_CEM_ROWS * n; e += GMPC_DG_THREADS) {
      const int i = e / n, j = e - i * n;
      const float x = Xp[(size_t)min(b0 + i, last) * xs + (size_t)T * n + j];
      Ab[i * GMPC_DG_LDA + j] = x;
      if (b0 + i < B) cacts[(size_t)(b0 + i) * cst + a.cr.aoff[0] + j] = x;
    }
    __syncthreads();
    for (int l = 0; l <= Lc; ++l) {
      const int K = a.cost.dims[l], Nl = a.cost.dims[l + 1];
      dg_gemm(Ab, K, Nl, a.cost.W[l], wave, lane, acc);
      __syncthreads();
      const float* bias = a.cost.b[l];
      if (l < Lc) {
        const int ao = a.cr.aoff[l + 1];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const int j = (wave + 4 * ci) * 16 + l16;
          if (j >= Nl) continue;
          const float bj = bias[j];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int i = 4 * kq + rr;
            const float vp = fmaxf(acc.p[ci][rr] + bj, 0.f), vq = fmaxf(acc.q[ci][rr] + bj, 0.f);
            Ab[i * GMPC_DG_LDA + j] = vp;
            Ab[(16 + i) * GMPC_DG_LDA + j] = vq;
            if (ok[0][rr]) cacts[(size_t)bi[0][rr] * cst + ao + j] = vp;     // (read back below by this thread)
            if (ok[1][rr]) cacts[(size_t)bi[1][rr] * cst + ao + j] = vq;
          }
        }
      } else {
        cem_store_tiles(Ab, acc, Nl, wave, lane, [bias](float y, int j) { return y + bias[j]; });
      }
      __syncthreads();
    }
    // ---- y in Ab: |y|^2 of row rrow, then e_out = dL/dy = 2 gc_T w2 y
    const int fo = a.cost.dims[Lc + 1];
    {
      const float* row = Ab + rrow * GMPC_DG_LDA;
      float sy = 0.f;
      for (int j = rc; j < fo; j += 8) sy = fmaf(row[j], row[j], sy);
      sy = cem_row8_sum(sy);
      gm2 = gcp[(size_t)rb * (T + 1) + T] * ((w2 * (1.f - w2)) * sy);
    }
    __syncthreads();
    {
      const int dof = a.cr.doff[Lc];
      for (int e = tid; e < GMPC_CEM_ROWS * fo; e += GMPC_DG_THREADS) {
        const int i = e / fo, j = e - i * fo, b = min(b0 + i, last);
        const float d = (2.f * gcp[(size_t)b * (T + 1) + T] * w2) * Ab[i * GMPC_DG_LDA + j];
        Ab[i * GMPC_DG_LDA + j] = d;
        if (b0 + i < B) cdels[(size_t)b * cst + dof + j] = d;
      }
    }
    __syncthreads();
    for (int l = Lc; l >= 0; --l) {
      const int K = a.cost.dims[l + 1], Nl = a.cost.dims[l];       // e_{l-1} = relu'(a_l) . (e_l W_l^T)
      dg_gemm(Ab, K, Nl, a.cost.WT[l], wave, lane, acc);
      __syncthreads();
      if (l > 0) {
        const int ao = a.cr.aoff[l], dof = a.cr.doff[l - 1];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const int j = (wave + 4 * ci) * 16 + l16;
          if (j >= Nl) continue;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int i = 4 * kq + rr;
            const size_t rp = (size_t)bi[0][rr] * cst, rq = (size_t)bi[1][rr] * cst;
            const float dp = ok[0][rr] && cacts[rp + ao + j] > 0.f ? acc.p[ci][rr] : 0.f;     // (its own store)
            const float dq = ok[1][rr] && cacts[rq + ao + j] > 0.f ? acc.q[ci][rr] : 0.f;
            Ab[i * GMPC_DG_LDA + j] = dp;
            Ab[(16 + i) * GMPC_DG_LDA + j] = dq;
            if (ok[0][rr]) cdels[rp + dof + j] = dp;
            if (ok[1][rr]) cdels[rq + dof + j] = dq;
          }
        }
        __syncthreads();
      } else {
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const int j = (wave + 4 * ci) * 16 + l16;
          if (j >= n) continue;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            v.p[ci][rr] += acc.p[ci][rr];
            v.q[ci][rr] += acc.q[ci][rr];
          }
        }
      }
    }
    // the terminal cost does not read its goal
    if (a.ggoal) {
      float* gg = a.ggoal + p * B * xs;
      for (int e = tid; e < GMPC_CEM_ROWS * n; e += GMPC_DG_THREADS) {
        const int i = e / n, j = e - i * n;
        if (b0 + i < B) gg[(size_t)(b0 + i) * xs + (size_t)T * n + j] = 0.f;
      }
    }
  }
  // ---- the steps, last first
  const size_t R = (size_t)B * T, st = a.dr.stride;
  float* dels = a.dels ? a.dels + p * a.rstride : nullptr;
  const int dL = a.dr.doff[L - 1];
  for (int t = T - 1; t >= 0; --t) {
    // ---- e_{L-1} = v_{t+1}: the output layer's delta rows and the first operand
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int j = (wave + 4 * ci) * 16 + l16;
      if (j >= n) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int i = 4 * kq + rr;
        Ab[i * GMPC_DG_LDA + j] = v.p[ci][rr];
        Ab[(16 + i) * GMPC_DG_LDA + j] = v.q[ci][rr];
        if (dels) {
          if (ok[0][rr]) dels[((size_t)bi[0][rr] * T + t) * st + dL + j] = v.p[ci][rr];
          if (ok[1][rr]) dels[((size_t)bi[1][rr] * T + t) * st + dL + j] = v.q[ci][rr];
        }
      }
    }
    // ---- the stage cost's norms of row rrow (read behind at least one barrier)
    if (gcon) {
      const float* x = Xp + (size_t)rb * xs + (size_t)t * n;
      const float* g = a.goal + (size_t)rb * xs + (size_t)t * n;
      const float* u = a.U + ((size_t)rb * T + t) * m;
      float su = 0.f, sx = 0.f;
      for (int j = rc; j < m; j += 8) su = fmaf(u[j], u[j], su);
      for (int j = rc; j < n; j += 8) {
        const float d = x[j] - g[j];
        sx = fmaf(d, d, sx);
      }
      su = cem_row8_sum(su);
      sx = cem_row8_sum(sx);
      const float ru = sqrtf(su + al * al), rx = sqrtf(sx + al * al);
      const float gct = gcp[(size_t)rb * (T + 1) + t];
      gm0 = fmaf(gct, (w0 * (1.f - w0)) * (ru - al), gm0);
      gm1 = fmaf(gct, (w1 * (1.f - w1)) * (rx - al), gm1);
      if (rc == 0) {
        s_gcx[rrow] = gct * w1 * (1.f / rx);
        s_gcu[rrow] = gct * w0 * (1.f / ru);
      }
    }
    __syncthreads();
    for (int l = L - 1; l >= 1; --l) {
      const int K = a.dyn.dims[l + 1], Nl = a.dyn.dims[l];      // e_{l-1} = [z_{l-1} > 0] . (e_l W_l^T)
      dg_gemm(Ab, K, Nl, a.dyn.WT[l] + p * a.mstride, wave, lane, acc);
      __syncthreads();
      const int dof = a.dr.doff[l - 1];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const int j = (wave + 4 * ci) * 16 + l16;
        if (j >= Nl) continue;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int i = 4 * kq + rr;
          const size_t rp = (size_t)bi[0][rr] * T + t, rq = (size_t)bi[1][rr] * T + t;
          const uint32_t mp = a.masks[ensvjp_mask_at(p, R, rp, Lh, l - 1) + (j >> 5)];
          const uint32_t mq = a.masks[ensvjp_mask_at(p, R, rq, Lh, l - 1) + (j >> 5)];
          const float dp = (mp >> (j & 31)) & 1u ? acc.p[ci][rr] : 0.f;
          const float dq = (mq >> (j & 31)) & 1u ? acc.q[ci][rr] : 0.f;
          Ab[i * GMPC_DG_LDA + j] = dp;
          Ab[(16 + i) * GMPC_DG_LDA + j] = dq;
          if (dels) {
            if (ok[0][rr]) dels[rp * st + dof + j] = dp;
            if (ok[1][rr]) dels[rq * st + dof + j] = dq;
          }
        }
      }
      __syncthreads();
    }
    // ---- [px; pu] = e_0 W_0^T:  v_t = gX_t + gc_t grad_x c_t + v_{t+1} + px,  dL/dU_t = gc_t grad_u c_t + pu
    dg_gemm(Ab, a.dyn.dims[1], n + m, a.dyn.WT[0] + p * a.mstride, wave, lane, acc);
    __syncthreads();     // (every wave has read the deltas: the next step's stores may follow)
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int j = (wave + 4 * ci) * 16 + l16;
      if (j < n) {
        // v_t of (half h, register rr) from v_{t+1} = vr and px; member p's dL/dgoal_t on the way
        auto step = [&](int h, int rr, float vr, float px) -> float {
          const size_t o = (size_t)bi[h][rr] * xs + (size_t)t * n + j;
          const float gx = gXp ? gXp[o] : 0.f;
          if (!gcon) return (gx + vr) + px;
          const float gcx = s_gcx[16 * h + 4 * kq + rr];
          const float d = Xp[o] - a.goal[o];
          if (a.ggoal && ok[h][rr]) a.ggoal[p * B * xs + o] = gcx * -d;
          return ((gx + gcx * d) + vr) + px;
        };
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          v.p[ci][rr] = step(0, rr, v.p[ci][rr], acc.p[ci][rr]);
          v.q[ci][rr] = step(1, rr, v.q[ci][rr], acc.q[ci][rr]);
        }
      } else if (j < n + m && a.gU) {
        auto ctrl = [&](int h, int rr, float pu) {
          if (!ok[h][rr]) return;
          const size_t o = ((size_t)bi[h][rr] * T + t) * m + (j - n);
          a.gU[p * R * m + o] = gcon ? fmaf(s_gcu[16 * h + 4 * kq + rr], a.U[o], pu) : pu;
        };
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          ctrl(0, rr, acc.p[ci][rr]);
          ctrl(1, rr, acc.q[ci][rr]);
        }
      }
    }
    __syncthreads();     // (s_gcx / s_gcu are read: the next step may rewrite them)
  }
  if (a.gx0) {
    float* g0 = a.gx0 + p * B * (size_t)n;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int j = (wave + 4 * ci) * 16 + l16;
      if (j >= n) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        if (ok[0][rr]) g0[(size_t)bi[0][rr] * n + j] = v.p[ci][rr];
        if (ok[1][rr]) g0[(size_t)bi[1][rr] * n + j] = v.q[ci][rr];
      }
    }
  }
  if (a.gm && rc == 0 && rlive) {
    float* g = a.gm + (p * B + b0 + rrow) * 3;
    g[0] = gm0; g[1] = gm1; g[2] = gm2;
  }
}

// out[i] = ((g^0[i] + g^1[i]) + ...) + g^{P-1}[i] for the three per-problem outputs in one launch: every addition one
// IEEE fp32 operation in ascending p (k_ens_moments' form), so the sums are a function of the members' values alone.
__global__ __launch_bounds__(GMPC_THREADS) void k_ensvjp_reduce(EnsVjpReduce r) {
#pragma clang fp contract(off)
  size_t i = (size_t)blockIdx.x * GMPC_THREADS + threadIdx.x;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const size_t count = r.count[s];
    if (i < count) {
      const float* g = r.planes[s];
      float sum = g[i];
      for (int p = 1; p < r.P; ++p) sum = sum + g[p * count + i];
      r.out[s][i] = sum;
      return;
    }
    i -= count;
  }
}

// Host-side launchers ---------------------------------------------------------------------------
int gmpc_launch_ens_rollout_vjp(const EnsVjpArgs& a, int P, hipStream_t s) {
  for (int l = 0; l <= a.dyn.L; ++l)
    if (a.dyn.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return 1;
  for (int l = 0; l <= a.cost.L; ++l)
    if (a.cost.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return 1;
  if (a.n + a.m > GMPC_SAMPLED_MAX_WIDTH || a.B < 1 || a.T < 1 || P < 1 || P > GMPC_MAX_ENSEMBLE) return 1;
  if (!a.gX && !a.gc) return 1;
  if ((a.acts != nullptr) != (a.dels != nullptr)) return 1;
  if (a.gc && (!a.cacts || !a.cdels)) return 1;
  if (a.dyn.L > 1 || a.acts) {
    const int R = a.B * a.T;
    hipLaunchKernelGGL(k_ensvjp_rows, dim3((R + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS, P), dim3(GMPC_DG_THREADS), 0, s, a);
  }
  hipLaunchKernelGGL(k_ensvjp_sweep, dim3((a.B + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS, P), dim3(GMPC_DG_THREADS), 0, s, a);
  return 0;
}

void gmpc_launch_ens_vjp_reduce(const EnsVjpReduce& r, hipStream_t s) {
  const size_t total = r.count[0] + r.count[1] + r.count[2];
  if (total == 0) return;
  hipLaunchKernelGGL(k_ensvjp_reduce, dim3((unsigned)((total + GMPC_THREADS - 1) / GMPC_THREADS)), dim3(GMPC_THREADS),
                     0, s, r);
}
