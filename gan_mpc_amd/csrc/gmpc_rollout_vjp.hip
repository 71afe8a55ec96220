// Vector-Jacobian product of the rollout and its per-step costs (gmpc_rollout_vjp).
// f(x, u) = x + MLP([x; u]) (relu), c_t the staging cost, c_T = w2 |MLP_c(x_T)|^2.  Cotangents gX = dL/dX, gc = dL/dc:
//
//   v_T = gX_T + gc_T grad_x c_T
//   t = T-1 .. 0:  [px; pu] = [J_x; J_u]^T v_{t+1}   (backprop through the dynamics MLP at (X_t, U_t))
//                  dL/dU_t = gc_t grad_u c_t + pu,   v_t = gX_t + gc_t grad_x c_t + v_{t+1} + px
//   dL/dx0 = v_0,  dL/dgoal_t = -gc_t w1 d_t / s_t (t < T; row T = 0)
//
// with d_t = x_t - g_t, s_t = sqrt(|d_t|^2 + a^2), r_t = sqrt(|u_t|^2 + a^2), w = sigmoid(mpc_w):
//   grad_x c_t = w1 d_t / s_t,  grad_u c_t = w0 u_t / r_t,  dc_t/dmpc_w = (w0 (1-w0) (r_t - a), w1 (1-w1) (s_t - a), 0),
//   dc_T/dmpc_w2 = w2 (1-w2) |y|^2,  e_out = dL/dy = 2 gc_T w2 y  (y = MLP_c(x_T)).
//
//   k_rvjp_acts   (grad_dyn_sum only) one forward pass per (trajectory, step) row, 4 rows per workgroup: the layer
//                 inputs a_0 .. a_{L-1} as rows, and the relu masks (without grad_dyn_sum the masks come from k_masks)
//   k_rvjp_sweep  4 trajectories per workgroup for the whole horizon, sequential in t: the terminal-cost VJP through
//                 the cost MLP, then per step the backward pass of v_{t+1} through the dynamics MLP with that step's
//                 masks, the staging-cost terms in closed form.  Writes grad_U, grad_x0, grad_goal, the per-trajectory
//                 mpc_w terms, the cost layers' input / delta rows and (grad_dyn_sum) the dynamics' delta rows.
// The batch sums (mpc_w, cost and dynamics weights) are the weight-gradient GEMMs of gmpc_wgrad.hip.
#include "gmpc_traj_layers.h"
#include "gmpc_launch.h"

#include <cstring>

struct RvjpArgs {
  int B, n, m, T;
  MlpDesc dyn, cost;
  const float* mpc_w;
  const float *X, *U, *goal, *gX, *gc;   // gX / gc may be null (zero)
  const uint32_t* masks;                 // [B][T][Lh][GMPC_MW]
  float *gx0, *gU, *ggoal;               // [B][n], [B][T][m], [B][T+1][n]; each may be null
  float* gm;                             // [B][3] d/d mpc_w per trajectory, or null
  float *cacts, *cdels;                  // [B][cr.stride] cost-layer inputs / deltas, or null
  float *acts, *dels;                    // [B T][dr.stride] dynamics-layer inputs (k_rvjp_acts) / deltas, or null
  MlpRows dr, cr;                        // column of a_l / e_l in a dynamics row / a cost row, and the row strides
  int aw;                                // float4 per LDS activation buffer
};

// out[j] = sum_k in[k] M[k][j] for the 4 slots, M (K, N) row-major: one output per thread (N > 64, chunks of 256), or
// the K range split over thread groups (N <= 64).  Fixed summation order.  The caller synchronises before reading out.
__device__ __forceinline__ void rv_product(const float* M, int K, int N, const float4* in, float4* out, float4* part) {
  const int tid = threadIdx.x;
  if (N <= 64) {
    dense_small<1>(M, K, N, in, part);
    if (tid < N) out[tid] = part[tid];
    return;
  }
  for (int jb = 0; jb < N; jb += GMPC_THREADS) {
    float4 acc[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
    dense_rows<1>(M, K, N, jb + tid, in, acc);
    if (jb + tid < N) out[jb + tid] = acc[0];
  }
}

// component c of v to base[row_c * stride] for the slots whose bit is set in wbits
__device__ __forceinline__ void rv_store4(float* base, size_t stride, unsigned wbits, const int* row, float4 v) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if ((wbits >> c) & 1u) base[(size_t)row[c] * stride] = f4get(v, c);
}

__global__ __launch_bounds__(GMPC_THREADS) void k_rvjp_sweep(RvjpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_rv[];
  float4* const bufA = reinterpret_cast<float4*>(smem_rv);
  float4* const bufB = bufA + a.aw;
  float4* const part = bufB + a.aw;          // [GMPC_THREADS]
  float4* const vcur = part + GMPC_THREADS;  // [n]: v_{t+1}
  float4* const cin = vcur + a.n;            // cost-layer inputs a_0 .. a_{Lc} at x_T
  __shared__ float s_gc[4], s_isx[4], s_isu[4];
  __shared__ int s_bi[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = a.n, m = a.m, T = a.T, L = a.dyn.L, Lh = L - 1, Lc = a.cost.L - 1;
  const int b0 = blockIdx.x * 4;
  if (tid < 4) s_bi[tid] = min(b0 + tid, a.B - 1);
  __syncthreads();
  int bi[4];
  unsigned wbits = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    bi[c] = s_bi[c];
    wbits |= (b0 + c < a.B ? 1u : 0u) << c;
  }
  const float al = GMPC_ALPHA;
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]), w2 = sigmoidf_(a.mpc_w[2]);
  const bool gcon = a.gc != nullptr;
  const size_t xs = (size_t)(T + 1) * n;   // X / goal / gX floats per trajectory
  float gm0 = 0.f, gm1 = 0.f, gm2 = 0.f;   // wave c: slot c's d/d mpc_w

  // ---- terminal: v_T = gX_T + gc_T grad_x c_T
  for (int i = tid; i < n; i += GMPC_THREADS) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f), x = v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t o = (size_t)bi[c] * xs + (size_t)T * n + i;
      if (a.gX) f4set(v, c, a.gX[o]);
      f4set(x, c, a.X[o]);
    }
    vcur[i] = v;
    cin[i] = x;
  }
  if (tid < 4) s_gc[tid] = gcon ? a.gc[(size_t)bi[tid] * (T + 1) + T] : 0.f;
  __syncthreads();
  if (gcon) {
    for (int l = 0; l < Lc; ++l) {
      hidden_layer(a.cost.W[l], a.cost.b[l], a.cost.dims[l], a.cost.dims[l + 1], cin + a.cr.aoff[l],
                   cin + a.cr.aoff[l + 1], nullptr, 0, 0u);
      __syncthreads();
    }
    const int fo = a.cost.dims[Lc + 1];
    dense_small<1>(a.cost.W[Lc], a.cost.dims[Lc], fo, cin + a.cr.aoff[Lc], part);
    const float* pf = reinterpret_cast<const float*>(part);
    {
      const int c = wave;
      float yy = 0.f;
      for (int r = lane; r < fo; r += 64) {
        const float y = pf[r * 4 + c] + a.cost.b[Lc][r];
        yy = fmaf(y, y, yy);
      }
      yy = wave_sum(yy);
      gm2 = s_gc[c] * ((w2 * (1.f - w2)) * yy);
    }
    // e_Lc = dL/dy = 2 gc_T w2 y
    float* bAf = reinterpret_cast<float*>(bufA);
    for (int e = tid; e < 4 * fo; e += GMPC_THREADS) {
      const int r = e >> 2, c = e & 3;
      bAf[e] = (2.f * s_gc[c] * w2) * (pf[e] + a.cost.b[Lc][r]);
    }
    __syncthreads();
    float4* in = bufA;
    float4* out = bufB;
    for (int l = Lc; l >= 0; --l) {
      const int K = a.cost.dims[l + 1], N = a.cost.dims[l];
      if (a.cdels) {
        for (int j = tid; j < K; j += GMPC_THREADS)
          rv_store4(a.cdels + a.cr.doff[l] + j, a.cr.stride, wbits, bi, in[j]);
        for (int j = tid; j < N; j += GMPC_THREADS)
          rv_store4(a.cacts + a.cr.aoff[l] + j, a.cr.stride, wbits, bi, cin[a.cr.aoff[l] + j]);
      }
      rv_product(a.cost.WT[l], K, N, in, out, part);
      __syncthreads();
      if (l > 0) {
        // relu mask of the layer input: a_l > 0 exactly where its pre-activation was
        const float4* al4 = cin + a.cr.aoff[l];
        for (int j = tid; j < N; j += GMPC_THREADS) {
          float4 g = out[j];
          const float4 h = al4[j];
          g.x = h.x > 0.f ? g.x : 0.f; g.y = h.y > 0.f ? g.y : 0.f;
          g.z = h.z > 0.f ? g.z : 0.f; g.w = h.w > 0.f ? g.w : 0.f;
          out[j] = g;
        }
        __syncthreads();
      }
      float4* tmp = in; in = out; out = tmp;
    }
    for (int i = tid; i < n; i += GMPC_THREADS) {
      float4 v = vcur[i];
      const float4 g = in[i];
      v.x += g.x; v.y += g.y; v.z += g.z; v.w += g.w;
      vcur[i] = v;
    }
  }
  if (a.ggoal)
    for (int i = tid; i < n; i += GMPC_THREADS)
      rv_store4(a.ggoal + (size_t)T * n + i, xs, wbits, bi, make_float4(0.f, 0.f, 0.f, 0.f));
  __syncthreads();

  // ---- the steps, last first
  const size_t mst = (size_t)Lh * GMPC_MW;        // mask words per step
  const size_t drow = (size_t)T * a.dr.stride;      // delta-row floats per trajectory
  for (int t = T - 1; t >= 0; --t) {
    // staging-cost norms of slot `wave` (read by the update below, behind at least one barrier)
    {
      const int c = wave;
      const size_t xo = (size_t)bi[c] * xs + (size_t)t * n;
      float dd = 0.f, uu = 0.f;
      if (gcon) {
        for (int i = lane; i < n; i += 64) {
          const float d = a.X[xo + i] - a.goal[xo + i];
          dd = fmaf(d, d, dd);
        }
        for (int j = lane; j < m; j += 64) {
          const float u = a.U[((size_t)bi[c] * T + t) * m + j];
          uu = fmaf(u, u, uu);
        }
      }
      dd = wave_sum(dd);
      uu = wave_sum(uu);
      const float sx = sqrtf(dd + al * al), su = sqrtf(uu + al * al);
      const float gct = gcon ? a.gc[(size_t)bi[c] * (T + 1) + t] : 0.f;
      gm0 = fmaf(gct, (w0 * (1.f - w0)) * (su - al), gm0);
      gm1 = fmaf(gct, (w1 * (1.f - w1)) * (sx - al), gm1);
      if (lane == 0) {
        s_gc[c] = gct;
        s_isx[c] = 1.f / sx;
        s_isu[c] = 1.f / su;
      }
    }
    // backward pass of e_{L-1} = v_{t+1} through the dynamics MLP
    if (a.dels)
      for (int i = tid; i < n; i += GMPC_THREADS)
        rv_store4(a.dels + (size_t)t * a.dr.stride + a.dr.doff[L - 1] + i, drow, wbits, bi, vcur[i]);
    const float4* in = vcur;
    float4* out = bufA;
    for (int l = L - 1; l >= 0; --l) {
      const int K = a.dyn.dims[l + 1], N = a.dyn.dims[l];
      rv_product(a.dyn.WT[l], K, N, in, out, part);
      __syncthreads();
      if (l > 0) {
        // e_{l-1} = (e_l W_l^T) * [z_{l-1} > 0]; hidden widths <= 256: one unit per thread
        const int j = tid;
        if (j < N) {
          float4 g = out[j];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const uint32_t w = a.masks[((size_t)bi[c] * T + t) * mst + (size_t)(l - 1) * GMPC_MW + (j >> 5)];
            if (((w >> (j & 31)) & 1u) == 0u) f4set(g, c, 0.f);
          }
          out[j] = g;
          if (a.dels) rv_store4(a.dels + (size_t)t * a.dr.stride + a.dr.doff[l - 1] + j, drow, wbits, bi, g);
        }
        __syncthreads();
      }
      in = out;
      out = out == bufA ? bufB : bufA;
    }
    // in = [px; pu]:  v_t = gX_t + gc_t grad_x c_t + v_{t+1} + px,  dL/dU_t = gc_t grad_u c_t + pu
    for (int i = tid; i < n; i += GMPC_THREADS) {
      float4 v = vcur[i];
      const float4 p = in[i];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t o = (size_t)bi[c] * xs + (size_t)t * n + i;
        const float gcx = s_gc[c] * w1 * s_isx[c];
        const float d = a.X[o] - a.goal[o];
        const float gx = a.gX ? a.gX[o] : 0.f;
        f4set(v, c, ((gx + gcx * d) + f4get(v, c)) + f4get(p, c));
        if (a.ggoal && ((wbits >> c) & 1u)) a.ggoal[o] = gcx * -d;
      }
      vcur[i] = v;
    }
    if (a.gU)
      for (int e = tid; e < 4 * m; e += GMPC_THREADS) {
        const int c = e / m, j = e - c * m;
        if ((wbits >> c) & 1u) {
          const size_t o = ((size_t)bi[c] * T + t) * m + j;
          const float pu = reinterpret_cast<const float*>(in)[(n + j) * 4 + c];
          a.gU[o] = fmaf(s_gc[c] * w0 * s_isu[c], a.U[o], pu);
        }
      }
    __syncthreads();
  }
  if (a.gx0)
    for (int i = tid; i < n; i += GMPC_THREADS) rv_store4(a.gx0 + i, (size_t)n, wbits, bi, vcur[i]);
  if (a.gm && lane == 0 && ((wbits >> wave) & 1u)) {
    float* g = a.gm + (size_t)bi[wave] * 3;
    g[0] = gm0; g[1] = gm1; g[2] = gm2;
  }
}

// Layer inputs a_0 .. a_{L-1} of B T rows (r = b T + t), 4 rows per workgroup, and their relu masks (as k_masks).
__global__ __launch_bounds__(GMPC_THREADS) void k_rvjp_acts(RvjpArgs a, uint32_t* masks) {
  extern __shared__ __attribute__((aligned(16))) char smem_ra[];
  float4* const actA = reinterpret_cast<float4*>(smem_ra);
  float4* const actB = actA + a.aw;
  const int tid = threadIdx.x, n = a.n, m = a.m, T = a.T, NS = a.B * T, Lh = a.dyn.L - 1;
  const int s0 = blockIdx.x * 4;
  int si[4];
  unsigned wbits = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    si[c] = min(s0 + c, NS - 1);
    wbits |= (s0 + c < NS ? 1u : 0u) << c;
  }
  for (int i = tid; i < n + m; i += GMPC_THREADS) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int b = si[c] / T, t = si[c] - b * T;
      f4set(v, c, i < n ? a.X[((size_t)b * (T + 1) + t) * n + i] : a.U[(size_t)si[c] * m + (i - n)]);
    }
    actA[i] = v;
    rv_store4(a.acts + a.dr.aoff[0] + i, a.dr.stride, wbits, si, v);
  }
  __syncthreads();
  float4* in = actA;
  float4* out = actB;
  for (int l = 0; l < Lh; ++l) {
    const int N = a.dyn.dims[l + 1];
    hidden_layer(a.dyn.W[l], a.dyn.b[l], a.dyn.dims[l], N, in, out, masks + ((size_t)s0 * Lh + l) * GMPC_MW,
                 (size_t)Lh * GMPC_MW, wbits);
    if (tid < N) rv_store4(a.acts + a.dr.aoff[l + 1] + tid, a.dr.stride, wbits, si, out[tid]);
    __syncthreads();
    float4* tmp = in; in = out; out = tmp;
  }
}

// Host-side launchers ---------------------------------------------------------------------------
static int rv_width(int n, int m, const MlpDesc& d, const MlpDesc* d2) {
  int w = n + m;
  for (int l = 0; l <= d.L; ++l) w = d.dims[l] > w ? d.dims[l] : w;
  if (d2) for (int l = 0; l <= d2->L; ++l) w = d2->dims[l] > w ? d2->dims[l] : w;
  return (w + 3) & ~3;
}

void gmpc_launch_rvjp_sweep(int B, int n, int m, int T, const MlpDesc& dyn, const MlpDesc& cost, const float* mpc_w,
                            const float* X, const float* U, const float* goal, const float* gX, const float* gc,
                            const uint32_t* masks, float* gx0, float* gU, float* ggoal, float* gm, float* cacts,
                            float* cdels, float* dels, const MlpRows& dr, const MlpRows& cr, hipStream_t s) {
  RvjpArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.n = n; a.m = m; a.T = T; a.dyn = dyn; a.cost = cost; a.mpc_w = mpc_w;
  a.X = X; a.U = U; a.goal = goal; a.gX = gX; a.gc = gc; a.masks = masks;
  a.gx0 = gx0; a.gU = gU; a.ggoal = ggoal; a.gm = gm; a.cacts = cacts; a.cdels = cdels;
  a.dels = dels; a.dr = dr; a.cr = cr;
  a.aw = rv_width(n, m, dyn, &cost);
  const int cw = cr.aoff[cost.L - 1] + cost.dims[cost.L - 1];   // the cost-layer inputs a_0 .. a_{Lc}
  // n <= 1024, m <= 64, widths <= 256: at most 100 KB
  const size_t lds = ((size_t)2 * a.aw + GMPC_THREADS + n + cw) * sizeof(float4);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rvjp_sweep),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)hipGetLastError();
    attr = true;
  }
  hipLaunchKernelGGL(k_rvjp_sweep, dim3((B + 3) / 4), dim3(GMPC_THREADS), lds, s, a);
}

void gmpc_launch_rvjp_acts(int B, int n, int m, int T, const MlpDesc& dyn, const float* X, const float* U, float* acts,
                           const MlpRows& dr, uint32_t* masks, hipStream_t s) {
  RvjpArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.n = n; a.m = m; a.T = T; a.dyn = dyn; a.X = X; a.U = U; a.acts = acts; a.dr = dr;
  a.aw = rv_width(n, m, dyn, nullptr);
  const int NS = B * T;
  hipLaunchKernelGGL(k_rvjp_acts, dim3((NS + 3) / 4), dim3(GMPC_THREADS), 2 * (size_t)a.aw * sizeof(float4), s, a,
                     masks);
}
