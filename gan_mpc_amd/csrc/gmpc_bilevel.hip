// Upper-level ("bilevel") gradient pieces that are not the Riccati sweep itself.
//
// Reference arithmetic: policy/optimizers.py:61-73,78-105 (loss_grad_wrt_control, the dense
// Hessian solve -- here the equivalent structured solve, see k_riccati mode 1 -- and cost_vjp),
// norm/l2_policy.py:12-18.
#include "gmpc_launch.h"

// L2 loss  sum_dims mean_t (x - x*)^2  and its gradient wrt X.  `desired` has ng <= n columns: the loss sees
// the x part of xc (reference norm/l2_policy.py:15-16 splits xcseq at x_size), the gradient is zero on the rest.
__global__ __launch_bounds__(GMPC_THREADS) void k_l2loss(int B, int T, int n, int ng, const float* X,
                                                         const float* desired, float* loss,
                                                         float* lx) {
  __shared__ float sh[GMPC_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cnt = (T + 1) * n;
  const float inv = 1.0f / (float)(T + 1);
  float s = 0.f;
  for (int e = tid; e < cnt; e += blockDim.x) {
    const int r = e / n, i = e - r * n;
    float d = 0.f;
    if (i < ng) d = X[(size_t)b * cnt + e] - desired[((size_t)b * (T + 1) + r) * ng + i];
    s = fmaf(d, d, s);
    lx[(size_t)b * cnt + e] = 2.f * d * inv;
  }
  sh[tid] = s;
  __syncthreads();
  for (int o = GMPC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[b] = sh[0] * inv;
}

// a8: Bvec_t = B_t^T mu_{t+1} (+ lu_t), mu_T = lx_T, mu_t = lx_t + A_t^T mu_{t+1}.  One wave per trajectory.
// lu = dL/dU [B][T][m] of a loss that depends on the controls (gmpc_bilevel_grad_cotangent), or null: then the
// term is not added at all (adding 0 would turn a -0 of B^T mu into +0).
__global__ __launch_bounds__(64) void k_bvec(int /*B*/, int T, int n, int m, const float* AB,
                                             const float* lx, const float* lu, float* Bvec) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ABs = reinterpret_cast<float*>(smem);
  float* mu = ABs + n * (n + m);
  float* tv = mu + n;
  const int lane = threadIdx.x, b = blockIdx.x, nm = n + m;
  for (int i = lane; i < n; i += 64) mu[i] = lx[((size_t)b * (T + 1) + T) * n + i];
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    const size_t bt = (size_t)b * T + t;
    for (int e = lane; e < n * nm; e += 64) ABs[e] = AB[bt * n * nm + e];
    __syncthreads();
    for (int j = lane; j < m; j += 64) {
      float v = 0.f;
      for (int i = 0; i < n; ++i) v = fmaf(ABs[i * nm + n + j], mu[i], v);
      if (lu != nullptr) v = v + lu[bt * m + j];
      Bvec[bt * m + j] = v;
    }
    for (int c = lane; c < n; c += 64) {
      float v = 0.f;
      for (int i = 0; i < n; ++i) v = fmaf(ABs[i * nm + c], mu[i], v);
      tv[c] = lx[((size_t)b * (T + 1) + t) * n + c] + v;
    }
    __syncthreads();
    for (int c = lane; c < n; c += 64) mu[c] = tv[c];
    __syncthreads();
  }
}

// a11: per trajectory, the theta-gradient of  H . grad_U J(U; theta)  =  directional derivative of the
// total cost along (dX, H).  mpc_w part is finished here; for the cost MLP the kernel emits the layer
// inputs (primal row b, tangent row B+b) and the matching adjoints, and the weight gradients are the
// row-sum GEMMs  gW_l = sum_rows cact_l^T cdel_l,  gb_l = sum of the primal adjoint rows.
__global__ __launch_bounds__(GMPC_THREADS) void k_costvjp(int B, int T, int n, int m, MlpDesc cm,
                                                          const float* mpc_w, float sign,
                                                          const float* X, const float* U,
                                                          const float* goal, int ng, const float* Hc,
                                                          const float* dX, float* gmpc /*[B][3]*/,
                                                          float* cact, float* cdel, MlpRows rows) {
  // bufA holds the terminal state (n rows, may exceed the 256-wide layers); dynamic LDS
  extern __shared__ __attribute__((aligned(16))) char smem_cv[];
  float4* bufA = reinterpret_cast<float4*>(smem_cv);
  float4* bufB = bufA + (n > GMPC_THREADS ? n : GMPC_THREADS);
  __shared__ float zpos[GMPC_MAX_LAYERS][GMPC_THREADS];
  __shared__ float red[2][GMPC_THREADS / 64];
  __shared__ float yv[2][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x, stride = rows.stride;
  const float al = GMPC_ALPHA;
  const float r0 = mpc_w[0], r1 = mpc_w[1], r2 = mpc_w[2];
  const float w0 = sigmoidf_(r0), w1 = sigmoidf_(r1), w2 = sigmoidf_(r2);
  // ---- stage sums: each wave takes every 4th step
  float du_dir = 0.f, dx_dir = 0.f;
  for (int t = wave; t < T; t += GMPC_THREADS / 64) {
    float uu = 0.f, uh = 0.f, dd = 0.f, dxd = 0.f;
    for (int j = lane; j < m; j += 64) {
      const float u = U[((size_t)b * T + t) * m + j];
      uu = fmaf(u, u, uu);
      uh = fmaf(u, Hc[((size_t)b * T + t) * m + j], uh);
    }
    for (int i = lane; i < ng; i += 64) {        // the staging cost sees xc[:ng]
      const size_t xi = ((size_t)b * (T + 1) + t) * n + i;
      const float d = X[xi] - goal[((size_t)b * (T + 1) + t) * ng + i];
      dd = fmaf(d, d, dd);
      dxd = fmaf(d, dX[xi], dxd);
    }
    uu = wave_sum(uu); uh = wave_sum(uh); dd = wave_sum(dd); dxd = wave_sum(dxd);
    du_dir += uh / sqrtf(uu + al * al);
    dx_dir += dxd / sqrtf(dd + al * al);
  }
  if (lane == 0) { red[0][wave] = du_dir; red[1][wave] = dx_dir; }
  // ---- terminal: primal (.x) and tangent (.y) streams through the cost MLP
  const int Lc = cm.L - 1;
  const int fo = cm.dims[Lc + 1];
  float4* in = bufA;
  float4* out = bufB;
  for (int i = tid; i < n; i += blockDim.x) {
    const size_t xi = ((size_t)b * (T + 1) + T) * n + i;
    in[i] = make_float4(X[xi], dX[xi], 0.f, 0.f);
    cact[(size_t)b * stride + i] = X[xi];
    cact[(size_t)(B + b) * stride + i] = dX[xi];
  }
  __syncthreads();
  for (int l = 0; l < Lc; ++l) {
    const int K = cm.dims[l], N = cm.dims[l + 1], aoff = rows.aoff[l + 1];
    float4 acc[1] = {make_float4(tid < N ? cm.b[l][tid] : 0.f, 0.f, 0.f, 0.f)};
    dense_rows<1>(cm.W[l], K, N, tid, in, acc);
    if (tid < N) {
      const float mk = acc[0].x > 0.f ? 1.f : 0.f;
      zpos[l][tid] = mk;
      const float pa = acc[0].x * mk, ta = acc[0].y * mk;
      out[tid] = make_float4(pa, ta, 0.f, 0.f);
      cact[(size_t)b * stride + aoff + tid] = pa;
      cact[(size_t)(B + b) * stride + aoff + tid] = ta;
    }
    __syncthreads();
    float4* tmp = in; in = out; out = tmp;
  }
  if (tid < fo) {
    const int K = cm.dims[Lc];
    float y = cm.b[Lc][tid], yd = 0.f;
    for (int k = 0; k < K; ++k) {
      const float w = cm.W[Lc][(size_t)k * fo + tid];
      y = fmaf(w, in[k].x, y);
      yd = fmaf(w, in[k].y, yd);
    }
    yv[0][tid] = y;
    yv[1][tid] = yd;
  }
  __syncthreads();
  if (tid == 0) {
    float td = 0.f;
    for (int r = 0; r < fo; ++r) td = fmaf(yv[0][r], yv[1][r], td);
    td *= 2.f;
    const float du = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const float dx = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    gmpc[(size_t)b * 3 + 0] = sign * (w0 * (1.f - w0)) * du;
    gmpc[(size_t)b * 3 + 1] = sign * (w1 * (1.f - w1)) * dx;
    gmpc[(size_t)b * 3 + 2] = sign * (w2 * (1.f - w2)) * td;
  }
  // ---- backward: adjoints of (y, ydot) are (ydot, y) * 2 w2 * sign
  const float scale = 2.f * w2 * sign;
  if (tid < fo) {
    const int doff = rows.doff[Lc];
    const float yb = yv[1][tid] * scale, ydb = yv[0][tid] * scale;
    out[tid] = make_float4(yb, ydb, 0.f, 0.f);
    cdel[(size_t)b * stride + doff + tid] = yb;
    cdel[(size_t)(B + b) * stride + doff + tid] = ydb;
  }
  __syncthreads();
  for (int l = Lc; l >= 1; --l) {
    const int K = cm.dims[l + 1], N = cm.dims[l];
    float4 acc[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
    dense_rows<1>(cm.WT[l], K, N, tid, out, acc);
    if (tid < N) {
      const int doff = rows.doff[l - 1];
      const float mk = zpos[l - 1][tid];
      const float zb = acc[0].x * mk, zdb = acc[0].y * mk;
      in[tid] = make_float4(zb, zdb, 0.f, 0.f);
      cdel[(size_t)b * stride + doff + tid] = zb;
      cdel[(size_t)(B + b) * stride + doff + tid] = zdb;
    }
    __syncthreads();
    float4* tmp = in; in = out; out = tmp;
  }
}

// Host-side launchers ---------------------------------------------------------------------------
void gmpc_launch_l2loss(int B, int T, int n, int ng, const float* X, const float* desired, float* loss,
                        float* lx, hipStream_t s) {
  hipLaunchKernelGGL(k_l2loss, dim3(B), dim3(GMPC_THREADS), 0, s, B, T, n, ng, X, desired, loss, lx);
}
// The clamped set of a held box solve: one word per step (b, t), bit j = control j sits on a bound that
// the solve's full gradient pushes it against -- (U == lo and grad > 0) or (U == hi and grad < 0), exact comparisons (a
// NaN compares false: the entry is free).  It is the set the box solve's continuation test leaves out of its
// projected-gradient norm.  u_lo / u_hi [m] or null (unbounded on that side); m <= 32.
__global__ __launch_bounds__(256) void k_box_clamped(int steps, int m, const float* U, const float* grad,
                                                     const float* u_lo, const float* u_hi, uint32_t* clamped) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= steps) return;
  uint32_t w = 0u;
  for (int j = 0; j < m; ++j) {
    const float u = U[(size_t)s * m + j], g = grad[(size_t)s * m + j];
    const bool lo = u_lo != nullptr && u == u_lo[j] && g > 0.f;
    const bool hi = u_hi != nullptr && u == u_hi[j] && g < 0.f;
    if (lo || hi) w |= 1u << j;
  }
  clamped[s] = w;
}
void gmpc_launch_box_clamped(int B, int T, int m, const float* U, const float* grad, const float* u_lo,
                             const float* u_hi, uint32_t* clamped, hipStream_t s) {
  const int steps = B * T;
  hipLaunchKernelGGL(k_box_clamped, dim3((steps + 255) / 256), dim3(256), 0, s, steps, m, U, grad, u_lo, u_hi,
                     clamped);
}

void gmpc_launch_bvec(int B, int T, int n, int m, const float* AB, const float* lx, const float* lu, float* Bvec,
                      hipStream_t s) {
  const size_t lds = ((size_t)n * (n + m) + 2 * n) * sizeof(float);
  hipLaunchKernelGGL(k_bvec, dim3(B), dim3(64), lds, s, B, T, n, m, AB, lx, lu, Bvec);
}
void gmpc_launch_costvjp(int B, int T, int n, int m, const MlpDesc& cm, const float* mpc_w,
                         float sign, const float* X, const float* U, const float* goal, int ng,
                         const float* Hc, const float* dX, float* gmpc, float* cact, float* cdel,
                         const MlpRows& rows, hipStream_t s) {
  const size_t lds = ((size_t)(n > GMPC_THREADS ? n : GMPC_THREADS) + GMPC_THREADS) * sizeof(float4);
  hipLaunchKernelGGL(k_costvjp, dim3(B), dim3(GMPC_THREADS), lds, s, B, T, n, m, cm, mpc_w, sign, X, U,
                     goal, ng, Hc, dX, gmpc, cact, cdel, rows);
}

// a4: cost_model.get_cost(x, u, t, ...) for one (x, u) per workgroup, outside a rollout (reference
// cost/cost_model.py:20-42, cost/nn.py:23-29).  terminal == 0: the staging branch
// w0 (sqrt(u.u + a^2) - a) + w1 (sqrt(|x - goal_t|^2 + a^2) - a); otherwise the terminal branch
// w2 |MLP(x)|^2 of an ARBITRARY state (inside a rollout only x_T ever reaches it).
__global__ __launch_bounds__(GMPC_THREADS) void k_get_cost(int B, int n, int ng, int m, MlpDesc cm,
                                                           const float* mpc_w, const float* x,
                                                           const float* u, const float* goal_row,
                                                           int terminal, int width, float* out) {
  extern __shared__ __attribute__((aligned(16))) char smem_gc[];
  float* act0 = reinterpret_cast<float*>(smem_gc);
  float* act1 = act0 + width;
  __shared__ float red[2][GMPC_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const float al = GMPC_ALPHA;
  float s0 = 0.f, s1 = 0.f;
  if (!terminal) {
    for (int j = tid; j < m; j += GMPC_THREADS) { const float v = u[(size_t)b * m + j]; s0 = fmaf(v, v, s0); }
    for (int i = tid; i < ng; i += GMPC_THREADS) {
      const float d = x[(size_t)b * n + i] - goal_row[(size_t)b * ng + i];
      s1 = fmaf(d, d, s1);
    }
  } else {
    for (int i = tid; i < n; i += GMPC_THREADS) act0[i] = x[(size_t)b * n + i];
    __syncthreads();
    for (int l = 0; l < cm.L; ++l) {
      const int K = cm.dims[l], N = cm.dims[l + 1];
      const float* W = cm.W[l];
      for (int j = tid; j < N; j += GMPC_THREADS) {
        float acc = cm.b[l][j];
        for (int k = 0; k < K; ++k) acc = fmaf(act0[k], W[(size_t)k * N + j], acc);
        act1[j] = (l + 1 < cm.L) ? fmaxf(acc, 0.f) : acc;
      }
      __syncthreads();
      float* t_ = act0; act0 = act1; act1 = t_;
    }
    const int f = cm.dims[cm.L];
    for (int j = tid; j < f; j += GMPC_THREADS) s0 = fmaf(act0[j], act0[j], s0);
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (lane == 0) { red[0][wave] = s0; red[1][wave] = s1; }
  __syncthreads();
  if (tid == 0) {
    float t0 = 0.f, t1 = 0.f;
    for (int w = 0; w < GMPC_THREADS / 64; ++w) { t0 += red[0][w]; t1 += red[1][w]; }
    if (terminal) out[b] = sigmoidf_(mpc_w[2]) * t0;
    else out[b] = sigmoidf_(mpc_w[0]) * (sqrtf(t0 + al * al) - al) + sigmoidf_(mpc_w[1]) * (sqrtf(t1 + al * al) - al);
  }
}

void gmpc_launch_get_cost(int B, int n, int ng, int m, const MlpDesc& cm, const float* mpc_w, const float* x,
                          const float* u, const float* goal_row, int terminal, float* out, hipStream_t s) {
  int width = n;
  for (int l = 1; l <= cm.L; ++l) width = cm.dims[l] > width ? cm.dims[l] : width;
  hipLaunchKernelGGL(k_get_cost, dim3(B), dim3(GMPC_THREADS), 2 * (size_t)width * sizeof(float), s, B, n, ng, m,
                     cm, mpc_w, x, u, goal_row, terminal, width, out);
}
