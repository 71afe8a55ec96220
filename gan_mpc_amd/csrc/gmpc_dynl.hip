// The LSTM variant of the dynamics model (reference dynamics/nn.py:37-57, dynamics_model.py:20-48):
//   xc = [x (nx), c (F), h (F)];  q0 = [x, u];  (c', h') = OptimizedLSTMCell((c, h), q0)  (gates i, f, g, o:
//   i, f, o sigmoid, g tanh, c' = f c + i g, h' = o tanh(c'));  next_x = tail(h') + x with a relu MLP tail;
//   next_xc = [next_x, c', h'].
// Everything after the dynamics step is generic in the state size N = nx + 2F (Riccati sweep, adjoint,
// bilevel solve: the kernels of gmpc_backward.hip / gmpc_large.hip on the [A_t | B_t] this file emits),
// and the staging cost / L2 loss / critic see xc[:nx] only (their `ng` argument).
//
// Two kernels: the trajectory kernel (rollout + per-step costs; as line-search candidate evaluator it takes
// the (trajectory, halving) work list of gmpc_linesearch.hip's k_ls_place and applies the DDP feedback
// u = U_t + alpha k_t + K_t (x_new - X_t)), and the Jacobian kernel (forward recompute at (xc_t, u_t), then
// the chain rule through the cell and the tail).  One 256-thread workgroup per trajectory / sample; the
// reference's default is the MLP variant (yaml `use: "mlp"`), so these are written for clarity, not tuned.
#include "gmpc_launch.h"

namespace {

__device__ __forceinline__ void dense_layer(const float* __restrict__ W, const float* __restrict__ bias, int K,
                                            int Nout, const float* in, float* out, bool relu) {
  for (int j = threadIdx.x; j < Nout; j += GMPC_THREADS) {
    float acc = bias[j];
    for (int k = 0; k < K; ++k) acc = fmaf(in[k], W[(size_t)k * Nout + j], acc);
    out[j] = relu ? fmaxf(acc, 0.f) : acc;
  }
}

// sum over the workgroup of two per-thread partials; result to every thread
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[wave] = a; red[4 + wave] = b; }
  __syncthreads();
  a = (red[0] + red[1]) + (red[2] + red[3]);
  b = (red[4] + red[5]) + (red[6] + red[7]);
}

// gate pre-activations z = [x, u] Wx + h Wh + b, then the cell: writes c', h' into cn / hn (LDS, F each)
// and leaves the activated gates in zg (i, f, g, o blocks) for the Jacobian kernel.
__device__ __forceinline__ void lstm_cell(const DynlDesc& d, const float* x, const float* u, const float* c,
                                          const float* h, float* zg, float* cn, float* hn, float* tc) {
  const int F = d.F, G4 = 4 * F, nx = d.nx, m = d.m;
  for (int j = threadIdx.x; j < G4; j += GMPC_THREADS) {
    float acc = d.b[j];
    for (int k = 0; k < nx; ++k) acc = fmaf(x[k], d.Wx[(size_t)k * G4 + j], acc);
    for (int k = 0; k < m; ++k) acc = fmaf(u[k], d.Wx[(size_t)(nx + k) * G4 + j], acc);
    for (int k = 0; k < F; ++k) acc = fmaf(h[k], d.Wh[(size_t)k * G4 + j], acc);
    const bool is_g = j >= 2 * F && j < 3 * F;
    zg[j] = is_g ? tanhf(acc) : sigmoidf_(acc);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < F; j += GMPC_THREADS) {
    const float c2 = zg[F + j] * c[j] + zg[j] * zg[2 * F + j];
    const float t = tanhf(c2);
    cn[j] = c2;
    if (tc) tc[j] = t;
    hn[j] = zg[3 * F + j] * t;
  }
  __syncthreads();
}

}  // namespace

template <bool LS>
__global__ __launch_bounds__(GMPC_THREADS) void k_dynl_traj(DynlTrajArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_dl[];
  const DynlDesc& d = a.d;
  const int nx = d.nx, F = d.F, m = d.m, N = nx + 2 * F, T = a.T, W = a.width;
  float* xc = reinterpret_cast<float*>(smem_dl);   // N   current state [x, c, h]
  float* xn = xc + N;                              // N   next state
  float* uv = xn + N;                              // m
  float* zg = uv + m;                              // 4F  activated gates
  float* act0 = zg + 4 * F;                        // W
  float* act1 = act0 + W;                          // W
  __shared__ float red[8];
  const int tid = threadIdx.x;
  int b = blockIdx.x, item = blockIdx.x;
  float alpha = 0.f;
  if (LS) {
    if (item >= *a.nitems) return;
    b = a.item_b[item];
    alpha = a.alpha_0;
    for (int k = a.item_k[item]; k > 0; --k) alpha *= 0.5f;
  }
  const float* x_init = LS ? a.Xn + (size_t)b * (T + 1) * N : a.x0 + (size_t)b * N;
  float* Xout = LS ? a.Xc + (size_t)item * (T + 1) * N : a.X + (size_t)b * (T + 1) * N;
  for (int i = tid; i < N; i += GMPC_THREADS) { const float v = x_init[i]; xc[i] = v; Xout[i] = v; }
  __syncthreads();
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]), w2 = sigmoidf_(a.mpc_w[2]);
  const float al = GMPC_ALPHA;
  float total = 0.f;
  for (int t = 0; t < T; ++t) {
    const size_t bt = (size_t)b * T + t;
    // control of this step
    if (!LS) {
      for (int j = tid; j < m; j += GMPC_THREADS) uv[j] = a.U[bt * m + j];
    } else {
      const float* xbar = a.Xn + ((size_t)b * (T + 1) + t) * N;
      const int wave = tid >> 6, lane = tid & 63;
      for (int j = wave; j < m; j += GMPC_THREADS / 64) {
        const float* Kr = a.Kg + (bt * m + j) * N;
        float v = 0.f;
        for (int i = lane; i < N; i += 64) v = fmaf(Kr[i], xc[i] - xbar[i], v);
        v = wave_sum(v);
        if (lane == 0) {
          const float un = a.Un[bt * m + j] + (alpha * a.kg[bt * m + j] + v);
          uv[j] = un;
          a.Uc[((size_t)item * T + t) * m + j] = un;
        }
      }
    }
    __syncthreads();
    // staging cost of (xc_t, u_t): the x part against goal_t
    float uu = 0.f, dd = 0.f;
    for (int j = tid; j < m; j += GMPC_THREADS) uu = fmaf(uv[j], uv[j], uu);
    for (int i = tid; i < nx; i += GMPC_THREADS) {
      const float dv = xc[i] - a.goal[((size_t)b * (T + 1) + t) * nx + i];
      dd = fmaf(dv, dv, dd);
    }
    block_sum2(uu, dd, red);
    const float ct = w0 * (sqrtf(uu + al * al) - al) + w1 * (sqrtf(dd + al * al) - al);
    total += ct;
    if (!LS && a.costs && tid == 0) a.costs[(size_t)b * (T + 1) + t] = ct;
    // dynamics step
    lstm_cell(d, xc, uv, xc + nx, xc + nx + F, zg, xn + nx, xn + nx + F, nullptr);
    float* in = xn + nx + F;      // h'
    float* o0 = act0;
    float* o1 = act1;
    for (int l = 0; l < d.tail.L; ++l) {
      dense_layer(d.tail.W[l], d.tail.b[l], d.tail.dims[l], d.tail.dims[l + 1], in, o0, l + 1 < d.tail.L);
      __syncthreads();
      in = o0;
      float* sw = o0; o0 = o1; o1 = sw;
    }
    for (int i = tid; i < nx; i += GMPC_THREADS) xn[i] = in[i] + xc[i];
    __syncthreads();
    for (int i = tid; i < N; i += GMPC_THREADS) {
      const float v = xn[i];
      xc[i] = v;
      Xout[(size_t)(t + 1) * N + i] = v;
    }
    __syncthreads();
  }
  // terminal cost w2 |cost MLP(xc_T)|^2
  {
    float* in = xc;
    float* o0 = act0;
    float* o1 = act1;
    for (int l = 0; l < a.cost.L; ++l) {
      dense_layer(a.cost.W[l], a.cost.b[l], a.cost.dims[l], a.cost.dims[l + 1], in, o0, l + 1 < a.cost.L);
      __syncthreads();
      in = o0;
      float* sw = o0; o0 = o1; o1 = sw;
    }
    float yy = 0.f, zero = 0.f;
    for (int j = tid; j < a.cost.dims[a.cost.L]; j += GMPC_THREADS) yy = fmaf(in[j], in[j], yy);
    block_sum2(yy, zero, red);
    const float cT = w2 * yy;
    total += cT;
    if (tid == 0) {
      if (LS) {
        a.objc[item] = total;
      } else {
        if (a.costs) a.costs[(size_t)b * (T + 1) + T] = cT;
        if (a.obj) a.obj[b] = total;
      }
    }
  }
}

static size_t dynl_traj_lds(const DynlTrajArgs& a) {
  const int N = a.d.nx + 2 * a.d.F;
  return ((size_t)2 * N + a.d.m + 4 * a.d.F + 2 * (size_t)a.width) * sizeof(float);
}

static int dynl_width(const DynlDesc& d, const MlpDesc* cost) {
  int w = d.nx + 2 * d.F;
  for (int l = 0; l <= d.tail.L; ++l) w = d.tail.dims[l] > w ? d.tail.dims[l] : w;
  if (cost)
    for (int l = 0; l <= cost->L; ++l) w = cost->dims[l] > w ? cost->dims[l] : w;
  return w;
}

void gmpc_launch_dynl_rollout(DynlTrajArgs a, hipStream_t s) {
  a.width = dynl_width(a.d, &a.cost);
  hipLaunchKernelGGL(k_dynl_traj<false>, dim3(a.B), dim3(GMPC_THREADS), dynl_traj_lds(a), s, a);
}

void gmpc_launch_dynl_candidates(DynlTrajArgs a, int max_items, hipStream_t s) {
  a.width = dynl_width(a.d, &a.cost);
  hipLaunchKernelGGL(k_dynl_traj<true>, dim3(max_items), dim3(GMPC_THREADS), dynl_traj_lds(a), s, a);
}

// ------------------------------------------------------------------------------------------------
// Jacobians  [A | B] = d next_xc / d [xc | u]  at (xc_t, u_t): N rows of N + m columns, columns ordered
// x | c | h | u.  Sample s = blockIdx.x is trajectory b = s / nt at step t = t0 + tstride * (s % nt)
// (nt = T, tstride = 1, t0 = 0: all steps, output row-major [B][T]; nt = 1: one step for the
// step-major large-state pass, output [B]).
//   rows c':  dc'/d. = g i(1-i) dz_i + c f(1-f) dz_f + i (1-g^2) dz_g  (+ f on the c block's diagonal)
//   rows h':  dh'/d. = o (1 - tanh^2 c') dc'/d. + tanh(c') o (1-o) dz_o
//   rows x':  Jt dh'/d. (+ I on the x block), Jt = d tail / d h' through the relu masks
//   dz/d[x, u] = Wx^T, dz/dh = Wh^T, dz/dc = 0.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GMPC_THREADS) void k_dynl_jac(int B, int T, int nt, int t0, DynlDesc d,
                                                           const float* X, const float* U, const int* active,
                                                           float* AB, int width) {
  extern __shared__ __attribute__((aligned(16))) char smem_dj[];
  const int nx = d.nx, F = d.F, m = d.m, N = nx + 2 * F, NM = N + m, G4 = 4 * F;
  float* xc = reinterpret_cast<float*>(smem_dj);   // N
  float* uv = xc + N;                              // m
  float* zg = uv + m;                              // 4F activated gates
  float* cn = zg + G4;                             // F  c'
  float* hn = cn + F;                              // F  h'
  float* tc = hn + F;                              // F  tanh(c')
  float* act0 = tc + F;                            // width
  float* act1 = act0 + width;                      // width
  float* gv = act1 + width;                        // width  reverse-mode vector through the tail
  float* gw = gv + width;                          // width
  float* mask = gw + width;                        // GMPC_MAX_LAYERS * width relu masks of the tail
  const int tid = threadIdx.x;
  const int sidx = blockIdx.x, b = sidx / nt, t = t0 + (sidx - b * nt);
  if (active != nullptr && active[b] == 0) return;
  float* out = AB + (size_t)sidx * N * NM;
  for (int i = tid; i < N; i += GMPC_THREADS) xc[i] = X[((size_t)b * (T + 1) + t) * N + i];
  for (int j = tid; j < m; j += GMPC_THREADS) uv[j] = U[((size_t)b * T + t) * m + j];
  __syncthreads();
  lstm_cell(d, xc, uv, xc + nx, xc + nx + F, zg, cn, hn, tc);
  // tail forward: relu masks
  {
    float* in = hn;
    float* o0 = act0;
    float* o1 = act1;
    for (int l = 0; l + 1 < d.tail.L; ++l) {
      const int K = d.tail.dims[l], No = d.tail.dims[l + 1];
      for (int j = tid; j < No; j += GMPC_THREADS) {
        float acc = d.tail.b[l][j];
        for (int k = 0; k < K; ++k) acc = fmaf(in[k], d.tail.W[l][(size_t)k * No + j], acc);
        mask[l * width + j] = acc > 0.f ? 1.f : 0.f;
        o0[j] = fmaxf(acc, 0.f);
      }
      __syncthreads();
      in = o0;
      float* sw = o0; o0 = o1; o1 = sw;
    }
  }
  // rows c' (nx .. nx+F) and h' (nx+F .. N): thread per (row j, column col)
  const float* c = xc + nx;
  for (int e = tid; e < F * NM; e += GMPC_THREADS) {
    const int j = e / NM, col = e - j * NM;
    // dz_gate[j] / d col for the four gates
    float zi = 0.f, zf = 0.f, zgg = 0.f, zo = 0.f;
    const float* wrow = nullptr;
    if (col < nx) wrow = d.Wx + (size_t)col * G4;
    else if (col >= N) wrow = d.Wx + (size_t)(nx + col - N) * G4;
    else if (col >= nx + F) wrow = d.Wh + (size_t)(col - nx - F) * G4;
    if (wrow) { zi = wrow[j]; zf = wrow[F + j]; zgg = wrow[2 * F + j]; zo = wrow[3 * F + j]; }
    const float ig = zg[j], fg = zg[F + j], gg = zg[2 * F + j], og = zg[3 * F + j];
    float dc2 = (gg * ig * (1.f - ig)) * zi + (c[j] * fg * (1.f - fg)) * zf + (ig * (1.f - gg * gg)) * zgg;
    if (col == nx + j) dc2 += fg;
    const float dh2 = (og * (1.f - tc[j] * tc[j])) * dc2 + (tc[j] * og * (1.f - og)) * zo;
    out[(size_t)(nx + j) * NM + col] = dc2;
    out[(size_t)(nx + F + j) * NM + col] = dh2;
  }
  __syncthreads();      // the dh' rows are read back below by other threads of this workgroup
  // rows x': for each output r, the reverse pass through the tail gives g = d tail_r / d h' (F), then
  // row r = g^T dh'/d. (+ 1 at column r)
  const int L = d.tail.L;
  for (int r = 0; r < nx; ++r) {
    // seed: column r of the last layer's kernel
    {
      const int K = d.tail.dims[L - 1], No = d.tail.dims[L];
      for (int k = tid; k < K; k += GMPC_THREADS) gv[k] = d.tail.W[L - 1][(size_t)k * No + r];
    }
    __syncthreads();
    float* gin = gv;
    float* gout = gw;
    for (int l = L - 2; l >= 0; --l) {
      const int K = d.tail.dims[l], No = d.tail.dims[l + 1];   // layer l: K -> No, gin has No entries
      for (int k = tid; k < K; k += GMPC_THREADS) {
        float acc = 0.f;
        for (int j = 0; j < No; ++j) acc = fmaf(d.tail.W[l][(size_t)k * No + j], gin[j] * mask[l * width + j], acc);
        gout[k] = acc;
      }
      __syncthreads();
      float* sw = gin; gin = gout; gout = sw;
    }
    // gin = d tail_r / d h' (F entries)
    for (int col = tid; col < NM; col += GMPC_THREADS) {
      float acc = col == r ? 1.f : 0.f;
      for (int j = 0; j < F; ++j) acc = fmaf(gin[j], out[(size_t)(nx + F + j) * NM + col], acc);
      out[(size_t)r * NM + col] = acc;
    }
    __syncthreads();
  }
}

void gmpc_launch_dynl_jac(int B, int T, int nt, int t0, const DynlDesc& d, const float* X, const float* U,
                          const int* active, float* AB, hipStream_t s) {
  const int N = d.nx + 2 * d.F;
  const int width = dynl_width(d, nullptr);
  const size_t lds = ((size_t)N + d.m + 4 * d.F + 3 * d.F + 4 * (size_t)width + (size_t)GMPC_MAX_LAYERS * width) *
                     sizeof(float);
  hipLaunchKernelGGL(k_dynl_jac, dim3((unsigned)B * nt), dim3(GMPC_THREADS), lds, s, B, T, nt, t0, d, X, U, active,
                     AB, width);
}

// x columns of xc rows (the critic / loss side sees xc[:nx]) and the way back with zeros on the carry
__global__ void k_cols_gather(long rows, int n, int nx, const float* src, float* dst) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * nx) return;
  const long r = e / nx;
  const int i = (int)(e - r * nx);
  dst[e] = src[r * n + i];
}
__global__ void k_cols_scatter(long rows, int n, int nx, const float* src, float* dst) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * n) return;
  const long r = e / n;
  const int i = (int)(e - r * n);
  dst[e] = i < nx ? src[r * nx + i] : 0.f;
}
void gmpc_launch_cols_gather(long rows, int n, int nx, const float* src, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_cols_gather, dim3((unsigned)((rows * nx + 255) / 256)), dim3(256), 0, s, rows, n, nx, src, dst);
}
void gmpc_launch_cols_scatter(long rows, int n, int nx, const float* src, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_cols_scatter, dim3((unsigned)((rows * n + 255) / 256)), dim3(256), 0, s, rows, n, nx, src, dst);
}

// ------------------------------------------------------------------------------------------------
// Curvature of the LSTM dynamics for the bilevel Hessian solve:  Phi = d^2/dz^2 [lam_{t+1} . f(z_t)],
// z = (xc, u), (N+m) x (N+m), columns x | c | h | u  (oracle lstm_dynamics_curvature).  The reference solves with
// the dense Hessian of the rollout objective (policy/optimizers.py:86-90), which is the Hessian of the LQ model
// with Q + Phi_xx, R + Phi_uu, M = Phi_xu; the relu tail is piecewise linear, so all of Phi sits in the cell:
// with w_h = Jt^T lam_x + lam_h, w_c = lam_c, unit j has phi_j = w_h o tanh(c') + w_c c', c' = f c + i g, and
// Phi = sum_j D_j^T H_j D_j (H_j: 5 x 5 in (z_i, z_f, z_g, z_o, c_j); D_j: weight columns and a unit vector).
// Same sample indexing as k_dynl_jac.  One workgroup per sample, row a of Phi at a time: the row's
// contraction with H is staged in LDS, threads then run over the columns c >= a (Phi is symmetric).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GMPC_THREADS) void k_dynl_curv(int B, int T, int nt, int t0, DynlDesc d, const float* X,
                                                            const float* U, const float* adj, const int* active,
                                                            float* Phi, int width) {
  extern __shared__ __attribute__((aligned(16))) char smem_dc[];
  const int nx = d.nx, F = d.F, m = d.m, N = nx + 2 * F, NM = N + m, G4 = 4 * F;
  float* xc = reinterpret_cast<float*>(smem_dc);   // N
  float* uv = xc + N;                              // m
  float* zg = uv + m;                              // 4F
  float* cn = zg + G4;                             // F
  float* hn = cn + F;                              // F
  float* tc = hn + F;                              // F
  float* act0 = tc + F;                            // width
  float* act1 = act0 + width;                      // width
  float* gv = act1 + width;                        // width
  float* gw = gv + width;                          // width
  float* mask = gw + width;                        // GMPC_MAX_LAYERS * width
  float* Hs = mask + GMPC_MAX_LAYERS * width;      // F x 25
  float* ta = Hs + 25 * F;                         // 4F: sum_q wa[qF + j] H_j[q][r]
  const int tid = threadIdx.x;
  const int sidx = blockIdx.x, b = sidx / nt, t = t0 + (sidx - b * nt);
  if (active != nullptr && active[b] == 0) return;
  float* out = Phi + (size_t)sidx * NM * NM;
  const float* lam = adj + ((size_t)b * (T + 1) + t + 1) * N;
  for (int i = tid; i < N; i += GMPC_THREADS) xc[i] = X[((size_t)b * (T + 1) + t) * N + i];
  for (int j = tid; j < m; j += GMPC_THREADS) uv[j] = U[((size_t)b * T + t) * m + j];
  __syncthreads();
  lstm_cell(d, xc, uv, xc + nx, xc + nx + F, zg, cn, hn, tc);
  // tail forward (relu masks), then ONE reverse pass with the seed lam_x: gin = Jt^T lam_x
  {
    float* in = hn;
    float* o0 = act0;
    float* o1 = act1;
    for (int l = 0; l + 1 < d.tail.L; ++l) {
      const int K = d.tail.dims[l], No = d.tail.dims[l + 1];
      for (int j = tid; j < No; j += GMPC_THREADS) {
        float acc = d.tail.b[l][j];
        for (int k = 0; k < K; ++k) acc = fmaf(in[k], d.tail.W[l][(size_t)k * No + j], acc);
        mask[l * width + j] = acc > 0.f ? 1.f : 0.f;
        o0[j] = fmaxf(acc, 0.f);
      }
      __syncthreads();
      in = o0;
      float* sw = o0; o0 = o1; o1 = sw;
    }
  }
  const int L = d.tail.L;
  {
    const int K = d.tail.dims[L - 1], No = d.tail.dims[L];     // No == nx
    for (int k = tid; k < K; k += GMPC_THREADS) {
      float acc = 0.f;
      for (int r = 0; r < No; ++r) acc = fmaf(d.tail.W[L - 1][(size_t)k * No + r], lam[r], acc);
      gv[k] = acc;
    }
  }
  __syncthreads();
  float* gin = gv;
  float* gout = gw;
  for (int l = L - 2; l >= 0; --l) {
    const int K = d.tail.dims[l], No = d.tail.dims[l + 1];
    for (int k = tid; k < K; k += GMPC_THREADS) {
      float acc = 0.f;
      for (int j = 0; j < No; ++j) acc = fmaf(d.tail.W[l][(size_t)k * No + j], gin[j] * mask[l * width + j], acc);
      gout[k] = acc;
    }
    __syncthreads();
    float* sw = gin; gin = gout; gout = sw;
  }
  // per-unit 5 x 5 Hessians
  const float* c = xc + nx;
  for (int j = tid; j < F; j += GMPC_THREADS) {
    const float ig = zg[j], fg = zg[F + j], gg = zg[2 * F + j], og = zg[3 * F + j], cj = c[j], tj = tc[j];
    const float wh = gin[j] + lam[nx + F + j], wc = lam[nx + j];
    const float di = ig * (1.f - ig), df = fg * (1.f - fg), dg = 1.f - gg * gg, dov = og * (1.f - og);
    const float ddi = di * (1.f - 2.f * ig), ddf = df * (1.f - 2.f * fg), ddg = -2.f * gg * dg,
                ddo = dov * (1.f - 2.f * og);
    const float alpha = wh * og * (1.f - tj * tj) + wc;
    const float beta = wh * og * (-2.f * tj) * (1.f - tj * tj);
    const float gamma = wh * (1.f - tj * tj);
    const float gc[5] = {gg * di, cj * df, ig * dg, 0.f, fg};
    float H[5][5];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int r = 0; r < 5; ++r) H[q][r] = beta * gc[q] * gc[r];
    H[0][0] += alpha * gg * ddi;
    H[0][2] += alpha * di * dg; H[2][0] += alpha * di * dg;
    H[1][1] += alpha * cj * ddf;
    H[1][4] += alpha * df; H[4][1] += alpha * df;
    H[2][2] += alpha * ig * ddg;
    H[3][3] += wh * tj * ddo;
#pragma unroll
    for (int q = 0; q < 5; ++q)
      if (q != 3) { H[3][q] += gamma * dov * gc[q]; H[q][3] += gamma * dov * gc[q]; }
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int r = 0; r < 5; ++r) Hs[j * 25 + q * 5 + r] = H[q][r];
  }
  __syncthreads();
  auto wrow_of = [&](int col) -> const float* {
    if (col < nx) return d.Wx + (size_t)col * G4;
    if (col >= N) return d.Wx + (size_t)(nx + col - N) * G4;
    if (col >= nx + F) return d.Wh + (size_t)(col - nx - F) * G4;
    return nullptr;                                   // a c column: no gate depends on c
  };
  for (int a = 0; a < NM; ++a) {
    const float* wa = wrow_of(a);
    const int ja = (a >= nx && a < nx + F) ? a - nx : -1;          // a is the column of c_{ja}
    // ta[r F + j] = sum_q D_j[q][a] H_j[q][r], r < 4 (gate rows) ; r == 4 kept separately per c column below
    for (int e = tid; e < G4; e += GMPC_THREADS) {
      const int r = e / F, j = e - r * F;
      float v = 0.f;
      if (wa) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v = fmaf(wa[q * F + j], Hs[j * 25 + q * 5 + r], v);
      } else if (j == ja) {
        v = Hs[j * 25 + 4 * 5 + r];
      }
      ta[e] = v;
    }
    __syncthreads();
    for (int cc = a + tid; cc < NM; cc += GMPC_THREADS) {
      const float* wcr = wrow_of(cc);
      float acc = 0.f;
      if (wcr) {
        for (int e = 0; e < G4; ++e) acc = fmaf(ta[e], wcr[e], acc);
      } else {
        // cc is the column of c_{jc}: D_jc[4][cc] = 1 -> sum_q D_jc[q][a] H_jc[q][4]
        const int jc = cc - nx;
        if (wa) {
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = fmaf(wa[q * F + jc], Hs[jc * 25 + q * 5 + 4], acc);
        } else if (jc == ja) {
          acc = Hs[jc * 25 + 24];
        }
      }
      out[(size_t)a * NM + cc] = acc;
      out[(size_t)cc * NM + a] = acc;
    }
    __syncthreads();
  }
}

void gmpc_launch_dynl_curv(int B, int T, int nt, int t0, const DynlDesc& d, const float* X, const float* U,
                           const float* adj, const int* active, float* Phi, hipStream_t s) {
  const int N = d.nx + 2 * d.F;
  const int width = dynl_width(d, nullptr);
  const size_t lds = ((size_t)N + d.m + 4 * d.F + 3 * d.F + 4 * (size_t)width + (size_t)GMPC_MAX_LAYERS * width +
                      25 * (size_t)d.F + 4 * (size_t)d.F) * sizeof(float);
  hipLaunchKernelGGL(k_dynl_curv, dim3((unsigned)B * nt), dim3(GMPC_THREADS), lds, s, B, T, nt, t0, d, X, U, adj,
                     active, Phi, width);
}

// HG [B][m][n+m] += Phi[n:, :]  and  T1 [B][n][n] += Phi[:n, :n]  (large-state bilevel pass, one step)
__global__ void k_add_phi(int n, int m, const float* Phi, float* HG, float* T1) {
  const int b = blockIdx.y, nm = n + m;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const float* P = Phi + (size_t)b * nm * nm;
  if (HG != nullptr && e < (long)m * nm) HG[(size_t)b * m * nm + e] += P[(size_t)n * nm + e];
  if (T1 != nullptr && e < (long)n * n) {
    const int i = (int)(e / n), j = (int)(e - (long)i * n);
    T1[(size_t)b * n * n + e] += P[(size_t)i * nm + j];
  }
}
void gmpc_launch_add_phi(int B, int n, int m, const float* Phi, float* HG, float* T1, hipStream_t s) {
  const long cnt = HG ? (long)m * (n + m) : (long)n * n;
  hipLaunchKernelGGL(k_add_phi, dim3((unsigned)((cnt + 255) / 256), B), dim3(256), 0, s, n, m, Phi, HG, T1);
}

// ------------------------------------------------------------------------------------------------
// Dynamics regression of the LSTM variant (reference norm/dynamics_trainer.py:14-47 with dynamics/nn.py:37-57;
// oracle lstm_dynamics_fit_loss_and_grad): per sequence, from the zero carry,
//   x_in_t = teacher_forcing ? xseq[t] : pred_{t-1};  [pred_t, c, h] = f([x_in_t, c, h], u_t);
//   loss = sum_t g^t |pred_t - next_xseq[t]|^2           (the carry is never teacher-forced)
// forward sweep then BPTT, one 256-thread workgroup per sequence.  Like k_dynfit the kernel emits, per
// (sequence, step), the row operands of the weight-gradient GEMMs -- acts row: [x_in, u | h_prev | tail inputs
// a_0 .. a_{L-1}], dels row: [dz (4F) | tail deltas d_1 .. d_L] -- and gWx = sum rows [x_in, u]^T dz,
// gWh = sum h_prev^T dz, gb = sum dz, tail layers as for the MLP run on k_wgrad_mfma afterwards.
// save row: activated gates (4F) | c_prev (F) | tanh(c') (F).
// ------------------------------------------------------------------------------------------------
struct DynlFitArgs {
  int B, S;
  DynlDesc d;
  const float* xseq; const float* useq; const float* yseq;   // [B][S][nx], [B][S][m], [B][S][nx]
  float gamma;
  int teacher_forcing;
  float* pred;           // [B][S][nx]
  float* acts; float* dels;
  MlpRows tail;          // the tail's columns behind [x_in, u | h_prev] / dz in a row, and the whole row's stride
  float* save;           // [B*S][6F]
  float* loss;           // [B]
  int width;
};

__global__ __launch_bounds__(GMPC_THREADS) void k_dynl_fit(DynlFitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_df[];
  const DynlDesc& d = a.d;
  const int nx = d.nx, F = d.F, m = d.m, G4 = 4 * F, S = a.S, W = a.width, L = d.tail.L, kin = nx + m;
  const int stride = a.tail.stride, abase = kin + F, dbase = G4;   // where the tail's a_0 / d_1 start
  float* xin = reinterpret_cast<float*>(smem_df);   // nx
  float* uv = xin + nx;                             // m
  float* cs = uv + m;                               // F  c
  float* hs = cs + F;                               // F  h
  float* cn = hs + F;                               // F
  float* hn = cn + F;                               // F
  float* tcv = hn + F;                              // F
  float* zg = tcv + F;                              // 4F
  float* act0 = zg + G4;                            // W
  float* act1 = act0 + W;                           // W
  float* lam = act1 + W;                            // nx  d loss / d pred through the next input
  float* dcv = lam + nx;                            // F
  float* dhv = dcv + F;                             // F
  float* dzv = dhv + F;                             // 4F
  float* disc = dzv + G4;                           // S
  __shared__ float red[8];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid == 0) { float g = 1.f; for (int t = 0; t < S; ++t) { disc[t] = g; g *= a.gamma; } }
  for (int j = tid; j < F; j += GMPC_THREADS) { cs[j] = 0.f; hs[j] = 0.f; }
  for (int i = tid; i < nx; i += GMPC_THREADS) xin[i] = a.xseq[((size_t)b * S) * nx + i];
  __syncthreads();
  float lsum = 0.f, zero = 0.f;
  // per-row offsets: acts [x_in,u | h_prev | a_0 | a_1 ...], dels [dz | d_1 | ... | d_L]
  for (int t = 0; t < S; ++t) {
    const size_t row = (size_t)b * S + t;
    float* arow = a.acts + row * stride;
    if (a.teacher_forcing && t > 0) {
      for (int i = tid; i < nx; i += GMPC_THREADS) xin[i] = a.xseq[row * nx + i];
    }
    for (int j = tid; j < m; j += GMPC_THREADS) uv[j] = a.useq[row * m + j];
    __syncthreads();
    for (int i = tid; i < kin; i += GMPC_THREADS) arow[i] = i < nx ? xin[i] : uv[i - nx];
    for (int j = tid; j < F; j += GMPC_THREADS) { arow[kin + j] = hs[j]; a.save[row * 6 * F + G4 + j] = cs[j]; }
    lstm_cell(d, xin, uv, cs, hs, zg, cn, hn, tcv);
    for (int j = tid; j < G4; j += GMPC_THREADS) a.save[row * 6 * F + j] = zg[j];
    for (int j = tid; j < F; j += GMPC_THREADS) a.save[row * 6 * F + 5 * F + j] = tcv[j];
    // tail
    float* in = hn;
    float* o0 = act0;
    float* o1 = act1;
    for (int l = 0; l < L; ++l) {
      const int K = d.tail.dims[l], N = d.tail.dims[l + 1], ao = abase + a.tail.aoff[l];
      for (int k = tid; k < K; k += GMPC_THREADS) arow[ao + k] = in[k];
      dense_layer(d.tail.W[l], d.tail.b[l], K, N, in, o0, l + 1 < L);
      __syncthreads();
      in = o0;
      float* sw = o0; o0 = o1; o1 = sw;
    }
    for (int i = tid; i < nx; i += GMPC_THREADS) {
      const float p = in[i] + xin[i];
      a.pred[row * nx + i] = p;
      const float df = p - a.yseq[row * nx + i];
      lsum = fmaf(disc[t] * df, df, lsum);
    }
    __syncthreads();
    for (int i = tid; i < nx; i += GMPC_THREADS) xin[i] = a.pred[row * nx + i];   // own elements
    for (int j = tid; j < F; j += GMPC_THREADS) { cs[j] = cn[j]; hs[j] = hn[j]; }
    __syncthreads();
  }
  block_sum2(lsum, zero, red);
  if (tid == 0) a.loss[b] = lsum;
  // ---------------------------------------------------------------- BPTT
  for (int i = tid; i < nx; i += GMPC_THREADS) lam[i] = 0.f;
  for (int j = tid; j < F; j += GMPC_THREADS) { dcv[j] = 0.f; dhv[j] = 0.f; }
  __syncthreads();
  const int doff_last = dbase + a.tail.doff[L - 1];
  for (int t = S - 1; t >= 0; --t) {
    const size_t row = (size_t)b * S + t;
    const float* arow = a.acts + row * stride;
    float* drow = a.dels + row * stride;
    const float* sv = a.save + row * 6 * F;
    // gout = 2 g^t (pred - y) + lam  -> delta at the tail's output (d_L) ; act0 holds the current delta
    for (int i = tid; i < nx; i += GMPC_THREADS) {
      const float g = 2.f * disc[t] * (a.pred[row * nx + i] - a.yseq[row * nx + i]) + lam[i];
      act0[i] = g;
      xin[i] = g;                 // kept: the residual path x' = tail + x_in carries gout to x_in
      drow[doff_last + i] = g;
    }
    __syncthreads();
    float* cur = act0;
    float* nxt = act1;
    for (int l = L - 1; l >= 0; --l) {
      const int K = d.tail.dims[l], N = d.tail.dims[l + 1], ao = abase + a.tail.aoff[l];
      // delta at layer l's input: W_l cur, masked by relu'(a_l) for l > 0 (a_0 = h' has no relu)
      for (int k = tid; k < K; k += GMPC_THREADS) {
        float acc = 0.f;
        const float* w = d.tail.W[l] + (size_t)k * N;
        for (int j = 0; j < N; ++j) acc = fmaf(w[j], cur[j], acc);
        if (l > 0) acc = arow[ao + k] > 0.f ? acc : 0.f;
        nxt[k] = acc;
      }
      __syncthreads();
      if (l > 0) {
        const int dof = dbase + a.tail.doff[l - 1];
        for (int k = tid; k < K; k += GMPC_THREADS) drow[dof + k] = nxt[k];
      }
      float* sw = cur; cur = nxt; nxt = sw;
    }
    // cur = d loss / d h' from the tail (F)
    for (int j = tid; j < F; j += GMPC_THREADS) {
      const float ig = sv[j], fg = sv[F + j], gg = sv[2 * F + j], og = sv[3 * F + j], cp = sv[G4 + j], tc = sv[5 * F + j];
      const float dh2 = cur[j] + dhv[j];
      const float dc2 = dcv[j] + dh2 * og * (1.f - tc * tc);
      dzv[j] = dc2 * gg * ig * (1.f - ig);
      dzv[F + j] = dc2 * cp * fg * (1.f - fg);
      dzv[2 * F + j] = dc2 * ig * (1.f - gg * gg);
      dzv[3 * F + j] = dh2 * tc * og * (1.f - og);
      dcv[j] = dc2 * fg;
    }
    __syncthreads();
    for (int j = tid; j < G4; j += GMPC_THREADS) drow[j] = dzv[j];
    // d h_prev = dz Wh^T ; d x_in = dz Wx^T[:nx] (+ gout) when the input was the previous prediction
    for (int k = tid; k < F; k += GMPC_THREADS) {
      float acc = 0.f;
      const float* w = d.Wh + (size_t)k * G4;
      for (int j = 0; j < G4; ++j) acc = fmaf(w[j], dzv[j], acc);
      dhv[k] = acc;
    }
    for (int i = tid; i < nx; i += GMPC_THREADS) {
      float acc = 0.f;
      if (!a.teacher_forcing) {
        const float* w = d.Wx + (size_t)i * G4;
        for (int j = 0; j < G4; ++j) acc = fmaf(w[j], dzv[j], acc);
        acc += xin[i];
      }
      lam[i] = acc;
    }
    __syncthreads();
  }
}

size_t gmpc_dynl_fit_stride(const DynlDesc& d) {
  // [x_in, u | h_prev] / dz in front of the tail's rows
  const int L = d.tail.L;
  const MlpRows r = mlp_rows(L, d.tail.dims);
  const size_t in = (size_t)d.nx + d.m + d.F + r.aoff[L - 1] + d.tail.dims[L - 1];
  const size_t out = 4 * (size_t)d.F + r.doff[L - 1] + d.tail.dims[L];
  return in > out ? in : out;
}

void gmpc_launch_dynl_fit(int B, int S, const DynlDesc& d, const float* xseq, const float* useq, const float* yseq,
                          float gamma, int teacher_forcing, float* pred, float* acts, float* dels,
                          const MlpRows& tail, float* save, float* loss, hipStream_t s) {
  DynlFitArgs a;
  a.B = B; a.S = S; a.d = d; a.xseq = xseq; a.useq = useq; a.yseq = yseq; a.gamma = gamma;
  a.teacher_forcing = teacher_forcing; a.pred = pred; a.acts = acts; a.dels = dels; a.tail = tail;
  a.save = save; a.loss = loss;
  a.width = dynl_width(d, nullptr);
  const size_t lds = ((size_t)2 * d.nx + d.m + 7 * (size_t)d.F + 8 * (size_t)d.F + 2 * (size_t)a.width + S + 8) *
                     sizeof(float);
  hipLaunchKernelGGL(k_dynl_fit, dim3(B), dim3(GMPC_THREADS), lds, s, a);
}
