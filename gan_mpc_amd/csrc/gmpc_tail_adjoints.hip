// The backward recursions v_t = s_t + A_t^T v_{t+1} over the held solution that follow the bilevel tail, from the
// state a preceding gmpc_bilevel_grad(_cotangent) leaves in the ctx: H = A^{-1} Bvec (A = d^2 J / dU^2), dX its
// tangent roll (dX_0 = 0), [A_t | B_t], the terminal QT and qT and, for the LSTM dynamics, the curvature
// Phi_t = lam_{t+1} . d^2 f_t that the Hessian solve used.  For any input p of J,
//
//   dL/dp = dL/dp|_(U fixed) - d/dp [ H . grad_U J ]   (H held fixed),   H . grad_U J = sum_t q_t . dX_t + r_t . H_t
//
//   mu_T  = lx_T,      mu_t  = lx_t + A_t^T mu_{t+1}                                  (the loss adjoint)
//   nu_T  = QT dX_T,   nu_t  = Q_t dX_t + Phi_x(x,u),t [dX_t; H_t] + A_t^T nu_{t+1}   (the second-order adjoint)
//   lam_T = qT,        lam_t = q_t + A_t^T lam_{t+1}                                  (the cost adjoint)
//   q_t = w1 d / s,  Q_t dX_t = w1 (dX_t / s - d (d . dX_t) / s^3)  on the goal columns,  d = x_t[:ng] - g_t,
//   s = sqrt(|d|^2 + alpha^2): formed from x_t and g_t in closed form (the stage Hessian k_riccati builds), not stored.
//
// gmpc_bilevel_grad_inputs: dL/dx0 = mu_0 - nu_0, dL/dg_t = (Q_t dX_t)[:ng] for t < T (the
// terminal cost does not read g_T: 0).  gmpc_bilevel_grad_dynamics (section 13, relu dynamics: Phi = 0) takes the
// per-step planes w = mu_{t+1} - nu_{t+1} and lam_{t+1} to its row kernel (gmpc_dyn_grads.hip).
#include "gmpc_launch.h"

#define GMPC_TA_THREADS 256
#define GMPC_TA_CHUNK 8                // steps staged per chunk (at most)
#define GMPC_TA_FLOATS_INPUTS 15872    // LDS budget of the staged steps (62 KB; mu_0 / nu_0 add 512 B)
#define GMPC_TA_FLOATS_PLANES 14336    // (56 KB; the parked adjoints add up to 6 KB)

// n <= 64, m <= 32 ([A_t | B_t] is kept), one workgroup per trajectory.  Wave 0 runs mu, wave 1 nu and, with PLANES,
// wave 2 lam; lane c owns state c and holds its adjoint in a register (lanes >= n hold 0).  A_t^T v is an unrolled
// NMAX-term sum of LDS reads of column c of A_t -- independent, issued back to back -- times v_i broadcast with
// v_readlane, so no LDS round trip orders one step after the other.  Steps come in chunks of K (<= GMPC_TA_CHUNK):
// every thread loads the chunk into LDS, the waves run it backwards, and the chunk's outputs go out behind the
// barrier.  PLANES = false (the inputs call): wave 1 adds the Phi rows and leaves Q_t dX_t[:ng], the goal gradient,
// in LDS over g_t (which only that lane reads); out come gx0 and, unless null, ggoal.  PLANES = true (the dynamics
// call): each sweep parks v_{t+1} per step; out come the planes w and lam [B][T][n].
template <int NMAX, bool PLANES>
__global__ __launch_bounds__(GMPC_TA_THREADS) void k_tail_adjoints(TailAdjArgs a, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem_ta[];
  const int T = a.T, n = a.n, ng = a.ng, m = a.m, nm = n + m, fa = n * nm;
  const bool curv = !PLANES && a.Phi != nullptr;
  const int fp = curv ? nm * nm : 0;
  float* S = reinterpret_cast<float*>(smem_ta);
  float* ABs = S;                           // [K][n][nm]
  float* LXs = ABs + K * fa;                // [K][n]
  float* DXs = LXs + K * n;                 // [K][n]
  float* Xs = DXs + K * n;                  // [K][n]
  float* Gs = Xs + K * n;                   // [K][ng]
  float* PHs = Gs + K * ng;                 // [K][nm][nm] (inputs call, LSTM dynamics)
  float* Hs = PHs + K * fp;                 // [K][m] (inputs call)
  float* Vs = Hs + (PLANES ? 0 : K * m);    // PLANES: [3][K][64] v_{t+1} of each sweep; else [2][64] mu_0, nu_0
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const int lc = lane < n ? lane : 0;   // idle lanes read a valid column and discard the result
  const float al = GMPC_ALPHA;
  const float w1 = sigmoidf_(a.mpc_w[1]);
  const size_t xrow = (size_t)b * (T + 1), urow = (size_t)b * T;

  // ---- terminal values (dX_T through LDS for the QT product)
  if (tid < n) Xs[tid] = a.dX[(xrow + T) * n + tid];
  if (!PLANES && a.ggoal != nullptr && tid < ng) a.ggoal[(xrow + T) * ng + tid] = 0.f;
  __syncthreads();
  float v_adj = 0.f;
  if (lane < n) {
    if (wave == 0) {
      v_adj = a.lx[(xrow + T) * n + lane];
    } else if (wave == 1) {
      const float* q = a.QT + ((size_t)b * n + lane) * n;
      float v = 0.f;
      for (int k = 0; k < n; ++k) v = fmaf(q[k], Xs[k], v);
      v_adj = v;
    } else if (PLANES && wave == 2) {
      v_adj = a.qT[(size_t)b * n + lane];
    }
  }
  __syncthreads();

  // A_t^T v for column lc: terms i >= n read row n - 1 and multiply the 0 that lane i holds
  auto atv = [&](const float* A, float v) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) acc = fmaf(A[(i < n ? i : n - 1) * nm + lc], __int_as_float(
                                                  __builtin_amdgcn_readlane(__float_as_int(v), i)), acc);
    return acc;
  };
  for (int tend = T; tend > 0; tend -= K) {
    const int t0 = tend - K > 0 ? tend - K : 0, kc = tend - t0;
    for (int e = tid; e < kc * fa; e += GMPC_TA_THREADS) ABs[e] = a.AB[(urow + t0) * fa + e];
    for (int e = tid; e < kc * n; e += GMPC_TA_THREADS) {
      LXs[e] = a.lx[(xrow + t0) * n + e];
      DXs[e] = a.dX[(xrow + t0) * n + e];
      Xs[e] = a.X[(xrow + t0) * n + e];
    }
    for (int e = tid; e < kc * ng; e += GMPC_TA_THREADS) Gs[e] = a.goal[(xrow + t0) * ng + e];
    if (!PLANES) {
      for (int e = tid; e < kc * fp; e += GMPC_TA_THREADS) PHs[e] = a.Phi[(urow + t0) * fp + e];
      for (int e = tid; e < kc * m; e += GMPC_TA_THREADS) Hs[e] = a.H[(urow + t0) * m + e];
    }
    __syncthreads();
    if (wave < (PLANES ? 3 : 2)) {
      for (int k = kc - 1; k >= 0; --k) {
        if (PLANES) Vs[(wave * K + k) * 64 + lane] = v_adj;   // v_{t0 + k + 1}
        float src = 0.f;                                      // this sweep's source term at step t0 + k
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
            // (the roundings of the two calls are pinned bitwise, and they differ: the dynamics call fuses the second
            // product into the subtraction, the inputs call rounds both products)
            const float p1 = cdx * is, cdd = cd * dxd, is3 = is * is * is;
            float qd;
            if (PLANES) {
              qd = fmaf(-cdd, is3, p1);
            } else {
#pragma clang fp contract(off)
              qd = p1 - cdd * is3;
            }
            src = lane < ng ? w1 * qd : 0.f;
            if (!PLANES) {
              if (lane < ng) Gs[k * ng + lane] = src;
              float cp = 0.f;
              if (curv) {
                // row `lane` of Phi_t over (x, u): Phi_xx dX_t + Phi_xu H_t
                const float* ph = PHs + k * fp + lc * nm;
                for (int i = 0; i < n; ++i) cp = fmaf(ph[i], DXs[k * n + i], cp);
                for (int i = 0; i < m; ++i) cp = fmaf(ph[n + i], Hs[k * m + i], cp);
              }
              src = src + cp;   // (added without Phi too: it turns a -0 into +0, and the results are pinned bitwise)
            }
          } else {
            src = lane < ng ? w1 * cd * is : 0.f;
          }
        }
        const float v = atv(ABs + k * fa, v_adj);
        v_adj = lane < n ? src + v : 0.f;
      }
    }
    __syncthreads();
    if (PLANES) {
      for (int e = tid; e < kc * n; e += GMPC_TA_THREADS) {
        const int k = e / n, i = e - k * n;
        a.w[(urow + t0) * n + e] = Vs[k * 64 + i] - Vs[(K + k) * 64 + i];
        a.lam[(urow + t0) * n + e] = Vs[(2 * K + k) * 64 + i];
      }
    } else if (a.ggoal != nullptr) {
      for (int e = tid; e < kc * ng; e += GMPC_TA_THREADS) a.ggoal[(xrow + t0) * ng + e] = Gs[e];
    }
    __syncthreads();
  }
  if (!PLANES) {
    if (wave < 2 && lane < n) Vs[wave * 64 + lane] = v_adj;
    __syncthreads();
    if (tid < n) a.gx0[(size_t)b * n + tid] = Vs[tid] - Vs[64 + tid];
  }
}

// The goal gradient alone: rows (trajectory, step) are independent, one wave each, four per workgroup.  Any n (the
// step-major pipeline included: it needs X, goal and dX only).
__global__ __launch_bounds__(GMPC_TA_THREADS) void k_goal_grad(int rows, int T, int n, int ng, const float* mpc_w,
                                                               const float* X, const float* goal, const float* dX,
                                                               float* ggoal) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (GMPC_TA_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int t = row % (T + 1);
  if (t == T) {
    for (int i = lane; i < ng; i += 64) ggoal[(size_t)row * ng + i] = 0.f;
    return;
  }
  const float al = GMPC_ALPHA;
  const float w1 = sigmoidf_(mpc_w[1]);
  float dd = 0.f, dxd = 0.f;
  for (int i = lane; i < ng; i += 64) {
    const float d = X[(size_t)row * n + i] - goal[(size_t)row * ng + i];
    dd = fmaf(d, d, dd);
    dxd = fmaf(d, dX[(size_t)row * n + i], dxd);
  }
  dd = wave_sum(dd);
  dxd = wave_sum(dxd);
  const float s = sqrtf(dd + al * al);
  const float is = 1.f / s, is3 = is * is * is;
  for (int i = lane; i < ng; i += 64) {
    const float d = X[(size_t)row * n + i] - goal[(size_t)row * ng + i];
    ggoal[(size_t)row * ng + i] = w1 * (dX[(size_t)row * n + i] * is - d * dxd * is3);
  }
}

// Host-side launchers ---------------------------------------------------------------------------
int gmpc_launch_tail_adjoints(const TailAdjArgs& a, bool planes, hipStream_t s) {
  if (a.n > 64 || a.m > 32) return 1;
  const int nm = a.n + a.m;
  const int F = a.n * nm + 3 * a.n + a.ng + (planes ? 0 : (a.Phi != nullptr ? nm * nm : 0) + a.m);
  int K = (planes ? GMPC_TA_FLOATS_PLANES : GMPC_TA_FLOATS_INPUTS) / F;
  if (K > GMPC_TA_CHUNK) K = GMPC_TA_CHUNK;
  if (K > a.T) K = a.T;
  if (K < 1) return 1;   // (Phi of the largest shapes: one step does not fit)
  const size_t lds = ((size_t)K * F + (planes ? 3 * (size_t)K * 64 : 128)) * sizeof(float);
  auto kern = planes ? (a.n <= 32 ? k_tail_adjoints<32, true> : k_tail_adjoints<64, true>)
                     : (a.n <= 32 ? k_tail_adjoints<32, false> : k_tail_adjoints<64, false>);
  hipLaunchKernelGGL(kern, dim3(a.B), dim3(GMPC_TA_THREADS), lds, s, a, K);
  return 0;
}

void gmpc_launch_goal_grad(int B, int T, int n, int ng, const float* mpc_w, const float* X, const float* goal,
                           const float* dX, float* ggoal, hipStream_t s) {
  const int rows = B * (T + 1), per = GMPC_TA_THREADS / 64;
  hipLaunchKernelGGL(k_goal_grad, dim3((rows + per - 1) / per), dim3(GMPC_TA_THREADS), 0, s, rows, T, n, ng, mpc_w,
                     X, goal, dX, ggoal);
}
