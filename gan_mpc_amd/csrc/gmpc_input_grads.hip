// Gradients of an upper-level loss L(X*, U*) with respect to the solver's inputs x0 and goal
// (gmpc_bilevel_grad_inputs), from the state a preceding gmpc_bilevel_grad(_cotangent) leaves in the ctx:
// H = A^{-1} Bvec (A = d^2 J / dU^2), dX its tangent roll (dX_0 = 0), [A_t | B_t], the terminal Hessian QT and, for
// the LSTM dynamics, the curvature Phi_t = lam_{t+1} . d^2 f_t that the Hessian solve used.
//
//   dL/dp = dL/dp|_(U fixed) - d/dp [ H . grad_U J ]   (H held fixed),   H . grad_U J = sum_t q_t . dX_t + r_t . H_t
//
//   goal:  dL/dg_t = (Q_t dX_t)[:ng] = w1 (dX_t / s - d (d . dX_t) / s^3)[:ng],  d = x_t[:ng] - g_t,
//          s = sqrt(|d|^2 + alpha^2), t < T; the terminal cost does not read g_T: 0.
//   x0:    mu_T = lx_T,  mu_t = lx_t + A_t^T mu_{t+1}                               (mu_0 = dL/dx0 with U fixed)
//          nu_T = QT dX_T, nu_t = Q_t dX_t + Phi_x(x,u),t [dX_t; H_t] + A_t^T nu_{t+1}   (nu_0 = d/dx0 [H . grad_U J])
//          dL/dx0 = mu_0 - nu_0.
// Q_t is formed from x_t and g_t in closed form (the stage Hessian k_riccati builds), never stored.
#include "gmpc_launch.h"

#define GMPC_IG_THREADS 256
#define GMPC_IG_CHUNK_FLOATS 15872   // LDS for the staged steps (62 KB; the adjoints add 1 KB)

// Layout of one chunk of K steps t0 .. t0 + kc - 1 (kc <= K), in global memory as in LDS: each field is one
// contiguous run per trajectory -- [A_t | B_t] (n x nm per step), Phi_t (nm x nm per step, LSTM dynamics only),
// lx_t, dX_t, x_t (n each), goal_t (ng), H_t (m).  In LDS every field has room for K steps.
struct IgChunk {
  int fa, fp, n, ng, m;     // per-step sizes of the fields
  int K;
  __device__ int per_step() const { return fa + fp + 3 * n + ng + m; }
  // LDS offset of field f (0 AB, 1 Phi, 2 lx, 3 dX, 4 X, 5 goal, 6 H)
  __device__ int base(int f) const {
    return K * ((f > 0 ? fa : 0) + (f > 1 ? fp : 0) + (f > 2 ? n : 0) + (f > 3 ? n : 0) + (f > 4 ? n : 0) +
                (f > 5 ? ng : 0));
  }
};

// The global address of staged element e of a chunk of kc steps starting at t0, and its LDS slot.
__device__ __forceinline__ const float* ig_src(const IgChunk& c, int e, int kc, int t0, int b, int T, int& slot,
                                               const float* AB, const float* Phi, const float* lx, const float* dX,
                                               const float* X, const float* goal, const float* H) {
  const size_t st = (size_t)b * T + t0, sx = (size_t)b * (T + 1) + t0;
  int lim = kc * c.fa;
  if (e < lim) { slot = e; return AB + st * c.fa + e; }
  e -= lim; lim = kc * c.fp;
  if (e < lim) { slot = c.K * c.fa + e; return Phi + st * c.fp + e; }
  e -= lim;
  int ob = c.K * (c.fa + c.fp);
  if (e < kc * c.n) { slot = ob + e; return lx + sx * c.n + e; }
  e -= kc * c.n; ob += c.K * c.n;
  if (e < kc * c.n) { slot = ob + e; return dX + sx * c.n + e; }
  e -= kc * c.n; ob += c.K * c.n;
  if (e < kc * c.n) { slot = ob + e; return X + sx * c.n + e; }
  e -= kc * c.n; ob += c.K * c.n;
  if (e < kc * c.ng) { slot = ob + e; return goal + sx * c.ng + e; }
  e -= kc * c.ng; ob += c.K * c.ng;
  slot = ob + e;
  return H + st * c.m + e;
}

// Broadcast lane i's value of v to the wave (i uniform, here a compile-time constant after unrolling).
__device__ __forceinline__ float ig_lane(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}

// The x0 sweep (n <= 64, m <= 32: [A_t | B_t] is materialised), one workgroup per trajectory.  Wave 0 runs mu,
// wave 1 nu and the goal gradient, lane c owning state c and holding mu_c / nu_c in a register (lanes >= n hold 0);
// A_t^T v is an unrolled NMAX-term sum of LDS reads of column c of A_t -- independent, issued back to back -- times
// v_i broadcast with v_readlane, so no LDS round trip orders one step after the other.  Waves 2 and 3 only load.
// The steps come in chunks of K: while the waves run chunk j out of LDS, the raw operands of chunk j + 1 -- PFN
// floats per thread -- are in flight into registers; they are written to LDS behind the one barrier pair per chunk.
// No arithmetic touches a loaded value before that barrier, so nothing waits on the loads early.
template <int PFN, int NMAX>
__global__ __launch_bounds__(GMPC_IG_THREADS) void k_input_grads(int T, int n, int ng, int m, int K,
                                                                 const float* mpc_w, const float* X,
                                                                 const float* goal, const float* dX, const float* H,
                                                                 const float* lx, const float* AB, const float* QT,
                                                                 const float* Phi, float* gx0, float* ggoal) {
  extern __shared__ __attribute__((aligned(16))) char smem_ig[];
  const int nm = n + m;
  IgChunk c;
  c.fa = n * nm; c.fp = Phi != nullptr ? nm * nm : 0; c.n = n; c.ng = ng; c.m = m; c.K = K;
  float* S = reinterpret_cast<float*>(smem_ig);
  const float* ABs = S;
  const float* PHs = S + c.base(1);
  const float* LXs = S + c.base(2);
  const float* DXs = S + c.base(3);
  const float* Xs = S + c.base(4);
  const float* Gs = S + c.base(5);
  const float* Hs = S + c.base(6);
  float* fin = S + K * c.per_step();   // [2][64]: dX_T / lx_T at the start, mu_0 / nu_0 at the end
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const int lc = lane < n ? lane : 0;   // idle lanes read a valid column and discard the result
  const float al = GMPC_ALPHA;
  const float w1 = sigmoidf_(mpc_w[1]);
  const size_t xrow = (size_t)b * (T + 1);

  // ---- terminal: mu_T = lx_T, nu_T = QT dX_T, grad_goal_T = 0
  // (dX_T and lx_T pass through LDS: an adjoint register that a global load wrote would make hipcc wait for the
  // vector-memory counter -- the next chunk's loads -- at the head of every step loop)
  if (tid < n) {
    fin[tid] = dX[(xrow + T) * n + tid];
    fin[64 + tid] = lx[(xrow + T) * n + tid];
  }
  __syncthreads();
  float v_adj = 0.f;        // wave 0: mu_c, wave 1: nu_c (lane c < n)
  if (wave == 0 && lane < n) v_adj = fin[64 + lane];
  if (wave == 1 && lane < n) {
    const float* q = QT + ((size_t)b * n + lane) * n;
    float v = 0.f;
    for (int k = 0; k < n; ++k) v = fmaf(q[k], fin[k], v);
    v_adj = v;
    if (ggoal != nullptr && lane < ng) ggoal[(xrow + T) * ng + lane] = 0.f;
  }

  float pf[PFN];
  auto issue = [&](int t0, int kc) {   // raw loads only: no use of the values before the next barrier
    const int tot = kc * c.per_step();
#pragma unroll
    for (int r = 0; r < PFN; ++r) {
      const int e = tid + r * GMPC_IG_THREADS;
      int slot;   // (unused here)
      pf[r] = e < tot ? *ig_src(c, e, kc, t0, b, T, slot, AB, Phi, lx, dX, X, goal, H) : 0.f;
    }
  };
  auto commit = [&](int t0, int kc) {
    const int tot = kc * c.per_step();
#pragma unroll
    for (int r = 0; r < PFN; ++r) {
      const int e = tid + r * GMPC_IG_THREADS;
      if (e < tot) {
        int slot;
        ig_src(c, e, kc, t0, b, T, slot, AB, Phi, lx, dX, X, goal, H);
        S[slot] = pf[r];
      }
    }
  };
  // A_t^T v for column lc: terms i >= n read row n - 1 and multiply the 0 that lane i holds
  auto atv = [&](const float* A, float v) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i) acc = fmaf(A[(i < n ? i : n - 1) * nm + lc], ig_lane(v, i), acc);
    return acc;
  };
  const int nchunks = (T + K - 1) / K;
  auto chunk_t0 = [&](int j) { const int t0 = T - (j + 1) * K; return t0 > 0 ? t0 : 0; };
  auto chunk_kc = [&](int j) { return T - j * K - chunk_t0(j); };
  issue(chunk_t0(0), chunk_kc(0));
  __syncthreads();
  commit(chunk_t0(0), chunk_kc(0));
  __syncthreads();

  for (int j = 0; j < nchunks; ++j) {
    const int kc = chunk_kc(j);
    if (j + 1 < nchunks) issue(chunk_t0(j + 1), chunk_kc(j + 1));
    const int t0 = chunk_t0(j);
    if (wave == 0) {
      for (int k = kc - 1; k >= 0; --k) {
        const float v = atv(ABs + k * c.fa, v_adj);
        v_adj = lane < n ? LXs[k * n + lane] + v : 0.f;
      }
    } else if (wave == 1) {
      for (int k = kc - 1; k >= 0; --k) {
        // |d|^2 and d . dX over the goal columns, then Q_t dX_t in closed form
        const float cd = lane < ng ? Xs[k * n + lane] - Gs[k * ng + lane] : 0.f;
        const float cdx = lane < n ? DXs[k * n + lane] : 0.f;
        const float dd = wave_sum(cd * cd), dxd = wave_sum(cd * cdx);
        const float s = sqrtf(dd + al * al);
        const float is = 1.f / s, is3 = is * is * is;
        const float qd = lane < ng ? w1 * (cdx * is - cd * dxd * is3) : 0.f;
        // (kept in LDS over x_t, which only this lane reads, and stored after the chunk: a store inside the step
        // loop makes hipcc drain the vector-memory counter -- the next chunk's loads -- before the loop)
        if (lane < ng) const_cast<float*>(Xs)[k * n + lane] = qd;
        const float v = atv(ABs + k * c.fa, v_adj);
        float cp = 0.f;
        if (Phi != nullptr) {
          // row `lane` of Phi_t over (x, u): Phi_xx dX_t + Phi_xu H_t
          const float* ph = PHs + k * c.fp + lc * nm;
          for (int i = 0; i < n; ++i) cp = fmaf(ph[i], DXs[k * n + i], cp);
          for (int i = 0; i < m; ++i) cp = fmaf(ph[n + i], Hs[k * m + i], cp);
        }
        v_adj = lane < n ? (qd + cp) + v : 0.f;
      }
      if (ggoal != nullptr && lane < ng)
        for (int k = 0; k < kc; ++k) ggoal[(xrow + t0 + k) * ng + lane] = Xs[k * n + lane];
    }
    __syncthreads();        // chunk j's operands are dead; chunk j + 1's loads have had its K steps to land
    if (j + 1 < nchunks) commit(chunk_t0(j + 1), chunk_kc(j + 1));
    __syncthreads();
  }
  if (wave < 2 && lane < n) fin[wave * 64 + lane] = v_adj;
  __syncthreads();
  if (tid < n) gx0[(size_t)b * n + tid] = fin[tid] - fin[64 + tid];
}

// The goal gradient alone: rows (trajectory, step) are independent, one wave each, four per workgroup.  Any n (the
// step-major pipeline included: it needs X, goal and dX only).
__global__ __launch_bounds__(GMPC_IG_THREADS) void k_goal_grad(int rows, int T, int n, int ng, const float* mpc_w,
                                                               const float* X, const float* goal, const float* dX,
                                                               float* ggoal) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (GMPC_IG_THREADS / 64) + (threadIdx.x >> 6);
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
// x0 (and, with ggoal, the goal) gradient: n <= 64, m <= 32 (the caller checks); 0 on success.  The chunk length K:
// up to 8 steps, as many as the register staging (PFN floats per thread) and the LDS budget hold.
int gmpc_launch_input_grads(int B, int T, int n, int ng, int m, const float* mpc_w, const float* X,
                            const float* goal, const float* dX, const float* H, const float* lx, const float* AB,
                            const float* QT, const float* Phi, float* gx0, float* ggoal, hipStream_t s) {
  if (n > 64 || m > 32) return 1;
  const int nm = n + m;
  const int F = n * nm + (Phi != nullptr ? nm * nm : 0) + 3 * n + ng + m;
  const int want = (T < 8 ? T : 8) * F;
  int pfn = 64;
  for (int p : {4, 8, 16, 32})
    if (p * GMPC_IG_THREADS >= want) { pfn = p; break; }
  int K = pfn * GMPC_IG_THREADS / F;
  if (K > GMPC_IG_CHUNK_FLOATS / F) K = GMPC_IG_CHUNK_FLOATS / F;
  if (K > T) K = T;
  if (K < 1) return 1;
  const size_t lds = ((size_t)K * F + 128) * sizeof(float);
#define GMPC_IG_LAUNCH(P)                                                                                   \
  do {                                                                                                      \
    if (n <= 32)                                                                                            \
      hipLaunchKernelGGL((k_input_grads<P, 32>), dim3(B), dim3(GMPC_IG_THREADS), lds, s, T, n, ng, m, K, mpc_w, \
                         X, goal, dX, H, lx, AB, QT, Phi, gx0, ggoal);                                          \
    else                                                                                                    \
      hipLaunchKernelGGL((k_input_grads<P, 64>), dim3(B), dim3(GMPC_IG_THREADS), lds, s, T, n, ng, m, K, mpc_w, \
                         X, goal, dX, H, lx, AB, QT, Phi, gx0, ggoal);                                          \
  } while (0)
  switch (pfn) {
    case 4: GMPC_IG_LAUNCH(4); break;
    case 8: GMPC_IG_LAUNCH(8); break;
    case 16: GMPC_IG_LAUNCH(16); break;
    case 32: GMPC_IG_LAUNCH(32); break;
    default: GMPC_IG_LAUNCH(64); break;
  }
#undef GMPC_IG_LAUNCH
  return 0;
}

void gmpc_launch_goal_grad(int B, int T, int n, int ng, const float* mpc_w, const float* X, const float* goal,
                           const float* dX, float* ggoal, hipStream_t s) {
  const int rows = B * (T + 1), per = GMPC_IG_THREADS / 64;
  hipLaunchKernelGGL(k_goal_grad, dim3((rows + per - 1) / per), dim3(GMPC_IG_THREADS), 0, s, rows, T, n, ng, mpc_w,
                     X, goal, dX, ggoal);
}
