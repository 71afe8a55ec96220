// The iLQR Riccati sweep with its products on the matrix pipe, for the reference's state / action sizes: k_riccati_w2,
// one kernel body in two modes -- HESS = false is mode 0 of k_riccati (gmpc_backward.hip), the backward sweep of an
// iLQR step; HESS = true is mode 1, the bilevel Hessian solve with the loss adjoint and the tangent roll folded in.
// Same recursion as k_riccati (trajax lqr_step / tvlqr with delta = 1e-8, adjoint); the association of the
// products differs (A^T (P A) instead of (A^T P) A, the K terms through V), the results agree to rounding.
// Reference arithmetic: trajax tvlqr as called from policy/optimizers.py:19,41; cost/cost_model.py:20-31.
#include "gmpc_launch.h"
#include "gmpc_riccati_parts.h"
#include <cstdlib>
#include <cstring>

typedef float f32x16_w __attribute__((ext_vector_type(16)));

// Inside one wave the LDS instructions execute in program order, so a value written by one lane is there for
// the lane of the same wave that reads it later -- what is needed between two phases of a wave's work is only that
// hipcc keeps them in order.  __syncthreads() also drains the vector-memory counter (the next step's prefetch, the
// K / k / gradient stores of this one: a round trip to the Infinity Cache or HBM at every phase boundary).
#ifdef GMPC_RICCATI_W_BARRIERS
#define RW_SYNC() __syncthreads()
#else
// wave_barrier alone is a scheduling barrier the optimiser models as touching no memory: the wavefront-scope fences
// around it are what tells the compiler that LDS stores before it are visible to the loads after it (they emit no
// instruction at this scope -- in particular no s_waitcnt vmcnt --, the hardware keeps one wave's LDS accesses in order)
#define RW_SYNC()                                             \
  do {                                                        \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
    __builtin_amdgcn_wave_barrier();                          \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
  } while (0)
#endif

// ------------------------------------------------------------------------------------------------
// Two waves per trajectory (k_riccati_w2).  The three matrix products of a step run on the matrix pipe instead of
// 15 k multiply-adds with two LDS operands each:
//     W = P [A | B]                          (n x (n+m); P symmetric, so P is the "TN" left operand)
//     Z = [A | B]^T W = [[A^T P A, A^T P B], [B^T P A, B^T P B]]      -> T1, H, G_r in one tile
//     Z[:n, :n] += [K; V]^T [V; K]           (V = H + G K / 2: K^T V + V^T K = K^T H + H^T K + K^T G K)
// as v_mfma_f32_32x32x2_f32 with the operands zero-padded to 32 columns and an even row count in LDS (9 + 9 +
// M MFMAs per step); every operand row is a k-step, so nothing is transposed.  The 32 x 32 accumulator tile
// of a lane holds column (lane & 31) and rows (rg & 3) + 8 (rg >> 2) + 4 (lane >> 5).  What stays on the
// vector pipe: the two vector recursions (lambda, p), the M x M factorisation (lane 0, in registers, as in
// k_riccati) and the substitutions (one right-hand-side column per lane).
// The sweep is one dependent chain per step --
//   W = P [A|B] -> Z = [A|B]^T W -> G -> factorisation -> [K k] -> S = Z_xx + [K;V]^T [V;K] -> P
// -- and a single wave would also run everything else of the step in that chain's program order: the stage-cost
// scalars (a 17-term sum, two square roots, the reciprocals), q_t, r_t, the adjoint recursion lambda_t = q_t +
// A_t^T lambda_{t+1} with the control gradient, A_t^T p and h = r_t + B_t^T p, the next step's operands coming in
// from global memory (stamps of the one-wave form: 3.0 k + 1.0 k of the 13.9 k cycles of a step).  None of that
// needs this step's P.  Wave 1 (the helper) does it one step AHEAD into double-buffered LDS; wave 0 (the chain) finds
// [A|B]_t, x - g, u, the scalars and q_t ready at the top of step t and h, A^T p before its solve.  Two workgroup
// barriers per step (LDS counter only: the helper's prefetch and the chain's K stores stay in flight across them).
//
// HESS = false, the iLQR step: G + delta I (delta = 1e-8) is factored by Cholesky; the helper's linear terms are q_t,
// r_t, its recursion the adjoint lambda with the control gradient (a.grad, a.adj, a.K, a.k are optional outputs);
// trajectories with a.active[b] == 0 leave at once; after the sweep the helper evaluates the continuation test.
//
// HESS = true, the bilevel Hessian solve (a.active must be null, a.K / a.k are the caller's scratch).  Same sweep with
//   * no regulariser (delta = 0) and G possibly indefinite (make_psd = False): the m x m systems are solved by
//     Gaussian elimination with partial pivoting, as k_riccati<N, M> does in mode 1 -- the factorisation on lane 0 in
//     registers, then one right-hand-side column per lane with the recorded pivots and multipliers (the same
//     operations in the same order as the serial elimination of k_riccati, which spent 0.9 ms of a 1.4 ms
//     gmpc_bilevel_grad on one lane walking m (n + 1) columns through LDS);
//   * linear terms q~ = 0, r~_t = -Bvec_t with Bvec_t = B_t^T mu_{t+1}, mu_T = lx_T, mu_t = lx_t + A_t^T mu_{t+1}
//     (policy/optimizers.py:78-83: the gradient of the upper loss with respect to the controls).  The helper wave
//     runs that adjoint recursion in the same backward sweep -- it is the recursion it runs for lambda in the iLQR
//     step with lx_t in the place of q_t -- and writes Bvec out: k_bvec (a launch of its own, 0.14 ms) is folded in.
//     q~ is absent from p, not a zero term (adding 0 would turn a -0 into +0).
//     LU: a loss that depends on the controls adds its cotangent, Bvec_t = lu_t + B_t^T mu_{t+1}
//     (gmpc_bilevel_grad_cotangent); lu_t is prefetched one step ahead with lx_t.  Without LU the term is absent,
//     not zero (adding 0 would turn a -0 of B^T mu into +0);
//   * after the sweep (one more workgroup barrier, F), the forward tangent roll dU_t = k_t + K_t dX_t, dX_{t+1} =
//     A_t dX_t + B_t dU_t on wave 0, the next step's operands requested one step ahead;
//   * BOX (a held box solve): a.clamped holds one word per step, bit j = control j sits on a bound.  The
//     system is solved on the step's free rows and the clamped rows of K_t, k_t are 0: row and column j of G become the
//     unit vector where G is symmetrised into LDS and row j of every right-hand-side column is zeroed where it is
//     loaded, then the same elimination runs (an empty word changes nothing).  The helper fetches the word with the
//     step's other operands.  Nothing else changes: S and p are already in the general-gain form.
// Reference: policy/optimizers.py:61-71, 86-105 (dense hessian + solve), restated as the structured solve of
// oracle/gan_mpc_oracle.py:hessian_solve.
// ------------------------------------------------------------------------------------------------
#define RW2_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// lx, lu, bvec_out: HESS only (lu: LU only)
template <int N_, int M_, bool HESS, bool LU = false, bool BOX = false>
__global__ __launch_bounds__(128) void k_riccati_w2(RiccatiArgs a, const float* lx, const float* lu, float* bvec_out) {
  static_assert(HESS || (!LU && !BOX), "the loss cotangent and the clamped words belong to the Hessian solve");
  constexpr int n = N_, m = M_, nm = n + m, LD = 32;
  constexpr int NR = (n + 1) & ~1;
  constexpr int KP = NR / 2;
  static_assert(nm <= 32 && m <= 8 && n >= m, "one 32 x 32 tile");
  __shared__ float Xs[2][NR * LD];                       // [A | B] of step t in buffer t & 1 (helper -> chain)
  __shared__ float Ps[NR * LD], Ws[NR * LD], Ss[n * LD];
  __shared__ float KVs[2 * m * LD], VKs[2 * m * LD], Hm[m * LD], HGK[m * LD], Kk[m * LD];
  __shared__ float Gr[m * m], Gp[m * m], G[m * m], Lc[m * m];
  __shared__ float dvb[2][LD], uvb[2][8], rvb[2][8], scal[2][4];   // helper -> chain, buffer t & 1
  // (a mode's LDS holds the arrays it names: qvb the iLQR step only, pivs the Hessian solve only, mskb BOX only)
  __shared__ float qvb[2][LD];                                     // q_t, buffer t & 1
  __shared__ int pivs[8];
  __shared__ uint32_t mskb[2];                                     // the step's clamped word, buffer t & 1
  __shared__ float pv[LD], lam[LD], Ap[LD], hv[8];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int b = blockIdx.x, T = a.T;
  if constexpr (!HESS)
    if (a.active != nullptr && a.active[b] == 0) return;
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]);
  const int ng = a.ng > 0 ? a.ng : n;

  for (int e = tid; e < 2 * NR * LD; e += 128) (&Xs[0][0])[e] = 0.f;
  for (int e = tid; e < NR * LD; e += 128) { Ps[e] = 0.f; Ws[e] = 0.f; }
  for (int e = tid; e < 2 * m * LD; e += 128) { KVs[e] = 0.f; VKs[e] = 0.f; }
  RW2_BARRIER();

  if (wave == 1) {
    // ================= helper =================
    constexpr int PFN = (n * nm + 63) / 64;
    float pf_ab[PFN];
    float pf_d = 0.f, pf_u = 0.f, pf_lx = 0.f, pf_lu = 0.f;
    uint32_t pf_msk = 0u;
    float gn2 = 0.f;
    auto prefetch = [&](int tp) {
      const size_t btp = (size_t)b * T + tp;
#pragma unroll
      for (int r = 0; r < PFN; ++r) {
        const int e = lane + r * 64;
        pf_ab[r] = e < n * nm ? a.AB[btp * n * nm + e] : 0.f;
      }
      if (lane < n) {
        pf_d = lane < ng ? a.X[((size_t)b * (T + 1) + tp) * n + lane] - a.goal[((size_t)b * (T + 1) + tp) * ng + lane]
                         : 0.f;
        if constexpr (HESS) pf_lx = lx[((size_t)b * (T + 1) + tp) * n + lane];
      }
      if (lane < m) pf_u = a.U[btp * m + lane];
      if (LU && lane >= n && lane < nm) pf_lu = lu[btp * m + lane - n];
      if (BOX && lane == 0) pf_msk = a.clamped[btp];
    };
    // everything of step tp that needs neither P nor p: operands into buffer tp & 1, scalars, and the linear terms
    // with their adjoint recursion -- q, r and lambda, or the loss adjoint mu and Bvec
    auto prepare = [&](int tp) {
      const int bf = tp & 1;
      float* X_ = Xs[bf];
#pragma unroll
      for (int r = 0; r < PFN; ++r) {
        const int e = lane + r * 64;
        if (e < n * nm) X_[(e / nm) * LD + e % nm] = pf_ab[r];
      }
      if (lane < n) dvb[bf][lane] = pf_d;
      if (lane < m) uvb[bf][lane] = pf_u;
      if (BOX && lane == 0) mskb[bf] = pf_msk;
      const float lxt = pf_lx, lut = pf_lu;
      RW_SYNC();
      if (tp > 0) prefetch(tp - 1);
      const float* dv = dvb[bf];
      const float* uv = uvb[bf];
      float dd = 0.f, uu = 0.f;
#pragma unroll
      for (int i = 0; i < n; ++i) dd = fmaf(dv[i], dv[i], dd);
#pragma unroll
      for (int j = 0; j < m; ++j) uu = fmaf(uv[j], uv[j], uu);
      const auto [is, is3, isu, isu3] = gmpc_ric_stage(dd, uu);
      if (lane == 0) { scal[bf][0] = is; scal[bf][1] = is3; scal[bf][2] = isu; scal[bf][3] = isu3; }
      const size_t bt = (size_t)b * T + tp;
      float ln = 0.f;
      if (lane < nm) {
        float vl = 0.f;
#pragma unroll
        for (int k = 0; k < n; ++k) vl = fmaf(X_[k * LD + lane], lam[k], vl);
        if constexpr (HESS) {
          if (lane < n) {
            ln = lxt + vl;                             // mu_t = lx_t + A^T mu
          } else {
            const int j = lane - n;
            const float bv = LU ? vl + lut : vl;
            bvec_out[bt * m + j] = bv;                 // Bvec_t = B^T mu (+ lu_t)
            rvb[bf][j] = -bv;                          // the Riccati sweep's linear term r~_t
          }
        } else {
          if (lane < n) {
            const float q = w1 * dv[lane] * is;
            qvb[bf][lane] = q;
            ln = q + vl;                               // lam_t = q_t + A^T lam
          } else {
            const int j = lane - n;
            const float r = w0 * uv[j] * isu;
            rvb[bf][j] = r;
            const float g = r + vl;                    // g_t = r_t + B^T lam
            gn2 = fmaf(g, g, gn2);
            if (a.grad) a.grad[bt * m + j] = g;
          }
        }
      }
      RW_SYNC();                                     // (every lane has read lam)
      if (lane < n) {
        lam[lane] = ln;
        if constexpr (!HESS)
          if (a.adj) a.adj[((size_t)b * (T + 1) + tp) * n + lane] = ln;
      }
      RW_SYNC();
    };
    if (lane < n) {
      if constexpr (HESS) {
        pv[lane] = 0.f;
        lam[lane] = lx[((size_t)b * (T + 1) + T) * n + lane];
      } else {
        const float q = a.qT[(size_t)b * n + lane];
        pv[lane] = q;
        lam[lane] = q;
        if (a.adj) a.adj[((size_t)b * (T + 1) + T) * n + lane] = q;
      }
    }
    RW_SYNC();
    prefetch(T - 1);
    prepare(T - 1);
    for (int t = T - 1; t >= 0; --t) {
      RW2_BARRIER();                                 // S_t: p_{t+1} is in pv
      const int bf = t & 1;
      if (lane < nm) {
        float vp = 0.f;
#pragma unroll
        for (int k = 0; k < n; ++k) vp = fmaf(Xs[bf][k * LD + lane], pv[k], vp);
        if (lane < n) Ap[lane] = vp;                 // A^T p
        else hv[lane - n] = rvb[bf][lane - n] + vp;  // h = r_t + B^T p  (HESS: r~_t = -Bvec_t)
      }
      RW2_BARRIER();                                 // V_t: h, A^T p are there for the chain's solve
      if (t > 0) prepare(t - 1);
    }
    if constexpr (HESS) {
      RW2_BARRIER();                                 // F: the sweep is over (the chain rolls the tangent forward)
    } else {
      if (a.cont != nullptr) {
        float un2 = 0.f;
        for (int e = lane; e < T * m; e += 64) {
          const float u = a.U[(size_t)b * T * m + e];
          un2 = fmaf(u, u, un2);
        }
        gn2 = wave_sum(gn2);
        un2 = wave_sum(un2);
        if (lane == 0) {
          const bool go = gmpc_ric_continue(gn2, un2, b, a.obj, a.obj_step, a.U_step, a.iters, a.alpha, a.opts);
          a.cont[b] = go ? 1 : 0;
        }
      }
    }
    return;
  }

  // ================= the chain =================
  for (int e = lane; e < n * n; e += 64) Ps[(e / n) * LD + e % n] = a.QT[(size_t)b * n * n + e];
  for (int t = T - 1; t >= 0; --t) {
    const size_t bt = (size_t)b * T + t;
    const int bf = t & 1;
    RW2_BARRIER();                                   // S_t: [A | B]_t, x - g, u, scalars, q_t are in buffer bf
    const uint32_t cw = BOX ? mskb[bf] : 0u;         // the step's clamped controls
    const float* X_ = Xs[bf];
    const float* dv = dvb[bf];
    const float* uv = uvb[bf];
    const float is = scal[bf][0], is3 = scal[bf][1], isu = scal[bf][2], isu3 = scal[bf][3];
    // ---- W = P [A | B]
    f32x16_w acc;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) acc[rg] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ps[(2 * kk + half) * LD + l31], X_[(2 * kk + half) * LD + l31], acc,
                                                 0, 0, 0);
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int row = (rg & 3) + 8 * (rg >> 2) + 4 * half;
      if (row < NR) Ws[row * LD + l31] = acc[rg];
    }
    RW_SYNC();
    // ---- Z = [A | B]^T W
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) acc[rg] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(X_[(2 * kk + half) * LD + l31], Ws[(2 * kk + half) * LD + l31], acc,
                                                 0, 0, 0);
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int row = (rg & 3) + 8 * (rg >> 2) + 4 * half;
      if (row >= n && row < nm) {
        if (l31 < n) Hm[(row - n) * LD + l31] = acc[rg];
        else if (l31 < nm) Gr[(row - n) * m + l31 - n] = acc[rg];
      }
    }
    RW_SYNC();
    // ---- G = sym(R + G_r); its factorisation on lane 0, in registers.  (Both factorisations and their column solves
    // are written out here, not called: as routines taking the LDS arrays they compile to another schedule -- the
    // same bits, but the Hessian form at 114 + 16 registers, 3 waves per SIMD for 4, and the iLQR form 1 % slower.)
    if (lane < m * m) {
      const int i = lane / m, j = lane - i * m;
      const float Rij = w0 * ((i == j ? isu : 0.f) - uv[i] * uv[j] * isu3);
      Gp[lane] = Rij + Gr[lane];
    }
    RW_SYNC();
    if (lane < m * m) {
      const int i = lane / m, j = lane - i * m;
      float g = (Gp[lane] + Gp[j * m + i]) * 0.5f;
      if (BOX && (((cw >> i) | (cw >> j)) & 1u)) g = i == j ? 1.f : 0.f;
      G[lane] = g;
    }
    RW_SYNC();
    if (lane == 0) {
      if constexpr (HESS) {                          // LU with partial pivoting (jax.scipy.linalg.solve)
        float Lr[m][m];
#pragma unroll
        for (int i = 0; i < m; ++i)
#pragma unroll
          for (int j = 0; j < m; ++j) Lr[i][j] = G[i * m + j];
#pragma unroll
        for (int j = 0; j < m; ++j) {
          int piv = j;
          float best = fabsf(Lr[j][j]);
#pragma unroll
          for (int i = j + 1; i < m; ++i) {
            const float v = fabsf(Lr[i][j]);
            if (v > best) { best = v; piv = i; }
          }
          pivs[j] = piv;
#pragma unroll
          for (int i = j + 1; i < m; ++i) {
            if (piv == i) {
              // (columns >= j only: the multipliers already stored in columns < j belong to the row POSITIONS, because
              // the right-hand-side columns below apply swap j and elimination j in turn, like the serial elimination)
#pragma unroll
              for (int c = j; c < m; ++c) { const float t_ = Lr[j][c]; Lr[j][c] = Lr[i][c]; Lr[i][c] = t_; }
            }
          }
          const float d = Lr[j][j];
#pragma unroll
          for (int i = j + 1; i < m; ++i) {
            const float f = Lr[i][j] / d;
#pragma unroll
            for (int c = j; c < m; ++c) Lr[i][c] -= f * Lr[j][c];
            Lr[i][j] = f;                              // the multiplier, for the right-hand-side columns
          }
        }
#pragma unroll
        for (int i = 0; i < m; ++i)
#pragma unroll
          for (int j = 0; j < m; ++j) Lc[i * m + j] = Lr[i][j];
      } else {                                       // Cholesky of G + delta I, the diagonal kept as its reciprocal
        float Lr[m][m];
#pragma unroll
        for (int j = 0; j < m; ++j) {
          float sdiag = G[j * m + j] + 1e-8f;
#pragma unroll
          for (int k = 0; k < j; ++k) sdiag -= Lr[j][k] * Lr[j][k];
          const float di = 1.0f / sqrtf(sdiag);
          Lr[j][j] = di;
#pragma unroll
          for (int i = j + 1; i < m; ++i) {
            float v = G[i * m + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= Lr[i][k] * Lr[j][k];
            Lr[i][j] = v * di;
          }
        }
#pragma unroll
        for (int i = 0; i < m; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) Lc[i * m + j] = Lr[i][j];
      }
    }
    RW2_BARRIER();                                   // V_t: h and A^T p have arrived
    // ---- [K k] = -(G + delta I)^-1 [H h]: one column per lane
    if (lane <= n) {
      const int c = lane;
      if constexpr (HESS) {                          // row swaps, elimination with the multipliers, back substitution
        float Lr[m][m], y[m];
#pragma unroll
        for (int i = 0; i < m; ++i)
#pragma unroll
          for (int j = 0; j < m; ++j) Lr[i][j] = Lc[i * m + j];
#pragma unroll
        for (int i = 0; i < m; ++i) {
          y[i] = c < n ? Hm[i * LD + c] : hv[i];
          if (BOX && ((cw >> i) & 1u)) y[i] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < m; ++j) {
          const int piv = pivs[j];
#pragma unroll
          for (int i = j + 1; i < m; ++i)
            if (piv == i) { const float t_ = y[j]; y[j] = y[i]; y[i] = t_; }
#pragma unroll
          for (int i = j + 1; i < m; ++i) y[i] -= Lr[i][j] * y[j];
        }
#pragma unroll
        for (int i = m - 1; i >= 0; --i) {
          float v = y[i];
#pragma unroll
          for (int k = i + 1; k < m; ++k) v -= Lr[i][k] * y[k];
          y[i] = v / Lr[i][i];
        }
#pragma unroll
        for (int i = 0; i < m; ++i) Kk[i * LD + c] = -y[i];
      } else {
        float Lr[m][m], y[m];
#pragma unroll
        for (int i = 0; i < m; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) Lr[i][j] = Lc[i * m + j];
#pragma unroll
        for (int i = 0; i < m; ++i) {
          float v = c < n ? Hm[i * LD + c] : hv[i];
#pragma unroll
          for (int k = 0; k < i; ++k) v -= Lr[i][k] * y[k];
          y[i] = v * Lr[i][i];
        }
#pragma unroll
        for (int i = m - 1; i >= 0; --i) {
          float v = y[i];
#pragma unroll
          for (int k = i + 1; k < m; ++k) v -= Lr[k][i] * y[k];
          y[i] = v * Lr[i][i];
        }
#pragma unroll
        for (int i = 0; i < m; ++i) Kk[i * LD + c] = -y[i];
      }
    }
    RW_SYNC();
    // ---- outputs K_t, k_t; H + G K; the stacked operands [K; V], [V; K]
    for (int e = lane; e < m * n; e += 64) {
      const int i = e / n, j = e - i * n;
      const float kij = Kk[i * LD + j];
      if (HESS || a.K) a.K[bt * m * n + e] = kij;
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < m; ++k) v = fmaf(G[i * m + k], Kk[k * LD + j], v);
      const float h = Hm[i * LD + j];
      HGK[i * LD + j] = h + v;
      const float vv = fmaf(0.5f, v, h);
      KVs[i * LD + j] = kij; KVs[(m + i) * LD + j] = vv;
      VKs[i * LD + j] = vv;  VKs[(m + i) * LD + j] = kij;
    }
    if ((HESS || a.k) && lane < m) a.k[bt * m + lane] = Kk[lane * LD + n];
    RW_SYNC();
    // ---- S = A^T P A + K^T V + V^T K, P = Q_t + sym(S)
#pragma unroll
    for (int kk = 0; kk < m; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(KVs[(2 * kk + half) * LD + l31], VKs[(2 * kk + half) * LD + l31], acc,
                                                 0, 0, 0);
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int row = (rg & 3) + 8 * (rg >> 2) + 4 * half;
      if (row < n) Ss[row * LD + l31] = acc[rg];
    }
    // p = q + A^T p + (H + G K)^T k + K^T h   (HESS: q~ = 0, absent)
    float pn = 0.f;
    if (lane < n) {
      float v1 = 0.f, v2 = 0.f;
#pragma unroll
      for (int k = 0; k < m; ++k) {
        v1 = fmaf(HGK[k * LD + lane], Kk[k * LD + n], v1);
        v2 = fmaf(Kk[k * LD + lane], hv[k], v2);
      }
      if constexpr (HESS) pn = (Ap[lane] + v1) + v2;
      else pn = ((qvb[bf][lane] + Ap[lane]) + v1) + v2;
    }
    RW_SYNC();
    for (int e = lane; e < n * n; e += 64) {
      const int i = e / n, j = e - i * n;
      const float Qij = w1 * ((i == j && i < ng ? is : 0.f) - dv[i] * dv[j] * is3);
      Ps[i * LD + j] = Qij + (Ss[i * LD + j] + Ss[j * LD + i]) * 0.5f;
    }
    if (lane < n) pv[lane] = pn;
    RW_SYNC();
  }
  if constexpr (HESS) {
    RW2_BARRIER();                                     // F: (the helper has left the LDS buffers alone since V_0)
    // ================= forward tangent roll (this wave; the gains of step t come back from global memory -- this
    // wave's own stores, drained first) =================
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    constexpr int PFA = (n * nm + 63) / 64, PFK = (m * n + 63) / 64;
    float fa[PFA], fk[PFK], fk0 = 0.f;
    auto fetch = [&](int tp) {
      const size_t btp = (size_t)b * T + tp;
#pragma unroll
      for (int r = 0; r < PFA; ++r) {
        const int e = lane + r * 64;
        fa[r] = e < n * nm ? a.AB[btp * n * nm + e] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < PFK; ++r) {
        const int e = lane + r * 64;
        fk[r] = e < m * n ? a.K[btp * m * n + e] : 0.f;
      }
      if (lane < m) fk0 = a.k[btp * m + lane];
    };
    float* const Xr = Xs[0];                           // [A | B]_t rows; the gains K_t in Ws; dX in pv, dU in hv
    if (lane < n) { pv[lane] = 0.f; a.dX[(size_t)b * (T + 1) * n + lane] = 0.f; }
    fetch(0);
    for (int t = 0; t < T; ++t) {
      const size_t bt = (size_t)b * T + t;
#pragma unroll
      for (int r = 0; r < PFA; ++r) {
        const int e = lane + r * 64;
        if (e < n * nm) Xr[(e / nm) * LD + e % nm] = fa[r];
      }
#pragma unroll
      for (int r = 0; r < PFK; ++r) {
        const int e = lane + r * 64;
        if (e < m * n) Ws[(e / n) * LD + e % n] = fk[r];
      }
      const float k0 = fk0;
      RW_SYNC();
      if (t + 1 < T) fetch(t + 1);
      if (lane < m) {
        float v = k0;
#pragma unroll
        for (int i = 0; i < n; ++i) v = fmaf(Ws[lane * LD + i], pv[i], v);
        hv[lane] = v;
        a.Hout[bt * m + lane] = v;
      }
      RW_SYNC();
      float xn = 0.f;
      if (lane < n) {
#pragma unroll
        for (int k = 0; k < n; ++k) xn = fmaf(Xr[lane * LD + k], pv[k], xn);
#pragma unroll
        for (int k = 0; k < m; ++k) xn = fmaf(Xr[lane * LD + n + k], hv[k], xn);
      }
      RW_SYNC();
      if (lane < n) {
        pv[lane] = xn;
        a.dX[((size_t)b * (T + 1) + t + 1) * n + lane] = xn;
      }
      RW_SYNC();
    }
  }
}

// the shapes the two-wave sweep is instantiated for: MLP dynamics (no curvature term) at the reference's sizes;
// GMPC_RICCATI=valu keeps k_riccati
static bool riccati_w_shape(const RiccatiArgs& a, int mode) {
  const char* e = getenv("GMPC_RICCATI");
  if (e != nullptr && strcmp(e, "valu") == 0) return false;
  return a.mode == mode && a.Phi == nullptr && a.n == 17 && a.m == 6;
}
bool gmpc_riccati_w_shape(const RiccatiArgs& a) { return riccati_w_shape(a, 0); }
// the Hessian solve (mode 1) with the loss adjoint folded in
bool gmpc_riccati_w2h_shape(const RiccatiArgs& a) {
  return riccati_w_shape(a, 1) && a.active == nullptr && (a.ng == 0 || a.ng == a.n);
}
// mode 0: lx, lu, bvec_out null.  mode 1: lu optional; a.clamped (a held box solve) selects the masked solve
void gmpc_launch_riccati_w(const RiccatiArgs& a, const float* lx, const float* lu, float* bvec_out, hipStream_t s) {
#define RW2_LAUNCH(...) \
  hipLaunchKernelGGL((k_riccati_w2<17, 6, __VA_ARGS__>), dim3(a.B), dim3(128), 0, s, a, lx, lu, bvec_out)
  if (a.mode == 0) RW2_LAUNCH(false);
  else if (a.clamped != nullptr && lu != nullptr) RW2_LAUNCH(true, true, true);
  else if (a.clamped != nullptr) RW2_LAUNCH(true, false, true);
  else if (lu != nullptr) RW2_LAUNCH(true, true);
  else RW2_LAUNCH(true, false);
#undef RW2_LAUNCH
}
