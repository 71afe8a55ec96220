// One-launch iLQR solve (gmpc_ilqr_solve_fused): one workgroup of 256 threads owns one trajectory from the first
// rollout to the last iteration -- trajax ilqr_base / line_search_ddp as restated at oracle/gan_mpc_oracle.py:ilqr --
// with no host round trip and no communication between workgroups.  Every loop is bounded by maxiter and by the
// halving count k_max.
//
// Phases of an iteration, each reusing the same dynamic LDS:
//  * line search: GMPC_FZ_NC halvings at once are the rows of every forward pass (weights streamed from L2 by
//    dense_rows, one weight read serving all rows); the first row in halving order whose objective decreases is
//    accepted -- the result of trying them one after another.  Candidate trajectories go to a ctx scratch buffer.
//  * linearisation: the relu masks of all T steps (a forward pass with the steps as rows), then the rows of every
//    step's Jacobian as the rows of a reverse pass over the transposed weights (n rows per step instead of n + m
//    tangent columns), [A_t | B_t] written to the ctx's AB; the terminal quadratisation the same way on the cost MLP.
//  * Riccati sweep with the adjoint, the control gradient and the continuation test (the arithmetic of k_riccati's
//    general form, Cholesky of G + 1e-8 I on one lane).
//
// The control-limited form (gmpc_ilqr_solve_box, template parameter BOX) is the same kernel with box
// bounds lo <= u <= hi on the controls: the start and every candidate control are clamped, the gains of a step come
// from a box QP (projected Newton on one lane, fz_box_qp) and the continuation test sees the projected gradient.
// With no bound active every phase performs the arithmetic of the unconstrained form, operation for operation.
#include "gmpc_fused_solve.h"
#include "gmpc_riccati_parts.h"

#define FZ_THREADS GMPC_THREADS

static __host__ __device__ inline int fz_ric_floats(int n, int m) {
  const int nm = n + m;
  return n * nm + 3 * n * n + 3 * m * n + m * (n + 1) + 2 * m * m + 5 * n + 3 * m;
}
// QP workspace of the box form behind the Riccati carve-out: y, g, d, trial y (floats), free list, clamped flags, the
// free count and the iteration count (ints)
static __host__ __device__ inline int fz_box_floats(int m) { return 6 * m + 2; }
static __host__ __device__ inline int fz_ls_floats(int n, int m) {
  return 2 * FZ_THREADS * GMPC_FZ_NC + GMPC_FZ_NC * (n + m);
}
static __host__ __device__ inline int fz_lin_floats(int n, int T) {
  return 2 * FZ_THREADS * GMPC_FZ_JR + (T + 1) * GMPC_FZ_LHM * GMPC_MW + 32 + 32 * n;
}
// the largest of the phases' carve-outs
static __host__ __device__ inline int fz_phase_floats(int n, int m, int T, bool box) {
  int f = fz_ric_floats(n, m) + (box ? fz_box_floats(m) : 0);
  f = f > fz_ls_floats(n, m) ? f : fz_ls_floats(n, m);
  f = f > fz_lin_floats(n, T) ? f : fz_lin_floats(n, T);
  return f;
}

// sum of one value per thread, in thread order (deterministic); every thread gets the result
__device__ float fz_block_sum(float v, float* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < FZ_THREADS; ++i) s += red[i];
  __syncthreads();
  return s;
}

// clamp to [lo, hi] that keeps a NaN (fmaxf / fminf would return the bound)
__host__ __device__ __forceinline__ float fz_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ bool fz_bit(const uint32_t* mb, int slot, int l, int c) {
  return (mb[(slot * GMPC_FZ_LHM + l) * GMPC_MW + (c >> 5)] >> (c & 31)) & 1u;
}

// Forward pass of the relu MLP d for R = 4 R4 rows.  The input is in bufA as an LDS image [dims[0]][R] (float r of
// element k at k * R + r); returns the buffer holding the output [dims[L]][R].  mb != null: the relu bits of hidden
// layer l of row r (< nrows) go to mask slot slot0 + r.
template <int R4>
__device__ __forceinline__ float4* fz_forward(const MlpDesc& d, float4* bufA, float4* bufB, int nrows, uint32_t* mb, int slot0) {
  const int j = threadIdx.x, wave = j >> 6, lane = j & 63;
  float4* in = bufA;
  float4* out = bufB;
  for (int l = 0; l < d.L; ++l) {
    const int K = d.dims[l], N = d.dims[l + 1];
    const bool valid = j < N;
    const float bj = valid ? d.b[l][j] : 0.f;
    float4 acc[R4];
#pragma unroll
    for (int q = 0; q < R4; ++q) acc[q] = make_float4(bj, bj, bj, bj);
    dense_rows<R4>(d.W[l], K, N, j, in, acc);
    if (l < d.L - 1) {
      if (mb != nullptr) {
#pragma unroll
        for (int q = 0; q < R4; ++q)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int r = 4 * q + c;
            const unsigned long long bal = __ballot(valid && f4get(acc[q], c) > 0.f);
            if (r < nrows && lane == 0) {
              uint32_t* w = mb + ((slot0 + r) * GMPC_FZ_LHM + l) * GMPC_MW;
              w[2 * wave] = (uint32_t)bal;
              w[2 * wave + 1] = (uint32_t)(bal >> 32);
            }
          }
      }
#pragma unroll
      for (int q = 0; q < R4; ++q)
        acc[q] = make_float4(fmaxf(acc[q].x, 0.f), fmaxf(acc[q].y, 0.f), fmaxf(acc[q].z, 0.f), fmaxf(acc[q].w, 0.f));
    }
    if (valid)
#pragma unroll
      for (int q = 0; q < R4; ++q) out[j * R4 + q] = acc[q];
    __syncthreads();
    float4* tmp = in; in = out; out = tmp;
  }
  return in;
}

// Reverse pass: row r (< nrows) is e_i^T d out / d in of the MLP d at the point whose relu bits are mask slot s,
// with (i, s) = (rho % div, slot_base + rho / div), rho = rho0 + r.  Result in the returned buffer, [dims[0]][R].
template <int R4>
__device__ __forceinline__ float4* fz_reverse(const MlpDesc& d, float4* bufA, float4* bufB, int nrows, int rho0, int div,
                              int slot_base, const uint32_t* mb) {
  constexpr int R = 4 * R4;
  const int c = threadIdx.x;
  const int L = d.L;
  float* in = reinterpret_cast<float*>(bufA);
  {
    const int Kl = d.dims[L - 1], N = d.dims[L];
    if (c < Kl)
      for (int r = 0; r < R; ++r) {
        float g = 0.f;
        if (r < nrows) {
          const int rho = rho0 + r, i = rho % div, s = slot_base + rho / div;
          g = d.W[L - 1][(size_t)c * N + i];
          if (L > 1 && !fz_bit(mb, s, L - 2, c)) g = 0.f;
        }
        in[c * R + r] = g;
      }
  }
  __syncthreads();
  float4* cur = bufA;
  float4* nxt = bufB;
  for (int l = L - 2; l >= 0; --l) {
    const int K = d.dims[l + 1], N = d.dims[l];
    float4 acc[R4];
#pragma unroll
    for (int q = 0; q < R4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    dense_rows<R4>(d.WT[l], K, N, c, cur, acc);
    if (c < N) {
      float* o = reinterpret_cast<float*>(nxt) + c * R;
#pragma unroll
      for (int q = 0; q < R4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q + e;
          float g = f4get(acc[q], e);
          if (l > 0 && r < nrows) {
            const int rho = rho0 + r;
            if (!fz_bit(mb, slot_base + rho / div, l - 1, c)) g = 0.f;
          }
          o[r] = g;
        }
    }
    __syncthreads();
    float4* tmp = cur; cur = nxt; nxt = tmp;
  }
  return cur;
}

// Rollouts of nc rows.  NOMINAL: one row, u = U (the iterate's own rollout, X written to the ctx).  Otherwise row r
// is the step size alpha_0 / 2^(kfirst + r) of trajax ddp_rollout: u = U_t + (alpha k_t + K_t (x - X_t)), trajectory
// written to the candidate buffer.  BOX: that u clamped to [lo, hi] (bnd: lo[m] then hi[m]).  Returns the objective of
// row r in thread r (r < nc).
template <bool NOMINAL, bool BOX>
__device__ __forceinline__ float fz_rollout(const FusedSolveArgs& a, int b, int nc, int kfirst, float* sm, const float* bnd) {
  constexpr int R4 = GMPC_FZ_NC / 4, R = GMPC_FZ_NC;
  const int n = a.n, m = a.m, T = a.T, tid = threadIdx.x;
  float4* bufA = reinterpret_cast<float4*>(sm);
  float4* bufB = bufA + FZ_THREADS * R4;
  float* xr = reinterpret_cast<float*>(bufB + FZ_THREADS * R4);   // [R][n]
  float* ur = xr + R * n;                                           // [R][m]
  float* act = reinterpret_cast<float*>(bufA);
  const float* Xb = a.X + (size_t)b * (T + 1) * n;
  const float* Ub = a.U + (size_t)b * T * m;
  const float* gb = a.goal + (size_t)b * (T + 1) * n;
  const size_t cstride = (size_t)(T + 1) * n + (size_t)T * m;
  float* cb = a.cand + (size_t)b * GMPC_FZ_NC * cstride;
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]), w2 = sigmoidf_(a.mpc_w[2]);
  const float al = GMPC_ALPHA;
  for (int e = tid; e < R * n; e += FZ_THREADS) {
    const int r = e / n, i = e - r * n;
    const float x = a.x0[(size_t)b * n + i];
    xr[e] = x;
    if (NOMINAL && r == 0) a.X[(size_t)b * (T + 1) * n + i] = x;
    if (!NOMINAL && r < nc) cb[r * cstride + i] = x;
  }
  float cost = 0.f;   // running objective of row tid
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    // controls of the step
    for (int e = tid; e < R * m; e += FZ_THREADS) {
      const int r = e / m, i = e - r * m;
      float u = 0.f;
      if (r < nc) {
        const float U0 = Ub[(size_t)t * m + i];
        if (NOMINAL) {
          u = U0;
        } else {
          float alr = a.opts.alpha_0;
          for (int k = 0; k < kfirst + r; ++k) alr *= 0.5f;
          const float* Kr = a.K + (((size_t)b * T + t) * m + i) * n;
          float v = 0.f;
          for (int j = 0; j < n; ++j) v = fmaf(Kr[j], xr[r * n + j] - Xb[(size_t)t * n + j], v);
          u = U0 + (alr * a.k[((size_t)b * T + t) * m + i] + v);
          if constexpr (BOX) u = fz_clamp(u, bnd[i], bnd[m + i]);
          cb[r * cstride + (size_t)(T + 1) * n + (size_t)t * m + i] = u;
        }
      }
      ur[e] = u;
      act[(n + i) * R + r] = u;
    }
    for (int e = tid; e < R * n; e += FZ_THREADS) {
      const int r = e / n, i = e - r * n;
      act[i * R + r] = xr[e];
    }
    __syncthreads();
    // stage cost of (x_t, u_t), row tid
    if (tid < nc) {
      float uu = 0.f, dd = 0.f;
      for (int i = 0; i < m; ++i) uu = fmaf(ur[tid * m + i], ur[tid * m + i], uu);
      for (int i = 0; i < n; ++i) {
        const float dv = xr[tid * n + i] - gb[(size_t)t * n + i];
        dd = fmaf(dv, dv, dd);
      }
      cost += w0 * (sqrtf(uu + al * al) - al) + w1 * (sqrtf(dd + al * al) - al);
    }
    const float4* out = fz_forward<R4>(a.dyn, bufA, bufB, nc, nullptr, 0);
    const float* of = reinterpret_cast<const float*>(out);
    for (int e = tid; e < R * n; e += FZ_THREADS) {
      const int r = e / n, i = e - r * n;
      const float x = of[i * R + r] + xr[e];
      xr[e] = x;
      if (NOMINAL && r == 0) a.X[((size_t)b * (T + 1) + t + 1) * n + i] = x;
      if (!NOMINAL && r < nc) cb[r * cstride + (size_t)(t + 1) * n + i] = x;
    }
    __syncthreads();
  }
  // terminal cost w2 |MLP(x_T)|^2
  for (int e = tid; e < R * n; e += FZ_THREADS) {
    const int r = e / n, i = e - r * n;
    act[i * R + r] = xr[e];
  }
  __syncthreads();
  const float4* out = fz_forward<R4>(a.cost, bufA, bufB, nc, nullptr, 0);
  if (tid < nc) {
    const float* of = reinterpret_cast<const float*>(out);
    const int fo = a.cost.dims[a.cost.L];
    float yy = 0.f;
    for (int f = 0; f < fo; ++f) yy = fmaf(of[f * R + tid], of[f * R + tid], yy);
    cost += w2 * yy;
  }
  __syncthreads();
  return cost;
}

// Linearisation of the dynamics at every step of the iterate (AB) and the terminal quadratisation (QT, qT).
__device__ __forceinline__ void fz_linearize(const FusedSolveArgs& a, int b, float* sm) {
  constexpr int R4 = GMPC_FZ_JR / 4, R = GMPC_FZ_JR;
  const int n = a.n, m = a.m, T = a.T, nm = n + m, tid = threadIdx.x;
  float4* bufA = reinterpret_cast<float4*>(sm);
  float4* bufB = bufA + FZ_THREADS * R4;
  uint32_t* mb = reinterpret_cast<uint32_t*>(bufB + FZ_THREADS * R4);   // [(T+1)][LHM][MW]
  float* yT = reinterpret_cast<float*>(mb + (T + 1) * GMPC_FZ_LHM * GMPC_MW);   // [32]
  float* Jc = yT + 32;                                                            // [fout][n]
  float* act = reinterpret_cast<float*>(bufA);
  const float* Xb = a.X + (size_t)b * (T + 1) * n;
  const float* Ub = a.U + (size_t)b * T * m;
  // relu masks of every step (steps as rows)
  for (int t0 = 0; t0 < T; t0 += R) {
    const int nr = min(R, T - t0);
    for (int e = tid; e < nm * R; e += FZ_THREADS) {
      const int k = e / R, r = e - k * R;
      float v = 0.f;
      if (r < nr) v = k < n ? Xb[(size_t)(t0 + r) * n + k] : Ub[(size_t)(t0 + r) * m + (k - n)];
      act[e] = v;
    }
    __syncthreads();
    fz_forward<R4>(a.dyn, bufA, bufB, nr, mb, t0);
  }
  // the cost MLP at x_T: masks in slot T, output y
  for (int e = tid; e < n * R; e += FZ_THREADS) {
    const int k = e / R, r = e - k * R;
    act[e] = r == 0 ? Xb[(size_t)T * n + k] : 0.f;
  }
  __syncthreads();
  {
    const float4* out = fz_forward<R4>(a.cost, bufA, bufB, 1, mb, T);
    const int fo = a.cost.dims[a.cost.L];
    if (tid < fo) yT[tid] = reinterpret_cast<const float*>(out)[tid * R];
    __syncthreads();
  }
  // Jacobian rows of the dynamics: row rho = t n + i
  float* ABb = a.AB + (size_t)b * T * n * nm;
  for (int rho0 = 0; rho0 < T * n; rho0 += R) {
    const int nr = min(R, T * n - rho0);
    const float* J = reinterpret_cast<const float*>(fz_reverse<R4>(a.dyn, bufA, bufB, nr, rho0, n, 0, mb));
    for (int e = tid; e < nr * nm; e += FZ_THREADS) {
      const int r = e / nm, c = e - r * nm;
      const int rho = rho0 + r, i = rho % n;
      ABb[(size_t)rho * nm + c] = J[c * R + r] + (c == i ? 1.f : 0.f);
    }
    __syncthreads();
  }
  // terminal quadratisation: Jc = d y / d x_T, qT = 2 w2 Jc^T y, QT = 2 w2 Jc^T Jc
  const int fo = a.cost.dims[a.cost.L];
  for (int f0 = 0; f0 < fo; f0 += R) {
    const int nr = min(R, fo - f0);
    const float* J = reinterpret_cast<const float*>(fz_reverse<R4>(a.cost, bufA, bufB, nr, f0, fo, T, mb));
    for (int e = tid; e < nr * n; e += FZ_THREADS) {
      const int r = e / n, c = e - r * n;
      Jc[(f0 + r) * n + c] = J[c * R + r];
    }
    __syncthreads();
  }
  const float tw2 = 2.f * sigmoidf_(a.mpc_w[2]);
  for (int e = tid; e < n * n; e += FZ_THREADS) {
    const int i = e / n, j = e - i * n;
    float v = 0.f;
    for (int f = 0; f < fo; ++f) v = fmaf(Jc[f * n + i], Jc[f * n + j], v);
    a.QT[(size_t)b * n * n + e] = tw2 * v;
  }
  for (int i = tid; i < n; i += FZ_THREADS) {
    float v = 0.f;
    for (int f = 0; f < fo; ++f) v = fmaf(Jc[f * n + i], yT[f], v);
    a.qT[(size_t)b * n + i] = tw2 * v;
  }
  __syncthreads();
}

// Box QP of one step of the control-limited backward pass, on ONE lane: min 1/2 y^T Gd y + h^T y subject to
// lo - u <= y <= hi - u, Gd = G + delta I, by projected Newton from y = 0.  The clamped set is
// c = {j : y_j at its lower bound and g_j > 0, or at its upper bound and g_j < 0}, g = h + Gd y; the step on the free
// set is d_f = -Gd_ff^-1 g_f (Cholesky of Gd_ff, compact in Lc, the substitution order and the negation of
// fz_riccati's gain solve); projected Armijo backtracking on yt = clamp(y + s d) with the decrease written as
// g^T D + 1/2 D^T Gd D, D = yt - y; done when a full step leaves the clamped set unchanged.  Leaves y, the free list
// fi[0 .. nf) the factor in Lc belongs to, nf in qi[2m] and the iteration count in qi[2m+1]; returns true when the
// QP stopped at the iteration cap or without an acceptable step.  No comparison is true for a NaN, so NaN data
// takes the full step of the unconstrained solve and ends after one iteration.
__host__ __device__ __forceinline__ bool fz_box_qp(int m, const float* __restrict__ G, const float* __restrict__ hv,
                                                const float* __restrict__ uv, const float* __restrict__ bnd,
                                                float* __restrict__ Lc, float* __restrict__ qf, int* __restrict__ qi) {
  const float delta = 1e-8f;
  float* y = qf;
  float* g = y + m;
  float* d = g + m;
  float* yt = d + m;
  int* fi = qi;
  int* cl = qi + m;
  for (int j = 0; j < m; ++j) {
    y[j] = 0.f;
    g[j] = hv[j];
    const float lb = bnd[j] - uv[j], ub = bnd[m + j] - uv[j];
    cl[j] = (y[j] == lb && g[j] > 0.f) || (y[j] == ub && g[j] < 0.f);
  }
  int it = 0, nf = 0;
  bool capped = true;
  while (it < GMPC_BOX_QP_ITERS) {
    nf = 0;
    for (int j = 0; j < m; ++j)
      if (!cl[j]) fi[nf++] = j;
    for (int j = 0; j < nf; ++j) {
      float sdiag = G[fi[j] * m + fi[j]] + delta;
      for (int k = 0; k < j; ++k) sdiag -= Lc[j * m + k] * Lc[j * m + k];
      const float dg = sqrtf(sdiag);
      Lc[j * m + j] = dg;
      for (int i = j + 1; i < nf; ++i) {
        float v = G[fi[i] * m + fi[j]];
        for (int k = 0; k < j; ++k) v -= Lc[i * m + k] * Lc[j * m + k];
        Lc[i * m + j] = v / dg;
      }
    }
    // d_f = -Gd_ff^-1 g_f (yt is the compact work vector), d_c = 0
    for (int i = 0; i < nf; ++i) {
      float v = g[fi[i]];
      for (int k = 0; k < i; ++k) v -= Lc[i * m + k] * yt[k];
      yt[i] = v / Lc[i * m + i];
    }
    for (int i = nf - 1; i >= 0; --i) {
      float v = yt[i];
      for (int k = i + 1; k < nf; ++k) v -= Lc[k * m + i] * yt[k];
      yt[i] = v / Lc[i * m + i];
    }
    for (int j = 0; j < m; ++j) d[j] = 0.f;
    for (int i = 0; i < nf; ++i) d[fi[i]] = -yt[i];
    // projected Armijo backtracking
    float s = 1.f;
    bool found = false;
    for (int ls = 0; ls < GMPC_BOX_QP_HALVINGS; ++ls) {
      float gd = 0.f, quad = 0.f;
      for (int j = 0; j < m; ++j) yt[j] = fz_clamp(y[j] + s * d[j], bnd[j] - uv[j], bnd[m + j] - uv[j]);
      for (int i = 0; i < m; ++i) {
        const float di = yt[i] - y[i];
        float v = 0.f;
        for (int j = 0; j < m; ++j) v = fmaf(G[i * m + j] + (i == j ? delta : 0.f), yt[j] - y[j], v);
        gd = fmaf(g[i], di, gd);
        quad = fmaf(di, v, quad);
      }
      if (!(gd + 0.5f * quad > GMPC_BOX_ARMIJO * gd)) { found = true; break; }
      s *= 0.5f;
    }
    if (!found) break;
    ++it;
    bool changed = false;
    for (int j = 0; j < m; ++j) y[j] = yt[j];
    for (int i = 0; i < m; ++i) {
      float v = 0.f;
      for (int j = 0; j < m; ++j) v = fmaf(G[i * m + j] + (i == j ? delta : 0.f), y[j], v);
      g[i] = hv[i] + v;
      const float lb = bnd[i] - uv[i], ub = bnd[m + i] - uv[i];
      const int c = (y[i] == lb && g[i] > 0.f) || (y[i] == ub && g[i] < 0.f);
      changed |= c != cl[i];
      cl[i] = c;
    }
    if (s == 1.f && !changed) { capped = false; break; }
  }
  qi[2 * m] = nf;
  qi[2 * m + 1] = it;
  return capped;
}

// Riccati sweep (trajax tvlqr / lqr_step, c = 0, M = 0) with the adjoint recursion and the control gradient, then the
// continuation test of ilqr_base.  Returns the continuation flag (every thread).  BOX: the gains of a step are those
// of its box QP (k = y, the free rows of K = -Gd_ff^-1 H_f, the clamped rows 0.0), the value update is the same
// general form, and the continuation test's gradient norm leaves out the components a bound holds back.
template <bool BOX>
__device__ __forceinline__ bool fz_riccati(const FusedSolveArgs& a, const BoxSolveArgs& x, int b, float* sm, float* red,
                                           const float* bnd) {
  const int n = a.n, m = a.m, T = a.T, nm = n + m, lane = threadIdx.x;
  constexpr int NTH = FZ_THREADS;
  float* ABs = sm;                 // n x nm
  float* P = ABs + n * nm;         // n x n
  float* AtP = P + n * n;          // n x n (later S)
  float* T1 = AtP + n * n;         // n x n
  float* BtP = T1 + n * n;         // m x n
  float* Hm = BtP + m * n;         // m x n
  float* HGK = Hm + m * n;         // m x n
  float* Kk = HGK + m * n;         // m x (n+1)
  float* G = Kk + m * (n + 1);     // m x m
  float* Lc = G + m * m;           // m x m
  float* pv = Lc + m * m;          // n
  float* lam = pv + n;             // n
  float* dv = lam + n;             // n
  float* qv = dv + n;              // n
  float* tv = qv + n;              // n
  float* uv = tv + n;              // m
  float* rv = uv + m;              // m
  float* hv = rv + m;              // m
  float* qf = hv + m;              // BOX: fz_box_qp's floats (4 m), then its ints (2 m + 2)
  int* qi = reinterpret_cast<int*>(qf + 4 * m);
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]);
  const float delta = 1e-8f;
  for (int e = lane; e < n * n; e += NTH) P[e] = a.QT[(size_t)b * n * n + e];
  for (int i = lane; i < n; i += NTH) {
    const float q = a.qT[(size_t)b * n + i];
    pv[i] = q;
    lam[i] = q;
    a.adj[((size_t)b * (T + 1) + T) * n + i] = q;
  }
  float gn2 = 0.f;
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    const size_t bt = (size_t)b * T + t;
    for (int e = lane; e < n * nm; e += NTH) ABs[e] = a.AB[bt * n * nm + e];
    for (int i = lane; i < n; i += NTH)
      dv[i] = a.X[((size_t)b * (T + 1) + t) * n + i] - a.goal[((size_t)b * (T + 1) + t) * n + i];
    for (int j = lane; j < m; j += NTH) uv[j] = a.U[bt * m + j];
    __syncthreads();
    float dd = 0.f, uu = 0.f;
    for (int i = 0; i < n; ++i) dd = fmaf(dv[i], dv[i], dd);
    for (int j = 0; j < m; ++j) uu = fmaf(uv[j], uv[j], uu);
    const auto [is, is3, isu, isu3] = gmpc_ric_stage(dd, uu);
    for (int i = lane; i < n; i += NTH) qv[i] = w1 * dv[i] * is;
    for (int j = lane; j < m; j += NTH) rv[j] = w0 * uv[j] * isu;
    __syncthreads();
    // g_t = r_t + B^T lam ; lam_t = q_t + A^T lam
    for (int j = lane; j < m; j += NTH) {
      float g = 0.f;
      for (int i = 0; i < n; ++i) g = fmaf(ABs[i * nm + n + j], lam[i], g);
      g = rv[j] + g;
      if constexpr (BOX) {
        const bool held = (uv[j] == bnd[j] && g > 0.f) || (uv[j] == bnd[m + j] && g < 0.f);
        if (!held) gn2 = fmaf(g, g, gn2);
      } else {
        gn2 = fmaf(g, g, gn2);
      }
      a.grad[bt * m + j] = g;
    }
    for (int c = lane; c < n; c += NTH) {
      float v = 0.f;
      for (int i = 0; i < n; ++i) v = fmaf(ABs[i * nm + c], lam[i], v);
      tv[c] = qv[c] + v;
    }
    __syncthreads();
    for (int c = lane; c < n; c += NTH) {
      lam[c] = tv[c];
      a.adj[((size_t)b * (T + 1) + t) * n + c] = tv[c];
    }
    // AtP = A^T P ; BtP = B^T P
    for (int e = lane; e < n * n; e += NTH) {
      const int i = e / n, j = e - i * n;
      float v = 0.f;
      for (int k = 0; k < n; ++k) v = fmaf(ABs[k * nm + i], P[k * n + j], v);
      AtP[e] = v;
    }
    for (int e = lane; e < m * n; e += NTH) {
      const int i = e / n, j = e - i * n;
      float v = 0.f;
      for (int k = 0; k < n; ++k) v = fmaf(ABs[k * nm + n + i], P[k * n + j], v);
      BtP[e] = v;
    }
    __syncthreads();
    // T1 = AtP A ; Hm = BtP A ; G = sym(R + BtP B) ; h = r + B^T p
    for (int e = lane; e < n * n; e += NTH) {
      const int i = e / n, j = e - i * n;
      float v = 0.f;
      for (int k = 0; k < n; ++k) v = fmaf(AtP[i * n + k], ABs[k * nm + j], v);
      T1[e] = v;
    }
    for (int e = lane; e < m * n; e += NTH) {
      const int i = e / n, j = e - i * n;
      float v = 0.f;
      for (int k = 0; k < n; ++k) v = fmaf(BtP[i * n + k], ABs[k * nm + j], v);
      Hm[e] = v;
    }
    for (int e = lane; e < m * m; e += NTH) {
      const int i = e / m, j = e - i * m;
      float v = 0.f;
      for (int k = 0; k < n; ++k) v = fmaf(BtP[i * n + k], ABs[k * nm + n + j], v);
      const float Rij = w0 * ((i == j ? isu : 0.f) - uv[i] * uv[j] * isu3);
      Lc[e] = Rij + v;   // unsymmetrised, staged in Lc
    }
    for (int j = lane; j < m; j += NTH) {
      float v = 0.f;
      for (int i = 0; i < n; ++i) v = fmaf(ABs[i * nm + n + j], pv[i], v);
      hv[j] = rv[j] + v;
    }
    __syncthreads();
    for (int e = lane; e < m * m; e += NTH) {
      const int i = e / m, j = e - i * m;
      G[e] = (Lc[e] + Lc[j * m + i]) * 0.5f;
    }
    __syncthreads();
    // Cholesky of G + delta I (NaN on a non-positive pivot, like jax cho_factor), then [K k] = -(G + delta I)^-1 [H h]
    if constexpr (BOX) {
      if (lane == 0) {
        const bool capped = fz_box_qp(m, G, hv, uv, bnd, Lc, qf, qi);
        x.count[2 * b] += capped ? 1.f : 0.f;
        x.count[2 * b + 1] += (float)qi[2 * m + 1];
        x.iters[bt] = (float)qi[2 * m + 1];
      }
      __syncthreads();
      const int nf = qi[2 * m];
      const int* fi = qi;
      for (int c = lane; c < n; c += NTH) {
        for (int i = 0; i < m; ++i) Kk[i * (n + 1) + c] = 0.f;
        for (int i = 0; i < nf; ++i) {
          float v = Hm[fi[i] * n + c];
          for (int k = 0; k < i; ++k) v -= Lc[i * m + k] * Kk[fi[k] * (n + 1) + c];
          Kk[fi[i] * (n + 1) + c] = v / Lc[i * m + i];
        }
        for (int i = nf - 1; i >= 0; --i) {
          float v = Kk[fi[i] * (n + 1) + c];
          for (int k = i + 1; k < nf; ++k) v -= Lc[k * m + i] * Kk[fi[k] * (n + 1) + c];
          Kk[fi[i] * (n + 1) + c] = v / Lc[i * m + i];
        }
        for (int i = 0; i < nf; ++i) Kk[fi[i] * (n + 1) + c] = -Kk[fi[i] * (n + 1) + c];
      }
      for (int j = lane; j < m; j += NTH) {
        Kk[j * (n + 1) + n] = qf[j];
        x.clamped[bt * m + j] = 1.f;
      }
      __syncthreads();
      for (int i = lane; i < nf; i += NTH) x.clamped[bt * m + fi[i]] = 0.f;
    } else {
      if (lane == 0) gmpc_chol_lds_factor(m, G, delta, Lc);
      __syncthreads();
      for (int c = lane; c <= n; c += NTH) gmpc_chol_lds_solve(n, m, Lc, Hm, hv, c, Kk);
    }
    __syncthreads();
    for (int e = lane; e < m * n; e += NTH) {
      const int i = e / n, j = e - i * n;
      a.K[bt * m * n + e] = Kk[i * (n + 1) + j];
    }
    for (int j = lane; j < m; j += NTH) a.k[bt * m + j] = Kk[j * (n + 1) + n];
    for (int e = lane; e < m * n; e += NTH) {
      const int i = e / n, j = e - i * n;
      float v = 0.f;
      for (int k = 0; k < m; ++k) v = fmaf(G[i * m + k], Kk[k * (n + 1) + j], v);
      HGK[e] = Hm[e] + v;
    }
    __syncthreads();
    // S = Q + sym(T1) + HGK^T K + K^T H (staged in AtP), P = sym(S) ; p = q + A^T p + HGK^T k + K^T h
    for (int e = lane; e < n * n; e += NTH) {
      const int i = e / n, j = e - i * n;
      const float Qij = w1 * ((i == j ? is : 0.f) - dv[i] * dv[j] * is3);
      float v1 = 0.f, v2 = 0.f;
      for (int k = 0; k < m; ++k) {
        v1 = fmaf(HGK[k * n + i], Kk[k * (n + 1) + j], v1);
        v2 = fmaf(Kk[k * (n + 1) + i], Hm[k * n + j], v2);
      }
      AtP[e] = ((Qij + (T1[e] + T1[j * n + i]) * 0.5f) + v1) + v2;
    }
    for (int i = lane; i < n; i += NTH) {
      float v = 0.f, v1 = 0.f, v2 = 0.f;
      for (int k = 0; k < n; ++k) v = fmaf(ABs[k * nm + i], pv[k], v);
      for (int k = 0; k < m; ++k) {
        v1 = fmaf(HGK[k * n + i], Kk[k * (n + 1) + n], v1);
        v2 = fmaf(Kk[k * (n + 1) + i], hv[k], v2);
      }
      tv[i] = ((qv[i] + v) + v1) + v2;
    }
    __syncthreads();
    for (int e = lane; e < n * n; e += NTH) {
      const int i = e / n, j = e - i * n;
      P[e] = (AtP[e] + AtP[j * n + i]) * 0.5f;
    }
    for (int i = lane; i < n; i += NTH) pv[i] = tv[i];
    __syncthreads();
  }
  // continuation test (ilqr_base: maxiter, still improving obj / U, gradient norm thresholds, alpha > alpha_min)
  float un2 = 0.f;
  for (int e = lane; e < T * m; e += NTH) {
    const float u = a.U[(size_t)b * T * m + e];
    un2 = fmaf(u, u, un2);
  }
  gn2 = fz_block_sum(gn2, red);
  un2 = fz_block_sum(un2, red);
  const bool go = gmpc_ric_continue(gn2, un2, b, a.obj, a.obj_step, a.U_step, a.iters, a.alpha, a.opts);
  __syncthreads();
  return go;
}

template <bool BOX>
__device__ __forceinline__ void fz_solve(const FusedSolveArgs& a, const BoxSolveArgs& x) {
  extern __shared__ float4 fz_smem[];
  float* sm = reinterpret_cast<float*>(fz_smem);
  __shared__ float red[FZ_THREADS];
  __shared__ float s_on[GMPC_FZ_NC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = a.n, m = a.m, T = a.T;
  // BOX: the bounds, lo[m] then hi[m], behind the phases' carve-outs (a null pointer: unbounded on that side)
  const float* bnd = nullptr;
  if constexpr (BOX) {
    float* bw = sm + fz_phase_floats(n, m, T, true);
    for (int j = tid; j < m; j += FZ_THREADS) {
      bw[j] = x.u_lo ? x.u_lo[j] : -INFINITY;
      bw[m + j] = x.u_hi ? x.u_hi[j] : INFINITY;
    }
    if (tid == 0) {
      x.count[2 * b] = 0.f;
      x.count[2 * b + 1] = 0.f;
    }
    __syncthreads();
    bnd = bw;
  }
  // start: the ctx's copies of U_init / goal, the loop state of ilqr_base
  for (int e = tid; e < T * m; e += FZ_THREADS) {
    float u = a.U_init[(size_t)b * T * m + e];
    if constexpr (BOX) u = fz_clamp(u, bnd[e % m], bnd[m + e % m]);
    a.U[(size_t)b * T * m + e] = u;
  }
  for (int e = tid; e < (T + 1) * n; e += FZ_THREADS)
    a.goal[(size_t)b * (T + 1) * n + e] = a.goal_in[(size_t)b * (T + 1) * n + e];
  if (tid == 0) {
    a.iters[b] = 0;
    a.alpha[b] = a.opts.alpha_0;
    a.obj_step[b] = INFINITY;
    a.U_step[b] = INFINITY;
  }
  __syncthreads();
  {
    const float o = fz_rollout<true, BOX>(a, b, 1, 0, sm, bnd);
    if (tid == 0) a.obj[b] = o;
  }
  __syncthreads();
  fz_linearize(a, b, sm);
  bool go = fz_riccati<BOX>(a, x, b, sm, red, bnd);
  const size_t cstride = (size_t)(T + 1) * n + (size_t)T * m;
  for (int it = 0; it < a.opts.maxiter && go; ++it) {
    // line_search_ddp: halvings k = 0 .. k_max-1, GMPC_FZ_NC at a time, the first decrease in halving order wins
    float oo = a.obj[b];
    if (isnan(oo)) oo = INFINITY;
    int acc = -1;
    float on_acc = 0.f;
    for (int k0 = 0; k0 < a.k_max && acc < 0; k0 += GMPC_FZ_NC) {
      const int nc = min(GMPC_FZ_NC, a.k_max - k0);
      const float o = fz_rollout<false, BOX>(a, b, nc, k0, sm, bnd);
      if (tid < nc) s_on[tid] = o;
      __syncthreads();
      for (int j = 0; j < nc; ++j) {
        float on = s_on[j];
        if (isnan(on)) on = oo;
        if (on < oo) { acc = k0 + j; on_acc = on; break; }
      }
      __syncthreads();
    }
    auto halved = [&](int k) { float al = a.opts.alpha_0; for (; k > 0; --k) al *= 0.5f; return al; };
    if (acc >= 0) {
      const float* cb = a.cand + ((size_t)b * GMPC_FZ_NC + (acc % GMPC_FZ_NC)) * cstride;
      float us = 0.f;
      for (int e = tid; e < T * m; e += FZ_THREADS) {
        const float un = cb[(size_t)(T + 1) * n + e], d = un - a.U[(size_t)b * T * m + e];
        us = fmaf(d, d, us);
        a.U[(size_t)b * T * m + e] = un;
      }
      for (int e = tid; e < (T + 1) * n; e += FZ_THREADS) a.X[(size_t)b * (T + 1) * n + e] = cb[e];
      us = fz_block_sum(us, red);
      if (tid == 0) {
        a.obj[b] = on_acc;
        a.obj_step[b] = fabsf(on_acc - oo);
        a.alpha[b] = halved(acc + 1);
        a.U_step[b] = sqrtf(us);
      }
    } else if (tid == 0) {
      // every step size down to alpha_min failed (or alpha_0 <= alpha_min: no trial at all)
      a.alpha[b] = halved(a.k_max);
      a.U_step[b] = 0.f;
      a.obj_step[b] = 0.f;
    }
    if (tid == 0) a.iters[b] += 1;
    __syncthreads();
    fz_linearize(a, b, sm);
    go = fz_riccati<BOX>(a, x, b, sm, red, bnd);
  }
  // caller outputs
  if (a.oX) for (int e = tid; e < (T + 1) * n; e += FZ_THREADS) a.oX[(size_t)b * (T + 1) * n + e] = a.X[(size_t)b * (T + 1) * n + e];
  if (a.oU) for (int e = tid; e < T * m; e += FZ_THREADS) a.oU[(size_t)b * T * m + e] = a.U[(size_t)b * T * m + e];
  if (a.ograd) for (int e = tid; e < T * m; e += FZ_THREADS) a.ograd[(size_t)b * T * m + e] = a.grad[(size_t)b * T * m + e];
  if (a.oadj)
    for (int e = tid; e < (T + 1) * n; e += FZ_THREADS) a.oadj[(size_t)b * (T + 1) * n + e] = a.adj[(size_t)b * (T + 1) * n + e];
  if (tid == 0) {
    if (a.oobj) a.oobj[b] = a.obj[b];
    if (a.oiters) a.oiters[b] = a.iters[b];
  }
}

__global__ __launch_bounds__(FZ_THREADS) void k_ilqr_fused(FusedSolveArgs a) { fz_solve<false>(a, BoxSolveArgs{}); }
__global__ __launch_bounds__(FZ_THREADS) void k_ilqr_box(FusedSolveArgs a, BoxSolveArgs x) { fz_solve<true>(a, x); }

size_t gmpc_fused_lds_bytes(int n, int m, int T, bool box) {
  return (size_t)(fz_phase_floats(n, m, T, box) + (box ? 2 * m : 0)) * sizeof(float);
}

void gmpc_launch_ilqr_fused(const FusedSolveArgs& a, int B, hipStream_t s) {
  const size_t lds = gmpc_fused_lds_bytes(a.n, a.m, a.T);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ilqr_fused),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
    attr = true;
  }
  hipLaunchKernelGGL(k_ilqr_fused, dim3(B), dim3(FZ_THREADS), lds, s, a);
}

// fz_box_qp on the host, for the CPU tests: the routine the kernel runs on one lane, compiled for the host from the same
// source, on one QP in host memory.
extern "C" int gmpc_box_qp_host(int m, const float* G, const float* h, const float* u, const float* u_lo,
                                const float* u_hi, float* y, int* clamped, int* iterations) {
  if (m < 1 || m > GMPC_BOX_MAX_M || !G || !h || !u || !u_lo || !u_hi || !y || !clamped || !iterations)
    return GMPC_EINVAL;
  float bnd[2 * GMPC_BOX_MAX_M], Lc[GMPC_BOX_MAX_M * GMPC_BOX_MAX_M], qf[4 * GMPC_BOX_MAX_M];
  int qi[2 * GMPC_BOX_MAX_M + 2];
  for (int j = 0; j < m; ++j) {
    bnd[j] = u_lo[j];
    bnd[m + j] = u_hi[j];
  }
  const bool capped = fz_box_qp(m, G, h, u, bnd, Lc, qf, qi);
  for (int j = 0; j < m; ++j) {
    y[j] = qf[j];
    clamped[j] = 1;
  }
  for (int i = 0; i < qi[2 * m]; ++i) clamped[qi[i]] = 0;
  iterations[0] = qi[2 * m + 1];
  iterations[1] = capped ? 1 : 0;
  return 0;
}

void gmpc_launch_ilqr_box(const FusedSolveArgs& a, const BoxSolveArgs& x, int B, hipStream_t s) {
  const size_t lds = gmpc_fused_lds_bytes(a.n, a.m, a.T, true);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ilqr_box),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
    attr = true;
  }
  hipLaunchKernelGGL(k_ilqr_box, dim3(B), dim3(FZ_THREADS), lds, s, a, x);
}
