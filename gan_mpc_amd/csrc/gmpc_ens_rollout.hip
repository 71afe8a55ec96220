// A plan's rollout under every member of a dynamics ensemble (gmpc_ensemble_rollout): forward
// only, B different problems, each with its own x0, goals and controls.
//
//   k_ens_rollout   one 256-thread workgroup per 32 PROBLEMS under one member (grid: tiles of 32 problems by members).
//                   The arithmetic is cem_rollout_body's (gmpc_cem_rollout.h), reused: the 32 states in registers in
//                   dg_gemm's accumulator layout, the layer inputs in one [32][GMPC_DG_LDA] fp32 LDS block, every
//                   layer on dg_gemm, the row sums by cem_row8_sum -- so a problem's X and obj are bitwise those of
//                   the sampled rollout's mean_row form under the same network.  What differs: x0, goal and U are per
//                   row, every row's states are written (from the LDS block, rows of n floats), the costs are kept
//                   per step, and the horizon may be cut short (S <= T steps, then without costs).
//   k_ens_rollout_feedback  (gmpc_ensemble_rollout_feedback) the same body in closed loop: a
//                   row's controls are formed at every step from its own state by a time-varying feedback law around
//                   a reference trajectory, clamped, and written out per member.
//   k_ens_moments   one thread per (problem, step, state): mean and population variance over the members' planes,
//                   both sums sequential in ascending member order.
//   k_ens_disagreement  (gmpc_ensemble_disagreement) k_ens_rollout's grid, the rows rolled out
//                   under the bound dynamics and member p's one-step output measured against theirs at every step.
#include "gmpc_cem_rollout.h"

// The body of k_ens_rollout and of k_ens_rollout_feedback, over where a step's controls come
// from.  Fb false: U[b][t] as given (f is not read).  Fb true: the row's 8 lanes form u_t = clamp(U_ref + K (x_t -
// X_ref) + alpha k) from the row's x_t in the operand block -- lane rc the controls rc, rc + 8, ..., each a sequential
// fmaf chain over the states in ascending order, so a row's controls depend on neither its place in the tile nor on B
// or P -- behind the step's first barrier, and a second barrier hands the block to layer 0.  The stage cost reads the
// controls its own lane wrote.  Everything else is one text for both.
template <bool Fb>
__device__ __forceinline__ void ens_rollout_body(const EnsRollArgs& a, const EnsFeedbackArgs& f, float* Ab) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, T = a.T, S = a.S, B = a.B;
  const int b0 = blockIdx.x * GMPC_CEM_ROWS;     // row i of the tile is problem b0 + i
  const size_t p = blockIdx.y;                   // the member
  const int rrow = tid >> 3, rc = tid & 7;       // the row whose sums this thread shares in, its lane of the row's 8
  const bool costed = a.goal != nullptr;         // (the launcher: only with S == T)
  // Rows past B (the last tile): every read goes to problem B - 1, a valid one, and nothing is written for them.
  const int last = B - 1;
  const int rb = min(b0 + rrow, last);           // the problem whose goals this thread's row reads
  const bool rlive = b0 + rrow < B;
  float w0 = 0.f, w1 = 0.f, w2 = 0.f;
  if (costed) {
    w0 = sigmoidf_(a.mpc_w[0]); w1 = sigmoidf_(a.mpc_w[1]); w2 = sigmoidf_(a.mpc_w[2]);
  }
  const float al = GMPC_ALPHA;
  // a.x0's rows: n floats apart, or -- the feedback call without an x0 of its own -- X_ref's, S + 1 states apart
  const size_t xstride = Fb ? f.x0_stride : (size_t)n;
  // x_t of the 32 rows, in dg_gemm's accumulator layout: the output layer's tile of a thread is its tile of x
  DgTiles xs;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const int j = (wave + 4 * ci) * 16 + l16;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int bp = min(b0 + 4 * kq + rr, last), bq = min(b0 + 16 + 4 * kq + rr, last);
      xs.p[ci][rr] = j < n ? a.x0[(size_t)bp * xstride + j] : 0.f;
      xs.q[ci][rr] = j < n ? a.x0[(size_t)bq * xstride + j] : 0.f;
    }
  }
  float* Xp = a.X ? a.X + p * B * (size_t)(S + 1) * n : nullptr;          // the member's planes
  float* Cp = a.costs ? a.costs + p * B * (size_t)(T + 1) : nullptr;
  float csum = 0.f;   // the cost of row rrow so far (the same in its 8 lanes)
  DgTiles acc;
  for (int t = 0; t < S; ++t) {
    // ---- layer 0 input [x_t; u_t]
    cem_store_tiles(Ab, xs, n, wave, lane, [](float v, int) { return v; });
    if constexpr (!Fb)
      for (int e = tid; e < GMPC_CEM_ROWS * m; e += GMPC_DG_THREADS) {
        const int i = e / m, j = e - i * m;
        Ab[i * GMPC_DG_LDA + n + j] = a.U[((size_t)min(b0 + i, last) * S + t) * m + j];
      }
    __syncthreads();
    // ---- x_t of every live row, from the operand block
    if (Xp)
      for (int e = tid; e < GMPC_CEM_ROWS * n; e += GMPC_DG_THREADS) {
        const int i = e / n, j = e - i * n;
        if (b0 + i < B) Xp[((size_t)(b0 + i) * (S + 1) + t) * n + j] = Ab[i * GMPC_DG_LDA + j];
      }
    // ---- the feedback law: u_t of row rrow from its x_t, into the block and to U[p][b][t]
    if constexpr (Fb) {
      float* row = Ab + rrow * GMPC_DG_LDA;
      const size_t bt = (size_t)rb * S + t;
      const float* xr = f.X_ref + ((size_t)rb * (S + 1) + t) * n;
      for (int j = rc; j < m; j += 8) {
        const float* Kj = f.K + (bt * m + j) * n;
        float du = 0.f;
        for (int c = 0; c < n; ++c) du = fmaf(Kj[c], row[c] - xr[c], du);
        if (f.k) du = du + __fmul_rn(f.alpha, f.k[bt * m + j]);
        float u = f.U_ref[bt * m + j] + du;
        if (f.u_lo) {     // (comparisons, not fminf / fmaxf: a NaN control stays one)
          const float lo = f.u_lo[j], hi = f.u_hi[j];
          u = u < lo ? lo : u;
          u = u > hi ? hi : u;
        }
        row[n + j] = u;
        if (f.U && rlive) f.U[((p * B + b0 + rrow) * S + t) * m + j] = u;
      }
    }
    // ---- stage cost of (x_t, u_t) against goal_t
    if (costed) {
      const float* row = Ab + rrow * GMPC_DG_LDA;
      const float* g = a.goal + ((size_t)rb * (T + 1) + t) * n;
      float su = 0.f, sx = 0.f;
      for (int j = rc; j < m; j += 8) su = fmaf(row[n + j], row[n + j], su);
      for (int j = rc; j < n; j += 8) {
        const float d = row[j] - g[j];
        sx = fmaf(d, d, sx);
      }
      su = cem_row8_sum(su);
      sx = cem_row8_sum(sx);
      // (the roundings of the sampled body's `csum += w0 * .. + w1 * ..` as the compiler contracts it there, written
      // out: here the two products would be paired into one packed multiply and stay unfused)
      const float c = fmaf(w0, sqrtf(su + al * al) - al, w1 * (sqrtf(sx + al * al) - al));
      csum += c;
      if (Cp && rc == 0 && rlive) Cp[(size_t)(b0 + rrow) * (T + 1) + t] = c;
    }
    if constexpr (Fb) __syncthreads();   // every row's u_t is in the block
    // ---- x_{t+1} = x_t + MLP([x_t; u_t]) under member p
    for (int l = 0; l < a.dyn.L; ++l) {
      const int K = a.dyn.dims[l], Nl = a.dyn.dims[l + 1];
      dg_gemm(Ab, K, Nl, a.dyn.W[l] + p * a.mstride, wave, lane, acc);
      __syncthreads();   // every wave has read its operand rows (and the stage cost and the copy of x_t theirs)
      const float* bias = a.dyn.b[l] + p * a.mstride;
      if (l < a.dyn.L - 1) {
        cem_store_tiles(Ab, acc, Nl, wave, lane, [bias](float v, int j) { return fmaxf(v + bias[j], 0.f); });
        __syncthreads();
      } else {
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const int j = (wave + 4 * ci) * 16 + l16;
          if (j >= n) continue;
          const float bj = bias[j];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            xs.p[ci][rr] = (acc.p[ci][rr] + bj) + xs.p[ci][rr];
            xs.q[ci][rr] = (acc.q[ci][rr] + bj) + xs.q[ci][rr];
          }
        }
      }
    }
  }
  // ---- x_S into the operand block: the last copy of the states and the cost MLP's input
  cem_store_tiles(Ab, xs, n, wave, lane, [](float v, int) { return v; });
  __syncthreads();
  if (Xp)
    for (int e = tid; e < GMPC_CEM_ROWS * n; e += GMPC_DG_THREADS) {
      const int i = e / n, j = e - i * n;
      if (b0 + i < B) Xp[((size_t)(b0 + i) * (S + 1) + S) * n + j] = Ab[i * GMPC_DG_LDA + j];
    }
  if (!costed) return;     // (uniform over the workgroup)
  // ---- terminal cost w2 |MLP_c(x_T)|^2
  for (int l = 0; l < a.cost.L; ++l) {
    const int K = a.cost.dims[l], Nl = a.cost.dims[l + 1];
    dg_gemm(Ab, K, Nl, a.cost.W[l], wave, lane, acc);
    __syncthreads();
    const float* bias = a.cost.b[l];
    if (l < a.cost.L - 1)
      cem_store_tiles(Ab, acc, Nl, wave, lane, [bias](float v, int j) { return fmaxf(v + bias[j], 0.f); });
    else
      cem_store_tiles(Ab, acc, Nl, wave, lane, [bias](float v, int j) { return v + bias[j]; });
    __syncthreads();
  }
  {
    const float* row = Ab + rrow * GMPC_DG_LDA;
    const int fout = a.cost.dims[a.cost.L];
    float sy = 0.f;
    for (int j = rc; j < fout; j += 8) sy = fmaf(row[j], row[j], sy);
    sy = cem_row8_sum(sy);
    const float c = w2 * sy;
    csum = fmaf(w2, sy, csum);     // (the sampled body's `csum += w2 * sy`, one rounding, as it is contracted there)
    if (rc == 0 && rlive) {
      if (Cp) Cp[(size_t)(b0 + rrow) * (T + 1) + T] = c;
      if (a.obj) a.obj[p * B + b0 + rrow] = csum;
    }
  }
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_ens_rollout(EnsRollArgs a) {
  __shared__ __attribute__((aligned(16))) float Ab[GMPC_CEM_ROWS * GMPC_DG_LDA];   // the layer inputs of the 32 rows
  ens_rollout_body<false>(a, EnsFeedbackArgs{}, Ab);
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_ens_rollout_feedback(EnsRollArgs a, EnsFeedbackArgs f) {
  __shared__ __attribute__((aligned(16))) float Ab[GMPC_CEM_ROWS * GMPC_DG_LDA];
  ens_rollout_body<true>(a, f, Ab);
}

// A plan's one-step disagreement under every member (gmpc_ensemble_disagreement): k_ens_rollout's
// tiles of 32 problems by members, the steps cem_disagree_step's -- the arithmetic of the sampled rollout under
// CemDisagree, so d and D are bitwise what a disagreement solve adds to a row with these controls.  The rows run
// under the nominal layers; member blockIdx.y only measures.  X (the nominal rollout) is written by grid row 0.
struct EnsDisMember {
  size_t mstride;
  const CemNominal& nom;     // (the kernel's argument, read where it lies)
  __device__ __forceinline__ const float* W(const float* w, uint32_t) const { return w + blockIdx.y * mstride; }
  __device__ __forceinline__ const float* b(const float* v, uint32_t) const { return v + blockIdx.y * mstride; }
  __device__ __forceinline__ const CemNominal& nominal() const { return nom; }
};

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_ens_disagreement(EnsDisArgs a) {
  __shared__ __attribute__((aligned(16))) float Ab[GMPC_CEM_ROWS * GMPC_DG_LDA];   // the layer inputs of the 32 rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, S = a.S, B = a.B;
  const int b0 = blockIdx.x * GMPC_CEM_ROWS;     // row i of the tile is problem b0 + i
  const size_t p = blockIdx.y;                   // the member
  const int rrow = tid >> 3, rc = tid & 7;
  // Rows past B (the last tile): every read goes to problem B - 1, a valid one, and nothing is written for them.
  const int last = B - 1;
  const bool rlive = b0 + rrow < B;
  const EnsDisMember ens{a.mstride, a.nom};
  DgTiles xs;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const int j = (wave + 4 * ci) * 16 + l16;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int bp = min(b0 + 4 * kq + rr, last), bq = min(b0 + 16 + 4 * kq + rr, last);
      xs.p[ci][rr] = j < n ? a.x0[(size_t)bp * n + j] : 0.f;
      xs.q[ci][rr] = j < n ? a.x0[(size_t)bq * n + j] : 0.f;
    }
  }
  float* Xp = a.X && p == 0 ? a.X : nullptr;
  float* dp = a.d ? a.d + p * B * (size_t)S : nullptr;
  float dsum = 0.f;   // D of row rrow so far (the same in its 8 lanes)
  for (int t = 0; t < S; ++t) {
    // ---- layer 0 input [x_t; u_t]
    cem_store_tiles(Ab, xs, n, wave, lane, [](float v, int) { return v; });
    for (int e = tid; e < GMPC_CEM_ROWS * m; e += GMPC_DG_THREADS) {
      const int i = e / m, j = e - i * m;
      Ab[i * GMPC_DG_LDA + n + j] = a.U[((size_t)min(b0 + i, last) * S + t) * m + j];
    }
    __syncthreads();
    // ---- x_t of every live row, from the operand block (read before the step's first barrier releases the block)
    if (Xp)
      for (int e = tid; e < GMPC_CEM_ROWS * n; e += GMPC_DG_THREADS) {
        const int i = e / n, j = e - i * n;
        if (b0 + i < B) Xp[((size_t)(b0 + i) * (S + 1) + t) * n + j] = Ab[i * GMPC_DG_LDA + j];
      }
    const float dt = cem_disagree_step<false>(a.dyn, ens, 0u, n, Ab, nullptr, xs, wave, lane, rrow, rc);
    dsum += dt;
    if (dp && rc == 0 && rlive) dp[(size_t)(b0 + rrow) * S + t] = dt;
  }
  if (a.D && rc == 0 && rlive) a.D[p * B + b0 + rrow] = dsum;
  if (Xp) {
    cem_store_tiles(Ab, xs, n, wave, lane, [](float v, int) { return v; });
    __syncthreads();
    for (int e = tid; e < GMPC_CEM_ROWS * n; e += GMPC_DG_THREADS) {
      const int i = e / n, j = e - i * n;
      if (b0 + i < B) Xp[((size_t)(b0 + i) * (S + 1) + S) * n + j] = Ab[i * GMPC_DG_LDA + j];
    }
  }
}

// Mean and population variance over the planes X [P][count] of one element each: sum_p x_p, then / P; sum_p (x_p -
// mean)^2, then / P -- every operation one IEEE fp32 operation in ascending p (no contraction), so the result is a
// function of the planes alone and NumPy restates it bit for bit.  mean / var: either may be null.
__global__ __launch_bounds__(GMPC_THREADS) void k_ens_moments(const float* __restrict__ X, int P, size_t count,
                                                              float* __restrict__ mean, float* __restrict__ var) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * GMPC_THREADS + threadIdx.x;
  if (i >= count) return;
  const float fP = (float)P;
  float sum = X[i];
  for (int p = 1; p < P; ++p) sum = sum + X[p * count + i];
  const float mu = sum / fP;
  if (mean) mean[i] = mu;
  if (!var) return;
  float ss = 0.f;
  for (int p = 0; p < P; ++p) {
    const float d = X[p * count + i] - mu;
    const float dd = d * d;
    ss = ss + dd;
  }
  var[i] = ss / fP;
}

// Host-side launchers ---------------------------------------------------------------------------
// What both forms of the rollout cover
static bool ens_rollout_covered(const EnsRollArgs& a, int P) {
  for (int l = 0; l <= a.dyn.L; ++l)
    if (a.dyn.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return false;
  for (int l = 0; l <= a.cost.L; ++l)
    if (a.cost.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return false;
  if (a.n + a.m > GMPC_SAMPLED_MAX_WIDTH || a.B < 1 || a.S < 1 || a.S > a.T || P < 1 || P > GMPC_MAX_ENSEMBLE)
    return false;
  if ((a.costs || a.obj) && !a.goal) return false;
  return !a.goal || a.S == a.T;
}

int gmpc_launch_ens_rollout(const EnsRollArgs& a, int P, hipStream_t s) {
  if (!ens_rollout_covered(a, P)) return 1;
  const dim3 grid((a.B + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS, P);
  hipLaunchKernelGGL(k_ens_rollout, grid, dim3(GMPC_DG_THREADS), 0, s, a);
  return 0;
}

int gmpc_launch_ens_rollout_feedback(const EnsRollArgs& a, const EnsFeedbackArgs& f, int P, hipStream_t s) {
  if (!ens_rollout_covered(a, P)) return 1;
  if (!a.x0 || !f.X_ref || !f.U_ref || !f.K || !f.u_lo != !f.u_hi) return 1;
  if (f.x0_stride != (size_t)a.n && f.x0_stride != (size_t)(a.S + 1) * a.n) return 1;
  const dim3 grid((a.B + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS, P);
  hipLaunchKernelGGL(k_ens_rollout_feedback, grid, dim3(GMPC_DG_THREADS), 0, s, a, f);
  return 0;
}

int gmpc_launch_ens_disagreement(const EnsDisArgs& a, int P, hipStream_t s) {
  for (int l = 0; l <= a.dyn.L; ++l)
    if (a.dyn.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return 1;
  if (a.n + a.m > GMPC_SAMPLED_MAX_WIDTH || a.B < 1 || a.S < 1 || P < 1 || P > GMPC_MAX_ENSEMBLE) return 1;
  if (!a.X && !a.d && !a.D) return 1;
  const dim3 grid((a.B + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS, P);
  hipLaunchKernelGGL(k_ens_disagreement, grid, dim3(GMPC_DG_THREADS), 0, s, a);
  return 0;
}

void gmpc_launch_ens_moments(const float* X, int P, size_t count, float* mean, float* var, hipStream_t s) {
  const unsigned blocks = (unsigned)((count + GMPC_THREADS - 1) / GMPC_THREADS);
  hipLaunchKernelGGL(k_ens_moments, dim3(blocks), dim3(GMPC_THREADS), 0, s, X, P, count, mean, var);
}
