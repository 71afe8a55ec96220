// The pieces of one iLQR Riccati step that the forms of the sweep share: k_riccati (gmpc_backward.hip), the two-wave
// k_riccati_w2 (gmpc_riccati_w.hip), fz_riccati (gmpc_fused_solve.hip) and k_big_cont (gmpc_large.hip).  Each is the
// text its callers used to carry, inlined: the operations and their order are part of the results' bits.
#pragma once
#include "gmpc_device.h"

// trajax' continuation test (ilqr_base: maxiter, still improving obj / U, gradient norm thresholds, alpha > alpha_min)
// of trajectory b, from the squared norms of its control gradient and controls; the callers reduce those themselves
__device__ __forceinline__ bool gmpc_ric_continue(float gn2, float un2, int b, const float* obj, const float* obj_step,
                                                  const float* U_step, const int* iters, const float* alpha,
                                                  const gmpc_ilqr_opts& opts) {
  float gn = sqrtf(gn2);
  if (isnan(gn)) gn = INFINITY;
  const float aobj = fabsf(obj[b]) + 1.0f;
  const float un = sqrtf(un2) + 1.0f;
  const bool progressing = (obj_step[b] > opts.obj_step_threshold * aobj) &&
                           (U_step[b] > opts.inputs_step_threshold * un);
  const bool potential = (gn > opts.grad_norm_threshold) && (gn > opts.relative_grad_norm_threshold * aobj);
  return (iters[b] < opts.maxiter) && progressing && potential && (alpha[b] > opts.alpha_min);
}

// the stage cost's scalars from dd = |x - g|^2, uu = |u|^2: 1 / s, 1 / s^3 of s = sqrt(dd + alpha^2), the same of uu
struct RicStage { float is, is3, isu, isu3; };
__device__ __forceinline__ RicStage gmpc_ric_stage(float dd, float uu) {
  const float al = GMPC_ALPHA;
  const float s = sqrtf(dd + al * al), su = sqrtf(uu + al * al);
  const float is = 1.f / s, is3 = is * is * is, isu = 1.f / su, isu3 = isu * isu * isu;
  return {is, is3, isu, isu3};
}

// Cholesky of G + delta I for a run-time m, through LDS, into Lc (NaN on a non-positive pivot, like jax cho_factor),
// on one lane.  (The in-register form for a compile-time m stays written out in k_riccati and k_riccati_w2: as a
// routine, whatever its signature, it reschedules the two-wave iLQR sweep -- same registers, same LDS, same bits --
// and that costs the headline step's Riccati kernel 0.1723 -> 0.1739 ms, 1 %, on an MI355X.)
__device__ __forceinline__ void gmpc_chol_lds_factor(int m, const float* G, float delta, float* Lc) {
  for (int j = 0; j < m; ++j) {
    float sdiag = G[j * m + j] + delta;
    for (int k = 0; k < j; ++k) sdiag -= Lc[j * m + k] * Lc[j * m + k];
    const float d = sqrtf(sdiag);
    Lc[j * m + j] = d;
    for (int i = j + 1; i < m; ++i) {
      float v = G[i * m + j];
      for (int k = 0; k < j; ++k) v -= Lc[i * m + k] * Lc[j * m + k];
      Lc[i * m + j] = v / d;
    }
  }
}
// column c of the right-hand side (H[:, c] for c < n, h for c == n; Hm is m x n) into column c of Kk (m x (n + 1))
__device__ __forceinline__ void gmpc_chol_lds_solve(int n, int m, const float* Lc, const float* Hm, const float* hv,
                                                    int c, float* Kk) {
  for (int i = 0; i < m; ++i) {
    float v = c < n ? Hm[i * n + c] : hv[i];
    for (int k = 0; k < i; ++k) v -= Lc[i * m + k] * Kk[k * (n + 1) + c];
    Kk[i * (n + 1) + c] = v / Lc[i * m + i];
  }
  for (int i = m - 1; i >= 0; --i) {
    float v = Kk[i * (n + 1) + c];
    for (int k = i + 1; k < m; ++k) v -= Lc[k * m + i] * Kk[k * (n + 1) + c];
    Kk[i * (n + 1) + c] = v / Lc[i * m + i];
  }
  for (int i = 0; i < m; ++i) Kk[i * (n + 1) + c] = -Kk[i * (n + 1) + c];
}
