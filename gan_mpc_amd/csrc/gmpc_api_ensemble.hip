// C-ABI entry point of the ensemble rollout: a plan's trajectories and costs under every member of a
// dynamics ensemble, and the members' spread per step; and of the plan's one-step disagreement.  Forward
// only, stateless; no kernel in this file.
#include "gmpc_ctx.h"

// Two launches at most on the caller's stream (k_ens_rollout, k_ens_moments), nothing waited for.  It reads mpc_w and
// the cost MLP of the bound parameters; the set ensemble, its mode, the sampled precision and a held solution are
// neither read nor changed.  The members' planes of a call that wants moments but no X live in the call workspace.
extern "C" int gmpc_ensemble_rollout(gmpc_ctx* c, int B, int S, int P, const float* dyn_members, const float* x0,
                                     const float* U, const float* goal, float* X, float* costs, float* obj,
                                     float* x_mean, float* x_var, void* stream) {
  const char* who = "ensemble rollout";
  if (!c) return fail(GMPC_EINVAL, "%s: ctx is null", who);
  if (!dyn_members || !x0 || !U) return fail(GMPC_EINVAL, "%s: dyn_members, x0 and U must not be null", who);
  const gmpc_shape& sh = c->sh;
  if (B < 1 || B > c->maxB) return fail(GMPC_EINVAL, "%s: B = %d outside [1, max_batch = %d]", who, B, c->maxB);
  if (S < 1 || S > sh.T) return fail(GMPC_EINVAL, "%s: S = %d outside [1, T = %d]", who, S, sh.T);
  if (P < 1 || P > GMPC_MAX_ENSEMBLE) return fail(GMPC_EINVAL, "%s: P = %d outside [1, %d]", who, P, GMPC_MAX_ENSEMBLE);
  if (!c->params_set) return fail(GMPC_EINVAL, "%s: gmpc_set_params has not been called", who);
  if (!X && !costs && !obj && !x_mean && !x_var) return fail(GMPC_EINVAL, "%s: every output is null", who);
  if ((costs || obj) && !goal) return fail(GMPC_EINVAL, "%s: costs and obj need goal", who);
  if ((costs || obj) && S != sh.T)
    return fail(GMPC_EINVAL, "%s: costs and obj need the whole horizon, S = %d is not T = %d", who, S, sh.T);
  TRY(gmpc_sampled_coverage(c, who));
  if (hipSetDevice(c->device) != hipSuccess) return fail(GMPC_EHIP, "hipSetDevice failed");
  (void)hipGetLastError();
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t plane = (size_t)B * (S + 1) * sh.n;
  const bool moments = x_mean || x_var;
  float* planes = X;
  if (moments && !planes) {
    TRY(c->cw.save.grow(c, (size_t)P * plane));
    planes = c->cw.save.p;
  }
  EnsRollArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.S = S; a.T = sh.T; a.n = sh.n; a.m = sh.m;
  bind_mlp(a.dyn, sh.dyn_layers, sh.dyn_dims, dyn_members, nullptr);
  a.mstride = (size_t)mlp_count(sh.dyn_layers, sh.dyn_dims);
  a.cost = c->cost; a.mpc_w = c->mpc_w;
  a.x0 = x0; a.U = U;
  a.goal = costs || obj ? goal : nullptr;     // a goal nobody costs against is not read
  a.X = planes; a.costs = costs; a.obj = obj;
  if (gmpc_launch_ens_rollout(a, P, s)) return fail(GMPC_EINVAL, "%s: shape not covered", who);
  if (moments) gmpc_launch_ens_moments(planes, P, plane, x_mean, x_var, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The one-step disagreement of every member with the bound dynamics along a plan's nominal rollout: one
// launch on the caller's stream (k_ens_disagreement), fp32, nothing waited for.  It reads the dynamics of the bound
// parameters; the set ensemble, its mode, the disagreement setting, the sampled precision and a held solution are
// neither read nor changed.
extern "C" int gmpc_ensemble_disagreement(gmpc_ctx* c, int B, int S, int P, const float* dyn_members, const float* x0,
                                          const float* U, float* X, float* d, float* D, void* stream) {
  const char* who = "ensemble disagreement";
  if (!c) return fail(GMPC_EINVAL, "%s: ctx is null", who);
  if (!dyn_members || !x0 || !U) return fail(GMPC_EINVAL, "%s: dyn_members, x0 and U must not be null", who);
  const gmpc_shape& sh = c->sh;
  if (B < 1 || B > c->maxB) return fail(GMPC_EINVAL, "%s: B = %d outside [1, max_batch = %d]", who, B, c->maxB);
  if (S < 1 || S > sh.T) return fail(GMPC_EINVAL, "%s: S = %d outside [1, T = %d]", who, S, sh.T);
  if (P < 1 || P > GMPC_MAX_ENSEMBLE) return fail(GMPC_EINVAL, "%s: P = %d outside [1, %d]", who, P, GMPC_MAX_ENSEMBLE);
  if (!c->params_set) return fail(GMPC_EINVAL, "%s: gmpc_set_params has not been called", who);
  if (!X && !d && !D) return fail(GMPC_EINVAL, "%s: every output is null", who);
  TRY(gmpc_sampled_coverage(c, who));
  if (hipSetDevice(c->device) != hipSuccess) return fail(GMPC_EHIP, "hipSetDevice failed");
  (void)hipGetLastError();
  EnsDisArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.S = S; a.n = sh.n; a.m = sh.m;
  bind_mlp(a.dyn, sh.dyn_layers, sh.dyn_dims, dyn_members, nullptr);
  a.mstride = (size_t)mlp_count(sh.dyn_layers, sh.dyn_dims);
  for (int l = 0; l < c->dyn.L; ++l) {
    a.nom.W[l] = c->dyn.W[l];
    a.nom.b[l] = c->dyn.b[l];
  }
  a.x0 = x0; a.U = U;
  a.X = X; a.d = d; a.D = D;
  if (gmpc_launch_ens_disagreement(a, P, static_cast<hipStream_t>(stream)))
    return fail(GMPC_EINVAL, "%s: shape not covered", who);
  HIP_TRY(hipGetLastError());
  return 0;
}
