// C-ABI entry point of the ensemble rollout: a plan's trajectories and costs under every member of a
// dynamics ensemble, and the members' spread per step; of the same in closed loop around a reference trajectory
// (DESIGN §31); of the plan's one-step disagreement; of the
// rollout's VJP under every member; and of the disagreement's VJP.  Stateless; no kernel in
// this file.
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

// The ensemble rollout in closed loop: gmpc_ensemble_rollout's checks, workspace rule and two launches,
// the rollout kernel in its feedback form (k_ens_rollout_feedback).  alpha is used only with k.
extern "C" int gmpc_ensemble_rollout_feedback(gmpc_ctx* c, int B, int S, int P, const float* dyn_members,
                                              const float* x0, const float* X_ref, const float* U_ref, const float* K,
                                              const float* k, float alpha, const float* u_lo, const float* u_hi,
                                              const float* goal, float* X, float* U, float* costs, float* obj,
                                              float* x_mean, float* x_var, void* stream) {
  const char* who = "ensemble feedback";
  if (!c) return fail(GMPC_EINVAL, "%s: ctx is null", who);
  if (!dyn_members || !X_ref || !U_ref || !K)
    return fail(GMPC_EINVAL, "%s: dyn_members, X_ref, U_ref and K must not be null", who);
  if (!u_lo != !u_hi)
    return fail(GMPC_EINVAL, "%s: u_lo and u_hi must both be given or both be null (u_lo %s, u_hi %s)", who,
                u_lo ? "given" : "null", u_hi ? "given" : "null");
  if (!std::isfinite(alpha)) return fail(GMPC_EINVAL, "%s: alpha = %g is not finite", who, (double)alpha);
  const gmpc_shape& sh = c->sh;
  if (B < 1 || B > c->maxB) return fail(GMPC_EINVAL, "%s: B = %d outside [1, max_batch = %d]", who, B, c->maxB);
  if (S < 1 || S > sh.T) return fail(GMPC_EINVAL, "%s: S = %d outside [1, T = %d]", who, S, sh.T);
  if (P < 1 || P > GMPC_MAX_ENSEMBLE) return fail(GMPC_EINVAL, "%s: P = %d outside [1, %d]", who, P, GMPC_MAX_ENSEMBLE);
  if (!c->params_set) return fail(GMPC_EINVAL, "%s: gmpc_set_params has not been called", who);
  if (!X && !U && !costs && !obj && !x_mean && !x_var) return fail(GMPC_EINVAL, "%s: every output is null", who);
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
  a.x0 = x0 ? x0 : X_ref;
  a.goal = costs || obj ? goal : nullptr;     // a goal nobody costs against is not read
  a.X = planes; a.costs = costs; a.obj = obj;
  EnsFeedbackArgs f;
  memset(&f, 0, sizeof(f));
  f.X_ref = X_ref; f.U_ref = U_ref; f.K = K; f.k = k; f.alpha = alpha;
  f.u_lo = u_lo; f.u_hi = u_hi;
  f.x0_stride = x0 ? (size_t)sh.n : (size_t)(S + 1) * sh.n;
  f.U = U;
  if (gmpc_launch_ens_rollout_feedback(a, f, P, s)) return fail(GMPC_EINVAL, "%s: shape not covered", who);
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

// The VJP of the ensemble rollout and its costs.  Launches on the caller's stream: the members'
// transposes, the row pass, the sweep, the ascending-p reduce, then the weight-gradient GEMMs (mpc_w column sum and the
// cost MLP over P B rows; the dynamics member by member).  Everything it writes is the caller's or the call
// workspace's: save = the transposes [P][count], then the per-member x0 / U / goal gradients; aux = the relu masks;
// aux2 = the mpc_w terms [P B][3]; acts / dels = per member B T + GMPC_WGRAD_PAD rows (the row pass zeroes the pad
// rows); acts2 / dels2 = the cost MLP's P B rows.
extern "C" int gmpc_ensemble_rollout_vjp(gmpc_ctx* c, int B, int P, const float* dyn_members, const float* X,
                                         const float* U, const float* goal, const float* gX, const float* gcost,
                                         float* grad_x0, float* grad_U, float* grad_goal, float* grad_theta_sum,
                                         float* grad_members, void* stream) {
  const char* who = "ensemble rollout vjp";
  if (!c) return fail(GMPC_EINVAL, "%s: ctx is null", who);
  if (!dyn_members || !X || !U || !goal)
    return fail(GMPC_EINVAL, "%s: dyn_members, X, U and goal must not be null", who);
  const gmpc_shape& sh = c->sh;
  if (B < 1 || B > c->maxB) return fail(GMPC_EINVAL, "%s: B = %d outside [1, max_batch = %d]", who, B, c->maxB);
  if (P < 1 || P > GMPC_MAX_ENSEMBLE) return fail(GMPC_EINVAL, "%s: P = %d outside [1, %d]", who, P, GMPC_MAX_ENSEMBLE);
  if (!c->params_set) return fail(GMPC_EINVAL, "%s: gmpc_set_params has not been called", who);
  if (!gX && !gcost) return fail(GMPC_EINVAL, "%s: gX and gcost are both null: no cotangent", who);
  if (!grad_x0 && !grad_U && !grad_goal && !grad_theta_sum && !grad_members)
    return fail(GMPC_EINVAL, "%s: every output is null", who);
  TRY(gmpc_sampled_coverage(c, who));
  if (hipSetDevice(c->device) != hipSuccess) return fail(GMPC_EHIP, "hipSetDevice failed");
  (void)hipGetLastError();
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = sh.n, m = sh.m, T = sh.T, Lh = sh.dyn_layers - 1;
  const size_t count = (size_t)mlp_count(sh.dyn_layers, sh.dyn_dims), steps = (size_t)B * T, rows = (size_t)P * B;
  const size_t ntheta = 3 + (size_t)mlp_count(sh.cost_layers, sh.cost_dims);
  const bool want_theta = grad_theta_sum && gcost, want_goal = grad_goal && gcost;
  EnsVjpArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.T = T; a.n = n; a.m = m;
  a.dr = c->drows; a.cr = c->crows;
  a.mstride = count;
  a.rstride = (steps + GMPC_WGRAD_PAD) * a.dr.stride;
  // the call workspace
  CallWork& k = c->cw;
  const size_t plane[3] = {grad_x0 ? (size_t)B * n : 0, grad_U ? steps * m : 0,
                           want_goal ? (size_t)B * (T + 1) * n : 0};
  size_t off[4] = {(P * count + 3) & ~(size_t)3, 0, 0, 0};
  for (int i = 0; i < 3; ++i) off[i + 1] = off[i] + ((P * plane[i] + 3) & ~(size_t)3);
  TRY(k.save.grow(c, off[3]));
  if (Lh > 0) TRY(k.aux.grow(c, (size_t)P * steps * Lh * GMPC_MW));
  if (want_theta) TRY(k.aux2.grow(c, rows * 3 + 8));
  if (gcost) {
    TRY(k.acts2.reserve(c, rows, a.cr.stride, s));
    TRY(k.dels2.reserve(c, rows, a.cr.stride, s));
  }
  if (grad_members) {
    TRY(k.acts.grow(c, (size_t)P * a.rstride));
    TRY(k.dels.grow(c, (size_t)P * a.rstride));
  }
  bind_mlp(a.dyn, sh.dyn_layers, sh.dyn_dims, dyn_members, k.save.p);
  a.cost = c->cost; a.mpc_w = c->mpc_w;
  a.X = X; a.U = U; a.goal = goal; a.gX = gX; a.gc = gcost;
  a.masks = reinterpret_cast<uint32_t*>(k.aux.p);
  a.gx0 = grad_x0 ? k.save.p + off[0] : nullptr;
  a.gU = grad_U ? k.save.p + off[1] : nullptr;
  a.ggoal = want_goal ? k.save.p + off[2] : nullptr;
  a.gm = want_theta ? k.aux2.p : nullptr;
  a.acts = grad_members ? k.acts.p : nullptr;
  a.dels = grad_members ? k.dels.p : nullptr;
  a.cacts = gcost ? k.acts2.p : nullptr;
  a.cdels = gcost ? k.dels2.p : nullptr;
  gmpc_launch_dynfit_transpose(a.dyn, count, P, k.save.p, s);
  if (gmpc_launch_ens_rollout_vjp(a, P, s)) return fail(GMPC_EINVAL, "%s: shape not covered", who);
  EnsVjpReduce r;
  memset(&r, 0, sizeof(r));
  r.P = P;
  float* outs[3] = {grad_x0, grad_U, want_goal ? grad_goal : nullptr};
  for (int i = 0; i < 3; ++i) {
    r.count[i] = plane[i];
    r.planes[i] = k.save.p + off[i];
    r.out[i] = outs[i];
  }
  gmpc_launch_ens_vjp_reduce(r, s);
  // no cost cotangent: nothing reaches the goals or the costs' parameters
  if (grad_goal && !gcost) HIP_TRY(hipMemsetAsync(grad_goal, 0, (size_t)B * (T + 1) * n * sizeof(float), s));
  if (grad_theta_sum && !gcost) HIP_TRY(hipMemsetAsync(grad_theta_sum, 0, ntheta * sizeof(float), s));
  if (want_theta) {
    float* gm = k.aux2.p;
    gmpc_launch_wgrad((int)rows, 1, 3, gm, 0, gm, 3, gm + rows * 3, grad_theta_sum, (int)rows, c->wpart, s,
                      c->wpart_floats, false);
    gmpc_launch_wgrad_mlp((int)rows, (int)rows, sh.cost_layers, sh.cost_dims, k.acts2.p, k.dels2.p, a.cr,
                          grad_theta_sum + 3, c->wpart, c->wpart_floats, s);
  }
  if (grad_members)
    for (int p = 0; p < P; ++p)
      gmpc_launch_wgrad_mlp((int)steps, (int)steps, sh.dyn_layers, sh.dyn_dims, a.acts + p * a.rstride,
                            a.dels + p * a.rstride, a.dr, grad_members + p * count, c->wpart, c->wpart_floats, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The VJP of the one-step disagreement.  Launches on the caller's stream: the members' transposes; the
// local part (k_disvjp_rows, k_disvjp_back, k_disvjp_reduce); then, with grad_x0, grad_U or grad_nominal wanted, the
// chain through the nominal rollout -- §29's row pass and sweep with P = 1 on the bound dynamics under gX = rx, no cost
// cotangent -- and grad_U = ru + chain; then the weight-gradient GEMMs, the nominal's over dels = local + chain.
// Everything it writes is the caller's or the call workspace's: save = the members' transposes [P][count], the outputs
// [P+1][B T][n], the local input gradients [P+1][B T][n+m], rx, ru and the chain's dL/dU; aux = the relu masks
// [P+1][B T][L-1][GMPC_MW], plane P the nominal's (the chain's row pass writes the same bits there again); acts = the
// members' rows, then the nominal's (written by the chain's row pass); dels = the members' rows, the chain's, then the
// nominal's local ones.
extern "C" int gmpc_ensemble_disagreement_vjp(gmpc_ctx* c, int B, int P, const float* dyn_members, const float* X,
                                              const float* U, const float* gd, const float* gD, float* grad_x0,
                                              float* grad_U, float* grad_nominal, float* grad_members, void* stream) {
  const char* who = "ensemble disagreement vjp";
  if (!c) return fail(GMPC_EINVAL, "%s: ctx is null", who);
  if (!dyn_members || !X || !U) return fail(GMPC_EINVAL, "%s: dyn_members, X and U must not be null", who);
  const gmpc_shape& sh = c->sh;
  if (B < 1 || B > c->maxB) return fail(GMPC_EINVAL, "%s: B = %d outside [1, max_batch = %d]", who, B, c->maxB);
  if (P < 1 || P > GMPC_MAX_ENSEMBLE) return fail(GMPC_EINVAL, "%s: P = %d outside [1, %d]", who, P, GMPC_MAX_ENSEMBLE);
  if (!c->params_set) return fail(GMPC_EINVAL, "%s: gmpc_set_params has not been called", who);
  if (!gd && !gD) return fail(GMPC_EINVAL, "%s: gd and gD are both null: no cotangent", who);
  if (!grad_x0 && !grad_U && !grad_nominal && !grad_members) return fail(GMPC_EINVAL, "%s: every output is null", who);
  TRY(gmpc_sampled_coverage(c, who));
  if (hipSetDevice(c->device) != hipSuccess) return fail(GMPC_EHIP, "hipSetDevice failed");
  (void)hipGetLastError();
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = sh.n, m = sh.m, T = sh.T, Lh = sh.dyn_layers - 1;
  const size_t count = (size_t)mlp_count(sh.dyn_layers, sh.dyn_dims), steps = (size_t)B * T;
  const bool chain = grad_x0 || grad_U || grad_nominal;
  DisVjpArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.T = T; a.n = n; a.m = m; a.P = P;
  a.dr = c->drows;
  a.mstride = count;
  a.rstride = (steps + GMPC_WGRAD_PAD) * a.dr.stride;
  // the call workspace
  CallWork& k = c->cw;
  const size_t part[6] = {P * count, (P + 1) * steps * n, (P + 1) * steps * (n + m), (size_t)B * (T + 1) * n,
                          steps * m, steps * m};
  size_t off[7] = {0};
  for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + ((part[i] + 3) & ~(size_t)3);
  TRY(k.save.grow(c, off[6]));
  if (Lh > 0) TRY(k.aux.grow(c, (size_t)(P + 1) * steps * Lh * GMPC_MW));
  if (grad_members || grad_nominal) {
    TRY(k.acts.grow(c, (size_t)(P + 1) * a.rstride));
    TRY(k.dels.grow(c, (size_t)(P + 2) * a.rstride));
  }
  bind_mlp(a.dyn, sh.dyn_layers, sh.dyn_dims, dyn_members, k.save.p);
  a.nom = c->dyn;
  a.X = X; a.U = U; a.gd = gd; a.gD = gD;
  a.masks = reinterpret_cast<uint32_t*>(k.aux.p);
  a.out = k.save.p + off[1];
  a.q = k.save.p + off[2];
  a.rx = k.save.p + off[3];
  a.ru = k.save.p + off[4];
  float* chain_gU = k.save.p + off[5];
  a.acts = grad_members ? k.acts.p : nullptr;
  a.dels = grad_members ? k.dels.p : nullptr;
  float* nom_acts = grad_nominal ? k.acts.p + (size_t)P * a.rstride : nullptr;
  float* chain_dels = grad_nominal ? k.dels.p + (size_t)P * a.rstride : nullptr;
  a.ndels = grad_nominal ? k.dels.p + (size_t)(P + 1) * a.rstride : nullptr;
  gmpc_launch_dynfit_transpose(a.dyn, count, P, k.save.p, s);
  if (gmpc_launch_dis_vjp_local(a, s)) return fail(GMPC_EINVAL, "%s: shape not covered", who);
  if (chain) {
    EnsVjpArgs v;
    memset(&v, 0, sizeof(v));
    v.B = B; v.T = T; v.n = n; v.m = m;
    v.dr = c->drows; v.cr = c->crows;
    v.mstride = count; v.rstride = a.rstride;
    v.dyn = c->dyn; v.cost = c->cost; v.mpc_w = c->mpc_w;
    v.X = X; v.U = U; v.gX = a.rx;
    v.masks = a.masks ? a.masks + (size_t)P * steps * Lh * GMPC_MW : nullptr;
    v.gx0 = grad_x0;
    v.gU = grad_U ? chain_gU : nullptr;
    v.acts = nom_acts; v.dels = chain_dels;
    if (gmpc_launch_ens_rollout_vjp(v, 1, s)) return fail(GMPC_EINVAL, "%s: shape not covered", who);
    if (grad_U) gmpc_launch_dis_vjp_add(steps, m, (size_t)m, a.ru, chain_gU, grad_U, s);
    if (grad_nominal) {
      // dels = local + chain over every layer's columns of the B T rows, then one pass of the GEMMs
      const int width = a.dr.doff[sh.dyn_layers - 1] + n;
      gmpc_launch_dis_vjp_add(steps, width, (size_t)a.dr.stride, a.ndels, chain_dels, chain_dels, s);
      gmpc_launch_wgrad_mlp((int)steps, (int)steps, sh.dyn_layers, sh.dyn_dims, nom_acts, chain_dels, a.dr,
                            grad_nominal, c->wpart, c->wpart_floats, s);
    }
  }
  if (grad_members)
    for (int p = 0; p < P; ++p)
      gmpc_launch_wgrad_mlp((int)steps, (int)steps, sh.dyn_layers, sh.dyn_dims, a.acts + p * a.rstride,
                            a.dels + p * a.rstride, a.dr, grad_members + p * count, c->wpart, c->wpart_floats, s);
  HIP_TRY(hipGetLastError());
  return 0;
}
