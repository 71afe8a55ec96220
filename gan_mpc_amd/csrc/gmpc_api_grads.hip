// C-ABI entry points of the gradients that end in weight sums: the bilevel tail and what follows it, the rollout VJP,
// the dynamics regression, the expert model.
#include "gmpc_ctx.h"

// bilevel ----------------------------------------------------------------------------------------
// a8-a11 from the loss's cotangents at the solution held by the ctx: lx = dL/dX [B][T+1][n] (never null here),
// lu = dL/dU [B][T][m] or null (a loss of X only).  Writes Bvec, H, dX and grad_sum.
static int bilevel_from_cotangents(gmpc_ctx* c, int B, const float* lx, const float* lu, float sign,
                                   float* grad_sum, hipStream_t s) {
  const gmpc_shape& sh = c->sh;
  const int n = sh.n, m = sh.m, T = sh.T;
  c->gradB = 0;
  // a8: Bvec; a9+solve: structured Hessian solve; a11: cost_vjp
  if (c->big) {
    // step-major: the loss adjoint (Bvec) and the Riccati sweep of the Hessian solve share one
    // backward pass over re-linearised steps, the tangent roll is a second, forward pass
    if (gmpc_big_backward(c->bw, B, c->dyn, c->lp, c->masks, c->Xs, c->Us, c->goals, c->mpc_w, c->QT,
                          c->qT, nullptr, c->Ks, c->ks, nullptr, nullptr, lx, c->Bvec, s,
                          c->dynl ? &c->dl : nullptr, c->dynl ? c->adjs : nullptr, lu) != 0 ||
        gmpc_big_forward_tangent(c->bw, B, c->dyn, c->lp, c->masks, c->Ks, c->ks, c->Hout, c->dX, s,
                                 c->dynl ? &c->dl : nullptr, c->Xs, c->Us) != 0)
      return fail(GMPC_EINVAL, "large-state bilevel: Jacobian kernel does not cover this shape");
  } else {
    RiccatiArgs r;
    memset(&r, 0, sizeof(r));
    r.B = B; r.n = n; r.ng = c->nx; r.m = m; r.T = T; r.mode = 1;
    r.X = c->Xs; r.U = c->Us; r.goal = c->goals; r.mpc_w = c->mpc_w; r.AB = c->AB; r.QT = c->QT;
    r.qT = c->qT; r.K = c->Ks; r.k = c->ks; r.Bvec = c->Bvec; r.Hout = c->Hout; r.dX = c->dX;
    r.clamped = c->solBox ? c->box_mask : nullptr;     // a held box solve: the solve on each step's free rows
    if (!c->dynl && gmpc_riccati_w2h_shape(r)) {
      // two waves per trajectory, products on the matrix pipe, the loss adjoint (a8) in the same sweep
      ProfScope ps(c, PROF_RICCATI, s);      // (bench.py: secondary.bilevel.kernel_ms)
      gmpc_launch_riccati_w(r, lx, lu, c->Bvec, s);
    } else {
      gmpc_launch_bvec(B, T, n, m, c->AB, lx, lu, c->Bvec, s);
      if (c->dynl) {
        // smooth dynamics: the dense Hessian the reference solves with carries lam_{t+1} . d^2 f (oracle
        // second_order_lqr); lam = the adjoints of the solve's last backward pass
        gmpc_launch_dynl_curv(B, T, T, 0, c->dl, c->Xs, c->Us, c->adjs, nullptr, c->phi, s);
        r.Phi = c->phi;
      }
      ProfScope ps(c, PROF_RICCATI, s);      // (bench.py: secondary.bilevel.kernel_ms)
      gmpc_launch_riccati(r, s);
    }
  }
  gmpc_launch_costvjp(B, T, n, m, c->cost, c->mpc_w, sign, c->Xs, c->Us, c->goals, c->nx, c->Hout, c->dX,
                      c->gmpc, c->cact, c->cdel, c->crows, s);
  // sums over the batch: mpc_w (3 columns of gmpc) and the cost layers
  gmpc_launch_wgrad(B, 1, 3, c->gmpc, 0, c->gmpc, 3, c->scratch + 512, grad_sum, B, c->wpart, s, c->wpart_floats, false);
  gmpc_launch_wgrad_mlp(2 * B, B, sh.cost_layers, sh.cost_dims, c->cact, c->cdel, c->crows, grad_sum + 3, c->wpart,
                        c->wpart_floats, s);
  c->gradB = B;   // H, dX (and Phi) now belong to the held solution: gmpc_bilevel_grad_inputs may follow
  return 0;
}

extern "C" int gmpc_bilevel_grad(gmpc_ctx* c, int B, int loss_kind, const float* desired,
                                 const float* critic, float sign, float* loss, float* grad_sum,
                                 void* stream) {
  TRY(check_call(c, B));
  if (c->solB != B) return fail(GMPC_EINVAL, "gmpc_ilqr_solve with B=%d must precede this call", B);
  if (!loss || !grad_sum) return fail(GMPC_EINVAL, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  c->gradB = 0;   // the loss below rewrites the ctx's lx
  TRY(upper_loss(c, B, loss_kind, desired, critic, loss, true, s));
  TRY(bilevel_from_cotangents(c, B, c->lx, nullptr, sign, grad_sum, s));
  HIP_TRY(hipGetLastError());
  return 0;
}

// a caller-defined upper-level loss (reference policy/optimizers.py:34-83 takes any `loss`): the caller has
// differentiated it; the kernels read its lx / lu directly.  A null lx is a loss of U only: c->lx is zeroed.
extern "C" int gmpc_bilevel_grad_cotangent(gmpc_ctx* c, int B, const float* lx, const float* lu, float sign,
                                           float* grad_sum, void* stream) {
  TRY(check_call(c, B));
  if (c->solB != B) return fail(GMPC_EINVAL, "gmpc_ilqr_solve with B=%d must precede this call", B);
  if (!grad_sum) return fail(GMPC_EINVAL, "null argument");
  if (!lx && !lu) return fail(GMPC_EINVAL, "lx and lu are both null: the loss has no cotangent");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!lx) {
    HIP_TRY(hipMemsetAsync(c->lx, 0, (size_t)B * (c->sh.T + 1) * c->sh.n * sizeof(float), s));
    lx = c->lx;
  }
  TRY(bilevel_from_cotangents(c, B, lx, lu, sign, grad_sum, s));
  HIP_TRY(hipGetLastError());
  return 0;
}

// The arguments that both calls of k_tail_adjoints share: the held solution and what the bilevel tail left
static TailAdjArgs tail_adj_args(const gmpc_ctx* c, int B, const float* lx) {
  TailAdjArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.T = c->sh.T; a.n = c->sh.n; a.ng = c->nx; a.m = c->sh.m;
  a.mpc_w = c->mpc_w; a.X = c->Xs; a.goal = c->goals; a.dX = c->dX; a.lx = lx; a.AB = c->AB; a.QT = c->QT;
  return a;
}

// dL/dx0 and dL/dgoal of the loss whose bilevel gradient the ctx has just computed (gmpc_tail_adjoints.hip): the
// implicit-function gradient through the held solution, from the H, dX (and Phi) the bilevel tail left.  Read-only
// for every other ctx buffer.
extern "C" int gmpc_bilevel_grad_inputs(gmpc_ctx* c, int B, const float* lx, float* grad_x0, float* grad_goal,
                                        void* stream) {
  TRY(check_call(c, B));
  if (c->solB != B || c->gradB != B)
    return fail(GMPC_EINVAL, "gmpc_bilevel_grad or gmpc_bilevel_grad_cotangent with B=%d on the held solution must "
                "precede this call", B);
  if (!grad_x0 && !grad_goal) return fail(GMPC_EINVAL, "grad_x0 and grad_goal are both null");
  if (grad_x0 && c->big)
    return fail(GMPC_EINVAL, "grad_x0: the step-major pipeline (n=%d > 64 or m=%d > 32) keeps no [A_t | B_t] of the "
                "solution; only grad_goal is available for this shape", c->sh.n, c->sh.m);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const gmpc_shape& sh = c->sh;
  if (!lx) lx = c->lx;
  if (grad_x0) {
    TailAdjArgs a = tail_adj_args(c, B, lx);
    a.H = c->Hout; a.Phi = c->dynl ? c->phi : nullptr; a.gx0 = grad_x0; a.ggoal = grad_goal;
    if (gmpc_launch_tail_adjoints(a, false, s) != 0)
      return fail(GMPC_EINVAL, "grad_x0: shape n=%d m=%d not covered", sh.n, sh.m);
  } else {
    gmpc_launch_goal_grad(B, sh.T, sh.n, c->nx, c->mpc_w, c->Xs, c->goals, c->dX, grad_goal, s);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// dL/dtheta_dyn of the loss whose bilevel gradient the ctx has just computed: the adjoint sweeps
// (gmpc_tail_adjoints.hip) give w = mu - nu and lam per step, the row kernel (gmpc_dyn_grads.hip) the layer inputs and
// deltas of 2 B T rows, and the weight GEMMs sum them over the batch.  Read-only for every ctx buffer but the call
// workspace and the GEMMs' shared scratch.
extern "C" int gmpc_bilevel_grad_dynamics(gmpc_ctx* c, int B, const float* lx, float* grad_dyn_sum, void* stream) {
  TRY(check_call(c, B));
  const gmpc_shape& sh = c->sh;
  if (c->dynl)
    return fail(GMPC_EINVAL, "dynamics gradient: relu-MLP dynamics only (dyn_lstm_features = %d)",
                sh.dyn_lstm_features);
  if (c->big)
    return fail(GMPC_EINVAL, "dynamics gradient: the step-major pipeline (n=%d > 64 or m=%d > 32) keeps no "
                "[A_t | B_t] of the solution; n <= 64 and m <= 32 only", sh.n, sh.m);
  if (!grad_dyn_sum) return fail(GMPC_EINVAL, "grad_dyn_sum is null");
  if (c->solB != B || c->gradB != B)
    return fail(GMPC_EINVAL, "gmpc_bilevel_grad or gmpc_bilevel_grad_cotangent with B=%d on the held solution must "
                "precede this call", B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = sh.n, m = sh.m, T = sh.T;
  if (!lx) lx = c->lx;
  const size_t steps = (size_t)B * T, rows = 2 * steps;
  CallWork& k = c->cw;     // aux, aux2: the adjoint planes w, lam
  TRY(k.aux.grow(c, steps * n));
  TRY(k.aux2.grow(c, steps * n));
  TRY(k.acts.reserve(c, rows, c->drows.stride, s));
  TRY(k.dels.reserve(c, rows, c->drows.stride, s));
  TailAdjArgs a = tail_adj_args(c, B, lx);
  a.qT = c->qT; a.w = k.aux.p; a.lam = k.aux2.p;
  gmpc_launch_tail_adjoints(a, true, s);     // (n <= 64, m <= 32: checked above)
  if (gmpc_launch_dyn_rows(B, T, n, m, c->dyn, c->Xs, c->Us, c->dX, c->Hout, k.aux.p, k.aux2.p, k.acts.p, k.dels.p,
                           c->drows, s) != 0)
    return fail(GMPC_EINVAL, "dynamics gradient: layer widths above 256");
  // gW_l = sum over the 2 B T rows of [a; -a']^T [delta(w); delta(lam)], gb_l = sum of the primal half's deltas
  gmpc_launch_wgrad_mlp((int)rows, (int)steps, sh.dyn_layers, sh.dyn_dims, k.acts.p, k.dels.p, c->drows, grad_dyn_sum,
                        c->wpart, c->wpart_floats, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The launches of gmpc_rollout_vjp for B <= max_batch checked rows (gmpc_mppi_vjp runs them on its sample rows too)
static int rollout_vjp_rows(gmpc_ctx* c, int B, const float* X, const float* U, const float* goal, const float* gX,
                            const float* gcost, float* grad_x0, float* grad_U, float* grad_goal,
                            float* grad_theta_sum, float* grad_dyn_sum, hipStream_t s) {
  const gmpc_shape& sh = c->sh;
  const int n = sh.n, m = sh.m, T = sh.T, Lh = sh.dyn_layers - 1;
  const size_t steps = (size_t)B * T;
  const bool want_theta = grad_theta_sum != nullptr && gcost != nullptr;
  CallWork& k = c->cw;     // acts / dels: the dynamics rows, acts2 / dels2: the cost rows
  // aux: the call's own relu masks (uint32 words in a float allocation)
  TRY(k.aux.grow(c, steps * Lh * GMPC_MW));
  if (want_theta) {
    // aux2: the per-trajectory mpc_w terms [B][3] and the 1 x 3 product their column sum's launch leaves behind
    TRY(k.aux2.grow(c, (size_t)B * 3 + 8));
    TRY(k.acts2.reserve(c, B, c->crows.stride, s));
    TRY(k.dels2.reserve(c, B, c->crows.stride, s));
  }
  if (grad_dyn_sum) {
    TRY(k.acts.reserve(c, steps, c->drows.stride, s));
    TRY(k.dels.reserve(c, steps, c->drows.stride, s));
  }
  uint32_t* masks = reinterpret_cast<uint32_t*>(k.aux.p);
  float* gm = k.aux2.p;
  if (grad_dyn_sum)
    gmpc_launch_rvjp_acts(B, n, m, T, c->dyn, X, U, k.acts.p, c->drows, masks, s);
  else
    gmpc_launch_masks(B, n, m, T, c->dyn, X, U, masks, s);
  gmpc_launch_rvjp_sweep(B, n, m, T, c->dyn, c->cost, c->mpc_w, X, U, goal, gX, gcost, masks, grad_x0, grad_U,
                         grad_goal, want_theta ? gm : nullptr, want_theta ? k.acts2.p : nullptr,
                         want_theta ? k.dels2.p : nullptr, grad_dyn_sum ? k.dels.p : nullptr, c->drows, c->crows, s);
  if (grad_theta_sum && !want_theta) {
    // no cost cotangent: the costs' parameters get nothing
    HIP_TRY(hipMemsetAsync(grad_theta_sum, 0, (3 + (size_t)mlp_count(sh.cost_layers, sh.cost_dims)) * sizeof(float),
                           s));
  } else if (want_theta) {
    gmpc_launch_wgrad(B, 1, 3, gm, 0, gm, 3, gm + (size_t)B * 3, grad_theta_sum, B, c->wpart, s, c->wpart_floats,
                      false);
    gmpc_launch_wgrad_mlp(B, B, sh.cost_layers, sh.cost_dims, k.acts2.p, k.dels2.p, c->crows, grad_theta_sum + 3,
                          c->wpart, c->wpart_floats, s);
  }
  if (grad_dyn_sum)
    gmpc_launch_wgrad_mlp((int)steps, (int)steps, sh.dyn_layers, sh.dyn_dims, k.acts.p, k.dels.p, c->drows,
                          grad_dyn_sum, c->wpart, c->wpart_floats, s);
  return 0;
}

// The VJP of the rollout and its costs at (X, U, goal) (gmpc_rollout_vjp.hip).  Stateless: the masks and rows live in
// the call workspace, no held solution is dropped; the GEMMs' partials use the shared scratch.
extern "C" int gmpc_rollout_vjp(gmpc_ctx* c, int B, const float* X, const float* U, const float* goal, const float* gX,
                                const float* gcost, float* grad_x0, float* grad_U, float* grad_goal,
                                float* grad_theta_sum, float* grad_dyn_sum, void* stream) {
  TRY(check_call(c, B));
  const gmpc_shape& sh = c->sh;
  if (c->dynl)
    return fail(GMPC_EINVAL, "rollout vjp: relu-MLP dynamics only (dyn_lstm_features = %d)", sh.dyn_lstm_features);
  if (!X || !U || !goal) return fail(GMPC_EINVAL, "rollout vjp: X, U and goal must not be null");
  if (!gX && !gcost) return fail(GMPC_EINVAL, "rollout vjp: gX and gcost are both null: no cotangent");
  if (!grad_x0 && !grad_U && !grad_goal && !grad_theta_sum && !grad_dyn_sum)
    return fail(GMPC_EINVAL, "rollout vjp: every output is null");
  TRY(rollout_vjp_rows(c, B, X, U, goal, gX, gcost, grad_x0, grad_U, grad_goal, grad_theta_sum, grad_dyn_sum,
                       static_cast<hipStream_t>(stream)));
  HIP_TRY(hipGetLastError());
  return 0;
}

// The VJP of gmpc_mppi_solve: the adjoint of the weighted-mean recursion, last iteration first.  Per
// iteration and chunk of floor(max_batch / N) problems: k_mppi_cotangent lays the samples out as rows, the rollout
// kernel gives their states, rollout_vjp_rows the heavy VJP under one cost cotangent per sample, k_mppi_reduce the
// masked sums.  The rollout writes the ctx's masks and objectives: a held solution is dropped.
extern "C" int gmpc_mppi_vjp(gmpc_ctx* c, int B, const float* x0, const float* goal, const float* u_lo,
                             const float* u_hi, const gmpc_mppi_opts* o, const float* std, const float* means_trace,
                             const float* costs_trace, const float* U, const float* X, const float* gU,
                             const float* gX, const float* gobj, float* grad_x0, float* grad_Uinit, float* grad_goal,
                             float* grad_theta_sum, float* grad_dyn_sum, void* stream) {
  TRY(check_call(c, B));
  const gmpc_shape& sh = c->sh;
  TRY(gmpc_sampled_coverage(c, "mppi"));
  // the derivative of the fp32 solve: its rows are re-rolled in fp32, which a bf16-mode forward pass did not see
  if (c->sampled_precision != GMPC_SAMPLED_FP32) return fail(GMPC_EINVAL, "mppi vjp: fp32 sampled rollouts only");
  // ... and of the nominal model's costs: under an ensemble the forward pass weighted the samples by other costs
  if (c->ens_P > 0) return fail(GMPC_EINVAL, "mppi vjp: not while a sampled ensemble is set (nominal dynamics only)");
  TRY(gmpc_mppi_check_opts(o));
  if (!x0 || !goal || !std || !U || !X) return fail(GMPC_EINVAL, "mppi: x0, goal, std, U and X must not be null");
  if (o->max_iter > 0 && (!means_trace || !costs_trace))
    return fail(GMPC_EINVAL, "mppi: the vjp needs means_trace and costs_trace of the forward call");
  if (!gU && !gX && !gobj) return fail(GMPC_EINVAL, "mppi: gU, gX and gobj are all null: no cotangent");
  if (!grad_x0 && !grad_Uinit && !grad_goal && !grad_theta_sum && !grad_dyn_sum)
    return fail(GMPC_EINVAL, "mppi: every output is null");
  const int N = o->num_samples;
  if (N > c->maxB)
    return fail(GMPC_EINVAL, "mppi: num_samples = %d above max_batch = %d (the vjp's rows are samples)", N, c->maxB);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = sh.n, m = sh.m, T = sh.T, K = o->max_iter;
  const int chunk = c->maxB / N < B ? c->maxB / N : B;     // problems per chunk
  const size_t R = (size_t)chunk * N, Tm = (size_t)T * m, Tn = (size_t)(T + 1) * n;
  const size_t ntheta = 3 + (size_t)mlp_count(sh.cost_layers, sh.cost_dims);
  const size_t ndyn = (size_t)mlp_count(sh.dyn_layers, sh.dyn_dims);
  // the call's workspace, behind what rollout_vjp_rows reserves for itself
  const size_t sizes[] = {R * Tm, R * Tn, R * Tn, R * n, R * (T + 1), R * Tm, R * n, R * Tn, R, chunk * Tm,
                          ntheta, ndyn, B * Tm, (size_t)B * (T + 1)};
  size_t total = 0;
  for (size_t v : sizes) total += (v + 3) & ~(size_t)3;
  TRY(c->cw.save.grow(c, total));
  float* wp[sizeof(sizes) / sizeof(sizes[0])];
  {
    float* p = c->cw.save.p;
    for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) { wp[i] = p; p += (sizes[i] + 3) & ~(size_t)3; }
  }
  float *Us = wp[0], *Xr = wp[1], *goalr = wp[2], *x0r = wp[3], *gc = wp[4], *GU = wp[5], *Gx0 = wp[6],
        *Ggoal = wp[7], *wn = wp[8], *nm = wp[9], *th_tmp = wp[10], *dyn_tmp = wp[11], *gbuf = wp[12], *gcB = wp[13];
  float* g = grad_Uinit ? grad_Uinit : gbuf;
  c->solB = 0;     // the sample rollouts overwrite the ctx's relu masks and objectives: any held solution is gone
  c->gradB = 0;
  if (grad_theta_sum) HIP_TRY(hipMemsetAsync(grad_theta_sum, 0, ntheta * sizeof(float), s));
  if (grad_dyn_sum) HIP_TRY(hipMemsetAsync(grad_dyn_sum, 0, ndyn * sizeof(float), s));
  // ---- the final mean's rollout under gX and gobj (broadcast over the T + 1 costs)
  if (gX || gobj) {
    if (gobj) gmpc_launch_mppi_bcast(B, T + 1, gobj, gcB, s);
    TRY(rollout_vjp_rows(c, B, X, U, goal, gX, gobj ? gcB : nullptr, grad_x0, g, grad_goal,
                         grad_theta_sum ? th_tmp : nullptr, grad_dyn_sum ? dyn_tmp : nullptr, s));
    if (gU) gmpc_launch_mppi_add((long)(B * Tm), gU, g, s);
    if (grad_theta_sum) gmpc_launch_mppi_add((long)ntheta, th_tmp, grad_theta_sum, s);
    if (grad_dyn_sum) gmpc_launch_mppi_add((long)ndyn, dyn_tmp, grad_dyn_sum, s);
  } else {
    HIP_TRY(hipMemcpyAsync(g, gU, B * Tm * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (grad_x0) HIP_TRY(hipMemsetAsync(grad_x0, 0, (size_t)B * n * sizeof(float), s));
    if (grad_goal) HIP_TRY(hipMemsetAsync(grad_goal, 0, B * Tn * sizeof(float), s));
  }
  // ---- the iterations, last first
  MppiCotArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.N = N; ca.T = T; ca.n = n; ca.m = m;
  ca.sd = std; ca.lo = u_lo; ca.hi = u_hi; ca.g = g; ca.x0 = x0; ca.goal = goal;
  ca.gamma = o->evolution_smoothing; ca.lam = o->temperature;
  ca.Us = Us; ca.gc = gc; ca.x0r = x0r; ca.goalr = goalr; ca.wn = wn; ca.nm = nm;
  MppiRedArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.N = N; ra.T = T; ra.n = n; ra.m = m;
  ra.lo = u_lo; ra.hi = u_hi; ra.wn = wn; ra.Us = Us; ra.GU = GU; ra.Gx0 = Gx0; ra.Ggoal = Ggoal;
  ra.gamma = o->evolution_smoothing; ra.g = g; ra.gx0 = grad_x0; ra.ggoal = grad_goal;
  TrajArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.n = n; ta.m = m; ta.T = T; ta.dyn = c->dyn; ta.cost = c->cost; ta.mpc_w = c->mpc_w;
  ta.goal = goalr; ta.x0 = x0r; ta.U = Us; ta.X = Xr; ta.obj = c->obj; ta.masks = c->masks;
  for (int k = K - 1; k >= 0; --k) {
    ca.rng = gmpc_sampled_rng(o->seed, o->iter_offset + k, o->sampling_smoothing);
    ca.mean = means_trace + (size_t)k * B * Tm;
    ca.costs = costs_trace + (size_t)k * B * N;
    for (int b0 = 0; b0 < B; b0 += chunk) {
      const int Bc = B - b0 < chunk ? B - b0 : chunk, rows = Bc * N;
      ca.b0 = ra.b0 = b0; ca.Bc = ra.Bc = Bc;
      if (gmpc_launch_mppi_cotangent(ca, s)) return fail(GMPC_EINVAL, "mppi: shape not covered");
      ta.B = rows;
      gmpc_launch_rollout(ta, s);
      TRY(rollout_vjp_rows(c, rows, Xr, Us, goalr, nullptr, gc, grad_x0 ? Gx0 : nullptr, GU,
                           grad_goal ? Ggoal : nullptr, grad_theta_sum ? th_tmp : nullptr,
                           grad_dyn_sum ? dyn_tmp : nullptr, s));
      gmpc_launch_mppi_reduce(ra, s);
      if (grad_theta_sum) gmpc_launch_mppi_add((long)ntheta, th_tmp, grad_theta_sum, s);
      if (grad_dyn_sum) gmpc_launch_mppi_add((long)ndyn, dyn_tmp, grad_dyn_sum, s);
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// dynamics regression (N3) ---------------------------------------------------------------------
extern "C" int gmpc_dynamics_loss_grad(gmpc_ctx* c, int B, int S, const float* xseq, const float* useq,
                                       const float* next_xseq, double discount, int teacher_forcing,
                                       float* loss_sum, float* grad_sum, void* stream) {
  TRY(check_call(c, B));
  const gmpc_shape& sh = c->sh;
  if (S < 1 || S > sh.T) return fail(GMPC_EINVAL, "S=%d outside [1, T=%d]", S, sh.T);
  if (!xseq || !useq || !next_xseq || !loss_sum || !grad_sum) return fail(GMPC_EINVAL, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!c->dfacts) {
    // (zeroed whole, once: the pad rows of the weight-gradient GEMM's operands stay finite whatever B * S a call has)
    const size_t rows = (size_t)c->maxB * sh.T, padded = rows + GMPC_WGRAD_PAD;
    c->dfstride = c->dynl ? (int)gmpc_dynl_fit_stride(c->dl) : c->drows.stride;
    int rc = dalloc(c, &c->dfpred, rows * c->nx);
    if (!rc) rc = dalloc(c, &c->dfacts, padded * c->dfstride);
    if (!rc) rc = dalloc(c, &c->dfdels, padded * c->dfstride);
    if (!rc && c->dynl) rc = dalloc(c, &c->dfsave, rows * 6 * c->dl.F);
    if (!rc) rc = dalloc(c, &c->dfloss, c->maxB);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->dfacts, 0, padded * c->dfstride * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(c->dfdels, 0, padded * c->dfstride * sizeof(float), s));
  }
  const int rows = B * S;
  if (c->dynl) {
    // LSTM variant: BPTT through the cell and the tail (gmpc_dynl.hip); gradient layout Wx | Wh | b | tail
    const DynlDesc& d = c->dl;
    const long Fd = d.F, kin = d.nx + d.m, G4 = 4 * Fd;
    MlpRows tail = c->drows;     // the tail's columns, in rows that start with the cell's
    tail.stride = c->dfstride;
    gmpc_launch_dynl_fit(B, S, d, xseq, useq, next_xseq, (float)discount, teacher_forcing != 0, c->dfpred,
                         c->dfacts, c->dfdels, tail, c->dfsave, c->dfloss, s);
    float* gWx = grad_sum;
    float* gWh = gWx + kin * G4;
    float* gb = gWh + Fd * G4;
    gmpc_launch_wgrad(rows, (int)kin, (int)G4, c->dfacts, c->dfstride, c->dfdels, c->dfstride, gWx, nullptr, 0,
                      c->wpart, s, c->wpart_floats, true);
    gmpc_launch_wgrad(rows, (int)Fd, (int)G4, c->dfacts + kin, c->dfstride, c->dfdels, c->dfstride, gWh, gb, rows,
                      c->wpart, s, c->wpart_floats, true);
    gmpc_launch_wgrad_mlp(rows, rows, d.tail.L, d.tail.dims, c->dfacts + kin + Fd, c->dfdels + G4, tail,
                          gb + G4, c->wpart, c->wpart_floats, s);
  } else {
    if (gmpc_launch_dynfit(B, S, sh.n, sh.m, c->dyn, xseq, useq, next_xseq, (float)discount,
                           teacher_forcing != 0, c->dfpred, c->dfacts, c->dfdels, c->drows, c->dfloss,
                           s) != 0)
      return fail(GMPC_EINVAL, "dynamics regression: unsupported layer width");
    gmpc_launch_wgrad_mlp(rows, rows, sh.dyn_layers, sh.dyn_dims, c->dfacts, c->dfdels, c->drows, grad_sum,
                          c->wpart, c->wpart_floats, s);
  }
  gmpc_launch_sum(B, c->dfloss, loss_sum, 0, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The same regression for the P members of an ensemble: the members' transposes, k_dynfit_rows over the
// grid (tiles of 32 sequences, members), the loss sums, then the weight-gradient GEMMs member by member.  Everything it
// writes is the caller's or the call workspace's: save = the transposes [P][count], aux = the losses [P][B], acts /
// dels = per member B S + GMPC_WGRAD_PAD rows (the kernel zeroes the pad rows).
extern "C" int gmpc_dynamics_ensemble_loss_grad(gmpc_ctx* c, int P, const float* dyn_members, int D, int B, int S,
                                                const float* xseq, const float* useq, const float* next_xseq,
                                                const int* rows, double discount, int teacher_forcing,
                                                float* loss_sum, float* grad_sum, void* stream) {
  if (!c) return fail(GMPC_EINVAL, "ensemble fit: ctx is null");
  const gmpc_shape& sh = c->sh;
  if (P < 1 || P > GMPC_MAX_ENSEMBLE)
    return fail(GMPC_EINVAL, "ensemble fit: P = %d outside [1, %d]", P, GMPC_MAX_ENSEMBLE);
  if (B < 1 || B > c->maxB) return fail(GMPC_EINVAL, "ensemble fit: B = %d outside [1, max_batch = %d]", B, c->maxB);
  if (S < 1 || S > sh.T) return fail(GMPC_EINVAL, "ensemble fit: S = %d outside [1, T = %d]", S, sh.T);
  if (D < 1) return fail(GMPC_EINVAL, "ensemble fit: D = %d dataset rows", D);
  if (!rows && D != B) return fail(GMPC_EINVAL, "ensemble fit: D = %d is not B = %d and rows is null", D, B);
  if (!dyn_members || !xseq || !useq || !next_xseq || !loss_sum || !grad_sum)
    return fail(GMPC_EINVAL, "ensemble fit: null argument");
  TRY(gmpc_sampled_coverage(c, "ensemble fit"));
  if (hipSetDevice(c->device) != hipSuccess) return fail(GMPC_EHIP, "hipSetDevice failed");
  (void)hipGetLastError();
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t count = (size_t)mlp_count(sh.dyn_layers, sh.dyn_dims), steps = (size_t)B * S;
  DynFitRowsArgs a;
  memset(&a, 0, sizeof(a));
  a.lay = mlp_rows(sh.dyn_layers, sh.dyn_dims);
  a.mstride = count;
  a.rstride = (steps + GMPC_WGRAD_PAD) * a.lay.stride;
  CallWork& k = c->cw;
  TRY(k.save.grow(c, (size_t)P * count));
  TRY(k.aux.grow(c, (size_t)P * B));
  TRY(k.acts.grow(c, (size_t)P * a.rstride));
  TRY(k.dels.grow(c, (size_t)P * a.rstride));
  bind_mlp(a.dyn, sh.dyn_layers, sh.dyn_dims, dyn_members, k.save.p);
  a.B = B; a.S = S; a.n = sh.n; a.m = sh.m;
  a.xseq = xseq; a.useq = useq; a.yseq = next_xseq; a.rows = rows;
  a.gamma = (float)discount; a.teacher_forcing = teacher_forcing != 0;
  a.acts = k.acts.p; a.dels = k.dels.p; a.loss = k.aux.p;
  if (gmpc_launch_dynfit_rows(a, P, k.save.p, loss_sum, s) != 0)
    return fail(GMPC_EINVAL, "ensemble fit: S = %d discounts do not fit the workgroup's LDS", S);
  for (int p = 0; p < P; ++p)
    gmpc_launch_wgrad_mlp((int)steps, (int)steps, sh.dyn_layers, sh.dyn_dims, a.acts + p * a.rstride,
                          a.dels + p * a.rstride, a.lay, grad_sum + p * count, c->wpart, c->wpart_floats, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

// expert sequence model (N2) --------------------------------------------------------------------

static int check_expert_shape(const gmpc_expert_shape* es, int n, int m) {
  if (!es) return fail(GMPC_EINVAL, "expert shape is null");
  if (es->head_layers < 1 || es->head_layers > GMPC_MAX_LAYERS)
    return fail(GMPC_EINVAL, "expert head_layers=%d outside [1, %d]", es->head_layers, GMPC_MAX_LAYERS);
  if (es->lstm_features < 0 || es->lstm_features > 128)
    return fail(GMPC_EINVAL, "expert lstm_features=%d outside [0, 128]", es->lstm_features);
  const int L = es->head_layers;
  if (es->head_dims_x[L] != n || es->head_dims_u[L] != m)
    return fail(GMPC_EINVAL, "expert heads must end in n=%d and m=%d", n, m);
  if (es->head_dims_x[0] != es->head_dims_u[0] ||
      (es->lstm_features > 0 && es->head_dims_x[0] != es->lstm_features))
    return fail(GMPC_EINVAL, "expert heads must start at the width of y");
  for (int l = 0; l <= L; ++l)
    if (es->head_dims_x[l] < 1 || es->head_dims_x[l] > 1024 || es->head_dims_u[l] < 1 ||
        es->head_dims_u[l] > 1024)
      return fail(GMPC_EINVAL, "expert head widths must be in [1, 1024]");
  return 0;
}

extern "C" long gmpc_expert_param_count(int n, const gmpc_expert_shape* es) {
  if (!es || es->head_layers < 1 || es->head_layers > GMPC_MAX_LAYERS) return -1;
  const long F = es->lstm_features, h = es->head_dims_x[0];
  long cnt = F > 0 ? (n + F) * 4 * F + 4 * F : (long)n * h + h;
  return cnt + mlp_count(es->head_layers, es->head_dims_x) + mlp_count(es->head_layers, es->head_dims_u);
}

// The expert's weight gradient in the flat layout: the first matrix ([Wx; Wh] or W_first) and its bias over `rows`
// rows, then head_x's and head_u's layers over `head_rows` rows (k_expert_vjp has head deltas on its last rows only).
static void expert_wgrad(gmpc_ctx* c, const ExpertNet& e, const float* acts, const float* dels, int rows,
                         const float* head_acts, const float* head_dels, int head_rows, float* g, hipStream_t s) {
  const int M0 = e.n + e.F, N0 = e.F > 0 ? 4 * e.F : e.Y;
  gmpc_launch_wgrad(rows, M0, N0, acts, e.stride, dels, e.stride, g, g + (long)M0 * N0, rows, c->wpart, s,
                    c->wpart_floats, true);
  g += (long)M0 * N0 + N0;
  for (int h = 0; h < 2; ++h) {
    const MlpDesc& d = h == 0 ? e.hx : e.hu;
    const int* ao = h == 0 ? e.ax : e.au;
    const int* dof = h == 0 ? e.dx : e.du;
    for (int l = 0; l < d.L; ++l) {
      const int M = d.dims[l], N = d.dims[l + 1];
      gmpc_launch_wgrad(head_rows, M, N, head_acts + ao[l], e.stride, head_dels + dof[l], e.stride, g, g + (long)M * N,
                        head_rows, c->wpart, s, c->wpart_floats, true);
      g += (long)M * N + N;
    }
  }
}

extern "C" int gmpc_expert_rollout(gmpc_ctx* c, int B, int hist, const gmpc_expert_shape* es,
                                   const float* expert, const float* history, float* goal, float* init_U,
                                   void* stream) {
  TRY(check_call(c, B, false));     // the expert model has its own parameters
  const gmpc_shape& sh = c->sh;
  const int nx = c->nx;     // the expert model predicts x sequences (goals have x_size columns)
  TRY(check_expert_shape(es, nx, sh.m));
  if (hist < 1) return fail(GMPC_EINVAL, "hist=%d: at least one history row is needed (yaml: history >= 1)", hist);
  if (!expert || !history || !goal || !init_U) return fail(GMPC_EINVAL, "null argument");
  ExpertArgs a{};
  a.B = B; a.T = sh.T; a.hist = hist;
  bind_expert(a.net, nx, sh.m, es, expert, nullptr);
  a.history = history; a.goal = goal; a.U = init_U;
  if (gmpc_launch_expert(a, static_cast<hipStream_t>(stream)) != 0)
    return fail(GMPC_EINVAL, "expert kernel: unsupported shape");
  HIP_TRY(hipGetLastError());
  return 0;
}

// expert model training --------------------------------------------------------------------------

extern "C" int gmpc_expert_loss_grad(gmpc_ctx* c, int B, int S, const gmpc_expert_shape* es, const float* expert,
                                     const float* xseq, const float* useq, const float* next_xseq, double discount,
                                     int teacher_forcing, float* loss_sum, float* grad_sum, void* stream) {
  TRY(check_call(c, B, false));     // the expert model has its own parameters
  const int nx = c->nx, m = c->sh.m;
  TRY(check_expert_shape(es, nx, m));
  if (S < 1) return fail(GMPC_EINVAL, "S=%d: at least one step is needed", S);
  if ((long)B * S > (1L << 30)) return fail(GMPC_EINVAL, "B*S=%ld rows: too many", (long)B * S);
  if (es->lstm_features == 0 && es->head_dims_x[0] > 512)
    return fail(GMPC_EINVAL, "expert MLP first width %d > 512", es->head_dims_x[0]);
  if (!expert || !xseq || !useq || !next_xseq || !loss_sum) return fail(GMPC_EINVAL, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ExpertFitArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.S = S;
  bind_expert(a.net, nx, m, es, expert, nullptr);
  a.xseq = xseq; a.useq = useq; a.yseq = next_xseq;
  a.gamma = (float)discount;
  a.teacher_forcing = teacher_forcing != 0;
  a.grad = grad_sum != nullptr;
  a.sstride = (a.net.F > 0 ? 6 * a.net.F : 0) + nx + m;
  const size_t rows = (size_t)B * S;
  if (!c->efloss) TRY(dalloc(c, &c->efloss, c->maxB));
  a.loss = c->efloss;
  if (a.grad) {
    CallWork& k = c->cw;
    TRY(k.acts.reserve(c, rows, a.net.stride, s));
    TRY(k.dels.reserve(c, rows, a.net.stride, s));
    TRY(k.save.grow(c, rows * a.sstride));
    a.acts = k.acts.p; a.dels = k.dels.p; a.save = k.save.p;
  }
  gmpc_launch_expert_fit(a, s);
  if (a.grad) expert_wgrad(c, a.net, a.acts, a.dels, (int)rows, a.acts, a.dels, (int)rows, grad_sum, s);
  gmpc_launch_sum(B, c->efloss, loss_sum, 0, s);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The VJP of gmpc_expert_rollout at (expert, history) (gmpc_expert_vjp.hip).  Stateless: rows, save rows and the
// transposed weight copies live in the call workspace, no held solution is dropped; the GEMMs' partials use
// the shared scratch.
extern "C" int gmpc_expert_vjp(gmpc_ctx* c, int B, int hist, const gmpc_expert_shape* es, const float* expert,
                               const float* history, const float* g_goal, const float* g_U, float* grad_expert_sum,
                               float* grad_history, void* stream) {
  TRY(check_call(c, B, false));     // the expert model has its own parameters
  const int nx = c->nx, m = c->sh.m, T = c->sh.T;
  TRY(check_expert_shape(es, nx, m));
  if (hist < 1) return fail(GMPC_EINVAL, "hist=%d: at least one history row is needed (yaml: history >= 1)", hist);
  if (es->lstm_features == 0 && es->head_dims_x[0] > 512)
    return fail(GMPC_EINVAL, "expert MLP first width %d > 512", es->head_dims_x[0]);
  if (!expert || !history) return fail(GMPC_EINVAL, "expert vjp: expert and history must not be null");
  if (!g_goal && !g_U) return fail(GMPC_EINVAL, "expert vjp: g_goal and g_U are both null: no cotangent");
  if (!grad_expert_sum && !grad_history) return fail(GMPC_EINVAL, "expert vjp: every output is null");
  if ((long)B * (hist + T) > (1L << 30)) return fail(GMPC_EINVAL, "B*(hist+T)=%ld rows: too many", (long)B * (hist + T));
  hipStream_t s = static_cast<hipStream_t>(stream);
  CallWork& k = c->cw;     // aux: each matrix's transposed copy at the matrix's own offset
  TRY(k.aux.grow(c, (size_t)gmpc_expert_param_count(nx, es)));
  ExpertVjpArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.T = T; a.hist = hist;
  bind_expert(a.net, nx, m, es, expert, k.aux.p);
  a.st0 = a.net.F > 0 ? 0 : hist;
  a.sstride = (a.net.F > 0 ? 6 * a.net.F : 0) + m;
  const size_t rows = (size_t)B * (hist + T - a.st0), head0 = (size_t)B * (hist - a.st0), stride = (size_t)a.net.stride;
  TRY(k.acts.reserve(c, rows, stride, s));
  if (grad_expert_sum) TRY(k.dels.reserve(c, rows, stride, s));
  TRY(k.save.grow(c, gmpc_expert_vjp_save_floats(a)));
  a.history = history; a.g_goal = g_goal; a.g_U = g_U;
  a.acts = k.acts.p;
  a.dels = grad_expert_sum ? k.dels.p : nullptr;
  a.save = reinterpret_cast<float4*>(k.save.p);
  a.grad_history = grad_history;
  if (gmpc_launch_expert_vjp(a, s) != 0) return fail(GMPC_EINVAL, "expert vjp kernel: unsupported shape");
  // [Wx | Wh] (or W_first) over every row the kernel ran; the heads over the rows with head deltas (st >= hist) only
  if (grad_expert_sum)
    expert_wgrad(c, a.net, a.acts, a.dels, (int)rows, a.acts + head0 * stride, a.dels + head0 * stride, B * T,
                 grad_expert_sum, s);
  HIP_TRY(hipGetLastError());
  return 0;
}
