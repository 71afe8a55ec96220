// C-ABI entry points of the lower level: rollout, backward pass, the iLQR solves, single model evaluations.
#include "gmpc_ctx.h"
#include "gmpc_fused_solve.h"

static TrajArgs base_traj(gmpc_ctx* c, int B, const float* goal) {
  TrajArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.n = c->sh.n; a.m = c->sh.m; a.T = c->sh.T;
  a.dyn = c->dyn; a.cost = c->cost; a.mpc_w = c->mpc_w; a.goal = goal;
  return a;
}

static DynlTrajArgs base_dynl(gmpc_ctx* c, int B, const float* goal) {
  DynlTrajArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.T = c->sh.T; a.d = c->dl; a.cost = c->cost; a.mpc_w = c->mpc_w; a.goal = goal;
  return a;
}

extern "C" int gmpc_rollout_cost(gmpc_ctx* c, int B, const float* x0, const float* U,
                                 const float* goal, float* X, float* costs, void* stream) {
  TRY(check_call(c, B));
  if (!x0 || !U || !goal || !X) return fail(GMPC_EINVAL, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  c->solB = 0;   // overwrites the ctx's relu masks and objectives: any held solution is gone
  c->gradB = 0;
  if (c->dynl) {
    DynlTrajArgs d = base_dynl(c, B, goal);
    d.x0 = x0; d.U = U; d.X = X; d.costs = costs; d.obj = c->obj;
    {
      ProfScope ps(c, PROF_ROLLOUT, s);
      gmpc_launch_dynl_rollout(d, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
  }
  TrajArgs a = base_traj(c, B, goal);
  a.x0 = x0; a.U = U; a.X = X; a.costs = costs; a.obj = c->obj; a.masks = c->masks;
  {
    ProfScope ps(c, PROF_ROLLOUT, s);
    gmpc_launch_rollout(a, s);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// linearise + terminal quadratisation + Riccati/adjoint sweep on (X, U)
static int backward_pass(gmpc_ctx* c, int B, const float* X, const float* U, const float* goal,
                         const int* active, float* K, float* k, float* grad, float* adj, float* AB,
                         int* cont, const gmpc_ilqr_opts* opts, hipStream_t s) {
  const gmpc_shape& sh = c->sh;
  if (c->big) {
    if (c->lin_event) HIP_TRY(hipEventRecord(c->lin_event, s));
    // large state: terminal quadratisation, then the step-major MFMA pipeline (gmpc_large.hip)
    if (gmpc_launch_terminal(B, sh.T, sh.n, c->cost, c->mpc_w, X, active, c->QT, c->qT, s) != 0)
      return fail(GMPC_EINVAL, "terminal: unsupported fout");
    HIP_TRY(hipGetLastError());
    {
      ProfScope ps(c, PROF_RICCATI, s);
      // the gains feed the GEMMs as a padded operand: always build them in the ctx buffer
      if (gmpc_big_backward(c->bw, B, c->dyn, c->lp, c->masks, X, U, goal, c->mpc_w, c->QT, c->qT, active,
                            c->Ks, k, grad ? grad : c->grads, adj ? adj : c->adjs, nullptr, nullptr, s,
                            c->dynl ? &c->dl : nullptr) != 0)
        return fail(GMPC_EINVAL, "large-state backward: Jacobian kernel does not cover this shape");
      // (the chain every step of the pass launched: the same call of the same function as big_step_jacobians)
      set_lin_kernel(c, gmpc_linearize_family_of(true, c->bw.h, c->dynl, B, sh.n, sh.m, sh.dyn_layers, sh.dyn_dims,
                                                 true));
      if (K != c->Ks)
        HIP_TRY(hipMemcpyAsync(K, c->Ks, (size_t)B * sh.T * sh.m * sh.n * sizeof(float),
                               hipMemcpyDeviceToDevice, s));
    }
    if (cont)
      gmpc_launch_big_cont(B, sh.T, sh.m, U, c->bw.gn2, c->iters, c->obj, c->alpha, c->obj_step,
                           c->U_step, *opts, active, cont, s);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  // The terminal quadratisation needs X only: it runs BEFORE the Jacobian chain, so that the Riccati sweep is the
  // launch right behind the chain.  With the critic step on a second stream gated by lin_event, the sweep's
  // one-wave workgroups are then dispatched first and take the low end of every SIMD's register file; launched
  // 0.03 ms later (behind k_terminal) they landed BETWEEN the critic's waves, and the 272-register waves of
  // k_lstm_bwd2 found no contiguous block until the sweep had finished (0.105 -> 0.24 ms for that kernel).
  {
    ProfScope ps(c, PROF_TERMINAL, s);
    if (gmpc_launch_terminal(B, sh.T, sh.n, c->cost, c->mpc_w, X, active, c->QT, c->qT, s) != 0)
      return fail(GMPC_EINVAL, "terminal: unsupported fout");
  }
  {
    ProfScope ps(c, PROF_LINEARIZE, s);
    // matrix-core chain; the VALU chain only serves shapes the MFMA tiling does not cover -- both are HIP
    // kernels of this library
    // 1st choice: the chain over each sample's active relu units (200-wide hidden layers; bitwise the dense
    // chain's result), 2nd: register-resident dense chain (compiled for the common equal-width shapes), 3rd: the
    // LDS-operand chain (any shape), 4th: VALU.  GMPC_LIN=dense skips the first (read per call: the tests compare
    // the two routes inside one process).  The order itself is gmpc_linearize_family_of's.
    const int fam = gmpc_linearize_family_of(false, 0, c->dynl, (long)B * sh.T, sh.n, sh.m, sh.dyn_layers, sh.dyn_dims,
                                             false);
    if (fam == LIN_DYNL) {
      gmpc_launch_dynl_jac(B, sh.T, sh.T, 0, c->dl, X, U, active, AB, s);
    } else if (gmpc_launch_linearize_family(fam, B * sh.T, sh.T, sh.n, sh.m, c->dyn, c->lp, c->masks, active, AB, 1,
                                            0, s) != 0) {
      return fail(GMPC_EINVAL, "linearize: unsupported row count for n=%d", sh.n);
    }
    set_lin_kernel(c, fam);
  }
  HIP_TRY(hipGetLastError());
  if (c->lin_event) HIP_TRY(hipEventRecord(c->lin_event, s));     // gmpc_set_linearize_event
  RiccatiArgs r;
  memset(&r, 0, sizeof(r));
  r.B = B; r.n = sh.n; r.ng = c->nx; r.m = sh.m; r.T = sh.T; r.mode = 0;
  r.X = X; r.U = U; r.goal = goal; r.mpc_w = c->mpc_w; r.AB = AB; r.QT = c->QT; r.qT = c->qT;
  r.active = active; r.K = K; r.k = k; r.grad = grad; r.adj = adj;
  if (cont) {
    r.cont = cont; r.iters = c->iters; r.obj = c->obj; r.alpha = c->alpha;
    r.obj_step = c->obj_step; r.U_step = c->U_step; r.opts = *opts;
  }
  {
    ProfScope ps(c, PROF_RICCATI, s);
    gmpc_launch_riccati(r, s);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_lqr_backward(gmpc_ctx* c, int B, const float* X, const float* U,
                                 const float* goal, float* K, float* k, float* grad,
                                 float* adjoints, float* AB, void* stream) {
  TRY(check_call(c, B));
  if (!X || !U || !goal) return fail(GMPC_EINVAL, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (c->big && AB) return fail(GMPC_EINVAL, "AB output is not materialised for n > 64 (pass NULL)");
  c->solB = 0;   // overwrites masks, QT/qT and (with NULL outputs) the ctx's K / AB
  c->gradB = 0;
  // relu masks at (X, U): recomputed so that any trajectory may be passed (the LSTM variant's Jacobian
  // kernel recomputes its forward pass itself)
  if (!c->dynl) gmpc_launch_masks(B, c->sh.n, c->sh.m, c->sh.T, c->dyn, X, U, c->masks, s);
  return backward_pass(c, B, X, U, goal, nullptr, K ? K : c->Ks, k ? k : c->ks, grad, adjoints,
                       AB ? AB : c->AB, nullptr, nullptr, s);
}

// Same as gmpc_lqr_backward but reuses the relu masks the preceding gmpc_rollout_cost of this ctx
// produced for exactly this (X, U) -- the rollout+backward "step" timed by bench.py.
extern "C" int gmpc_lqr_backward_after_rollout(gmpc_ctx* c, int B, const float* X, const float* U,
                                               const float* goal, float* K, float* k, float* grad,
                                               float* adjoints, float* AB, void* stream) {
  TRY(check_call(c, B));
  if (!X || !U || !goal) return fail(GMPC_EINVAL, "null argument");
  if (c->big && AB) return fail(GMPC_EINVAL, "AB output is not materialised for n > 64 (pass NULL)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  c->solB = 0;   // overwrites QT/qT and (with NULL outputs) the ctx's K / AB
  c->gradB = 0;
  return backward_pass(c, B, X, U, goal, nullptr, K ? K : c->Ks, k ? k : c->ks, grad, adjoints,
                       AB ? AB : c->AB, nullptr, nullptr, s);
}

// line-search candidate evaluation of the LSTM dynamics variant: same (trajectory, halving) work list and
// the same decide / commit kernels as the MLP path, the rollouts by k_dynl_traj<true>
static void dynl_ls_eval(void* user, const TrajArgs& t, int max_items, hipStream_t s) {
  gmpc_ctx* c = static_cast<gmpc_ctx*>(user);
  DynlTrajArgs d = base_dynl(c, t.B, t.goal);
  d.item_b = t.item_b; d.item_k = t.item_k; d.nitems = t.nitems;
  d.Xn = t.X; d.Un = t.Uio; d.Kg = t.Kg; d.kg = t.kg;
  d.Xc = t.Xc; d.Uc = t.Uc; d.objc = t.objc; d.alpha_0 = t.alpha_0;
  gmpc_launch_dynl_candidates(d, max_items, s);
}

extern "C" int gmpc_ilqr_solve(gmpc_ctx* c, int B, const float* x0, const float* U_init,
                               const float* goal, const gmpc_ilqr_opts* opts, float* X, float* U,
                               float* obj, float* grad, float* adjoints, int* iterations,
                               void* stream) {
  TRY(check_call(c, B));
  if (!x0 || !U_init || !goal || !opts) return fail(GMPC_EINVAL, "null argument");
  if (opts->make_psd) return fail(GMPC_EINVAL, "make_psd=1 is not on the reference path");
  hipStream_t s = static_cast<hipStream_t>(stream);
  c->solB = 0;   // restored only when the solve has completed (an early error return leaves none)
  c->solBox = false;
  c->gradB = 0;
  const gmpc_shape& sh = c->sh;
  const size_t n = sh.n, m = sh.m, T = sh.T;
  HIP_TRY(hipMemcpyAsync(c->Us, U_init, B * T * m * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->goals, goal, B * (T + 1) * (size_t)c->nx * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(c->iters, 0, B * sizeof(int), s));
  // alpha = alpha_0, steps = +inf
  std::vector<float> init(3 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    init[b] = opts->alpha_0;
    init[B + b] = INFINITY;
    init[2 * (size_t)B + b] = INFINITY;
  }
  HIP_TRY(hipMemcpyAsync(c->alpha, init.data(), B * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->obj_step, init.data() + B, B * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->U_step, init.data() + 2 * (size_t)B, B * sizeof(float),
                         hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // `init` goes out of scope below
  if (c->dynl) {
    DynlTrajArgs d = base_dynl(c, B, c->goals);
    d.x0 = x0; d.U = c->Us; d.X = c->Xs; d.costs = nullptr; d.obj = c->obj;
    gmpc_launch_dynl_rollout(d, s);
  } else {
    TrajArgs a = base_traj(c, B, c->goals);
    a.x0 = x0; a.U = c->Us; a.X = c->Xs; a.costs = nullptr; a.obj = c->obj; a.masks = c->masks;
    gmpc_launch_rollout(a, s);
  }
  TRY(backward_pass(c, B, c->Xs, c->Us, c->goals, nullptr, c->Ks, c->ks, c->grads, c->adjs, c->AB,
                    c->cont, opts, s));
  TrajArgs ls = base_traj(c, B, c->goals);
  ls.X = c->Xs; ls.Uio = c->Us; ls.obj = c->obj; ls.masks = c->masks; ls.Kg = c->Ks; ls.kg = c->ks;
  ls.Xc = c->Xc; ls.Uc = c->Uc; ls.maskc = c->maskc; ls.active = c->cont; ls.alpha = c->alpha;
  ls.obj_step = c->obj_step; ls.U_step = c->U_step; ls.iters = c->iters;
  ls.alpha_0 = opts->alpha_0; ls.alpha_min = opts->alpha_min;
  // which kernels evaluate the line searches' candidates, how many rounds: fixed for the solve
  LsPlan plan;
  if (gmpc_ls_plan(ls, c->ncu, c->dynl, &plan) != 0 && opts->maxiter > 0)
    return fail(GMPC_EINVAL, "line search: alpha_0 / alpha_min need more than %d rounds", GMPC_LS_ROUNDS_MAX);
  // a fresh solve starts its first line search with a single full step per trajectory
  HIP_TRY(hipMemsetAsync(c->lsw.prevk, 0, B * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(c->lsw.counts + GMPC_LS_ROUNDS_MAX, 0, (1 + GMPC_LS_STATS) * sizeof(int), s));
  // "Has every trajectory stopped?" is answered without stalling the queue: the continuation flags of
  // iteration `it` are copied to a pinned ring slot when the iteration is enqueued and looked at
  // GMPC_POLL_DEPTH iterations later, so the host runs at most that many iterations ahead of what it
  // knows.  Iterations enqueued after the last trajectory stopped are exact no-ops (every kernel of the
  // loop is masked by the same flags), at most GMPC_POLL_DEPTH of them.
  if (!c->hcont) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->hcont), (size_t)GMPC_POLL_DEPTH * c->maxB * sizeof(int),
                          hipHostMallocDefault));
    for (int i = 0; i < GMPC_POLL_DEPTH; ++i) HIP_TRY(hipEventCreateWithFlags(&c->poll_ev[i], hipEventDisableTiming));
  }
  for (int it = 0; it < opts->maxiter; ++it) {
    const int slot = it % GMPC_POLL_DEPTH;
    int* hc = c->hcont + (size_t)slot * c->maxB;
    if (it >= GMPC_POLL_DEPTH) {
      HIP_TRY(hipEventSynchronize(c->poll_ev[slot]));     // flags as of iteration it - GMPC_POLL_DEPTH
      bool any = false;
      for (int b = 0; b < B; ++b) any |= hc[b] != 0;
      if (!any) break;
    }
    HIP_TRY(hipMemcpyAsync(hc, c->cont, B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(c->poll_ev[slot], s));
    {
      ProfScope ps(c, PROF_LINESEARCH, s);
      gmpc_launch_linesearch(ls, plan, c->lsw, s, c->dynl ? &dynl_ls_eval : nullptr, c);
    }
    TRY(backward_pass(c, B, c->Xs, c->Us, c->goals, c->cont, c->Ks, c->ks, c->grads, c->adjs, c->AB,
                      c->cont, opts, s));
  }
  if (X) HIP_TRY(hipMemcpyAsync(X, c->Xs, B * (T + 1) * n * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (U) HIP_TRY(hipMemcpyAsync(U, c->Us, B * T * m * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (obj) HIP_TRY(hipMemcpyAsync(obj, c->obj, B * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (grad) HIP_TRY(hipMemcpyAsync(grad, c->grads, B * T * m * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (adjoints)
    HIP_TRY(hipMemcpyAsync(adjoints, c->adjs, B * (T + 1) * n * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (iterations)
    HIP_TRY(hipMemcpyAsync(iterations, c->iters, B * sizeof(int), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  c->solB = B;
  return 0;
}

// The whole solve in one launch (gmpc_fused_solve.hip), shared by gmpc_ilqr_solve_fused and gmpc_ilqr_solve_box
// (`who` heads the refusals): coverage checks, the argument block, the launch.
static int solve_one_launch(gmpc_ctx* c, int B, const float* x0, const float* U_init, const float* goal,
                            const gmpc_ilqr_opts* opts, float* X, float* U, float* obj, float* grad, float* adjoints,
                            int* iterations, void* stream, const char* who, bool box, const float* u_lo,
                            const float* u_hi) {
  TRY(check_call(c, B));
  if (!x0 || !U_init || !goal || !opts) return fail(GMPC_EINVAL, "null argument");
  if (opts->make_psd) return fail(GMPC_EINVAL, "make_psd=1 is not on the reference path");
  const gmpc_shape& sh = c->sh;
  if (c->dynl) return fail(GMPC_EINVAL, "%s: MLP dynamics only (dyn_lstm_features = %d)", who, sh.dyn_lstm_features);
  if (c->big)
    return fail(GMPC_EINVAL, "%s: n <= 64 and m <= 32 only (n=%d m=%d)", who, sh.n, sh.m);
  if (sh.T > GMPC_FZ_MAX_T) return fail(GMPC_EINVAL, "%s: T <= %d only (T=%d)", who, GMPC_FZ_MAX_T, sh.T);
  const int k_max = gmpc_ls_halvings(opts->alpha_0, opts->alpha_min, GMPC_FZ_MAX_HALVINGS + 1);
  if (k_max > GMPC_FZ_MAX_HALVINGS)
    return fail(GMPC_EINVAL, "%s: alpha_0 / alpha_min allow more than %d halvings", who, GMPC_FZ_MAX_HALVINGS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  c->solB = 0;
  c->solBox = false;
  c->gradB = 0;
  FusedSolveArgs a;
  memset(&a, 0, sizeof(a));
  a.n = sh.n; a.m = sh.m; a.T = sh.T; a.k_max = k_max;
  a.dyn = c->dyn; a.cost = c->cost; a.mpc_w = c->mpc_w; a.opts = *opts;
  a.x0 = x0; a.U_init = U_init; a.goal_in = goal;
  a.X = c->Xs; a.U = c->Us; a.goal = c->goals; a.AB = c->AB; a.QT = c->QT; a.qT = c->qT;
  a.K = c->Ks; a.k = c->ks; a.grad = c->grads; a.adj = c->adjs;
  a.obj = c->obj; a.alpha = c->alpha; a.obj_step = c->obj_step; a.U_step = c->U_step; a.iters = c->iters;
  a.cand = c->fzcand;
  a.oX = X; a.oU = U; a.oobj = obj; a.ograd = grad; a.oadj = adjoints; a.oiters = iterations;
  if (box) {
    BoxSolveArgs x;
    x.u_lo = u_lo; x.u_hi = u_hi;
    x.count = c->box_count; x.iters = c->box_iters; x.clamped = c->box_clamped;
    gmpc_launch_ilqr_box(a, x, B, s);
  } else {
    gmpc_launch_ilqr_fused(a, B, s);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// Same results and ctx state as gmpc_ilqr_solve on the shapes it covers, nothing waited for on the host.
extern "C" int gmpc_ilqr_solve_fused(gmpc_ctx* c, int B, const float* x0, const float* U_init,
                                     const float* goal, const gmpc_ilqr_opts* opts, float* X, float* U,
                                     float* obj, float* grad, float* adjoints, int* iterations,
                                     void* stream) {
  TRY(solve_one_launch(c, B, x0, U_init, goal, opts, X, U, obj, grad, adjoints, iterations, stream, "fused solve",
                       false, nullptr, nullptr));
  c->solB = B;   // stream-ordered: a later call on the same stream sees the finished solve
  return 0;
}

// The control-limited solve.  It holds no solution for the bilevel tail (solB stays 0): the MPC action
// path does not pay for the clamped-set launch; gmpc_ilqr_solve_box_held is the variant the tail may follow.
extern "C" int gmpc_ilqr_solve_box(gmpc_ctx* c, int B, const float* x0, const float* U_init,
                                   const float* goal, const gmpc_ilqr_opts* opts, float* X, float* U,
                                   float* obj, float* grad, float* adjoints, int* iterations,
                                   void* stream, const float* u_lo, const float* u_hi) {
  return solve_one_launch(c, B, x0, U_init, goal, opts, X, U, obj, grad, adjoints, iterations, stream, "box solve",
                          true, u_lo, u_hi);
}

// The control-limited solve, held for the bilevel tail: the same launch, then the clamped set of the
// solution -- from the ctx's U and full gradient and the caller's bounds -- as one word per step; the tail's Hessian
// solve runs on each step's free rows.
extern "C" int gmpc_ilqr_solve_box_held(gmpc_ctx* c, int B, const float* x0, const float* U_init,
                                        const float* goal, const gmpc_ilqr_opts* opts, float* X, float* U,
                                        float* obj, float* grad, float* adjoints, int* iterations,
                                        void* stream, const float* u_lo, const float* u_hi) {
  TRY(solve_one_launch(c, B, x0, U_init, goal, opts, X, U, obj, grad, adjoints, iterations, stream, "box solve",
                       true, u_lo, u_hi));
  gmpc_launch_box_clamped(B, c->sh.T, c->sh.m, c->Us, c->grads, u_lo, u_hi, c->box_mask,
                          static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  c->solB = B;   // stream-ordered, as after the fused solve
  c->solBox = true;
  return 0;
}

// single model evaluations (the reference's model protocol, base.py:4-49) -----------------------

extern "C" int gmpc_get_cost(gmpc_ctx* c, int B, const float* x, const float* u, const float* goal_row,
                             int terminal, float* cost, void* stream) {
  TRY(check_call(c, B));
  if (!x || !cost || (!terminal && (!u || !goal_row))) return fail(GMPC_EINVAL, "null argument");
  gmpc_launch_get_cost(B, c->sh.n, c->nx, c->sh.m, c->cost, c->mpc_w, x, u, goal_row, terminal != 0, cost,
                       static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_predict(gmpc_ctx* c, int B, const float* x, const float* u, float* next_x,
                            void* stream) {
  TRY(check_call(c, B));
  if (!x || !u || !next_x) return fail(GMPC_EINVAL, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = c->sh.n;
  c->solB = 0;   // the one-step rollout below overwrites the ctx's relu masks and objectives
  c->gradB = 0;
  // a horizon-1 rollout through the trajectory kernel: X = [x, f(x, u)] in the line-search scratch
  HIP_TRY(hipMemsetAsync(c->goals, 0, (size_t)B * 2 * n * sizeof(float), s));
  if (c->dynl) {
    DynlTrajArgs d = base_dynl(c, B, c->goals);
    d.T = 1;
    d.x0 = x; d.U = u; d.X = c->Xc; d.costs = nullptr; d.obj = c->obj;
    gmpc_launch_dynl_rollout(d, s);
  } else {
    TrajArgs a = base_traj(c, B, c->goals);
    a.T = 1;
    a.x0 = x; a.U = u; a.X = c->Xc; a.costs = nullptr; a.obj = c->obj; a.masks = c->masks;
    gmpc_launch_rollout(a, s);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy2DAsync(next_x, n * sizeof(float), c->Xc + n, 2 * n * sizeof(float), n * sizeof(float),
                           B, hipMemcpyDeviceToDevice, s));
  return 0;
}

extern "C" long gmpc_linesearch_candidates(gmpc_ctx* c) {
  if (!c) return -1;
  int v = 0;
  if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(&v, c->lsw.counts + GMPC_LS_ROUNDS_MAX, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return v;
}

extern "C" int gmpc_linesearch_stats(gmpc_ctx* c, long* out, int n) {
  if (!c || !out) return fail(GMPC_EINVAL, "ctx / out is null");
  int v[GMPC_LS_STATS];
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());      // (streams created non-blocking are not ordered against a null-stream copy)
  HIP_TRY(hipMemcpy(v, c->lsw.counts + GMPC_LS_ROUNDS_MAX + 1, sizeof(v), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) out[i] = i < GMPC_LS_STATS ? v[i] : 0;
  return 0;
}
