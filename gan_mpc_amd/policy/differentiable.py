"""The batched iLQR solve as a differentiable torch op: (X, U) = ilqr_layer(policy, params, x0, goal, init_U).

Backward is the implicit-function gradient through the solution U* (grad_U J(U*; x0, goal, theta) = 0): the incoming
cotangents gX = dL/dX, gU = dL/dU go to gmpc_bilevel_grad_cotangent with sign -1 (the true derivative, not the
reference's sign), then gmpc_bilevel_grad_inputs gives dL/dx0 and dL/dgoal from the same Hessian solve (DESIGN.md
section 12), and, with dynamics_grad=True, gmpc_bilevel_grad_dynamics dL/dtheta_dyn.

  - params: a DeviceParams; its flat vector `params.flat` is the differentiable leaf.  Its mpc_weights and
    cost_params ranges receive gradient, summed over the batch.  The dynamics_params range receives gradient only
    with dynamics_grad=True (relu-MLP dynamics, n <= 64 and m <= 32: anything else fails in forward); by default it
    gets none, as in the reference.  Critic and expert parameters get none (critic_layer and expert_layer are
    their layers).
  - x0 (B, n) -- xc, carry columns included for LSTM dynamics -- and goal (B, T+1, x_size) receive per-sample
    gradients.  dL/dx0 is not available on the step-major pipeline (n > 64 or m > 32): asking for it (x0 requiring
    grad) fails in forward.
  - init_U receives none: at a stationary point the solution does not depend on the initial guess (away from the
    solver's stopping tolerance, where it does, but not differentiably).
  - The engine holds one solution at a time.  Backward must run before another solve on the same engine; otherwise it
    raises instead of differentiating the wrong solution.

(X, costs) = rollout_layer(policy, params, x0, U, goal) is the rollout and its per-step costs as a differentiable torch
op: backward is one call of gmpc_rollout_vjp, the true derivative w.r.t. x0, U, goal and the
mpc_weights / cost_params / dynamics_params ranges of params.flat (dynamics_grad=False leaves the last one out).  Its
forward runs on a second engine of the policy bound to the same parameters, so an iLQR solution held for
ilqr_layer's backward survives it.  Relu-MLP dynamics only (LSTM dynamics fail in forward).

(goal, init_U) = expert_layer(policy, expert_flat, expert_shape, history) is the expert sequence model's rollout
(gmpc_expert_rollout on the policy's engine) as a differentiable torch op: backward is one call of gmpc_expert_vjp
(DESIGN.md section 15), the true derivative w.r.t. expert_flat -- a device fp32 vector in params.pack_expert's layout,
e.g. ExpertModel.device_params' -- summed over the batch, and w.r.t. history per window.  The expert's parameters are
not part of params.flat: expert_flat is their leaf, and this layer is the one way a task loss reaches them
(ilqr_layer's dL/dgoal, rollout_layer's dL/dU).  Both its forward and its backward leave a held iLQR solution and its
bilevel tail alone, so it composes with the other two layers in one backward():
expert_layer -> ilqr_layer -> loss (init_U gets no cotangent) and expert_layer -> rollout_layer(U=init_U) -> loss.

score = critic_layer(policy, params, xseq) is the critic's score of Bc state sequences (gmpc_critic_score_vjp on the
policy's engine) as a differentiable torch op: backward is one call of gmpc_critic_vjp with the
incoming dL/dscore, the true derivative w.r.t. xseq per sequence and w.r.t. the critic_params range of params.flat,
summed over the batch (zeros on every other range).  Any objective of the scores written in torch -- Wasserstein,
least squares, hinge, label smoothing, per-sequence weights -- so reaches the discriminator's parameters, and the
generator loss runs through expert_layer -> ilqr_layer -> critic_layer -> loss in one backward(): neither its forward
nor its backward touches a held iLQR solution or its bilevel tail.  xseq has x_size columns (with LSTM dynamics the
caller slices X[..., :x_size]); it never rebuilds the policy's engine, so Bc <= 2 max_batch of the bound engine.
The layer is differentiable twice in xseq: torch.autograd.grad(score.sum(), xseq, create_graph=True) returns an input
gradient with a graph behind it, whose backward is one call of gmpc_critic_dir_vjp -- what a
gradient penalty on the critic needs (gan_policy.gradient_penalty).  The parameter gradient is not differentiable again
(NotImplementedError), third derivatives are refused, and critics with x_size + lstm_features > 256 are refused by the
second backward.  Without create_graph the layer runs the same calls as before.

X, U, obj = mppi_layer(policy, params, x0, goal, init_U, control_bounds, ...) is the path-integral solve
(gmpc_mppi_solve) as a differentiable torch op: backward is one call of gmpc_mppi_vjp, the true
derivative through the sampler w.r.t. x0, goal, init_U and the mpc_weights / cost_params (and, asked for,
dynamics_params) ranges of params.flat.  It is the way to train through a control-limited controller at any horizon;
it runs on the second engine, as rollout_layer does.

(X, costs) = ensemble_rollout_layer(policy, params, x0, U, goal, members=None) is rollout_layer under every member of a
dynamics ensemble at once (Engine.ensemble_rollout; X (P, B, T+1, n), costs (P, B, T+1)): backward is one call of
gmpc_ensemble_rollout_vjp, the true derivative w.r.t. x0, U, goal, the mpc_weights / cost_params
ranges of params.flat and, for a members tensor that requires grad, the members' weights.  Any torch function of the
members' states and costs -- a risk aggregate, their spread -- so reaches the plan and the cost network."""

import torch
from torch.autograd.function import once_differentiable

from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.engine import MPPI_KWARGS, Engine
from gan_mpc_amd.policy import optimizers as opt

_THETA_KEYS = ("mpc_weights", "cost_params")


class ILQRFunction(torch.autograd.Function):
    """forward(policy, dparams, kwargs, flat, x0, goal, init_U, dynamics_grad=False) -> (X, U); flat is
    dparams.flat."""

    @staticmethod
    def forward(ctx, policy, dparams, kwargs, flat, x0, goal, init_U, dynamics_grad=False):
        B = x0.shape[0]
        eng = policy.bind(dparams, B)
        if dynamics_grad and (eng.shape.dyn_lstm_features > 0 or eng.big):
            raise GmpcError(f"ilqr_layer: dynamics_grad=True needs relu-MLP dynamics with n <= 64 and m <= 32 "
                            f"(n={eng.n}, m={eng.m}, dyn_lstm_features={eng.shape.dyn_lstm_features})")
        if ctx.needs_input_grad[4] and eng.big:
            raise GmpcError(f"ilqr_layer: dL/dx0 is not available on the step-major pipeline (n={eng.n} > 64 or "
                            f"m={eng.m} > 32); pass x0 without requires_grad (goal gradients work)")
        f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        solve = opt._solver(policy, eng, hold=True)       # a "box" policy: the solve the tail may follow
        sol = solve(f32(x0), f32(init_U), f32(goal), kwargs or policy.trajax_ilqr_kwargs)
        ctx.eng, ctx.solve_count, ctx.B = eng, eng.solve_count, B
        ctx.theta = dparams.range_of(_THETA_KEYS)
        ctx.dyn = dparams.range_of(("dynamics_params",)) if dynamics_grad else None
        ctx.flat_shape = flat.shape
        return sol["X"], sol["U"]

    @staticmethod
    def backward(ctx, gX, gU):
        eng, B = ctx.eng, ctx.B
        if eng.ctx is None or eng.solve_count != ctx.solve_count:
            raise RuntimeError("ilqr_layer backward: another iLQR solve ran on this engine after the forward, so the "
                               "solution it differentiates is gone; run backward before the next solve")
        want_theta, want_x0, want_goal = ctx.needs_input_grad[3:6]
        f32 = lambda t: None if t is None else t.to(torch.float32).contiguous()  # noqa: E731
        lx, lu = f32(gX), f32(gU)
        if lx is None and lu is None:
            return (None,) * 8
        try:
            grad_sum = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0)
            gx0 = ggoal = None
            if want_x0 or want_goal:
                gx0, ggoal = eng.bilevel_grad_inputs(B, lx, want_x0=want_x0, want_goal=want_goal)
            gdyn = eng.bilevel_grad_dynamics(B, lx) if want_theta and ctx.dyn is not None else None
        except GmpcError as e:
            raise RuntimeError(f"ilqr_layer backward: the engine no longer holds the forward's solution ({e})") from e
        gflat = None
        if want_theta:
            lo, cnt = ctx.theta
            gflat = torch.zeros(ctx.flat_shape, dtype=grad_sum.dtype, device=grad_sum.device)
            gflat[lo:lo + cnt] = grad_sum
            if gdyn is not None:
                lo, cnt = ctx.dyn
                gflat[lo:lo + cnt] = gdyn
        return None, None, None, gflat, gx0, ggoal, None, None


def ilqr_layer(policy, params, x0, goal, init_U, trajax_ilqr_kwargs=None, dynamics_grad=False):
    """(X (B, T+1, n), U (B, T, m)) of the policy's iLQR solve (its `solver`: "rounds", "fused", or "box" -- then
    through the solution's active set held fixed), differentiable w.r.t. x0, goal and the
    mpc_weights / cost_params ranges of params.flat, and with dynamics_grad=True its dynamics_params range (see the
    module docstring).  params: the policy's DeviceParams (a parameter tree is
    converted, and then is not differentiable); x0, goal, init_U: device tensors.  A "cem" policy is refused
    (NotImplementedError): the sampler has no derivative."""
    opt.refuse_cem(policy, "ilqr_layer")
    dparams = policy.to_device_params(params)
    return ILQRFunction.apply(policy, dparams, trajax_ilqr_kwargs, dparams.flat, x0, goal, init_U,
                              bool(dynamics_grad))


def _rollout_engine(policy, dparams, B):
    """The policy's second engine (not the one holding its iLQR solution), sized for B and bound to dparams."""
    n, m, nx, dyn_lstm = dparams.sizes_of_state()
    if dyn_lstm:
        raise GmpcError(f"rollout_layer: relu-MLP dynamics only (dyn_lstm_features = {dyn_lstm})")
    key = policy._shape_key(dparams)
    cached = getattr(policy, "_rollout_eng", None)
    if cached is None or cached[0] != key or B > cached[1].max_batch:
        if cached is not None:
            cached[1].close()
        eng = Engine(n, m, policy.config.mpc.horizon, dparams.meta["dyn_dims"], dparams.meta["cost_dims"],
                     max_batch=max(B, 8), device=policy.device().index)
        policy._rollout_eng = (key, eng)
    eng = policy._rollout_eng[1]
    eng.set_params(dparams.view("mpc_weights"), dparams.view("dynamics_params"), dparams.view("cost_params"))
    return eng


class RolloutFunction(torch.autograd.Function):
    """forward(eng, dparams, flat, x0, U, goal, dynamics_grad) -> (X, costs); eng is bound to dparams."""

    @staticmethod
    def forward(ctx, eng, dparams, flat, x0, U, goal, dynamics_grad):
        f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        U32, goal32 = f32(U), f32(goal)
        X, costs = eng.rollout_cost(f32(x0), U32, goal32)
        ctx.eng = eng
        ctx.views = eng._bound
        ctx.theta = dparams.range_of(_THETA_KEYS)
        ctx.dyn = dparams.range_of(("dynamics_params",)) if dynamics_grad else None
        ctx.flat_shape = flat.shape
        ctx.save_for_backward(X, U32, goal32)
        ctx.set_materialize_grads(False)
        return X, costs

    @staticmethod
    def backward(ctx, gX, gc):
        want_theta, want_x0, want_U, want_goal = ctx.needs_input_grad[2:6]
        if (gX is None and gc is None) or not (want_theta or want_x0 or want_U or want_goal):
            return (None,) * 7
        eng = ctx.eng
        X, U, goal = ctx.saved_tensors
        if eng._bound is None or any(a.data_ptr() != b.data_ptr() for a, b in zip(eng._bound, ctx.views)):
            eng.set_params(*ctx.views)      # another rollout_layer rebound the engine in between
        f32 = lambda t: None if t is None else t.to(torch.float32).contiguous()  # noqa: E731
        out = eng.rollout_vjp(X, U, goal, f32(gX), f32(gc), want_x0=want_x0, want_U=want_U, want_goal=want_goal,
                              want_theta=want_theta, want_dyn=want_theta and ctx.dyn is not None)
        gflat = None
        if want_theta:
            lo, cnt = ctx.theta
            gflat = torch.zeros(ctx.flat_shape, dtype=torch.float32, device=X.device)
            gflat[lo:lo + cnt] = out["theta"]
            if ctx.dyn is not None:
                lo, cnt = ctx.dyn
                gflat[lo:lo + cnt] = out["dyn"]
        return None, None, gflat, out["x0"], out["U"], out["goal"], None


def rollout_layer(policy, params, x0, U, goal, dynamics_grad=True):
    """(X (B, T+1, n), costs (B, T+1)) = the rollout of (x0, U) under the policy's dynamics and its per-step costs
    against goal (gmpc_rollout_cost), differentiable w.r.t. x0, U, goal and the mpc_weights / cost_params (and, with
    dynamics_grad, dynamics_params) ranges of params.flat: the true derivative (see the module docstring).  params:
    the policy's DeviceParams (a parameter tree is converted, and then is not differentiable); x0 (B, n), U (B, T, m),
    goal (B, T+1, n): device tensors."""
    dparams = policy.to_device_params(params)
    eng = _rollout_engine(policy, dparams, x0.shape[0])
    return RolloutFunction.apply(eng, dparams, dparams.flat, x0, U, goal, bool(dynamics_grad))


class EnsembleRolloutFunction(torch.autograd.Function):
    """forward(eng, dparams, flat, members, x0, U, goal) -> (X (P, B, T+1, n), costs (P, B, T+1)); eng is bound to
    dparams.  backward is one gmpc_ensemble_rollout_vjp call."""

    @staticmethod
    def forward(ctx, eng, dparams, flat, members, x0, U, goal):
        f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        mem32, U32, goal32 = eng.to_dev(members.detach()), f32(U), f32(goal)
        out = eng.ensemble_rollout(mem32, f32(x0), U32, goal32, want=("X", "costs"))
        ctx.eng = eng
        ctx.views = eng._bound
        ctx.theta = dparams.range_of(_THETA_KEYS)
        ctx.flat_shape = flat.shape
        ctx.save_for_backward(mem32, out["X"], U32, goal32)
        ctx.set_materialize_grads(False)
        return out["X"], out["costs"]

    @staticmethod
    def backward(ctx, gX, gc):
        want_theta, want_mem, want_x0, want_U, want_goal = ctx.needs_input_grad[2:7]
        if (gX is None and gc is None) or not (want_theta or want_mem or want_x0 or want_U or want_goal):
            return (None,) * 7
        eng = ctx.eng
        members, X, U, goal = ctx.saved_tensors
        if eng._bound is None or any(a.data_ptr() != b.data_ptr() for a, b in zip(eng._bound, ctx.views)):
            eng.set_params(*ctx.views)      # another layer rebound the engine in between
        f32 = lambda t: None if t is None else t.to(torch.float32).contiguous()  # noqa: E731
        keys = [k for k, w in zip(Engine.ENSEMBLE_ROLLOUT_VJP_WANT, (want_x0, want_U, want_goal, want_theta, want_mem))
                if w]
        out = eng.ensemble_rollout_vjp(members, X, U, goal, f32(gX), f32(gc), want=keys)
        gflat = None
        if want_theta:
            lo, cnt = ctx.theta
            gflat = torch.zeros(ctx.flat_shape, dtype=torch.float32, device=X.device)
            gflat[lo:lo + cnt] = out["theta"]
        return None, None, gflat, out.get("members"), out.get("x0"), out.get("U"), out.get("goal")


def ensemble_rollout_layer(policy, params, x0, U, goal, members=None):
    """(X (P, B, T+1, n), costs (P, B, T+1)) = the rollout of (x0, U) under every member of a dynamics ensemble and
    its per-step costs against goal (Engine.ensemble_rollout on the policy's second engine), differentiable w.r.t. x0,
    U, goal and the mpc_weights / cost_params ranges of params.flat: backward is one call of gmpc_ensemble_rollout_vjp
    (DESIGN.md section 29).  members: a float32 (P, dyn_count) tensor -- differentiated too when it requires grad --;
    None: the policy's dynamics ensemble, which is not differentiated (ValueError when the policy has none).  The
    dynamics_params range of params.flat gets no gradient: the members, not the nominal network, roll the plan out."""
    dparams = policy.to_device_params(params)
    eng = _rollout_engine(policy, dparams, x0.shape[0])
    if members is None:
        if policy.dynamics_ensemble is None:
            raise ValueError("ensemble_rollout_layer needs members or a dynamics_ensemble (the constructor's, or "
                             "set_dynamics_ensemble): none is set")
        if policy._ensemble_dev is None or policy._ensemble_dev.device != eng.device:
            policy._ensemble_dev = eng.to_dev(policy.dynamics_ensemble)
        members = policy._ensemble_dev
    elif not torch.is_tensor(members):
        members = eng.to_dev(members)
    return EnsembleRolloutFunction.apply(eng, dparams, dparams.flat, members, x0, U, goal)


class EnsembleDisagreementFunction(torch.autograd.Function):
    """forward(eng, dparams, flat, members, x0, U) -> (d (P, B, T), D (P, B)); eng is bound to dparams.  backward is
    one gmpc_ensemble_disagreement_vjp call at the nominal rollout the forward kept."""

    @staticmethod
    def forward(ctx, eng, dparams, flat, members, x0, U):
        f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        mem32, U32 = eng.to_dev(members.detach()), f32(U)
        out = eng.ensemble_disagreement(mem32, f32(x0), U32, want=("X", "d", "D"))
        ctx.eng = eng
        ctx.views = eng._bound
        ctx.dyn = dparams.range_of(("dynamics_params",))
        ctx.flat_shape = flat.shape
        ctx.save_for_backward(mem32, out["X"], U32)
        ctx.set_materialize_grads(False)
        return out["d"], out["D"]

    @staticmethod
    def backward(ctx, gd, gD):
        want_nom, want_mem, want_x0, want_U = ctx.needs_input_grad[2:6]
        if (gd is None and gD is None) or not (want_nom or want_mem or want_x0 or want_U):
            return (None,) * 6
        eng = ctx.eng
        members, X, U = ctx.saved_tensors
        if eng._bound is None or any(a.data_ptr() != b.data_ptr() for a, b in zip(eng._bound, ctx.views)):
            eng.set_params(*ctx.views)      # another layer rebound the engine in between
        f32 = lambda t: None if t is None else t.to(torch.float32).contiguous()  # noqa: E731
        keys = [k for k, w in zip(Engine.ENSEMBLE_DISAGREEMENT_VJP_WANT, (want_x0, want_U, want_nom, want_mem)) if w]
        out = eng.ensemble_disagreement_vjp(members, X, U, f32(gd), f32(gD), want=keys)
        gflat = None
        if want_nom:
            lo, cnt = ctx.dyn
            gflat = torch.zeros(ctx.flat_shape, dtype=torch.float32, device=X.device)
            gflat[lo:lo + cnt] = out["nominal"]
        return None, None, gflat, out.get("members"), out.get("x0"), out.get("U")


def ensemble_disagreement_layer(policy, params, x0, U, members=None):
    """(d (P, B, T), D (P, B)) = the one-step disagreement of every member of a dynamics ensemble with the policy's
    (nominal) dynamics along the nominal rollout of (x0, U) (Engine.ensemble_disagreement on the policy's second
    engine, the same bits), differentiable w.r.t. x0, U and the dynamics_params range of params.flat -- the nominal
    network, a real gradient here: it both measures and rolls the plan out --: backward is one call of
    gmpc_ensemble_disagreement_vjp.  members: a float32 (P, dyn_count) tensor -- differentiated
    too when it requires grad --; None: the policy's dynamics ensemble, which is not differentiated (ValueError when
    the policy has none).  The whole horizon only: U is (B, T, m)."""
    dparams = policy.to_device_params(params)
    eng = _rollout_engine(policy, dparams, x0.shape[0])
    if members is None:
        if policy.dynamics_ensemble is None:
            raise ValueError("ensemble_disagreement_layer needs members or a dynamics_ensemble (the constructor's, or "
                             "set_dynamics_ensemble): none is set")
        if policy._ensemble_dev is None or policy._ensemble_dev.device != eng.device:
            policy._ensemble_dev = eng.to_dev(policy.dynamics_ensemble)
        members = policy._ensemble_dev
    elif not torch.is_tensor(members):
        members = eng.to_dev(members)
    if U.dim() != 3 or U.shape[1] != eng.T:
        raise ValueError(f"ensemble_disagreement_layer: U must be (B, T = {eng.T}, m), got {tuple(U.shape)}")
    return EnsembleDisagreementFunction.apply(eng, dparams, dparams.flat, members, x0, U)


MPPI_CHUNK = 16     # problems whose sample rows mppi_layer's engine holds at once


class MPPIFunction(torch.autograd.Function):
    """forward(eng, dparams, bounds, kw, init_std, flat, x0, goal, init_U, dynamics_grad) -> (X, U, obj); eng is bound
    to dparams.  backward is one gmpc_mppi_vjp call on the traces the forward kept."""

    @staticmethod
    def forward(ctx, eng, dparams, bounds, kw, init_std, flat, x0, goal, init_U, dynamics_grad):
        f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        x32, goal32 = f32(x0), f32(goal)
        sol = eng.mppi_solve(x32, f32(init_U), goal32, bounds[0], bounds[1], kw, init_std=init_std, trace=True)
        ctx.eng, ctx.bounds, ctx.kw, ctx.sol = eng, bounds, kw, sol
        ctx.views = eng._bound
        ctx.theta = dparams.range_of(_THETA_KEYS)
        ctx.dyn = dparams.range_of(("dynamics_params",)) if dynamics_grad else None
        ctx.flat_shape = flat.shape
        ctx.save_for_backward(x32, goal32)
        ctx.set_materialize_grads(False)
        return sol["X"], sol["U"], sol["obj"]

    @staticmethod
    def backward(ctx, gX, gU, gobj):
        want_theta, want_x0, want_goal, want_U = ctx.needs_input_grad[5:9]
        if (gX is None and gU is None and gobj is None) or not (want_theta or want_x0 or want_U or want_goal):
            return (None,) * 10
        eng = ctx.eng
        x0, goal = ctx.saved_tensors
        if eng._bound is None or any(a.data_ptr() != b.data_ptr() for a, b in zip(eng._bound, ctx.views)):
            eng.set_params(*ctx.views)      # another layer rebound the engine in between
        f32 = lambda t: None if t is None else t.to(torch.float32).contiguous()  # noqa: E731
        out = eng.mppi_vjp(x0, goal, ctx.bounds[0], ctx.bounds[1], ctx.sol, f32(gU), f32(gX), f32(gobj), ctx.kw,
                           want_x0=want_x0, want_U=want_U, want_goal=want_goal, want_theta=want_theta,
                           want_dyn=want_theta and ctx.dyn is not None)
        gflat = None
        if want_theta:
            lo, cnt = ctx.theta
            gflat = torch.zeros(ctx.flat_shape, dtype=torch.float32, device=x0.device)
            gflat[lo:lo + cnt] = out["theta"]
            if ctx.dyn is not None:
                lo, cnt = ctx.dyn
                gflat[lo:lo + cnt] = out["dyn"]
        return None, None, None, None, None, gflat, out["x0"], out["goal"], out["U"], None


def mppi_layer(policy, params, x0, goal, init_U, control_bounds, mppi_kwargs=None, init_std=None,
               dynamics_grad=False):
    """(X (B, T+1, n), U (B, T, m), obj (B,)) of the path-integral solve from init_U under control_bounds = (lo, hi)
    (gmpc_mppi_solve; keywords engine.MPPI_KWARGS; init_std as for Engine.mppi_solve), differentiable w.r.t. x0, goal,
    init_U and the mpc_weights / cost_params ranges of params.flat, and with dynamics_grad=True its dynamics_params
    range: the true derivative through the sampler (gmpc_mppi_vjp), at any horizon.  U is the
    solver's mean, not clipped.  It runs on the policy's second engine, so the solution the policy's own engine holds
    stays usable; that engine is sized for max(B, num_samples * min(B, MPPI_CHUNK)) rows: the backward pass takes the
    sample rows of floor(rows / num_samples) problems per chunk, and one problem per chunk is launch-bound (DESIGN.md
    section 21).  params: the policy's DeviceParams (a parameter tree is converted, and then is not differentiable);
    x0, goal, init_U: device tensors."""
    dparams = policy.to_device_params(params)
    kw = dict(mppi_kwargs or {})
    N = int(kw.get("num_samples", MPPI_KWARGS["num_samples"]))
    B = x0.shape[0]
    eng = _rollout_engine(policy, dparams, max(B, N * min(B, MPPI_CHUNK)))
    return MPPIFunction.apply(eng, dparams, tuple(control_bounds), kw, init_std, dparams.flat, x0, goal, init_U,
                              bool(dynamics_grad))


class ExpertFunction(torch.autograd.Function):
    """forward(eng, expert_shape, expert_flat, history) -> (goal, init_U)."""

    @staticmethod
    def forward(ctx, eng, expert_shape, expert_flat, history):
        f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        flat32, hist32 = f32(expert_flat), f32(history)
        goal, init_U = eng.expert_rollout(hist32, flat32, expert_shape)
        ctx.eng, ctx.shape = eng, expert_shape
        ctx.save_for_backward(flat32, hist32)
        ctx.set_materialize_grads(False)
        return goal, init_U

    @staticmethod
    def backward(ctx, g_goal, g_U):
        want_params, want_history = ctx.needs_input_grad[2:4]
        if (g_goal is None and g_U is None) or not (want_params or want_history):
            return (None,) * 4
        eng = ctx.eng
        if eng.ctx is None:
            raise RuntimeError("expert_layer backward: the engine of the forward has been closed (the policy rebuilt "
                               "it for another shape or a larger batch)")
        flat, history = ctx.saved_tensors
        f32 = lambda t: None if t is None else t.to(torch.float32).contiguous()  # noqa: E731
        out = eng.expert_vjp(history, flat, ctx.shape, f32(g_goal), f32(g_U), want_params=want_params,
                             want_history=want_history)
        return None, None, out["params"], out["history"]


def expert_layer(policy, expert_flat, expert_shape, history):
    """(goal (B, T+1, x_size), init_U (B, T, m)) of the expert sequence model on the policy's engine, differentiable
    w.r.t. expert_flat (device fp32 vector in params.pack_expert's layout; gradient summed over the batch) and history
    (B, hist+1, x_size) (see the module docstring).  expert_shape: the model's gmpc_expert_shape
    (engine.make_expert_shape, or ExpertModel.device_params)."""
    B = history.shape[0]
    eng = policy._engine
    if eng is None or B > eng.max_batch:
        if policy._bound is None:
            raise GmpcError(f"expert_layer: the policy has no engine for a batch of {B} yet; bind its parameters first "
                            "(policy.bind(params, batch))")
        eng = policy.engine_for(B)
    return ExpertFunction.apply(eng, expert_shape, expert_flat, history)


class CriticFunction(torch.autograd.Function):
    """forward(eng, dparams, flat, xseq) -> score; flat is dparams.flat."""

    @staticmethod
    def forward(ctx, eng, dparams, flat, xseq):
        xs = xseq.detach().to(torch.float32).contiguous()
        crit = dparams.view("critic_params")
        score, _ = eng.critic_score_vjp(xs, crit, want_dx=False)
        ctx.eng, ctx.crit = eng, crit
        ctx.range = dparams.range_of(("critic_params",))
        ctx.flat, ctx.xseq = flat, xseq      # the graph's own inputs: a create_graph backward goes through them
        ctx.save_for_backward(xs)
        ctx.set_materialize_grads(False)
        return score

    @staticmethod
    def backward(ctx, g_score):
        want_params, want_dx = ctx.needs_input_grad[2:4]
        if g_score is None or not (want_params or want_dx):
            return (None,) * 4
        eng = ctx.eng
        if eng.ctx is None:
            raise RuntimeError("critic_layer backward: the engine of the forward has been closed (the policy rebuilt "
                               "it for another shape or a larger batch)")
        xs, = ctx.saved_tensors
        gflat, dx = CriticGradFunction.apply(eng, ctx.crit, ctx.range, xs, ctx.flat, ctx.xseq, g_score, want_params,
                                             want_dx)
        return None, None, gflat, dx


class CriticGradFunction(torch.autograd.Function):
    """CriticFunction's backward as a function of (flat, xseq, g_score) -> (gflat, dx): one gmpc_critic_vjp call.  Under
    create_graph its own backward, for the cotangent v on dx, is one gmpc_critic_dir_vjp call with g_dir = g_score:
    sdot for g_score, `params` into the critic range of flat, dx for xs."""

    @staticmethod
    def forward(ctx, eng, crit, rng, xs, flat, xseq, g_score, want_params, want_dx):
        # (xs: the fp32 copy of xseq the layer's forward ran on; flat and xseq take part for the graph only)
        lo, cnt = rng
        gflat = torch.zeros(flat.shape, dtype=torch.float32, device=xs.device) if want_params else None
        g32 = g_score.detach().to(torch.float32).contiguous()
        out = eng.critic_vjp(xs, crit, g32, want_dx=want_dx, want_params=want_params,
                             grad_sum=gflat[lo:lo + cnt] if want_params else None)
        ctx.eng, ctx.crit, ctx.range, ctx.flat_shape = eng, crit, rng, flat.shape
        ctx.save_for_backward(xs, g32)
        ctx.set_materialize_grads(False)
        return gflat, out["dx"]

    @staticmethod
    @once_differentiable
    def backward(ctx, v_gflat, v_dx):
        if v_gflat is not None:
            raise NotImplementedError(
                "critic_layer: a cotangent on the parameter gradient (d2 score / d theta2, d2 score / d theta dx "
                "contracted on the theta side) is not implemented; only the input gradient dscore/dxseq is "
                "differentiable again")
        want_params, want_dx, want_g = ctx.needs_input_grad[4:7]
        if v_dx is None or not (want_params or want_dx or want_g):
            return (None,) * 9
        eng = ctx.eng
        if eng.ctx is None:
            raise RuntimeError("critic_layer double backward: the engine of the forward has been closed (the policy "
                               "rebuilt it for another shape or a larger batch)")
        xs, g32 = ctx.saved_tensors
        gflat = None
        if want_params:
            lo, cnt = ctx.range
            gflat = torch.zeros(ctx.flat_shape, dtype=torch.float32, device=xs.device)
        grads = want_params or want_dx
        out = eng.critic_dir_vjp(xs, ctx.crit, v_dx.detach().to(torch.float32).contiguous(),
                                 g_dir=g32 if grads else None, want_dx=want_dx, want_params=want_params,
                                 grad_sum=gflat[lo:lo + cnt] if want_params else None)
        return None, None, None, None, gflat, out["dx"], out["sdot"] if want_g else None, None, None


def critic_layer(policy, params, xseq):
    """score (Bc,) of the policy's critic on xseq (Bc, T+1, x_size), differentiable w.r.t. xseq and the critic_params
    range of params.flat (see the module docstring).  params: the policy's DeviceParams (a parameter tree is converted,
    and then is not differentiable); runs on the policy's engine as it is."""
    dparams = policy.to_device_params(params)
    Bc = xseq.shape[0]
    eng = policy._engine
    if eng is None:
        raise GmpcError(f"critic_layer: the policy has no engine for a batch of {Bc} yet; bind its parameters first "
                        "(policy.bind(params, batch))")
    if Bc > 2 * eng.max_batch:
        raise GmpcError(f"critic_layer: Bc = {Bc} sequences exceed 2 * max_batch = {2 * eng.max_batch} of the policy's "
                        f"engine (max_batch = {eng.max_batch}); bind the policy for a larger batch first")
    return CriticFunction.apply(eng, dparams, dparams.flat, xseq)
