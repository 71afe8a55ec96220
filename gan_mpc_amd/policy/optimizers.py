"""Trajectory optimiser entry points with the reference's names (reference policy/optimizers.py).

The reference passes `cost` / `dynamics` callables to trajax; here the iLQR loop, the model
evaluations and their derivatives are fused HIP kernels behind the C ABI, so the callables are
replaced by the policy object that owns the engine and the bound parameters.  Everything is batched
over the leading axis (the reference's jax.vmap axis)."""

import functools

import torch


def _solver(policy, eng, hold=False):
    """The engine entry point of the policy's solver: "rounds" (gmpc_ilqr_solve, host-driven iterations), "fused"
    (gmpc_ilqr_solve_fused, the whole solve in one launch) or "box" (the one-launch solve under the policy's
    control_bounds: gmpc_ilqr_solve_box, or with hold=True gmpc_ilqr_solve_box_held, whose solution the bilevel tail
    may follow).  "rounds" and "fused" always hold their solution; "cem" (gmpc_cem_solve under the same bounds) holds none and refuses
    hold=True."""
    solver = getattr(policy, "solver", "rounds")
    if solver in ("cem", "mppi", "icem"):      # ("mppi": gmpc_mppi_solve, "icem": gmpc_icem_solve, handled like "cem")
        if hold:
            refuse_cem(policy, "a solve held for the bilevel tail")
        return functools.partial({"cem": _cem_solve, "mppi": _mppi_solve, "icem": _icem_solve}[solver], policy, eng)
    if solver == "box":
        lo, hi = policy.control_bounds
        return functools.partial(_box_solve_held if hold else _box_solve, eng, lo, hi)
    return eng.ilqr_solve_fused if solver == "fused" else eng.ilqr_solve


def refuse_cem(policy, what):
    """The training calls of a "cem" policy: the sampler has no derivative (raised before any device work)."""
    if getattr(policy, "solver", "rounds") == "mppi":
        raise NotImplementedError(f'solver="mppi": {what} does not go through the sampler; train through '
                                  "policy.differentiable.mppi_layer, which differentiates the path-integral solve")
    if getattr(policy, "solver", "rounds") in ("cem", "icem"):
        raise NotImplementedError(f'solver="{policy.solver}" has no gradient through the sampler: {what} needs an '
                                  'iLQR solver ("rounds", "fused" or "box")')


def _cem_solve(policy, eng, x0, U, goal, kwargs=None):
    """The policy's CEM solve in the shape of an iLQR solve's dict (no grad / adjoints; iterations = max_iter); kwargs
    (the iLQR keyword set of the caller) does not apply.  Solve k of the policy runs under seed + k.  The engine's
    mean is trajax' -- not clipped: a start outside the bounds decays by evolution_smoothing per iteration only, and a
    mean of controls on a bound may pass it by a rounding -- so the policy, whose controls go to an actuator, clamps
    the start before the solve and U after it (X and obj are those of the mean: the same up to that rounding)."""
    del kwargs
    lo, hi = policy.control_bounds
    kw = dict(policy.cem_kwargs)
    kw["seed"] = int(kw["seed"]) + policy.cem_solves
    policy.cem_solves += 1
    _, _, lo_t, hi_t = eng._device_bounds(lo, hi)      # (the cached device copies the solve itself uses)
    clamp = (lambda t: t) if lo_t is None and hi_t is None else (lambda t: torch.clamp(t, min=lo_t, max=hi_t))
    sol = eng.cem_solve(x0, clamp(U), goal, lo, hi, kw)
    sol["U"] = clamp(sol["U"])
    sol["iterations"] = torch.full((x0.shape[0],), int(kw["max_iter"]), dtype=torch.int32, device=x0.device)
    return sol


def shift_warm_start(U):
    """U (B, T, m) shifted one step towards the horizon's end, the last row repeated: the next solve's start."""
    return torch.cat([U[:, 1:], U[:, -1:]], dim=1).contiguous()


def _mppi_solve(policy, eng, x0, U, goal, kwargs=None):
    """The policy's MPPI solve, handled like _cem_solve: the start clamped, U clamped after the solve, solve k under
    seed + k.  With mppi_kwargs["warm_start"] the start is the previous solve's U of the same batch shape, shifted one
    step (shift_warm_start), instead of the expert's U; policy.reset_warm_start() drops it."""
    del kwargs
    lo, hi = policy.control_bounds
    kw = dict(policy.mppi_kwargs)
    warm = bool(kw.pop("warm_start"))
    kw["seed"] = int(kw["seed"]) + policy.mppi_solves
    policy.mppi_solves += 1
    _, _, lo_t, hi_t = eng._device_bounds(lo, hi)
    clamp = (lambda t: t) if lo_t is None and hi_t is None else (lambda t: torch.clamp(t, min=lo_t, max=hi_t))
    prev = policy._warm_U
    if warm and prev is not None and prev.shape == U.shape and prev.device == U.device:
        U = shift_warm_start(prev)
    sol = eng.mppi_solve(x0, clamp(U), goal, lo, hi, kw)
    sol["U"] = clamp(sol["U"])
    policy._warm_U = sol["U"] if warm else None
    sol["iterations"] = torch.full((x0.shape[0],), int(kw["max_iter"]), dtype=torch.int32, device=x0.device)
    return sol


def _icem_solve(policy, eng, x0, U, goal, kwargs=None):
    """The policy's iCEM solve, handled like _cem_solve: the start clamped, U clamped after the solve (the best row is
    inside the bounds already; the mean, returned where no cost was finite, need not be), solve k under seed + k.  With
    icem_kwargs["shift_elites"] the next solve of the same batch shape carries the previous solve's kept rows, shifted
    one step (shift_warm_start per row), as carry_in = num_keep; the best cost starts at +inf in every solve, since the
    best row of another state prices nothing here.  policy.reset_warm_start() drops the kept rows."""
    del kwargs
    lo, hi = policy.control_bounds
    kw = dict(policy.icem_kwargs)
    shift = bool(kw.pop("shift_elites"))
    kw["seed"] = int(kw["seed"]) + policy.icem_solves
    policy.icem_solves += 1
    _, _, lo_t, hi_t = eng._device_bounds(lo, hi)
    clamp = (lambda t: t) if lo_t is None and hi_t is None else (lambda t: torch.clamp(t, min=lo_t, max=hi_t))
    prev, state = policy._icem_state, None
    if shift and prev is not None and prev["best_U"].shape == U.shape and prev["best_U"].device == U.device:
        keep = prev["keep"]
        state = dict(keep=shift_warm_start(keep.flatten(0, 1)).reshape(keep.shape),
                     best_U=prev["best_U"], best_cost=torch.full_like(prev["best_cost"], float("inf")))
    sol = eng.icem_solve(x0, clamp(U), goal, lo, hi, kw, state=state)
    sol["U"] = clamp(sol["U"])
    policy._icem_state = sol["state"] if shift else None
    sol["iterations"] = torch.full((x0.shape[0],), int(kw["max_iter"]), dtype=torch.int32, device=x0.device)
    return sol


def _box_solve(eng, lo, hi, x0, U, goal, kwargs=None):
    return eng.ilqr_solve_box(x0, U, goal, lo, hi, kwargs)


def _box_solve_held(eng, lo, hi, x0, U, goal, kwargs=None):
    return eng.ilqr_solve_box_held(x0, U, goal, lo, hi, kwargs)


def ilqr_solve(policy, dparams, x0, U, goal, trajax_ilqr_kwargs=None, hold=False):
    """reference policy/optimizers.py:10-21 -> trajax ilqr.  Device tensors in, dict of device
    tensors out: X, U, obj, grad, adjoints, iterations (the `lqr` tuple stays in the ctx).  hold: a "box" policy's
    solution is held for upper_loss / the bilevel tail (the other solvers always hold theirs)."""
    eng = policy.bind(dparams, x0.shape[0])
    return _solver(policy, eng, hold=hold)(x0, U, goal, trajax_ilqr_kwargs or policy.trajax_ilqr_kwargs)


def bilevel_optimization(policy, dparams, x0, init_U, goal, loss_kind, desired=None,
                         trajax_ilqr_kwargs=None, sign=1.0, grad_sum=None, loss_args=(), loss_vmap=None,
                         cotangents=None):
    """reference policy/optimizers.py:34-75, batched, WITHOUT the batch mean: returns
    (loss [B], low_level_grad [B,T,m], grad_sum [3 + cost_count] summed over the batch, itr [B]).
    sign=+1 reproduces the reference as written.  Under a "box" policy the gradient is the implicit
    one through the solution's active set held fixed.

    loss_kind 0 (L2, against `desired`) and 1 (JS, the policy's critic) run on the kernels' own losses.  A
    callable is the reference's `loss(X, U, params, *loss_args)` of ONE trajectory: it is evaluated and
    differentiated per trajectory under torch.func.vmap (loss_cotangents; loss_vmap: the in_dims of loss_args,
    default 0 for each), its cotangents go to gmpc_bilevel_grad_cotangent.

    cotangents (loss_kind is then ignored): a callable (X, U) -> (loss [B], lx (B, T+1, n) or None, lu (B, T, m) or
    None) for the whole batch at once, for a loss that is not a vmap of per-trajectory torch code (BaseMPC.
    batch_cotangents); a None cotangent is passed on as NULL, not as zeros."""
    refuse_cem(policy, "bilevel_optimization")
    B = x0.shape[0]
    eng = policy.bind(dparams, B)
    sol = _solver(policy, eng, hold=True)(x0, init_U, goal, trajax_ilqr_kwargs or policy.trajax_ilqr_kwargs)
    if cotangents is not None or callable(loss_kind):
        if cotangents is not None:
            loss, lx, lu = cotangents(sol["X"], sol["U"])
        else:
            loss, lx, lu = loss_cotangents(loss_kind, sol["X"], sol["U"], dparams, loss_args, loss_vmap)
        grad_sum = eng.bilevel_grad_cotangent(B, lx, lu, sign=sign, grad_sum=grad_sum)
        return loss, sol["grad"], grad_sum, sol["iterations"]
    critic = dparams.view("critic_params") if loss_kind == 1 else None
    loss, grad_sum = eng.bilevel_grad(B, loss_kind, desired=desired, critic=critic, sign=sign,
                                      grad_sum=grad_sum)
    return loss, sol["grad"], grad_sum, sol["iterations"]


def loss_cotangents(loss, X, U, params, loss_args=(), loss_vmap=None, want_grad=True):
    """Per-trajectory values and cotangents of a caller-defined upper-level loss, the reference's
    jax.vmap(loss, in_axes=(0, 0, None) + loss_vmap) with jax.grad wrt (X, U): `loss(x, u, params, *args)` takes one
    trajectory x (T+1, n), u (T, m) and returns a scalar.  X (B, T+1, n), U (B, T, m); `params` is passed unmapped
    and not differentiated (the reference drops the loss's direct parameter dependence as well); loss_args mapped
    over loss_vmap (an int or None per argument; default 0 each), arrays moved to X's device.
    -> (loss [B], lx [B, T+1, n], lu [B, T, m]) as contiguous fp32 tensors; lx, lu None without want_grad."""
    from torch.func import grad_and_value, vmap

    loss_args = tuple(loss_args)
    loss_vmap = (0,) * len(loss_args) if loss_vmap is None else tuple(loss_vmap)
    if len(loss_vmap) != len(loss_args):
        raise ValueError(f"loss_vmap has {len(loss_vmap)} entries for {len(loss_args)} loss arguments")
    args = tuple(a if d is None else _as_tensor(a, X.device) for a, d in zip(loss_args, loss_vmap))
    in_dims = (0, 0, None) + loss_vmap
    B = X.shape[0]
    if not want_grad:
        val = vmap(loss, in_dims=in_dims)(X, U, params, *args)
        return _per_sample(val, B), None, None
    (lx, lu), val = vmap(grad_and_value(loss, argnums=(0, 1)), in_dims=in_dims)(X, U, params, *args)
    f32 = lambda t: t.to(torch.float32).contiguous()  # noqa: E731
    return _per_sample(val, B), f32(lx), f32(lu)


def _as_tensor(a, device):
    t = torch.as_tensor(a, device=device) if not torch.is_tensor(a) else a.to(device)
    return t.to(torch.float32) if t.is_floating_point() else t


def _per_sample(val, B):
    if tuple(val.shape) != (B,):
        raise ValueError(f"the loss must return a scalar per trajectory, got shape {tuple(val.shape[1:])}")
    return val.to(torch.float32).contiguous()
