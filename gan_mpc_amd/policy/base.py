"""Training-time policy (reference policy/base.py:12-128): zero dynamics carry, loss_and_grad =
batched bilevel optimisation + batch mean (+ the multi-GPU all-reduce at exactly that mean)."""

import numpy as np
import torch

from gan_mpc_amd import parallel
from gan_mpc_amd import params as params_lib
from gan_mpc_amd.engine import TRAJAX_iLQR_KWARGS
from gan_mpc_amd.policy import eval as eval_policy
from gan_mpc_amd.policy import optimizers as opt


class BaseMPC(eval_policy.EvalMPC):
    # 0: L2, 1: JS generator (the kernels' own losses); None: the subclass's torch `loss`, differentiated per
    # trajectory under torch.func (optimizers.loss_cotangents)
    LOSS_KIND = None

    def __init__(self, config, cost_model, dynamics_model, expert_model, loss_vmap=(0,),
                 trajax_ilqr_kwargs=TRAJAX_iLQR_KWARGS, device=None, bilevel_sign=1.0, solver="rounds",
                 control_bounds=None, cem_kwargs=None, mppi_kwargs=None, icem_kwargs=None,
                 sampled_precision=None, dynamics_ensemble=None, ensemble_mode=None, ensemble_disagreement=None):
        super().__init__(config=config, cost_model=cost_model, dynamics_model=dynamics_model,
                         expert_model=expert_model, trajax_ilqr_kwargs=trajax_ilqr_kwargs,
                         device=device, solver=solver, control_bounds=control_bounds, cem_kwargs=cem_kwargs,
                         mppi_kwargs=mppi_kwargs, icem_kwargs=icem_kwargs, sampled_precision=sampled_precision,
                         dynamics_ensemble=dynamics_ensemble, ensemble_mode=ensemble_mode,
                         ensemble_disagreement=ensemble_disagreement)
        self.loss_vmap = loss_vmap
        # +1 reproduces the reference as written; -1 is the implicit-function gradient
        self.bilevel_sign = float(bilevel_sign)

    def get_dynamics_carry(self, history_x, *args):
        """reference policy/base.py:31-38: the training policy always starts from the zero carry."""
        del args
        hx = np.asarray(history_x)
        zero = self.dynamics_model.get_zero_carry(hx[..., :-1, :] if hx.ndim == 2 else hx[0, :-1])
        return zero if hx.ndim == 2 else np.zeros((hx.shape[0], zero.shape[-1]), np.float32)

    def get_optimal_values(self, params, history_x, *args):
        del args
        return super().get_optimal_values(params, history_x)

    def plan_spread(self, params, x, U):
        """Where the members of the policy's dynamics ensemble disagree along a plan (Engine.ensemble_rollout, DESIGN.md
        section 27): x (B, n) initial states, U (B, T, m) controls.  -> (X_members (P, B, T+1, n), the members'
        predicted states; disagreement (B, T+1), the members' population variance per step summed over the state
        entries).  Forward only: a disagreement bonus or penalty, or a check before acting."""
        if self.dynamics_ensemble is None:
            raise ValueError("plan_spread needs a dynamics_ensemble (the constructor's, or set_dynamics_ensemble): "
                             "none is set")
        xs, Us = tuple(getattr(x, "shape", np.shape(x))), tuple(getattr(U, "shape", np.shape(U)))
        if len(xs) != 2 or len(Us) != 3 or Us[0] != xs[0]:
            raise ValueError(f"plan_spread: x must be (B, n) and U (B, T, m), got {xs} and {Us}")
        eng = self.bind(self.to_device_params(params), xs[0])
        out = eng.ensemble_rollout(self._ensemble_dev, eng.to_dev(x), eng.to_dev(U), want=("X", "var"))
        return out["X"], out["var"].sum(-1)

    def closed_loop_spread(self, params, x, U, goal, x0=None, members=None, feedforward=False):
        """Where the members of a dynamics ensemble end up when each of them TRACKS a plan with the plan's own iLQR
        gains (Engine.ensemble_rollout_feedback): x (B, n) the states the plan starts from, U
        (B, T, m) its controls, goal (B, T+1, n).  The plan is rolled out from x under params["dynamics_params"]
        (Engine.rollout_cost), the time-varying gains K (and k) are those of Engine.lqr_backward at that trajectory,
        and every member then applies u_t = U_t + K_t (x_t - X_t) (+ k_t with feedforward=True) from x0 (B, n), default
        x, clamped to the policy's control_bounds when it has them.  members: None -- the policy's dynamics_ensemble
        (a "cem" / "mppi" / "icem" policy) --, or an explicit (P, dyn_count) float32 array or tensor, or a sequence of
        dynamics parameter trees: the way in for the iLQR policies, which hold no ensemble.  -> (X_members
        (P, B, T+1, n), U_members (P, B, T, m) the controls each member applied, spread (B, T+1) the members'
        population variance per step summed over the state entries).  Forward only.  On a "box" policy the gains are
        the unconstrained ones (lqr_backward knows no bounds) and the clamp does the rest: a saturated control does not
        feed back."""
        if members is None:
            if self.dynamics_ensemble is None:
                raise ValueError("closed_loop_spread needs members= or a dynamics_ensemble (the constructor's, or "
                                 "set_dynamics_ensemble): neither is there")
        elif not (torch.is_tensor(members) or isinstance(members, np.ndarray)):
            if len(members) == 0:
                raise ValueError("closed_loop_spread: members must hold at least one dynamics parameter tree")
            members = np.stack([params_lib.pack_mlp(tree) for tree in members]).astype(np.float32)
        xs, Us, gs = (tuple(getattr(a, "shape", np.shape(a))) for a in (x, U, goal))
        if len(xs) != 2 or len(Us) != 3 or Us[0] != xs[0] or len(gs) != 3 or gs[0] != xs[0]:
            raise ValueError(f"closed_loop_spread: x must be (B, n), U (B, T, m) and goal (B, T+1, n), got {xs}, {Us} "
                             f"and {gs}")
        if x0 is not None and tuple(getattr(x0, "shape", np.shape(x0))) != xs:
            raise ValueError(f"closed_loop_spread: x0 must be {xs} as x is, got "
                             f"{tuple(getattr(x0, 'shape', np.shape(x0)))}")
        eng = self.bind(self.to_device_params(params), xs[0])
        d = eng.to_dev
        x, U, goal = d(x), d(U), d(goal)
        X, _ = eng.rollout_cost(x, U, goal)
        gains = eng.lqr_backward(X, U, goal, after_rollout=True)
        lo = hi = None
        if self.control_bounds is not None:
            lo, hi = self.control_bounds
            lo, hi = (-np.inf if lo is None else lo), (np.inf if hi is None else hi)
        out = eng.ensemble_rollout_feedback(
            self._ensemble_dev if members is None else members, X, U, gains["K"], x0=x if x0 is None else d(x0),
            k=gains["k"] if feedforward else None, u_lo=lo, u_hi=hi, want=("X", "U", "var"))
        return out["X"], out["U"], out["var"].sum(-1)

    def plan_disagreement(self, params, x, U):
        """The one-step disagreement of the policy's dynamics ensemble with params["dynamics_params"] along a plan
        (Engine.ensemble_disagreement): x (B, n) initial states, U (B, T, m) controls.  -> (d
        (P, B, T), member p's squared one-step deviation from the nominal model at every step of the nominal rollout;
        D (P, B), its sum over the steps -- what ensemble_disagreement=penalty adds to a row's cost, per unit of
        penalty).  Forward only."""
        if self.dynamics_ensemble is None:
            raise ValueError("plan_disagreement needs a dynamics_ensemble (the constructor's, or "
                             "set_dynamics_ensemble): none is set")
        xs, Us = tuple(getattr(x, "shape", np.shape(x))), tuple(getattr(U, "shape", np.shape(U)))
        if len(xs) != 2 or len(Us) != 3 or Us[0] != xs[0]:
            raise ValueError(f"plan_disagreement: x must be (B, n) and U (B, T, m), got {xs} and {Us}")
        eng = self.bind(self.to_device_params(params), xs[0])
        out = eng.ensemble_disagreement(self._ensemble_dev, eng.to_dev(x), eng.to_dev(U), want=("d", "D"))
        return out["d"], out["D"]

    RISK_AGGREGATES = ("mean", "mean_std", "max")

    @staticmethod
    def _risk(J, aggregate, risk):
        """DESIGN.md section 26's aggregate of the members' objectives J (P, B) -> (R (B,), dR/dJ (P, B)): mean; mean +
        risk * the population standard deviation; max (the first member that attains it)."""
        P = J.shape[0]
        mean = J.sum(0) / P
        if aggregate == "mean":
            return mean, torch.full_like(J, 1.0 / P)
        if aggregate == "mean_std":
            d = J - mean
            sd = torch.sqrt((d * d).sum(0) / P)
            w = 1.0 / P + risk * d / (P * torch.where(sd > 0, sd, torch.ones_like(sd)))
            return mean + risk * sd, w
        R, arg = J.max(0)
        return R, torch.zeros_like(J).scatter_(0, arg[None], 1.0)

    def _plan_risk(self, eng, x, U, goal, aggregate, risk, grad):
        out = eng.ensemble_rollout(self._ensemble_dev, x, U, goal, want=("X", "costs") if grad else ("costs",))
        R, w = self._risk(out["costs"].sum(-1), aggregate, float(risk))
        if not grad:
            return R, None
        gcost = w[:, :, None].expand(-1, -1, out["costs"].shape[2]).contiguous()
        return R, eng.ensemble_rollout_vjp(self._ensemble_dev, out["X"], U, goal, gcost=gcost, want=("U",))["U"]

    def _risk_engine(self, who, params, x, U, goal, aggregate):
        if self.dynamics_ensemble is None:
            raise ValueError(f"{who} needs a dynamics_ensemble (the constructor's, or set_dynamics_ensemble): "
                             "none is set")
        if aggregate not in self.RISK_AGGREGATES:
            raise ValueError(f"{who}: aggregate must be one of {self.RISK_AGGREGATES}, got {aggregate!r}")
        xs, Us, gs = (tuple(getattr(a, "shape", np.shape(a))) for a in (x, U, goal))
        if len(xs) != 2 or len(Us) != 3 or Us[0] != xs[0] or len(gs) != 3 or gs[0] != xs[0]:
            raise ValueError(f"{who}: x must be (B, n), U (B, T, m) and goal (B, T+1, n), got {xs}, {Us} and {gs}")
        eng = self.bind(self.to_device_params(params), xs[0])
        return eng, eng.to_dev(x), eng.to_dev(U), eng.to_dev(goal)

    def _plan_risk_penalised(self, eng, x, U, goal, aggregate, risk, grad, penalty):
        """plan_risk under the one-step disagreement penalty: the planes J_0 + penalty * D_p of
        section 28 -- J_0 the nominal rollout's objective, the product rounded before it is added -- under section
        26's aggregate; dR/dU = (sum_p w_p) dJ_0/dU + penalty * sum_p w_p dD_p/dU with w = dR/dJ_p: one
        Engine.rollout_vjp under gcost and one Engine.ensemble_disagreement_vjp under gD = penalty * w."""
        X, costs = eng.rollout_cost(x, U, goal)
        D = eng.ensemble_disagreement(self._ensemble_dev, x, U, want=("D",))["D"]
        R, w = self._risk(costs.sum(-1)[None] + penalty * D, aggregate, float(risk))
        if not grad:
            return R, None
        gcost = w.sum(0)[:, None].expand(-1, costs.shape[1]).contiguous()
        g = eng.rollout_vjp(X, U, goal, None, gcost, want_x0=False, want_goal=False, want_theta=False,
                            want_dyn=False)["U"]
        gD = (penalty * w).contiguous()
        return R, g + eng.ensemble_disagreement_vjp(self._ensemble_dev, X, U, gD=gD, want=("U",))["U"]

    def _plan_objective(self, eng, x, U, goal, aggregate, risk, grad, disagreement):
        if disagreement is None:
            return self._plan_risk(eng, x, U, goal, aggregate, risk, grad)
        return self._plan_risk_penalised(eng, x, U, goal, aggregate, risk, grad, disagreement)

    @staticmethod
    def _check_disagreement(who, disagreement):
        if disagreement is None:
            return None
        penalty = float(disagreement)
        if not np.isfinite(penalty):
            raise ValueError(f"{who}: disagreement must be None or a finite number, got {disagreement!r}")
        return penalty

    def plan_risk(self, params, x, U, goal, aggregate="mean", risk=0.0, grad=False, disagreement=None):
        """The risk of a plan under the policy's dynamics ensemble: R (B,) = the aggregate --
        "mean", "mean_std" (mean + risk * standard deviation) or "max", section 26's formulas -- of the members'
        objectives, each the sum of the member's per-step costs against goal (B, T+1, n) for x (B, n), U (B, T, m).
        grad=True: -> (R, dR/dU (B, T, m)), one Engine.ensemble_rollout_vjp call behind the rollout.
        disagreement=penalty (a finite number): the objective a policy built with
        ensemble_disagreement=penalty chooses its plan on instead -- the aggregate of J_0 + penalty * D_p, J_0 the
        objective of the rollout under params["dynamics_params"], D_p member p's summed one-step disagreement with it."""
        disagreement = self._check_disagreement("plan_risk", disagreement)
        eng, x, U, goal = self._risk_engine("plan_risk", params, x, U, goal, aggregate)
        R, g = self._plan_objective(eng, x, U, goal, aggregate, risk, grad, disagreement)
        return (R, g) if grad else R

    def refine_plan(self, params, x, U, goal, steps=5, step_size=0.1, aggregate="mean", risk=0.0, disagreement=None):
        """Polish a plan by projected gradient steps on its ensemble risk (plan_risk): per step U <- clamp(U - a g),
        g = dR/dU, clamped to the policy's control bounds when set.  Backtracking per problem: a starts at step_size and
        is halved at most 10 times until the problem's R strictly decreases; a problem that finds no such a keeps its U.
        Every round is one batched forward call.  -> (U' (B, T, m), R_before (B,), R_after (B,)).  disagreement: as
        for plan_risk -- pass the policy's ensemble_disagreement penalty to polish the objective its solver chose the
        plan on."""
        disagreement = self._check_disagreement("refine_plan", disagreement)
        eng, x, U, goal = self._risk_engine("refine_plan", params, x, U, goal, aggregate)
        lo = hi = None
        if self.control_bounds is not None:
            lo, hi = (torch.as_tensor(np.asarray(b, np.float32), device=U.device) for b in self.control_bounds)
        U = U.clone()
        R = R_before = self._plan_objective(eng, x, U, goal, aggregate, risk, False, disagreement)[0]
        for _ in range(int(steps)):
            _, g = self._plan_objective(eng, x, U, goal, aggregate, risk, True, disagreement)
            alpha = torch.full_like(R, float(step_size))
            done = torch.zeros_like(R, dtype=torch.bool)
            U_next, R_next = U, R
            for _ in range(11):
                cand = U - alpha[:, None, None] * g
                if lo is not None:
                    cand = torch.minimum(torch.maximum(cand, lo), hi)
                Rc = self._plan_objective(eng, x, cand.contiguous(), goal, aggregate, risk, False, disagreement)[0]
                take = (Rc < R) & ~done
                U_next = torch.where(take[:, None, None], cand, U_next)
                R_next = torch.where(take, Rc, R_next)
                done = done | take
                if bool(done.all()):
                    break
                alpha = torch.where(done, alpha, alpha * 0.5)
            U, R = U_next.contiguous(), R_next
        return U, R_before, R

    def loss(self, xcseq, useq, params, *args):
        """The upper-level loss of ONE trajectory (reference policy/base.py:84-85): xcseq (T+1, n) -- xc, carry
        columns included --, useq (T, m), params the device parameters; a scalar torch tensor.  A subclass with
        LOSS_KIND None overrides it with torch operations that torch.func can vmap and differentiate."""
        raise NotImplementedError

    def batch_cotangents(self, X, U, dparams, loss_args, want_grad=True):
        """Optional: the upper-level loss of the WHOLE batch and its cotangents, (loss [B], lx (B, T+1, n) or None,
        lu (B, T, m) or None) as contiguous fp32 device tensors (lx, lu None without want_grad; a cotangent that is
        identically zero is None).  A subclass that overrides it is asked here instead of LOSS_KIND / loss(): for
        losses that go through another layer (gan/gan_policy.py: the critic) rather than per-trajectory torch code."""
        raise NotImplementedError

    def _batched_loss(self):
        return type(self).batch_cotangents is not BaseMPC.batch_cotangents

    def _custom_loss(self):
        """True for the subclass's own torch loss; NotImplementedError when there is no loss at all."""
        if self.LOSS_KIND is not None or self._batched_loss():
            return False
        if type(self).loss is BaseMPC.loss:
            raise NotImplementedError(f"{type(self).__name__} sets no LOSS_KIND and does not override loss()")
        return True

    def batch_loss(self, dparams, history_X, desired):
        """mean over the (global) batch of loss(iLQR(x)) -- norm/cost_trainer.py:13-21."""
        opt.refuse_cem(self, "batch_loss")
        custom = self._custom_loss()
        B = len(history_X)
        packed = parallel.new_packed(1, self.device(), B)
        if B > 0:            # an empty shard still joins the exchange, with count 0
            dparams, sol = self._solve(dparams, history_X, hold=True)
            eng = self._engine
            if self._batched_loss():
                loss, _, _ = self.batch_cotangents(sol["X"], sol["U"], dparams, (desired,), want_grad=False)
            elif custom:       # the reference's jax.vmap(policy.loss, in_axes=(0, 0, None, 0))
                loss, _, _ = opt.loss_cotangents(self.loss, sol["X"], sol["U"], dparams, (desired,),
                                                 (0 if desired is not None else None,), want_grad=False)
            else:
                crit = dparams.view("critic_params") if self.LOSS_KIND == 1 else None
                loss = eng.upper_loss(B, self.LOSS_KIND, desired=eng.to_dev(desired) if desired is not None
                                      else None, critic=crit)
            torch.sum(loss, dim=0, keepdim=True, out=packed[:1])
        return parallel.allreduce_mean_from_sums(packed)[0]

    def loss_and_grad(self, history_X, params, batch_loss_args):
        """reference policy/base.py:87-128.  history_X (B, hist+1, n) is THIS rank's shard;
        returns (avg_loss, grads) where grads is a flat device vector over [mpc_weights | cost_params]
        (every other leaf's gradient is exactly zero in the reference), both averaged
        over the global batch."""
        opt.refuse_cem(self, "loss_and_grad")
        custom = self._custom_loss()
        dparams = self.to_device_params(params)
        hx = np.asarray(history_X, np.float32)
        B = hx.shape[0]
        # [loss_sum | grad_sum | sample count]: the kernels write into views of the exchange buffer
        packed = parallel.new_packed(1 + 3 + dparams.sizes["cost_params"], self.device(), B)
        if B > 0:            # an empty shard still joins the exchange, with count 0
            goal, init_U = self.get_goal_states_init_actions(hx, dparams)
            eng = self.engine_for(B, dparams)
            d = eng.to_dev
            desired = (d(batch_loss_args[0]) if batch_loss_args and batch_loss_args[0] is not None
                       else None)
            x0 = d(hx[:, -1])
            if eng.n > eng.nx:       # xc = concat[x, carry], the training policy's carry is zero (:31-38, :101-102)
                x0 = torch.cat([x0, d(self.get_dynamics_carry(hx))], dim=1).contiguous()
            if self._batched_loss():
                args = tuple(batch_loss_args or ())
                loss, _, _, _ = opt.bilevel_optimization(
                    self, dparams, x0, d(init_U), d(goal), None, sign=self.bilevel_sign, grad_sum=packed[1:-1],
                    cotangents=lambda X, U: self.batch_cotangents(X, U, dparams, args))
            elif custom:     # loss(xcseq, useq, params, *batch_loss_args), vmapped over (0, 0, None) + loss_vmap
                loss, _, _, _ = opt.bilevel_optimization(
                    self, dparams, x0, d(init_U), d(goal), self.loss, sign=self.bilevel_sign,
                    grad_sum=packed[1:-1], loss_args=tuple(batch_loss_args or ()), loss_vmap=self.loss_vmap)
            else:
                loss, _, _, _ = opt.bilevel_optimization(
                    self, dparams, x0, d(init_U), d(goal), self.LOSS_KIND, desired=desired,
                    sign=self.bilevel_sign, grad_sum=packed[1:-1])
            torch.sum(loss, dim=0, keepdim=True, out=packed[:1])
        means = parallel.allreduce_mean_from_sums(packed)
        return means[0], means[1:]
