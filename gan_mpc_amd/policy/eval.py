"""Evaluation policy (reference policy/eval.py:25-128): holds the models, builds the solver,
get_optimal_values / get_optimal_action.  Accepts one sample (hist+1, n) like the reference or a
batch (B, hist+1, n)."""

import numpy as np
import torch

from gan_mpc_amd import params as params_lib
from gan_mpc_amd.engine import ICEM_KWARGS, MPPI_KWARGS, TRAJAX_CEM_KWARGS, TRAJAX_iLQR_KWARGS, Engine
from gan_mpc_amd.policy import optimizers as opt
from gan_mpc_amd.policy.device_params import DeviceParams

COST_ARGS_NAME = ("goal_state",)


class LqrBlock:
    """The `lqr` slot of trajax' 7-tuple: a lazy handle on the ctx-resident dynamics linearisation
    [A_t | B_t] of the final iterate.  Nothing is copied (and the stream is not synchronised) until
    `.tensor()` is called; the reference never reads this slot (policy/optimizers.py:19-21 passes it
    through).  Shape (B, T, n, n+m) for n <= 64; the large-state backward pass is step-major and
    keeps one step only, so for n > 64 the block is (B, n, n+m): the Jacobians at t = 0.  Valid until
    the next call into the same engine."""

    def __init__(self, engine, batch, index=None):
        self._engine, self._batch, self._index = engine, int(batch), index

    @property
    def shape(self):
        e = self._engine
        full = (self._batch, e.T, e.n, e.n + e.m) if not e.big else (self._batch, e.n, e.n + e.m)
        return full if self._index is None else full[1:]

    def __getitem__(self, i):
        if self._index is not None or not isinstance(i, (int, np.integer)):
            return self.tensor()[i]          # slices, tuples, masks: plain tensor indexing
        if not -self._batch <= i < self._batch:
            raise IndexError(i)
        return LqrBlock(self._engine, self._batch, i % self._batch)

    def tensor(self):
        e = self._engine
        full = (self._batch, e.T, e.n, e.n + e.m) if not e.big else (self._batch, e.n, e.n + e.m)
        t = e.debug_buffer(5, full)
        return t if self._index is None else t[self._index]


class EvalMPC:
    SOLVERS = ("rounds", "fused", "box", "cem", "mppi", "icem")

    def __init__(self, config, cost_model, dynamics_model, expert_model,
                 trajax_ilqr_kwargs=TRAJAX_iLQR_KWARGS, device=None, solver="rounds", control_bounds=None,
                 cem_kwargs=None, mppi_kwargs=None, icem_kwargs=None, sampled_precision=None,
                 dynamics_ensemble=None, ensemble_mode=None, ensemble_disagreement=None):
        """solver: "rounds" -- gmpc_ilqr_solve, the host enqueues the iterations (every shape); "fused" --
        gmpc_ilqr_solve_fused, the whole solve in one kernel launch (MLP dynamics, n <= 64, m <= 32, T <= 32: the
        short-horizon / batch-1 MPC action); "box" -- gmpc_ilqr_solve_box, the one-launch solve with the controls
        limited to control_bounds = (lo, hi), each None, a scalar or one value per control; the training calls
        (loss_and_grad, batch_loss, ilqr_layer) use gmpc_ilqr_solve_box_held and differentiate through the solution's
        active set held fixed, the action path (get_optimal_values / get_optimal_action) the plain one;
        "cem" -- gmpc_cem_solve, the cross-entropy method under control_bounds with trajax' keywords cem_kwargs (DESIGN
        §20: MLP dynamics, any horizon; the action path only -- the training calls raise NotImplementedError; the seed
        advances by one per solve); "mppi" -- gmpc_mppi_solve, path-integral control under control_bounds with the
        keywords mppi_kwargs (engine.MPPI_KWARGS plus the policy keyword warm_start, default False: the next solve of
        the same batch shape starts from the previous U shifted one step), handled like "cem"; its
        training calls raise NotImplementedError too and name policy.differentiable.mppi_layer, the way to train;
        "icem" -- gmpc_icem_solve, the sample-efficient cross-entropy method under control_bounds with the keywords
        icem_kwargs (engine.ICEM_KWARGS plus the policy keyword shift_elites, default True: the next solve of the same
        batch shape carries the previous solve's kept rows, shifted one step), handled like "cem".
        sampled_precision: None, "fp32" or "bf16" -- with a "cem" / "mppi" / "icem" solver, the operand precision of
        the sampled rollouts (Engine.set_sampled_precision), set wherever the policy binds its engine;
        None leaves the engine's default, "fp32".
        dynamics_ensemble: None, or a sequence of 1 to 16 dynamics parameter trees shaped like
        params["dynamics_params"] -- with a "cem" / "mppi" / "icem" solver, the members of the dynamics ensemble the
        sampled rows are costed on (Engine.set_sampled_ensemble, DESIGN §24: a row's cost is its mean over the members;
        X and obj stay those of params["dynamics_params"]), set wherever the policy binds its engine.
        ensemble_mode: None, or a dict of Engine.set_sampled_ensemble_mode's keywords (aggregate, risk, propagation,
        particles) -- with a "cem" / "mppi" / "icem" solver, what the solver does with the ensemble: mean plus
        a multiple of the members' spread or the worst member instead of the mean, and particles that draw their member
        per step.  Set next to the ensemble wherever the policy binds its engine; without dynamics_ensemble it is
        accepted and inert.
        ensemble_disagreement: None, or a finite number -- with a "cem" / "mppi" / "icem" solver and a
        dynamics_ensemble, the penalty on the members' one-step disagreement with params["dynamics_params"] along every
        sampled row (Engine.set_sampled_disagreement, DESIGN §28: positive is pessimism, negative exploration), set
        next to ensemble_mode wherever the policy binds its engine.  Not with propagation "ts1"."""
        if solver not in self.SOLVERS:
            raise ValueError(f"solver must be one of {self.SOLVERS}, got {solver!r}")
        if (solver in ("box", "cem", "mppi", "icem")) != (control_bounds is not None):
            raise ValueError('control_bounds=(lo, hi) and solver="box" / "cem" / "mppi" / "icem" go together: got '
                             f"solver={solver!r}, control_bounds={control_bounds!r}")
        if cem_kwargs is not None and solver != "cem":
            raise ValueError(f'cem_kwargs and solver="cem" go together: got solver={solver!r}')
        if mppi_kwargs is not None and solver != "mppi":
            raise ValueError(f'mppi_kwargs and solver="mppi" go together: got solver={solver!r}')
        unknown = set(mppi_kwargs or {}) - set(MPPI_KWARGS) - {"warm_start"}
        if unknown:
            raise ValueError(f"mppi_kwargs has unknown keyword(s) {sorted(unknown)}")
        if icem_kwargs is not None and solver != "icem":
            raise ValueError(f'icem_kwargs and solver="icem" go together: got solver={solver!r}')
        unknown = set(icem_kwargs or {}) - set(ICEM_KWARGS) - {"shift_elites"}
        if unknown:
            raise ValueError(f"icem_kwargs has unknown keyword(s) {sorted(unknown)}")
        if sampled_precision is not None and solver not in ("cem", "mppi", "icem"):
            raise ValueError('sampled_precision and solver="cem" / "mppi" / "icem" go together: got '
                             f"solver={solver!r}")
        if sampled_precision not in (None, "fp32", "bf16"):
            raise ValueError(f'sampled_precision must be None, "fp32" or "bf16", got {sampled_precision!r}')
        if dynamics_ensemble is not None and solver not in ("cem", "mppi", "icem"):
            raise ValueError('dynamics_ensemble and solver="cem" / "mppi" / "icem" go together: got '
                             f"solver={solver!r}")
        if dynamics_ensemble is not None and len(dynamics_ensemble) == 0:
            raise ValueError("dynamics_ensemble must hold at least one dynamics parameter tree")
        if control_bounds is not None and len(control_bounds) != 2:
            raise ValueError(f"control_bounds must be a pair (lo, hi), got {control_bounds!r}")
        self.solver = solver
        self.ensemble_mode = self._checked_ensemble_mode(ensemble_mode)
        if ensemble_disagreement is not None:
            if solver not in ("cem", "mppi", "icem"):
                raise ValueError('ensemble_disagreement and solver="cem" / "mppi" / "icem" go together: got '
                                 f"solver={solver!r}")
            if dynamics_ensemble is None:
                raise ValueError("ensemble_disagreement needs a dynamics_ensemble: the penalty measures its members")
            if (self.ensemble_mode or {}).get("propagation", "fixed") == "ts1":
                raise ValueError('ensemble_disagreement does not go with ensemble_mode propagation "ts1"')
            if isinstance(ensemble_disagreement, bool) or not isinstance(
                    ensemble_disagreement, (int, float, np.integer, np.floating)) or not np.isfinite(
                    ensemble_disagreement):
                raise ValueError(f"ensemble_disagreement must be None or a finite number, got "
                                 f"{ensemble_disagreement!r}")
        self.ensemble_disagreement = None if ensemble_disagreement is None else float(ensemble_disagreement)
        self.control_bounds = None if control_bounds is None else tuple(control_bounds)
        self.config = config
        self.cost_model = cost_model
        self.dynamics_model = dynamics_model
        self.expert_model = expert_model
        self.trajax_ilqr_kwargs = dict(trajax_ilqr_kwargs)
        self.cem_kwargs = dict(TRAJAX_CEM_KWARGS, **(cem_kwargs or {}))
        self.cem_solves = 0       # solves issued by a "cem" policy: solve k runs under seed + k
        self.mppi_kwargs = {**MPPI_KWARGS, "warm_start": False, **(mppi_kwargs or {})}
        self.mppi_solves = 0      # the same for a "mppi" policy
        self._warm_U = None       # warm_start: the previous solve's clamped U
        self.icem_kwargs = {**ICEM_KWARGS, "shift_elites": True, **(icem_kwargs or {})}
        self.icem_solves = 0      # the same for an "icem" policy
        self._icem_state = None   # shift_elites: the previous solve's state (its kept rows)
        self.sampled_precision = sampled_precision
        # the members' flat vectors, stacked (P, dyn count); its device copy is made by the first bind
        self.dynamics_ensemble = None if dynamics_ensemble is None else np.stack(
            [params_lib.pack_mlp(tree) for tree in dynamics_ensemble])
        self._ensemble_dev = None
        self.critic_model = getattr(self, "critic_model", None)
        self._device = device
        self._engine = None
        self._engine_key = None
        self._bound = None
        self._single = None

    # ---- parameters -------------------------------------------------------------------------
    def init(self, mpc_weights, cost_args, dynamics_args, expert_args):
        params = {}
        params["mpc_weights"] = np.array(mpc_weights, dtype=np.float32)
        params["cost_params"] = self.cost_model.init(*cost_args)
        params["dynamics_params"] = self.dynamics_model.init(*dynamics_args)
        params["expert_params"] = self.expert_model.init(*expert_args)
        return params

    def reset_warm_start(self):
        """Forget the previous solve's controls: the next "mppi" solve starts from the expert's init_U again, the
        next "icem" solve carries no kept rows."""
        self._warm_U = None
        self._icem_state = None

    def device(self):
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    def to_device_params(self, params):
        return params if isinstance(params, DeviceParams) else DeviceParams.from_tree(params, self.device())

    # ---- engine -----------------------------------------------------------------------------
    def _shape_key(self, dparams):
        return (tuple(dparams.meta["dyn_dims"]), dparams.meta.get("dyn_lstm", 0), tuple(dparams.meta["cost_dims"]),
                None if dparams.meta["critic"] is None else
                (dparams.meta["critic"][1], tuple(dparams.meta["critic"][2])))

    def engine_for(self, batch, dparams=None):
        dparams = dparams or self._bound
        key = self._shape_key(dparams)
        if self._engine is None or self._engine_key != key or batch > self._engine.max_batch:
            if self._engine is not None:
                self._engine.close()
            dyn_dims, cost_dims = dparams.meta["dyn_dims"], dparams.meta["cost_dims"]
            n, m, nx, dyn_lstm = dparams.sizes_of_state()
            cr = dparams.meta["critic"]
            self._engine = Engine(n, m, self.config.mpc.horizon, dyn_dims, cost_dims,
                                  max_batch=max(batch, 8), lstm_features=cr[1] if cr else 0,
                                  head_dims=cr[2] if cr else None, device=self.device().index,
                                  dyn_lstm=dyn_lstm, x_size=nx)
            self._engine_key = key
            self._bound_ptr = None
        return self._engine

    def bind(self, dparams, batch=1):
        """Engine sized for `batch` with the ctx pointed at this parameter vector (rebuilds the
        transposed weight copies)."""
        self._bound = dparams
        eng = self.engine_for(batch, dparams)
        eng.set_params(dparams.view("mpc_weights"), dparams.view("dynamics_params"),
                       dparams.view("cost_params"))
        if self.sampled_precision is not None:
            eng.set_sampled_precision(self.sampled_precision)
        if self.dynamics_ensemble is not None:
            if self._ensemble_dev is None or self._ensemble_dev.device != eng.device:
                self._ensemble_dev = eng.to_dev(self.dynamics_ensemble)
            eng.set_sampled_ensemble(self._ensemble_dev)
        if self.ensemble_mode is not None:
            eng.set_sampled_ensemble_mode(**self.ensemble_mode)
        if self.ensemble_disagreement is not None:
            eng.set_sampled_disagreement(self.ensemble_disagreement)
        return eng

    ENSEMBLE_MODE_KEYS = ("aggregate", "risk", "propagation", "particles")

    def _checked_ensemble_mode(self, mode):
        """The constructor's / set_ensemble_mode's keywords as a dict, or None (the values are the engine's to check)."""
        if mode is None:
            return None
        if self.solver not in ("cem", "mppi", "icem"):
            raise ValueError('ensemble_mode and solver="cem" / "mppi" / "icem" go together: got '
                             f"solver={self.solver!r}")
        mode = dict(mode)
        unknown = set(mode) - set(self.ENSEMBLE_MODE_KEYS)
        if unknown:
            raise ValueError(f"ensemble_mode has unknown keyword(s) {sorted(unknown, key=str)}")
        return mode

    def set_ensemble_mode(self, **kw):
        """Replace the ensemble mode of a "cem" / "mppi" / "icem" policy (the constructor's ensemble_mode=) by
        Engine.set_sampled_ensemble_mode's keywords; none: the default mode.  Set on the bound engine now and by every
        later bind."""
        mode = self._checked_ensemble_mode(kw)
        if getattr(self, "ensemble_disagreement", None) is not None and (mode or {}).get("propagation") == "ts1":
            raise ValueError('ensemble_mode propagation "ts1" does not go with ensemble_disagreement')
        if self._engine is not None:
            self._engine.set_sampled_ensemble_mode(**mode)      # the engine checks the values: a refused mode is not kept
        self.ensemble_mode = mode

    def set_dynamics_ensemble(self, members):
        """Replace the dynamics ensemble of a "cem" / "mppi" / "icem" policy (the constructor's dynamics_ensemble=):
        None -- no ensemble --, a sequence of 1 to 16 dynamics parameter trees, or the members' flat vectors as a
        (P, dyn_count) float32 array or device tensor (norm/ensemble_trainer's; a device tensor is used as it is, not
        copied: train it further in place and call this again).  Set on the bound engine now and by every later bind."""
        if members is not None and self.solver not in ("cem", "mppi", "icem"):
            raise ValueError('dynamics_ensemble and solver="cem" / "mppi" / "icem" go together: got '
                             f"solver={self.solver!r}")
        dev = None
        if members is None:
            flat = None
        elif torch.is_tensor(members) or isinstance(members, np.ndarray):
            flat = members
            if len(members.shape) != 2 or not 1 <= members.shape[0] <= 16:
                raise ValueError("dynamics_ensemble must be (P, dyn_count) with 1 <= P <= 16, got shape "
                                 f"{tuple(members.shape)}")
            if members.dtype not in (torch.float32, np.dtype(np.float32)):
                raise ValueError(f"dynamics_ensemble must be float32, got {members.dtype}")
            if torch.is_tensor(members):
                dev = members if members.is_cuda else None
                flat = members.detach().cpu().numpy()
        else:
            if len(members) == 0:
                raise ValueError("dynamics_ensemble must hold at least one dynamics parameter tree")
            flat = np.stack([params_lib.pack_mlp(tree) for tree in members])
        self.dynamics_ensemble = flat
        self._ensemble_dev = dev
        eng = self._engine
        if eng is not None:
            if flat is None:
                eng.set_sampled_ensemble(None)
            else:
                if self._ensemble_dev is None or self._ensemble_dev.device != eng.device:
                    self._ensemble_dev = eng.to_dev(flat)
                eng.set_sampled_ensemble(self._ensemble_dev)

    # ---- reference API ----------------------------------------------------------------------
    def get_dynamics_carry(self, history_x, history_u, params):
        """reference policy/eval.py:75-85: the carry the dynamics model reaches after the history (empty
        for the MLP variant; the LSTM variant scans its cell over the (x_i, u_i) pairs from a zero carry).
        One sample (hist+1, nx) / (hist, m) or a batch with a leading axis."""
        hx = np.asarray(history_x, np.float32)
        single = hx.ndim == 2
        if single:
            hx = hx[None]
        zero = self.dynamics_model.get_zero_carry(hx[0, :-1])
        if zero.shape[-1] == 0 or history_u is None:
            carry = np.zeros((hx.shape[0], zero.shape[-1]), np.float32)
            return carry[0] if single else carry
        hu = np.asarray(history_u, np.float32)
        hu = hu[None] if hu.ndim == 2 else hu
        dparams = self.to_device_params(params)
        eng = self.bind(dparams, hx.shape[0])
        d = eng.to_dev
        carry = d(np.zeros((hx.shape[0], zero.shape[-1]), np.float32))
        for i in range(hu.shape[1]):          # dynamics_model.get_history_carry's fori_loop (:34-43)
            xc = torch.cat([d(hx[:, i]), carry], dim=1).contiguous()
            carry = eng.predict(xc, d(hu[:, i]))[:, hx.shape[-1]:].contiguous()
        return carry[0] if single else carry

    def get_goal_states_init_actions(self, history_X, params):
        """reference policy/eval.py:87-107, batched: history_X (B, hist+1, n) -> goal, init_U (host
        arrays from a table / hold expert, device tensors from the GPU sequence model)."""
        expert_params = params.expert_params if isinstance(params, DeviceParams) else params.get(
            "expert_params")
        if getattr(self.expert_model, "needs_engine", False):
            dparams = self.to_device_params(params)
            eng = self.engine_for(len(history_X), dparams)
            return self.expert_model.get_goal_states_init_actions(history_X, expert_params, engine=eng)
        return self.expert_model.get_goal_states_init_actions(history_X, expert_params)

    def _solve(self, params, history_X, history_U=None, hold=False):
        """hold: a "box" policy's solution is held for upper_loss / the bilevel tail (optimizers.ilqr_solve)."""
        dparams = self.to_device_params(params)
        hx = np.asarray(history_X, np.float32)
        goal, init_U = self.get_goal_states_init_actions(hx, dparams)
        eng = self.engine_for(hx.shape[0], dparams)
        d = eng.to_dev
        # xc = concat[x, carry] (policy/eval.py:118-123): empty for the MLP dynamics, (c, h) for the LSTM
        # variant -- from the history in the evaluation policy, zero in the training policy
        x0 = d(hx[:, -1])
        if eng.n > eng.nx:
            carry = self.get_dynamics_carry(hx, history_U, dparams)
            x0 = torch.cat([x0, d(carry)], dim=1).contiguous()
        sol = opt.ilqr_solve(self, dparams, x0, d(init_U), d(goal), hold=hold)
        return dparams, sol

    def get_optimal_values(self, params, history_x, history_u=None):
        """-> (X, U, obj, gradient, adjoints, lqr, iteration), the 7-tuple of trajax ilqr.  `lqr`
        is the device-resident [A_t | B_t] block of the final linearisation."""
        single = np.ndim(history_x) == 2
        hx = np.asarray(history_x, np.float32)[None] if single else history_x
        hu = None
        if history_u is not None:
            hu = np.asarray(history_u, np.float32)
            hu = hu[None] if single else hu
        _, sol = self._solve(params, hx, hu)
        B = sol["X"].shape[0]
        if self.solver in ("cem", "mppi", "icem"):  # no gradient, adjoints or linearisation; every problem runs max_iter iterations
            out = (sol["X"], sol["U"], sol["obj"], None, None, None, sol["iterations"])
            return tuple(o if o is None else o[0] for o in out) if single else out
        lqr = LqrBlock(self._engine, B)
        out = (sol["X"], sol["U"], sol["obj"], sol["grad"], sol["adjoints"], lqr, sol["iterations"])
        if single:
            out = tuple(o[0] for o in out)
        return out

    def get_optimal_action(self, params, history_x, history_u=None):
        _, useq, *_ = self.get_optimal_values(params, history_x, history_u)
        return useq[0] if useq.dim() == 2 else useq[:, 0]

    # ---- single-sample model evaluations (cost_model.get_cost / dynamics_model.predict) --------
    def _single_engine(self, dparams):
        key = self._shape_key(dparams)
        if self._single is None or self._single[0] != key:
            dyn_dims, cost_dims = dparams.meta["dyn_dims"], dparams.meta["cost_dims"]
            n, m, nx, dyn_lstm = dparams.sizes_of_state()
            eng = Engine(n, m, 1, dyn_dims, cost_dims, max_batch=8, device=self.device().index,
                         dyn_lstm=dyn_lstm, x_size=nx)
            self._single = (key, eng)
        eng = self._single[1]
        eng.set_params(dparams.view("mpc_weights"), dparams.view("dynamics_params"),
                       dparams.view("cost_params"))
        return eng

    def single_predict(self, xc, u, params):
        dparams = self.to_device_params(params)
        eng = self._single_engine(dparams)
        d = eng.to_dev
        x = np.asarray(xc, np.float32).reshape(1, -1)
        return eng.predict(d(x), d(np.asarray(u, np.float32).reshape(1, -1)))[0]

    def single_cost(self, xc, u, t, params, weights, goal_X):
        """cost_model.get_cost(xc, u, t, ...) with this policy's parameters: staging branch for t < horizon,
        terminal branch of the given state for t == horizon (reference cost/cost_model.py:33-42)."""
        dparams = self.to_device_params(params)
        if weights is not None:
            dparams = dparams.clone()
            dparams.view("mpc_weights").copy_(torch.as_tensor(np.asarray(weights, np.float32)))
        eng = self._single_engine(dparams)
        d = eng.to_dev
        x = np.asarray(xc, np.float32).reshape(1, -1)
        terminal = int(t) == self.config.mpc.horizon
        goal_row = None if terminal else d(np.asarray(goal_X, np.float32)[int(t)][None])
        return eng.get_cost(d(x), d(np.asarray(u, np.float32).reshape(1, -1)), goal_row, terminal)[0]

    # the two callbacks the reference hands to trajax (policy/eval.py:64-73), one sample at a time
    def cost(self, xc, u, t, params, goal_X):
        return self.single_cost(xc, u, t, params, None, goal_X)

    def dynamics(self, xc, u, t, params):
        del t
        return self.single_predict(xc, u, params)
