"""Thin host wrapper around one ``gmpc_ctx``: torch tensors own the device memory and the stream,
every method is a single call through the C ABI (include/gan_mpc_amd.h).

torch is plumbing only here (device buffers, ``torch.cuda.current_stream``); no arithmetic on the
hot path is done by torch.
"""

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import CemOpts, IlqrOpts, MppiOpts, Shape

# trajax iLQR keywords exactly as the reference passes them (policy/eval.py:10-20)
TRAJAX_iLQR_KWARGS = {
    "maxiter": 100,
    "grad_norm_threshold": 1e-4,
    "relative_grad_norm_threshold": 0.0,
    "obj_step_threshold": 0.0,
    "inputs_step_threshold": 0.0,
    "make_psd": False,
    "psd_delta": 0.0,
    "alpha_0": 1.0,
    "alpha_min": 0.00005,
}

# trajax cem keywords at their defaults (trajax optimizers.py `cem`: hyperparams)
TRAJAX_CEM_KWARGS = {
    "sampling_smoothing": 0.0,
    "evolution_smoothing": 0.1,
    "elite_portion": 0.1,
    "max_iter": 10,
    "num_samples": 400,
    "seed": 0,
}

# the path-integral solver's keywords: TRAJAX_CEM_KWARGS without the elites, plus the softmax temperature
MPPI_KWARGS = {
    "sampling_smoothing": 0.0,
    "evolution_smoothing": 0.0,
    "temperature": 1.0,
    "max_iter": 5,
    "num_samples": 400,
    "seed": 0,
}

# the sample-efficient CEM's keywords at the defaults of Pinneri et al. (CoRL 2020, table 2)
ICEM_KWARGS = {
    "noise_beta": 2.0,
    "evolution_smoothing": 0.1,
    "elite_portion": 0.1,
    "keep_portion": 0.3,
    "decay": 1.25,
    "max_iter": 3,
    "num_samples": 100,
    "seed": 0,
    "add_mean": True,
    "return_best": True,
}


def make_shape(n, m, T, dyn_dims, cost_dims, lstm_features=0, head_dims=None, dyn_lstm=0, x_size=0):
    """dyn_lstm = F > 0: the LSTM dynamics variant -- n = x_size + 2F is the size of xc = [x, c, h],
    dyn_dims the relu tail [F, hidden..., x_size] (see include/gan_mpc_amd.h)."""
    s = Shape()
    s.n, s.m, s.T = int(n), int(m), int(T)
    s.dyn_lstm_features, s.x_size = int(dyn_lstm), int(x_size)
    s.dyn_layers = len(dyn_dims) - 1
    s.cost_layers = len(cost_dims) - 1
    for i, d in enumerate(dyn_dims):
        s.dyn_dims[i] = int(d)
    for i, d in enumerate(cost_dims):
        s.cost_dims[i] = int(d)
    s.lstm_features = int(lstm_features)
    if lstm_features:
        head_dims = list(head_dims or [lstm_features, 1])
        s.head_layers = len(head_dims) - 1
        for i, d in enumerate(head_dims):
            s.head_dims[i] = int(d)
    return s


LIN_ROUTE_INTS = 12       # GMPC_LIN_ROUTE_INTS


def linearize_route_of(shape, nsamp, strided=False, lib=None):
    """gmpc_linearize_route as a dict (host only, no GPU): the family of Jacobian chain a ctx of `shape` launches for
    nsamp samples, and the plan of k_linearize_mfma<NT, NTF> for that launch."""
    lib = lib or _lib.load()
    r = (C.c_int * LIN_ROUTE_INTS)()
    _lib.check(lib.gmpc_linearize_route(C.byref(shape), int(nsamp), int(bool(strided)), r))
    return dict(family=Engine.LIN_FAMILIES[r[0]], NT=r[1], NTF=r[2], NGF=r[3], stage_w1=r[4], stage_wl=r[5],
                body=Engine.LIN_BODIES[r[6]], ntiles=r[7], grid=r[8], lds=r[9], nsmax=r[10], mfma_ok=bool(r[11]))


def make_expert_shape(lstm_features, head_dims_x, head_dims_u):
    """gmpc_expert_shape: y width (= lstm_features, or the first dense width of the MLP variant),
    hidden widths, then n / m."""
    es = _lib.ExpertShape()
    es.lstm_features = int(lstm_features)
    assert len(head_dims_x) == len(head_dims_u)
    es.head_layers = len(head_dims_x) - 1
    for i, (dx, du) in enumerate(zip(head_dims_x, head_dims_u)):
        es.head_dims_x[i], es.head_dims_u[i] = int(dx), int(du)
    return es


def make_opts(kwargs=None):
    kw = dict(TRAJAX_iLQR_KWARGS)
    if kwargs:
        kw.update(kwargs)
    o = IlqrOpts()
    o.maxiter = int(kw["maxiter"])
    o.grad_norm_threshold = float(kw["grad_norm_threshold"])
    o.relative_grad_norm_threshold = float(kw["relative_grad_norm_threshold"])
    o.obj_step_threshold = float(kw["obj_step_threshold"])
    o.inputs_step_threshold = float(kw["inputs_step_threshold"])
    o.make_psd = int(bool(kw["make_psd"]))
    o.psd_delta = float(kw["psd_delta"])
    o.alpha_0 = float(kw["alpha_0"])
    o.alpha_min = float(kw["alpha_min"])
    return o


def _merged_kwargs(who, defaults, kwargs):
    """A sampling solver's keyword set: `defaults` under the caller's `kwargs`, which may name known keywords only."""
    unknown = set(kwargs or ()) - set(defaults)
    if unknown:
        raise _lib.GmpcError(f"{who}: unknown keyword(s) {sorted(unknown)}")
    return {**defaults, **(kwargs or {})}


def make_cem_opts(kwargs=None, iter_offset=0):
    """gmpc_cem_opts from trajax' keyword set: num_elites = int(num_samples * elite_portion), as trajax computes it."""
    kw = _merged_kwargs("cem", TRAJAX_CEM_KWARGS, kwargs)
    o = CemOpts()
    o.max_iter, o.num_samples = int(kw["max_iter"]), int(kw["num_samples"])
    o.num_elites = int(kw["num_samples"] * kw["elite_portion"])
    o.iter_offset = int(iter_offset)
    o.sampling_smoothing = float(kw["sampling_smoothing"])
    o.evolution_smoothing = float(kw["evolution_smoothing"])
    o.seed = int(kw["seed"]) & 0xFFFFFFFFFFFFFFFF
    return o


def make_mppi_opts(kwargs=None, iter_offset=0):
    """gmpc_mppi_opts from MPPI_KWARGS' keyword set."""
    kw = _merged_kwargs("mppi", MPPI_KWARGS, kwargs)
    o = MppiOpts()
    o.max_iter, o.num_samples, o.iter_offset = int(kw["max_iter"]), int(kw["num_samples"]), int(iter_offset)
    o.sampling_smoothing = float(kw["sampling_smoothing"])
    o.evolution_smoothing = float(kw["evolution_smoothing"])
    o.temperature = float(kw["temperature"])
    o.seed = int(kw["seed"]) & 0xFFFFFFFFFFFFFFFF
    return o


def make_icem_opts(kwargs=None, iter_offset=0, carry_in=0):
    """gmpc_icem_opts from ICEM_KWARGS' keyword set: num_elites = int(num_samples * elite_portion) and num_keep =
    int(num_elites * keep_portion), both on the host."""
    kw = _merged_kwargs("icem", ICEM_KWARGS, kwargs)
    o = _lib.IcemOpts()
    o.max_iter, o.num_samples, o.iter_offset = int(kw["max_iter"]), int(kw["num_samples"]), int(iter_offset)
    o.num_elites = int(kw["num_samples"] * kw["elite_portion"])
    o.num_keep = int(o.num_elites * kw["keep_portion"])
    o.carry_in = int(carry_in)
    o.add_mean, o.return_best = int(bool(kw["add_mean"])), int(bool(kw["return_best"]))
    o.noise_beta = float(kw["noise_beta"])
    o.evolution_smoothing = float(kw["evolution_smoothing"])
    o.decay = float(kw["decay"])
    o.seed = int(kw["seed"]) & 0xFFFFFFFFFFFFFFFF
    return o


def pack_layout(shape, which):
    """[(flax tree path, offset, rows, cols, ld), ...] of a flat parameter vector (gmpc_pack_layout):
    which = 0 dyn, 1 cost, 2 critic, 3 the training vector [mpc_weights | cost | dynamics | critic]."""
    lib = _lib.load()
    count = lib.gmpc_pack_layout(C.byref(shape), int(which), None, 0)
    if count < 0:
        _lib.check(count)
    leaves = (_lib.Leaf * count)()
    _lib.check(min(0, lib.gmpc_pack_layout(C.byref(shape), int(which), leaves, count)))
    return [(lf.name.decode(), lf.offset, lf.rows, lf.cols, lf.ld) for lf in leaves]


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype in (torch.float32, torch.int32) and t.is_contiguous(), \
        "C-ABI buffers must be contiguous fp32/int32 device tensors"
    return C.c_void_p(t.data_ptr())


class Engine:
    """One context on one GPU.  All tensor arguments are contiguous fp32 CUDA(HIP) tensors."""

    def __init__(self, n, m, T, dyn_dims, cost_dims, max_batch, lstm_features=0, head_dims=None,
                 device=None, dyn_lstm=0, x_size=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.GmpcError("no HIP device visible to torch; gan_mpc_amd has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.shape = make_shape(n, m, T, dyn_dims, cost_dims, lstm_features, head_dims, dyn_lstm, x_size)
        self.n, self.m, self.T = int(n), int(m), int(T)
        self.nx = int(x_size) if dyn_lstm else int(n)      # x part of xc: goals / critic / expert columns
        self.max_batch = int(max_batch)
        # the step-major ("large-state") pipeline: n > 64, or more than 32 controls; it keeps ONE step of Jacobians
        self.big = self.n > 64 or self.m > 32
        self.dyn_count = self.lib.gmpc_param_count(C.byref(self.shape), 0)
        self.cost_count = self.lib.gmpc_param_count(C.byref(self.shape), 1)
        self.critic_count = self.lib.gmpc_param_count(C.byref(self.shape), 2) if lstm_features else 0
        ctx = C.c_void_p()
        _lib.check(self.lib.gmpc_create(C.byref(self.shape), self.max_batch, self.device.index,
                                        C.byref(ctx)))
        self.ctx = ctx
        self._bound = None
        self._ensemble = None          # set_sampled_ensemble's members, kept alive
        self._ensemble_mode = None     # set_sampled_ensemble_mode's keywords; None: never set (the default mode)
        self._disagreement = None      # set_sampled_disagreement's penalty; None: off
        self.solve_count = 0      # solves issued on this ctx (policy.differentiable: a backward checks it is current)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.gmpc_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def new(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def to_dev(self, a, dtype=torch.float32):
        if torch.is_tensor(a):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device).contiguous()

    def set_params(self, mpc_w, dyn, cost):
        assert mpc_w.numel() == 3 and dyn.numel() == self.dyn_count and cost.numel() == self.cost_count
        self._bound = (mpc_w, dyn, cost)  # keep the tensors alive: the ctx holds raw pointers
        _lib.check(self.lib.gmpc_set_params(self.ctx, _ptr(mpc_w), _ptr(dyn), _ptr(cost),
                                            self._stream()))

    def rollout_cost(self, x0, U, goal, X=None, costs=None):
        B = x0.shape[0]
        X = self.new(B, self.T + 1, self.n) if X is None else X
        costs = self.new(B, self.T + 1) if costs is None else costs
        _lib.check(self.lib.gmpc_rollout_cost(self.ctx, B, _ptr(x0), _ptr(U), _ptr(goal), _ptr(X),
                                              _ptr(costs), self._stream()))
        return X, costs

    @staticmethod
    def _check_rows(call, B, **args):
        """The single-evaluation kernels read B rows of a fixed width from each argument: a tensor with fewer or
        narrower rows would be read past its end.  args: name -> (tensor or None, row width)."""
        for name, (t, width) in args.items():
            if t is not None and (t.dim() != 2 or tuple(t.shape) != (B, width)):
                raise _lib.GmpcError(f"{call}: {name} must be ({B}, {width}), got {tuple(t.shape)}")

    def get_cost(self, x, u, goal_row, terminal):
        """cost_model.get_cost for B independent (x, u) pairs: the staging branch against goal_row
        (B, n), or (terminal) the terminal branch of an arbitrary state -> (B,)."""
        B = x.shape[0]
        self._check_rows("get_cost", B, x=(x, self.n), u=(u, self.m), goal_row=(goal_row, self.nx))
        cost = self.new(B)
        _lib.check(self.lib.gmpc_get_cost(self.ctx, B, _ptr(x), _ptr(u), _ptr(goal_row),
                                          int(bool(terminal)), _ptr(cost), self._stream()))
        return cost

    def predict(self, x, u):
        """dynamics_model.predict for B independent (x, u) pairs -> next_x (B, n)."""
        B = x.shape[0]
        self._check_rows("predict", B, x=(x, self.n), u=(u, self.m))
        nxt = self.new(B, self.n)
        _lib.check(self.lib.gmpc_predict(self.ctx, B, _ptr(x), _ptr(u), _ptr(nxt), self._stream()))
        return nxt

    def lqr_backward(self, X, U, goal, after_rollout=False, out=None):
        B = X.shape[0]
        n, m, T = self.n, self.m, self.T
        if out is None:
            out = dict(K=self.new(B, T, m, n), k=self.new(B, T, m), grad=self.new(B, T, m),
                       adjoints=self.new(B, T + 1, n))
            if not self.big:   # the large-state pass is step-major and never holds all T Jacobians
                out["AB"] = self.new(B, T, n, n + m)
        fn = self.lib.gmpc_lqr_backward_after_rollout if after_rollout else self.lib.gmpc_lqr_backward
        _lib.check(fn(self.ctx, B, _ptr(X), _ptr(U), _ptr(goal), _ptr(out["K"]), _ptr(out["k"]),
                      _ptr(out["grad"]), _ptr(out["adjoints"]), _ptr(out.get("AB")), self._stream()))
        return out

    LIN_FAMILIES = ("none", "sparse", "regs", "mfma", "valu", "dynl", "lowrank")
    LIN_BODIES = ("single", "ring", "multi")

    def linearize_route(self, nsamp, strided=False):
        """The Jacobian chain this engine's shape runs for nsamp samples: linearize_route_of(self.shape, ...)."""
        return linearize_route_of(self.shape, nsamp, strided, lib=self.lib)

    def linearize(self, masks, AB, nsamp, active=None, samp_mul=1, samp_add=0):
        """The Jacobian chain on the caller's relu bits (gmpc_linearize_ex): masks int32 words
        [(s * samp_mul + samp_add) * Lh + l][8], AB (at least nsamp * n * (n + m) floats) is written in place."""
        nsamp, samp_mul, samp_add = int(nsamp), int(samp_mul), int(samp_add)
        if nsamp < 1 or samp_mul < 1 or samp_add < 0:
            raise _lib.GmpcError(f"linearize: nsamp={nsamp}, samp_mul={samp_mul}, samp_add={samp_add} out of range")
        last = (nsamp - 1) * samp_mul + samp_add                       # the furthest sample of `masks` the launch reads
        Lh = self.shape.dyn_layers - 1
        if masks is None or masks.dtype != torch.int32 or masks.numel() < (last + 1) * Lh * 8:
            raise _lib.GmpcError(f"linearize: masks must hold {(last + 1) * Lh * 8} int32 words")
        if AB is None or AB.dtype != torch.float32 or AB.numel() < nsamp * self.n * (self.n + self.m):
            raise _lib.GmpcError(f"linearize: AB must hold {nsamp * self.n * (self.n + self.m)} floats")
        if active is not None and (active.dtype != torch.int32 or active.numel() < last // self.T + 1):
            raise _lib.GmpcError(f"linearize: active must hold {last // self.T + 1} int32 entries")
        _lib.check(self.lib.gmpc_linearize_ex(self.ctx, int(nsamp), _ptr(masks), _ptr(active), _ptr(AB), int(samp_mul),
                                              int(samp_add), self._stream()))
        return AB

    def ilqr_solve(self, x0, U, goal, kwargs=None):
        return self._solve(self.lib.gmpc_ilqr_solve, x0, U, goal, kwargs)

    def ilqr_solve_fused(self, x0, U, goal, kwargs=None):
        """The same solve in one kernel launch (gmpc_ilqr_solve_fused: MLP dynamics, n <= 64, m <= 32, T <= 32);
        returns the same dict as ilqr_solve without synchronising the stream."""
        return self._solve(self.lib.gmpc_ilqr_solve_fused, x0, U, goal, kwargs)

    def ilqr_solve_box(self, x0, U, goal, u_lo, u_hi, kwargs=None):
        """The one-launch solve under box bounds u_lo <= u_t <= u_hi on the controls (gmpc_ilqr_solve_box: the shapes
        of ilqr_solve_fused).  u_lo, u_hi: None (unbounded on that side), a scalar or m values, -inf / +inf allowed;
        checked on the host before any launch (their device copies are uploaded when the values change).  Returns the
        same dict as ilqr_solve; the ctx holds no solution for bilevel_grad* / upper_loss afterwards
        (ilqr_solve_box_held's does)."""
        return self._solve_box("gmpc_ilqr_solve_box", x0, U, goal, u_lo, u_hi, kwargs)

    def ilqr_solve_box_held(self, x0, U, goal, u_lo, u_hi, kwargs=None):
        """ilqr_solve_box with the solution held for the bilevel tail (gmpc_ilqr_solve_box_held): the same launch, the
        same bound handling and cache, then the clamped set of the solution (debug buffer 18).  bilevel_grad,
        bilevel_grad_cotangent, bilevel_grad_inputs, bilevel_grad_dynamics and upper_loss may follow: they
        differentiate through the active set held fixed."""
        return self._solve_box("gmpc_ilqr_solve_box_held", x0, U, goal, u_lo, u_hi, kwargs)

    def _solve_box(self, name, x0, U, goal, u_lo, u_hi, kwargs):
        _, _, lo_d, hi_d = self._device_bounds(u_lo, u_hi)
        return self._solve(getattr(self.lib, name), x0, U, goal, kwargs, tail=(_ptr(lo_d), _ptr(hi_d)))

    def _device_bounds(self, u_lo, u_hi):
        """The checked host vectors of a pair of bounds and their cached device copies -> (lo, hi, lo_d, hi_d)."""
        lo, hi = self._bound_vector("u_lo", u_lo), self._bound_vector("u_hi", u_hi)
        if lo is not None and hi is not None and not bool(np.all(lo <= hi)):
            raise _lib.GmpcError("u_lo must be <= u_hi")
        # the device copies are kept: a policy solves with the same bounds at every control step
        key = (None if lo is None else lo.tobytes(), None if hi is None else hi.tobytes())
        cache = self.__dict__.setdefault("_box_bounds", {})
        if key not in cache:
            if len(cache) >= 8:
                cache.clear()
            cache[key] = (None if lo is None else self.to_dev(lo), None if hi is None else self.to_dev(hi))
        return (lo, hi) + cache[key]

    SAMPLED_PRECISIONS = {"fp32": 0, "bf16": 1}     # GMPC_SAMPLED_FP32 / GMPC_SAMPLED_BF16

    def set_sampled_precision(self, precision):
        """The operand precision of the sampled rollouts of cem_solve / mppi_solve / icem_solve on this engine
        (gmpc_set_sampled_precision): "fp32" (the default) or "bf16" -- the dynamics and cost
        layers of every sampled row on the bf16 matrix instruction (weights and layer inputs rounded to bf16, fp32
        accumulation, states and cost terms in fp32).  The samples are bitwise those of "fp32"; the costs, and with
        them the elites, the weights and icem_solve's best_cost, are bf16-mode costs; X and obj are always the fp32
        rollout of the returned U.  mppi_vjp is refused in "bf16" mode.  No device work."""
        if not isinstance(precision, str) or precision not in self.SAMPLED_PRECISIONS:
            raise _lib.GmpcError(f'sampled precision: {precision!r} is neither "fp32" nor "bf16"')
        _lib.check(self.lib.gmpc_set_sampled_precision(self.ctx, self.SAMPLED_PRECISIONS[precision]))

    MAX_ENSEMBLE = 16     # GMPC_MAX_ENSEMBLE

    def set_sampled_ensemble(self, members):
        """A dynamics ensemble under the sampled rollouts of cem_solve / mppi_solve / icem_solve on this engine
        (gmpc_set_sampled_ensemble).  members: None -- no ensemble (the default) --, or a float32
        (P, dyn_count) tensor or array, 1 <= P <= 16, each row a dynamics parameter vector laid out like set_params'
        `dyn`; moved to the device and kept alive here.  While set, a sampled row's cost is the mean of its costs
        under the members (summed in member order, times float32(1 / P)); the samples are bitwise unchanged; X and obj
        are the rollout of the returned U under the bound (nominal) dynamics; mppi_vjp is refused.  set_params keeps
        the ensemble.  A tensor changed in place needs this call again.  No device work beyond the copy."""
        if members is None:
            _lib.check(self.lib.gmpc_set_sampled_ensemble(self.ctx, 0, None))
            self._ensemble = None
            return
        shape = tuple(getattr(members, "shape", ()))
        if len(shape) != 2:
            raise _lib.GmpcError(f"ensemble: members must be (P, {self.dyn_count}), got shape {shape}")
        if shape[1] != self.dyn_count:
            raise _lib.GmpcError(f"ensemble: members must be (P, {self.dyn_count}), got {shape}")
        if not 1 <= shape[0] <= self.MAX_ENSEMBLE:
            raise _lib.GmpcError(f"ensemble: P = {shape[0]} outside [1, {self.MAX_ENSEMBLE}]")
        dtype = members.dtype if torch.is_tensor(members) else np.asarray(members).dtype
        if dtype not in (torch.float32, np.dtype(np.float32)):
            raise _lib.GmpcError(f"ensemble: members must be float32, got {dtype}")
        dev = self.to_dev(members)
        _lib.check(self.lib.gmpc_set_sampled_ensemble(self.ctx, int(shape[0]), _ptr(dev)))
        self._ensemble = dev      # keep the tensor alive: the ctx holds a raw pointer

    ENSEMBLE_AGGREGATES = {"mean": 0, "mean_std": 1, "max": 2}     # GMPC_ENS_MEAN / MEAN_STD / MAX
    ENSEMBLE_PROPAGATIONS = {"fixed": 0, "ts1": 1}                 # GMPC_ENS_FIXED / TS1

    def set_sampled_ensemble_mode(self, aggregate="mean", risk=0.0, propagation="fixed", particles=None):
        """What cem_solve / mppi_solve / icem_solve do with a set ensemble (gmpc_set_sampled_ensemble_mode; DESIGN.md
        section 26); the defaults are the mean over the members of set_sampled_ensemble.
        propagation: "fixed" -- one cost plane per member (particles must be None) --, or "ts1" -- `particles` planes,
        1 to 16, each a particle that draws its member anew at every step from a schedule shared by all rows and
        problems of an iteration.
        aggregate over the planes' costs of a row: "mean"; "mean_std" -- mean + risk * (population standard deviation
        of the planes), risk < 0 is optimism --; "max" -- the worst plane.  risk goes with "mean_std" only.
        Independent of the members: it may be set before them, set_sampled_ensemble and set_params keep it, and it
        does nothing while no ensemble is set.  Every refusal is a GmpcError("ensemble mode: ...") raised here, before
        the library is called.  No device work."""
        who = "ensemble mode"
        if not isinstance(aggregate, str) or aggregate not in self.ENSEMBLE_AGGREGATES:
            raise _lib.GmpcError(f'{who}: aggregate {aggregate!r} is none of "mean", "mean_std", "max"')
        if not isinstance(propagation, str) or propagation not in self.ENSEMBLE_PROPAGATIONS:
            raise _lib.GmpcError(f'{who}: propagation {propagation!r} is neither "fixed" nor "ts1"')
        if isinstance(risk, bool) or not isinstance(risk, (int, float, np.integer, np.floating)):
            raise _lib.GmpcError(f"{who}: risk must be a number, got {risk!r}")
        with np.errstate(over="ignore"):
            risk32 = float(np.float32(risk))
        if not np.isfinite(risk32):
            raise _lib.GmpcError(f"{who}: risk = {risk!r} is not finite in float32")
        if risk32 != 0.0 and aggregate != "mean_std":
            raise _lib.GmpcError(f'{who}: risk = {risk!r} goes with aggregate "mean_std" only, got {aggregate!r}')
        if propagation == "fixed":
            if particles is not None:
                raise _lib.GmpcError(f'{who}: particles = {particles!r} goes with propagation "ts1" only')
            count = 0
        else:
            if isinstance(particles, bool) or not isinstance(particles, (int, np.integer)):
                raise _lib.GmpcError(f'{who}: propagation "ts1" needs particles, an integer in [1, '
                                     f"{self.MAX_ENSEMBLE}], got {particles!r}")
            if not 1 <= particles <= self.MAX_ENSEMBLE:
                raise _lib.GmpcError(f"{who}: particles = {particles} outside [1, {self.MAX_ENSEMBLE}]")
            count = int(particles)
        mode = _lib.EnsembleMode(self.ENSEMBLE_AGGREGATES[aggregate], risk32, self.ENSEMBLE_PROPAGATIONS[propagation],
                                 count)
        _lib.check(self.lib.gmpc_set_sampled_ensemble_mode(self.ctx, C.byref(mode)))
        self._ensemble_mode = dict(aggregate=aggregate, risk=risk32, propagation=propagation, particles=particles)

    DISAGREEMENT_KINDS = {"off": 0, "onestep": 1}     # GMPC_DIS_OFF / GMPC_DIS_ONESTEP

    def set_sampled_disagreement(self, penalty):
        """A penalty on the members' one-step disagreement with the bound (nominal) dynamics along every sampled row
        of cem_solve / mppi_solve / icem_solve (gmpc_set_sampled_disagreement).  penalty: None
        -- off (the default) --, or a finite number: the rows are rolled out under the nominal model, and plane p's
        cost is the nominal cost + penalty * sum_t |MLP_p([x_t; u_t]) - MLP_0([x_t; u_t])|^2; the planes then go
        through set_sampled_ensemble_mode's aggregate.  penalty > 0 is pessimism, < 0 exploration, 0 allowed.
        Independent of the members and the mode: set_sampled_ensemble and set_params keep it, and it does nothing while
        no ensemble is set.  Propagation "ts1" is refused by the solves while it is on.  Every refusal is a
        GmpcError("disagreement: ...") raised here, before the library is called.  No device work."""
        who = "disagreement"
        if penalty is None:
            _lib.check(self.lib.gmpc_set_sampled_disagreement(self.ctx, self.DISAGREEMENT_KINDS["off"], 0.0))
            self._disagreement = None
            return
        if isinstance(penalty, bool) or not isinstance(penalty, (int, float, np.integer, np.floating)):
            raise _lib.GmpcError(f"{who}: penalty must be None or a number, got {penalty!r}")
        with np.errstate(over="ignore"):
            pen32 = float(np.float32(penalty))
        if not np.isfinite(pen32):
            raise _lib.GmpcError(f"{who}: penalty = {penalty!r} is not finite in float32")
        _lib.check(self.lib.gmpc_set_sampled_disagreement(self.ctx, self.DISAGREEMENT_KINDS["onestep"], pen32))
        self._disagreement = pen32

    CEM_WANT = ("costs", "elites", "samples")

    def cem_solve(self, x0, U_init, goal, u_lo, u_hi, kwargs=None, init_std=None, want=(), iter_offset=0):
        """The cross-entropy method from the mean U_init under u_lo <= u <= u_hi (gmpc_cem_solve; trajax `cem`, keywords
        TRAJAX_CEM_KWARGS).  u_lo, u_hi as for ilqr_solve_box.  init_std: None -- (u_hi - u_lo) / 2 per control, as
        trajax does, which needs both bounds finite --, a scalar, m values or a (B, T, m) tensor.  -> dict(X, U (the
        final mean, not clipped), obj, std) plus the last iteration's `want`ed debug outputs: "costs" (B, N), "elites"
        (B, E) int32, "samples" (B, N, T, m).  iter_offset: the noise stream's first iteration (chained calls).
        Stateless: a held iLQR solution stays valid; nothing is synchronised."""
        B, n, m, T = x0.shape[0], self.n, self.m, self.T
        opts, lo_d, hi_d, std = self._sampling_prologue(
            "cem", self.CEM_WANT, make_cem_opts, kwargs, iter_offset, x0, U_init, goal, u_lo, u_hi, init_std, want)
        N, E = opts.num_samples, opts.num_elites
        out = dict(X=self.new(B, T + 1, n), U=U_init.clone(), obj=self.new(B), std=std)
        if "costs" in want:
            out["costs"] = self.new(B, N)
        if "elites" in want:
            out["elites"] = self.new(B, max(E, 0), dtype=torch.int32)
        if "samples" in want:
            out["samples"] = self.new(B, N, T, m)
        _lib.check(self.lib.gmpc_cem_solve(
            self.ctx, B, _ptr(x0), _ptr(goal), _ptr(lo_d), _ptr(hi_d), C.byref(opts), _ptr(out["U"]), _ptr(out["std"]),
            _ptr(out["X"]), _ptr(out["obj"]), _ptr(out.get("costs")), _ptr(out.get("elites")), _ptr(out.get("samples")),
            self._stream()))
        return out

    MPPI_WANT = ("costs", "weights", "samples")

    def _sampling_prologue(self, who, known_want, make_opts, kwargs, iter_offset, x0, U_init, goal, u_lo, u_hi,
                           init_std, want):
        """What cem_solve, mppi_solve and icem_solve check and build first, in this order: the shapes, `want` against
        the solver's known entries, the options (make_opts), the device bounds and the std.  -> opts, lo_d, hi_d,
        std."""
        B, n, m, T = x0.shape[0], self.n, self.m, self.T
        for name, t, shape in (("x0", x0, (B, n)), ("U_init", U_init, (B, T, m)), ("goal", goal, (B, T + 1, self.nx))):
            if tuple(t.shape) != shape:
                raise _lib.GmpcError(f"{who}: {name} must be {shape}, got {tuple(t.shape)}")
        unknown = set(want) - set(known_want)
        if unknown:
            raise _lib.GmpcError(f"{who}: want has unknown entries {sorted(unknown)}; known: {known_want}")
        opts = make_opts(kwargs, iter_offset)
        lo, hi, lo_d, hi_d = self._device_bounds(u_lo, u_hi)
        return opts, lo_d, hi_d, self._sampling_std(who, B, init_std, lo, hi)

    def _sampling_std(self, who, B, init_std, lo, hi):
        """The (B, T, m) device std of a sampling solver: cem_solve's rules for init_std."""
        T, m = self.T, self.m
        if init_std is None and (lo is None or hi is None or not (np.isfinite(lo).all() and np.isfinite(hi).all())):
            raise _lib.GmpcError(f"{who}: without init_std both bounds must be finite (std = (u_hi - u_lo) / 2)")
        if init_std is None:
            return self.to_dev(np.broadcast_to((hi - lo) / np.float32(2), (B, T, m)))
        if torch.is_tensor(init_std) and tuple(init_std.shape) == (B, T, m):
            return self.to_dev(init_std).clone()
        return self.to_dev(np.broadcast_to(self._bound_vector("init_std", init_std), (B, T, m)))

    def mppi_solve(self, x0, U_init, goal, u_lo, u_hi, kwargs=None, init_std=None, want=(), iter_offset=0,
                   trace=False):
        """Model-predictive path integral control from the mean U_init under u_lo <= u <= u_hi (gmpc_mppi_solve;
        keywords MPPI_KWARGS): cem_solve's samples and costs, softmax weights exp(-(J - J_min) / temperature) instead
        of the elite cut, std fixed.  u_lo, u_hi, init_std as for cem_solve.  -> dict(X, U (the final mean, not
        clipped), obj, std) plus the last iteration's `want`ed debug outputs: "costs" (B, N), "weights" (B, N,
        normalised), "samples" (B, N, T, m); trace: also means_trace (K, B, T, m), the mean before each iteration,
        and costs_trace (K, B, N), what mppi_vjp needs.  Stateless: a held iLQR solution stays valid; nothing is
        synchronised."""
        B, n, m, T = x0.shape[0], self.n, self.m, self.T
        opts, lo_d, hi_d, std = self._sampling_prologue(
            "mppi", self.MPPI_WANT, make_mppi_opts, kwargs, iter_offset, x0, U_init, goal, u_lo, u_hi, init_std, want)
        N, K = opts.num_samples, max(opts.max_iter, 0)
        out = dict(X=self.new(B, T + 1, n), U=U_init.clone(), obj=self.new(B), std=std)
        if "costs" in want:
            out["costs"] = self.new(B, max(N, 0))
        if "weights" in want:
            out["weights"] = self.new(B, max(N, 0))
        if "samples" in want:
            out["samples"] = self.new(B, max(N, 0), T, m)
        if trace:
            out["means_trace"] = self.new(K, B, T, m)
            out["costs_trace"] = self.new(K, B, max(N, 0))
        _lib.check(self.lib.gmpc_mppi_solve(
            self.ctx, B, _ptr(x0), _ptr(goal), _ptr(lo_d), _ptr(hi_d), C.byref(opts), _ptr(out["U"]), _ptr(std),
            _ptr(out["X"]), _ptr(out["obj"]), _ptr(out.get("costs")), _ptr(out.get("weights")),
            _ptr(out.get("samples")), _ptr(out.get("means_trace")), _ptr(out.get("costs_trace")), self._stream()))
        return out

    ICEM_WANT = ("costs", "elites", "samples")

    def icem_solve(self, x0, U_init, goal, u_lo, u_hi, kwargs=None, init_std=None, want=(), iter_offset=0, state=None):
        """The sample-efficient cross-entropy method from the mean U_init under u_lo <= u <= u_hi (gmpc_icem_solve;
        keywords ICEM_KWARGS).  u_lo, u_hi, init_std as for cem_solve.  state: None -- nothing is
        carried in, the best cost starts at +inf --, or the `state` of an earlier call (dict(keep (B, num_keep, T, m),
        best_U (B, T, m), best_cost (B,)), not written; an entry "carry" gives carry_in, default num_keep): its kept
        rows join the first iteration's pool and its best row stays the one to beat.  -> dict(X, U (the returned
        sequence: the best row seen with return_best, the final mean otherwise), obj, mean, std, state) plus the last
        iteration's `want`ed debug outputs: "costs" (B, R) over the pool's rows, "elites" (B, E) int32 pool rows,
        "samples" (B, N_last, T, m), the fresh rows.  iter_offset: the noise stream's (and the sample count's) first
        iteration.  Stateless on the context: a held iLQR solution stays valid; nothing is synchronised."""
        B, n, m, T = x0.shape[0], self.n, self.m, self.T
        opts, lo_d, hi_d, std = self._sampling_prologue(
            "icem", self.ICEM_WANT, make_icem_opts, kwargs, iter_offset, x0, U_init, goal, u_lo, u_hi, init_std, want)
        N, E, nk, K = opts.num_samples, opts.num_elites, max(opts.num_keep, 0), max(opts.max_iter, 0)
        if state is None:
            st = dict(keep=torch.zeros(B, nk, T, m, device=self.device),
                      best_U=torch.zeros(B, T, m, device=self.device),
                      best_cost=torch.full((B,), float("inf"), device=self.device))
        else:
            for name, shape in (("keep", (B, nk, T, m)), ("best_U", (B, T, m)), ("best_cost", (B,))):
                if name not in state or tuple(state[name].shape) != shape:
                    raise _lib.GmpcError(f"icem: state[{name!r}] must be {shape}: the state of a call with these kwargs")
            st = {k: self.to_dev(state[k]).clone() for k in ("keep", "best_U", "best_cost")}
            opts.carry_in = int(state.get("carry", nk))
        nit = (C.c_int * max(K, 1))()
        _lib.check(self.lib.gmpc_icem_plan_host(C.byref(opts), T, nit, None))
        n_last = int(nit[K - 1]) if K else 0
        rows = n_last + (opts.carry_in if K == 1 else nk) + int(bool(opts.add_mean)) if K else 0
        out = dict(X=self.new(B, T + 1, n), U=self.new(B, T, m), obj=self.new(B), mean=U_init.clone(), std=std, state=st)
        costs = self.new(B, N + nk + 1) if "costs" in want else None
        elites = self.new(B, max(E, 0), dtype=torch.int32) if "elites" in want else None
        samples = self.new(B, max(N, 0), T, m) if "samples" in want else None
        _lib.check(self.lib.gmpc_icem_solve(
            self.ctx, B, _ptr(x0), _ptr(goal), _ptr(lo_d), _ptr(hi_d), C.byref(opts), _ptr(out["mean"]), _ptr(std),
            _ptr(st["keep"]) if nk else None, _ptr(st["best_U"]), _ptr(st["best_cost"]), _ptr(out["U"]),
            _ptr(out["X"]), _ptr(out["obj"]), _ptr(costs), _ptr(elites), _ptr(samples), self._stream()))
        if costs is not None:
            out["costs"] = costs[:, :rows]
        if elites is not None:
            out["elites"] = elites
        if samples is not None:
            out["samples"] = samples[:, :n_last]
        return out

    def mppi_vjp(self, x0, goal, u_lo, u_hi, sol, gU=None, gX=None, gobj=None, kwargs=None, iter_offset=0,
                 want_x0=True, want_U=True, want_goal=True, want_theta=True, want_dyn=True):
        """The VJP of mppi_solve (gmpc_mppi_vjp): sol is the dict of a mppi_solve(..., trace=True) with the same x0,
        goal, bounds, kwargs and iter_offset; gU (B, T, m), gX (B, T+1, n), gobj (B,) the cotangents of its U, X and
        obj (any may be None, not all).  -> dict(x0 (B, n), U (B, T, m) w.r.t. U_init, goal (B, T+1, n), theta
        [3 + cost_count], dyn [dyn_count]), None where not wanted; theta and dyn are summed over the batch.  The true
        derivative through the sampler.  It drops a solution held by this engine (solve_count advances)."""
        B, n, m, T = x0.shape[0], self.n, self.m, self.T
        for name, t, shape in (("x0", x0, (B, n)), ("goal", goal, (B, T + 1, self.nx)), ("U", sol["U"], (B, T, m)),
                               ("X", sol["X"], (B, T + 1, n)), ("std", sol["std"], (B, T, m)),
                               ("gU", gU, (B, T, m)), ("gX", gX, (B, T + 1, n)), ("gobj", gobj, (B,))):
            if t is not None and tuple(t.shape) != shape:
                raise _lib.GmpcError(f"mppi_vjp: {name} must be {shape}, got {tuple(t.shape)}")
        opts = make_mppi_opts(kwargs, iter_offset)
        K, N = max(opts.max_iter, 0), opts.num_samples
        for name, shape in (("means_trace", (K, B, T, m)), ("costs_trace", (K, B, N))):
            if name not in sol or tuple(sol[name].shape) != shape:
                raise _lib.GmpcError(f"mppi_vjp: sol[{name!r}] must be {shape}: solve with trace=True and these kwargs")
        _, _, lo_d, hi_d = self._device_bounds(u_lo, u_hi)
        out = dict(x0=self.new(B, n) if want_x0 else None, U=self.new(B, T, m) if want_U else None,
                   goal=self.new(B, T + 1, self.nx) if want_goal else None,
                   theta=self.new(3 + self.cost_count) if want_theta else None,
                   dyn=self.new(self.dyn_count) if want_dyn else None)
        self.solve_count += 1     # the sample rollouts overwrite the ctx's masks: a held solution is gone
        _lib.check(self.lib.gmpc_mppi_vjp(
            self.ctx, B, _ptr(x0), _ptr(goal), _ptr(lo_d), _ptr(hi_d), C.byref(opts), _ptr(sol["std"]),
            _ptr(sol["means_trace"]), _ptr(sol["costs_trace"]), _ptr(sol["U"]), _ptr(sol["X"]), _ptr(gU), _ptr(gX),
            _ptr(gobj), _ptr(out["x0"]), _ptr(out["U"]), _ptr(out["goal"]), _ptr(out["theta"]), _ptr(out["dyn"]),
            self._stream()))
        return out

    def _bound_vector(self, name, b):
        """None, a scalar or m values -> None or a host fp32 vector [m] without NaN."""
        if b is None:
            return None
        v = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
        v = np.array(np.broadcast_to(v.astype(np.float32), (self.m,)) if v.ndim == 0 else v.astype(np.float32))
        if v.shape != (self.m,):
            raise _lib.GmpcError(f"{name} must be a scalar or {self.m} values, got shape {v.shape}")
        if np.isnan(v).any():
            raise _lib.GmpcError(f"{name} has a NaN entry: u_lo must be <= u_hi")
        return v

    def _solve(self, fn, x0, U, goal, kwargs, tail=()):
        B = x0.shape[0]
        self.solve_count += 1     # before the call: a failed solve drops the held solution as well
        n, m, T = self.n, self.m, self.T
        opts = make_opts(kwargs)
        out = dict(X=self.new(B, T + 1, n), U=self.new(B, T, m), obj=self.new(B),
                   grad=self.new(B, T, m), adjoints=self.new(B, T + 1, n),
                   iterations=self.new(B, dtype=torch.int32))
        _lib.check(fn(
            self.ctx, B, _ptr(x0), _ptr(U), _ptr(goal), C.byref(opts), _ptr(out["X"]), _ptr(out["U"]),
            _ptr(out["obj"]), _ptr(out["grad"]), _ptr(out["adjoints"]), _ptr(out["iterations"]),
            self._stream(), *tail))
        return out

    def bilevel_grad(self, B, loss_kind, desired=None, critic=None, sign=1.0, grad_sum=None):
        """grad_sum: optional caller-owned [3 + cost_count] view (e.g. of a packed all-reduce buffer)."""
        loss = self.new(B)
        grad_sum = self.new(3 + self.cost_count) if grad_sum is None else grad_sum
        assert grad_sum.numel() == 3 + self.cost_count
        _lib.check(self.lib.gmpc_bilevel_grad(self.ctx, B, int(loss_kind), _ptr(desired), _ptr(critic),
                                              float(sign), _ptr(loss), _ptr(grad_sum), self._stream()))
        return loss, grad_sum

    def bilevel_grad_cotangent(self, B, lx=None, lu=None, sign=1.0, grad_sum=None):
        """The bilevel gradient of a caller-defined loss L(X, U) at the held solution: lx = dL/dX (B, T+1, n), lu =
        dL/dU (B, T, m), either may be None (gmpc_bilevel_grad_cotangent).  -> grad_sum [3 + cost_count], summed
        over the batch; grad_sum: optional caller-owned view."""
        for name, t, shape in (("lx", lx, (B, self.T + 1, self.n)), ("lu", lu, (B, self.T, self.m))):
            if t is not None and tuple(t.shape) != shape:
                raise _lib.GmpcError(f"bilevel_grad_cotangent: {name} must be {shape}, got {tuple(t.shape)}")
        grad_sum = self.new(3 + self.cost_count) if grad_sum is None else grad_sum
        assert grad_sum.numel() == 3 + self.cost_count
        _lib.check(self.lib.gmpc_bilevel_grad_cotangent(self.ctx, B, _ptr(lx), _ptr(lu), float(sign),
                                                        _ptr(grad_sum), self._stream()))
        return grad_sum

    def bilevel_grad_inputs(self, B, lx=None, want_x0=True, want_goal=True):
        """dL/dx0 (B, n) and dL/dgoal (B, T+1, nx) of the loss whose bilevel gradient was just computed
        (gmpc_bilevel_grad_inputs; must follow bilevel_grad or bilevel_grad_cotangent on the same held solution).  The
        true derivative, whatever `sign` the bilevel call used.  lx: the dL/dX passed to bilevel_grad_cotangent, or
        None for the ctx's own (bilevel_grad's loss; the zeroed one of a cotangent call without lx).  -> (grad_x0,
        grad_goal), None where not wanted.  grad_x0 is refused on the step-major pipeline (self.big)."""
        if lx is not None and tuple(lx.shape) != (B, self.T + 1, self.n):
            raise _lib.GmpcError(f"bilevel_grad_inputs: lx must be {(B, self.T + 1, self.n)}, got {tuple(lx.shape)}")
        gx0 = self.new(B, self.n) if want_x0 else None
        ggoal = self.new(B, self.T + 1, self.nx) if want_goal else None
        _lib.check(self.lib.gmpc_bilevel_grad_inputs(self.ctx, B, _ptr(lx), _ptr(gx0), _ptr(ggoal), self._stream()))
        return gx0, ggoal

    def bilevel_grad_dynamics(self, B, lx=None, grad_sum=None):
        """dL/dtheta_dyn [dyn_count] (gmpc_set_params' dyn layout), summed over the batch, of the loss whose bilevel
        gradient was just computed (gmpc_bilevel_grad_dynamics; same precondition and lx as bilevel_grad_inputs).  The
        true derivative, whatever `sign` the bilevel call used.  Relu-MLP dynamics and n <= 64, m <= 32 only.
        grad_sum: optional caller-owned view."""
        if lx is not None and tuple(lx.shape) != (B, self.T + 1, self.n):
            raise _lib.GmpcError(f"bilevel_grad_dynamics: lx must be {(B, self.T + 1, self.n)}, got {tuple(lx.shape)}")
        grad_sum = self.new(self.dyn_count) if grad_sum is None else grad_sum
        assert grad_sum.numel() == self.dyn_count
        _lib.check(self.lib.gmpc_bilevel_grad_dynamics(self.ctx, B, _ptr(lx), _ptr(grad_sum), self._stream()))
        return grad_sum

    def rollout_vjp(self, X, U, goal, gX=None, gcost=None, want_x0=True, want_U=True, want_goal=True,
                    want_theta=True, want_dyn=True):
        """The VJP of the rollout and its costs at (X, U, goal) (gmpc_rollout_vjp): gX = dL/dX (B, T+1, n) and/or
        gcost = dL/dcosts (B, T+1).  -> dict(x0 (B, n), U (B, T, m), goal (B, T+1, n), theta [3 + cost_count],
        dyn [dyn_count]), None where not wanted; theta and dyn are summed over the batch.  Stateless: a held iLQR
        solution stays valid.  Relu-MLP dynamics only."""
        B = X.shape[0]
        n, m, T = self.n, self.m, self.T
        for name, t, shape in (("X", X, (B, T + 1, n)), ("U", U, (B, T, m)), ("goal", goal, (B, T + 1, self.nx)),
                               ("gX", gX, (B, T + 1, n)), ("gcost", gcost, (B, T + 1))):
            if t is not None and tuple(t.shape) != shape:
                raise _lib.GmpcError(f"rollout_vjp: {name} must be {shape}, got {tuple(t.shape)}")
        out = dict(x0=self.new(B, n) if want_x0 else None, U=self.new(B, T, m) if want_U else None,
                   goal=self.new(B, T + 1, self.nx) if want_goal else None,
                   theta=self.new(3 + self.cost_count) if want_theta else None,
                   dyn=self.new(self.dyn_count) if want_dyn else None)
        _lib.check(self.lib.gmpc_rollout_vjp(
            self.ctx, B, _ptr(X), _ptr(U), _ptr(goal), _ptr(gX), _ptr(gcost), _ptr(out["x0"]), _ptr(out["U"]),
            _ptr(out["goal"]), _ptr(out["theta"]), _ptr(out["dyn"]), self._stream()))
        return out

    def upper_loss(self, B, loss_kind, desired=None, critic=None):
        loss = self.new(B)
        _lib.check(self.lib.gmpc_upper_loss(self.ctx, B, int(loss_kind), _ptr(desired), _ptr(critic),
                                            _ptr(loss), self._stream()))
        return loss

    def expert_rollout(self, history, expert_flat, expert_shape):
        """history (B, hist+1, n) -> goal (B, T+1, n), init_U (B, T, m) from the expert sequence model."""
        B, hist = history.shape[0], history.shape[1] - 1
        want = self.lib.gmpc_expert_param_count(self.nx, C.byref(expert_shape))
        assert expert_flat.numel() == want, (expert_flat.numel(), want)
        goal = self.new(B, self.T + 1, self.nx)
        init_U = self.new(B, self.T, self.m)
        _lib.check(self.lib.gmpc_expert_rollout(self.ctx, B, hist, C.byref(expert_shape), _ptr(expert_flat),
                                                _ptr(history), _ptr(goal), _ptr(init_U), self._stream()))
        return goal, init_U

    def expert_loss_grad(self, xseq, useq, next_xseq, expert_flat, expert_shape, discount, teacher_forcing,
                         want_grad=True, loss_sum=None, grad_sum=None):
        """Expert-model training loss of B windows xseq, next_xseq (B, S, nx), useq (B, S, m) ->
        (loss_sum[1], grad_sum[expert count] or None): sums over the batch (gmpc_expert_loss_grad)."""
        B, S = xseq.shape[0], xseq.shape[1]
        count = self.lib.gmpc_expert_param_count(self.nx, C.byref(expert_shape))
        assert expert_flat.numel() == count, (expert_flat.numel(), count)
        loss_sum = self.new(1) if loss_sum is None else loss_sum
        if want_grad:
            grad_sum = self.new(count) if grad_sum is None else grad_sum
            assert grad_sum.numel() == count
        else:
            grad_sum = None
        _lib.check(self.lib.gmpc_expert_loss_grad(
            self.ctx, B, S, C.byref(expert_shape), _ptr(expert_flat), _ptr(xseq), _ptr(useq), _ptr(next_xseq),
            float(discount), int(bool(teacher_forcing)), _ptr(loss_sum), _ptr(grad_sum), self._stream()))
        return loss_sum, grad_sum

    def expert_vjp(self, history, expert_flat, expert_shape, g_goal=None, g_U=None, want_params=True,
                   want_history=True):
        """The VJP of expert_rollout at (expert_flat, history) (gmpc_expert_vjp): g_goal = dL/dgoal (B, T+1, nx) and/or
        g_U = dL/dinit_U (B, T, m).  -> dict(params [expert count], summed over the batch, history (B, hist+1, nx)),
        None where not wanted.  Stateless: a held iLQR solution and its bilevel tail stay valid."""
        B, hist = history.shape[0], history.shape[1] - 1
        count = self.lib.gmpc_expert_param_count(self.nx, C.byref(expert_shape))
        assert expert_flat.numel() == count, (expert_flat.numel(), count)
        for name, t, shape in (("history", history, (B, hist + 1, self.nx)), ("g_goal", g_goal, (B, self.T + 1, self.nx)),
                               ("g_U", g_U, (B, self.T, self.m))):
            if t is not None and tuple(t.shape) != shape:
                raise _lib.GmpcError(f"expert_vjp: {name} must be {shape}, got {tuple(t.shape)}")
        out = dict(params=self.new(count) if want_params else None,
                   history=self.new(B, hist + 1, self.nx) if want_history else None)
        _lib.check(self.lib.gmpc_expert_vjp(
            self.ctx, B, hist, C.byref(expert_shape), _ptr(expert_flat), _ptr(history), _ptr(g_goal), _ptr(g_U),
            _ptr(out["params"]), _ptr(out["history"]), self._stream()))
        return out

    def dynamics_loss_grad(self, xseq, useq, next_xseq, discount, teacher_forcing, loss_sum=None,
                           grad_sum=None):
        """-> (loss_sum[1], grad_sum[dyn_count]) of the multi-step prediction loss over the batch."""
        B, S = xseq.shape[0], xseq.shape[1]
        loss_sum = self.new(1) if loss_sum is None else loss_sum
        grad_sum = self.new(self.dyn_count) if grad_sum is None else grad_sum
        assert loss_sum.numel() == 1 and grad_sum.numel() == self.dyn_count
        _lib.check(self.lib.gmpc_dynamics_loss_grad(
            self.ctx, B, S, _ptr(xseq), _ptr(useq), _ptr(next_xseq), float(discount),
            int(bool(teacher_forcing)), _ptr(loss_sum), _ptr(grad_sum), self._stream()))
        return loss_sum, grad_sum

    def dynamics_ensemble_loss_grad(self, members, xseq, useq, next_xseq, discount, teacher_forcing, rows=None,
                                    loss_sum=None, grad_sum=None):
        """dynamics_loss_grad for the P members of a dynamics ensemble in one call (gmpc_dynamics_ensemble_loss_grad;
        DESIGN.md section 25).  members: float32 device tensor (P, dyn_count), 1 <= P <= 16, each row laid out like
        set_params' `dyn`; xseq, next_xseq (D, S, n), useq (D, S, m): the dataset, float32 device tensors; rows: None
        -- every member takes the D = B dataset rows in order --, or an int32 (P, B) tensor or array of dataset rows in
        [0, D), duplicates allowed (checked here: the device trusts them).  -> (loss_sum (P,), grad_sum (P, dyn_count)):
        sums over each member's B sequences.  Relu-MLP dynamics, widths and n + m up to 256.  Reads nothing of the bound
        parameters (set_params need not have been called); a held solution, the bilevel tail and a set sampled ensemble
        stay as they are."""
        who = "ensemble fit"
        P = self._check_ensemble_members(who, members)
        if not torch.is_tensor(members):
            raise _lib.GmpcError(f"{who}: members must be a device tensor, got {type(members).__name__}")
        for name, t, width in (("xseq", xseq, self.n), ("useq", useq, self.m), ("next_xseq", next_xseq, self.n)):
            if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != width:
                raise _lib.GmpcError(f"{who}: {name} must be (D, S, {width}), got {tuple(getattr(t, 'shape', ()))}")
            if t.dtype != torch.float32:
                raise _lib.GmpcError(f"{who}: {name} must be float32, got {t.dtype}")
            if tuple(t.shape[:2]) != tuple(xseq.shape[:2]):
                raise _lib.GmpcError(f"{who}: {name} must share xseq's (D, S) = {tuple(xseq.shape[:2])}, got "
                                     f"{tuple(t.shape[:2])}")
        D, S = int(xseq.shape[0]), int(xseq.shape[1])
        B = D
        if rows is not None:
            shape = tuple(getattr(rows, "shape", ()))
            if len(shape) != 2 or shape[0] != P:
                raise _lib.GmpcError(f"{who}: rows must be ({P}, B), got shape {shape}")
            dtype = rows.dtype if torch.is_tensor(rows) else np.asarray(rows).dtype
            if dtype not in (torch.int32, np.dtype(np.int32)):
                raise _lib.GmpcError(f"{who}: rows must be int32, got {dtype}")
            B = int(shape[1])
            if B > 0:
                lo, hi = int(rows.min()), int(rows.max())
                if lo < 0 or hi >= D:
                    raise _lib.GmpcError(f"{who}: rows must lie in [0, D = {D}), got [{lo}, {hi}]")
            rows = self.to_dev(rows, dtype=torch.int32)
        for name, t, shape in (("loss_sum", loss_sum, (P,)), ("grad_sum", grad_sum, (P, self.dyn_count))):
            if t is not None and tuple(t.shape) != shape:
                raise _lib.GmpcError(f"{who}: {name} must be {shape}, got {tuple(t.shape)}")
        loss_sum = self.new(P) if loss_sum is None else loss_sum
        grad_sum = self.new(P, self.dyn_count) if grad_sum is None else grad_sum
        _lib.check(self.lib.gmpc_dynamics_ensemble_loss_grad(
            self.ctx, P, _ptr(members), D, B, S, _ptr(xseq), _ptr(useq), _ptr(next_xseq), _ptr(rows), float(discount),
            int(bool(teacher_forcing)), _ptr(loss_sum), _ptr(grad_sum), self._stream()))
        return loss_sum, grad_sum

    ENSEMBLE_ROLLOUT_WANT = ("X", "costs", "obj", "mean", "var")

    def ensemble_rollout(self, members, x0, U, goal=None, want=("X", "obj")):
        """A plan's rollout under every member of a dynamics ensemble, in one launch (gmpc_ensemble_rollout; DESIGN.md
        section 27).  members: float32 (P, dyn_count) tensor or array, 1 <= P <= 16, as set_sampled_ensemble takes
        them, passed per call; x0 (B, n), U (B, S, m) with 1 <= S <= T, goal (B, T + 1, n) or None: float32 device
        tensors.  -> a dict of the `want`ed tensors: "X" (P, B, S + 1, n) the members' states, "costs" (P, B, T + 1)
        the stage costs and the terminal cost, "obj" (P, B) their sum, "mean" / "var" (B, S + 1, n) the members' mean
        and population variance per step and state.  "costs" and "obj" need goal and S == T.  X[p] and obj[p] are
        bitwise what cem_solve(max_iter=0) returns for U on an engine bound to member p.  Stateless: the bound mpc_w
        and cost network are read; a set ensemble, its mode, the sampled precision and a held solution stay as they
        are.  Every refusal is a GmpcError("ensemble rollout: ..."); nothing is synchronised."""
        who = "ensemble rollout"
        P = self._check_ensemble_members(who, members)
        want = (want,) if isinstance(want, str) else tuple(want)
        unknown = set(want) - set(self.ENSEMBLE_ROLLOUT_WANT)
        if unknown:
            raise _lib.GmpcError(f"{who}: want has unknown entries {sorted(unknown, key=str)}; known: "
                                 f"{self.ENSEMBLE_ROLLOUT_WANT}")
        if not want:
            raise _lib.GmpcError(f"{who}: want is empty; known: {self.ENSEMBLE_ROLLOUT_WANT}")
        if goal is None and ("costs" in want or "obj" in want):
            raise _lib.GmpcError(f'{who}: "costs" and "obj" need goal (want = {want})')
        n, m, T = self.n, self.m, self.T
        for name, t in (("x0", x0), ("U", U), ("goal", goal)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32):
                raise _lib.GmpcError(f"{who}: {name} must be a float32 tensor, got "
                                     f"{getattr(t, 'dtype', type(t).__name__)}")
        if x0.dim() != 2 or x0.shape[1] != n:
            raise _lib.GmpcError(f"{who}: x0 must be (B, {n}), got {tuple(x0.shape)}")
        B = int(x0.shape[0])
        if U.dim() != 3 or U.shape[0] != B or U.shape[2] != m:
            raise _lib.GmpcError(f"{who}: U must be ({B}, S, {m}), got {tuple(U.shape)}")
        S = int(U.shape[1])
        if goal is not None and tuple(goal.shape) != (B, T + 1, n):
            raise _lib.GmpcError(f"{who}: goal must be {(B, T + 1, n)}, got {tuple(goal.shape)}")
        shapes = dict(X=(P, B, S + 1, n), costs=(P, B, T + 1), obj=(P, B), mean=(B, S + 1, n), var=(B, S + 1, n))
        out = {k: self.new(*shapes[k]) for k in self.ENSEMBLE_ROLLOUT_WANT if k in want}
        dev = self.to_dev(members)
        _lib.check(self.lib.gmpc_ensemble_rollout(
            self.ctx, B, S, P, _ptr(dev), _ptr(x0), _ptr(U), _ptr(goal), _ptr(out.get("X")), _ptr(out.get("costs")),
            _ptr(out.get("obj")), _ptr(out.get("mean")), _ptr(out.get("var")), self._stream()))
        return out

    ENSEMBLE_FEEDBACK_WANT = ("X", "U", "costs", "obj", "mean", "var")

    def ensemble_rollout_feedback(self, members, X_ref, U_ref, K, goal=None, x0=None, k=None, alpha=1.0, u_lo=None,
                                  u_hi=None, want=("X", "U", "obj")):
        """A reference trajectory tracked in closed loop under every member of a dynamics ensemble, in one launch
        (gmpc_ensemble_rollout_feedback): per member u_t = clamp(U_ref_t + K_t (x_t - X_ref_t)
        + alpha k_t, u_lo, u_hi), x_{t+1} = x_t + MLP_p([x_t; u_t]).  members as for ensemble_rollout; X_ref
        (B, S + 1, n), U_ref (B, S, m) with 1 <= S <= T, K (B, S, m, n) (lqr_backward's layout), goal (B, T + 1, n) or
        None, x0 (B, n) or None (then X_ref[:, 0]), k (B, S, m) or None (no feed-forward term): float32 device tensors;
        alpha a finite number; u_lo, u_hi as for ilqr_solve_box (None, a scalar or m values), both or neither.  -> a
        dict of the `want`ed tensors: "X" (P, B, S + 1, n) the members' states, "U" (P, B, S, m) the controls each
        member applied, "costs" (P, B, T + 1) and "obj" (P, B) on those controls, "mean" / "var" (B, S + 1, n) the
        members' moments per step and state.  "costs" and "obj" need goal and S == T.  With K = 0, no k and no bounds
        it is ensemble_rollout(members, x0, U_ref) bit for bit.  Stateless as ensemble_rollout is.  Every refusal is a
        GmpcError("ensemble feedback: ..."); nothing is synchronised."""
        who = "ensemble feedback"
        P = self._check_ensemble_members(who, members)
        want = (want,) if isinstance(want, str) else tuple(want)
        unknown = set(want) - set(self.ENSEMBLE_FEEDBACK_WANT)
        if unknown:
            raise _lib.GmpcError(f"{who}: want has unknown entries {sorted(unknown, key=str)}; known: "
                                 f"{self.ENSEMBLE_FEEDBACK_WANT}")
        if not want:
            raise _lib.GmpcError(f"{who}: want is empty; known: {self.ENSEMBLE_FEEDBACK_WANT}")
        if goal is None and ("costs" in want or "obj" in want):
            raise _lib.GmpcError(f'{who}: "costs" and "obj" need goal (want = {want})')
        n, m, T = self.n, self.m, self.T
        for name, t in (("X_ref", X_ref), ("U_ref", U_ref), ("K", K), ("goal", goal), ("x0", x0), ("k", k)):
            if name in ("X_ref", "U_ref", "K") and t is None:
                raise _lib.GmpcError(f"{who}: {name} must not be None")
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32):
                raise _lib.GmpcError(f"{who}: {name} must be a float32 tensor, got "
                                     f"{getattr(t, 'dtype', type(t).__name__)}")
        if U_ref.dim() != 3 or U_ref.shape[2] != m:
            raise _lib.GmpcError(f"{who}: U_ref must be (B, S, {m}), got {tuple(U_ref.shape)}")
        B, S = int(U_ref.shape[0]), int(U_ref.shape[1])
        if not 1 <= B <= self.max_batch:
            raise _lib.GmpcError(f"{who}: B = {B} outside [1, max_batch = {self.max_batch}]")
        if not 1 <= S <= T:
            raise _lib.GmpcError(f"{who}: S = {S} outside [1, T = {T}]")
        shapes = dict(X_ref=(B, S + 1, n), K=(B, S, m, n), goal=(B, T + 1, n), x0=(B, n), k=(B, S, m))
        for name, t in (("X_ref", X_ref), ("K", K), ("goal", goal), ("x0", x0), ("k", k)):
            if t is not None and tuple(t.shape) != shapes[name]:
                raise _lib.GmpcError(f"{who}: {name} must be {shapes[name]}, got {tuple(t.shape)}")
        for name, t in (("X_ref", X_ref), ("U_ref", U_ref), ("K", K), ("goal", goal), ("x0", x0), ("k", k)):
            if t is not None and not t.is_contiguous():
                raise _lib.GmpcError(f"{who}: {name} must be contiguous")
        try:
            alpha = float(alpha)
        except (TypeError, ValueError):
            raise _lib.GmpcError(f"{who}: alpha must be a finite number, got {alpha!r}") from None
        if not np.isfinite(alpha):
            raise _lib.GmpcError(f"{who}: alpha must be a finite number, got {alpha!r}")
        if (u_lo is None) != (u_hi is None):
            raise _lib.GmpcError(f"{who}: u_lo and u_hi must both be given or both be None")
        lo_d = hi_d = None
        if u_lo is not None:
            try:
                _, _, lo_d, hi_d = self._device_bounds(u_lo, u_hi)
            except _lib.GmpcError as e:
                raise _lib.GmpcError(f"{who}: {e}") from None
        if S != T and ("costs" in want or "obj" in want):
            raise _lib.GmpcError(f'{who}: "costs" and "obj" need the whole horizon, S = {S} is not T = {T}')
        shapes = dict(X=(P, B, S + 1, n), U=(P, B, S, m), costs=(P, B, T + 1), obj=(P, B), mean=(B, S + 1, n),
                      var=(B, S + 1, n))
        out = {key: self.new(*shapes[key]) for key in self.ENSEMBLE_FEEDBACK_WANT if key in want}
        dev = self.to_dev(members)
        _lib.check(self.lib.gmpc_ensemble_rollout_feedback(
            self.ctx, B, S, P, _ptr(dev), _ptr(x0), _ptr(X_ref), _ptr(U_ref), _ptr(K), _ptr(k), alpha, _ptr(lo_d),
            _ptr(hi_d), _ptr(goal), _ptr(out.get("X")), _ptr(out.get("U")), _ptr(out.get("costs")),
            _ptr(out.get("obj")), _ptr(out.get("mean")), _ptr(out.get("var")), self._stream()))
        return out

    ENSEMBLE_DISAGREEMENT_WANT = ("X", "d", "D")

    def ensemble_disagreement(self, members, x0, U, want=("d", "D")):
        """The one-step disagreement of every member with the bound (nominal) dynamics along a plan, in one launch
        (gmpc_ensemble_disagreement).  members, x0 (B, n), U (B, S, m) with 1 <= S <= T as for
        ensemble_rollout.  -> a dict of the `want`ed tensors: "X" (B, S + 1, n) the nominal rollout, "d" (P, B, S) the
        squared deviation of member p's one-step output from the nominal one at every visited (x_t, u_t), "D" (P, B)
        its sum over the steps.  fp32; the arithmetic is that of the solves under set_sampled_disagreement.
        Stateless: the bound dynamics are read; the set ensemble, its mode, the disagreement setting, the sampled
        precision and a held solution stay as they are.  Every refusal is a GmpcError("ensemble disagreement: ...");
        nothing is synchronised."""
        who = "ensemble disagreement"
        P = self._check_ensemble_members(who, members)
        want = (want,) if isinstance(want, str) else tuple(want)
        unknown = set(want) - set(self.ENSEMBLE_DISAGREEMENT_WANT)
        if unknown:
            raise _lib.GmpcError(f"{who}: want has unknown entries {sorted(unknown, key=str)}; known: "
                                 f"{self.ENSEMBLE_DISAGREEMENT_WANT}")
        if not want:
            raise _lib.GmpcError(f"{who}: want is empty; known: {self.ENSEMBLE_DISAGREEMENT_WANT}")
        n, m = self.n, self.m
        for name, t in (("x0", x0), ("U", U)):
            if not torch.is_tensor(t) or t.dtype != torch.float32:
                raise _lib.GmpcError(f"{who}: {name} must be a float32 tensor, got "
                                     f"{getattr(t, 'dtype', type(t).__name__)}")
        if x0.dim() != 2 or x0.shape[1] != n:
            raise _lib.GmpcError(f"{who}: x0 must be (B, {n}), got {tuple(x0.shape)}")
        B = int(x0.shape[0])
        if U.dim() != 3 or U.shape[0] != B or U.shape[2] != m:
            raise _lib.GmpcError(f"{who}: U must be ({B}, S, {m}), got {tuple(U.shape)}")
        S = int(U.shape[1])
        shapes = dict(X=(B, S + 1, n), d=(P, B, S), D=(P, B))
        out = {k: self.new(*shapes[k]) for k in self.ENSEMBLE_DISAGREEMENT_WANT if k in want}
        dev = self.to_dev(members)
        _lib.check(self.lib.gmpc_ensemble_disagreement(
            self.ctx, B, S, P, _ptr(dev), _ptr(x0), _ptr(U), _ptr(out.get("X")), _ptr(out.get("d")),
            _ptr(out.get("D")), self._stream()))
        return out

    ENSEMBLE_ROLLOUT_VJP_WANT = ("x0", "U", "goal", "theta", "members")

    def ensemble_rollout_vjp(self, members, X, U, goal, gX=None, gcost=None,
                             want=("x0", "U", "goal", "theta", "members")):
        """The VJP of ensemble_rollout's X and costs under every member, in one call (gmpc_ensemble_rollout_vjp;
        DESIGN.md section 29).  members: float32 (P, dyn_count) tensor or array, 1 <= P <= 16, passed per call; X
        (P, B, T + 1, n) the members' states for U (B, T, m), as ensemble_rollout returns them; goal (B, T + 1, n);
        gX (P, B, T + 1, n) = dL/dX and / or gcost (P, B, T + 1) = dL/dcosts: float32 device tensors.  -> a dict of
        the `want`ed tensors: "x0" (B, n), "U" (B, T, m), "goal" (B, T + 1, n) the members' gradients summed in
        ascending member order, "theta" [3 + cost_count] summed over the batch and the members, "members"
        (P, dyn_count) summed over the batch, one row per member.  Stateless as ensemble_rollout is.  Every refusal is
        a GmpcError("ensemble rollout vjp: ..."); nothing is synchronised."""
        who = "ensemble rollout vjp"
        P = self._check_ensemble_members(who, members)
        want = (want,) if isinstance(want, str) else tuple(want)
        unknown = set(want) - set(self.ENSEMBLE_ROLLOUT_VJP_WANT)
        if unknown:
            raise _lib.GmpcError(f"{who}: want has unknown entries {sorted(unknown, key=str)}; known: "
                                 f"{self.ENSEMBLE_ROLLOUT_VJP_WANT}")
        if not want:
            raise _lib.GmpcError(f"{who}: want is empty; known: {self.ENSEMBLE_ROLLOUT_VJP_WANT}")
        if gX is None and gcost is None:
            raise _lib.GmpcError(f"{who}: gX and gcost are both None: no cotangent")
        n, m, T = self.n, self.m, self.T
        for name, t in (("X", X), ("U", U), ("goal", goal), ("gX", gX), ("gcost", gcost)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32):
                raise _lib.GmpcError(f"{who}: {name} must be a float32 tensor, got "
                                     f"{getattr(t, 'dtype', type(t).__name__)}")
        if X.dim() != 4 or X.shape[0] != P or tuple(X.shape[2:]) != (T + 1, n):
            raise _lib.GmpcError(f"{who}: X must be ({P}, B, {T + 1}, {n}), got {tuple(X.shape)}")
        B = int(X.shape[1])
        for name, t, shape in (("U", U, (B, T, m)), ("goal", goal, (B, T + 1, n)), ("gX", gX, (P, B, T + 1, n)),
                               ("gcost", gcost, (P, B, T + 1))):
            if t is not None and tuple(t.shape) != shape:
                raise _lib.GmpcError(f"{who}: {name} must be {shape}, got {tuple(t.shape)}")
        shapes = dict(x0=(B, n), U=(B, T, m), goal=(B, T + 1, n), theta=(3 + self.cost_count,),
                      members=(P, self.dyn_count))
        out = {k: self.new(*shapes[k]) for k in self.ENSEMBLE_ROLLOUT_VJP_WANT if k in want}
        dev = self.to_dev(members)
        _lib.check(self.lib.gmpc_ensemble_rollout_vjp(
            self.ctx, B, P, _ptr(dev), _ptr(X), _ptr(U), _ptr(goal), _ptr(gX), _ptr(gcost), _ptr(out.get("x0")),
            _ptr(out.get("U")), _ptr(out.get("goal")), _ptr(out.get("theta")), _ptr(out.get("members")),
            self._stream()))
        return out

    ENSEMBLE_DISAGREEMENT_VJP_WANT = ("x0", "U", "nominal", "members")

    def ensemble_disagreement_vjp(self, members, X, U, gd=None, gD=None, want=("x0", "U", "nominal", "members")):
        """The VJP of ensemble_disagreement's d and D, in one call (gmpc_ensemble_disagreement_vjp; DESIGN.md section
        30).  members: float32 (P, dyn_count) tensor or array, 1 <= P <= 16, passed per call; X (B, T + 1, n) the
        nominal rollout for U (B, T, m), as ensemble_disagreement returns it (the whole horizon); gd (P, B, T) = dL/dd
        and / or gD (P, B) = dL/dD: float32 device tensors.  -> a dict of the `want`ed tensors: "x0" (B, n) and "U"
        (B, T, m), through the members' and the nominal one-step outputs and through the nominal rollout; "nominal"
        [dyn_count] w.r.t. the bound dynamics and "members" (P, dyn_count), one row per member, both summed over the
        batch.  Stateless as ensemble_disagreement is.  Every refusal is a GmpcError("ensemble disagreement vjp:
        ..."); nothing is synchronised."""
        who = "ensemble disagreement vjp"
        P = self._check_ensemble_members(who, members)
        want = (want,) if isinstance(want, str) else tuple(want)
        unknown = set(want) - set(self.ENSEMBLE_DISAGREEMENT_VJP_WANT)
        if unknown:
            raise _lib.GmpcError(f"{who}: want has unknown entries {sorted(unknown, key=str)}; known: "
                                 f"{self.ENSEMBLE_DISAGREEMENT_VJP_WANT}")
        if not want:
            raise _lib.GmpcError(f"{who}: want is empty; known: {self.ENSEMBLE_DISAGREEMENT_VJP_WANT}")
        if gd is None and gD is None:
            raise _lib.GmpcError(f"{who}: gd and gD are both None: no cotangent")
        n, m, T = self.n, self.m, self.T
        for name, t in (("X", X), ("U", U), ("gd", gd), ("gD", gD)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32):
                raise _lib.GmpcError(f"{who}: {name} must be a float32 tensor, got "
                                     f"{getattr(t, 'dtype', type(t).__name__)}")
        if X.dim() != 3 or tuple(X.shape[1:]) != (T + 1, n):
            raise _lib.GmpcError(f"{who}: X must be (B, {T + 1}, {n}), got {tuple(X.shape)}")
        B = int(X.shape[0])
        for name, t, shape in (("U", U, (B, T, m)), ("gd", gd, (P, B, T)), ("gD", gD, (P, B))):
            if t is not None and tuple(t.shape) != shape:
                raise _lib.GmpcError(f"{who}: {name} must be {shape}, got {tuple(t.shape)}")
        X, U = X.contiguous(), U.contiguous()
        gd = None if gd is None else gd.contiguous()
        gD = None if gD is None else gD.contiguous()
        shapes = dict(x0=(B, n), U=(B, T, m), nominal=(self.dyn_count,), members=(P, self.dyn_count))
        out = {k: self.new(*shapes[k]) for k in self.ENSEMBLE_DISAGREEMENT_VJP_WANT if k in want}
        dev = self.to_dev(members)
        _lib.check(self.lib.gmpc_ensemble_disagreement_vjp(
            self.ctx, B, P, _ptr(dev), _ptr(X), _ptr(U), _ptr(gd), _ptr(gD), _ptr(out.get("x0")), _ptr(out.get("U")),
            _ptr(out.get("nominal")), _ptr(out.get("members")), self._stream()))
        return out

    def _check_ensemble_members(self, who, members):
        """The rank, width, count and dtype of a (P, dyn_count) float32 tensor or array -> P."""
        shape = tuple(getattr(members, "shape", ()))
        if len(shape) != 2 or shape[1] != self.dyn_count:
            raise _lib.GmpcError(f"{who}: members must be (P, {self.dyn_count}), got shape {shape}")
        if not 1 <= shape[0] <= self.MAX_ENSEMBLE:
            raise _lib.GmpcError(f"{who}: P = {shape[0]} outside [1, {self.MAX_ENSEMBLE}]")
        dtype = members.dtype if torch.is_tensor(members) else np.asarray(members).dtype
        if dtype not in (torch.float32, np.dtype(np.float32)):
            raise _lib.GmpcError(f"{who}: members must be float32, got {dtype}")
        return int(shape[0])

    def polyak(self, prev, cur, factor, out=None):
        out = cur if out is None else out
        _lib.check(self.lib.gmpc_polyak(self.ctx, prev.numel(), _ptr(prev), _ptr(cur), float(factor),
                                        _ptr(out), self._stream()))
        return out

    def critic_loss_grad(self, xseq, label, critic, loss_sum=None, grad_sum=None):
        """loss_sum [1], grad_sum [critic_count]: optional caller-owned views (a packed all-reduce buffer)."""
        Bc = xseq.shape[0]
        loss_sum = self.new(1) if loss_sum is None else loss_sum
        grad_sum = self.new(self.critic_count) if grad_sum is None else grad_sum
        assert loss_sum.numel() == 1 and grad_sum.numel() == self.critic_count
        _lib.check(self.lib.gmpc_critic_loss_grad(self.ctx, Bc, _ptr(xseq), _ptr(label), _ptr(critic),
                                                  _ptr(loss_sum), _ptr(grad_sum), self._stream()))
        return loss_sum, grad_sum

    def critic_score_vjp(self, xseq, critic, want_dx=True):
        Bc = xseq.shape[0]
        score = self.new(Bc)
        dx = self.new(Bc, self.T + 1, self.nx) if want_dx else None
        _lib.check(self.lib.gmpc_critic_score_vjp(self.ctx, Bc, _ptr(xseq), _ptr(critic), _ptr(score),
                                                  _ptr(dx), self._stream()))
        return score, dx

    def critic_vjp(self, xseq, critic, g_score, want_dx=True, want_params=True, grad_sum=None):
        """The VJP of the critic's scores at (critic, xseq) for g_score = dL/dscore (Bc,) (gmpc_critic_vjp).
        -> dict(score (Bc,), dx (Bc, T+1, nx) = g_b dscore_b/dxseq_b, params [critic_count] = sum_b g_b dscore_b/dtheta
        in critic_loss_grad's layout), None where not wanted.  grad_sum: optional caller-owned [critic_count] view
        (e.g. of a packed all-reduce buffer) for params.  Stateless: a held iLQR solution and its bilevel tail stay
        valid."""
        Bc = xseq.shape[0]
        for name, t, shape in (("xseq", xseq, (Bc, self.T + 1, self.nx)), ("critic", critic, (self.critic_count,)),
                               ("g_score", g_score, (Bc,))):
            if tuple(t.shape) != shape:
                raise _lib.GmpcError(f"critic_vjp: {name} must be {shape}, got {tuple(t.shape)}")
        if grad_sum is not None and (not want_params or tuple(grad_sum.shape) != (self.critic_count,)):
            raise _lib.GmpcError(f"critic_vjp: grad_sum must be ({self.critic_count},) and goes with want_params, got "
                                 f"{tuple(grad_sum.shape)}, want_params={want_params}")
        out = dict(score=self.new(Bc), dx=self.new(Bc, self.T + 1, self.nx) if want_dx else None,
                   params=(self.new(self.critic_count) if grad_sum is None else grad_sum) if want_params else None)
        _lib.check(self.lib.gmpc_critic_vjp(self.ctx, Bc, _ptr(xseq), _ptr(critic), _ptr(g_score), _ptr(out["score"]),
                                            _ptr(out["dx"]), _ptr(out["params"]), self._stream()))
        return out

    def critic_dir_vjp(self, xseq, critic, v, g_dir=None, want_dx=True, want_params=True, grad_sum=None):
        """The second-order VJP of the critic's scores (gmpc_critic_dir_vjp): sdot_b = <dscore_b/dxseq_b, v_b> for the
        directions v (Bc, T+1, nx), and for g_dir = dL/dsdot (Bc,) its reverse sweep.  -> dict(score (Bc,), sdot (Bc,),
        dx (Bc, T+1, nx) = g_b dsdot_b/dxseq_b, params [critic_count] = sum_b g_b dsdot_b/dtheta in critic_loss_grad's
        layout, head biases exactly zero), None where not wanted.  Without g_dir the call is the forward only: dx and
        params are None whatever want_dx / want_params say.  grad_sum: optional caller-owned [critic_count] view for
        params.  Critics with nx + lstm_features <= 256.  Stateless, as critic_vjp."""
        Bc = xseq.shape[0]
        for name, t, shape in (("xseq", xseq, (Bc, self.T + 1, self.nx)), ("critic", critic, (self.critic_count,)),
                               ("v", v, (Bc, self.T + 1, self.nx)), ("g_dir", g_dir, (Bc,))):
            if t is not None and tuple(t.shape) != shape:
                raise _lib.GmpcError(f"critic_dir_vjp: {name} must be {shape}, got {tuple(t.shape)}")
        want_dx, want_params = bool(want_dx and g_dir is not None), bool(want_params and g_dir is not None)
        if grad_sum is not None and (not want_params or tuple(grad_sum.shape) != (self.critic_count,)):
            raise _lib.GmpcError(f"critic_dir_vjp: grad_sum must be ({self.critic_count},) and goes with want_params and "
                                 f"g_dir, got {tuple(grad_sum.shape)}, want_params={want_params}")
        out = dict(score=self.new(Bc), sdot=self.new(Bc), dx=self.new(Bc, self.T + 1, self.nx) if want_dx else None,
                   params=(self.new(self.critic_count) if grad_sum is None else grad_sum) if want_params else None)
        _lib.check(self.lib.gmpc_critic_dir_vjp(self.ctx, Bc, _ptr(xseq), _ptr(critic), _ptr(v), _ptr(g_dir),
                                                _ptr(out["score"]), _ptr(out["sdot"]), _ptr(out["dx"]),
                                                _ptr(out["params"]), self._stream()))
        return out

    def adam_clip_step(self, params, grad, m, v, step, lr, grad_scale=1.0, max_norm=100.0, b1=0.9,
                       b2=0.999, eps=1e-8):
        _lib.check(self.lib.gmpc_adam_clip_step(
            self.ctx, params.numel(), _ptr(params), _ptr(grad), _ptr(m), _ptr(v), float(grad_scale),
            int(step), float(lr), float(max_norm), float(b1), float(b2), float(eps), self._stream()))

    def set_linearize_event(self, event=None):
        """Record `event` (a torch.cuda.Event that has been recorded once, or None) after the Jacobian chain of
        every backward pass: gmpc_set_linearize_event.  The caller keeps the event alive."""
        import ctypes as C
        h = None if event is None else C.c_void_p(event.cuda_event)
        _lib.check(self.lib.gmpc_set_linearize_event(self.ctx, h))
        self._lin_event = event

    def linesearch_candidates(self):
        """Candidate rollouts evaluated by the line searches of the last ilqr_solve."""
        return int(self.lib.gmpc_linesearch_candidates(self.ctx))

    def linesearch_stats(self):
        """Counters of the last ilqr_solve's line searches: how many accepted alpha_0 / 2^k (list `accepted`,
        k = 0..15), how many ran out of step sizes, candidate rollouts per speculative round."""
        out = (C.c_long * 64)()
        _lib.check(self.lib.gmpc_linesearch_stats(self.ctx, out, 64))
        v = list(out)
        rounds = v[24:64]
        while rounds and rounds[-1] == 0:
            rounds.pop()
        return {"accepted": v[:16], "exhausted": v[16], "deepest_accepted": v[17], "round_items": rounds}

    PROF_SLOTS = ("rollout", "linearize", "terminal", "riccati", "linesearch", "lstm_fwd", "head",
                  "lstm_bwd", "wgrad", "adam")

    def profile_enable(self, on=True):
        _lib.check(self.lib.gmpc_profile_enable(self.ctx, int(bool(on))))

    def profile_read(self):
        """{kernel: (total_ms, launches)} since the last read (HIP events on the launch stream)."""
        out = {}
        for i, name in enumerate(self.PROF_SLOTS):
            ms, cnt = C.c_double(), C.c_int()
            _lib.check(self.lib.gmpc_profile_read(self.ctx, i, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out

    def profile_kernel_name(self, slot_name):
        """Name of the kernel the slot's last launch ran on ('' when the slot has one kernel only)."""
        name = self.lib.gmpc_profile_kernel_name(self.ctx, self.PROF_SLOTS.index(slot_name))
        return name.decode() if name else ""

    def debug_buffer(self, which, shape):
        """Copy of one of the ctx's internal solution buffers (see gmpc_debug_buffer)."""
        p = self.lib.gmpc_debug_buffer(self.ctx, which)
        if not p:
            raise _lib.GmpcError(f"no debug buffer {which}")
        n = int(np.prod(shape))
        have = self.lib.gmpc_debug_buffer_count(self.ctx, which)
        if n > have:
            raise _lib.GmpcError(f"debug buffer {which} holds {have} floats, {n} requested {tuple(shape)}")
        torch.cuda.synchronize(self.device)
        view = torch.as_tensor(_RawDevBuffer(p, n), device=self.device)
        return view.clone().reshape(shape)


class _RawDevBuffer:
    """__cuda_array_interface__ view of a raw fp32 device pointer."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {
            "shape": (count,), "typestr": "<f4", "data": (int(ptr), False), "version": 2}
