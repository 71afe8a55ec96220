"""GAN-MPC policy with a choice of adversarial objective: JS_MPC's interface with the critic's loss and the generator's
loss written in torch on top of critic_layer (policy/differentiable.py), so any function of the scores is an objective.

  objective = "js"     critic  softplus(-label score)              (= JS_MPC's BCE)    generator  -score
              "wgan"   critic  -label score                                             generator  -score
              "lsgan"  critic  (score - [label > 0])^2 / 2                              generator  (score - 1)^2 / 2
              "hinge"  critic  relu(1 - label score)                                    generator  -score
  or a pair of torch callables (critic_objective(score, label) -> (Bc,), generator_objective(score) -> (B,)): the loss
  of each sequence; label is +1 for a true sequence and -1 for a predicted one.

The critic step differentiates sum_b critic_objective through critic_layer's backward (one gmpc_critic_vjp call) and
joins the packed [loss | grad | count] all-reduce as JS_MPC does.  The generator step hands lx = d generator_objective /
dX -- through critic_layer again -- to the bilevel gradient as a batched cotangent (BaseMPC.batch_cotangents), with no
lu.  Plain torch.autograd only: no torch.func transform of the layer.

gradient_penalty = dict(weight, target=1.0, at="mixed" | "true", seed=0) adds weight * mean_p (||dscore/dxhat_p||_2 -
target)^2 to the critic's loss (critic_layer is differentiable twice in its sequences: one gmpc_critic_dir_vjp call):
  at = "true"   xhat = the batch's true sequences (label > 0); with target 0 this is the R1 penalty up to its factor 1/2
  at = "mixed"  xhat_k = eps_k true_k + (1 - eps_k) pred_k, the k-th true sequence with the k-th predicted one in batch
                order, P = the smaller of the two counts (WGAN-GP at target 1); eps ~ U[0, 1) from the device generator
                `penalty_generator`.
Per rank the packed sums get weight (Bc / P) sum_p penalty_p with count Bc, so a single rank reports mean objective +
weight * mean penalty; a shard without penalty points (P = 0) adds exact zeros and runs no kernel for it.  The generator
step does not see the penalty."""

import math

import torch
import torch.nn.functional as Fn

from gan_mpc_amd.gan import js_policy
from gan_mpc_amd.policy import differentiable as diff

OBJECTIVES = {
    "js": (lambda score, label: Fn.softplus(-label * score), lambda score: -score),
    "wgan": (lambda score, label: -label * score, lambda score: -score),
    "lsgan": (lambda score, label: 0.5 * (score - (label > 0).to(score.dtype)) ** 2,
              lambda score: 0.5 * (score - 1.0) ** 2),
    "hinge": (lambda score, label: torch.relu(1.0 - label * score), lambda score: -score),
}


def get_objective(objective):
    """(critic_objective, generator_objective) of a name in OBJECTIVES or of a pair of callables."""
    if isinstance(objective, str):
        if objective not in OBJECTIVES:
            raise ValueError(f"objective must be one of {sorted(OBJECTIVES)} or a pair of callables, got {objective!r}")
        return OBJECTIVES[objective]
    try:
        critic_obj, gen_obj = objective
    except (TypeError, ValueError):
        critic_obj = gen_obj = None
    if not (callable(critic_obj) and callable(gen_obj)):
        raise ValueError("objective must be a name or a pair (critic_objective(score, label), "
                         "generator_objective(score)) of callables")
    return critic_obj, gen_obj


def get_gradient_penalty(spec):
    """The validated penalty spec dict(weight, target, at, seed) of GAN_MPC's `gradient_penalty` argument, or None."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError(f"gradient_penalty must be None or a dict(weight, target=1.0, at='mixed', seed=0), got {spec!r}")
    unknown = sorted(set(spec) - {"weight", "target", "at", "seed"})
    if unknown:
        raise ValueError(f"gradient_penalty: unknown keys {unknown}; the keys are weight, target, at, seed")
    if "weight" not in spec:
        raise ValueError("gradient_penalty: weight is required")
    out = dict(weight=spec["weight"], target=spec.get("target", 1.0), at=spec.get("at", "mixed"), seed=spec.get("seed", 0))
    for key in ("weight", "target"):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"gradient_penalty: {key} must be a finite number >= 0, got {v!r}")
        out[key] = float(v)
    if out["at"] not in ("mixed", "true"):
        raise ValueError(f"gradient_penalty: at must be 'mixed' or 'true', got {out['at']!r}")
    if isinstance(out["seed"], bool) or not isinstance(out["seed"], int) or out["seed"] < 0:
        raise ValueError(f"gradient_penalty: seed must be an integer >= 0, got {out['seed']!r}")
    return out


def gradient_penalty(policy, dparams, flat, xhat, target, eng=None):
    """(P,) penalties (||dscore/dxhat_p||_2 - target)^2 of the policy's critic at the sequences xhat (P, T+1, x_size),
    the norm over all (T+1) x_size entries; differentiable w.r.t. flat (dparams.flat or a leaf sharing its storage):
    its backward is critic_layer's second derivative.  eng: the engine to run on (default: the policy's)."""
    eng = policy._engine if eng is None else eng
    xs = xhat.detach().to(torch.float32).contiguous().requires_grad_(True)
    with torch.enable_grad():
        score = diff.CriticFunction.apply(eng, dparams, flat, xs)
        g, = torch.autograd.grad(score.sum(), xs, create_graph=True)
        return (torch.linalg.vector_norm(g.reshape(g.shape[0], -1), dim=1) - target) ** 2


def _per_sequence(val, count, what):
    if tuple(val.shape) != (count,):
        raise ValueError(f"{what} must return one loss per sequence, shape ({count},), got {tuple(val.shape)}")
    return val


class GAN_MPC(js_policy.JS_MPC):
    def __init__(self, *args, objective="js", gradient_penalty=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.objective = objective
        self.critic_objective, self.generator_objective = get_objective(objective)
        self.gradient_penalty = get_gradient_penalty(gradient_penalty)
        self.penalty_generator = None
        if self.gradient_penalty is not None:
            # eps of the mixed sequences: a device generator of its own, so that a caller can replay its state
            self.penalty_generator = torch.Generator(device=self.device())
            self.penalty_generator.manual_seed(self.gradient_penalty["seed"])

    def penalty_points(self, xs, lab):
        """The sequences the penalty is taken at, (P, T+1, x_size): see the module docstring."""
        spec = self.gradient_penalty
        true = xs[lab > 0]
        if spec["at"] == "true":
            return true
        pred = xs[~(lab > 0)]
        P = min(true.shape[0], pred.shape[0])
        eps = torch.rand(P, generator=self.penalty_generator, device=xs.device, dtype=torch.float32)[:, None, None]
        return eps * true[:P] + (1.0 - eps) * pred[:P]

    # ---- critic step ------------------------------------------------------------------------
    def _critic_sums(self, batch_xseq, batch_label, dparams, packed=None):
        """Sums over this rank's shard of the critic objective and its gradient w.r.t. critic_params; with `packed`
        ([loss | grads | count], parallel.new_packed) they are written into that buffer."""
        Bc = batch_xseq.shape[0]
        eng = self.engine_for((Bc + 1) // 2, dparams)
        xs = batch_xseq if torch.is_tensor(batch_xseq) else eng.to_dev(batch_xseq)
        lab = batch_label if torch.is_tensor(batch_label) else eng.to_dev(batch_label)
        flat = dparams.flat.detach().requires_grad_(True)        # the same storage, a leaf of this step's graph
        with torch.enable_grad():
            score = diff.CriticFunction.apply(eng, dparams, flat, xs)
            loss = _per_sequence(self.critic_objective(score, lab.to(score.dtype)), Bc, "critic_objective").sum()
            if self.gradient_penalty is not None:
                xhat = self.penalty_points(xs.to(torch.float32), lab)
                if xhat.shape[0] > 0:
                    pen = gradient_penalty(self, dparams, flat, xhat, self.gradient_penalty["target"], eng=eng)
                    loss = loss + (self.gradient_penalty["weight"] * Bc / xhat.shape[0]) * pen.sum()
        grad, = torch.autograd.grad(loss, flat, allow_unused=True)
        lo, cnt = dparams.range_of(("critic_params",))
        gs = torch.zeros(cnt, dtype=torch.float32, device=xs.device) if grad is None else grad[lo:lo + cnt]
        ls = loss.detach().to(torch.float32)
        if packed is not None:
            packed[0] = ls
            packed[1:-1].copy_(gs)
            gs = packed[1:-1]
        return ls, gs

    # ---- generator step ---------------------------------------------------------------------
    def batch_cotangents(self, X, U, dparams, loss_args, want_grad=True):
        """(generator_objective(score(X)) [B], lx = its gradient w.r.t. X -- zero on the carry columns of LSTM
        dynamics --, None): the loss does not depend on U."""
        del U, loss_args
        B, nx = X.shape[0], self._engine.nx
        xs = X[..., :nx].detach().contiguous().requires_grad_(bool(want_grad))
        with torch.enable_grad():
            score = diff.critic_layer(self, dparams, xs)
            loss = _per_sequence(self.generator_objective(score), B, "generator_objective")
        if not want_grad:
            return loss.detach().to(torch.float32).contiguous(), None, None
        gx, = torch.autograd.grad(loss.sum(), xs)
        if nx < X.shape[-1]:
            lx = torch.zeros_like(X, dtype=torch.float32)
            lx[..., :nx] = gx
        else:
            lx = gx
        return loss.detach().to(torch.float32).contiguous(), lx.contiguous(), None

    def generator_loss(self, xcseq, useq, params, actual_xseq):
        del useq, actual_xseq
        with torch.no_grad():
            return self.generator_objective(self.critic_scores(xcseq, params))
