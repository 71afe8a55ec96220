"""Reference of gmpc_critic_dir_vjp (TEST INFRASTRUCTURE, no GPU import): torch's double backward of
critic_vjp_ref.forward_t.  sdot_b = <dscore_b/dxseq_b, v_b>; for g_dir = dL/dsdot the gradients of sum_b g_b sdot_b
w.r.t. the flat parameters and the sequences.  fp64 by default; dtype=np.float32 gives the fp32 reference of the parity
protocol.  Checked against the oracle by tests/test_critic_dir_vjp_host.py."""

import numpy as np
import torch

import critic_cases as cc
import critic_vjp_ref as V
import gan_mpc_oracle as orc
import gpu_util as gu


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype))


def dir_vjp(flat, n, F, head_dims, xseq, v, g_dir, dtype=np.float64):
    """(score (Bc,), sdot (Bc,), grad_params [count] = sum_b g_b dsdot_b/dflat, grad_xseq (Bc, T1, n) =
    g_b dsdot_b/dxseq_b)."""
    fl = _t(flat, dtype).requires_grad_(True)
    xs = _t(xseq, dtype).requires_grad_(True)
    score = V.forward_t(fl, n, F, head_dims, xs)
    gx, = torch.autograd.grad(score.sum(), xs, create_graph=True)
    sdot = (gx * _t(v, dtype)).sum((1, 2))
    gp, gxx = torch.autograd.grad((sdot * _t(g_dir, dtype)).sum(), (fl, xs))
    return score.detach().numpy(), sdot.detach().numpy(), gp.numpy(), gxx.numpy()


def case_v(case):
    """The direction of a case: standard normal, seeded from the case."""
    n, F, T, Bc, head, seed = case
    return np.random.default_rng(3000 + seed).standard_normal((Bc, T + 1, n)).astype(np.float32)


def case_gdir(case):
    """The delta on sdot of a case: standard normal, seeded from the case."""
    n, F, T, Bc, head, seed = case
    return np.random.default_rng(4000 + seed).standard_normal(Bc).astype(np.float32)


def outputs(flat, n, F, head, xseq, v, g, dtype=np.float64):
    """The compared blocks of one call: sdot, the gradient blocks of split_critic_flat of grad_params / Bc, then dx, dx
    at t = 0 and dx at t = T1 - 1."""
    dims = (F,) + tuple(head) + (1,)
    Bc = xseq.shape[0]
    _, sdot, gp, dx = dir_vjp(flat, n, F, dims, xseq, v, g, dtype)
    return ([("sdot", sdot)] + gu.split_critic_flat(gp / Bc, n, F, dims)
            + [("dx", dx), ("dx t=0", dx[:, 0]), ("dx t=T1-1", dx[:, -1])])


def sensitivity(case, v, g, trials=8, rel=2.0 ** -23):
    """critic_vjp_ref.sensitivity for this call: {block: elementwise change of the fp64 result when every parameter and
    input (v and g included) is perturbed by one fp32 ulp (relative Gaussian, largest over `trials` draws)}.  Blocks:
    see outputs()."""
    n, F, T, Bc, head, seed = case
    pb, xseq, _, _ = cc.make_case(case)
    flat = V.flat_of(orc.cast_problem(pb, np.float64)["critic"])
    x, v, g = (np.asarray(a, np.float64) for a in (xseq, v, g))
    ref = outputs(flat, n, F, head, x, v, g)
    rng = np.random.default_rng(seed)

    def pert(a):
        return a * (1 + rel * rng.standard_normal(a.shape))
    worst = {name: 0.0 for name, _ in ref}
    for _ in range(trials):
        for (name, a), (_, r) in zip(outputs(pert(flat), n, F, head, pert(x), pert(v), pert(g)), ref):
            worst[name] = max(worst[name], gu.el_err(a, r)[0])
    return worst


def penalty_points(xs, lab, at, eps):
    """GAN_MPC's penalty points: the true sequences, or eps_k true_k + (1 - eps_k) pred_k in batch order."""
    true, pred = xs[lab > 0], xs[~(lab > 0)]
    if at == "true":
        return true
    P = min(len(true), len(pred))
    e = np.asarray(eps, xs.dtype)[:P, None, None]
    return e * true[:P] + (1 - e) * pred[:P]


def penalty_loss_grad(flat, n, F, head_dims, xs, lab, weight, target, at, eps=None, dtype=np.float64):
    """GAN_MPC(objective="wgan", gradient_penalty=dict(weight, target, at))'s critic step on one rank: (mean of
    -label score + weight * mean penalty, its gradient w.r.t. flat, the penalty points' gradient norms (P,))."""
    xs, lab = np.asarray(xs, dtype), np.asarray(lab, dtype)
    fl = _t(flat, dtype).requires_grad_(True)
    score = V.forward_t(fl, n, F, head_dims, _t(xs, dtype))
    loss = (-_t(lab, dtype) * score).mean()
    xhat = penalty_points(xs, lab, at, eps)
    norms = np.zeros(0)
    if len(xhat) > 0:
        xh = _t(xhat, dtype).requires_grad_(True)
        g, = torch.autograd.grad(V.forward_t(fl, n, F, head_dims, xh).sum(), xh, create_graph=True)
        nrm = torch.linalg.vector_norm(g.reshape(len(xhat), -1), dim=1)
        loss = loss + weight * ((nrm - target) ** 2).mean()
        norms = nrm.detach().numpy()
    grad, = torch.autograd.grad(loss, fl)
    return float(loss.detach()), grad.numpy(), norms
