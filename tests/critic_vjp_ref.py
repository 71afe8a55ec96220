"""Reference of gmpc_critic_vjp (TEST INFRASTRUCTURE, no GPU import): a torch transcription of the critic forward -- the
LSTM scan from a zero carry (gate order i, f, g, o), then the relu head -- over the flat vector of params.pack_critic,
differentiated by torch.autograd.  fp64 by default; dtype=np.float32 gives the fp32 reference of the parity protocol.
Checked against the oracle by tests/test_critic_vjp_host.py."""

import numpy as np
import torch

import critic_cases as cc
import gan_mpc_oracle as orc
import gpu_util as gu


def unflatten(flat, n, F, head_dims):
    """Views of a flat torch vector in pack_critic's layout: Wx (n, 4F), Wh (F, 4F), b (4F), head [(W, b), ...];
    head_dims = (F, hidden..., 1)."""
    o = 0

    def take(*shape):
        nonlocal o
        cnt = int(np.prod(shape))
        v = flat[o:o + cnt].reshape(shape)
        o += cnt
        return v
    Wx, Wh, b = take(n, 4 * F), take(F, 4 * F), take(4 * F)
    head = [(take(K, N), take(N)) for K, N in zip(head_dims[:-1], head_dims[1:])]
    assert o == flat.numel(), (o, flat.numel())
    return Wx, Wh, b, head


def forward_t(flat, n, F, head_dims, xseq):
    """score (Bc,) as a torch expression of flat and xseq (Bc, T1, n)."""
    Wx, Wh, b, head = unflatten(flat, n, F, head_dims)
    Bc, T1, _ = xseq.shape
    c = torch.zeros(Bc, F, dtype=xseq.dtype)
    h = torch.zeros(Bc, F, dtype=xseq.dtype)
    for t in range(T1):
        z = xseq[:, t] @ Wx + h @ Wh + b
        i, f = torch.sigmoid(z[:, :F]), torch.sigmoid(z[:, F:2 * F])
        g, o = torch.tanh(z[:, 2 * F:3 * F]), torch.sigmoid(z[:, 3 * F:])
        c = f * c + i * g
        h = o * torch.tanh(c)
    a = h
    for li, (W, bb) in enumerate(head):
        a = a @ W + bb
        if li < len(head) - 1:
            a = torch.relu(a)
    return a[:, 0]


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype))


def forward(flat, n, F, head_dims, xseq, dtype=np.float64):
    with torch.no_grad():
        return forward_t(_t(flat, dtype), n, F, head_dims, _t(xseq, dtype)).numpy()


def vjp(flat, n, F, head_dims, xseq, g, dtype=np.float64):
    """(score (Bc,), grad_params [count] = sum_b g_b dscore_b/dflat, grad_xseq (Bc, T1, n) = g_b dscore_b/dxseq_b)."""
    fl = _t(flat, dtype).requires_grad_(True)
    xs = _t(xseq, dtype).requires_grad_(True)
    score = forward_t(fl, n, F, head_dims, xs)
    gp, gx = torch.autograd.grad((score * _t(g, dtype)).sum(), (fl, xs))
    return score.detach().numpy(), gp.numpy(), gx.numpy()


def flat_of(cr, dtype=np.float64):
    """pack_critic's order from the oracle's critic dict, without its cast to fp32."""
    out = [cr["Wx"].reshape(-1), cr["Wh"].reshape(-1), cr["b"].reshape(-1)]
    for W, b in cr["head"]:
        out += [np.asarray(W).reshape(-1), np.asarray(b).reshape(-1)]
    return np.concatenate(out).astype(dtype)


def case_g(case):
    """The output delta of a case: standard normal, seeded from the case."""
    n, F, T, Bc, head, seed = case
    return np.random.default_rng(2000 + seed).standard_normal(Bc).astype(np.float32)


def outputs(flat, n, F, head, xseq, g, dtype=np.float64):
    """The compared blocks of one VJP: the gradient blocks of split_critic_flat of grad_params / Bc, then dx, dx at
    t = 0 and dx at t = T1 - 1 -- critic_cases._outputs' list for this call."""
    dims = (F,) + tuple(head) + (1,)
    Bc = xseq.shape[0]
    if callable(g):          # an output delta that depends on the scores (a loss's own): g(score)
        g = g(forward(flat, n, F, dims, xseq, dtype))
    _, gp, dx = vjp(flat, n, F, dims, xseq, g, dtype)
    return gu.split_critic_flat(gp / Bc, n, F, dims) + [("dx", dx), ("dx t=0", dx[:, 0]), ("dx t=T1-1", dx[:, -1])]


def sensitivity(case, g, trials=8, rel=2.0 ** -23):
    """critic_cases.sensitivity for the VJP with output delta g: {block: elementwise change of the fp64 result when
    every parameter and input (g included) is perturbed by one fp32 ulp (relative Gaussian, largest over `trials`
    draws)}.  Blocks: see outputs()."""
    n, F, T, Bc, head, seed = case
    pb, xseq, _, _ = cc.make_case(case)
    flat = flat_of(orc.cast_problem(pb, np.float64)["critic"])
    return sensitivity_at(flat, n, F, head, xseq, g, seed, trials, rel)


def sensitivity_at(flat, n, F, head, xseq, g, seed=0, trials=8, rel=2.0 ** -23):
    """sensitivity() at given fp64 parameters and sequences; g an array, or a callable g(score) (not perturbed itself:
    it moves with the scores)."""
    x = np.asarray(xseq, np.float64)
    g = g if callable(g) else np.asarray(g, np.float64)
    ref = outputs(flat, n, F, head, x, g)
    rng = np.random.default_rng(seed)

    def pert(a):
        return a * (1 + rel * rng.standard_normal(a.shape))
    worst = {name: 0.0 for name, _ in ref}
    for _ in range(trials):
        for (name, a), (_, r) in zip(outputs(pert(flat), n, F, head, pert(x), g if callable(g) else pert(g)), ref):
            worst[name] = max(worst[name], gu.el_err(a, r)[0])
    return worst
