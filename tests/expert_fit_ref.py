"""Torch restatement of the expert model's training loss (TEST INFRASTRUCTURE): reference expert/nn.py:10-61
(LSTMCell / StackedMLPCell under nn.scan, zero initial carry, x_prev = xseq[0]) and expert/trainer.py:10-31
(calculate_loss), written over the flat vector of params.pack_expert so that autograd gives the gradient in
the layout gmpc_expert_loss_grad writes.  Runs in fp32 or fp64 on the CPU."""

import numpy as np
import torch


def unflatten(flat, F, dims_x, dims_u):
    """flat torch vector -> dict of views (lstm Wx/Wh/b or first W/b, head_x / head_u layer lists)."""
    n = dims_x[-1]
    off = [0]

    def take(*shape):
        size = int(np.prod(shape))
        v = flat[off[0]:off[0] + size].reshape(shape)
        off[0] += size
        return v

    ex = {}
    if F > 0:
        ex["lstm"] = dict(Wx=take(n, 4 * F), Wh=take(F, 4 * F), b=take(4 * F))
    else:
        ex["first"] = (take(n, dims_x[0]), take(dims_x[0]))
    for key, dims in (("head_x", dims_x), ("head_u", dims_u)):
        ex[key] = [(take(a, b), take(b)) for a, b in zip(dims[:-1], dims[1:])]
    assert off[0] == flat.numel()
    return ex


def _mlp(layers, y):
    for i, (W, b) in enumerate(layers):
        y = y @ W + b
        if i < len(layers) - 1:
            y = torch.relu(y)
    return y


def forward(ex, xseq, teacher_forcing):
    """xseq (B, S, n) -> next_x (B, S, n), u (B, S, m) of the scanned cell."""
    B, S, _ = xseq.shape
    lstm = ex.get("lstm")
    if lstm is not None:
        F = lstm["Wh"].shape[0]
        c = xseq.new_zeros(B, F)
        h = xseq.new_zeros(B, F)
    xprev = xseq[:, 0]
    nxs, us = [], []
    for t in range(S):
        x = xseq[:, t] if teacher_forcing else xprev        # jnp.where(teacher_forcing, x, xprev)
        if lstm is not None:
            z = x @ lstm["Wx"] + h @ lstm["Wh"] + lstm["b"]
            i, f, g, o = (z[:, k * F:(k + 1) * F] for k in range(4))
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            y = h
        else:
            W0, b0 = ex["first"]
            y = torch.relu(x @ W0 + b0)
        nx = _mlp(ex["head_x"], y) + x
        u = torch.tanh(_mlp(ex["head_u"], y))
        nxs.append(nx)
        us.append(u)
        xprev = nx
    return torch.stack(nxs, 1), torch.stack(us, 1)


def discounts(S, gamma, dtype):
    """utils.discounted_sum: g^t by repeated multiplication in the working precision."""
    d = np.ones(S, dtype=dtype)
    g = np.dtype(dtype).type(gamma)
    for t in range(1, S):
        d[t] = d[t - 1] * g
    return d


def loss_sum(ex, xseq, useq, next_xseq, gamma, teacher_forcing):
    """SUM over the batch of sum_dims sum_t g^t ((u - a)^2 + (next_x - next_s)^2) (calculate_loss times B)."""
    nx, u = forward(ex, xseq, teacher_forcing)
    d = torch.as_tensor(discounts(xseq.shape[1], gamma, np.float64 if xseq.dtype == torch.float64 else np.float32))
    d = d[None, :, None]
    return (d * (u - useq) ** 2).sum() + (d * (nx - next_xseq) ** 2).sum()


def loss_and_grad(flat, F, dims_x, dims_u, xseq, useq, next_xseq, gamma, teacher_forcing, dtype=np.float64):
    """numpy in -> (loss sum, gradient sum of the flat vector), both numpy in `dtype`."""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    p = torch.tensor(np.asarray(flat, dtype), dtype=tdt, requires_grad=True)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype), dtype=tdt)
    loss = loss_sum(unflatten(p, F, dims_x, dims_u), t(xseq), t(useq), t(next_xseq), gamma, teacher_forcing)
    loss.backward()
    return loss.detach().numpy(), p.grad.numpy()


def loss_only(flat, F, dims_x, dims_u, xseq, useq, next_xseq, gamma, teacher_forcing, dtype=np.float64):
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    t = lambda a: torch.as_tensor(np.asarray(a, dtype), dtype=tdt)
    with torch.no_grad():
        return float(loss_sum(unflatten(t(flat), F, dims_x, dims_u), t(xseq), t(useq), t(next_xseq), gamma,
                              teacher_forcing))


def make_windows(rng, B, S, n, m, scale=1.0):
    """Random windows: xseq, useq (in [-1, 1]), next_xseq = xseq shifted with a fresh last row."""
    traj = (scale * rng.standard_normal((B, S + 1, n))).astype(np.float32)
    useq = np.tanh(rng.standard_normal((B, S, m))).astype(np.float32)
    return np.ascontiguousarray(traj[:, :S]), useq, np.ascontiguousarray(traj[:, 1:])
