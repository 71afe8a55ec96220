"""Torch restatement of the expert model's ROLLOUT schedule (TEST INFRASTRUCTURE): oracle
expert_goal_states_init_actions (reference expert/expert_model.py:60-91, policy/eval.py:87-107) written over the flat
vector of params.pack_expert, so that autograd gives the VJP in the layout gmpc_expert_vjp writes: steps
st = 0 .. hist+T-1, the input of step st is history[st] for st <= hist and the previous step's next_x after that,
goal[st-hist+1] = next_x_st and init_U[st-hist] = u_st for st >= hist, goal[0] = history[hist].  Runs in fp32 or fp64
on the CPU."""

import numpy as np
import torch

import expert_fit_ref as R


def rollout(ex, history, T):
    """ex: expert_fit_ref.unflatten's dict; history (B, hist+1, n) -> goal (B, T+1, n), init_U (B, T, m)."""
    B, h1, _ = history.shape
    hist = h1 - 1
    lstm = ex.get("lstm")
    if lstm is not None:
        F = lstm["Wh"].shape[0]
        c = history.new_zeros(B, F)
        h = history.new_zeros(B, F)
    goal, us = [history[:, hist]], []
    x = history[:, 0]
    for st in range(hist + T):
        if st <= hist:
            x = history[:, st]
        if lstm is not None:
            z = x @ lstm["Wx"] + h @ lstm["Wh"] + lstm["b"]
            i, f, g, o = (z[:, k * F:(k + 1) * F] for k in range(4))
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            y = h
        else:
            W0, b0 = ex["first"]
            y = torch.relu(x @ W0 + b0)
        nx = R._mlp(ex["head_x"], y) + x
        u = torch.tanh(R._mlp(ex["head_u"], y))
        if st >= hist:
            goal.append(nx)
            us.append(u)
        x = nx
    return torch.stack(goal, 1), torch.stack(us, 1)


def _tdt(dtype):
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def flat_of_tree(ex, dtype=np.float64):
    """The flat vector in params.pack_expert's order built from the oracle dict WITHOUT a detour through fp32
    (pack_expert rounds to fp32)."""
    parts = []
    if ex.get("lstm") is not None:
        parts += [ex["lstm"]["Wx"], ex["lstm"]["Wh"], ex["lstm"]["b"]]
    else:
        parts += list(ex["first"])
    for key in ("head_x", "head_u"):
        for W, b in ex[key]:
            parts += [W, b]
    return np.concatenate([np.asarray(p, dtype).reshape(-1) for p in parts])


def forward(flat, F, dims_x, dims_u, history, T, dtype=np.float64):
    """numpy in -> (goal, init_U) numpy in `dtype`."""
    tdt = _tdt(dtype)
    t = lambda a: torch.as_tensor(np.array(a, dtype), dtype=tdt)  # noqa: E731
    with torch.no_grad():
        goal, U = rollout(R.unflatten(t(flat), F, dims_x, dims_u), t(history), T)
    return goal.numpy(), U.numpy()


def vjp(flat, F, dims_x, dims_u, history, T, g_goal=None, g_U=None, dtype=np.float64):
    """numpy in -> (grad_expert_sum [flat.size], grad_history (B, hist+1, n)) for the cotangents g_goal (B, T+1, n),
    g_U (B, T, m) (None = zero), numpy in `dtype`."""
    tdt = _tdt(dtype)
    t = lambda a: torch.as_tensor(np.array(a, dtype), dtype=tdt)  # noqa: E731
    p = t(flat).clone().requires_grad_(True)
    hx = t(history).clone().requires_grad_(True)
    goal, U = rollout(R.unflatten(p, F, dims_x, dims_u), hx, T)
    s = goal.new_zeros(())
    if g_goal is not None:
        s = s + (goal * t(g_goal)).sum()
    if g_U is not None:
        s = s + (U * t(g_U)).sum()
    s.backward()
    return p.grad.numpy(), hx.grad.numpy()


def near_kink(flat, F, dims_x, dims_u, history, T, thresh=3e-6):
    """(B,) bool: in the fp64 forward some relu pre-activation of the window (MLP first layer, head hidden layers, any
    step whose derivative the VJP uses) is within `thresh` of the kink, relative to that layer's largest
    pre-activation of the window and step (gpu_util.near_kink's rule)."""
    t = lambda a: torch.as_tensor(np.array(a, np.float64))  # noqa: E731
    ex = R.unflatten(t(flat), F, dims_x, dims_u)
    history = t(history)
    B, h1, _ = history.shape
    hist = h1 - 1
    bad = np.zeros(B, bool)

    def mark(z):
        z = z.numpy()
        bad[:] |= (np.abs(z) < thresh * np.abs(z).max(axis=1, keepdims=True)).any(axis=1)

    lstm = ex.get("lstm")
    if lstm is not None:
        c = history.new_zeros(B, F)
        h = history.new_zeros(B, F)
    x = history[:, 0]
    with torch.no_grad():
        for st in range(hist + T):
            if st <= hist:
                x = history[:, st]
            if lstm is not None:
                z = x @ lstm["Wx"] + h @ lstm["Wh"] + lstm["b"]
                i, f, g, o = (z[:, k * F:(k + 1) * F] for k in range(4))
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                y = h
            else:
                W0, b0 = ex["first"]
                z0 = x @ W0 + b0
                if st >= hist:
                    mark(z0)
                y = torch.relu(z0)
            outs = []
            for layers in (ex["head_x"], ex["head_u"]):
                a = y
                for l, (W, b) in enumerate(layers):
                    a = a @ W + b
                    if l < len(layers) - 1:
                        if st >= hist:
                            mark(a)
                        a = torch.relu(a)
                outs.append(a)
            x = outs[0] + x
    return bad
