"""References of the path-integral solver (gmpc_mppi_solve / gmpc_mppi_vjp; TEST INFRASTRUCTURE).

* A NumPy restatement of the forward pass in fp32 or fp64, on cem_ref's sampler and costs.  Per problem and iteration:
  samples and costs as cem_ref forms them; w_s = exp(-(J_s - J_min) / lam) with J_min over the finite costs and w_s = 0
  for a NaN or infinite cost; new_mean = sum_s w_s u_s / sum_s w_s, both sums sequential in sample order;
  mean <- gamma mean + (1 - gamma) new_mean.  A problem without a finite cost keeps its mean.
* A torch transcription of the whole solve on torch_ref.objective, the normals of cem_ref as constants: its float64
  autograd is the arbiter of the gradient, the same transcription in float32 the fp32 reference.
"""

import numpy as np
import torch

import cem_ref
import gan_mpc_oracle as orc
import torch_ref as tr

DEFAULTS = dict(sampling_smoothing=0.0, evolution_smoothing=0.0, temperature=1.0, max_iter=5, num_samples=400, seed=0)


def weights(costs, lam, dtype=np.float64):
    """(B, N) costs -> (w (B, N) unnormalised, alive (B,)): exp(-(J - J_min) / lam) over the finite costs."""
    dtype = np.dtype(dtype).type
    c = np.asarray(costs, dtype)
    fin = np.isfinite(c)
    alive = fin.any(axis=1)
    mn = np.where(fin, c, np.inf).min(axis=1)
    with np.errstate(all="ignore"):
        w = np.where(fin, np.exp(-((c - mn[:, None]) / dtype(np.float32(lam)))), 0).astype(dtype)
    return w, alive


def update(samples, costs, mean, lam, gamma, dtype=np.float64):
    """One update -> (mean, normalised weights).  Sums sequential in sample order, in `dtype`."""
    dtype = np.dtype(dtype).type
    w, alive = weights(costs, lam, dtype)
    B, N = w.shape
    u = np.asarray(samples, dtype)
    sw = np.zeros(B, dtype)
    su = np.zeros(u.shape[:1] + u.shape[2:], dtype)
    for s in range(N):
        sw = sw + w[:, s]
        with np.errstate(all="ignore"):
            su = su + np.where(w[:, s, None, None] != 0, w[:, s, None, None] * u[:, s], dtype(0))
    sw = np.where(alive, sw, dtype(1))
    g = dtype(np.float32(gamma))
    g1 = dtype(np.float32(1.0) - np.float32(gamma))
    mean = mean.astype(dtype)
    new = g * mean + g1 * (su / sw[:, None, None])
    return np.where(alive[:, None, None], new, mean), w / sw[:, None]


def mppi(pb, dtype, lo, hi, kwargs=None, trace=None, init_std=0.5, iter_offset=0, U_init=None):
    """The whole solve on the problem pb (cast to dtype).  trace: a list that receives one dict per iteration (mean0:
    the mean before the update, samples, costs, weights, mean after).  -> dict(X, U, obj)."""
    dtype = np.dtype(dtype).type
    kw = dict(DEFAULTS)
    kw.update(kwargs or {})
    p = orc.cast_problem(pb, dtype)
    N = int(kw["num_samples"])
    mean = (p["U"] if U_init is None else np.asarray(U_init)).astype(dtype).copy()
    B, T, m = mean.shape
    lo_v = None if lo is None else np.broadcast_to(np.asarray(lo, dtype), (m,))
    hi_v = None if hi is None else np.broadcast_to(np.asarray(hi, dtype), (m,))
    std = np.broadcast_to(np.asarray(init_std, dtype), (B, T, m)).astype(dtype)
    for i in range(int(kw["max_iter"])):
        u = cem_ref.draw(mean, std, lo_v, hi_v, int(kw["seed"]), iter_offset + i, N, kw["sampling_smoothing"], dtype)
        c = cem_ref.sample_costs(p, u)
        mean0 = mean
        mean, wn = update(u, c, mean, kw["temperature"], kw["evolution_smoothing"], dtype)
        if trace is not None:
            trace.append(dict(mean0=mean0.copy(), samples=u, costs=c, weights=wn, mean=mean.copy()))
    X = orc.rollout(p["dyn"], mean, p["x0"])
    obj = np.sum(orc.evaluate(p["cmlp"], p["mpc_w"], p["goal"], X, mean), axis=1)
    return dict(X=X, U=mean, obj=obj)


def ess(wn):
    """Effective sample size 1 / sum w~^2 of normalised weights (B, N) -> (B,)."""
    return 1.0 / np.sum(np.asarray(wn, np.float64) ** 2, axis=1)


# ---- the torch transcription -------------------------------------------------------------------------------------
def leaves(pb, dtype=torch.float64):
    """The differentiable inputs of the solve as torch leaves: dict(dyn, cmlp, mpc_w, x0, goal, U)."""
    def leaf(a):
        return torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=True)
    return dict(dyn=[(leaf(W), leaf(b)) for W, b in pb["dyn"]], cmlp=[(leaf(W), leaf(b)) for W, b in pb["cmlp"]],
                mpc_w=leaf(pb["mpc_w"]), x0=leaf(pb["x0"]), goal=leaf(pb["goal"]), U=leaf(pb["U"]))


def _objectives(lv, b, us):
    """torch_ref.objective of every sample us (N, T, m) of problem b -> (N,)."""
    f = lambda u: tr.objective(lv["dyn"], lv["cmlp"], lv["mpc_w"], lv["goal"][b], u, lv["x0"][b])
    return torch.func.vmap(f)(us)


def torch_mppi(lv, lo, hi, kwargs=None, init_std=0.5, iter_offset=0, pre=None):
    """The whole solve on the leaves lv, differentiable: -> (X (B, T+1, n), U (B, T, m), obj (B,)).  The normals are
    constants drawn by cem_ref in the leaves' precision.  pre: a list that receives, per problem and iteration, the
    pre-clamp samples (N, T, m) as an array."""
    kw = dict(DEFAULTS)
    kw.update(kwargs or {})
    dtype = lv["U"].dtype
    npd = np.float64 if dtype == torch.float64 else np.float32
    B, T, m = lv["U"].shape
    N, lam = int(kw["num_samples"]), float(np.float32(kw["temperature"]))
    gamma = float(np.float32(kw["evolution_smoothing"]))
    g1 = float(np.float32(1.0) - np.float32(kw["evolution_smoothing"]))
    std = torch.as_tensor(np.broadcast_to(np.asarray(init_std, npd), (B, T, m)).copy(), dtype=dtype)
    means = []
    for b in range(B):
        mean = lv["U"][b]
        for i in range(int(kw["max_iter"])):
            z = cem_ref.smooth(cem_ref.normals(int(kw["seed"]), iter_offset + i, b, np.arange(N), T * m,
                                               npd).reshape(N, T, m), kw["sampling_smoothing"], npd)
            u = std[b] * torch.as_tensor(z, dtype=dtype) + mean
            if pre is not None:
                pre.append(u.detach().numpy().copy())
            if lo is not None or hi is not None:
                u = torch.clamp(u, min=lo, max=hi)
            J = _objectives(lv, b, u)
            fin = torch.isfinite(J)
            if not bool(fin.any()):
                continue
            Jm = torch.where(fin, J, torch.full_like(J, float("inf"))).min().detach()
            w = torch.where(fin, torch.exp(-(torch.where(fin, J, Jm) - Jm) / lam), torch.zeros_like(J))
            new = (w[:, None, None] * u).sum(0) / w.sum()
            mean = gamma * mean + g1 * new
        means.append(mean)
    U = torch.stack(means)
    X = torch.stack([tr.rollout(lv["dyn"], U[b], lv["x0"][b]) for b in range(B)])
    obj = torch.stack([tr.objective(lv["dyn"], lv["cmlp"], lv["mpc_w"], lv["goal"][b], U[b], lv["x0"][b])
                       for b in range(B)])
    return X, U, obj


def cotangent_loss(X, U, obj, gX, gU, gobj):
    """<gX, X> + <gU, U> + <gobj, obj>: the scalar whose gradient is the VJP under the cotangents."""
    return (X * torch.as_tensor(gX, dtype=X.dtype)).sum() + (U * torch.as_tensor(gU, dtype=U.dtype)).sum() + \
        (obj * torch.as_tensor(gobj, dtype=obj.dtype)).sum()


def torch_grads(lv, L):
    """The gradient of the scalar L w.r.t. the leaves by autograd -> dict(x0, U, goal, theta, dyn) of arrays, theta and
    dyn in grad_theta_sum's / grad_dyn_sum's layouts (mpc_w, then each MLP as W_0 | b_0 | W_1 | ...)."""
    flat = [lv["x0"], lv["U"], lv["goal"], lv["mpc_w"]] + [a for Wb in lv["cmlp"] for a in Wb] + \
        [a for Wb in lv["dyn"] for a in Wb]
    g = [np.zeros(tuple(a.shape)) if x is None else x.numpy() for a, x in
         zip(flat, torch.autograd.grad(L, flat, allow_unused=True))]
    nc = 2 * len(lv["cmlp"])
    return dict(x0=g[0], U=g[1], goal=g[2], theta=np.concatenate([a.ravel() for a in g[3:4 + nc]]),
                dyn=np.concatenate([a.ravel() for a in g[4 + nc:]]))
