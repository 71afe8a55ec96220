"""NumPy restatement of the one-step disagreement's VJP (gmpc_ensemble_disagreement_vjp; TEST
INFRASTRUCTURE), in the dtype of X, on disagreement_ref.plan's quantities and the oracle's MLP forward.  At the given
nominal rollout X, with z_t = [x_t; u_t], o^0_t = MLP_0(z_t), o^p_t = MLP_p(z_t) and the weights w = gd + gD:

  e^p_t = o^p_t - o^0_t,  c^p_t = 2 w[p][b][t] e^p_t
  q^p_t = (dMLP_p/dz)^T c^p_t                        members[p] = sum_{b,t} (dMLP_p/dtheta)^T c^p_t
  c^N_t = -(((c^0_t + c^1_t) + ...) + c^{P-1}_t)      q^N_t = (dMLP_0/dz)^T c^N_t
  r_t   = ((((q^0_t + q^1_t) + ...) + q^{P-1}_t) + q^N_t) = [rx_t; ru_t]
  lambda_T = 0, lambda_t = rx_t + lambda_{t+1} + (dMLP_0/dx)^T lambda_{t+1}
  U_t = ru_t + (dMLP_0/du)^T lambda_{t+1},  x0 = lambda_0
  nominal = sum_{b,t} (dMLP_0/dtheta)^T (c^N_t + lambda_{t+1})

A relu unit is active iff its pre-activation is > 0.  Every sum over p is sequential in ascending p, one addition of
the dtype each."""

import numpy as np

import gan_mpc_oracle as orc
import sampled_ensemble_ref as er

KEYS = ("x0", "U", "nominal", "members")


def weights(gd, gD, dt):
    """w (P, B, T) = gd + gD in dt (one addition; with one given, that value)."""
    if gd is None:
        return np.asarray(gD, dt)[:, :, None]
    if gD is None:
        return np.asarray(gd, dt)
    return (np.asarray(gd, dt) + np.asarray(gD, dt)[:, :, None]).astype(dt)


def mlp_back(layers, q, c):
    """The backward pass of the relu MLP at the input rows q (R, K) under the output cotangents c (R, n) ->
    (dq (R, K), the flat gradient W_0 | b_0 | W_1 | b_1 | ... summed over the rows)."""
    _, zs = orc.mlp_forward(layers, q)
    acts = [q] + [np.maximum(z, 0) for z in zs]
    grads = [None] * len(layers)
    e = c
    for l in range(len(layers) - 1, -1, -1):
        W = layers[l][0]
        grads[l] = (acts[l].T @ e, e.sum(0))
        e = e @ W.T
        if l > 0:
            e = e * (zs[l - 1] > 0)
    return e, np.concatenate([np.concatenate([gW.reshape(-1), gb]) for gW, gb in grads])


def reference(nominal, members, X, U, gd=None, gD=None):
    """dict(x0 (B, n), U (B, T, m), nominal [dyn count], members (P, dyn count)) in X's dtype, and the per-term parts:
    q (P, B, T, n + m), qN (B, T, n + m), chain (B, T, n + m) = (dMLP_0/dz)^T lambda_{t+1}, lam (B, T + 1, n), and
    parts = dict(x0, U): the summed absolute values of the terms added into each entry, for the conditioning rule."""
    dt = X.dtype.type
    assert gd is not None or gD is not None
    nominal = er.cast_members([nominal], dt)[0]
    members = er.cast_members(members, dt)
    P = len(members)
    B, T, m = U.shape
    n = X.shape[-1]
    U = np.asarray(U, dt)
    w = np.broadcast_to(weights(gd, gD, dt), (P, B, T))
    z = np.concatenate([X[:, :T], U], -1).reshape(B * T, n + m)
    with np.errstate(all="ignore"):
        o0 = orc.mlp_forward(nominal, z)[0]
        q, gm, cs = [], [], []
        for p, layers in enumerate(members):
            e = (orc.mlp_forward(layers, z)[0] - o0).astype(dt)
            c = ((dt(2) * w[p].reshape(-1, 1)).astype(dt) * e).astype(dt)
            dq, g = mlp_back(layers, z, c)
            cs.append(c)
            q.append(dq.astype(dt))
            gm.append(g.astype(dt))
        s = cs[0]
        for c in cs[1:]:
            s = (s + c).astype(dt)
        cN = -s
        qN, _ = mlp_back(nominal, z, cN)
        qN = qN.astype(dt)
        r = q[0]
        for dq in q[1:]:
            r = (r + dq).astype(dt)
        r = (r + qN).astype(dt).reshape(B, T, n + m)
        # ---- the chain through x_{t+1} = x_t + MLP_0(z_t)
        lam = np.zeros((B, T + 1, n), dt)
        chain = np.zeros((B, T, n + m), dt)
        for t in range(T - 1, -1, -1):
            zt = z.reshape(B, T, n + m)[:, t]
            chain[:, t] = mlp_back(nominal, zt, lam[:, t + 1])[0]
            lam[:, t] = ((r[:, t, :n] + lam[:, t + 1]).astype(dt) + chain[:, t, :n]).astype(dt)
        gU = (r[:, :, n:] + chain[:, :, n:]).astype(dt)
        _, gnom = mlp_back(nominal, z, (cN.reshape(B, T, n) + lam[:, 1:]).astype(dt).reshape(B * T, n))
    q = np.stack(q).reshape(P, B, T, n + m)
    qN = qN.reshape(B, T, n + m)
    # what is summed into an entry of x0 / U: the local terms of the entry's own step and, for x0, every later step's
    # contribution as the chain carries it; the conditioning rule takes the terms of the last additions
    ax = np.abs(q[:, :, 0, :n]).sum(0) + np.abs(qN[:, 0, :n]) + np.abs(lam[:, 1]) + np.abs(chain[:, 0, :n])
    au = np.abs(q[..., n:]).sum(0) + np.abs(qN[..., n:]) + np.abs(chain[..., n:])
    return dict(x0=lam[:, 0].copy(), U=gU, nominal=gnom.astype(dt), members=np.stack(gm), q=q, qN=qN, chain=chain,
                lam=lam, parts=dict(x0=ax, U=au))


def kappa(ref):
    """The largest (sum_p |q^p| + |q^N| + |chain|) / |result| over the entries of x0 and U, the denominator floored at
    1e-6 of the largest entry as gpu_util.el_err floors it."""
    worst = 0.0
    for k in ("x0", "U"):
        s = np.abs(ref[k])
        if s.max() == 0:
            continue
        worst = max(worst, float((ref["parts"][k] / np.maximum(s, 1e-6 * s.max())).max()))
    return worst
