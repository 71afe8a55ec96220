"""NumPy restatement of the closed-loop ensemble rollout (gmpc_ensemble_rollout_feedback; TEST
INFRASTRUCTURE), in the dtype of its inputs: per member p and problem b, from x_0 = x0[b],

  du_j    = sum_c K[b][t][j][c] * (x_t[c] - X_ref[b][t][c])        c ascending, from 0
  du_j   += alpha * k[b][t][j]                                     only if k is given
  u_t     = clip(U_ref[b][t] + du, lo, hi)                         only if bounds are given
  x_{t+1} = x_t + MLP_p([x_t; u_t])

and the oracle's per-step costs (orc.evaluate) on the APPLIED controls.  gains() gives the tests their feedback law:
trajax's time-varying LQR gains, in fp64, at the fp32 nominal rollout of the problem's own controls."""

import numpy as np

import gan_mpc_oracle as orc
import sampled_ensemble_ref as er


def rollout(pb, members, X_ref, U_ref, K, x0=None, k=None, alpha=1.0, lo=None, hi=None, costs=True):
    """dict(X (P, B, S+1, n), U (P, B, S, m), costs (P, B, T+1), obj (P, B)) under `members` (lists of (W, b) layers),
    in the dtype of X_ref; S = U_ref.shape[1]; costs and obj only with S == T (pb["goal"] has T + 1 rows)."""
    dt = X_ref.dtype.type
    B, S, m = U_ref.shape
    n = X_ref.shape[-1]
    T = pb["goal"].shape[1] - 1
    x0 = X_ref[:, 0] if x0 is None else np.asarray(x0, dt)
    K, U_ref = np.asarray(K, dt), np.asarray(U_ref, dt)
    out = dict(X=[], U=[], costs=[], obj=[])
    cmlp = [(W.astype(dt), b.astype(dt)) for W, b in pb["cmlp"]]
    with np.errstate(invalid="ignore", over="ignore"):
        for layers in er.cast_members(members, dt):
            X = np.empty((B, S + 1, n), dt)
            U = np.empty((B, S, m), dt)
            X[:, 0] = x0
            for t in range(S):
                d = (X[:, t] - X_ref[:, t]).astype(dt)
                du = np.zeros((B, m), dt)
                for c in range(n):
                    du = (du + (K[:, t, :, c] * d[:, c:c + 1]).astype(dt)).astype(dt)
                if k is not None:
                    du = (du + (dt(alpha) * np.asarray(k, dt)[:, t]).astype(dt)).astype(dt)
                u = (U_ref[:, t] + du).astype(dt)
                if lo is not None:
                    u = np.clip(u, dt(lo), dt(hi)).astype(dt)       # (a NaN stays one)
                U[:, t] = u
                X[:, t + 1], _ = orc.dynamics_predict(layers, X[:, t], u)
            out["X"].append(X)
            out["U"].append(U)
            if costs and S == T:
                c = orc.evaluate(cmlp, np.asarray(pb["mpc_w"], dt), np.asarray(pb["goal"], dt), X, U)
                out["costs"].append(c)
                out["obj"].append(np.sum(c, axis=1))
    return {key: np.stack(v) for key, v in out.items() if v}


def gains_at(pb):
    """(X_ref fp32 (B, T+1, n), K fp32 (B, T, m, n), k fp32 (B, T, m), K fp64, k fp64): X_ref the fp32 rollout of
    pb["U"] from pb["x0"] under pb["dyn"]; the gains orc.tvlqr(*orc.get_lqr_params(...)) in fp64 at that trajectory."""
    X = orc.rollout(pb["dyn"], pb["U"], pb["x0"])
    pb64 = orc.cast_problem(pb, np.float64)
    with np.errstate(all="ignore"):
        K, k, _, _ = orc.tvlqr(*orc.get_lqr_params(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"],
                                                   X.astype(np.float64), pb64["U"]))
    assert np.isfinite(K).all() and np.isfinite(k).all()
    return X, K.astype(np.float32), k.astype(np.float32), K, k


def perturbed_x0(pb, scale, seed=7):
    """pb["x0"] + scale * N(0, 1), fp32."""
    rng = np.random.default_rng(seed)
    return (pb["x0"] + np.float32(scale) * rng.standard_normal(pb["x0"].shape)).astype(np.float32)


def cast_inputs(dtype, **arrays):
    """The named arrays (None stays None) in `dtype`."""
    return {key: (None if a is None else np.asarray(a, dtype)) for key, a in arrays.items()}
