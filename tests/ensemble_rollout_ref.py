"""NumPy restatement of the ensemble rollout (gmpc_ensemble_rollout; TEST INFRASTRUCTURE): per
member the oracle's own rollout, per-step costs and objective on dict(pb, dyn=member), in the dtype of pb; and the
moments over the members' planes exactly as the library forms them,

  mean = (((x_0 + x_1) + x_2) + ... + x_{P-1}) / P
  var  = (((0 + d_0 d_0) + d_1 d_1) + ... + d_{P-1} d_{P-1}) / P,   d_p = x_p - mean

every operation one operation of the dtype, in ascending p (the population variance)."""

import numpy as np

import gan_mpc_oracle as orc
import sampled_ensemble_ref as er


def rollout(pb, members, S=None, costs=True):
    """dict(X (P, B, S+1, n), costs (P, B, T+1), obj (P, B)) of pb's plans under `members` (lists of (W, b) layers), in
    pb's dtype; S: the steps rolled (default T, the only length with costs)."""
    T = pb["U"].shape[1]
    S = T if S is None else S
    U = pb["U"][:, :S]
    out = dict(X=[], costs=[], obj=[])
    for layers in er.cast_members(members, pb["x0"].dtype):
        X = orc.rollout(layers, U, pb["x0"])
        out["X"].append(X)
        if costs and S == T:
            out["costs"].append(orc.evaluate(pb["cmlp"], pb["mpc_w"], pb["goal"], X, U))
            out["obj"].append(orc.objective(layers, pb["cmlp"], pb["mpc_w"], pb["goal"], U, pb["x0"]))
    return {k: np.stack(v) for k, v in out.items() if v}


def moments(X, dtype=None):
    """(mean, var) over axis 0 of the planes X (P, ...), the library's rule in `dtype` (default: X's)."""
    dt = np.dtype(X.dtype if dtype is None else dtype).type
    X = np.asarray(X, dt)
    fP = dt(X.shape[0])
    with np.errstate(all="ignore"):
        s = X[0].copy()
        for p in range(1, X.shape[0]):
            s = (s + X[p]).astype(dt)
        mean = (s / fP).astype(dt)
        ss = np.zeros_like(mean)
        for p in range(X.shape[0]):
            d = (X[p] - mean).astype(dt)
            ss = (ss + (d * d).astype(dt)).astype(dt)
        return mean, (ss / fP).astype(dt)
