"""NumPy restatement of the ensemble rollout's VJP (gmpc_ensemble_rollout_vjp; TEST
INFRASTRUCTURE): test_rollout_vjp_host.reference -- the per-step form of section 14, shown there to equal torch autograd
and central differences -- looped over the members, each on dict(pb, dyn=member) at (X[p], U, goal) under (gX[p],
gc[p]), in X's dtype; then the sums as the library defines them,

  x0, U, goal = ((g^0 + g^1) + ...) + g^{P-1}     one addition of the dtype per member, ascending p, from member 0's value
  theta       = the members' batch sums, added in ascending p
  members     = one row per member: its batch sum in gmpc_set_params' dyn layout

and the risk aggregates of BaseMPC.plan_risk (DESIGN.md section 26's formulas) with their derivatives w.r.t. the
members' objectives."""

import numpy as np

import sampled_ensemble_ref as er
from test_rollout_vjp_host import reference as member_reference

KEYS = ("x0", "U", "goal", "theta", "members")


def reference(pb, members, X, U, goal, gX=None, gc=None):
    """dict(x0 (B, n), U (B, T, m), goal (B, T+1, n), theta [3 + cost count], members (P, dyn count)) in X's dtype; per:
    the members' own dicts (test_rollout_vjp_host.reference's)."""
    dt = X.dtype
    per = []
    for p, layers in enumerate(er.cast_members(members, dt)):
        per.append(member_reference(dict(pb, dyn=layers), X[p], np.asarray(U, dt), np.asarray(goal, dt),
                                    None if gX is None else gX[p], None if gc is None else gc[p]))
    out = {}
    with np.errstate(all="ignore"):
        for k in ("x0", "U", "goal", "theta"):
            s = per[0][k].astype(dt)
            for q in per[1:]:
                s = (s + q[k]).astype(dt)
            out[k] = s
    out["members"] = np.stack([q["dyn"] for q in per]).astype(dt)
    out["per"] = per
    return out


def risk(J, aggregate="mean", risk=0.0):
    """(R (B,), dR/dJ (P, B)) of the members' objectives J (P, B): plan_risk's definition, in J's dtype."""
    P = J.shape[0]
    mean = J.sum(0) / P
    if aggregate == "mean":
        return mean, np.full_like(J, 1.0 / P)
    if aggregate == "mean_std":
        d = J - mean
        sd = np.sqrt((d * d).sum(0) / P)
        return mean + risk * sd, 1.0 / P + risk * d / (P * np.where(sd > 0, sd, 1.0))
    assert aggregate == "max", aggregate
    arg = J.argmax(0)                          # the first member that attains the maximum
    w = np.zeros_like(J)
    w[arg, np.arange(J.shape[1])] = 1.0
    return J.max(0), w
