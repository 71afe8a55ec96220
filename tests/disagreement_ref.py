"""NumPy restatement of the one-step ensemble disagreement (gmpc_set_sampled_disagreement / gmpc_ensemble_disagreement,
DESIGN.md section 28; TEST INFRASTRUCTURE), in fp32 or fp64, on cem_ref and the oracle.  For a row with controls
u_0 .. u_{T-1} of problem b:

  x_t      the rollout under the problem's own (nominal) dynamics, x_{t+1} = x_t + o^0_t
  o^0_t    MLP_0([x_t; u_t]), the nominal network's output, bias included, before the residual add
  o^p_t    MLP_p([x_t; u_t]), member p's output on the same input
  d[p][t]  sum_j (o^p_t[j] - o^0_t[j])^2
  D[p]     sum_t d[p][t], sequential in t, in the run's dtype
  J_p      J + penalty * D[p], J the nominal cost (cem_ref.sample_costs), the product rounded before it is added

and the planes J_0 .. J_{P-1} go through ensemble_modes_ref.aggregate.  The bf16 restatement runs both passes on
sampled_bf16_ref's rounded operands; the difference, the sums and J stay fp32."""

import contextlib

import numpy as np

import cem_ref
import ensemble_modes_ref as mr
import gan_mpc_oracle as orc
import sampled_bf16_ref as sr
import sampled_ensemble_ref as er

_plain_sample_costs = cem_ref.sample_costs


def _seq_sum(d, dt):
    """(..., S) -> (...): the sum along the last axis, sequential, every partial sum rounded to dt."""
    s = np.zeros(d.shape[:-1], dt)
    for t in range(d.shape[-1]):
        s = (s + d[..., t]).astype(dt)
    return s


def plan(nominal, members, x0, U):
    """The disagreement along given plans: nominal, members: layer lists; x0 (R, n), U (R, S, m), in the dtype of x0.
    -> dict(X (R, S+1, n) the nominal rollout, d (P, R, S), D (P, R), o0 (R, S, n), op (P, R, S, n))."""
    dt = x0.dtype.type
    nominal = er.cast_members([nominal], dt)[0]
    members = er.cast_members(members, dt)
    R, S, _ = U.shape
    n = x0.shape[-1]
    U = U.astype(dt)
    X = np.empty((R, S + 1, n), dt)
    X[:, 0] = x0
    o0 = np.empty((R, S, n), dt)
    op = np.empty((len(members), R, S, n), dt)
    with np.errstate(all="ignore"):
        for t in range(S):
            q = np.concatenate([X[:, t], U[:, t]], axis=-1)
            o0[:, t] = orc.mlp_forward(nominal, q)[0]
            for p, layers in enumerate(members):
                op[p, :, t] = orc.mlp_forward(layers, q)[0]
            X[:, t + 1] = o0[:, t] + X[:, t]
        diff = (op - o0[None]).astype(dt)
        d = np.sum(diff * diff, axis=-1).astype(dt)
    return dict(X=X, d=d, D=_seq_sum(d, dt), o0=o0, op=op)


def plan_bf16(nominal, members, x0, U):
    """plan() in the bf16 mode of the sampled rollouts: both passes on sampled_bf16_ref's layers, everything else fp32."""
    f32 = lambda layers: [(sr.round_bf16(np.asarray(W, np.float32)), np.asarray(b, np.float32)) for W, b in layers]
    nominal, members = f32(nominal), [f32(layers) for layers in members]
    R, S, _ = U.shape
    n = x0.shape[-1]
    U = np.asarray(U, np.float32)
    X = np.empty((R, S + 1, n), np.float32)
    X[:, 0] = x0
    d = np.empty((len(members), R, S), np.float32)
    with np.errstate(all="ignore"):
        for t in range(S):
            q = np.concatenate([X[:, t], U[:, t]], axis=-1)
            o0 = sr._mlp(nominal, q, sr.matmul_f64, None)
            for p, layers in enumerate(members):
                diff = sr._mlp(layers, q, sr.matmul_f64, None) - o0
                d[p, :, t] = np.sum(diff * diff, axis=-1)
            X[:, t + 1] = o0 + X[:, t]
    return dict(X=X, d=d, D=_seq_sum(d, np.float32))


def sample_D(pb, members, samples, bf16=False):
    """(P, B, N): D of every sample, in the dtype of pb (bf16: the fp32 problem, bf16-mode passes)."""
    B, N, T, m = samples.shape
    x0 = np.repeat(pb["x0"], N, axis=0)
    U = samples.reshape(B * N, T, m).astype(x0.dtype)
    out = (plan_bf16 if bf16 else plan)(pb["dyn"], members, x0, U)
    return out["D"].reshape(len(members), B, N)


def penalised(J, penalty, D):
    """J + penalty * D in J's dtype, the product rounded before it is added; penalty through fp32, as the library's."""
    dt = J.dtype.type
    with np.errstate(all="ignore"):
        return (J + (dt(np.float32(penalty)) * D.astype(dt)).astype(dt)).astype(dt)


def plane_costs(pb, members, samples, penalty, bf16=False):
    """[P] arrays (B, N): J + penalty D[p]."""
    J = sr.sample_costs(pb, samples) if bf16 else _plain_sample_costs(pb, samples)
    D = sample_D(pb, members, samples, bf16)
    return [penalised(J, penalty, D[p]) for p in range(len(members))]


def sample_costs(pb, members, samples, penalty, aggregate="mean", bf16=False):
    return mr.aggregate(plane_costs(pb, members, samples, penalty, bf16), aggregate)


@contextlib.contextmanager
def disagreement(members, penalty, aggregate="mean"):
    """While open, cem_ref's loop costs its samples with the disagreement penalty."""
    saved = cem_ref.sample_costs
    cem_ref.sample_costs = lambda p, u: sample_costs(p, members, u, penalty, aggregate)
    try:
        yield
    finally:
        cem_ref.sample_costs = saved


def cem(pb, members, penalty, aggregate, dtype, lo, hi, kwargs=None, **more):
    """cem_ref.cem with the samples costed under the penalty."""
    with disagreement(members, penalty, aggregate):
        return cem_ref.cem(pb, dtype, lo, hi, kwargs, **more)
