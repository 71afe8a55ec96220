"""NumPy restatement of the sampling solvers' ensemble modes (gmpc_set_sampled_ensemble_mode; TEST
INFRASTRUCTURE).  A mode is a dict of Engine.set_sampled_ensemble_mode's keywords.  Q cost planes per row:

  FIXED  plane q is member q (sampled_ensemble_ref.member_costs), Q = P
  TS1    plane q is particle q, Q = particles: at step t of iteration `it` it runs under member
         schedule(seed, it, Q, T, P)[q, t] = (philox(counter (t, q, 0xFFFFFFFF, it), key seed)[0] * P) >> 32
         -- one sequence per particle, shared by every row and problem --, through orc.dynamics_predict per step and
         orc.evaluate on the states

and aggregate(): the library's rule in the run's dtype, every operation rounded once, in ascending q,

  mean      (((J_0 + J_1) + ...) + J_{Q-1}) * (1 / Q)
  mean_std  mean + risk * sqrt(ss * (1 / Q)), ss = (((0 + d_0 d_0) + d_1 d_1) + ...), d_q = J_q - mean
  max       w = J_0; w = J_q where J_q > w or J_q is a NaN

plugged into cem_ref's loop as sampled_ensemble_ref does.  X and obj of cem()'s result stay those of pb's own dynamics."""

import contextlib

import numpy as np

import cem_ref
import gan_mpc_oracle as orc
import sampled_ensemble_ref as er

DEFAULT = dict(aggregate="mean", risk=0.0, propagation="fixed", particles=None)
STREAM = 0xFFFFFFFF            # counter word 2 of the schedule: no problem index reaches it


def full(mode):
    out = dict(DEFAULT)
    out.update(mode or {})
    return out


def aggregate(planes, kind="mean", risk=0.0, dtype=None):
    """The planes' costs, a sequence of Q equal-shaped arrays, -> the row costs in `dtype` (default: theirs)."""
    dt = np.dtype(planes[0].dtype if dtype is None else dtype).type
    J = [np.asarray(c, dt) for c in planes]
    with np.errstate(all="ignore"):
        if kind == "max":
            w = J[0]
            for c in J[1:]:
                w = np.where((c > w) | np.isnan(c), c, w)
            return w.astype(dt)
        inv = dt(1.0) / dt(len(J))
        s = J[0]
        for c in J[1:]:
            s = (s + c).astype(dt)
        mean = (s * inv).astype(dt)
        if kind == "mean":
            return mean
        assert kind == "mean_std", kind
        ss = np.zeros_like(mean)
        for c in J:
            d = (c - mean).astype(dt)
            ss = (ss + (d * d).astype(dt)).astype(dt)
        sd = np.sqrt((ss * inv).astype(dt)).astype(dt)
        return (mean + (dt(np.float32(risk)) * sd).astype(dt)).astype(dt)


def schedule(seed, it, Q, T, P):
    """(Q, T) member indices of the particles at iteration `it`."""
    q, t = np.arange(Q)[:, None], np.arange(T)[None, :]
    r = cem_ref.philox((t, q, STREAM, it), (seed & cem_ref.MASK, (seed >> 32) & cem_ref.MASK))[0]
    return ((r.astype(np.uint64) * np.uint64(P)) >> np.uint64(32)).astype(np.int64)


def particle_costs(pb, members, samples, sched):
    """(B, N): the samples rolled out under member sched[t] at step t, in the dtype of pb."""
    B, N, T, m = samples.shape
    dt = pb["x0"].dtype
    layers = er.cast_members(members, dt)
    U = samples.reshape(B * N, T, m).astype(dt)
    x0 = np.repeat(pb["x0"], N, axis=0)
    goal = np.repeat(pb["goal"], N, axis=0)
    X = np.empty((B * N, T + 1, x0.shape[-1]), dt)
    X[:, 0] = x0
    with np.errstate(all="ignore"):
        for t in range(T):
            X[:, t + 1], _ = orc.dynamics_predict(layers[int(sched[t])], X[:, t], U[:, t])
        c = np.sum(orc.evaluate(pb["cmlp"], pb["mpc_w"], goal, X, U), axis=1)
    return c.reshape(B, N)


def plane_costs(pb, members, samples, mode=None, seed=0, it=0):
    """[Q] arrays (B, N): the cost planes of the mode."""
    mode = full(mode)
    if mode["propagation"] == "fixed":
        return er.member_costs(pb, members, samples)
    sched = schedule(seed, it, mode["particles"], samples.shape[2], len(members))
    return [particle_costs(pb, members, samples, sched[q]) for q in range(mode["particles"])]


def sample_costs(pb, members, samples, mode=None, seed=0, it=0):
    mode = full(mode)
    return aggregate(plane_costs(pb, members, samples, mode, seed, it), mode["aggregate"], mode["risk"])


def particle_costs_bf16(pb, members, samples, sched):
    """particle_costs in the bf16 mode of the sampled rollouts, on sampled_bf16_ref's layers: fp32 (B, N)."""
    import sampled_bf16_ref as sr
    B, N, T, m = samples.shape
    f32 = lambda layers: [(np.asarray(W, np.float32), np.asarray(b, np.float32)) for W, b in layers]
    dyn = [[(sr.round_bf16(W), b) for W, b in f32(layers)] for layers in members]
    cmlp = [(sr.round_bf16(W), b) for W, b in f32(pb["cmlp"])]
    U = np.asarray(samples, np.float32).reshape(B * N, T, m)
    x0 = np.repeat(np.asarray(pb["x0"], np.float32), N, axis=0)
    goal = np.repeat(np.asarray(pb["goal"], np.float32), N, axis=0)
    X = np.empty((B * N, T + 1, x0.shape[-1]), np.float32)
    X[:, 0] = x0
    with np.errstate(all="ignore"):
        for t in range(T):
            X[:, t + 1] = sr._mlp(dyn[int(sched[t])], np.concatenate([X[:, t], U[:, t]], axis=-1), sr.matmul_f64,
                                  None) + X[:, t]
        w = orc.sigmoid(np.asarray(pb["mpc_w"], np.float32))
        c = np.empty((B * N, T + 1), np.float32)
        c[:, :T] = orc.stage_cost(X[:, :T], U, goal[:, :T], w)
        y = sr._mlp(cmlp, X[:, T], sr.matmul_f64, None)
        c[:, T] = w[2] * np.sum(y * y, -1)
        return np.sum(c, axis=1).reshape(B, N)


@contextlib.contextmanager
def ensemble(members, mode, seed, iter_offset=0):
    """While open, cem_ref's loop costs its samples on the ensemble under the mode; the k-th costing inside is
    iteration iter_offset + k of the schedule."""
    calls = [0]

    def costs(p, u):
        it = iter_offset + calls[0]
        calls[0] += 1
        return sample_costs(p, members, u, mode, seed, it)

    saved = cem_ref.sample_costs
    cem_ref.sample_costs = costs
    try:
        yield
    finally:
        cem_ref.sample_costs = saved


def cem(pb, members, mode, dtype, lo, hi, kwargs=None, iter_offset=0, **more):
    """cem_ref.cem with the samples costed on the ensemble under the mode."""
    seed = int(dict(cem_ref.DEFAULTS, **(kwargs or {}))["seed"])
    with ensemble(members, mode, seed, iter_offset):
        return cem_ref.cem(pb, dtype, lo, hi, kwargs, iter_offset=iter_offset, **more)
