"""NumPy restatement of the sampling solvers' costs under a dynamics ensemble (gmpc_set_sampled_ensemble, DESIGN.md
section 24; TEST INFRASTRUCTURE): cem_ref.sample_costs per member on dict(pb, dyn=member), combined by the library's
rule in the run's dtype,

  cost = (((J_0 + J_1) + J_2) + ... + J_{P-1}) * (1 / P)      sequential in p, 1 / P rounded once in the dtype,

and plugged into cem_ref's loop.  X and obj of the result stay those of pb's own (nominal) dynamics, as the library's."""

import contextlib

import numpy as np

import cem_ref


def combine(member_costs, dtype=None):
    """The members' costs, a sequence of equal-shaped arrays, -> the ensemble's, in `dtype` (default: theirs)."""
    dt = np.dtype(member_costs[0].dtype if dtype is None else dtype).type
    with np.errstate(all="ignore"):
        s = np.asarray(member_costs[0], dt)
        for c in member_costs[1:]:
            s = (s + np.asarray(c, dt)).astype(dt)
        return (s * (dt(1.0) / dt(len(member_costs)))).astype(dt)


def cast_members(members, dtype):
    return [[(W.astype(dtype), b.astype(dtype)) for W, b in layers] for layers in members]


def member_costs(pb, members, samples):
    """[P] arrays (B, N): cem_ref.sample_costs under each member, in the dtype of pb."""
    return [_plain_sample_costs(dict(pb, dyn=layers), samples) for layers in cast_members(members, pb["x0"].dtype)]


def sample_costs(pb, members, samples):
    return combine(member_costs(pb, members, samples))


_plain_sample_costs = cem_ref.sample_costs


@contextlib.contextmanager
def ensemble(members):
    """While open, cem_ref's loop costs its samples on the ensemble."""
    cem_ref.sample_costs = lambda p, u: sample_costs(p, members, u)
    try:
        yield
    finally:
        cem_ref.sample_costs = _plain_sample_costs


def cem(pb, members, dtype, lo, hi, kwargs=None, **more):
    """cem_ref.cem with the samples costed on the ensemble."""
    with ensemble(members):
        return cem_ref.cem(pb, dtype, lo, hi, kwargs, **more)
