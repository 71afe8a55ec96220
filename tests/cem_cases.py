"""The cases of the cross-entropy method's tests (tests/test_cem_host.py, tests/test_gpu_cem.py), as (n, m, T, B, N, E)
plus the network widths (TEST INFRASTRUCTURE).  They cover a partial last tile of 32 samples (N = 40, 33, 400, 50), sort
lengths that are no power of two, one and two column tiles of the layer-0 input (n + m up to 66), ragged widths and
the width cap of 256.  Bounds are -1 / +1 on every control; problems come from seed 5 with bias scale 0.1."""

import functools

import numpy as np

import gpu_util as gu

PROBLEM_SEED = 5
CEM_SEED = 0x1234
LO, HI = -1.0, 1.0

#        name       n   m  T  B   N    E   extra keywords of gu.problem
CASES = {
    "base":    ((5, 2, 8, 3, 40, 4), {}),
    "m1":      ((3, 1, 5, 7, 33, 3), {}),
    "cheetah": ((17, 6, 5, 7, 400, 40), {}),
    "wide_m":  ((4, 32, 3, 2, 64, 6), dict(dyn_hidden=(32, 32))),
    "wide_n":  ((64, 2, 3, 2, 96, 9), {}),
    "ragged":  ((5, 2, 4, 3, 50, 5), dict(dyn_hidden=(7, 9), cost_hidden=(6,), cost_fout=4)),
    "w256":    ((8, 2, 2, 2, 32, 4), dict(dyn_hidden=(256, 256))),
}
# the cases of the decided protocol (w256 is there for the width cap only)
DECIDED = ("base", "m1", "cheetah", "wide_m", "wide_n", "ragged")


@functools.lru_cache(maxsize=None)
def problem(name):
    (n, m, T, B, N, E), extra = CASES[name]
    return gu.problem(n, m, T, B, seed=PROBLEM_SEED, bias_scale=0.1, **extra)


def kwargs(name, max_iter, **more):
    """The keyword set of cem_ref.cem for the case (num_elites given, not a portion)."""
    (_, _, _, _, N, E), _ = CASES[name]
    kw = dict(num_samples=N, num_elites=E, max_iter=max_iter, seed=CEM_SEED)
    kw.update(more)
    return kw


def engine_kwargs(name, max_iter, **more):
    """The same for Engine.cem_solve, which takes trajax' elite_portion: a portion whose int(N * portion) is E."""
    kw = kwargs(name, max_iter, **more)
    N, E = kw["num_samples"], kw.pop("num_elites")
    portion = (E + 0.5) / N
    assert int(N * portion) == E
    kw["elite_portion"] = portion
    return kw


@functools.lru_cache(maxsize=None)
def traces(name, iters=3):
    """The fp32 and the fp64 reference run of `iters` iterations: (result32, trace32, result64, trace64)."""
    pb = problem(name)
    t32, t64 = [], []
    import cem_ref
    r32 = cem_ref.cem(pb, np.float32, LO, HI, kwargs(name, iters), trace=t32)
    r64 = cem_ref.cem(pb, np.float64, LO, HI, kwargs(name, iters), trace=t64)
    return r32, t32, r64, t64
