"""The cases of the sample-efficient CEM's tests (tests/test_icem_host.py, tests/test_gpu_icem.py): cem_cases' shapes
and problems with a number of kept rows each (TEST INFRASTRUCTURE).  With decay 1.25 the sample counts of three
iterations are N, floor(N / 1.25), floor(N / 1.5625) (never below min(N, 2 E)), so the pools (samples + kept rows, + the
mean in the last iteration) wander over partial tiles of 32 rows and sort lengths that are no power of two:

  base    40 | 32+2 | 25+2+1        m1      33 | 26+1 | 21+1+1       cheetah 400 | 320+12 | 256+12+1
  wide_m  64 | 51+2 | 40+2+1        wide_n  96 | 76+3 | 61+3+1       ragged  50 | 40+2 | 32+2+1      w256  32 | 25+1 | 20+1+1

Bounds are -1 / +1 on every control and the initial std is 0.5 (inside the bounds, so that the coloured sums are not
all clamped)."""

import functools

import numpy as np

import cem_cases as cc

ICEM_SEED = 0xCE1       # (chosen among eight seeds for the share of decided problems: test_icem_host.py)
LO, HI = cc.LO, cc.HI
INIT_STD = 0.5
DECAY, NOISE_BETA = 1.25, 2.0

CASES = cc.CASES
NUM_KEEP = dict(base=2, m1=1, cheetah=12, wide_m=2, wide_n=3, ragged=2, w256=1)
DECIDED = cc.DECIDED
problem = cc.problem


def kwargs(name, max_iter, **more):
    """The keyword set of icem_ref.icem for the case (num_elites and num_keep given, not portions)."""
    (_, _, _, _, N, E), _ = CASES[name]
    kw = dict(num_samples=N, num_elites=E, num_keep=NUM_KEEP[name], max_iter=max_iter, seed=ICEM_SEED, decay=DECAY,
              noise_beta=NOISE_BETA)
    kw.update(more)
    return kw


def engine_kwargs(name, max_iter, **more):
    """The same for Engine.icem_solve, which takes portions: ones whose int(N * portion) is E and int(E * portion)
    num_keep."""
    kw = kwargs(name, max_iter, **more)
    N, E, nk = kw["num_samples"], kw.pop("num_elites"), kw.pop("num_keep")
    kw["elite_portion"] = (E + 0.5) / N
    kw["keep_portion"] = (nk + 0.5) / E if nk else 0.0
    assert int(N * kw["elite_portion"]) == E and int(E * kw["keep_portion"]) == nk
    return kw


@functools.lru_cache(maxsize=None)
def traces(name, iters=3):
    """The fp32 and the fp64 reference run of `iters` iterations: (result32, trace32, result64, trace64)."""
    import icem_ref
    pb = problem(name)
    t32, t64 = [], []
    r32 = icem_ref.icem(pb, np.float32, LO, HI, kwargs(name, iters), trace=t32, init_std=INIT_STD)
    r64 = icem_ref.icem(pb, np.float64, LO, HI, kwargs(name, iters), trace=t64, init_std=INIT_STD)
    return r32, t32, r64, t64
