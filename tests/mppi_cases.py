"""The cases of the path-integral solver's tests (tests/test_mppi_host.py, tests/test_gpu_mppi.py; TEST
INFRASTRUCTURE): cem_cases' shapes and problems (N = 40, 33, 400, 64, 96, 50, 32: a partial last tile of samples),
bounds -1 / +1, init_std 0.5, and one softmax temperature per case -- the median over the problems of the fp64 standard
deviation of the iteration-0 costs (recompute() prints them), so that the weights are neither uniform nor one-hot."""

import functools

import numpy as np

import cem_cases as cc
import cem_ref
import gan_mpc_oracle as orc

CASES = cc.CASES
problem = cc.problem
LO, HI = cc.LO, cc.HI
SEED = cc.CEM_SEED
INIT_STD = 0.5

TEMPERATURE = {
    "base": 1.860559886409759,
    "m1": 0.25780422548188603,
    "cheetah": 0.3661456280527624,
    "wide_m": 0.34622352108097254,
    "wide_n": 0.08520861469176595,
    "ragged": 0.158602904991636,
    "w256": 0.0685884766435011,
}


def recompute():
    """The temperatures from their definition -> dict."""
    out = {}
    for name in CASES:
        (n, m, T, B, N, E), _ = CASES[name]
        p = orc.cast_problem(problem(name), np.float64)
        u = cem_ref.draw(p["U"], np.full(p["U"].shape, INIT_STD), np.full(m, LO), np.full(m, HI), SEED, 0, N, 0.0,
                         np.float64)
        out[name] = float(np.median(np.std(cem_ref.sample_costs(p, u), axis=1)))
    return out


def kwargs(name, max_iter, **more):
    """The keyword set of mppi_ref.mppi and Engine.mppi_solve for the case."""
    kw = dict(num_samples=CASES[name][0][4], max_iter=max_iter, seed=SEED, temperature=TEMPERATURE[name])
    kw.update(more)
    return kw


@functools.lru_cache(maxsize=None)
def traces(name, iters=3):
    """The fp32 and the fp64 reference run of `iters` iterations: (result32, trace32, result64, trace64)."""
    import mppi_ref
    pb = problem(name)
    t32, t64 = [], []
    r32 = mppi_ref.mppi(pb, np.float32, LO, HI, kwargs(name, iters), trace=t32, init_std=INIT_STD)
    r64 = mppi_ref.mppi(pb, np.float64, LO, HI, kwargs(name, iters), trace=t64, init_std=INIT_STD)
    return r32, t32, r64, t64


# the gradient cases of B1: (case, iterations, extra keywords)
GRAD_CASES = {
    "base": ("base", 2, {}),
    "m1": ("m1", 2, {}),
    "ragged": ("ragged", 2, {}),
    "wide_m": ("wide_m", 2, {}),
    "cheetah": ("cheetah", 1, {}),
    "base_gamma": ("base", 2, dict(evolution_smoothing=0.3)),
    "m1_smooth": ("m1", 2, dict(sampling_smoothing=0.6)),
}


@functools.lru_cache(maxsize=None)
def cotangents(name):
    """Random (gX, gU, gobj) of the case's shapes, fp64."""
    (n, m, T, B, N, E), _ = CASES[name]
    rng = np.random.default_rng(11)
    return rng.standard_normal((B, T + 1, n)), rng.standard_normal((B, T, m)), rng.standard_normal(B)


@functools.lru_cache(maxsize=None)
def grad_refs(gname):
    """The arbiter of a gradient case: (grads64, grads32, forward64 (X, U, obj arrays), pre-clamp samples of the fp64
    run), from the float64 / float32 autograd of mppi_ref.torch_mppi under cotangents(case)."""
    import mppi_ref
    import torch
    name, K, more = GRAD_CASES[gname]
    gX, gU, gobj = cotangents(name)
    out = []
    pre = []
    for dt in (torch.float64, torch.float32):
        lv = mppi_ref.leaves(problem(name), dt)
        X, U, obj = mppi_ref.torch_mppi(lv, LO, HI, kwargs(name, K, **more), INIT_STD,
                                        pre=pre if dt == torch.float64 else None)
        out.append(mppi_ref.torch_grads(lv, mppi_ref.cotangent_loss(X, U, obj, gX, gU, gobj)))
        if dt == torch.float64:
            fwd = tuple(a.detach().numpy() for a in (X, U, obj))
    return out[0], out[1], fwd, pre
