"""The cases of the dynamics ensemble's tests (tests/test_sampled_ensemble_host.py, tests/test_gpu_sampled_ensemble.py;
gmpc_set_sampled_ensemble; TEST INFRASTRUCTURE): cem_cases' shapes and problems -- a partial last
tile of 32 rows, ragged widths, two column tiles, the width cap -- with the other two solvers' keywords from icem_cases /
mppi_cases / sampled_bf16_cases, and per case an ensemble of P = 3 members around the nominal network:

  member p's layer (W, b) = (W + 0.05f W', b + 0.05f b'), (W', b') the same layer of
  gpu_util.problem(n, m, T, B, seed=100 + p, bias_scale=0.1, **extra)

a perturbation of the nominal network, as a trained ensemble is.  Measured on the CPU with cem_ref (test_h3 prints it):
at iteration 0 the fp64 ensemble cost differs from the nominal cost by 2e-3 .. 8e-2 relative, two members from each other
by 9e-3 .. 1.2e-1, and the ensemble changes the elite set of 12 of the 24 problems -- a comparison against the nominal
costs cannot pass by accident."""

import functools

import numpy as np

import cem_cases as cc
import gpu_util as gu
import sampled_bf16_cases as sc
from gan_mpc_amd import params as P

CASES = cc.CASES
NAMES = list(cc.CASES)
DECIDED = cc.DECIDED
LO, HI = cc.LO, cc.HI
problem = cc.problem
MEMBERS = 3
MEMBER_SEED = 100
EPS = np.float32(0.05)
SOLVERS = sc.SOLVERS
PRECISIONS = ("fp32", "bf16")
# the cases of the bitwise groups E1 - E4: one tile, 13 tiles with a partial last one, ragged widths, the width cap
BITWISE = ("base", "cheetah", "ragged", "w256")
# cem_cases' names in sampled_bf16_cases, whose engine_kwargs give every solver's keywords per case
_SC_NAME = dict(m1="B", cheetah="C", w256="D", wide_n="E")
NUM_KEEP = dict(base=2, m1=1, cheetah=12, wide_m=2, wide_n=3, ragged=2, w256=1)    # icem_cases.NUM_KEEP


@functools.lru_cache(maxsize=None)
def members(name, count=MEMBERS):
    """The members' dynamics layers: a tuple of `count` lists of (W, b), fp32."""
    (n, m, T, B, N, E), extra = CASES[name]
    nominal = problem(name)["dyn"]
    out = []
    for p in range(count):
        other = gu.problem(n, m, T, B, seed=MEMBER_SEED + p, bias_scale=0.1, **extra)["dyn"]
        out.append([((W + EPS * W2).astype(np.float32), (b + EPS * b2).astype(np.float32))
                    for (W, b), (W2, b2) in zip(nominal, other)])
    return tuple(out)


def flat(layer_lists):
    """(P, dyn count) fp32: the members' flat parameter vectors in gmpc_set_params' layout."""
    return np.stack([P.pack_mlp(P.layers_to_tree(layers)) for layers in layer_lists]).astype(np.float32)


def nominal_flat(name, count=1):
    return flat([problem(name)["dyn"]] * count)


def engine_kwargs(solver, name, max_iter, **more):
    """The keyword set of Engine.cem_solve / icem_solve / mppi_solve for the case (sampled_bf16_cases' rule: CEM's seed
    and elites from cem_cases, iCEM's keep / decay / colour from icem_cases, MPPI's temperature from mppi_cases)."""
    import icem_cases as ic
    import mppi_cases as mc
    if solver == "cem":
        kw = cc.engine_kwargs(name, max_iter)
    elif solver == "icem":
        kw = ic.engine_kwargs(name, max_iter)
    else:
        kw = mc.kwargs(name, max_iter)
    kw.update(more)
    return kw


def init_std(solver):
    """None: CEM's default (hi - lo) / 2; the others' cases' 0.5."""
    return None if solver == "cem" else sc.INIT_STD[solver]
