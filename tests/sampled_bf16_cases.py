"""The cases of the bf16 sampled rollouts' tests (tests/test_sampled_bf16_host.py, tests/test_gpu_sampled_bf16.py;
TEST INFRASTRUCTURE), as (n, m, T, B, N, E) plus the network widths; bounds -1 / +1.  Each reaches a way the bf16
kernel can go wrong:

  A      K = 7 below one k-step of 32; K = 40: a full step and a tail; K = 24 behind a 40-wide layer: stale columns
         24 .. 31 of the operand block; N = 40 is no multiple of the 32-row tile
  B      (cem_cases "m1") one row in the second tile
  C      (cem_cases "cheetah") the widths 200 and 128
  C5, C3 the same widths, n and m with 2 problems of 40 rows, T = 5 and T = 3: the cases of the cost rule at these
         widths (below)
  D      (cem_cases "w256") width 256: no padding anywhere
  E      (cem_cases "wide_n") K = 66
  exact  integers that bf16 holds exactly: weights in {-1, 0, 1}, small integer biases, x0, goals and controls, init_std
         0 (every row is the integer mean), every matrix operand an integer of magnitude <= 256 (the host test checks
         it): bf16 mode and fp32 mode must agree bit for bit

The cost rule of the GPU test: |gpu - restatement| <= R_CAP * E_q per case, E_q = max |restatement - fp64 unrounded
costs| (what bf16 costs), and R_CAP from the restatement alone: 4 x the largest ratio E_o / E_q over the cases, E_o the
spread between two summation orders of the products (rounding flips).  test_sampled_bf16_host.py measures the ratios and
holds R_CAP to them.

Why C is not a case of the rule.  A flip of a hidden unit's rounding moves a cost by 1e-6 .. 1e-4, but a flip of a
STATE's rounding (x_t is O(1), so one bf16 step is 4e-3 .. 8e-3) moves it by 5e-4 .. 1e-2: a quarter of E_q itself,
which is the sum of thousands of such steps with random signs.  The chance of one is about 1 in a few thousand state
roundings; C has 2,800 rows x 5 steps x 17 states of them, so several of its rows flip under any change of the summation
order (measured E_o / E_q: cem 0.18, icem 0.33, mppi 0.20) and no cap below 0.5 covers it.  The rule is therefore held
at the same widths on 80 rows: C5 (cem; one state flip does occur, E_o / E_q = 0.091: it is what calibrates R_CAP --
without a case that shows a state flip the cap would be measured on hidden-unit flips alone) and C3 (icem and mppi, whose
samples at T = 5 flip two states of one row: 0.28).  C stays a case of every test that compares bit for bit or through
the fp32 rollout."""

import functools

import numpy as np

import cem_cases as cc
import cem_ref
import gan_mpc_oracle as orc
import gpu_util as gu
import icem_cases as ic
import mppi_cases as mc
import sampled_bf16_ref as sr

LO, HI = cc.LO, cc.HI
SEED = cc.CEM_SEED

CASES = {
    "A": ((5, 2, 4, 3, 40, 4), dict(dyn_hidden=(40, 24), cost_hidden=(33,), cost_fout=3)),
    "B": cc.CASES["m1"],
    "C": cc.CASES["cheetah"],
    "D": cc.CASES["w256"],
    "E": cc.CASES["wide_n"],
    "C5": ((17, 6, 5, 2, 40, 4), {}),
    "C3": ((17, 6, 3, 2, 40, 4), {}),
}
NAMES = ("A", "B", "C", "D", "E")
SOLVERS = ("cem", "icem", "mppi")
G2_CASES = {"cem": ("A", "B", "C5", "D", "E"), "icem": ("A", "C3"), "mppi": ("A", "C3")}
NUM_KEEP = dict(A=2, B=1, C=12, D=1, E=3, C5=2, C3=2)
# the softmax temperature per case: mppi_cases' rule (the median over the problems of the fp64 standard deviation of the
# iteration-0 costs; recompute_temperature(name) gives A's, C5's and C3's)
TEMPERATURE = dict(A=0.16320279942898477, B=mc.TEMPERATURE["m1"], C=mc.TEMPERATURE["cheetah"], D=mc.TEMPERATURE["w256"],
                   E=mc.TEMPERATURE["wide_n"], C5=0.3854586731325099, C3=0.1552122298040255)
# the initial std of the sampled controls: CEM's default (hi - lo) / 2, the others' cases' 0.5
INIT_STD = dict(cem=(HI - LO) / 2, icem=ic.INIT_STD, mppi=mc.INIT_STD)

# 4 x the largest E_o / E_q of the cases (measured by test_sampled_bf16_host.py::test_h3, which holds this to it)
R_CAP = 0.37

EXACT = (4, 2, 2, 2, 33, 3)          # n, m, T, B, N, E; dynamics [6, 8, 4], cost [4, 8, 3]
EXACT_SEED = 10


@functools.lru_cache(maxsize=None)
def problem(name):
    if name == "exact":
        return exact_problem()
    (n, m, T, B, N, E), extra = CASES[name]
    return gu.problem(n, m, T, B, seed=cc.PROBLEM_SEED, bias_scale=0.1, **extra)


def shape(name):
    return EXACT if name == "exact" else CASES[name][0]


def exact_problem():
    n, m, T, B, N, E = EXACT
    pb = gu.problem(n, m, T, B, seed=cc.PROBLEM_SEED, dyn_hidden=(8,), cost_hidden=(8,), cost_fout=3)
    rng = np.random.default_rng(EXACT_SEED)
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
    pb["dyn"] = [(ints(-1, 1, W.shape), ints(-2, 2, b.shape)) for W, b in pb["dyn"]]
    pb["cmlp"] = [(ints(-1, 1, W.shape), ints(-2, 2, b.shape)) for W, b in pb["cmlp"]]
    pb["x0"] = ints(-2, 2, pb["x0"].shape)
    pb["U"] = ints(-1, 1, pb["U"].shape)
    pb["goal"] = ints(-3, 3, pb["goal"].shape)
    return pb


def recompute_temperature(name="A"):
    (n, m, T, B, N, E), _ = CASES[name]
    p = orc.cast_problem(problem(name), np.float64)
    u = cem_ref.draw(p["U"], np.full(p["U"].shape, mc.INIT_STD), np.full(m, LO), np.full(m, HI), SEED, 0, N, 0.0,
                     np.float64)
    return float(np.median(np.std(cem_ref.sample_costs(p, u), axis=1)))


# ---- the keyword sets ---------------------------------------------------------------------------------------------
def ref_kwargs(solver, name, max_iter=None):
    """The keyword set of cem_ref.cem / icem_ref.icem / mppi_ref.mppi for the case; max_iter None: CEM 3 iterations,
    the others their defaults (iCEM 3, MPPI 5)."""
    n, m, T, B, N, E = shape(name)
    if solver == "cem":
        return dict(num_samples=N, num_elites=E, max_iter=3 if max_iter is None else max_iter, seed=SEED)
    if solver == "icem":
        return dict(num_samples=N, num_elites=E, num_keep=NUM_KEEP.get(name, 1), seed=ic.ICEM_SEED, decay=ic.DECAY,
                    noise_beta=ic.NOISE_BETA, max_iter=3 if max_iter is None else max_iter)
    return dict(num_samples=N, seed=SEED, temperature=TEMPERATURE.get(name, 1.0),
                max_iter=5 if max_iter is None else max_iter)


def engine_kwargs(solver, name, max_iter=None):
    """The same for Engine.cem_solve / icem_solve / mppi_solve (portions whose products truncate to E and num_keep)."""
    kw = ref_kwargs(solver, name, max_iter)
    if solver == "mppi":
        return kw
    N, E = kw["num_samples"], kw.pop("num_elites")
    kw["elite_portion"] = (E + 0.5) / N
    assert int(N * kw["elite_portion"]) == E
    if solver == "icem":
        nk = kw.pop("num_keep")
        kw["keep_portion"] = (nk + 0.5) / E if nk else 0.0
        assert int(E * kw["keep_portion"]) == nk
    return kw


# ---- the figures of the cost rule ---------------------------------------------------------------------------------
def cost_figures(pb, samples):
    """At `samples` (B, N, T, m): (restatement costs, E_q, E_o)."""
    ref = sr.sample_costs(pb, samples)
    c64 = cem_ref.sample_costs(orc.cast_problem(pb, np.float64), np.asarray(samples, np.float64))
    other = sr.sample_costs(pb, samples, sr.matmul_f32_blocks)
    return ref, float(np.max(np.abs(ref - c64))), float(np.max(np.abs(other.astype(np.float64) - ref)))


@functools.lru_cache(maxsize=None)
def first_samples(solver, name):
    """The fp32 reference's samples of iteration 0 from the mean pb["U"]: (B, N, T, m)."""
    import icem_ref
    pb = problem(name)
    n, m, T, B, N, E = shape(name)
    mean = pb["U"].astype(np.float32)
    std = np.full(mean.shape, INIT_STD[solver], np.float32)
    lo, hi = np.full(m, LO, np.float32), np.full(m, HI, np.float32)
    if solver == "icem":
        return icem_ref.draw(mean, std, lo, hi, ic.ICEM_SEED, 0, N, ic.NOISE_BETA, np.float32)
    return cem_ref.draw(mean, std, lo, hi, SEED, 0, N, 0.0, np.float32)


@functools.lru_cache(maxsize=None)
def figures(solver, name):
    """(E_q, E_o) of the case at the reference's iteration-0 samples."""
    _, eq, eo = cost_figures(problem(name), first_samples(solver, name))
    return eq, eo
