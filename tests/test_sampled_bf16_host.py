"""The bf16 mode of the sampled rollouts on the CPU: the rounding (H1), the exact case (H2), the
cap of the GPU test's cost rule measured on the restatement alone (H3), that the restatement-driven solvers still
lower the true objective (H4), and the plumbing of the new entry point (H5)."""

import functools
import os
import re

import numpy as np
import pytest

import cem_ref
import gan_mpc_oracle as orc
import icem_ref
import mppi_ref
import sampled_bf16_cases as sc
import sampled_bf16_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# ---- H1 ------------------------------------------------------------------------------------------------------------
def test_h1_round_bf16_known_answers():
    one = np.float32(1.0)
    r = lambda v: sr.round_bf16(np.array([v], np.float32))[0]
    assert r(one + np.float32(2.0 ** -8)) == one                                  # a tie, down to the even 1
    assert r(one + np.float32(3 * 2.0 ** -8)) == one + np.float32(2.0 ** -6)      # a tie, up to the even 1 + 2^-6
    assert r(one + np.float32(2.0 ** -8) + np.float32(2.0 ** -23)) == one + np.float32(2.0 ** -7)   # just above a tie
    assert r(np.finfo(np.float32).max) == np.float32(np.inf)
    assert r(-np.finfo(np.float32).max) == np.float32(-np.inf)
    assert np.isnan(r(np.float32(np.nan))) and np.isnan(r(_f32(0xFFC00001)))
    mz = r(np.float32(-0.0))
    assert mz == 0 and np.signbit(mz)
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 20, 100000))).astype(np.float32)
    q = sr.round_bf16(v)
    assert np.array_equal(sr.round_bf16(q), q)
    assert not np.any(q.view(np.uint32) & np.uint32(0xFFFF))
    assert np.all(np.abs(q - v) <= np.abs(v) * 2.0 ** -8)


# ---- H2 ------------------------------------------------------------------------------------------------------------
def test_h2_exact_case_costs_equal_the_fp32_costs_bitwise():
    pb = sc.problem("exact")
    n, m, T, B, N, E = sc.EXACT
    assert [W.shape for W, _ in pb["dyn"]] == [(6, 8), (8, 4)] and [W.shape for W, _ in pb["cmlp"]] == [(4, 8), (8, 3)]
    for W, b in pb["dyn"] + pb["cmlp"]:
        assert set(np.unique(W)) <= {-1.0, 0.0, 1.0} and np.array_equal(b, np.round(b))
    samples = np.repeat(np.clip(pb["U"], sc.LO, sc.HI)[:, None], N, axis=1)       # init_std 0: every row is the mean
    seen = []
    c = sr.sample_costs(pb, samples, seen=seen)
    assert max(seen) <= 256 and max(seen) >= 8, seen
    c32 = cem_ref.sample_costs(pb, samples)
    assert c32.dtype == np.float32 and np.array_equal(c.view(np.uint32), c32.view(np.uint32))
    assert np.array_equal(sr.sample_costs(pb, samples, sr.matmul_f32_blocks).view(np.uint32), c.view(np.uint32))
    assert np.all(np.isfinite(c)) and np.unique(c).size == B


# ---- H3 ------------------------------------------------------------------------------------------------------------
def test_h3_the_cap_of_the_cost_rule():
    worst = 0.0
    for solver in sc.SOLVERS:
        for name in sc.G2_CASES[solver]:
            eq, eo = sc.figures(solver, name)
            print(f"H3 {solver} {name}: E_q {eq:.3e}, E_o {eo:.3e}, ratio {eo / eq:.4f}")
            assert eq > 1e-3, "bf16 costs nothing here: the case shows nothing"
            assert eo / eq < 0.1, "not comfortably below 0.125: the wrong case"
            worst = max(worst, eo / eq)
    print(f"H3: r = 4 x {worst:.4f} = {4 * worst:.4f}; R_CAP = {sc.R_CAP}")
    assert 4 * worst <= sc.R_CAP < 0.5
    assert sc.R_CAP < 4 * worst * 1.05, "R_CAP is the measured cap, rounded up"


def test_h3_the_cheetah_case_is_beyond_the_rule():
    """What sampled_bf16_cases' docstring says of C: measured here, so that the figures there stay true."""
    for solver in sc.SOLVERS:
        eq, eo = sc.figures(solver, "C")
        print(f"H3 {solver} C: E_q {eq:.3e}, E_o {eo:.3e}, ratio {eo / eq:.4f}")
        assert eo / eq > 0.125


# ---- H4 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solve(solver, name):
    pb = sc.problem(name)
    kw = sc.ref_kwargs(solver, name)
    with sr.bf16_costs():
        if solver == "cem":
            return cem_ref.cem(pb, np.float32, sc.LO, sc.HI, kw)
        if solver == "icem":
            return icem_ref.icem(pb, np.float32, sc.LO, sc.HI, kw, init_std=sc.INIT_STD["icem"])
        return mppi_ref.mppi(pb, np.float32, sc.LO, sc.HI, kw, init_std=sc.INIT_STD["mppi"])


@pytest.mark.parametrize("name", sc.NAMES)
@pytest.mark.parametrize("solver", sc.SOLVERS)
def test_h4_restatement_driven_solvers_lower_the_true_objective(solver, name):
    pb64 = orc.cast_problem(sc.problem(name), np.float64)
    obj = lambda U: orc.objective(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"],
                                  np.asarray(U, np.float64), pb64["x0"])
    start = obj(np.clip(pb64["U"], sc.LO, sc.HI))
    end = obj(_solve(solver, name)["U"])
    print(f"H4 {solver} {name}: start {start}, end {end}")
    assert np.all(end < start)
    assert cem_ref.sample_costs.__module__ == "cem_ref"       # the wrapper put it back


# ---- H5 ------------------------------------------------------------------------------------------------------------
def test_h5_the_entry_point_is_declared_and_bound():
    from gan_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    assert re.search(r"\bint\s+gmpc_set_sampled_precision\s*\(\s*gmpc_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", header)
    assert re.search(r"GMPC_SAMPLED_FP32\s*=\s*0\b", header) and re.search(r"GMPC_SAMPLED_BF16\s*=\s*1\b", header)
    import ctypes as C
    assert _lib.SIGNATURES["gmpc_set_sampled_precision"] == (C.c_int, [C.c_void_p, C.c_int])


def test_h5_the_engine_refuses_other_precisions_before_the_library():
    from gan_mpc_amd._lib import GmpcError
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)          # no context, no library: a call into it would raise AttributeError
    for bad in ("fp16", None, 1):
        with pytest.raises(GmpcError, match="sampled precision: "):
            eng.set_sampled_precision(bad)


def test_h5_a_policy_refuses_the_precision_without_a_sampling_solver():
    from gan_mpc_amd.policy.eval import EvalMPC
    with pytest.raises(ValueError, match="sampled_precision"):
        EvalMPC(None, None, None, None, solver="rounds", sampled_precision="bf16")
    with pytest.raises(ValueError, match="sampled_precision"):
        EvalMPC(None, None, None, None, solver="cem", control_bounds=(-1.0, 1.0), sampled_precision="fp16")
    p = EvalMPC(None, None, None, None, solver="cem", control_bounds=(-1.0, 1.0), sampled_precision="bf16")
    assert p.sampled_precision == "bf16"
    assert EvalMPC(None, None, None, None).sampled_precision is None
