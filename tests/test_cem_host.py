"""The cross-entropy method solver without a device: the sampler of tests/cem_ref.py against
Philox' known answers and the normal distribution, the elite selection against brute force, the reference solve
lowering every objective, the decided protocol that the GPU test's free run relies on, the C ABI (header, ctypes table,
Engine argument order) and every refusal the host makes before a launch."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cem_cases as cc
import cem_ref as cr
import gan_mpc_oracle as orc
from gan_mpc_amd import _lib
from gan_mpc_amd import engine as E_
from gan_mpc_amd._lib import GmpcError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Share of the problems of cc.DECIDED that are decided through three iterations (fp32 and fp64 pick the same elites
# and the fp64 costs leave a relative gap above 1e-5 at the E-th place, at every iteration): 23 of 24 on seed 0x1234,
# problem seed 5 -- the one undecided problem is wide_n's second at the third iteration.
MIN_AGREE = 23 / 24


# ---- the sampler -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert " ".join("%08x" % int(x) for x in cr.philox(counter, key)) == want


def test_uniforms_are_exact_in_fp32_and_never_0_or_1():
    r = np.array([0, 1, 511, 512, 0xFFFFFFFF, 0x80000000], np.uint32)
    u32, u64 = cr.uniforms(r, np.float32), cr.uniforms(r, np.float64)
    np.testing.assert_array_equal(u32.astype(np.float64), u64)
    assert u64.min() == 2.0 ** -24 and u64.max() == 1.0 - 2.0 ** -24


def test_normals_mean_variance_and_independence():
    """1e5 draws: every statistic within 4 sigma of its value under N(0, 1) and independence."""
    T, m, S = 10, 5, 2000
    z = cr.normals(cc.CEM_SEED, 0, 0, np.arange(S), T * m)              # (S, T m)
    n = z.size
    assert n == 100000
    assert abs(z.mean()) < 4 / np.sqrt(n)
    assert abs(z.var() - 1) < 4 * np.sqrt(2 / n)
    assert abs((z ** 3).mean()) < 4 * np.sqrt(15 / n)
    assert abs((z ** 4).mean() - 3) < 4 * np.sqrt(96 / n)

    def corr(a, b):
        return abs(np.mean(a * b)) * np.sqrt(a.size)        # ~ |N(0, 1)| for independent standard normals

    assert corr(z[:, :-1], z[:, 1:]) < 4                     # neighbouring elements (the two Box-Muller outputs too)
    assert corr(z[:, :-2], z[:, 2:]) < 4 and corr(z[:, :-4], z[:, 4:]) < 4    # across pairs and across groups
    assert corr(z[:-1], z[1:]) < 4                           # neighbouring samples
    assert corr(z, cr.normals(cc.CEM_SEED, 0, 1, np.arange(S), T * m)) < 4           # problems
    assert corr(z, cr.normals(cc.CEM_SEED, 1, 0, np.arange(S), T * m)) < 4           # iterations
    assert corr(z, cr.normals(cc.CEM_SEED + 1, 0, 0, np.arange(S), T * m)) < 4       # seeds
    assert corr(z, cr.normals(cc.CEM_SEED + (1 << 32), 0, 0, np.arange(S), T * m)) < 4


def test_smoothing_keeps_the_variance_and_correlates_neighbouring_steps():
    z = cr.normals(3, 0, 0, np.arange(4000), 6 * 2).reshape(4000, 6, 2)
    s = cr.smooth(z, 0.6, np.float64)
    np.testing.assert_array_equal(s[:, 0], z[:, 0])
    np.testing.assert_allclose(s[:, 3], 0.6 * s[:, 2] + 0.8 * z[:, 3], rtol=0, atol=1e-6)   # (beta is an fp32 value)
    assert abs(s[:, 5].var() - 1) < 4 * np.sqrt(2 / 8000)
    assert abs(np.mean(s[:, 4] * s[:, 5]) - 0.6) < 4 / np.sqrt(8000)
    assert cr.smooth(z, 0.0, np.float64) is z


# ---- elites and update -----------------------------------------------------------------------------------------------
def test_elite_selection_against_brute_force_with_ties_and_nan():
    rng = np.random.default_rng(0)
    for N, E in ((40, 4), (33, 3), (50, 50), (7, 1)):
        c = rng.integers(0, 6, (5, N)).astype(np.float32)          # many ties
        c[1, ::3] = np.nan
        c[2, :] = np.nan
        c[3, 1] = np.inf
        c[3, 0] = np.nan                                           # NaN ties with +inf: the index decides
        c[4, :] = -0.0
        c[4, 5] = 0.0                                              # -0 and +0 tie: the index decides
        got = cr.elites_of(c, E)
        for b in range(5):
            key = [(np.inf if np.isnan(v) else float(v), i) for i, v in enumerate(c[b])]
            want = [i for _, i in sorted(key)][:E]
            assert list(got[b]) == want, (N, E, b)


def test_update_is_the_elites_mean_and_population_std():
    rng = np.random.default_rng(1)
    u = rng.standard_normal((2, 9, 3, 2))
    c = rng.standard_normal((2, 9))
    mean, std = rng.standard_normal((2, 3, 2)), rng.random((2, 3, 2))
    nm, ns, el = cr.update(u, c, mean, std, 4, 0.25)
    for b in range(2):
        e = u[b][np.argsort(c[b])[:4]]
        np.testing.assert_allclose(nm[b], 0.25 * mean[b] + 0.75 * e.mean(0), rtol=1e-12)
        np.testing.assert_allclose(ns[b], 0.25 * std[b] + 0.75 * e.std(0), rtol=1e-12)


# ---- the solve -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_cem_lowers_the_objective_of_every_problem(name):
    pb = cc.problem(name)
    p64 = orc.cast_problem(pb, np.float64)
    out = cr.cem(pb, np.float64, cc.LO, cc.HI, cc.kwargs(name, 10))
    start = orc.objective(p64["dyn"], p64["cmlp"], p64["mpc_w"], p64["goal"], np.clip(p64["U"], cc.LO, cc.HI),
                          p64["x0"])
    assert (out["obj"] < start).all(), (out["obj"], start)
    assert (np.abs(out["U"]) <= 1 + 1e-12).all() and (out["std"] <= 1 + 1e-12).all()


def test_the_decided_protocol_holds_for_most_problems():
    total = ok = 0
    for name in cc.DECIDED:
        (n, m, T, B, N, E), _ = cc.CASES[name]
        r32, t32, r64, t64 = cc.traces(name)
        d = cr.decided(t32, t64, E)
        assert d.shape == (3, B)
        print(name, "decided through iteration 1 / 2 / 3:", d.sum(1), "of", B)
        total += B
        ok += int(d[2].sum())
        # on a decided problem both runs refit the same elites: mean and std agree to fp32
        for k in ("U", "std"):
            assert np.abs(r32[k][d[2]] - r64[k][d[2]]).max(initial=0) < 1e-5
    assert MIN_AGREE >= 0.5 and ok / total >= MIN_AGREE, (ok, total)


# ---- C ABI -----------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()


def test_library_exports_and_header_declares_the_solver():
    assert hasattr(_lib.load(), "gmpc_cem_solve")
    m = re.search(r"int\s+gmpc_cem_solve\s*\(([^)]*)\)\s*;", _header())
    assert m, "gmpc_cem_solve is not declared"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["gmpc_ctx* ctx", "int B", "const float* x0", "const float* goal", "const float* u_lo",
                      "const float* u_hi", "const gmpc_cem_opts* opts", "float* mean_io", "float* std_io", "float* X",
                      "float* obj", "float* costs", "int* elites", "float* samples", "void* stream"]
    res, args = _lib.SIGNATURES["gmpc_cem_solve"]
    assert res is C.c_int and len(args) == len(params)
    for a, p in zip(args, params):
        if p.startswith("int "):
            assert a is C.c_int
        elif "gmpc_cem_opts" in p:
            assert a is C.POINTER(_lib.CemOpts)
        else:
            assert a is C.c_void_p


def test_opts_struct_matches_the_header():
    m = re.search(r"typedef struct gmpc_cem_opts \{(.*?)\} gmpc_cem_opts;", _header(), re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype = re.match(r"(unsigned long long|int|float)\s", decl).group(1)
            names = [x.strip() for x in decl[len(ctype):].split(",")]
            fields += [(x, ctype) for x in names]
    ctypes_of = {"int": C.c_int, "float": C.c_float, "unsigned long long": C.c_ulonglong}
    assert [(f, ctypes_of[t]) for f, t in fields] == list(_lib.CemOpts._fields_)
    assert C.sizeof(_lib.CemOpts) == 32


def test_make_cem_opts_follows_trajax():
    assert E_.TRAJAX_CEM_KWARGS == dict(sampling_smoothing=0.0, evolution_smoothing=0.1, elite_portion=0.1,
                                        max_iter=10, num_samples=400, seed=0)
    assert cr.DEFAULTS == E_.TRAJAX_CEM_KWARGS
    o = E_.make_cem_opts()
    assert (o.max_iter, o.num_samples, o.num_elites, o.iter_offset, o.seed) == (10, 400, 40, 0, 0)
    assert o.evolution_smoothing == np.float32(0.1) and o.sampling_smoothing == 0.0
    o = E_.make_cem_opts(dict(num_samples=33, elite_portion=0.1, seed=(5 << 32) + 7), iter_offset=3)
    assert (o.num_elites, o.iter_offset, o.seed) == (3, 3, (5 << 32) + 7)        # int(3.3), as trajax truncates
    with pytest.raises(GmpcError, match="cem: unknown"):
        E_.make_cem_opts(dict(num_elites=4))
    for name in cc.CASES:
        (n, m, T, B, N, E), _ = cc.CASES[name]
        o = E_.make_cem_opts(cc.engine_kwargs(name, 3))
        assert (o.num_samples, o.num_elites, o.max_iter, o.seed) == (N, E, 3, cc.CEM_SEED)


class _Recorder:
    """Stands in for the library: records the one call Engine.cem_solve makes."""

    def __init__(self):
        self.calls = []

    def gmpc_cem_solve(self, *args):
        self.calls.append(args)
        return 0


def _host_engine(n=3, m=2, T=4):
    eng = E_.Engine.__new__(E_.Engine)
    eng.n, eng.m, eng.T, eng.nx = n, m, T, n
    eng.device = torch.device("cpu")
    eng.ctx = None
    eng.lib = _Recorder()
    return eng


def test_engine_passes_the_arguments_in_the_header_order(monkeypatch):
    eng = _host_engine()
    B, n, m, T = 2, 3, 2, 4
    monkeypatch.setattr(E_, "_ptr", lambda t: None if t is None else t)
    monkeypatch.setattr(E_.Engine, "_stream", lambda self: "stream")
    x0, U, goal = torch.zeros(B, n), torch.full((B, T, m), 0.5), torch.zeros(B, T + 1, n)
    out = eng.cem_solve(x0, U, goal, [-1.0, -2.0], 3.0, dict(num_samples=20, max_iter=2, seed=9),
                        want=("samples", "costs"), iter_offset=5)
    (ctx, b, a_x0, a_goal, lo, hi, opts, mean, std, X, obj, costs, elites, samples, stream), = eng.lib.calls
    assert ctx is None and b == B and a_x0 is x0 and a_goal is goal and stream == "stream"
    assert lo.tolist() == [-1.0, -2.0] and hi.tolist() == [3.0, 3.0]
    o = opts._obj
    assert (o.num_samples, o.num_elites, o.max_iter, o.iter_offset, o.seed) == (20, 2, 2, 5, 9)
    assert mean is out["U"] and mean is not U and torch.equal(mean, U)           # the caller's start is not written
    assert std is out["std"] and tuple(std.shape) == (B, T, m)
    assert torch.equal(std[0, 0], torch.tensor([2.0, 2.5]))                      # (hi - lo) / 2 per control
    assert X is out["X"] and tuple(X.shape) == (B, T + 1, n) and obj is out["obj"] and tuple(obj.shape) == (B,)
    assert costs is out["costs"] and tuple(costs.shape) == (B, 20)
    assert samples is out["samples"] and tuple(samples.shape) == (B, 20, T, m)
    assert elites is None and "elites" not in out
    # init_std: a scalar, m values, or a whole (B, T, m) tensor
    eng.cem_solve(x0, U, goal, None, None, dict(num_samples=20), init_std=0.25)
    assert torch.equal(eng.lib.calls[-1][8], torch.full((B, T, m), 0.25)) and eng.lib.calls[-1][4] is None
    given = torch.rand(B, T, m)
    eng.cem_solve(x0, U, goal, None, 1.0, dict(num_samples=20), init_std=given, want=("elites",))
    assert torch.equal(eng.lib.calls[-1][8], given) and eng.lib.calls[-1][8] is not given
    assert eng.lib.calls[-1][12].dtype == torch.int32 and tuple(eng.lib.calls[-1][12].shape) == (B, 2)


def test_host_refusals_come_before_any_call():
    eng = _host_engine()
    B, n, m, T = 2, 3, 2, 4
    x0, U, goal = torch.zeros(B, n), torch.zeros(B, T, m), torch.zeros(B, T + 1, n)
    bad = [
        (dict(u_lo=-1.0, u_hi=None), "cem: .*init_std"),
        (dict(u_lo=None, u_hi=1.0), "cem: .*init_std"),
        (dict(u_lo=None, u_hi=None), "cem: .*init_std"),
        (dict(u_lo=-np.inf, u_hi=1.0), "cem: .*init_std"),
        (dict(u_lo=[-1.0, -1.0], u_hi=[1.0, np.inf]), "cem: .*init_std"),
        (dict(u_lo=1.0, u_hi=-1.0), "u_lo must be <= u_hi"),
        (dict(u_lo=[0.0, 0.0, 0.0], u_hi=1.0), "u_lo must be a scalar or 2 values"),
        (dict(u_lo=float("nan"), u_hi=1.0), "NaN"),
        (dict(kwargs=dict(bogus=1)), "cem: unknown keyword"),
        (dict(want=("noise",)), "cem: want"),
        (dict(x0=torch.zeros(B, n + 1)), "cem: x0 must be"),
        (dict(U_init=torch.zeros(B, T + 1, m)), "cem: U_init must be"),
        (dict(goal=torch.zeros(B, T, n)), "cem: goal must be"),
    ]
    for change, match in bad:
        args = dict(x0=x0, U_init=U, goal=goal, u_lo=-1.0, u_hi=1.0)
        args.update(change)
        with pytest.raises(GmpcError, match=match):
            eng.cem_solve(**args)
    assert eng.lib.calls == []


# ---- the policy ------------------------------------------------------------------------------------------------------
def _policy(cls, **kw):
    return cls(config=None, cost_model=None, dynamics_model=None, expert_model=None, **kw)


def test_policy_takes_the_solver_with_its_bounds():
    from gan_mpc_amd.policy.base import BaseMPC
    from gan_mpc_amd.policy.eval import EvalMPC
    assert "cem" in EvalMPC.SOLVERS
    p = _policy(EvalMPC, solver="cem", control_bounds=(-1.0, 1.0), cem_kwargs=dict(num_samples=64))
    assert p.solver == "cem" and p.control_bounds == (-1.0, 1.0) and p.cem_solves == 0
    assert p.cem_kwargs == dict(E_.TRAJAX_CEM_KWARGS, num_samples=64)
    assert _policy(EvalMPC, solver="cem", control_bounds=(-1.0, 1.0)).cem_kwargs == E_.TRAJAX_CEM_KWARGS
    assert _policy(BaseMPC, solver="cem", control_bounds=(-1.0, 1.0)).solver == "cem"
    # the existing error cases keep raising, and "cem" needs its bounds as "box" does
    for kw in (dict(solver="cem"), dict(solver="box"), dict(solver="rounds", control_bounds=(-1, 1)),
               dict(solver="fused", control_bounds=(-1, 1)), dict(control_bounds=(-1, 1)),
               dict(solver="cem", control_bounds=(-1, 0, 1)), dict(solver="box", control_bounds=(1,)),
               dict(solver="bogus"), dict(solver="rounds", cem_kwargs=dict(num_samples=8)),
               dict(solver="box", control_bounds=(-1, 1), cem_kwargs={})):
        with pytest.raises(ValueError):
            _policy(EvalMPC, **kw)
    assert _policy(EvalMPC, solver="box", control_bounds=(-1, 1)).solver == "box"
    assert _policy(EvalMPC).solver == "rounds"


def test_training_calls_of_a_cem_policy_raise_before_any_device_work():
    from gan_mpc_amd.norm.l2_policy import L2MPC
    from gan_mpc_amd.policy import differentiable as diff
    from gan_mpc_amd.policy import optimizers as opt
    p = _policy(L2MPC, solver="cem", control_bounds=(-1.0, 1.0))
    hist = np.zeros((2, 3, 4), np.float32)
    # (config, models and parameters are None: anything past the refusal would fail with another error)
    with pytest.raises(NotImplementedError, match="cem"):
        p.loss_and_grad(hist, None, (None,))
    with pytest.raises(NotImplementedError, match="cem"):
        p.batch_loss(None, hist, None)
    with pytest.raises(NotImplementedError, match="cem"):
        diff.ilqr_layer(p, None, None, None, None)
    with pytest.raises(NotImplementedError, match="cem"):
        opt.bilevel_optimization(p, None, torch.zeros(2, 4), None, None, 0)
    with pytest.raises(NotImplementedError, match="cem"):
        opt._solver(p, None, hold=True)
    assert p.cem_solves == 0 and p._engine is None
