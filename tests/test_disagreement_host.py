"""The one-step ensemble disagreement without a GPU (gmpc_set_sampled_disagreement / gmpc_ensemble_disagreement,
DESIGN.md section 28): the declarations, bindings, argument order and every Engine and policy refusal raised before the
library is called (H1); the reference where it must be exact -- members equal to the nominal layers, penalty 0 -- and
against a plain loop (H2); what the cases' penalties give (H3); the decided protocol (H4).

Measured with the committed reference (the tests print it): per sample penalty * mean_p D / J 0.011 .. 1.03 and D
1.4e-3 .. 0.91 over the seven cases, per case penalty * mean(D) / mean(J) 0.11 .. 0.59; the penalty changes the
iteration-0 elite set of 21 of the 24 problems of DECIDED; through the third iteration 21 of 24 problems stay decided
under aggregate mean (base 3, m1 7, cheetah 5, wide_m 2, wide_n 1, ragged 3) and 24 of 24 under max."""

import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import cem_cases as cc
import cem_ref as cr
import disagreement_cases as dc
import disagreement_ref as dr
import gan_mpc_oracle as orc
from gan_mpc_amd._lib import GmpcError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_ARGS = ["ctx", "kind", "penalty"]
PLAN_ARGS = ["ctx", "B", "S", "P", "dyn_members", "x0", "U", "X", "d", "D", "stream"]


# ---- H1 ------------------------------------------------------------------------------------------------------------
def _decl(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_h1_the_entry_points_are_declared_and_bound():
    from gan_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    assert re.search(r"enum\s*{\s*GMPC_DIS_OFF\s*=\s*0\s*,\s*GMPC_DIS_ONESTEP\s*=\s*1\s*}", header)
    decl = _decl(header, "gmpc_set_sampled_disagreement")
    assert [a.split()[-1].lstrip("*") for a in decl] == SET_ARGS
    assert decl[1].startswith("int ") and decl[2].startswith("float ")
    assert _lib.SIGNATURES["gmpc_set_sampled_disagreement"] == (C.c_int, [C.c_void_p, C.c_int, C.c_float])
    decl = _decl(header, "gmpc_ensemble_disagreement")
    assert [a.split()[-1].lstrip("*") for a in decl] == PLAN_ARGS
    kinds = [C.c_void_p if "*" in a else C.c_int for a in decl]
    assert _lib.SIGNATURES["gmpc_ensemble_disagreement"] == (C.c_int, kinds)
    # the existing mode struct and its enums are as they were
    assert re.search(r"enum\s*{\s*GMPC_ENS_FIXED\s*=\s*0\s*,\s*GMPC_ENS_TS1\s*=\s*1\s*}", header)
    assert "typedef struct { int aggregate; float risk; int propagation; int particles; } gmpc_ensemble_mode;" in header


class _Lib:
    def __init__(self):
        self.calls = []

    def gmpc_set_sampled_disagreement(self, *args):
        self.calls.append(("set",) + args)
        return 0

    def gmpc_ensemble_disagreement(self, *args):
        self.calls.append(("plan",) + args)
        return 0


def _engine(n=5, m=2, T=8, dyn_count=10):
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.dyn_count, eng.n, eng.m, eng.T, eng.device = _Lib(), "ctx", dyn_count, n, m, T, "cpu"
    eng._disagreement = None
    eng._stream = lambda: "stream"
    eng.to_dev = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    eng.new = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)
    return eng


def test_h1_the_engine_passes_the_arguments_in_the_headers_order(monkeypatch):
    import gan_mpc_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "_ptr", lambda t: t)
    eng = _engine()
    eng.set_sampled_disagreement(128)
    eng.set_sampled_disagreement(-0.5)
    eng.set_sampled_disagreement(0.0)
    assert eng._disagreement == 0.0
    eng.set_sampled_disagreement(None)
    assert eng._disagreement is None
    assert eng.lib.calls == [("set", "ctx", 1, 128.0), ("set", "ctx", 1, -0.5), ("set", "ctx", 1, 0.0),
                             ("set", "ctx", 0, 0.0)]
    eng.lib.calls.clear()
    z = torch.zeros
    mem, x0, U = z(3, 10), z(4, 5), z(4, 8, 2)
    out = eng.ensemble_disagreement(mem, x0, U)
    assert list(out) == ["d", "D"] and tuple(out["d"].shape) == (3, 4, 8) and tuple(out["D"].shape) == (3, 4)
    (call,) = eng.lib.calls
    assert call[:5] == ("plan", "ctx", 4, 8, 3) and call[11] == "stream"
    assert call[6] is x0 and call[7] is U and call[8] is None and call[9] is out["d"] and call[10] is out["D"]
    short = eng.ensemble_disagreement(mem, x0, U[:, :3].contiguous(), want="X")      # S from U, a lone key as a string
    assert tuple(short["X"].shape) == (4, 4, 5) and eng.lib.calls[1][3] == 3
    assert eng.lib.calls[1][8] is short["X"] and eng.lib.calls[1][9] is None and eng.lib.calls[1][10] is None


def test_h1_the_engine_refuses_before_the_library_is_called():
    eng = _engine()
    for bad in (float("inf"), float("nan"), -float("inf"), 1e39, "1", True, [1.0], np.array([1.0, 2.0])):
        with pytest.raises(GmpcError, match="^disagreement: "):
            eng.set_sampled_disagreement(bad)
    assert eng._disagreement is None
    z = torch.zeros
    good = dict(members=z(3, 10), x0=z(4, 5), U=z(4, 8, 2))
    cases = [
        (dict(members=z(3, 11)), "members must be"),
        (dict(members=z(17, 10)), "P = 17"),
        (dict(members=z(0, 10)), "P = 0"),
        (dict(members=z(3, 10, dtype=torch.float64)), "float32"),
        (dict(want=("d", "spread")), "unknown entries"),
        (dict(want=()), "want is empty"),
        (dict(x0=z(4, 6)), "x0 must be"),
        (dict(x0=z(4, 5, dtype=torch.float64)), "x0 must be a float32 tensor"),
        (dict(U=z(3, 8, 2)), "U must be"),
        (dict(U=z(4, 8, 3)), "U must be"),
        (dict(U=np.zeros((4, 8, 2), np.float32)), "U must be a float32 tensor"),
    ]
    for change, msg in cases:
        with pytest.raises(GmpcError, match="ensemble disagreement: .*" + re.escape(msg)):
            eng.ensemble_disagreement(**dict(good, **change))
    assert eng.lib.calls == []


def test_h1_the_policies_refuse_in_the_constructor():
    from gan_mpc_amd.gan import js_policy
    from gan_mpc_amd.norm import l2_policy
    from gan_mpc_amd.policy import base, eval as eval_policy
    tree = {"params": {"Dense_0": {"kernel": np.zeros((7, 5), np.float32), "bias": np.zeros(5, np.float32)}}}
    sampled = dict(solver="icem", control_bounds=(-1.0, 1.0))
    for cls, lead in ((eval_policy.EvalMPC, (None,) * 4), (base.BaseMPC, (None,) * 4), (l2_policy.L2MPC, (None,) * 4),
                      (js_policy.JS_MPC, (None,) * 5)):
        with pytest.raises(ValueError, match="ensemble_disagreement needs a dynamics_ensemble"):
            cls(*lead, ensemble_disagreement=1.0, **sampled)
        with pytest.raises(ValueError, match="ensemble_disagreement and solver"):
            cls(*lead, ensemble_disagreement=1.0)                      # the default solver, "rounds"
        with pytest.raises(ValueError, match='propagation "ts1"'):
            cls(*lead, ensemble_disagreement=1.0, dynamics_ensemble=[tree],
                ensemble_mode=dict(propagation="ts1", particles=2), **sampled)
        for bad in (float("nan"), float("inf"), "1", True):
            with pytest.raises(ValueError, match="ensemble_disagreement must be"):
                cls(*lead, ensemble_disagreement=bad, dynamics_ensemble=[tree], **sampled)
        pol = cls(*lead, ensemble_disagreement=-2, dynamics_ensemble=[tree], ensemble_mode=dict(aggregate="max"),
                  **sampled)
        assert pol.ensemble_disagreement == -2.0 and pol._engine is None
        with pytest.raises(ValueError, match="ts1"):
            pol.set_ensemble_mode(propagation="ts1", particles=2)
        assert pol.ensemble_mode == dict(aggregate="max")
        assert cls(*lead, dynamics_ensemble=[tree], **sampled).ensemble_disagreement is None


def test_h1_plan_disagreement_raises_the_policys_error_without_an_ensemble():
    from gan_mpc_amd.policy.base import BaseMPC
    policy = BaseMPC.__new__(BaseMPC)
    policy.dynamics_ensemble = None
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        policy.plan_disagreement(None, np.zeros((2, 5), np.float32), np.zeros((2, 8, 2), np.float32))
    policy.dynamics_ensemble = np.zeros((2, 10), np.float32)
    with pytest.raises(ValueError, match="plan_disagreement: x must be"):
        policy.plan_disagreement(None, np.zeros(5, np.float32), np.zeros((2, 8, 2), np.float32))


# ---- H2 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _samples(name):
    """Iteration 0's samples of the plain fp32 and fp64 reference runs."""
    _, t32, _, t64 = cc.traces(name, 1)
    return t32[0]["samples"], t64[0]["samples"]


@pytest.mark.parametrize("name", dc.NAMES)
def test_h2_members_equal_to_the_nominal_layers_and_penalty_zero_cost_the_nominal_model(name):
    pb = dc.problem(name)
    u32, _ = _samples(name)
    J = cr.sample_costs(pb, u32)
    assert J.dtype == np.float32
    same = [pb["dyn"]] * 3
    D = dr.sample_D(pb, same, u32)
    assert D.shape == (3,) + J.shape and not D.any()                         # exactly zero, not merely small
    got = dr.sample_costs(pb, same, u32, dc.PENALTY[name], "max")
    np.testing.assert_array_equal(got.view(np.uint32), J.view(np.uint32))
    got = dr.sample_costs(pb, dc.members(name), u32, 0.0, "max")
    np.testing.assert_array_equal(got.view(np.uint32), J.view(np.uint32))
    real = dr.sample_costs(pb, dc.members(name), u32, dc.PENALTY[name], "max")
    assert np.all(real > J)


@pytest.mark.parametrize("name", ["base", "ragged"])
def test_h2_the_reference_is_the_plain_loop(name):
    pb = orc.cast_problem(dc.problem(name), np.float64)
    members = dc.members(name)

    def mlp(layers, q):
        for W, b in layers[:-1]:
            q = np.maximum(q @ W.astype(np.float64) + b.astype(np.float64), 0.0)
        W, b = layers[-1]
        return q @ W.astype(np.float64) + b.astype(np.float64)

    B, T, _ = pb["U"].shape
    d = np.zeros((len(members), B, T))
    X = np.zeros((B, T + 1, pb["x0"].shape[1]))
    for b in range(B):
        x = pb["x0"][b]
        for t in range(T):
            X[b, t] = x
            q = np.concatenate([x, pb["U"][b, t]])
            o0 = mlp(pb["dyn"], q)
            for p, layers in enumerate(members):
                d[p, b, t] = np.sum((mlp(layers, q) - o0) ** 2)
            x = x + o0
        X[b, T] = x
    r64 = dr.plan(pb["dyn"], members, pb["x0"], pb["U"])
    r32 = dr.plan(dc.problem(name)["dyn"], members, dc.problem(name)["x0"], dc.problem(name)["U"])
    assert r32["d"].dtype == np.float32 and r64["D"].dtype == np.float64
    np.testing.assert_allclose(r64["X"], X, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(r64["d"], d, rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(r64["D"], d.sum(-1), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(r32["d"], d, rtol=1e-3, atol=1e-8)
    np.testing.assert_array_equal(r64["X"], orc.rollout(pb["dyn"], pb["U"], pb["x0"]))
    short = dr.plan(pb["dyn"], members, pb["x0"], pb["U"][:, :3])
    np.testing.assert_array_equal(short["d"], r64["d"][:, :, :3])
    assert d.min() > 0 and np.abs(d[0] - d[1]).max() > 1e-3 * d.max()        # the members differ


# ---- H3 ------------------------------------------------------------------------------------------------------------
def test_h3_what_the_penalties_give():
    changed = 0
    lo, hi, dlo, dhi, clo, chi = np.inf, 0.0, np.inf, 0.0, np.inf, 0.0
    for name in dc.NAMES:
        pb64 = orc.cast_problem(dc.problem(name), np.float64)
        (n, m, T, B, N, E), _ = dc.CASES[name]
        u = _samples(name)[1]
        J = cr.sample_costs(pb64, u)
        D = dr.sample_D(pb64, dc.members(name), u)
        pen = dc.PENALTY[name]
        assert np.log2(pen) == int(np.log2(pen))
        ratio = pen * D.mean(0) / J
        case = pen * D.mean() / J.mean()
        c = dr.sample_costs(pb64, dc.members(name), u, pen, "mean")
        ch = sum(set(a) != set(b) for a, b in zip(cr.elites_of(c, E), cr.elites_of(J, E)))
        print(f"H3 {name}: penalty {pen:g}: penalty mean_p D / J {ratio.min():.3g} .. {ratio.max():.3g} per sample, "
              f"{case:.3g} of the means; D {D.min():.3g} .. {D.max():.3g}; elite sets changed {ch} of {B}")
        lo, hi = min(lo, ratio.min()), max(hi, ratio.max())
        dlo, dhi = min(dlo, D.min()), max(dhi, D.max())
        clo, chi = min(clo, case), max(chi, case)
        if name in dc.DECIDED:
            changed += ch
    print(f"H3: ratio {lo:.3g} .. {hi:.3g}, of the means {clo:.3g} .. {chi:.3g}, D {dlo:.3g} .. {dhi:.3g}, elite sets "
          f"changed {changed} of 24")
    assert 0.01 < lo and hi < 1.1             # the penalty term is neither noise nor the whole cost
    assert 0.1 < clo and chi < 0.6
    assert 1e-3 < dlo and dhi < 1.0
    assert changed == 21


# ---- H4 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_traces(name, aggregate):
    """The fp32 and the fp64 reference run of three CEM iterations under the case's penalty."""
    pb = dc.problem(name)
    t32, t64 = [], []
    args = (dc.members(name), dc.PENALTY[name], aggregate)
    r32 = dr.cem(pb, *args, np.float32, dc.LO, dc.HI, cc.kwargs(name, 3), trace=t32)
    r64 = dr.cem(pb, *args, np.float64, dc.LO, dc.HI, cc.kwargs(name, 3), trace=t64)
    return r32, t32, r64, t64


# measured with this reference: the problems decided through the third iteration
DECIDED_COUNTS = dict(mean=dict(base=3, m1=7, cheetah=5, wide_m=2, wide_n=1, ragged=3),
                      max=dict(base=3, m1=7, cheetah=7, wide_m=2, wide_n=2, ragged=3))


@pytest.mark.parametrize("aggregate", ["mean", "max"])
def test_h4_the_decided_protocol(aggregate):
    total = 0
    for name in dc.DECIDED:
        E = dc.CASES[name][0][5]
        _, t32, _, t64 = ref_traces(name, aggregate)
        ok = cr.decided(t32, t64, E, margin=1e-5)
        print(f"H4 {aggregate} {name}: decided per iteration {ok.sum(1).tolist()} of {ok.shape[1]}")
        assert int(ok[2].sum()) == DECIDED_COUNTS[aggregate][name]
        total += int(ok[2].sum())
    print(f"H4 {aggregate}: {total} of 24 decided through the third iteration")
    assert total >= dc.DECIDED_MIN[aggregate]
