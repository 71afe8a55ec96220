"""The dynamics ensemble of the sampling solvers without a GPU (gmpc_set_sampled_ensemble): the
entry point's declaration and binding (H1), every Engine and policy refusal, raised before any library call (H2), the
figures sampled_ensemble_cases quotes (H3), the restatement against cem_ref.cem bit for bit where the rule is exact (H4)
and the decided protocol on the ensemble (H5)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import cem_cases as cc
import cem_ref
import gan_mpc_oracle as orc
import sampled_ensemble_cases as ec
import sampled_ensemble_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- H1 ------------------------------------------------------------------------------------------------------------
def test_h1_the_entry_point_is_declared_and_bound():
    from gan_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    assert re.search(r"\bint\s+gmpc_set_sampled_ensemble\s*\(\s*gmpc_ctx\s*\*\s*\w+\s*,\s*int\s+P\s*,"
                     r"\s*const\s+float\s*\*\s*dyn_members\s*\)\s*;", header)
    assert _lib.SIGNATURES["gmpc_set_sampled_ensemble"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p])


class _Lib:
    """Stands in for the library: records the calls of the entry point."""

    def __init__(self):
        self.calls = []

    def gmpc_set_sampled_ensemble(self, ctx, P, ptr):
        self.calls.append((ctx, P, ptr))
        return 0


def _engine(dyn_count=10):
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.dyn_count = _Lib(), "ctx", dyn_count
    return eng


def test_h1_the_engine_passes_ctx_count_pointer_in_that_order():
    eng = _engine()
    eng.set_sampled_ensemble(None)
    assert eng.lib.calls == [("ctx", 0, None)] and eng._ensemble is None
    kept = []
    eng.to_dev = lambda a: kept.append(a) or a
    import gan_mpc_amd.engine as engine_mod
    real = engine_mod._ptr
    engine_mod._ptr = lambda t: ("ptr", id(t))
    try:
        mem = np.zeros((3, 10), np.float32)
        eng.set_sampled_ensemble(mem)
    finally:
        engine_mod._ptr = real
    assert eng.lib.calls[-1] == ("ctx", 3, ("ptr", id(mem)))
    assert eng._ensemble is mem and kept == [mem]          # kept alive on the engine


# ---- H2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.zeros(10, np.float32), np.zeros((1, 2, 10), np.float32), np.zeros((2, 9), np.float32),
                                 np.zeros((0, 10), np.float32), np.zeros((17, 10), np.float32),
                                 np.zeros((2, 10), np.float64), [[0.0] * 10]],
                         ids=["rank1", "rank3", "width", "P0", "P17", "float64", "list"])
def test_h2_the_engine_refuses_before_the_library(bad):
    from gan_mpc_amd._lib import GmpcError
    eng = _engine()
    with pytest.raises(GmpcError, match="^ensemble: "):
        eng.set_sampled_ensemble(bad)
    assert eng.lib.calls == []


def test_h2_the_policy_refusals_and_the_packing():
    from gan_mpc_amd import params as P
    from gan_mpc_amd.gan.js_policy import JS_MPC
    from gan_mpc_amd.norm.l2_policy import L2MPC
    from gan_mpc_amd.policy.base import BaseMPC
    from gan_mpc_amd.policy.eval import EvalMPC
    trees = [P.layers_to_tree(layers) for layers in ec.members("base")]
    for solver in ("rounds", "fused"):
        with pytest.raises(ValueError, match="dynamics_ensemble"):
            EvalMPC(None, None, None, None, solver=solver, dynamics_ensemble=trees)
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        EvalMPC(None, None, None, None, solver="box", control_bounds=(-1.0, 1.0), dynamics_ensemble=trees)
    for solver in ("cem", "mppi", "icem"):
        with pytest.raises(ValueError, match="dynamics_ensemble"):
            EvalMPC(None, None, None, None, solver=solver, control_bounds=(-1.0, 1.0), dynamics_ensemble=[])
        p = EvalMPC(None, None, None, None, solver=solver, control_bounds=(-1.0, 1.0), dynamics_ensemble=trees)
        np.testing.assert_array_equal(p.dynamics_ensemble, ec.flat(ec.members("base")))
    assert EvalMPC(None, None, None, None).dynamics_ensemble is None
    kw = dict(solver="icem", control_bounds=(-1.0, 1.0), dynamics_ensemble=tuple(trees))
    for cls, args in ((BaseMPC, (None,) * 4), (L2MPC, (None,) * 4), (JS_MPC, (None,) * 5)):
        assert cls(*args, **kw).dynamics_ensemble.shape == (3, ec.flat(ec.members("base")).shape[1])


# ---- H3 ------------------------------------------------------------------------------------------------------------
def _iteration0(name):
    """fp64: (nominal costs, [member costs], ensemble costs) at iteration 0's samples of the fp64 run, and E."""
    (n, m, T, B, N, E), _ = ec.CASES[name]
    p = orc.cast_problem(ec.problem(name), np.float64)
    std = np.full(p["U"].shape, (cc.HI - cc.LO) / 2)
    u = cem_ref.draw(p["U"], std, np.full(m, cc.LO), np.full(m, cc.HI), cc.CEM_SEED, 0, N, 0.0, np.float64)
    Js = er.member_costs(p, ec.members(name), u)
    return cem_ref.sample_costs(p, u), Js, er.combine(Js), E


def test_h3_the_ensemble_is_no_copy_of_the_nominal_model():
    changed = total = 0
    for name in ec.NAMES:
        nom, Js, ens, E = _iteration0(name)
        d_nom = float(np.max(np.abs(ens - nom)) / np.max(np.abs(nom)))
        d_mem = float(np.max(np.abs(Js[0] - Js[1])) / np.max(np.abs(nom)))
        diff = sum(set(a) != set(b) for a, b in zip(cem_ref.elites_of(ens, E), cem_ref.elites_of(nom, E)))
        print(f"H3 {name}: |ensemble - nominal| {d_nom:.2e}, |J_0 - J_1| {d_mem:.2e}, elite sets changed {diff} of "
              f"{nom.shape[0]}")
        assert 2e-3 < d_nom < 9e-2 and 9e-3 < d_mem < 1.2e-1
        if name in ec.DECIDED:
            changed += diff
            total += nom.shape[0]
    assert total == 24 and changed == 12


# ---- H4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "ragged"])
@pytest.mark.parametrize("count", [1, 2])
def test_h4_identical_members_restate_cem_bit_for_bit(name, count):
    pb = ec.problem(name)
    kw = cc.kwargs(name, 3)
    t0, t1 = [], []
    ref = cem_ref.cem(pb, np.float32, cc.LO, cc.HI, kw, trace=t0)
    got = er.cem(pb, [pb["dyn"]] * count, np.float32, cc.LO, cc.HI, kw, trace=t1)
    assert cem_ref.sample_costs is er._plain_sample_costs          # the wrapper put it back
    for k in ref:
        np.testing.assert_array_equal(ref[k].view(np.uint32), got[k].view(np.uint32), err_msg=k)
    for a, b in zip(t0, t1):
        assert a["costs"].dtype == np.float32 and b["costs"].dtype == np.float32
        np.testing.assert_array_equal(a["costs"].view(np.uint32), b["costs"].view(np.uint32))
        np.testing.assert_array_equal(a["elites"], b["elites"])


def test_h4_the_rule_is_sequential_and_multiplies_by_the_rounded_inverse():
    rng = np.random.default_rng(0)
    J = [rng.standard_normal(1000).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 3)) for _ in range(3)]
    want = ((J[0] + J[1]) + J[2]) * np.float32(np.float32(1.0) / np.float32(3.0))
    np.testing.assert_array_equal(er.combine(J).view(np.uint32), want.view(np.uint32))
    other = (J[0] + (J[1] + J[2])) / np.float32(3.0)
    assert not np.array_equal(other, want)                 # another order or a division is another number
    J[1][5] = np.nan
    assert np.isnan(er.combine(J)[5]) and np.isfinite(np.delete(er.combine(J), 5)).all()
    assert er.combine([a.astype(np.float64) for a in J]).dtype == np.float64


# ---- H5 ------------------------------------------------------------------------------------------------------------
def test_h5_the_decided_protocol_holds_on_the_ensemble():
    decided = total = 0
    for name in ec.DECIDED:
        (n, m, T, B, N, E), _ = ec.CASES[name]
        pb = ec.problem(name)
        t32, t64 = [], []
        er.cem(pb, ec.members(name), np.float32, cc.LO, cc.HI, cc.kwargs(name, 3), trace=t32)
        er.cem(pb, ec.members(name), np.float64, cc.LO, cc.HI, cc.kwargs(name, 3), trace=t64)
        ok = cem_ref.decided(t32, t64, E, margin=1e-5)[2]
        print(f"H5 {name}: decided through the third iteration {int(ok.sum())} of {B}")
        decided += int(ok.sum())
        total += B
    assert total == 24
    assert decided >= 22, decided
