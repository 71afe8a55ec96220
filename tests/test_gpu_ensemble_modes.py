"""The ensemble modes of the sampling solvers on the GPU (gmpc_set_sampled_ensemble_mode): the
risk-sensitive aggregates over the members' costs and the TS1 propagation, in which a particle draws its member anew
at every step.  Most groups need no tolerance: modes that cannot change a cost change nothing (M1), the aggregates of
three one-member runs' costs are NumPy's bit for bit (M2), the samples and the nominal X / obj never see the mode (M3),
one call equals chained calls (M6), a row's cost depends on neither B nor N (M7).  Then the costs against the fp64
restatement (M4), three free-running CEM iterations on the decided problems (M5), the context's state (M8), the
refusals (M9) and the policy (M10).  Tolerance-based comparisons go through gpu_util.assert_parity at its defaults; the
bf16 comparison of M4 takes its bound from sampled_bf16_cases.

Achieved on MI355X (the tests print them; DESIGN.md section 26 lists every case): M2 no cost differs from NumPy's
aggregate in any of the 72 comparisons (the correctly rounded root: no 1-ulp allowance is needed); M4 max-norm error
against fp64 1.0e-7 .. 3.2e-7 for HIP and 9.6e-8 .. 3.0e-7 for the NumPy fp32 restatement, the mean mode's costs more
than 100 x further away; the bf16 TS1 kernel 5.1e-4 / 4.8e-7 / 4.9e-4 from its restatement (m1 / w256 / wide_n), allowed 5.4e-3 / 1.0e-3 / 1.6e-3; M5 after three
iterations mean and std 6.1e-8 .. 2.8e-7 for HIP, 1.0e-7 .. 3.6e-7 for NumPy fp32, on 21 / 21 / 24 decided problems."""

import functools

import numpy as np
import pytest
import torch

import cem_cases as cc
import cem_ref as cr
import ensemble_modes_cases as mc
import ensemble_modes_ref as mr
import gan_mpc_oracle as orc
import gpu_util as gu
import sampled_bf16_cases as sc
from gan_mpc_amd import _lib
from gan_mpc_amd._lib import GmpcError
from test_gpu_sampled_ensemble import _bits, _engine, _members, _np, _raw, _same, _solve

pytestmark = pytest.mark.gpu

GRID = [(s, n, p) for s in mc.SOLVERS for n in mc.BITWISE for p in mc.PRECISIONS]
TS1Q4 = mc.MODES["ts1q4"]


def _mode(eng, mode=None):
    eng.set_sampled_ensemble_mode(**(mode or {}))


# ---- M1 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _identity_runs(solver, name, prec):
    """Two iterations on one engine: without an ensemble; on the three members with the entry point never called,
    with the default mode set explicitly and with MEAN_STD at risk 0; and under modes that cannot move a cost."""
    eng = _engine(name, prec)
    run = lambda: _solve(eng, solver, name, 2)
    try:
        out = dict(none=run())
        eng.set_sampled_ensemble(_members(eng, name))
        out["never"] = run()
        _mode(eng)
        out["default"] = run()
        _mode(eng, dict(aggregate="mean_std", risk=0.0))
        out["risk0"] = run()
        for count in (1, 2):
            eng.set_sampled_ensemble(eng.to_dev(mc.nominal_flat(name, count)))
            for key in ("std+1", "max"):
                _mode(eng, mc.MODES[key])
                out[f"{key} x{count}"] = run()
        eng.set_sampled_ensemble(eng.to_dev(mc.nominal_flat(name, 3)))
        for key, mode in (("ts1 q1", mc.MODES["ts1q1"]), ("ts1 q2", dict(propagation="ts1", particles=2)),
                          ("ts1 q4 max", mc.MODES["ts1q4max"])):
            _mode(eng, mode)
            out[key] = run()
        torch.cuda.synchronize()
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("solver,name,prec", GRID)
def test_m1_the_default_mode_and_risk_zero_are_the_mean(solver, name, prec):
    r = _identity_runs(solver, name, prec)
    assert np.all(np.isfinite(r["never"]["costs"])) and not np.array_equal(r["never"]["costs"], r["none"]["costs"])
    _same(r["never"], r["default"], what=f"M1 default {solver} {name} {prec}")
    _same(r["never"], r["risk0"], what=f"M1 risk 0 {solver} {name} {prec}")


@pytest.mark.parametrize("solver,name,prec", GRID)
def test_m1_modes_on_copies_of_the_bound_dynamics_change_nothing(solver, name, prec):
    r = _identity_runs(solver, name, prec)
    assert np.all(np.isfinite(r["none"]["costs"])) and np.unique(r["none"]["costs"]).size > r["none"]["costs"].shape[0]
    for key in ("std+1 x1", "max x1", "std+1 x2", "max x2", "ts1 q1", "ts1 q2", "ts1 q4 max"):
        _same(r["none"], r[key], what=f"M1 {key} {solver} {name} {prec}")


# ---- M2, M3 --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_iteration(solver, name, prec):
    """One iteration on the three members under every mode setting and under each member alone (the default mode);
    for iCEM behind a first iteration, so that the pool holds fresh rows, kept rows and the mean row."""
    eng = _engine(name, prec)
    try:
        more = {}
        if solver == "icem":
            first = _raw(eng, solver, name, 1, add_mean=False)
            more = dict(U=first["mean"], std=first["std"], state=first["state"], iter_offset=1)
        plain = _raw(eng, solver, name, 1, **more)
        out = dict(plain=_np(plain), modes={}, nominal={}, single=[])
        for p in range(mc.MEMBERS):
            eng.set_sampled_ensemble(_members(eng, name, (p,)))
            out["single"].append(_solve(eng, solver, name, 1, **more))
        eng.set_sampled_ensemble(_members(eng, name))
        for key, mode in mc.MODES.items():
            _mode(eng, mode)
            raw = _raw(eng, solver, name, 1, **more)
            out["modes"][key] = _np(raw)
            eng.set_sampled_ensemble(None)
            out["nominal"][key] = _solve(eng, solver, name, 0, U=raw["U"], want=())
            eng.set_sampled_ensemble(_members(eng, name))
        torch.cuda.synchronize()
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("solver,name,prec", GRID)
def test_m2_fixed_aggregates_are_numpy_s_of_the_three_one_member_runs(solver, name, prec):
    r = _one_iteration(solver, name, prec)
    J = [s["costs"] for s in r["single"]]
    assert not np.array_equal(J[0], J[1]) and not np.array_equal(J[1], J[2]) and not np.array_equal(J[0], J[2])
    if solver == "icem":
        assert J[0].shape[1] == r["single"][0]["samples"].shape[1] + mc.NUM_KEEP[name] + 1
    for key in ("std+1", "std-0.5", "max"):
        mode = mr.full(mc.MODES[key])
        want = mr.aggregate(J, mode["aggregate"], mode["risk"])
        got = r["modes"][key]["costs"]
        assert want.dtype == np.float32 and want.shape == got.shape
        diff = np.nonzero(_bits(got) != _bits(want))
        print(f"M2 {solver} {name} {prec} {key}: {diff[0].size} of {want.size} costs differ from NumPy's")
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"M2 {key}")
        assert not np.array_equal(got, mr.aggregate(J))          # ... and it is not the mean


@pytest.mark.parametrize("solver,name,prec", GRID)
def test_m3_samples_and_the_nominal_rollout_never_see_the_mode(solver, name, prec):
    r = _one_iteration(solver, name, prec)
    for key in mc.MODES:
        got = r["modes"][key]
        _same(got, r["plain"], ["samples"], f"M3 {solver} {name} {prec} {key}")
        _same(got, r["nominal"][key], ["X", "obj"], f"M3 {solver} {name} {prec} {key}")
        assert not np.array_equal(got["costs"], r["plain"]["costs"])


# ---- M4 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cem_costs(name, prec="fp32"):
    """One CEM iteration on the three members under every mode setting: {mode: outputs}."""
    eng = _engine(name, prec)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        out = {}
        for key, mode in mc.MODES.items():
            _mode(eng, mode)
            out[key] = _solve(eng, "cem", name, 1)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("key", mc.MODE_NAMES)
@pytest.mark.parametrize("name", mc.NAMES)
def test_m4_costs_at_the_gpu_samples_against_the_fp64_restatement(name, key):
    pb = mc.problem(name)
    pb64 = orc.cast_problem(pb, np.float64)
    got = _cem_costs(name)[key]
    mode = mc.MODES[key]
    c32 = mr.sample_costs(pb, mc.members(name), got["samples"], mode, cc.CEM_SEED, 0)
    c64 = mr.sample_costs(pb64, mc.members(name), got["samples"].astype(np.float64), mode, cc.CEM_SEED, 0)
    assert c32.dtype == np.float32 and c64.dtype == np.float64
    e = gu.assert_parity(f"ensemble mode {key} costs {name}", got["costs"], c32, c64)
    mean = mr.sample_costs(pb64, mc.members(name), got["samples"].astype(np.float64))
    other = mr.sample_costs(pb64, mc.members(name), got["samples"].astype(np.float64), mode, cc.CEM_SEED, 1)
    print(f"M4 {name} {key}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}; mean-mode costs {gu.rel_err(mean, c64):.3e}, "
          f"iteration 1's schedule {gu.rel_err(other, c64):.3e}")
    assert gu.rel_err(mean, c64) > 100 * max(e[0], 1e-6)         # the mean mode's costs would not pass
    T = got["samples"].shape[2]
    if mr.full(mode)["propagation"] == "ts1" and not np.array_equal(
            mr.schedule(cc.CEM_SEED, 0, mode["particles"], T, mc.MEMBERS),
            mr.schedule(cc.CEM_SEED, 1, mode["particles"], T, mc.MEMBERS)):
        assert gu.rel_err(other, c64) > 100 * max(e[0], 1e-6)    # ... nor another iteration's schedule


# sampled_bf16_cases' names of the cases its cost rule is calibrated on (cheetah is left out there: its rows flip states)
BF16_CASES = {"m1": "B", "w256": "D", "wide_n": "E"}


@pytest.mark.parametrize("name", list(BF16_CASES))
def test_m4_bf16_costs_under_ts1_against_the_fp32_mode(name):
    """TS1 Q 4 / MEAN in bf16 mode under sampled_bf16_cases' cost rule, as test_gpu_sampled_bf16's G2 applies it: the
    kernel within R_CAP * E_q of the bf16 restatement (ensemble_modes_ref.particle_costs_bf16, the member switched per
    step), E_q = max |restatement - fp64 costs| being what bf16 costs, and more than that away from the fp32-mode costs
    of the same samples."""
    assert sc.CASES[BF16_CASES[name]] == mc.CASES[name]
    pb = mc.problem(name)
    g32, g16 = _cem_costs(name)["ts1q4"], _cem_costs(name, "bf16")["ts1q4"]
    _same(g32, g16, ["samples"], f"M4 bf16 {name}")
    u = g32["samples"]
    sched = mr.schedule(cc.CEM_SEED, 0, 4, u.shape[2], mc.MEMBERS)
    ref16 = mr.aggregate([mr.particle_costs_bf16(pb, mc.members(name), u, sched[q]) for q in range(4)])
    c64 = mr.sample_costs(orc.cast_problem(pb, np.float64), mc.members(name), u.astype(np.float64), TS1Q4, cc.CEM_SEED, 0)
    eq = float(np.max(np.abs(ref16 - c64)))
    moved = float(np.max(np.abs(g16["costs"].astype(np.float64) - g32["costs"])))
    err = float(np.max(np.abs(g16["costs"].astype(np.float64) - ref16)))
    print(f"M4 bf16 {name}: |gpu - bf16 restatement| {err:.3e}, allowed {sc.R_CAP * eq:.3e} (E_q {eq:.3e}); "
          f"|bf16 - fp32 mode| {moved:.3e}")
    assert np.all(np.isfinite(g16["costs"]))
    assert err <= sc.R_CAP * eq
    assert moved > sc.R_CAP * eq, "the costs are those of the fp32 mode: the bf16 kernel did not run"


# ---- M5 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cem_chain(name, key, prec="fp32"):
    """Three members under the mode: three chained CEM calls of one iteration and the whole solve of three."""
    eng = _engine(name, prec)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        _mode(eng, mc.MODES[key])
        links, mean, std = [], None, "case"
        for i in range(3):
            out = _raw(eng, "cem", name, 1, U=mean, std=std, iter_offset=i)
            links.append(_np(out))
            mean, std = out["U"], out["std"]
        whole = _solve(eng, "cem", name, 3)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return links, whole


@functools.lru_cache(maxsize=None)
def _ref_traces(name, key):
    pb = mc.problem(name)
    t32, t64 = [], []
    r32 = mr.cem(pb, mc.members(name), mc.MODES[key], np.float32, cc.LO, cc.HI, cc.kwargs(name, 3), trace=t32)
    r64 = mr.cem(pb, mc.members(name), mc.MODES[key], np.float64, cc.LO, cc.HI, cc.kwargs(name, 3), trace=t64)
    return r32, t32, r64, t64


@pytest.mark.parametrize("key", list(mc.DECIDED_MODES))
@pytest.mark.parametrize("name", mc.DECIDED)
def test_m5_three_free_running_iterations_on_the_decided_problems(name, key):
    (n, m, T, B, N, E), _ = mc.CASES[name]
    links, whole = _cem_chain(name, key)
    r32, t32, r64, t64 = _ref_traces(name, key)
    ok = cr.decided(t32, t64, E, margin=1e-5)[2]
    print(f"M5 {name} {key}: decided {int(ok.sum())} of {B}")
    assert ok.any()
    for i in range(3):
        for b in np.nonzero(ok)[0]:
            assert set(links[i]["elites"][b]) == set(t64[i]["elites"][b]), (name, key, i, b)
    e = gu.assert_parity(f"ensemble mode {key} cem mean after 3 {name}", whole["U"][ok], r32["U"][ok], r64["U"][ok])
    f = gu.assert_parity(f"ensemble mode {key} cem std after 3 {name}", whole["std"][ok], r32["std"][ok], r64["std"][ok])
    print(f"M5 {name} {key}: mean HIP {e[0]:.3e} / fp32 {e[1]:.3e}, std HIP {f[0]:.3e} / fp32 {f[1]:.3e}")


def test_m5_the_decided_counts_are_the_host_test_s():
    for key, need in mc.DECIDED_MODES.items():
        count = 0
        for name in mc.DECIDED:
            E = mc.CASES[name][0][5]
            _, t32, _, t64 = _ref_traces(name, key)
            count += int(cr.decided(t32, t64, E, margin=1e-5)[2].sum())
        assert count >= need, (key, count)


# ---- M6 ------------------------------------------------------------------------------------------------------------
CHAIN = [(n, p) for n in mc.BITWISE for p in mc.PRECISIONS]


@pytest.mark.parametrize("name,prec", CHAIN)
def test_m6_one_cem_call_is_the_chain_of_single_iterations(name, prec):
    links, whole = _cem_chain(name, "ts1q4", prec)
    _same(whole, links[2], what=f"M6 cem {name} {prec}")
    # the schedule follows the iteration: iteration 2's costs are those of iteration 2's schedule at its samples, not
    # those of iteration 0's (bf16 mode: against the bf16 restatement, the right schedule is the closer one)
    pb = mc.problem(name)
    u = links[2]["samples"]
    if prec == "fp32":
        at2 = mr.sample_costs(pb, mc.members(name), u, TS1Q4, cc.CEM_SEED, 2)
        at0 = mr.sample_costs(pb, mc.members(name), u, TS1Q4, cc.CEM_SEED, 0)
        assert gu.rel_err(links[2]["costs"], at2) < 1e-5 and gu.rel_err(links[2]["costs"], at0) > 1e-4
    else:
        at = {}
        for it in (0, 2):
            sched = mr.schedule(cc.CEM_SEED, it, 4, u.shape[2], mc.MEMBERS)
            at[it] = mr.aggregate([mr.particle_costs_bf16(pb, mc.members(name), u, sched[q]) for q in range(4)])
        e2, e0 = gu.rel_err(links[2]["costs"], at[2]), gu.rel_err(links[2]["costs"], at[0])
        print(f"M6 cem {name} bf16: iteration 2's costs against the bf16 restatement under schedule 2 {e2:.3e}, 0 {e0:.3e}")
        assert e2 < e0


@pytest.mark.parametrize("name,prec", CHAIN)
def test_m6_one_mppi_call_is_the_chain_of_single_iterations(name, prec):
    eng = _engine(name, prec)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        _mode(eng, TS1Q4)
        mean = None
        for i in range(3):
            out = _raw(eng, "mppi", name, 1, U=mean, iter_offset=i)
            mean = out["U"]
        whole = _solve(eng, "mppi", name, 3)
        last = _np(out)
    finally:
        eng.close()
    _same(whole, last, what=f"M6 mppi {name} {prec}")


@pytest.mark.parametrize("name,prec", CHAIN)
def test_m6_one_icem_call_is_the_chain_of_single_iterations(name, prec):
    eng = _engine(name, prec)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        _mode(eng, TS1Q4)
        mean, std, state = None, "case", None
        for i in range(3):
            out = _raw(eng, "icem", name, 1, U=mean, std=std, state=state, iter_offset=i, add_mean=i == 2)
            mean, std, state = out["mean"], out["std"], out["state"]
        whole = _solve(eng, "icem", name, 3)
        last = _np(out)
    finally:
        eng.close()
    _same(whole, last, what=f"M6 icem {name} {prec}")


# ---- M7 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", mc.PRECISIONS)
def test_m7_a_row_s_cost_depends_on_neither_b_nor_n(prec):
    name = "base"
    pb = mc.problem(name)
    (n, m, T, B, N, E), extra = mc.CASES[name]
    pb7 = gu.problem(n, m, T, 7, seed=cc.PROBLEM_SEED, bias_scale=0.1, **extra)
    for k in ("dyn", "cmlp", "mpc_w"):
        pb7[k] = pb[k]
    for k in ("x0", "U", "goal"):
        pb7[k][:3] = pb[k]
    eng = _engine(name, prec, max_batch=7)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        _mode(eng, dict(aggregate="mean_std", risk=1.0, propagation="ts1", particles=4))
        base = _solve(eng, "cem", name, 1)
        more = _solve(eng, "cem", name, 1, num_samples=72, elite_portion=4.5 / 72)
        wide = _solve(eng, "cem", name, 1, pb=pb7)
        again = _solve(eng, "cem", name, 1)
        _mode(eng, TS1Q4)
        mean = _solve(eng, "cem", name, 1)
    finally:
        eng.close()
    assert base["costs"].shape == (3, 40) and more["costs"].shape == (3, 72) and wide["costs"].shape == (7, 40)
    _same(base, again, what="M7 again")
    np.testing.assert_array_equal(more["samples"][:, :40], base["samples"])
    np.testing.assert_array_equal(_bits(more["costs"][:, :40]), _bits(base["costs"]))
    np.testing.assert_array_equal(_bits(wide["costs"][:3]), _bits(base["costs"]))
    assert np.all(np.isfinite(wide["costs"])) and np.all(np.isfinite(more["costs"]))
    assert np.all(base["costs"] >= mean["costs"]) and not np.array_equal(base["costs"], mean["costs"])


# ---- M8 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", mc.PRECISIONS)
def test_m8_the_mode_survives_new_members_and_set_params(prec):
    name = "ragged"
    eng = _engine(name, prec)
    fresh = _engine(name, prec)
    try:
        _mode(eng, mc.MODES["max"])                               # before any ensemble is set
        eng.set_sampled_ensemble(_members(eng, name))
        first = _solve(eng, "cem", name, 1)
        eng.set_params(*eng._bound)
        kept = _solve(eng, "cem", name, 1)
        eng.set_sampled_ensemble(_members(eng, name, (0, 0, 2)))
        new = _solve(eng, "cem", name, 1)
        fresh.set_sampled_ensemble(_members(fresh, name, (0, 0, 2)))
        mean = _solve(fresh, "cem", name, 1)
        _mode(fresh, mc.MODES["max"])
        want = _solve(fresh, "cem", name, 1)
    finally:
        eng.close()
        fresh.close()
    _same(first, kept, what="M8 set_params")
    _same(new, want, what="M8 new members")
    assert not np.array_equal(new["costs"], first["costs"]) and not np.array_equal(new["costs"], mean["costs"])


@pytest.mark.parametrize("solver", mc.SOLVERS)
def test_m8_the_mode_without_an_ensemble_changes_nothing_and_clearing_returns(solver):
    name = "base"
    eng = _engine(name)
    try:
        before = _solve(eng, solver, name, 2)
        _mode(eng, dict(aggregate="mean_std", risk=1.0, propagation="ts1", particles=4))
        inert = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(_members(eng, name))
        during = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(None)
        after = _solve(eng, solver, name, 2)
    finally:
        eng.close()
    _same(before, inert, what=f"M8 inert {solver}")
    _same(before, after, what=f"M8 cleared {solver}")
    assert not np.array_equal(before["costs"], during["costs"])


def test_m8_a_held_solution_survives_a_solve_under_a_mode():
    name = "base"
    pb = mc.problem(name)
    B = pb["B"]

    def tail(with_cem):
        eng = _engine(name)
        try:
            d = eng.to_dev
            x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
            sol = eng.ilqr_solve(x0, U, goal, {"maxiter": 3})
            if with_cem:
                eng.set_sampled_ensemble(_members(eng, name))
                _mode(eng, mc.MODES["ts1q4max"])
                cem = _solve(eng, "cem", name, 2)
                assert np.all(np.isfinite(cem["costs"]))
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return _np(sol), loss.cpu().numpy(), grad.cpu().numpy()
        finally:
            eng.close()

    s0, l0, g0 = tail(False)
    s1, l1, g1 = tail(True)
    _same(s0, s1, what="M8 held")
    np.testing.assert_array_equal(_bits(l0), _bits(l1))
    np.testing.assert_array_equal(_bits(g0), _bits(g1))


@pytest.mark.parametrize("prec", mc.PRECISIONS)
def test_m8_a_nan_member_poisons_as_the_reference_says(prec):
    name = "w256"                                     # T = 2: a particle misses the NaN member in 4 of 9 draws
    (n, m, T, B, N, E), _ = mc.CASES[name]
    layers = [list(mb) for mb in mc.members(name)]
    W, b = layers[1][-1]
    b = b.copy()
    b[0] = np.nan                                     # one member's output bias
    layers[1][-1] = (W, b)
    pb = mc.problem(name)
    eng = _engine(name, prec)
    seen = set()
    try:
        eng.set_sampled_ensemble(eng.to_dev(mc.flat(layers)))
        for key in ("max", "std+1"):
            _mode(eng, mc.MODES[key])
            for solver in ("cem", "mppi"):
                assert np.isnan(_solve(eng, solver, name, 1)["costs"]).all(), (key, solver)
        # TS1: a particle is poisoned from the first step it draws member 1 at.  The schedule is shared by every row,
        # so a plane is NaN in all rows or in none, and with it the cost
        for Q, kind in ((1, "mean"), (2, "max"), (4, "mean_std")):
            mode = dict(aggregate=kind, propagation="ts1", particles=Q)
            _mode(eng, mode)
            # Iterations 5 and 12: one and two particles never draw member 1.  The iterations are those at which member
            # 1 is drawn at step 0 or not at all: drawn at the last step only, the NaN reaches x_T alone, and the relu of
            # the terminal cost MLP (fmaxf, in every form of the rollout kernel, with or without an ensemble) returns 0
            # for it where NumPy's maximum returns the NaN -- a difference of the rollout itself, not of the modes
            for it in (0, 5, 12):
                got = _solve(eng, "cem", name, 1, iter_offset=it)
                sched = mr.schedule(cc.CEM_SEED, it, Q, T, mc.MEMBERS)
                assert bool((sched[:, :T - 1] == 1).any()) == bool((sched == 1).any()), (
                    f"Q {Q} it {it}: the NaN member is drawn at the last step only, where the rollout's relu drops "
                    f"the NaN (see above): choose another iteration for this seed and case")
                want = np.isnan(mr.sample_costs(pb, layers, got["samples"], mode, cc.CEM_SEED, it))
                assert want.all() or not want.any()
                assert bool(want.all()) == bool((mr.schedule(cc.CEM_SEED, it, Q, T, mc.MEMBERS) == 1).any())
                np.testing.assert_array_equal(np.isnan(got["costs"]), want, err_msg=f"Q {Q} it {it}")
                seen.add(bool(want.all()))
    finally:
        eng.close()
    assert seen == {False, True}                      # both outcomes occurred: the mask follows the schedule


# ---- M9 ------------------------------------------------------------------------------------------------------------
def test_m9_refused_modes_at_the_c_abi_leave_the_mode_as_it_was():
    name = "m1"
    eng = _engine(name)
    M = _lib.EnsembleMode
    import ctypes as C
    try:
        lib = eng.lib
        eng.set_sampled_ensemble(_members(eng, name))
        assert lib.gmpc_set_sampled_ensemble_mode(eng.ctx, C.byref(M(2, 0.0, 1, 4))) == 0
        on = _solve(eng, "cem", name, 1)
        bad = [M(3, 0.0, 0, 0), M(-1, 0.0, 0, 0), M(0, 0.0, 2, 0), M(0, 0.0, -1, 0), M(1, float("nan"), 0, 0),
               M(1, float("inf"), 0, 0), M(0, 1.0, 0, 0), M(2, -0.5, 0, 0), M(0, 0.0, 0, 4), M(1, 1.0, 0, 1),
               M(0, 0.0, 1, 0), M(0, 0.0, 1, 17), M(0, 0.0, 1, -1)]
        for mode in bad:
            assert lib.gmpc_set_sampled_ensemble_mode(eng.ctx, C.byref(mode)) == -1, tuple(
                getattr(mode, f) for f, _ in M._fields_)
            assert lib.gmpc_last_error().startswith(b"ensemble mode: "), lib.gmpc_last_error()
        for ctx, mode in ((None, C.byref(M(0, 0.0, 0, 0))), (eng.ctx, None)):
            assert lib.gmpc_set_sampled_ensemble_mode(ctx, mode) == -1
            assert lib.gmpc_last_error().startswith(b"ensemble mode: ")
        still = _solve(eng, "cem", name, 1)
        assert lib.gmpc_set_sampled_ensemble_mode(eng.ctx, C.byref(M(0, 0.0, 0, 0))) == 0
        mean = _solve(eng, "cem", name, 1)
    finally:
        eng.close()
    _same(on, still, what="M9 unchanged")
    assert not np.array_equal(on["costs"], mean["costs"])


@pytest.mark.parametrize("key", ["max", "ts1q4"])
def test_m9_the_vjp_stays_refused_with_an_ensemble_under_any_mode(key):
    name = "base"
    pb = mc.problem(name)
    (n, m, T, B, N, E), _ = mc.CASES[name]
    eng = gu.engine_for(pb, max_batch=max(B, N), critic=False)
    try:
        d = eng.to_dev
        x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
        kw = mc.engine_kwargs("mppi", name, 1)
        sol = eng.mppi_solve(x0, U, goal, mc.LO, mc.HI, kw, init_std=0.5, trace=True)
        _mode(eng, mc.MODES[key])
        eng.set_sampled_ensemble(_members(eng, name))
        with pytest.raises(GmpcError, match="mppi"):
            eng.mppi_vjp(x0, goal, mc.LO, mc.HI, sol, gU=torch.ones_like(U), kwargs=kw)
        eng.set_sampled_ensemble(None)
        out = eng.mppi_vjp(x0, goal, mc.LO, mc.HI, sol, gU=torch.ones_like(U), kwargs=kw)      # the mode alone: accepted
        assert bool(torch.isfinite(out["U"]).all())
    finally:
        eng.close()


# ---- M10 -----------------------------------------------------------------------------------------------------------
def test_m10_an_icem_policy_on_the_worst_member():
    import copy

    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    bound = 0.3
    kw = dict(num_samples=64, max_iter=3, seed=7)
    build = lambda **more: mirror._build(functools.partial(
        l2_policy.L2MPC, solver="icem", control_bounds=(-bound, bound), icem_kwargs=kw, **more), N=17, M=6)
    config, _, params, data = build()
    rng = np.random.default_rng(3)
    trees = []
    for p in range(3):                       # the nominal network's kernels, each entry moved by a few per cent
        tree = copy.deepcopy(params["dynamics_params"])
        for layer in tree["params"].values():
            layer["kernel"] = (np.asarray(layer["kernel"]) * rng.uniform(0.9, 1.1, np.shape(layer["kernel"]))
                               ).astype(np.float32)
        trees.append(tree)
    _, mean_pol, params1, _ = build(dynamics_ensemble=trees)
    _, policy, params2, _ = build(dynamics_ensemble=trees, ensemble_mode=dict(aggregate="max"))
    assert policy.ensemble_mode == dict(aggregate="max") and mean_pol.ensemble_mode is None
    for pol in (mean_pol, policy):
        pol.expert_model.select(np.array([2]))
    a0 = mean_pol.get_optimal_action(params1, data["hist"][2]).cpu().numpy()
    a1 = policy.get_optimal_action(params2, data["hist"][2]).cpu().numpy()
    assert policy._engine._ensemble_mode["aggregate"] == "max" and policy._engine._ensemble is not None
    assert mean_pol._engine._ensemble_mode is None
    assert a1.shape == (6,) and np.all(np.isfinite(a1)) and np.all(np.abs(a1) <= np.float32(bound))
    c0 = mean_pol._icem_state["best_cost"].cpu().numpy()
    c1 = policy._icem_state["best_cost"].cpu().numpy()
    assert np.all(np.isfinite(c1)) and not np.array_equal(c0, c1)      # the first solve's costs are the worst member's
    assert a0.shape == a1.shape
    a2 = policy.get_optimal_action(params2, data["hist"][2]).cpu().numpy()
    assert np.all(np.abs(a2) <= np.float32(bound))
    assert policy.icem_solves == 2           # the seed advances by one per solve
    with pytest.raises(GmpcError, match="ensemble mode: "):       # refused by the engine: the policy keeps its mode
        policy.set_ensemble_mode(risk=1.0)
    assert policy.ensemble_mode == dict(aggregate="max") and policy._engine._ensemble_mode["aggregate"] == "max"
    policy.set_ensemble_mode(propagation="ts1", particles=4)
    assert policy._engine._ensemble_mode["propagation"] == "ts1"
    a3 = policy.get_optimal_action(params2, data["hist"][2]).cpu().numpy()
    assert np.all(np.isfinite(a3)) and np.all(np.abs(a3) <= np.float32(bound)) and policy.icem_solves == 3
    with pytest.raises(ValueError, match="ensemble_mode"):
        l2_policy.L2MPC(config, None, None, None, solver="rounds", ensemble_mode=dict(aggregate="max"))
