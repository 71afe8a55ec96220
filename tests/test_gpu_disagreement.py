"""The one-step ensemble disagreement of the sampling solvers on the GPU (gmpc_set_sampled_disagreement /
gmpc_ensemble_disagreement).  Most groups need no tolerance: members equal to the bound dynamics
(D1) or a zero penalty (D2) give the solve without an ensemble; a plane's cost is NumPy's J + penalty * D of the plain
solve's costs and the plan call's D, bit for bit (D3: the product rounded before it is added, fp32 mode -- the plan call
is fp32); one call equals chained calls (D7); a row depends on neither B, N nor P (D8).  Then the plan call against the
fp64 reference and against gmpc_predict (D4), the costs against the fp64 and the bf16 restatement (D5), three
free-running CEM iterations on the decided problems (D6), the context's state (D9), a NaN member (D10), the refusals
(D11) and the policy (D12).  Tolerance-based comparisons go through gpu_util.assert_parity at its defaults.

Achieved on MI355X (the tests print them; DESIGN.md section 28 lists them): D3 no cost differs from NumPy's in any of
the 24 comparisons; D4 max-norm error against fp64 X 1.3e-7 .. 4.8e-7, d 1.4e-6 .. 9.4e-6, D 1.0e-6 .. 5.8e-6 (NumPy
fp32: 1.2e-7 .. 3.4e-7, 1.4e-6 .. 6.4e-6, 1.0e-6 .. 4.8e-6), d against squared differences of gmpc_predict outputs
2.2e-6 .. 9.3e-6 (allowed 1.6e-4 .. 4.6e-4); D5 costs 2.1e-7 .. 2.8e-6 (NumPy fp32 2.1e-7 .. 2.7e-6), the nominal
costs 0.24 .. 0.70 away; bf16 2.4e-2 / 1.9e-5 / 4.0e-4 from its restatement (m1 / w256 / wide_n), allowed 1.6e-1 /
3.1e-2 / 6.5e-2; D6 after three iterations mean 5.0e-8 .. 2.2e-7 and std 6.9e-8 .. 2.6e-7 on 21 (mean) and 24 (max)
decided problems."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cem_cases as cc
import cem_ref as cr
import disagreement_cases as dc
import disagreement_ref as dr
import ensemble_modes_ref as mr
import gan_mpc_oracle as orc
import gpu_util as gu
import sampled_bf16_cases as sc
from gan_mpc_amd._lib import GmpcError
from test_gpu_sampled_ensemble import _bits, _engine, _members, _np, _raw, _same, _solve

pytestmark = pytest.mark.gpu

GRID = [(s, n, p) for s in dc.SOLVERS for n in dc.BITWISE for p in dc.PRECISIONS]
# max |next_x| / max |o^p - o^0| over iteration 0's samples, from the fp64 reference (test_d4 prints it at its inputs):
# what a difference of two gmpc_predict outputs loses to cancellation
CANCELLATION = dict(base=46.2, m1=18.9, cheetah=29.6, wide_m=22.6, wide_n=24.7, ragged=25.3, w256=16.3)


def _mode(eng, aggregate):
    eng.set_sampled_ensemble_mode(aggregate=aggregate)


# ---- D1, D2 --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _identity_runs(solver, name, prec):
    """Two iterations on one engine: without an ensemble; three copies of the bound dynamics under the case's penalty;
    the real members under penalty 0; the real members under the penalty.  Aggregate max."""
    eng = _engine(name, prec)
    run = lambda: _solve(eng, solver, name, 2)
    try:
        out = dict(none=run())
        _mode(eng, "max")
        eng.set_sampled_disagreement(dc.PENALTY[name])
        eng.set_sampled_ensemble(eng.to_dev(dc.nominal_flat(name, 3)))
        out["copies"] = run()
        eng.set_sampled_ensemble(_members(eng, name))
        out["real"] = run()
        eng.set_sampled_disagreement(0.0)
        out["zero"] = run()
        torch.cuda.synchronize()
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("solver,name,prec", GRID)
def test_d1_members_equal_to_the_bound_dynamics_change_nothing(solver, name, prec):
    r = _identity_runs(solver, name, prec)
    assert np.all(np.isfinite(r["none"]["costs"])) and np.unique(r["none"]["costs"]).size > r["none"]["costs"].shape[0]
    _same(r["none"], r["copies"], what=f"D1 {solver} {name} {prec}")


@pytest.mark.parametrize("solver,name,prec", GRID)
def test_d2_a_zero_penalty_changes_nothing(solver, name, prec):
    r = _identity_runs(solver, name, prec)
    _same(r["none"], r["zero"], what=f"D2 {solver} {name} {prec}")
    assert np.all(np.isfinite(r["real"]["costs"])) and not np.array_equal(r["real"]["costs"], r["none"]["costs"])
    assert r["real"]["costs"].shape == r["none"]["costs"].shape


# ---- D3 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_iteration(solver, name):
    """fp32 mode, one iteration: without an ensemble, under the penalty with aggregate max and mean, and the plan
    call's D on the pool's rows; for iCEM behind a first iteration, so that the pool holds fresh rows, kept rows and
    the mean row."""
    (n, m, T, B, N, E), _ = dc.CASES[name]
    rows_max = N + dc.NUM_KEEP[name] + 1
    eng = _engine(name, "fp32", max_batch=B * rows_max)
    try:
        more, first = {}, None
        if solver == "icem":
            first = _raw(eng, solver, name, 1, add_mean=False)
            more = dict(U=first["mean"], std=first["std"], state=first["state"], iter_offset=1)
        plain = _solve(eng, solver, name, 1, **more)
        eng.set_sampled_ensemble(_members(eng, name))
        eng.set_sampled_disagreement(dc.PENALTY[name])
        out = dict(plain=plain)
        for agg in ("max", "mean"):
            _mode(eng, agg)
            out[agg] = _solve(eng, solver, name, 1, **more)
        # the pool's controls, row by row: the fresh rows, then iCEM's kept rows and the clamped mean
        pool = [torch.as_tensor(plain["samples"], device=eng.device)]
        if solver == "icem":
            pool.append(first["state"]["keep"])
            pool.append(first["mean"].clamp(dc.LO, dc.HI)[:, None])
        pool = torch.cat(pool, dim=1).contiguous()
        R = pool.shape[1]
        x0 = eng.to_dev(np.repeat(dc.problem(name)["x0"], R, axis=0))
        plan = eng.ensemble_disagreement(_members(eng, name), x0, pool.reshape(B * R, T, m))
        out["D"] = plan["D"].cpu().numpy().reshape(dc.MEMBERS, B, R)
        out["d"] = plan["d"].cpu().numpy().reshape(dc.MEMBERS, B, R, T)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("name", dc.BITWISE)
@pytest.mark.parametrize("solver", dc.SOLVERS)
def test_d3_a_plane_is_the_plain_cost_plus_penalty_times_the_plan_calls_d(solver, name):
    (n, m, T, B, N, E), _ = dc.CASES[name]
    r = _one_iteration(solver, name)
    J, D, pen = r["plain"]["costs"], r["D"], np.float32(dc.PENALTY[name])
    assert J.dtype == np.float32 and D.dtype == np.float32 and D.shape == (3,) + J.shape
    if solver == "icem":
        assert J.shape[1] == r["plain"]["samples"].shape[1] + dc.NUM_KEEP[name] + 1      # fresh, kept, the mean row
    assert np.all(np.isfinite(D)) and np.all(D > 0)
    assert not np.array_equal(D[0], D[1]) and not np.array_equal(D[1], D[2])
    # D is the fp32 sum of d, t ascending
    s = np.zeros_like(D)
    for t in range(T):
        s = s + r["d"][..., t]
    np.testing.assert_array_equal(_bits(D), _bits(s))
    planes = [J + pen * D[p] for p in range(3)]                      # NumPy fp32: the product rounded, then the sum
    assert all(p.dtype == np.float32 for p in planes)
    want_max = np.maximum(np.maximum(planes[0], planes[1]), planes[2])
    want_mean = ((planes[0] + planes[1]) + planes[2]) * np.float32(np.float32(1.0) / np.float32(3.0))
    np.testing.assert_array_equal(_bits(want_max), _bits(mr.aggregate(planes, "max")))
    np.testing.assert_array_equal(_bits(want_mean), _bits(mr.aggregate(planes, "mean")))
    for agg, want in (("max", want_max), ("mean", want_mean)):
        got = r[agg]["costs"]
        diff = int(np.count_nonzero(_bits(got) != _bits(want)))
        print(f"D3 {solver} {name} {agg}: {diff} of {want.size} costs differ from NumPy's")
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"D3 {solver} {name} {agg}")
        _same(r[agg], r["plain"], ["samples"], f"D3 {solver} {name} {agg}")
    assert not np.array_equal(r["max"]["costs"], J) and not np.array_equal(r["max"]["costs"], r["mean"]["costs"])


# ---- D4 ------------------------------------------------------------------------------------------------------------
def _plan_inputs(name, per=40):
    """x0 (R, n) and U (R, T, m): the first `per` iteration-0 samples of every problem -- more than one tile of 32
    rows and a partial last one."""
    pb = dc.problem(name)
    u = cc.traces(name, 1)[1][0]["samples"][:, :per].astype(np.float32)
    B, S, T, m = u.shape
    return np.repeat(pb["x0"], S, axis=0), u.reshape(B * S, T, m)


@pytest.mark.parametrize("name", dc.NAMES)
def test_d4_the_plan_call_against_the_fp64_reference_and_against_predict(name):
    pb = dc.problem(name)
    x0, U = _plan_inputs(name)
    R, T, m = U.shape
    members = dc.members(name)
    eng = _engine(name, max_batch=R * T)
    others = [_engine(name, pb=dict(pb, dyn=layers), max_batch=R * T) for layers in members]
    try:
        d_ = eng.to_dev
        got = eng.ensemble_disagreement(_members(eng, name), d_(x0), d_(U), want=("X", "d", "D"))
        Xs = got["X"][:, :-1].reshape(R * T, -1).contiguous()
        Us = d_(U).reshape(R * T, m).contiguous()
        nxt0 = eng.predict(Xs, Us).cpu().numpy().astype(np.float64)
        nxtp = [o.predict(Xs, Us).cpu().numpy().astype(np.float64) for o in others]
        got = {k: v.cpu().numpy() for k, v in got.items()}
    finally:
        eng.close()
        for o in others:
            o.close()
    r32 = dr.plan(pb["dyn"], members, x0, U)
    r64 = dr.plan(pb["dyn"], members, x0.astype(np.float64), U.astype(np.float64))
    assert got["d"].shape == (3, R, T) and got["D"].shape == (3, R) and got["X"].shape == r64["X"].shape
    e = [gu.assert_parity(f"disagreement plan {k} {name}", got[k], r32[k], r64[k]) for k in ("X", "d", "D")]
    factor = float(np.abs(r64["X"][:, 1:]).max() / np.abs(r64["op"] - r64["o0"][None]).max())
    comp = np.stack([np.sum((p - nxt0) ** 2, axis=-1).reshape(R, T) for p in nxtp])
    err = gu.rel_err(got["d"], comp)
    print(f"D4 {name}: X HIP {e[0][0]:.3e} / fp32 {e[0][1]:.3e}, d {e[1][0]:.3e} / {e[1][1]:.3e}, D {e[2][0]:.3e} / "
          f"{e[2][1]:.3e}; d against predict differences {err:.3e}, allowed {gu.TOL * CANCELLATION[name]:.3e} "
          f"(cancellation here {factor:.1f}, recorded {CANCELLATION[name]})")
    assert err <= gu.TOL * CANCELLATION[name]
    assert gu.rel_err(got["d"][0], r64["d"][1]) > 1e-2             # the members' planes are not one another's


# ---- D5 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cem_costs(name, prec="fp32"):
    """One CEM iteration on the three members under the case's penalty: {aggregate: outputs}."""
    eng = _engine(name, prec)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        eng.set_sampled_disagreement(dc.PENALTY[name])
        out = {}
        for agg in ("mean", "max"):
            _mode(eng, agg)
            out[agg] = _solve(eng, "cem", name, 1)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("agg", ["mean", "max"])
@pytest.mark.parametrize("name", dc.NAMES)
def test_d5_costs_at_the_gpu_samples_against_the_fp64_reference(name, agg):
    pb = dc.problem(name)
    pb64 = orc.cast_problem(pb, np.float64)
    got = _cem_costs(name)[agg]
    u = got["samples"]
    c32 = dr.sample_costs(pb, dc.members(name), u, dc.PENALTY[name], agg)
    c64 = dr.sample_costs(pb64, dc.members(name), u.astype(np.float64), dc.PENALTY[name], agg)
    assert c32.dtype == np.float32 and c64.dtype == np.float64
    e = gu.assert_parity(f"disagreement {agg} costs {name}", got["costs"], c32, c64)
    nominal = cr.sample_costs(pb64, u.astype(np.float64))
    print(f"D5 {name} {agg}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}; the nominal costs {gu.rel_err(nominal, c64):.3e}")
    assert gu.rel_err(nominal, c64) > 100 * max(e[0], 1e-6)        # the nominal model's costs would not pass


# sampled_bf16_cases' names of the cases its cost rule is calibrated on (cheetah is left out there: its rows flip states)
BF16_CASES = {"m1": "B", "w256": "D", "wide_n": "E"}


@pytest.mark.parametrize("name", list(BF16_CASES))
def test_d5_bf16_costs_against_the_bf16_restatement(name):
    """Aggregate mean in bf16 mode under sampled_bf16_cases' cost rule: the kernel within R_CAP * E_q of the bf16
    restatement, E_q = max |restatement - fp64 costs|, times the case's ratio (|J| + |penalty| D_q) / |J_q| -- the
    penalty term is a difference of two bf16-mode outputs; with J > 0 and penalty > 0 the ratio is 1."""
    assert sc.CASES[BF16_CASES[name]] == dc.CASES[name]
    pb = dc.problem(name)
    pen = dc.PENALTY[name]
    g32, g16 = _cem_costs(name)["mean"], _cem_costs(name, "bf16")["mean"]
    _same(g32, g16, ["samples"], f"D5 bf16 {name}")
    u = g32["samples"]
    ref16 = dr.sample_costs(pb, dc.members(name), u, pen, "mean", bf16=True)
    pb64 = orc.cast_problem(pb, np.float64)
    c64 = dr.sample_costs(pb64, dc.members(name), u.astype(np.float64), pen, "mean")
    J = cr.sample_costs(pb64, u.astype(np.float64))
    D = dr.sample_D(pb64, dc.members(name), u.astype(np.float64))
    ratio = float(np.max((np.abs(J)[None] + abs(pen) * D) / np.abs(J[None] + pen * D)))
    eq = float(np.max(np.abs(ref16 - c64)))
    moved = float(np.max(np.abs(g16["costs"].astype(np.float64) - g32["costs"])))
    err = float(np.max(np.abs(g16["costs"].astype(np.float64) - ref16)))
    print(f"D5 bf16 {name}: |gpu - bf16 restatement| {err:.3e}, allowed {sc.R_CAP * eq * ratio:.3e} (E_q {eq:.3e}, ratio "
          f"{ratio:.3f}); |bf16 - fp32 mode| {moved:.3e}")
    assert np.all(np.isfinite(g16["costs"])) and abs(ratio - 1.0) < 1e-12
    assert err <= sc.R_CAP * eq * ratio
    assert moved > 0


# ---- D6, D7 --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cem_chain(name, agg, prec="fp32"):
    """Three members under the penalty: three chained CEM calls of one iteration and the whole solve of three."""
    eng = _engine(name, prec)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        eng.set_sampled_disagreement(dc.PENALTY[name])
        _mode(eng, agg)
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


@pytest.mark.parametrize("agg", ["mean", "max"])
@pytest.mark.parametrize("name", dc.DECIDED)
def test_d6_three_free_running_iterations_on_the_decided_problems(name, agg):
    from test_disagreement_host import ref_traces
    (n, m, T, B, N, E), _ = dc.CASES[name]
    links, whole = _cem_chain(name, agg)
    r32, t32, r64, t64 = ref_traces(name, agg)
    ok = cr.decided(t32, t64, E, margin=1e-5)[2]
    print(f"D6 {name} {agg}: decided {int(ok.sum())} of {B}")
    assert ok.any()
    for i in range(3):
        for b in np.nonzero(ok)[0]:
            assert set(links[i]["elites"][b]) == set(t64[i]["elites"][b]), (name, agg, i, b)
    e = gu.assert_parity(f"disagreement {agg} cem mean after 3 {name}", whole["U"][ok], r32["U"][ok], r64["U"][ok])
    f = gu.assert_parity(f"disagreement {agg} cem std after 3 {name}", whole["std"][ok], r32["std"][ok], r64["std"][ok])
    print(f"D6 {name} {agg}: mean HIP {e[0]:.3e} / fp32 {e[1]:.3e}, std HIP {f[0]:.3e} / fp32 {f[1]:.3e}")


CHAIN = [(n, p) for n in dc.BITWISE for p in dc.PRECISIONS]


@pytest.mark.parametrize("name,prec", CHAIN)
def test_d7_one_cem_call_is_the_chain_of_single_iterations(name, prec):
    links, whole = _cem_chain(name, "mean", prec)
    _same(whole, links[2], what=f"D7 cem {name} {prec}")


def _with_penalty(name, prec):
    eng = _engine(name, prec)
    eng.set_sampled_ensemble(_members(eng, name))
    eng.set_sampled_disagreement(dc.PENALTY[name])
    _mode(eng, "max")
    return eng


@pytest.mark.parametrize("name,prec", CHAIN)
def test_d7_one_mppi_call_is_the_chain_of_single_iterations(name, prec):
    eng = _with_penalty(name, prec)
    try:
        mean = None
        for i in range(3):
            out = _raw(eng, "mppi", name, 1, U=mean, iter_offset=i)
            mean = out["U"]
        whole = _solve(eng, "mppi", name, 3)
        last = _np(out)
    finally:
        eng.close()
    _same(whole, last, what=f"D7 mppi {name} {prec}")


@pytest.mark.parametrize("name,prec", CHAIN)
def test_d7_one_icem_call_is_the_chain_of_single_iterations(name, prec):
    eng = _with_penalty(name, prec)
    try:
        mean, std, state = None, "case", None
        for i in range(3):
            out = _raw(eng, "icem", name, 1, U=mean, std=std, state=state, iter_offset=i, add_mean=i == 2)
            mean, std, state = out["mean"], out["std"], out["state"]
        whole = _solve(eng, "icem", name, 3)
        last = _np(out)
    finally:
        eng.close()
    _same(whole, last, what=f"D7 icem {name} {prec}")


# ---- D8 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", dc.PRECISIONS)
def test_d8_a_row_s_cost_depends_on_neither_b_nor_n(prec):
    name = "base"
    pb = dc.problem(name)
    (n, m, T, B, N, E), extra = dc.CASES[name]
    pb7 = gu.problem(n, m, T, 7, seed=cc.PROBLEM_SEED, bias_scale=0.1, **extra)
    for k in ("dyn", "cmlp", "mpc_w"):
        pb7[k] = pb[k]
    for k in ("x0", "U", "goal"):
        pb7[k][:3] = pb[k]
    eng = _engine(name, prec, max_batch=7)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        eng.set_sampled_disagreement(dc.PENALTY[name])
        base = _solve(eng, "cem", name, 1)
        more = _solve(eng, "cem", name, 1, num_samples=72, elite_portion=4.5 / 72)
        wide = _solve(eng, "cem", name, 1, pb=pb7)
        again = _solve(eng, "cem", name, 1)
    finally:
        eng.close()
    assert base["costs"].shape == (3, 40) and more["costs"].shape == (3, 72) and wide["costs"].shape == (7, 40)
    _same(base, again, what="D8 again")
    np.testing.assert_array_equal(more["samples"][:, :40], base["samples"])
    np.testing.assert_array_equal(_bits(more["costs"][:, :40]), _bits(base["costs"]))
    np.testing.assert_array_equal(_bits(wide["costs"][:3]), _bits(base["costs"]))
    assert np.all(np.isfinite(wide["costs"])) and np.all(np.isfinite(more["costs"]))


def test_d8_the_plan_call_depends_on_neither_p_nor_the_batch():
    name = "base"
    x0, U = _plan_inputs(name)
    R = x0.shape[0]
    eng = _engine(name, max_batch=R)
    try:
        d_ = eng.to_dev
        three = _np(eng.ensemble_disagreement(_members(eng, name), d_(x0), d_(U), want=("X", "d", "D")))
        one = _np(eng.ensemble_disagreement(_members(eng, name, (1,)), d_(x0), d_(U), want=("X", "d", "D")))
        part = _np(eng.ensemble_disagreement(_members(eng, name), d_(x0[35:]), d_(U[35:]), want=("X", "d", "D")))
        short = _np(eng.ensemble_disagreement(_members(eng, name), d_(x0), d_(U[:, :3]), want=("X", "d")))
    finally:
        eng.close()
    for k in ("d", "D"):
        np.testing.assert_array_equal(_bits(one[k][0]), _bits(three[k][1]), err_msg=f"D8 P {k}")
        np.testing.assert_array_equal(_bits(part[k]), _bits(three[k][:, 35:]), err_msg=f"D8 batch {k}")
    np.testing.assert_array_equal(_bits(one["X"]), _bits(three["X"]))
    np.testing.assert_array_equal(_bits(part["X"]), _bits(three["X"][35:]))
    np.testing.assert_array_equal(_bits(short["d"]), _bits(three["d"][:, :, :3]))
    np.testing.assert_array_equal(_bits(short["X"]), _bits(three["X"][:, :4]))


# ---- D9 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", dc.SOLVERS)
def test_d9_the_setting_is_the_contexts_and_inert_without_an_ensemble(solver):
    name = "ragged"
    eng = _engine(name)
    fresh = _engine(name)
    try:
        before = _solve(eng, solver, name, 2)
        eng.set_sampled_disagreement(dc.PENALTY[name])                # before any ensemble is set: inert
        inert = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(_members(eng, name))
        on = _solve(eng, solver, name, 2)
        eng.set_params(*eng._bound)
        kept = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(_members(eng, name, (0, 0, 2)))
        new = _solve(eng, solver, name, 2)
        eng.set_sampled_disagreement(None)
        off = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(None)
        after = _solve(eng, solver, name, 2)
        fresh.set_sampled_ensemble(_members(fresh, name, (0, 0, 2)))
        plain_ens = _solve(fresh, solver, name, 2)
        fresh.set_sampled_disagreement(dc.PENALTY[name])
        want_new = _solve(fresh, solver, name, 2)
    finally:
        eng.close()
        fresh.close()
    _same(before, inert, what=f"D9 inert {solver}")
    _same(on, kept, what=f"D9 set_params {solver}")
    _same(new, want_new, what=f"D9 new members {solver}")
    _same(off, plain_ens, what=f"D9 off {solver}")
    _same(before, after, what=f"D9 cleared {solver}")
    assert not np.array_equal(on["costs"], before["costs"]) and not np.array_equal(on["costs"], new["costs"])
    assert not np.array_equal(new["costs"], off["costs"])


def test_d9_a_held_solution_survives_a_solve_under_the_penalty():
    name = "base"
    pb = dc.problem(name)
    B = pb["B"]

    def tail(with_cem):
        eng = _engine(name)
        try:
            d = eng.to_dev
            x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
            sol = eng.ilqr_solve(x0, U, goal, {"maxiter": 3})
            if with_cem:
                eng.set_sampled_ensemble(_members(eng, name))
                eng.set_sampled_disagreement(dc.PENALTY[name])
                cem = _solve(eng, "cem", name, 2)
                assert np.all(np.isfinite(cem["costs"]))
                plan = eng.ensemble_disagreement(_members(eng, name), x0, U)
                assert bool(torch.isfinite(plan["D"]).all())
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return _np(sol), loss.cpu().numpy(), grad.cpu().numpy()
        finally:
            eng.close()

    s0, l0, g0 = tail(False)
    s1, l1, g1 = tail(True)
    _same(s0, s1, what="D9 held")
    np.testing.assert_array_equal(_bits(l0), _bits(l1))
    np.testing.assert_array_equal(_bits(g0), _bits(g1))


# ---- D10 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", dc.PRECISIONS)
def test_d10_a_nan_member_poisons_every_cost_and_only_its_own_plane(prec):
    name = "w256"
    (n, m, T, B, N, E), _ = dc.CASES[name]
    layers = [list(mb) for mb in dc.members(name)]
    W, b = layers[1][-1]
    b = b.copy()
    b[0] = np.nan                                     # member 1's output bias
    layers[1][-1] = (W, b)
    pb = dc.problem(name)
    eng = _engine(name, prec)
    try:
        bad = eng.to_dev(dc.flat(layers))
        eng.set_sampled_ensemble(bad)
        eng.set_sampled_disagreement(dc.PENALTY[name])
        for agg in ("mean", "max"):
            _mode(eng, agg)
            cem = _solve(eng, "cem", name, 1)
            assert np.isnan(cem["costs"]).all(), agg
            np.testing.assert_array_equal(cem["elites"], np.tile(np.arange(E, dtype=np.int32), (B, 1)))
            assert np.all(np.isfinite(cem["U"]))
            mppi = _solve(eng, "mppi", name, 1)
            assert np.isnan(mppi["costs"]).all(), agg
            np.testing.assert_array_equal(_bits(mppi["U"]), _bits(pb["U"]))
        plan = _np(eng.ensemble_disagreement(bad, eng.to_dev(pb["x0"]), eng.to_dev(pb["U"]), want=("X", "d", "D")))
    finally:
        eng.close()
    assert np.isnan(plan["D"][1]).all() and np.isnan(plan["d"][1]).all()
    assert np.all(np.isfinite(plan["D"][[0, 2]])) and np.all(np.isfinite(plan["d"][[0, 2]]))
    assert np.all(np.isfinite(plan["X"]))


# ---- D11 -----------------------------------------------------------------------------------------------------------
def test_d11_refused_settings_at_the_c_abi_leave_the_setting_as_it_was():
    name = "m1"
    eng = _engine(name)
    try:
        lib = eng.lib
        f = C.c_float
        nominal = _solve(eng, "cem", name, 1)
        eng.set_sampled_ensemble(_members(eng, name))
        assert lib.gmpc_set_sampled_disagreement(eng.ctx, 1, f(dc.PENALTY[name])) == 0
        on = _solve(eng, "cem", name, 1)
        for kind, pen in ((2, 1.0), (-1, 1.0), (1, float("inf")), (1, float("nan")), (1, -float("inf")), (0, 1.0),
                          (0, float("nan"))):
            assert lib.gmpc_set_sampled_disagreement(eng.ctx, kind, f(pen)) == -1, (kind, pen)
            assert lib.gmpc_last_error().startswith(b"disagreement: "), lib.gmpc_last_error()
        assert lib.gmpc_set_sampled_disagreement(None, 1, f(1.0)) == -1
        assert lib.gmpc_last_error().startswith(b"disagreement: ")
        still = _solve(eng, "cem", name, 1)
        assert lib.gmpc_set_sampled_disagreement(eng.ctx, 0, f(0.0)) == 0
        off = _solve(eng, "cem", name, 1)
        assert lib.gmpc_set_sampled_disagreement(eng.ctx, 1, f(-dc.PENALTY[name])) == 0       # either sign
        neg = _solve(eng, "cem", name, 1)
    finally:
        eng.close()
    _same(on, still, what="D11 unchanged")
    assert not np.array_equal(on["costs"], off["costs"])
    assert np.all(neg["costs"] < nominal["costs"]) and np.all(on["costs"] > nominal["costs"])


@pytest.mark.parametrize("solver", dc.SOLVERS)
def test_d11_ts1_is_refused_at_solve_time_and_writes_nothing(solver):
    name = "base"
    pb = dc.problem(name)
    eng = _engine(name)
    try:
        plain = _solve(eng, solver, name, 1)
        eng.set_sampled_disagreement(dc.PENALTY[name])
        eng.set_sampled_ensemble_mode(propagation="ts1", particles=2)     # accepted: the order does not matter
        inert = _solve(eng, solver, name, 1)                              # no ensemble: nothing to refuse
        eng.set_sampled_ensemble(_members(eng, name))
        d = eng.to_dev
        U = d(pb["U"])
        before = U.clone()
        with pytest.raises(GmpcError, match="disagreement: not with TS1 propagation"):
            _raw(eng, solver, name, 1, U=U)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(U.cpu().numpy(), before.cpu().numpy())
        eng.set_sampled_disagreement(None)
        ts1 = _solve(eng, solver, name, 1)                                # TS1 alone: accepted again
        eng.set_sampled_disagreement(dc.PENALTY[name])
        eng.set_sampled_ensemble_mode()
        fixed = _solve(eng, solver, name, 1)                              # the penalty under the fixed propagation
    finally:
        eng.close()
    _same(plain, inert, what=f"D11 inert {solver}")
    assert np.all(np.isfinite(ts1["costs"])) and np.all(np.isfinite(fixed["costs"]))
    assert not np.array_equal(ts1["costs"], fixed["costs"])


def test_d11_the_vjp_stays_refused_with_an_ensemble():
    name = "base"
    pb = dc.problem(name)
    (n, m, T, B, N, E), _ = dc.CASES[name]
    eng = gu.engine_for(pb, max_batch=max(B, N), critic=False)
    try:
        d = eng.to_dev
        x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
        kw = dc.engine_kwargs("mppi", name, 1)
        sol = eng.mppi_solve(x0, U, goal, dc.LO, dc.HI, kw, init_std=0.5, trace=True)
        eng.set_sampled_disagreement(dc.PENALTY[name])
        eng.set_sampled_ensemble(_members(eng, name))
        with pytest.raises(GmpcError, match="mppi"):
            eng.mppi_vjp(x0, goal, dc.LO, dc.HI, sol, gU=torch.ones_like(U), kwargs=kw)
        eng.set_sampled_ensemble(None)
        out = eng.mppi_vjp(x0, goal, dc.LO, dc.HI, sol, gU=torch.ones_like(U), kwargs=kw)   # the setting alone: accepted
        assert bool(torch.isfinite(out["U"]).all())
    finally:
        eng.close()


def test_d11_refused_arguments_of_the_plan_call():
    from gan_mpc_amd.engine import Engine
    name = "m1"
    pb = dc.problem(name)
    (n, m, T, B, _, _), _ = dc.CASES[name]
    eng = _engine(name)
    try:
        lib, d = eng.lib, eng.to_dev
        mem, x0, U = _members(eng, name), d(pb["x0"]), d(pb["U"])
        X, dd, D = eng.new(B, T + 1, n), eng.new(3, B, T), eng.new(3, B)
        p = lambda t: None if t is None else t.data_ptr()
        good = dict(ctx=eng.ctx, B=B, S=T, P=3, mem=mem, x0=x0, U=U, X=X, d=dd, D=D)

        def call(**change):
            a = dict(good, **change)
            return lib.gmpc_ensemble_disagreement(a["ctx"], a["B"], a["S"], a["P"], p(a["mem"]), p(a["x0"]), p(a["U"]),
                                                  p(a["X"]), p(a["d"]), p(a["D"]), None)

        assert call() == 0
        assert call(X=None, d=None) == 0 and call(S=1, X=None, D=None) == 0
        for change in (dict(ctx=None), dict(mem=None), dict(x0=None), dict(U=None), dict(B=0), dict(B=B + 1),
                       dict(S=0), dict(S=T + 1), dict(P=0), dict(P=17), dict(X=None, d=None, D=None)):
            assert call(**change) == -1, change
            assert lib.gmpc_last_error().startswith(b"ensemble disagreement: "), (change, lib.gmpc_last_error())
        fresh = Engine(n, m, T, [n + m, 8, n], [n, 8, 2], max_batch=B)       # no parameters set
        try:
            assert lib.gmpc_ensemble_disagreement(fresh.ctx, B, T, 1, p(eng.new(1, fresh.dyn_count)), p(x0), p(U),
                                                  p(X), None, None, None) != 0
            assert lib.gmpc_last_error().startswith(b"ensemble disagreement: "), lib.gmpc_last_error()
            assert b"gmpc_set_params" in lib.gmpc_last_error()
        finally:
            fresh.close()
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300"])
def test_d11_refused_shapes_carry_the_prefix(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        with pytest.raises(GmpcError, match="error -1: disagreement: "):
            eng.set_sampled_disagreement(1.0)
        assert eng._disagreement is None
        with pytest.raises(GmpcError, match="error -1: ensemble disagreement: "):
            eng.ensemble_disagreement(torch.zeros(2, eng.dyn_count, device=eng.device), d(pb["x0"]), d(pb["U"]))
    finally:
        eng.close()


# ---- D12 -----------------------------------------------------------------------------------------------------------
def test_d12_an_icem_policy_under_the_penalty():
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
    _, plain, params1, _ = build(dynamics_ensemble=trees)
    _, policy, params2, _ = build(dynamics_ensemble=trees, ensemble_disagreement=1024.0)
    assert policy.ensemble_disagreement == 1024.0 and plain.ensemble_disagreement is None
    for pol in (plain, policy):
        pol.expert_model.select(np.array([2]))
    a0 = plain.get_optimal_action(params1, data["hist"][2]).cpu().numpy()
    a1 = policy.get_optimal_action(params2, data["hist"][2]).cpu().numpy()
    assert policy._engine._disagreement == 1024.0 and policy._engine._ensemble is not None
    assert plain._engine._disagreement is None
    assert a1.shape == (6,) and np.all(np.isfinite(a1)) and np.all(np.abs(a1) <= np.float32(bound))
    assert a0.shape == a1.shape and not np.array_equal(a0, a1)
    a2 = policy.get_optimal_action(params2, data["hist"][2]).cpu().numpy()
    assert np.all(np.abs(a2) <= np.float32(bound))
    assert policy.icem_solves == 2           # the seed advances by one per solve
    x = data["hist"][2:3, -1]
    U = np.broadcast_to(a1, (1, config.mpc.horizon, 6)).astype(np.float32).copy()
    d, D = policy.plan_disagreement(params2, x, U)
    d, D = d.cpu().numpy(), D.cpu().numpy()
    assert d.shape == (3, 1, config.mpc.horizon) and D.shape == (3, 1)
    assert np.all(np.isfinite(d)) and np.all(d > 0) and np.all(D > 0)
