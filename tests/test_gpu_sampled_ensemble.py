"""The dynamics ensemble of the sampling solvers on the GPU (gmpc_set_sampled_ensemble).  Most
groups need no tolerance, because the combination rule is exact: one member equal to the bound dynamics, or two, change
nothing (E1, E2); one other member gives the costs of an engine bound to it and the nominal X / obj (E3); three members
give ((J_0 + J_1) + J_2) * float32(1 / 3) of their three one-member runs bit for bit (E4: the member strides, the bf16
member images, the reduce).  Then the costs against the fp64 reference's member mean (E5), three free-running CEM
iterations on the decided problems (E6), one call against chained calls (E7), independence from B and N (E8), the
context's state (E9), a NaN member (E10), refusals (E11) and the policy (E12).  Tolerance-based comparisons go through
gpu_util.assert_parity at its defaults.

Achieved on MI355X (the tests print them; DESIGN.md section 24 lists every case): E5 max-norm error against fp64 1.2e-7 ..
2.0e-7 for HIP and 1.2e-7 .. 2.2e-7 for the NumPy fp32 restatement, the nominal model's costs 2e-3 .. 9e-2 away; E6
after three iterations mean 1.0e-7 .. 2.4e-7 and std 1.5e-7 .. 2.9e-7 for HIP, 2.1e-7 .. 3.1e-7 and 1.7e-7 .. 3.7e-7 for
NumPy fp32; 23 of 24 problems decided."""

import functools

import numpy as np
import pytest
import torch

import cem_cases as cc
import cem_ref as cr
import gan_mpc_oracle as orc
import gpu_util as gu
import icem_cases as ic
import sampled_ensemble_cases as ec
import sampled_ensemble_ref as er
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

WANT = dict(cem=("costs", "elites", "samples"), icem=("costs", "elites", "samples"),
            mppi=("costs", "weights", "samples"))
GRID = [(s, n, p) for s in ec.SOLVERS for n in ec.BITWISE for p in ec.PRECISIONS]


def _np(out):
    flat = {}
    for k, v in out.items():
        if isinstance(v, dict):
            flat.update({f"{k}.{kk}": vv.cpu().numpy() for kk, vv in v.items()})
        else:
            flat[k] = v.cpu().numpy()
    return flat


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, keys=None, what=""):
    assert keys is not None or a.keys() == b.keys()
    for k in (a.keys() if keys is None else keys):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what} {k}")


def _raw(eng, solver, name, max_iter, pb=None, B=None, U=None, std="case", want=None, iter_offset=0, state=None,
         **more):
    """One call of the solver on the case, device tensors out."""
    pb = ec.problem(name) if pb is None else pb
    B = pb["B"] if B is None else B
    d = eng.to_dev
    kw = ec.engine_kwargs(solver, name, max_iter, **more)
    std = ec.init_std(solver) if isinstance(std, str) else std
    U = d(pb["U"][:B]) if U is None else U
    args = (d(pb["x0"][:B]), U, d(pb["goal"][:B]), ec.LO, ec.HI, kw)
    opt = dict(init_std=std, want=WANT[solver] if want is None else want, iter_offset=iter_offset)
    if solver == "icem":
        return eng.icem_solve(*args, state=state, **opt)
    return (eng.cem_solve if solver == "cem" else eng.mppi_solve)(*args, **opt)


def _solve(eng, solver, name, max_iter, **more):
    return _np(_raw(eng, solver, name, max_iter, **more))


def _engine(name, prec="fp32", pb=None, **more):
    eng = gu.engine_for(ec.problem(name) if pb is None else pb, critic=False, **more)
    eng.set_sampled_precision(prec)
    return eng


def _members(eng, name, which=(0, 1, 2)):
    """The case's members `which` as one device tensor (P, dyn count)."""
    return eng.to_dev(ec.flat([ec.members(name)[p] for p in which]))


# ---- E1, E2 --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nominal_runs(solver, name, prec):
    """Two iterations without an ensemble, with the bound dynamics as the one member, and as two members."""
    eng = _engine(name, prec)
    try:
        none = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(eng.to_dev(ec.nominal_flat(name, 1)))
        one = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(eng.to_dev(ec.nominal_flat(name, 2)))
        two = _solve(eng, solver, name, 2)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return none, one, two


@pytest.mark.parametrize("solver,name,prec", GRID)
def test_e1_the_bound_dynamics_as_the_one_member_changes_nothing(solver, name, prec):
    none, one, _ = _nominal_runs(solver, name, prec)
    assert np.all(np.isfinite(none["costs"])) and np.unique(none["costs"]).size > none["costs"].shape[0]
    _same(none, one, what=f"E1 {solver} {name} {prec}")


@pytest.mark.parametrize("solver,name,prec", GRID)
def test_e2_two_identical_members_change_nothing(solver, name, prec):
    none, _, two = _nominal_runs(solver, name, prec)
    _same(none, two, what=f"E2 {solver} {name} {prec}")


# ---- E3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name,prec", GRID)
def test_e3_one_other_member_costs_like_an_engine_bound_to_it_and_reports_the_nominal_model(solver, name, prec):
    pb = ec.problem(name)
    eng = _engine(name, prec)
    other = _engine(name, prec, pb=dict(pb, dyn=ec.members(name)[1]))
    try:
        plain = _solve(eng, solver, name, 1)
        eng.set_sampled_ensemble(_members(eng, name, (1,)))
        raw = _raw(eng, solver, name, 1)
        got = _np(raw)
        bound = _solve(other, solver, name, 1)
        # the nominal model's rollout of the returned controls: no iteration, so no sampled row
        eng.set_sampled_ensemble(None)
        nominal = _solve(eng, solver, name, 0, U=raw["U"], want=())
    finally:
        eng.close()
        other.close()
    _same(got, bound, ["costs", "samples"], f"E3 {solver} {name} {prec}")
    assert not np.array_equal(got["costs"], plain["costs"])
    _same(got, plain, ["samples"], f"E3 {solver} {name} {prec}")      # the sampler never sees a cost
    _same(got, nominal, ["X", "obj"], f"E3 {solver} {name} {prec}")
    assert not np.array_equal(got["X"], bound["X"])


# ---- E4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name,prec", GRID)
def test_e4_three_members_cost_the_rule_of_their_three_one_member_runs(solver, name, prec):
    (n, m, T, B, N, E), _ = ec.CASES[name]
    eng = _engine(name, prec)
    try:
        more = {}
        if solver == "icem":
            # a first iteration's kept rows, so that the pool holds fresh rows, kept rows and the mean
            first = _raw(eng, solver, name, 1, add_mean=False)
            more = dict(U=first["mean"], std=first["std"], state=first["state"], iter_offset=1)
        eng.set_sampled_ensemble(_members(eng, name))
        got = _solve(eng, solver, name, 1, **more)
        single = []
        for p in range(ec.MEMBERS):
            eng.set_sampled_ensemble(_members(eng, name, (p,)))
            single.append(_solve(eng, solver, name, 1, **more))
    finally:
        eng.close()
    if solver == "icem":
        assert got["costs"].shape[1] == got["samples"].shape[1] + ec.NUM_KEEP[name] + 1
    else:
        assert got["costs"].shape == (B, N)
    for s in single:
        _same(got, s, ["samples"], f"E4 {solver} {name} {prec}")
    J = [s["costs"] for s in single]
    assert not np.array_equal(J[0], J[1]) and not np.array_equal(J[1], J[2]) and not np.array_equal(J[0], J[2])
    want = ((J[0] + J[1]) + J[2]) * np.float32(np.float32(1.0) / np.float32(3.0))
    assert want.dtype == np.float32
    np.testing.assert_array_equal(_bits(got["costs"]), _bits(want))
    np.testing.assert_array_equal(_bits(want), _bits(er.combine(J)))


# ---- E5, E6, E7 (CEM) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cem_runs(name):
    """fp32 mode, the case's three members: three chained calls of one iteration and the whole solve of three."""
    eng = _engine(name)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
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
def _ref_traces(name):
    pb = ec.problem(name)
    t32, t64 = [], []
    r32 = er.cem(pb, ec.members(name), np.float32, cc.LO, cc.HI, cc.kwargs(name, 3), trace=t32)
    r64 = er.cem(pb, ec.members(name), np.float64, cc.LO, cc.HI, cc.kwargs(name, 3), trace=t64)
    return r32, t32, r64, t64


@pytest.mark.parametrize("name", ec.NAMES)
def test_e5_costs_at_the_gpu_samples_against_the_fp64_member_mean(name):
    pb = ec.problem(name)
    pb64 = orc.cast_problem(pb, np.float64)
    lk = _cem_runs(name)[0][0]
    c32 = er.sample_costs(pb, ec.members(name), lk["samples"])
    c64 = er.sample_costs(pb64, ec.members(name), lk["samples"].astype(np.float64))
    assert c32.dtype == np.float32 and c64.dtype == np.float64
    e = gu.assert_parity(f"ensemble costs {name}", lk["costs"], c32, c64)
    nominal = cr.sample_costs(pb64, lk["samples"].astype(np.float64))
    print(f"E5 {name}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}; nominal costs {gu.rel_err(nominal, c64):.3e}")
    assert gu.rel_err(nominal, c64) > 100 * max(e[0], 1e-6)      # the nominal model's costs would not pass


@pytest.mark.parametrize("name", ec.DECIDED)
def test_e6_three_free_running_iterations_on_the_decided_problems(name):
    (n, m, T, B, N, E), _ = ec.CASES[name]
    links, whole = _cem_runs(name)
    r32, t32, r64, t64 = _ref_traces(name)
    ok = cr.decided(t32, t64, E, margin=1e-5)[2]
    print(f"E6 {name}: decided {int(ok.sum())} of {B}")
    assert ok.sum() >= B - 1
    for i in range(3):
        for b in np.nonzero(ok)[0]:
            assert set(links[i]["elites"][b]) == set(t64[i]["elites"][b]), (name, i, b)
    e = gu.assert_parity(f"ensemble cem mean after 3 {name}", whole["U"][ok], r32["U"][ok], r64["U"][ok])
    f = gu.assert_parity(f"ensemble cem std after 3 {name}", whole["std"][ok], r32["std"][ok], r64["std"][ok])
    print(f"E6 {name}: mean HIP {e[0]:.3e} / fp32 {e[1]:.3e}, std HIP {f[0]:.3e} / fp32 {f[1]:.3e}")


@pytest.mark.parametrize("name", ["base", "cheetah"])
def test_e7_one_cem_call_is_the_chain_of_single_iterations(name):
    links, whole = _cem_runs(name)
    _same(whole, links[2], what=f"E7 cem {name}")


@pytest.mark.parametrize("name", ["base", "cheetah"])
def test_e7_one_mppi_call_is_the_chain_of_single_iterations(name):
    eng = _engine(name)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        mean = None
        for i in range(3):
            out = _raw(eng, "mppi", name, 1, U=mean, iter_offset=i)
            mean = out["U"]
        whole = _solve(eng, "mppi", name, 3)
        last = _np(out)
    finally:
        eng.close()
    _same(whole, last, what=f"E7 mppi {name}")


@pytest.mark.parametrize("name", ["base", "cheetah"])
def test_e7_one_icem_call_is_the_chain_of_single_iterations(name):
    eng = _engine(name)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        mean, std, state = None, "case", None
        for i in range(3):
            out = _raw(eng, "icem", name, 1, U=mean, std=std, state=state, iter_offset=i, add_mean=i == 2)
            mean, std, state = out["mean"], out["std"], out["state"]
        whole = _solve(eng, "icem", name, 3)
        last = _np(out)
    finally:
        eng.close()
    _same(whole, last, what=f"E7 icem {name}")


# ---- E8 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ec.PRECISIONS)
def test_e8_a_row_s_cost_depends_on_neither_b_nor_n(prec):
    name = "base"
    pb = ec.problem(name)
    (n, m, T, B, N, E), extra = ec.CASES[name]
    pb7 = gu.problem(n, m, T, 7, seed=cc.PROBLEM_SEED, bias_scale=0.1, **extra)
    for k in ("dyn", "cmlp", "mpc_w"):
        pb7[k] = pb[k]
    for k in ("x0", "U", "goal"):
        pb7[k][:3] = pb[k]
    eng = _engine(name, prec, max_batch=7)
    try:
        eng.set_sampled_ensemble(_members(eng, name))
        base = _solve(eng, "cem", name, 1)
        more = _solve(eng, "cem", name, 1, num_samples=72, elite_portion=4.5 / 72)
        wide = _solve(eng, "cem", name, 1, pb=pb7)
        again = _solve(eng, "cem", name, 1)
    finally:
        eng.close()
    assert base["costs"].shape == (3, 40) and more["costs"].shape == (3, 72) and wide["costs"].shape == (7, 40)
    _same(base, again, what="E8 again")
    np.testing.assert_array_equal(more["samples"][:, :40], base["samples"])
    np.testing.assert_array_equal(_bits(more["costs"][:, :40]), _bits(base["costs"]))
    np.testing.assert_array_equal(_bits(wide["costs"][:3]), _bits(base["costs"]))
    assert np.all(np.isfinite(wide["costs"])) and np.all(np.isfinite(more["costs"]))


# ---- E9 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ec.SOLVERS)
def test_e9_set_solve_clear_solve(solver):
    name = "base"
    eng = _engine(name)
    try:
        before = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(_members(eng, name))
        during = _solve(eng, solver, name, 2)
        eng.set_sampled_ensemble(None)
        after = _solve(eng, solver, name, 2)
    finally:
        eng.close()
    _same(before, after, what=f"E9 {solver}")
    assert not np.array_equal(before["costs"], during["costs"])


@pytest.mark.parametrize("prec", ec.PRECISIONS)
def test_e9_set_params_keeps_the_ensemble_and_a_second_set_picks_up_new_values(prec):
    name = "ragged"
    eng = _engine(name, prec)
    fresh = _engine(name, prec)
    try:
        mem = _members(eng, name)
        eng.set_sampled_ensemble(mem)
        first = _solve(eng, "cem", name, 1)
        eng.set_params(*eng._bound)
        kept = _solve(eng, "cem", name, 1)
        # member 1 overwritten in place with member 0: unseen by the bf16 images until the entry point is called again
        swapped = ec.flat([ec.members(name)[p] for p in (0, 0, 2)])
        mem.copy_(eng.to_dev(swapped))
        ptr = mem.data_ptr()
        eng.set_sampled_ensemble(mem)
        assert eng._ensemble.data_ptr() == ptr
        new = _solve(eng, "cem", name, 1)
        fresh.set_sampled_ensemble(fresh.to_dev(swapped))
        want = _solve(fresh, "cem", name, 1)
    finally:
        eng.close()
        fresh.close()
    _same(first, kept, what="E9 set_params")
    _same(new, want, what="E9 same pointer")
    assert not np.array_equal(new["costs"], first["costs"])


def test_e9_a_held_solution_survives_an_ensemble_solve():
    name = "base"
    pb = ec.problem(name)
    B = pb["B"]

    def tail(with_cem):
        eng = _engine(name)
        try:
            d = eng.to_dev
            x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
            sol = eng.ilqr_solve(x0, U, goal, {"maxiter": 3})
            if with_cem:
                eng.set_sampled_ensemble(_members(eng, name))
                cem = _solve(eng, "cem", name, 2)
                assert np.all(np.isfinite(cem["costs"]))
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return _np(sol), loss.cpu().numpy(), grad.cpu().numpy()
        finally:
            eng.close()

    s0, l0, g0 = tail(False)
    s1, l1, g1 = tail(True)
    _same(s0, s1, what="E9 held")
    np.testing.assert_array_equal(_bits(l0), _bits(l1))
    np.testing.assert_array_equal(_bits(g0), _bits(g1))


# ---- E10 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ec.PRECISIONS)
def test_e10_a_nan_member_poisons_every_cost(prec):
    name = "base"
    (n, m, T, B, N, E), _ = ec.CASES[name]
    layers = [list(mb) for mb in ec.members(name)]
    W, b = layers[1][-1]
    b = b.copy()
    b[0] = np.nan                                     # one member's output bias
    layers[1][-1] = (W, b)
    eng = _engine(name, prec)
    try:
        eng.set_sampled_ensemble(eng.to_dev(ec.flat(layers)))
        cem = _solve(eng, "cem", name, 2)
        U0 = eng.to_dev(ec.problem(name)["U"])
        mppi = _solve(eng, "mppi", name, 2)
    finally:
        eng.close()
    assert np.isnan(cem["costs"]).all() and np.isnan(mppi["costs"]).all()
    np.testing.assert_array_equal(cem["elites"], np.tile(np.arange(E), (B, 1)))
    assert np.isfinite(cem["U"]).all() and np.isfinite(cem["std"]).all()
    np.testing.assert_array_equal(_bits(mppi["U"]), _bits(U0.cpu().numpy()))
    assert np.isfinite(cem["X"]).all() and np.isfinite(mppi["obj"]).all()       # the nominal model's


# ---- E11 -----------------------------------------------------------------------------------------------------------
def test_e11_refused_arguments_at_the_c_abi():
    name = "m1"
    eng = _engine(name)
    try:
        mem = _members(eng, name)
        ptr = mem.data_ptr()
        lib = eng.lib
        for P, p in ((17, ptr), (-1, ptr), (1, None)):
            assert lib.gmpc_set_sampled_ensemble(eng.ctx, P, p) != 0
            assert lib.gmpc_last_error().startswith(b"ensemble: "), lib.gmpc_last_error()
        assert lib.gmpc_set_sampled_ensemble(None, 1, ptr) != 0
        assert lib.gmpc_last_error().startswith(b"ensemble: ")
        assert lib.gmpc_set_sampled_ensemble(eng.ctx, 16, ptr) == 0     # (no device work: nothing is read)
        assert lib.gmpc_set_sampled_ensemble(eng.ctx, 0, None) == 0
        plain = _solve(eng, "cem", name, 1)
        assert lib.gmpc_set_sampled_ensemble(eng.ctx, 3, ptr) == 0
        assert lib.gmpc_set_sampled_ensemble(eng.ctx, 17, ptr) != 0     # a refused call leaves the ensemble as it was
        on = _solve(eng, "cem", name, 1)
        assert lib.gmpc_set_sampled_ensemble(eng.ctx, 0, ptr) == 0      # P = 0 with any pointer clears
        off = _solve(eng, "cem", name, 1)
    finally:
        eng.close()
    _same(plain, off)
    assert not np.array_equal(plain["costs"], on["costs"])


@pytest.mark.parametrize("case", ["lstm", "n300"])
def test_e11_refused_shapes_carry_the_ensemble_prefix(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    eng = gu.engine_for(pb, critic=False)
    try:
        with pytest.raises(GmpcError, match="error -1: ensemble: "):          # (GMPC_EINVAL, the library's message)
            eng.set_sampled_ensemble(torch.zeros(2, eng.dyn_count, device=eng.device))
        d = eng.to_dev
        with pytest.raises(GmpcError, match="cem: "):             # ... and the solvers refuse as before
            eng.cem_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), ec.LO, ec.HI, dict(num_samples=32, max_iter=1))
    finally:
        eng.close()


def test_e11_the_vjp_is_refused_while_an_ensemble_is_set():
    name = "base"
    pb = ec.problem(name)
    (n, m, T, B, N, E), _ = ec.CASES[name]
    eng = gu.engine_for(pb, max_batch=max(B, N), critic=False)
    try:
        d = eng.to_dev
        x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
        kw = ec.engine_kwargs("mppi", name, 1)
        sol = eng.mppi_solve(x0, U, goal, ec.LO, ec.HI, kw, init_std=0.5, trace=True)
        eng.set_sampled_ensemble(_members(eng, name))
        with pytest.raises(GmpcError, match="mppi"):
            eng.mppi_vjp(x0, goal, ec.LO, ec.HI, sol, gU=torch.ones_like(U), kwargs=kw)
        eng.set_sampled_ensemble(None)
        out = eng.mppi_vjp(x0, goal, ec.LO, ec.HI, sol, gU=torch.ones_like(U), kwargs=kw)
        assert bool(torch.isfinite(out["U"]).all())
    finally:
        eng.close()


# ---- E12 -----------------------------------------------------------------------------------------------------------
def test_e12_an_icem_policy_on_an_ensemble():
    import copy

    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    bound = 0.3
    kw = dict(num_samples=64, max_iter=3, seed=7)
    build = lambda **more: mirror._build(functools.partial(
        l2_policy.L2MPC, solver="icem", control_bounds=(-bound, bound), icem_kwargs=kw, **more), N=17, M=6)
    config, plain, params, data = build()
    rng = np.random.default_rng(3)
    trees = []
    for p in range(3):                       # the nominal network's kernels, each entry moved by a few per cent
        tree = copy.deepcopy(params["dynamics_params"])
        for layer in tree["params"].values():
            layer["kernel"] = (np.asarray(layer["kernel"]) * rng.uniform(0.9, 1.1, np.shape(layer["kernel"]))
                               ).astype(np.float32)
        trees.append(tree)
    _, policy, params2, _ = build(dynamics_ensemble=trees)
    assert policy.dynamics_ensemble.shape[0] == 3
    for pol, par in ((plain, params), (policy, params2)):
        pol.expert_model.select(np.array([2]))
    a0 = plain.get_optimal_action(params, data["hist"][2]).cpu().numpy()
    a1 = policy.get_optimal_action(params2, data["hist"][2]).cpu().numpy()
    assert policy._engine._ensemble is not None and tuple(policy._engine._ensemble.shape) == (3, policy._engine.dyn_count)
    assert getattr(plain._engine, "_ensemble", None) is None
    assert a1.shape == (6,) and np.all(np.isfinite(a1)) and np.all(np.abs(a1) <= np.float32(bound))
    assert not np.array_equal(a0, a1)
    a2 = policy.get_optimal_action(params2, data["hist"][2]).cpu().numpy()
    assert np.all(np.abs(a2) <= np.float32(bound))
    assert policy.icem_solves == 2           # the seed advances by one per solve
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        l2_policy.L2MPC(config, None, None, None, solver="rounds", dynamics_ensemble=trees)
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        l2_policy.L2MPC(config, None, None, None, solver="icem", control_bounds=(-bound, bound), dynamics_ensemble=[])
