"""The bf16 mode of the sampled rollouts on the GPU (gmpc_set_sampled_precision) against
tests/sampled_bf16_ref.py: the samples (G1), one iteration's costs under the cost rule of sampled_bf16_cases (G2), the
exact case (G3), independence (G4), a NaN problem (G5), whole solves through the fp32 rollout (G6), stale weights (G7),
switching the mode (G8), refusals (G9) and the policy (G10).

Achieved on MI355X by G2: max |gpu - restatement| / the allowance R_CAP * E_q (and max |bf16 mode - fp32 mode|):
  cem   A 9.5e-07 / 1.06e-02 (2.9e-02)   B 4.1e-04 / 9.96e-03 (2.7e-02)   C5 2.7e-03 / 1.10e-02 (3.0e-02)
        D 4.8e-07 / 1.50e-03 (4.1e-03)   E 4.1e-04 / 3.26e-03 (8.8e-03)
  icem  A 1.9e-06 / 1.04e-02 (2.8e-02)   C3 1.9e-03 / 3.19e-03 (9.0e-03)
  mppi  A 9.5e-07 / 1.02e-02 (2.7e-02)   C3 1.9e-06 / 3.45e-03 (9.3e-03)
(1e-6: no rounding flipped; 4e-4: a hidden unit's; 2e-3 .. 3e-3: a state's, see sampled_bf16_cases.)"""

import functools

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu
import sampled_bf16_cases as sc
import sampled_bf16_ref as sr
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

WANT = dict(cem=("costs", "elites", "samples"), icem=("costs", "elites", "samples"),
            mppi=("costs", "weights", "samples"))
G2 = [(s, n) for s in sc.SOLVERS for n in sc.G2_CASES[s]]
WHOLE = [(s, n) for s in sc.SOLVERS for n in sc.NAMES]


def _np(out):
    flat = {}
    for k, v in out.items():
        if isinstance(v, dict):
            flat.update({f"{k}.{kk}": vv.cpu().numpy() for kk, vv in v.items()})
        else:
            flat[k] = v.cpu().numpy()
    return flat


def _solve(eng, solver, name, max_iter=None, pb=None, B=None, init_std="case", want=None, **more):
    pb = sc.problem(name) if pb is None else pb
    B = pb["B"] if B is None else B
    d = eng.to_dev
    kw = dict(sc.engine_kwargs(solver, name, max_iter), **more)
    std = sc.INIT_STD[solver] if init_std == "case" else init_std
    if solver == "cem" and init_std == "case":
        std = None
    fn = dict(cem=eng.cem_solve, icem=eng.icem_solve, mppi=eng.mppi_solve)[solver]
    return _np(fn(d(pb["x0"][:B]), d(pb["U"][:B]), d(pb["goal"][:B]), sc.LO, sc.HI, kw, init_std=std,
                  want=WANT[solver] if want is None else want))


def _same(a, b, keys=None):
    for k in (a.keys() if keys is None else keys):
        np.testing.assert_array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                      b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k], err_msg=k)


@functools.lru_cache(maxsize=None)
def _runs(solver, name):
    """Per (solver, case), computed once on one engine: one iteration in fp32 mode and in bf16 mode, and the whole
    solve in bf16 mode (CEM 3 iterations, the others their defaults)."""
    eng = gu.engine_for(sc.problem(name), critic=False)
    try:
        one32 = _solve(eng, solver, name, 1)
        eng.set_sampled_precision("bf16")
        one16 = _solve(eng, solver, name, 1)
        whole16 = _solve(eng, solver, name)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return one32, one16, whole16


def _pool(solver, name, out):
    """The rows whose costs `out` holds: the samples, and for iCEM's one iteration the mean's row behind them."""
    s = out["samples"]
    if solver != "icem":
        return s
    mean = np.clip(sc.problem(name)["U"], sc.LO, sc.HI).astype(np.float32)
    return np.concatenate([s, mean[:, None]], axis=1)


# ---- G1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_g1_samples_are_those_of_the_fp32_mode(name):
    one32, one16, _ = _runs("cem", name)
    _same(one32, one16, ["samples"])
    assert np.unique(one16["samples"]).size > 10


# ---- G2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name", G2)
def test_g2_costs_are_the_restatement_s(solver, name):
    one32, one16, _ = _runs(solver, name)
    _same(one32, one16, ["samples"])
    rows = _pool(solver, name, one16)
    assert rows.shape[:2] == one16["costs"].shape
    ref = sr.sample_costs(sc.problem(name), rows)
    eq, _ = sc.figures(solver, name)
    err = float(np.max(np.abs(one16["costs"].astype(np.float64) - ref)))
    moved = float(np.max(np.abs(one16["costs"].astype(np.float64) - one32["costs"])))
    print(f"G2 {solver} {name}: |gpu - ref| {err:.3e}, allowed {sc.R_CAP * eq:.3e} (E_q {eq:.3e}); "
          f"|bf16 - fp32 mode| {moved:.3e}")
    assert np.all(np.isfinite(one16["costs"]))
    assert err <= sc.R_CAP * eq
    assert moved > sc.R_CAP * eq, "the costs are those of the fp32 mode: the bf16 kernel did not run"


# ---- G3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["cem", "icem"])
def test_g3_exact_case_costs_are_bitwise_those_of_the_fp32_mode(solver):
    pb = sc.problem("exact")
    eng = gu.engine_for(pb, critic=False)
    try:
        a = _solve(eng, solver, "exact", 1, init_std=0.0)
        eng.set_sampled_precision("bf16")
        b = _solve(eng, solver, "exact", 1, init_std=0.0)
    finally:
        eng.close()
    assert np.all(np.isfinite(a["costs"])) and np.unique(a["costs"]).size == pb["B"]
    _same(a, b, ["costs", "samples", "elites"])
    # and they are the restatement's, to the fp32 rounding of the stage costs
    ref = sr.sample_costs(pb, _pool(solver, "exact", b))
    assert gu.rel_err(b["costs"], ref) < 1e-6


# ---- G4 ------------------------------------------------------------------------------------------------------------
def test_g4_a_row_s_cost_depends_on_neither_n_nor_b_nor_the_call():
    name = "A"
    pb = sc.problem(name)
    eng = gu.engine_for(pb, max_batch=7, critic=False)
    try:
        eng.set_sampled_precision("bf16")
        base = _solve(eng, "cem", name, 1)
        again = _solve(eng, "cem", name, 1)
        more = _solve(eng, "cem", name, 1, num_samples=72, elite_portion=4.5 / 72)
        pb7 = gu.problem(5, 2, 4, 7, seed=sc.cc.PROBLEM_SEED, bias_scale=0.1, **sc.CASES[name][1])
        for k in ("dyn", "cmlp", "mpc_w"):
            pb7[k] = pb[k]
        for k in ("x0", "U", "goal"):
            pb7[k][:3] = pb[k]
        wide = _solve(eng, "cem", name, 1, pb=pb7)
    finally:
        eng.close()
    _same(base, again)
    np.testing.assert_array_equal(more["samples"][:, :40], base["samples"])
    np.testing.assert_array_equal(more["costs"][:, :40].view(np.uint32), base["costs"].view(np.uint32))
    np.testing.assert_array_equal(wide["costs"][:3].view(np.uint32), base["costs"].view(np.uint32))
    assert wide["costs"].shape == (7, 40)


# ---- G5 ------------------------------------------------------------------------------------------------------------
def test_g5_a_nan_problem_poisons_itself_only():
    name = "A"
    pb = sc.problem(name)
    bad = dict(pb, x0=pb["x0"].copy())
    bad["x0"][1, 2] = np.nan
    eng = gu.engine_for(pb, critic=False)
    try:
        eng.set_sampled_precision("bf16")
        good = _solve(eng, "cem", name, 1)
        out = _solve(eng, "cem", name, 1, pb=bad)
    finally:
        eng.close()
    assert np.all(np.isnan(out["costs"][1]))
    for b in (0, 2):
        np.testing.assert_array_equal(out["costs"][b].view(np.uint32), good["costs"][b].view(np.uint32))
        np.testing.assert_array_equal(out["U"][b].view(np.uint32), good["U"][b].view(np.uint32))
    E = out["elites"].shape[1]
    c = np.where(np.isnan(out["costs"]), np.inf, out["costs"])
    np.testing.assert_array_equal(out["elites"], np.argsort(c, axis=1, kind="stable")[:, :E])


# ---- G6 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,name", WHOLE)
def test_g6_whole_solves_return_the_true_model_s_rollout_and_improve(solver, name):
    pb = sc.problem(name)
    _, _, sol = _runs(solver, name)
    U = sol["U"]
    assert np.all(np.isfinite(U))
    if solver == "icem":     # (the best row is a clamped sample; CEM's and MPPI's means are averages of clamped samples)
        assert U.min() >= sc.LO and U.max() <= sc.HI
    assert U.min() >= sc.LO - 1e-6 and U.max() <= sc.HI + 1e-6
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        Xr, cr = eng.rollout_cost(d(pb["x0"]), d(U), d(pb["goal"]))
        start = eng.rollout_cost(d(pb["x0"]), d(np.clip(pb["U"], sc.LO, sc.HI)), d(pb["goal"]))[1].sum(dim=1)
        Xr, objr, start = Xr.cpu().numpy(), cr.sum(dim=1).cpu().numpy(), start.cpu().numpy()
    finally:
        eng.close()
    pb64 = orc.cast_problem(pb, np.float64)
    U64 = U.astype(np.float64)
    X64 = orc.rollout(pb64["dyn"], U64, pb64["x0"])
    obj64 = np.sum(orc.evaluate(pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X64, U64), axis=1)
    gu.assert_parity(f"bf16 {solver} {name} X", sol["X"], Xr, X64)
    gu.assert_parity(f"bf16 {solver} {name} obj", sol["obj"], objr, obj64)
    print(f"G6 {solver} {name}: start {start}, end {sol['obj']}")
    assert np.all(sol["obj"] < start)


# ---- G7 ------------------------------------------------------------------------------------------------------------
def test_g7_set_params_marks_the_weight_image_stale():
    name = "A"
    pb = sc.problem(name)
    rng = np.random.default_rng(1)
    pb2 = dict(pb, dyn=[((W * rng.uniform(0.8, 1.2, W.shape)).astype(np.float32), b) for W, b in pb["dyn"]],
               cmlp=[((W * rng.uniform(0.8, 1.2, W.shape)).astype(np.float32), b) for W, b in pb["cmlp"]])
    fresh = gu.engine_for(pb2, critic=False)
    try:
        fresh.set_sampled_precision("bf16")
        want = _solve(fresh, "cem", name, pb=pb2)
    finally:
        fresh.close()
    eng = gu.engine_for(pb, critic=False)
    other = gu.engine_for(pb2, critic=False)       # (its bound tensors are pb2's packed parameters)
    try:
        eng.set_sampled_precision("bf16")
        first = _solve(eng, "cem", name)
        eng.set_params(*other._bound)
        eng.set_params(*other._bound)              # twice without a solve in between
        got = _solve(eng, "cem", name, pb=pb2)
    finally:
        eng.close()
        other.close()
    _same(want, got)
    assert not np.array_equal(first["costs"], got["costs"])


# ---- G8 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", sc.SOLVERS)
def test_g8_the_mode_switches_back_and_belongs_to_one_engine(solver):
    name = "A"
    pb = sc.problem(name)
    eng = gu.engine_for(pb, critic=False)
    second = gu.engine_for(pb, critic=False)
    try:
        a = _solve(eng, solver, name)
        eng.set_sampled_precision("bf16")
        b = _solve(eng, solver, name)
        other = _solve(second, solver, name)
        eng.set_sampled_precision("fp32")
        c = _solve(eng, solver, name)
    finally:
        eng.close()
        second.close()
    _same(a, c)
    _same(a, other)
    assert not np.array_equal(a["costs"], b["costs"])


# ---- G9 ------------------------------------------------------------------------------------------------------------
def test_g9_the_vjp_is_refused_in_bf16_mode():
    name = "A"
    pb = sc.problem(name)
    n, m, T, B, N, E = sc.shape(name)
    eng = gu.engine_for(pb, max_batch=max(B, N), critic=False)
    try:
        d = eng.to_dev
        x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
        kw = sc.engine_kwargs("mppi", name, 1)
        sol = eng.mppi_solve(x0, U, goal, sc.LO, sc.HI, kw, init_std=0.5, trace=True)
        eng.set_sampled_precision("bf16")
        before = eng.rollout_cost(x0, U, goal)[0].clone()
        with pytest.raises(GmpcError, match="fp32 sampled rollouts only"):
            eng.mppi_vjp(x0, goal, sc.LO, sc.HI, sol, gU=torch.ones_like(U), kwargs=kw)
        eng.set_sampled_precision("fp32")
        out = eng.mppi_vjp(x0, goal, sc.LO, sc.HI, sol, gU=torch.ones_like(U), kwargs=kw)
        assert bool(torch.isfinite(out["U"]).all())
        assert torch.equal(before, eng.rollout_cost(x0, U, goal)[0])
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300"])
def test_g9_refused_shapes_are_refused_as_in_fp32_mode(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    eng = gu.engine_for(pb, critic=False)
    try:
        eng.set_sampled_precision("bf16")
        d = eng.to_dev
        with pytest.raises(GmpcError, match="cem: "):
            eng.cem_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), sc.LO, sc.HI, dict(num_samples=32, max_iter=1))
    finally:
        eng.close()


def test_g9_precision_2_is_refused_at_the_c_abi():
    eng = gu.engine_for(sc.problem("B"), critic=False)
    try:
        assert eng.lib.gmpc_set_sampled_precision(eng.ctx, 2) != 0
        assert b"sampled precision: " in eng.lib.gmpc_last_error()
        assert eng.lib.gmpc_set_sampled_precision(eng.ctx, -1) != 0
        assert eng.lib.gmpc_set_sampled_precision(eng.ctx, 1) == 0
        assert eng.lib.gmpc_set_sampled_precision(eng.ctx, 0) == 0
    finally:
        eng.close()


# ---- G10 -----------------------------------------------------------------------------------------------------------
def test_g10_a_cem_policy_in_bf16_mode():
    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    bound = 0.3
    kw = dict(num_samples=64, max_iter=4, seed=7)
    build = lambda prec: mirror._build(functools.partial(
        l2_policy.L2MPC, solver="cem", control_bounds=(-bound, bound), cem_kwargs=kw, sampled_precision=prec))
    config, policy, params, data = build("bf16")
    assert policy.sampled_precision == "bf16"
    policy.expert_model.select(np.array([2]))
    out = policy.get_optimal_values(params, data["hist"][2])
    assert len(out) == 7
    X, U, obj, grad, adj, lqr, itr = out
    assert grad is None and adj is None and lqr is None and int(itr) == 4
    assert tuple(U.shape) == (policy._engine.T, policy._engine.m)
    assert tuple(X.shape) == (policy._engine.T + 1, policy._engine.n)
    u = U.cpu().numpy()
    assert np.all(np.isfinite(u)) and u.min() >= -bound and u.max() <= bound
    a = policy.get_optimal_action(params, data["hist"][2]).cpu().numpy()
    assert np.all(np.isfinite(a)) and np.all(np.abs(a) <= bound)
    assert policy.cem_solves == 2           # the seed advances by one per solve
    # the mode reached the policy's engine: the derivative of the fp32 solve is refused on it
    eng = policy._engine
    z = lambda *s: torch.zeros(*s, device=eng.device)
    sol = dict(U=z(1, eng.T, eng.m), X=z(1, eng.T + 1, eng.n), std=z(1, eng.T, eng.m),
               means_trace=z(0, 1, eng.T, eng.m), costs_trace=z(0, 1, 8))
    with pytest.raises(GmpcError, match="fp32 sampled rollouts only"):
        eng.mppi_vjp(z(1, eng.n), z(1, eng.T + 1, eng.nx), -bound, bound, sol, gU=z(1, eng.T, eng.m),
                     kwargs=dict(num_samples=8, max_iter=0))
