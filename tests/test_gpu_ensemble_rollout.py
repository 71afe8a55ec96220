"""The ensemble rollout on the GPU (gmpc_ensemble_rollout): every member's states, per-step costs
and objective against the fp64 oracle (R1); bit for bit the sampled rollout's arithmetic (R2); independence of a
problem's outputs from its place in the batch, from B and from P (R3); the moments (R4); short rollouts (R5); a NaN
member (R6); statelessness (R7); refusals (R8); the trainer's and the policy's helpers (R9).  Tolerance-based
comparisons go through gpu_util.assert_parity at its defaults; everything else is exact.

Cases: cem_cases' shapes (ragged widths, two column tiles of the layer-0 input, the width cap) with their problems and
sampled_ensemble_cases' three members, and three tile cases on the smallest shape (n 5, m 2, T 8): B = 1, B = 33 (a
full tile of 32 problems plus one row) and B = 64 (two full tiles).

Achieved on MI355X (the tests print them): R1 max-norm error against fp64, HIP / NumPy fp32, over
the ten cases and three members: X 5.8e-8 .. 5.9e-7 / 5.8e-8 .. 2.9e-7, costs 4.5e-8 .. 8.1e-7 / 4.5e-8 .. 5.4e-7, obj
1.3e-9 .. 4.8e-7 / 2.2e-8 .. 1.9e-7; R4 mean 4.2e-8 .. 9.9e-8 and var 1.9e-8 .. 7.5e-8 for both (the same bits)."""

import functools

import numpy as np
import pytest
import torch

import cem_cases as cc
import ensemble_rollout_ref as rr
import gan_mpc_oracle as orc
import gpu_util as gu
import sampled_ensemble_cases as ec
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.norm import ensemble_trainer as et

pytestmark = pytest.mark.gpu

ALL = ("X", "costs", "obj", "mean", "var")
TILES = dict(tile1=1, tile33=33, tile64=64)
CASES = list(ec.NAMES) + list(TILES)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what=""):
    np.testing.assert_array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)), err_msg=what)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _name(case):
    return "base" if case in TILES else case


@functools.lru_cache(maxsize=None)
def _problem(case):
    """cem_cases' problem; a tile case: B problems of the smallest shape on base's networks."""
    if case not in TILES:
        return ec.problem(case)
    (n, m, T, _, _, _), extra = ec.CASES["base"]
    pb = gu.problem(n, m, T, TILES[case], seed=cc.PROBLEM_SEED + 1, bias_scale=0.1, **extra)
    for k in ("dyn", "cmlp", "mpc_w"):
        pb[k] = ec.problem("base")[k]
    return pb


def _engine(case, pb=None, **more):
    return gu.engine_for(_problem(case) if pb is None else pb, critic=False, **more)


def _members(eng, case, which=(0, 1, 2), count=ec.MEMBERS):
    return eng.to_dev(ec.flat([ec.members(_name(case), count)[p] for p in which]))


def _call(eng, case, members, want=ALL, S=None, pb=None, rows=None):
    pb = _problem(case) if pb is None else pb
    rows = slice(None) if rows is None else rows
    d = eng.to_dev
    U = pb["U"][rows] if S is None else pb["U"][rows][:, :S]
    goal = d(pb["goal"][rows]) if ("costs" in want or "obj" in want) else None
    return _np(eng.ensemble_rollout(members, d(pb["x0"][rows]), d(U), goal, want=want))


@functools.lru_cache(maxsize=None)
def _run(case):
    """Everything of the case's three members in one call."""
    eng = _engine(case)
    try:
        out = _call(eng, case, _members(eng, case))
        torch.cuda.synchronize()
    finally:
        eng.close()
    return out


# ---- R1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_r1_every_members_states_costs_and_objective_against_the_oracle(case):
    pb = _problem(case)
    mem = ec.members(_name(case))
    out = _run(case)
    B, T, n = pb["B"], pb["T"], pb["n"]
    assert out["X"].shape == (ec.MEMBERS, B, T + 1, n) and out["costs"].shape == (ec.MEMBERS, B, T + 1)
    assert out["obj"].shape == (ec.MEMBERS, B)
    r32, r64 = rr.rollout(pb, mem), rr.rollout(orc.cast_problem(pb, np.float64), mem)
    gu.set_config(f"ensemble rollout {case}")
    for p in range(ec.MEMBERS):
        for k in ("X", "costs", "obj"):
            e = gu.assert_parity(f"ensemble rollout {k}[{p}] {case}", out[k][p], r32[k][p], r64[k][p])
            print(f"R1 {case} {k}[{p}]: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")
    _same(out["X"][:, :, 0], np.broadcast_to(pb["x0"], (ec.MEMBERS, B, n)), "x_0 is x0")
    assert gu.rel_err(r64["X"][0], r64["X"][1]) > 1e-3       # another member's plane would not pass


# ---- R2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.BITWISE)
def test_r2_bitwise_the_sampled_rollout_of_an_engine_bound_to_the_member(name):
    pb = ec.problem(name)
    out = _run(name)
    for p in range(ec.MEMBERS):
        eng = _engine(name, pb=dict(pb, dyn=ec.members(name)[p]))
        try:
            d = eng.to_dev
            sol = _np(eng.cem_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), ec.LO, ec.HI,
                                    ec.engine_kwargs("cem", name, 0)))
        finally:
            eng.close()
        _same(sol["U"], pb["U"])
        _same(out["X"][p], sol["X"], f"R2 {name} X[{p}]")
        _same(out["obj"][p], sol["obj"], f"R2 {name} obj[{p}]")
    assert not np.array_equal(out["obj"][0], out["obj"][1])


# ---- R3 ------------------------------------------------------------------------------------------------------------
def test_r3_a_problems_outputs_depend_on_neither_its_row_nor_b():
    pb = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _problem("tile33").items()}
    for k in ("x0", "U", "goal"):
        pb[k][32] = pb[k][0]                  # the same problem at row 0 of tile 0 and as the 33rd row
    eng = _engine("tile33", pb=pb)
    try:
        mem = _members(eng, "tile33")
        batch = _call(eng, "tile33", mem, pb=pb)
        alone = _call(eng, "tile33", mem, pb=pb, rows=slice(0, 1))
    finally:
        eng.close()
    assert alone["X"].shape[1] == 1 and batch["X"].shape[1] == 33
    for k in ("X", "costs", "obj"):
        _same(batch[k][:, 0], alone[k][:, 0], f"R3 row 0 {k}")
        _same(batch[k][:, 32], alone[k][:, 0], f"R3 row 32 {k}")
        assert not np.array_equal(batch[k][:, 1], batch[k][:, 0])
    for k in ("mean", "var"):
        _same(batch[k][0], alone[k][0], f"R3 row 0 {k}")
        _same(batch[k][32], alone[k][0], f"R3 row 32 {k}")


def test_r3_a_members_plane_does_not_depend_on_p():
    case = "tile33"
    eng = _engine(case)
    try:
        one = _call(eng, case, _members(eng, case, (0,)), want=("X", "costs", "obj"))
        three = _call(eng, case, _members(eng, case), want=("X", "costs", "obj"))
        sixteen = _call(eng, case, _members(eng, case, tuple(range(16)), count=16), want=("X", "costs", "obj"))
    finally:
        eng.close()
    assert sixteen["X"].shape[0] == 16
    for k in ("X", "costs", "obj"):
        _same(one[k][0], three[k][0], f"R3 P=3 {k}")
        _same(one[k][0], sixteen[k][0], f"R3 P=16 {k}")
        _same(three[k][2], sixteen[k][2], f"R3 P=16 {k}, member 2")
        assert np.isfinite(sixteen[k]).all() and not np.array_equal(sixteen[k][15], sixteen[k][0])
    _same(three["X"], _run(case)["X"], "R3 want does not change X")


# ---- R4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_r4_the_moments_of_the_gpus_own_planes(case):
    out = _run(case)
    m32, v32 = rr.moments(out["X"])
    m64, v64 = rr.moments(out["X"].astype(np.float64))
    np.testing.assert_allclose(m64, out["X"].astype(np.float64).mean(0), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(v64, out["X"].astype(np.float64).var(0), rtol=1e-10, atol=1e-16)
    gu.set_config(f"ensemble rollout {case}")
    e = gu.assert_parity(f"ensemble mean {case}", out["mean"], m32, m64)
    f = gu.assert_parity(f"ensemble var {case}", out["var"], v32, v64)
    print(f"R4 {case}: mean HIP {e[0]:.3e} / fp32 {e[1]:.3e}, var HIP {f[0]:.3e} / fp32 {f[1]:.3e}")
    # the members share x0 -- fl(fl(3 x) / 3) is x or its neighbour, so the spread there is a squared rounding -- and
    # differ behind it
    x0 = out["X"][0, :, 0]
    assert out["var"][:, 1:].max() > 0 and np.all(out["var"][:, 0] <= (np.float32(2.0 ** -23) * np.abs(x0)) ** 2)
    # one IEEE operation each, in member order: the fp32 restatement gives the same bits
    _same(out["mean"], m32, "R4 mean")
    _same(out["var"], v32, "R4 var")


def test_r4_one_member_and_two_identical_members_have_no_spread():
    case = "tile33"
    eng = _engine(case)
    try:
        one = _call(eng, case, _members(eng, case, (1,)), want=("X", "mean", "var"))
        two = _call(eng, case, _members(eng, case, (1, 1)), want=("X", "mean", "var"))
    finally:
        eng.close()
    for out in (one, two):
        _same(out["mean"], out["X"][0], "R4 mean is the member")
        assert not out["var"].any()
    _same(two["X"][1], two["X"][0])
    _same(one["X"][0], _run(case)["X"][1])


@pytest.mark.parametrize("case", ["ragged", "tile33"])
def test_r4_the_moments_without_x_are_the_moments_with_it(case):
    eng = _engine(case)
    try:
        mem = _members(eng, case)
        both = _call(eng, case, mem, want=("mean", "var"))
        mean = _call(eng, case, mem, want=("mean",))
        var = _call(eng, case, mem, want=("var", "obj"))
    finally:
        eng.close()
    full = _run(case)
    assert set(both) == {"mean", "var"} and set(mean) == {"mean"} and set(var) == {"var", "obj"}
    _same(both["mean"], full["mean"])
    _same(both["var"], full["var"])
    _same(mean["mean"], full["mean"])
    _same(var["var"], full["var"])
    _same(var["obj"], full["obj"])


# ---- R5 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["base", "tile33"])
def test_r5_a_short_rollout_is_the_prefix_of_the_whole_one(case):
    pb = _problem(case)
    T = pb["T"]
    full = _run(case)
    eng = _engine(case)
    try:
        mem = _members(eng, case)
        for S in (1, T - 1):
            short = _call(eng, case, mem, want=("X", "mean", "var"), S=S)
            assert short["X"].shape == (ec.MEMBERS, pb["B"], S + 1, pb["n"])
            _same(short["X"], full["X"][:, :, :S + 1], f"R5 S={S} X")
            _same(short["mean"], full["mean"][:, :S + 1], f"R5 S={S} mean")
            _same(short["var"], full["var"][:, :S + 1], f"R5 S={S} var")
        d = eng.to_dev
        for want in (("obj",), ("X", "costs")):
            with pytest.raises(GmpcError, match=r"error -1: ensemble rollout: .*S = 3"):
                eng.ensemble_rollout(mem, d(pb["x0"]), d(pb["U"][:, :3]), d(pb["goal"]), want=want)
    finally:
        eng.close()


# ---- R6 ------------------------------------------------------------------------------------------------------------
def test_r6_a_nan_member_poisons_its_own_plane_and_the_moments_only():
    case = "tile33"
    layers = [list(mb) for mb in ec.members("base")]
    W, b = layers[1][-1]
    W = W.copy()
    W[0, 0] = np.nan                         # one weight of member 1's output layer: state column 0, from step 1 on
    layers[1][-1] = (W, b)
    eng = _engine(case)
    try:
        out = _call(eng, case, eng.to_dev(ec.flat(layers)))
    finally:
        eng.close()
    clean = _run(case)
    for p in (0, 2):
        for k in ("X", "costs", "obj"):
            _same(out[k][p], clean[k][p], f"R6 {k}[{p}]")
    assert np.isnan(out["X"][1][:, 1:, 0]).all() and np.isnan(out["obj"][1]).all()
    assert np.isnan(out["costs"][1][:, 1:-1]).all()
    assert np.isnan(out["mean"][:, 1:, 0]).all() and np.isnan(out["var"][:, 1:, 0]).all()
    _same(out["mean"][:, 0], clean["mean"][:, 0])


# ---- R7 ------------------------------------------------------------------------------------------------------------
def test_r7_a_solve_under_a_set_ensemble_is_the_same_before_and_after():
    name = "base"
    pb = ec.problem(name)
    eng = _engine(name)
    try:
        d = eng.to_dev
        eng.set_sampled_ensemble(_members(eng, name))
        eng.set_sampled_ensemble_mode(aggregate="mean_std", risk=0.5)
        eng.set_sampled_precision("bf16")
        args = (d(pb["x0"]), d(pb["U"]), d(pb["goal"]), ec.LO, ec.HI, ec.engine_kwargs("cem", name, 2))
        before = _np(eng.cem_solve(*args, want=("costs", "elites", "samples")))
        other = _members(eng, name, (3, 4), count=5)
        mid = _call(eng, name, other)
        after = _np(eng.cem_solve(*args, want=("costs", "elites", "samples")))
        eng.set_sampled_ensemble(None)
        plain = _np(eng.cem_solve(*args, want=("costs", "elites", "samples")))
    finally:
        eng.close()
    assert before.keys() == after.keys()
    for k in before:
        _same(before[k], after[k], f"R7 {k}")
    assert np.isfinite(mid["obj"]).all() and not np.array_equal(mid["X"][0], _run(name)["X"][0])
    assert not np.array_equal(before["costs"], plain["costs"])          # the ensemble was in force


def test_r7_a_held_solution_survives_the_call():
    name = "base"
    pb = ec.problem(name)
    B = pb["B"]

    def tail(with_call):
        eng = _engine(name)
        try:
            d = eng.to_dev
            sol = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 3})
            if with_call:
                out = _call(eng, name, _members(eng, name))
                assert np.isfinite(out["obj"]).all() and np.isfinite(out["var"]).all()
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return _np(sol), loss.cpu().numpy(), grad.cpu().numpy()
        finally:
            eng.close()

    s0, l0, g0 = tail(False)
    s1, l1, g1 = tail(True)
    assert s0.keys() == s1.keys()
    for k in s0:
        _same(s0[k], s1[k], f"R7 held {k}")
    _same(l0, l1)
    _same(g0, g1)


# ---- R8 ------------------------------------------------------------------------------------------------------------
def test_r8_refused_arguments_at_the_c_abi():
    from gan_mpc_amd.engine import Engine
    name = "m1"
    pb = ec.problem(name)
    (n, m, T, B, _, _), _ = ec.CASES[name]
    eng = _engine(name)
    try:
        lib, d = eng.lib, eng.to_dev
        mem, x0, U, goal = _members(eng, name), d(pb["x0"]), d(pb["U"]), d(pb["goal"])
        X, costs, obj = eng.new(3, B, T + 1, n), eng.new(3, B, T + 1), eng.new(3, B)
        p = lambda t: None if t is None else t.data_ptr()
        good = dict(ctx=eng.ctx, B=B, S=T, P=3, mem=mem, x0=x0, U=U, goal=goal, X=X, costs=costs, obj=obj, mean=None,
                    var=None)

        def call(**change):
            a = dict(good, **change)
            return lib.gmpc_ensemble_rollout(a["ctx"], a["B"], a["S"], a["P"], p(a["mem"]), p(a["x0"]), p(a["U"]),
                                             p(a["goal"]), p(a["X"]), p(a["costs"]), p(a["obj"]), p(a["mean"]),
                                             p(a["var"]), None)

        assert call() == 0
        torch.cuda.synchronize()
        first = X.cpu().numpy().copy()
        for change in (dict(ctx=None), dict(mem=None), dict(x0=None), dict(U=None), dict(B=0), dict(B=B + 1),
                       dict(S=0), dict(S=T + 1), dict(P=0), dict(P=17), dict(X=None, costs=None, obj=None),
                       dict(goal=None), dict(goal=None, costs=None), dict(goal=None, obj=None),
                       dict(S=T - 1), dict(S=T - 1, obj=None), dict(S=T - 1, costs=None)):
            assert call(**change) != 0, change
            assert lib.gmpc_last_error().startswith(b"ensemble rollout: "), (change, lib.gmpc_last_error())
        assert b"B = 8" in (call(B=B + 1), lib.gmpc_last_error())[1]
        assert b"P = 17" in (call(P=17), lib.gmpc_last_error())[1]
        assert b"S = 6" in (call(S=T + 1), lib.gmpc_last_error())[1]
        # what is allowed: no goal or a short horizon without cost outputs, the moments alone
        assert call(goal=None, costs=None, obj=None) == 0
        assert call(S=T - 1, costs=None, obj=None) == 0
        assert call(X=None, costs=None, obj=None, mean=eng.new(B, T + 1, n)) == 0
        assert call() == 0
        torch.cuda.synchronize()
        _same(X.cpu().numpy(), first)
        fresh = Engine(n, m, T, [n + m, 8, n], [n, 8, 2], max_batch=B)       # no parameters set
        try:
            assert lib.gmpc_ensemble_rollout(fresh.ctx, B, T, 1, p(eng.new(1, fresh.dyn_count)), p(x0), p(U), None,
                                             p(X), None, None, None, None, None) != 0
            assert lib.gmpc_last_error().startswith(b"ensemble rollout: "), lib.gmpc_last_error()
            assert b"gmpc_set_params" in lib.gmpc_last_error()
        finally:
            fresh.close()
    finally:
        eng.close()


def test_r8_refusals_through_the_engine():
    name = "m1"
    pb = ec.problem(name)
    eng = _engine(name)
    try:
        d = eng.to_dev
        mem, x0, U, goal = _members(eng, name), d(pb["x0"]), d(pb["U"]), d(pb["goal"])
        with pytest.raises(GmpcError, match="ensemble rollout: .*unknown entries"):
            eng.ensemble_rollout(mem, x0, U, goal, want=("X", "std"))
        with pytest.raises(GmpcError, match="ensemble rollout: .*need goal"):
            eng.ensemble_rollout(mem, x0, U)
        with pytest.raises(GmpcError, match="ensemble rollout: P = 17"):
            eng.ensemble_rollout(torch.zeros(17, eng.dyn_count, device=eng.device), x0, U, goal)
        big = d(np.zeros((pb["B"] + 1, pb["n"]), np.float32)), d(np.zeros((pb["B"] + 1, pb["T"], pb["m"]), np.float32))
        with pytest.raises(GmpcError, match="error -1: ensemble rollout: B = 8"):       # the library's own
            eng.ensemble_rollout(mem, *big, want=("X",))
        with pytest.raises(GmpcError, match="error -1: ensemble rollout: S = 6"):
            eng.ensemble_rollout(mem, x0, d(np.zeros((pb["B"], pb["T"] + 1, pb["m"]), np.float32)), want=("X",))
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300"])
def test_r8_refused_shapes_carry_the_prefix(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        with pytest.raises(GmpcError, match="error -1: ensemble rollout: "):
            eng.ensemble_rollout(torch.zeros(2, eng.dyn_count, device=eng.device), d(pb["x0"]), d(pb["U"]),
                                 want=("X",))
    finally:
        eng.close()


# ---- R9 ------------------------------------------------------------------------------------------------------------
def test_r9_holdout_errors_and_the_elites():
    name = "cheetah"
    pb = ec.problem(name)
    (n, m, T, B, _, _), extra = ec.CASES[name]
    data = gu.problem(n, m, T, 12, seed=77, bias_scale=0.1, **extra)
    nominal = pb["dyn"]
    # the holdout data: the nominal network's own open-loop trajectories
    Xn = orc.rollout(nominal, data["U"], data["x0"])
    layers = [list(mb) for mb in ec.members(name)]
    other = gu.problem(n, m, T, B, seed=999, bias_scale=0.1, **extra)["dyn"]
    bad = list(nominal)
    bad[-1] = tuple((a + 20 * ec.EPS * b).astype(np.float32) for a, b in zip(nominal[-1], other[-1]))
    layers = [bad] + layers + [list(nominal)]                    # the worst first, the best last
    eng = _engine(name, max_batch=5)                             # 12 sequences: chunks of 5, 5 and 2
    wide = _engine(name, max_batch=12)
    try:
        for e in (eng, wide):
            d = e.to_dev
            mem, xseq, useq, nxt = d(ec.flat(layers)), d(Xn[:, :T]), d(data["U"]), d(Xn[:, 1:])
            errors = et.holdout_errors(e, mem, xseq, useq, nxt)
            if e is wide:
                X = e.ensemble_rollout(mem, xseq[:, 0].contiguous(), useq, want=("X",))["X"]
                want = ((X[:, :, 1:].double() - nxt.double()[None]) ** 2).mean(dim=(1, 3))
                # fp32 difference and square (2^-23 each), an fp64 sum, one rounding to fp32
                np.testing.assert_allclose(errors.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=0)
                whole = errors.cpu().numpy()
            else:
                chunked = errors.cpu().numpy()
        np.testing.assert_allclose(chunked, whole, rtol=1e-6, atol=0)
        assert chunked.shape == (5, T) and chunked.dtype == np.float32
        order = et.elite_members(errors, 5).tolist()
        print(f"R9 summed holdout errors {chunked.sum(1)}, order {order}")
        assert order[0] == 4 and order[-1] == 0                 # the data's own network first, the perturbed one last
        assert chunked[4].sum() < 1e-6 * chunked[1:4].sum(1).min()       # (fp32 rounding against the 5 % members)
        assert chunked[0].sum() > chunked[1:4].sum(1).max()
    finally:
        eng.close()
        wide.close()


def test_r9_from_holdout_errors_to_the_policys_ensemble_and_its_spread():
    import copy

    import test_gpu_mirror as mirror
    from gan_mpc_amd import params as params_lib
    from gan_mpc_amd.norm import l2_policy
    bound = 0.3
    build = lambda **more: mirror._build(functools.partial(
        l2_policy.L2MPC, solver="icem", control_bounds=(-bound, bound),
        icem_kwargs=dict(num_samples=64, max_iter=2, seed=7), **more), N=17, M=6)
    config, plain, params, data = build()
    rng = np.random.default_rng(3)
    trees = []
    for scale in (0.5, 0.02, 0.1, 0.0):                  # member 3 is the nominal network, member 0 the furthest
        tree = copy.deepcopy(params["dynamics_params"])
        for layer in tree["params"].values():
            layer["kernel"] = (np.asarray(layer["kernel"]) * rng.uniform(1 - scale, 1 + scale,
                                                                         np.shape(layer["kernel"]))).astype(np.float32)
        trees.append(tree)
    _, policy, params2, _ = build(dynamics_ensemble=trees)
    B = 6
    x, U = data["hist"][:B, -1], data["init_U"][:B]
    T = U.shape[1]
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        plain.plan_spread(params, x, U)
    Xm, spread = policy.plan_spread(params2, x, U)
    eng = policy._engine
    assert tuple(Xm.shape) == (4, B, T + 1, 17) and tuple(spread.shape) == (B, T + 1)
    direct = eng.ensemble_rollout(policy._ensemble_dev, eng.to_dev(x), eng.to_dev(U), want=("X", "var"))
    _same(Xm.cpu().numpy(), direct["X"].cpu().numpy())
    _same(spread.cpu().numpy(), direct["var"].sum(-1).cpu().numpy())
    # at step 0 the members share x: what is left is the squared rounding of the mean, at most 17 (4 * 2^-22)^2 =
    # 1.5e-11
    assert float(spread[:, 0].max()) < 1e-9 < float(spread[:, 1:].min())
    # holdout data from the nominal network -> the errors -> the two best members -> the policy's ensemble
    nominal = params_lib.tree_to_layers(params2["dynamics_params"])
    Xn = orc.rollout(nominal, U, x)
    d = eng.to_dev
    members = policy._ensemble_dev
    errors = et.holdout_errors(eng, members, d(Xn[:, :T]), d(U), d(Xn[:, 1:]))
    assert tuple(errors.shape) == (4, T)
    elite = et.elite_members(errors, 2)
    print(f"R9 policy: summed errors {errors.sum(1).cpu().numpy()}, elites {elite.tolist()}")
    assert elite.tolist() == [3, 1]
    policy.set_dynamics_ensemble(members[elite])
    assert tuple(policy._engine._ensemble.shape) == (2, eng.dyn_count)
    Xe, spread_e = policy.plan_spread(params2, x, U)
    assert tuple(Xe.shape) == (2, B, T + 1, 17)
    _same(Xe.cpu().numpy(), Xm[elite.to(Xm.device)].cpu().numpy())
    assert float(spread_e[:, 1:].max()) < float(spread[:, 1:].max())
    policy.expert_model.select(np.array([2]))
    a = policy.get_optimal_action(params2, data["hist"][2]).cpu().numpy()
    assert a.shape == (6,) and np.all(np.isfinite(a)) and np.all(np.abs(a) <= np.float32(bound))
