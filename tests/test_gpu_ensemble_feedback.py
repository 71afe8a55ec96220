"""The closed-loop ensemble rollout on the GPU (gmpc_ensemble_rollout_feedback): every member's
states, applied controls, per-step costs and objective against the fp64 reference (F1); bit for bit the open-loop call
without gains (F2) and the reference trajectory itself when a member reproduces it (F3); the clamp (F4); independence
of a problem's outputs from its place in the batch, from B, from P and from S (F5); statelessness (F6); refusals (F7);
the policy's closed_loop_spread (F8).  Tolerance-based comparisons go through gpu_util.assert_parity at its defaults;
everything else is exact.

Cases: test_gpu_ensemble_rollout's ten -- cem_cases' seven shapes with sampled_ensemble_cases' three members, and B = 1,
33 and 64 on the smallest shape (n 5, m 2, T 8).  The gains are trajax's (ensemble_feedback_ref.gains_at): fp64
tvlqr at the fp32 nominal rollout of the problem's controls, cast to fp32, so kernel and reference read the same bits.
F1's two settings: (a) x0 + 0.1 N(0, 1) (seed 7), k given, alpha = 0.5, no bounds; (b) x0 + 0.02 N(0, 1), no k, bounds
-1 / +1.

Achieved on MI355X (the tests print them): F1 max-norm error against fp64, HIP / NumPy fp32, over
the ten cases and three members: (a) X 5.1e-8 .. 7.7e-7 / 5.1e-8 .. 7.0e-7, U 1.3e-8 .. 6.1e-7 / 1.3e-8 .. 7.5e-7, costs
1.7e-8 .. 1.0e-6 / 1.7e-8 .. 1.1e-6, obj 3.3e-8 .. 7.9e-7 / 3.3e-8 .. 1.0e-6; (b) X 5.6e-8 .. 6.4e-7 / the same, U
8.9e-8 .. 1.9e-5 / 1.5e-7 .. 1.8e-5, costs 3.6e-8 .. 4.8e-7 / 1.2e-8 .. 3.6e-7, obj 1.6e-8 .. 2.4e-7 / 2.3e-9 .. 2.1e-7; the
member's open-loop rollout from the same x0 is 0.74 .. 1.02 (a) and 1.4e-2 .. 1.4e-1 (b) away from its closed-loop X."""

import functools

import numpy as np
import pytest
import torch

import ensemble_feedback_ref as fr
import ensemble_rollout_ref as rr
import gan_mpc_oracle as orc
import gpu_util as gu
import sampled_ensemble_cases as ec
import test_gpu_ensemble_rollout as ero
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

ALL = ("X", "U", "costs", "obj", "mean", "var")
CASES = ero.CASES
SETTINGS = dict(a=dict(scale=0.1, k=True, alpha=0.5, lo=None, hi=None),
                b=dict(scale=0.02, k=False, alpha=1.0, lo=ec.LO, hi=ec.HI))
_same, _np, _name, _problem, _engine, _members = ero._same, ero._np, ero._name, ero._problem, ero._engine, ero._members


@functools.lru_cache(maxsize=None)
def _law(case):
    """The case's reference trajectory and gains: dict(X_ref, U_ref, K, k), fp32."""
    pb = _problem(case)
    X_ref, K, k, _, _ = fr.gains_at(pb)
    return dict(X_ref=X_ref, U_ref=pb["U"], K=K, k=k)


def _call(eng, case, members, want=ALL, x0=None, k=False, alpha=1.0, lo=None, hi=None, S=None, rows=None, law=None,
          pb=None):
    """Engine.ensemble_rollout_feedback on the case's law (or `law`), as NumPy arrays."""
    pb = _problem(case) if pb is None else pb
    law = _law(case) if law is None else law
    rows = slice(None) if rows is None else rows
    T = pb["T"]
    S = T if S is None else S
    d = lambda a: eng.to_dev(np.ascontiguousarray(a))
    goal = d(pb["goal"][rows]) if ("costs" in want or "obj" in want) else None
    return _np(eng.ensemble_rollout_feedback(
        members, d(law["X_ref"][rows][:, :S + 1]), d(law["U_ref"][rows][:, :S]), d(law["K"][rows][:, :S]), goal,
        x0=None if x0 is None else d(x0[rows]), k=d(law["k"][rows][:, :S]) if k else None, alpha=alpha, u_lo=lo,
        u_hi=hi, want=want))


@functools.lru_cache(maxsize=None)
def _setting(case, tag):
    """(x0, keywords of _call) of F1's setting `tag`."""
    s = SETTINGS[tag]
    return fr.perturbed_x0(_problem(case), s["scale"]), dict(k=s["k"], alpha=s["alpha"], lo=s["lo"], hi=s["hi"])


@functools.lru_cache(maxsize=None)
def _run(case, tag):
    """Everything of the case's three members in one call, under F1's setting `tag`."""
    x0, kw = _setting(case, tag)
    eng = _engine(case)
    try:
        out = _call(eng, case, _members(eng, case), x0=x0, **kw)
        torch.cuda.synchronize()
    finally:
        eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _refs(case, tag):
    """(fp32 reference, fp64 reference, fp64 open-loop X of U_ref from the same x0) of F1's setting `tag`."""
    pb, mem, law = _problem(case), ec.members(_name(case)), _law(case)
    x0, kw = _setting(case, tag)
    out = []
    for dt in (np.float32, np.float64):
        a = fr.cast_inputs(dt, x0=x0, **law)
        out.append(fr.rollout(pb, mem, a["X_ref"], a["U_ref"], a["K"], x0=a["x0"], k=a["k"] if kw["k"] else None,
                              alpha=kw["alpha"], lo=kw["lo"], hi=kw["hi"]))
    pb64 = orc.cast_problem(pb, np.float64)
    out.append(rr.rollout(dict(pb64, x0=x0.astype(np.float64)), mem, costs=False)["X"])
    return tuple(out)


# ---- F1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(SETTINGS))
@pytest.mark.parametrize("case", CASES)
def test_f1_every_members_states_controls_costs_and_objective_against_the_reference(case, tag):
    pb = _problem(case)
    out = _run(case, tag)
    r32, r64, open_loop = _refs(case, tag)
    x0, _ = _setting(case, tag)
    P, B, T, n, m = ec.MEMBERS, pb["B"], pb["T"], pb["n"], pb["m"]
    assert out["X"].shape == (P, B, T + 1, n) and out["U"].shape == (P, B, T, m)
    assert out["costs"].shape == (P, B, T + 1) and out["obj"].shape == (P, B)
    gu.set_config(f"ensemble feedback {case} ({tag})")
    for p in range(P):
        for key in ("X", "U", "costs", "obj"):
            e = gu.assert_parity(f"ensemble feedback {key}[{p}] {case} ({tag})", out[key][p], r32[key][p], r64[key][p])
            el = gu.el_err(out[key][p], r64[key][p])[0]
            print(f"F1 {case} ({tag}) {key}[{p}]: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}, elementwise HIP {el:.3e}")
        # ignoring K (or k) cannot pass: the member's open-loop rollout of U_ref from the same x0 is elsewhere
        gap = gu.rel_err(open_loop[p], r64["X"][p])
        print(f"F1 {case} ({tag}) open loop vs closed loop, member {p}: {gap:.3e}")
        assert gap > 1e-3
    _same(out["X"][:, :, 0], np.broadcast_to(x0, (P, B, n)), "x_0 is x0")
    assert gu.rel_err(r64["X"][0], r64["X"][1]) > 1e-3       # another member's plane would not pass
    if tag == "b":
        at = (out["U"] == np.float32(ec.LO)) | (out["U"] == np.float32(ec.HI))
        print(f"F1 {case} (b): {100 * at.mean():.1f} % of the applied controls at a bound")


# ---- F2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.BITWISE)
def test_f2_without_gains_bitwise_the_open_loop_call(name):
    pb, law = _problem(name), _law(name)
    open_loop = ero._run(name)
    eng = _engine(name)
    try:
        mem = _members(eng, name)
        zero = dict(law, K=np.zeros_like(law["K"]))
        out = _call(eng, name, mem, x0=pb["x0"], law=zero)
        moved = _call(eng, name, mem, x0=pb["x0"], want=("X",))
    finally:
        eng.close()
    for key in ("X", "costs", "obj", "mean", "var"):
        _same(out[key], open_loop[key], f"F2 {name} {key}")
    _same(out["U"], np.broadcast_to(pb["U"], out["U"].shape), f"F2 {name} U is U_ref")
    assert np.isfinite(out["X"]).all() and not np.array_equal(moved["X"], out["X"])      # the real gains do act


# ---- F3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["base", "cheetah", "tile33"])
def test_f3_a_member_that_reproduces_the_reference_tracks_it_bit_for_bit(case):
    pb, law = _problem(case), _law(case)
    open_loop = ero._run(case)
    eng = _engine(case)
    try:
        mem = _members(eng, case)
        for p in range(ec.MEMBERS):
            own = dict(law, X_ref=open_loop["X"][p])          # member p's own open-loop states; x0 = X_ref[:, 0]
            out = _call(eng, case, mem, want=("X", "U"), law=own)
            _same(out["X"][p], open_loop["X"][p], f"F3 {case} X[{p}]")
            _same(out["U"][p], pb["U"], f"F3 {case} U[{p}]")
            q = (p + 1) % ec.MEMBERS
            assert not np.array_equal(out["U"][q], pb["U"])   # the gains are real: another member is steered
            _same(out["X"][:, :, 0], open_loop["X"][:, :, 0])
        # (four of them: the sum of 2^k equal values and its division by 2^k are exact; with three, fl(fl(3 x) / 3) may
        # be x's neighbour -- section 27's R4)
        twins = _members(eng, case, (1, 1, 1, 1))
        out = _call(eng, case, twins, want=("X", "U", "mean", "var"), law=dict(law, X_ref=open_loop["X"][1]))
        moved = _call(eng, case, twins, want=("X", "mean", "var"), x0=fr.perturbed_x0(pb, 0.02))
    finally:
        eng.close()
    _same(out["mean"], open_loop["X"][1], "F3 mean is the member")
    assert not out["var"].any()
    for p in range(4):
        _same(out["X"][p], open_loop["X"][1])
        _same(moved["X"][p], moved["X"][0])
    _same(moved["mean"], moved["X"][0])
    assert not moved["var"].any() and not np.array_equal(moved["X"][0], open_loop["X"][1])


# ---- F4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_f4_every_applied_control_is_within_the_bounds(case):
    out = _run(case, "b")
    _, r64, _ = _refs(case, "b")
    lo, hi = np.float32(ec.LO), np.float32(ec.HI)
    assert np.all(out["U"] >= lo) and np.all(out["U"] <= hi)
    inside = (r64["U"] >= ec.LO + 1e-4) & (r64["U"] <= ec.HI - 1e-4)
    at = (out["U"] == lo) | (out["U"] == hi)
    assert inside.any() and not (at & inside).any()
    ref_at = (r64["U"] == ec.LO) | (r64["U"] == ec.HI)
    print(f"F4 {case}: at a bound, HIP {100 * at.mean():.1f} % / fp64 {100 * ref_at.mean():.1f} %")
    if case != "w256":        # (its gains are small: nothing saturates there)
        assert at.any() and ref_at.any()


@pytest.mark.parametrize("case", ["base", "tile33", "wide_m"])
def test_f4_bounds_nothing_reaches_are_no_bounds(case):
    x0, kw = _setting(case, "a")
    eng = _engine(case)
    try:
        mem = _members(eng, case)
        wide = _call(eng, case, mem, x0=x0, **dict(kw, lo=-1e30, hi=1e30))
        per_control = _call(eng, case, mem, x0=x0, **dict(kw, lo=np.full(_problem(case)["m"], -1e30, np.float32),
                                                          hi=float("inf")))
    finally:
        eng.close()
    free = _run(case, "a")
    for key in ALL:
        _same(wide[key], free[key], f"F4 {case} {key}")
        _same(per_control[key], free[key], f"F4 {case} {key}, per-control bounds")


# ---- F5 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(SETTINGS))
def test_f5_a_problems_outputs_depend_on_neither_its_row_nor_b(tag):
    case = "tile33"
    copy = lambda v: v.copy() if isinstance(v, np.ndarray) else v
    pb = {key: copy(v) for key, v in _problem(case).items()}
    law = {key: v.copy() for key, v in _law(case).items()}
    x0, kw = _setting(case, tag)
    x0 = x0.copy()
    for arr in (pb["goal"], x0, *law.values()):
        arr[32] = arr[0]                       # the same problem at row 0 of tile 0 and as the 33rd row
    eng = _engine(case, pb=pb)
    try:
        mem = _members(eng, case)
        batch = _call(eng, case, mem, x0=x0, law=law, pb=pb, **kw)
        alone = _call(eng, case, mem, x0=x0, law=law, pb=pb, rows=slice(0, 1), **kw)
    finally:
        eng.close()
    assert alone["X"].shape[1] == 1 and batch["X"].shape[1] == 33
    for key in ("X", "U", "costs", "obj"):
        _same(batch[key][:, 0], alone[key][:, 0], f"F5 row 0 {key}")
        _same(batch[key][:, 32], alone[key][:, 0], f"F5 row 32 {key}")
        assert not np.array_equal(batch[key][:, 1], batch[key][:, 0])
    for key in ("mean", "var"):
        _same(batch[key][0], alone[key][0], f"F5 row 0 {key}")
        _same(batch[key][32], alone[key][0], f"F5 row 32 {key}")
    _same(batch["X"][:, :32], _run(case, tag)["X"][:, :32])       # the other rows do not notice


def test_f5_a_members_planes_do_not_depend_on_p():
    case = "tile33"
    x0, kw = _setting(case, "a")
    want = ("X", "U", "costs", "obj")
    eng = _engine(case)
    try:
        one = _call(eng, case, _members(eng, case, (0,)), want=want, x0=x0, **kw)
        sixteen = _call(eng, case, _members(eng, case, tuple(range(16)), count=16), want=want, x0=x0, **kw)
    finally:
        eng.close()
    three = _run(case, "a")
    assert sixteen["X"].shape[0] == 16 and sixteen["U"].shape[0] == 16
    for key in want:
        _same(one[key][0], three[key][0], f"F5 P=3 {key}")
        _same(one[key][0], sixteen[key][0], f"F5 P=16 {key}")
        _same(three[key][2], sixteen[key][2], f"F5 P=16 {key}, member 2")
        assert np.isfinite(sixteen[key]).all() and not np.array_equal(sixteen[key][15], sixteen[key][0])


@pytest.mark.parametrize("case", ["base", "tile33"])
def test_f5_a_short_rollout_is_the_prefix_of_the_whole_one(case):
    pb = _problem(case)
    T = pb["T"]
    x0, kw = _setting(case, "b")
    full = _run(case, "b")
    eng = _engine(case)
    try:
        mem = _members(eng, case)
        for S in (1, T - 1):
            short = _call(eng, case, mem, want=("X", "U", "mean", "var"), x0=x0, S=S, **kw)
            assert short["X"].shape == (ec.MEMBERS, pb["B"], S + 1, pb["n"])
            assert short["U"].shape == (ec.MEMBERS, pb["B"], S, pb["m"])
            _same(short["X"], full["X"][:, :, :S + 1], f"F5 S={S} X")
            _same(short["U"], full["U"][:, :, :S], f"F5 S={S} U")
            _same(short["mean"], full["mean"][:, :S + 1], f"F5 S={S} mean")
            _same(short["var"], full["var"][:, :S + 1], f"F5 S={S} var")
        for want in (("obj",), ("X", "costs")):
            with pytest.raises(GmpcError, match=r"ensemble feedback: .*S = 3"):
                _call(eng, case, mem, want=want, x0=x0, S=3, **kw)
    finally:
        eng.close()


# ---- F6 ------------------------------------------------------------------------------------------------------------
def test_f6_a_solve_under_a_set_ensemble_is_the_same_before_and_after():
    name = "base"
    pb = ec.problem(name)
    x0, kw = _setting(name, "a")
    eng = _engine(name)
    try:
        d = eng.to_dev
        eng.set_sampled_ensemble(_members(eng, name))
        eng.set_sampled_ensemble_mode(aggregate="mean_std", risk=0.5)
        eng.set_sampled_precision("bf16")
        args = (d(pb["x0"]), d(pb["U"]), d(pb["goal"]), ec.LO, ec.HI, ec.engine_kwargs("cem", name, 2))
        before = _np(eng.cem_solve(*args, want=("costs", "elites", "samples")))
        other = _members(eng, name, (3, 4), count=5)
        mid = _call(eng, name, other, x0=x0, **kw)
        after = _np(eng.cem_solve(*args, want=("costs", "elites", "samples")))
        eng.set_sampled_ensemble(None)
        plain = _np(eng.cem_solve(*args, want=("costs", "elites", "samples")))
    finally:
        eng.close()
    assert before.keys() == after.keys()
    for key in before:
        _same(before[key], after[key], f"F6 {key}")
    assert np.isfinite(mid["obj"]).all() and not np.array_equal(mid["X"][0], _run(name, "a")["X"][0])
    assert not np.array_equal(before["costs"], plain["costs"])          # the ensemble was in force


def test_f6_a_held_solution_survives_the_call():
    name = "base"
    pb = ec.problem(name)
    B = pb["B"]
    x0, kw = _setting(name, "b")

    def tail(with_call):
        eng = _engine(name)
        try:
            d = eng.to_dev
            sol = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 3})
            if with_call:
                out = _call(eng, name, _members(eng, name), x0=x0, **kw)
                assert np.isfinite(out["obj"]).all() and np.isfinite(out["var"]).all()
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return _np(sol), loss.cpu().numpy(), grad.cpu().numpy()
        finally:
            eng.close()

    s0, l0, g0 = tail(False)
    s1, l1, g1 = tail(True)
    assert s0.keys() == s1.keys()
    for key in s0:
        _same(s0[key], s1[key], f"F6 held {key}")
    _same(l0, l1)
    _same(g0, g1)


# ---- F7 ------------------------------------------------------------------------------------------------------------
def test_f7_refused_arguments_at_the_c_abi():
    import ctypes as C

    from gan_mpc_amd.engine import Engine
    name = "m1"
    pb, law = ec.problem(name), _law(name)
    (n, m, T, B, _, _), _ = ec.CASES[name]
    eng = _engine(name)
    try:
        lib, d = eng.lib, eng.to_dev
        mem, goal = _members(eng, name), d(pb["goal"])
        x0, Xr, Ur, K, k = d(pb["x0"]), d(law["X_ref"]), d(law["U_ref"]), d(law["K"]), d(law["k"])
        lo, hi = d(np.full(m, -1, np.float32)), d(np.full(m, 1, np.float32))
        X, U, costs, obj = eng.new(3, B, T + 1, n), eng.new(3, B, T, m), eng.new(3, B, T + 1), eng.new(3, B)
        p = lambda t: None if t is None else t.data_ptr()
        good = dict(ctx=eng.ctx, B=B, S=T, P=3, mem=mem, x0=x0, Xr=Xr, Ur=Ur, K=K, k=k, alpha=0.5, lo=lo, hi=hi,
                    goal=goal, X=X, U=U, costs=costs, obj=obj, mean=None, var=None)

        def call(**change):
            a = dict(good, **change)
            return lib.gmpc_ensemble_rollout_feedback(
                a["ctx"], a["B"], a["S"], a["P"], p(a["mem"]), p(a["x0"]), p(a["Xr"]), p(a["Ur"]), p(a["K"]),
                p(a["k"]), C.c_float(a["alpha"]), p(a["lo"]), p(a["hi"]), p(a["goal"]), p(a["X"]), p(a["U"]),
                p(a["costs"]), p(a["obj"]), p(a["mean"]), p(a["var"]), None)

        assert call() == 0
        torch.cuda.synchronize()
        first = X.cpu().numpy().copy(), U.cpu().numpy().copy()
        nothing = dict(X=None, U=None, costs=None, obj=None)
        for change in (dict(ctx=None), dict(mem=None), dict(Xr=None), dict(Ur=None), dict(K=None), dict(lo=None),
                       dict(hi=None), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-float("inf")),
                       dict(alpha=float("nan"), k=None), dict(B=0), dict(B=B + 1), dict(S=0), dict(S=T + 1),
                       dict(P=0), dict(P=17), nothing, dict(goal=None), dict(goal=None, costs=None),
                       dict(goal=None, obj=None), dict(S=T - 1), dict(S=T - 1, obj=None), dict(S=T - 1, costs=None)):
            assert call(**change) != 0, change
            assert lib.gmpc_last_error().startswith(b"ensemble feedback: "), (change, lib.gmpc_last_error())
        assert b"B = 8" in (call(B=B + 1), lib.gmpc_last_error())[1]
        assert b"P = 17" in (call(P=17), lib.gmpc_last_error())[1]
        assert b"S = 6" in (call(S=T + 1), lib.gmpc_last_error())[1]
        assert b"S = 4 is not T = 5" in (call(S=T - 1), lib.gmpc_last_error())[1]
        assert b"u_lo null, u_hi given" in (call(lo=None), lib.gmpc_last_error())[1]
        assert b"alpha = inf" in (call(alpha=float("inf")), lib.gmpc_last_error())[1]
        # the accepted neighbours: no x0, no k, no bounds, no goal or a short horizon without cost outputs, one
        # output alone -- the applied controls, or a moment
        assert call(x0=None) == 0
        assert call(k=None) == 0
        assert call(lo=None, hi=None) == 0
        assert call(alpha=0.0) == 0
        assert call(goal=None, costs=None, obj=None) == 0
        assert call(S=T - 1, costs=None, obj=None) == 0
        assert call(X=None, costs=None, obj=None) == 0
        assert call(**nothing, mean=eng.new(B, T + 1, n)) == 0
        assert call() == 0
        torch.cuda.synchronize()
        _same(X.cpu().numpy(), first[0])
        _same(U.cpu().numpy(), first[1])
        fresh = Engine(n, m, T, [n + m, 8, n], [n, 8, 2], max_batch=B)       # no parameters set
        try:
            assert lib.gmpc_ensemble_rollout_feedback(
                fresh.ctx, B, T, 1, p(eng.new(1, fresh.dyn_count)), p(x0), p(Xr), p(Ur), p(K), None, C.c_float(1.0),
                None, None, None, p(X), None, None, None, None, None, None) != 0
            assert lib.gmpc_last_error().startswith(b"ensemble feedback: "), lib.gmpc_last_error()
            assert b"gmpc_set_params" in lib.gmpc_last_error()
        finally:
            fresh.close()
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300"])
def test_f7_refused_shapes_carry_the_prefix(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    eng = gu.engine_for(pb, critic=False)
    try:
        z = lambda *shape: torch.zeros(*shape, device=eng.device)
        B, T, n, m = pb["B"], pb["T"], eng.n, eng.m
        with pytest.raises(GmpcError, match="error -1: ensemble feedback: "):
            eng.ensemble_rollout_feedback(z(2, eng.dyn_count), z(B, T + 1, n), z(B, T, m), z(B, T, m, n), want=("X",))
    finally:
        eng.close()


# ---- F8 ------------------------------------------------------------------------------------------------------------
def _policy(**more):
    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    return mirror._build(functools.partial(l2_policy.L2MPC, **more), N=17, M=6)


def _trees(params, scales=(0.5, 0.02, 0.1)):
    import copy
    rng = np.random.default_rng(3)
    trees = []
    for scale in scales:
        tree = copy.deepcopy(params["dynamics_params"])
        for layer in tree["params"].values():
            layer["kernel"] = (np.asarray(layer["kernel"]) * rng.uniform(1 - scale, 1 + scale,
                                                                         np.shape(layer["kernel"]))).astype(np.float32)
        trees.append(tree)
    return trees


def _check_policy(policy, params, data, members, flat, bounds):
    """closed_loop_spread against the Engine calls it is made of, bit for bit; the documented shapes; step 0."""
    B = 6
    x, U, goal = data["hist"][:B, -1], data["init_U"][:B], data["goal"][:B]
    T = U.shape[1]
    Xm, Um, spread = policy.closed_loop_spread(params, x, U, goal, members=members)
    P = flat.shape[0]
    assert tuple(Xm.shape) == (P, B, T + 1, 17) and tuple(Um.shape) == (P, B, T, 6)
    assert tuple(spread.shape) == (B, T + 1)
    eng = policy._engine
    d = eng.to_dev
    X, _ = eng.rollout_cost(d(x), d(U), d(goal))
    gains = eng.lqr_backward(X, d(U), d(goal), after_rollout=True)
    lo, hi = (None, None) if bounds is None else bounds
    direct = eng.ensemble_rollout_feedback(d(flat), X, d(U), gains["K"], x0=d(x), u_lo=lo, u_hi=hi,
                                           want=("X", "U", "var"))
    _same(Xm.cpu().numpy(), direct["X"].cpu().numpy())
    _same(Um.cpu().numpy(), direct["U"].cpu().numpy())
    _same(spread.cpu().numpy(), direct["var"].sum(-1).cpu().numpy())
    # at step 0 the three members share x: fl(fl(3 x) / 3) is x or its neighbour (section 27's R4), so the spread
    # there is at most sum_j (2^-23 |x_j|)^2 (the fp32 sum over j allowed one part in 1e6)
    bound = ((2.0 ** -23 * np.abs(x.astype(np.float64))) ** 2).sum(-1) * (1 + 1e-6)
    s = spread.cpu().numpy().astype(np.float64)
    assert P == 3 and np.all(s[:, 0] <= bound) and s[:, 1:].min() > 1e-9
    # another start, the feed-forward term: both change the answer, and the states start where they are told to
    x1 = (x + 0.05).astype(np.float32)
    Xs, Us, _ = policy.closed_loop_spread(params, x, U, goal, x0=x1, members=members)
    _same(Xs[:, :, 0].cpu().numpy(), np.broadcast_to(x1, (P, B, 17)))
    assert not np.array_equal(Us.cpu().numpy(), Um.cpu().numpy())
    Xf, Uf, _ = policy.closed_loop_spread(params, x, U, goal, members=members, feedforward=True)
    with_k = eng.ensemble_rollout_feedback(d(flat), X, d(U), gains["K"], x0=d(x), k=gains["k"], alpha=1.0, u_lo=lo,
                                           u_hi=hi, want=("X", "U"))
    _same(Xf.cpu().numpy(), with_k["X"].cpu().numpy())
    _same(Uf.cpu().numpy(), with_k["U"].cpu().numpy())
    assert not np.array_equal(Uf.cpu().numpy(), Um.cpu().numpy())
    return Um.cpu().numpy()


def test_f8_closed_loop_spread_of_an_ilqr_policy_with_explicit_members():
    from gan_mpc_amd import params as params_lib
    _, policy, params, data = _policy()
    assert policy.solver == "rounds" and policy.dynamics_ensemble is None
    x, U, goal = data["hist"][:6, -1], data["init_U"][:6], data["goal"][:6]
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        policy.closed_loop_spread(params, x, U, goal)
    trees = _trees(params)
    flat = np.stack([params_lib.pack_mlp(tree) for tree in trees]).astype(np.float32)
    from_trees = _check_policy(policy, params, data, trees, flat, None)
    Xa, Ua, _ = policy.closed_loop_spread(params, x, U, goal, members=flat)
    _same(Ua.cpu().numpy(), from_trees)
    Xt, Ut, _ = policy.closed_loop_spread(params, x, U, goal, members=torch.as_tensor(flat))
    _same(Ut.cpu().numpy(), from_trees)
    assert policy.dynamics_ensemble is None                      # nothing was kept


def test_f8_closed_loop_spread_of_a_sampling_policy_with_its_own_ensemble():
    bound = 0.3
    build = lambda **more: _policy(solver="icem", control_bounds=(-bound, bound),
                                   icem_kwargs=dict(num_samples=64, max_iter=2, seed=7), **more)
    _, _, params, _ = build()
    _, policy, params2, data = build(dynamics_ensemble=_trees(params))
    Um = _check_policy(policy, params2, data, None, policy.dynamics_ensemble, (-bound, bound))
    assert np.abs(Um).max() == np.float32(bound)
