"""The ensemble rollout's VJP on the GPU (gmpc_ensemble_rollout_vjp): every output against the
fp64 reference at the GPU's own X (V1); against the VALU kernel of gmpc_rollout_vjp on engines bound to one member
each (V2); the members' weight gradients against gmpc_dynamics_ensemble_loss_grad under discounted-MSE cotangents (V3);
exactness -- repeats, a problem's place in the batch, P, zero cotangents, subsets of outputs, a NULL gcost -- (V4); a NaN
member (V5); statelessness (V6); refusals (V7); ensemble_rollout_layer (V8); plan_risk and refine_plan (V9).

Cases: sampled_ensemble_cases' shapes with their three members, and test_gpu_ensemble_rollout's three tile cases (B = 1,
33, 64 on n 5, m 2, T 8).  Tolerances: test_gpu_rollout_vjp's for the same quantities -- gpu_util.assert_parity at its
defaults for x0 / U / goal, tol=1e-4, slack=10, el_tol=1e-2 for the sums over the batch --, and rel_err <= 1e-4 between
two differently ordered kernels.  A problem is left out of V1 / V8 / V9 when any member's rollout is within
gpu_util's 3e-6 of a relu kink.

Achieved on MI355X (the tests print them): see DESIGN.md section 29."""

import functools
import itertools

import numpy as np
import pytest
import torch

import ensemble_rollout_vjp_ref as vr
import gan_mpc_oracle as orc
import gpu_util as gu
import sampled_ensemble_cases as ec
import test_gpu_ensemble_rollout as ero
from gan_mpc_amd import params as params_lib
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

CASES = ero.CASES
KEYS = vr.KEYS
SUMS = ("theta", "members")
_same = ero._same


def _tol(key):
    return dict(tol=1e-4, slack=10.0, el_tol=1e-2) if key in SUMS else {}


def _cots(X, which, seed=5):
    rng = np.random.default_rng(seed)
    gX = rng.standard_normal(X.shape).astype(np.float32) if which in ("gX", "both") else None
    gc = rng.standard_normal(X.shape[:3]).astype(np.float32) if which in ("gc", "both") else None
    return gX, gc


def _call(eng, members, X, U, goal, gX, gc, want=KEYS):
    d = lambda a: None if a is None else eng.to_dev(a)  # noqa: E731
    out = eng.ensemble_rollout_vjp(members, d(X), d(U), d(goal), d(gX), d(gc), want=want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _kept(pb64, mem64, X64):
    """(B,) bool: no member's rollout of the problem is near a relu kink."""
    T = pb64["T"]
    bad = np.zeros(X64.shape[1], bool)
    for p, layers in enumerate(mem64):
        bad |= gu.dyn_near_kink(layers, X64[p], pb64["U"]).any(1) | gu.near_kink(pb64["cmlp"], X64[p][:, T])
    return ~bad


def _mem64(case, count=ec.MEMBERS):
    return [[(W.astype(np.float64), b.astype(np.float64)) for W, b in layers]
            for layers in ec.members(ero._name(case), count)]


# The sums over the members can cancel: an entry ((g^0 + g^1) + g^2) far below the members' own values carries their
# rounding, amplified by kappa = sum_p |g^p| / |sum_p g^p| (the denominator floored as gpu_util.el_err floors it).
# Any fp32 evaluation leaves about two ulps (4 * 2^-24) on a member's value -- NumPy fp32's own figure here, 1e-7 --,
# so the elementwise bound el_tol = 1e-3 can be met by an fp32 result only where kappa <= 1e-3 / 2^-22 = 4194.  V1
# draws its cotangents from the first seed whose fp64 reference stays below that on x0, U and goal (decided on the
# reference alone).  Seed 5 on wide_m under gcost has an entry of dL/dU with kappa = 2.7e4 (-0.0697 + 0.0634 + 0.0063
# = -5.2e-6): the kernel's 1.8e-3 and NumPy fp32's 4.9e-3 there are that entry's rounding, not an error.
KAPPA = 1e-3 / 2.0 ** -22


def _conditioned(r64):
    for k in ("x0", "U", "goal"):
        s = np.abs(r64[k])
        if s.max() == 0:
            continue
        tot = sum(np.abs(q[k]) for q in r64["per"])
        if (tot / np.maximum(s, gu.EL_FLOOR * s.max())).max() > KAPPA:
            return False
    return True


def _refs(pb, members, X, U, goal, gX, gc):
    r32 = vr.reference(pb, members, X, U, goal, gX, gc)
    f64 = lambda a: None if a is None else a.astype(np.float64)  # noqa: E731
    r64 = vr.reference(orc.cast_problem(pb, np.float64), members, f64(X), f64(U), f64(goal), f64(gX), f64(gc))
    return r32, r64


# ---- V1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,which", list(itertools.product(CASES, ("gX", "gc", "both"))))
def test_v1_every_output_against_fp64_at_the_gpus_own_states(case, which):
    pb = ero._problem(case)
    members = ec.members(ero._name(case))
    X = ero._run(case)["X"]
    ok = _kept(orc.cast_problem(pb, np.float64), _mem64(case), X.astype(np.float64))
    print(f"V1 {case}: {ok.sum()} of {pb['B']} problems kept")
    assert ok.sum() >= max(1, pb["B"] // 2)
    X, U, goal = (np.ascontiguousarray(a) for a in (X[:, ok], pb["U"][ok], pb["goal"][ok]))
    for seed in range(5, 21):
        gX, gc = _cots(X, which, seed)
        r32, r64 = _refs(pb, members, X, U, goal, gX, gc)
        if _conditioned(r64):
            break
    else:
        raise AssertionError("no well-conditioned draw of the cotangents in 16 seeds")
    print(f"V1 {case} {which}: cotangents of seed {seed}")
    eng = ero._engine(case)
    try:
        got = _call(eng, ero._members(eng, case), X, U, goal, gX, gc)
        torch.cuda.synchronize()
    finally:
        eng.close()
    gu.set_config(f"ensemble rollout vjp {case}")
    assert got["members"].shape == (ec.MEMBERS, r64["members"].shape[1])
    for key in KEYS:
        if which == "gX" and key in ("goal", "theta"):
            assert np.abs(got[key]).max() == 0, key       # no cost cotangent: nothing reaches these
            continue
        e = gu.assert_parity(f"ensemble rollout vjp {key} ({which}) {case}", got[key], r32[key], r64[key], **_tol(key))
        print(f"V1 {case} {which} {key}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")
    assert not got["goal"][:, -1].any()
    if which == "both":
        # another member's plane does not pass: member p differentiated at member p + 1's states
        wrong = vr.reference(orc.cast_problem(pb, np.float64), members, np.roll(X, 1, 0).astype(np.float64),
                             U.astype(np.float64), goal.astype(np.float64), gX, gc)
        for key in KEYS:
            assert gu.rel_err(wrong[key], r64[key]) > 1e-3, key         # 100 x and 10 x the tolerances above


# ---- V2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_v2_against_the_valu_kernel_on_engines_bound_to_one_member_each(case):
    pb = ero._problem(case)
    members = ec.members(ero._name(case))
    X = ero._run(case)["X"]
    gX, gc = _cots(X, "both", 6)
    eng = ero._engine(case)
    try:
        got = _call(eng, ero._members(eng, case), X, pb["U"], pb["goal"], gX, gc)
    finally:
        eng.close()
    want = {k: 0.0 for k in ("x0", "U", "goal", "theta")}
    for p in range(ec.MEMBERS):
        one = ero._engine(case, pb=dict(pb, dyn=members[p]))
        try:
            d = one.to_dev
            r = one.rollout_vjp(d(X[p]), d(pb["U"]), d(pb["goal"]), d(gX[p]), d(gc[p]))
            r = {k: v.cpu().numpy().astype(np.float64) for k, v in r.items()}
        finally:
            one.close()
        for k in want:
            want[k] = want[k] + r[k]
        e = gu.rel_err(got["members"][p], r["dyn"])
        print(f"V2 {case} members[{p}]: {e:.3e}")
        assert e <= 1e-4, (p, e)
    for k in want:
        e = gu.rel_err(got[k], want[k])
        print(f"V2 {case} {k}: {e:.3e}")
        assert e <= 1e-4, (k, e)


# ---- V3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["base", "cheetah", "ragged", "tile33"])
def test_v3_discounted_mse_cotangents_give_the_ensemble_fits_gradient(case):
    pb = ero._problem(case)
    B, T, n = pb["B"], pb["T"], pb["n"]
    X = ero._run(case)["X"]
    rng = np.random.default_rng(2)
    Y = (X[0][:, 1:] + 0.1 * rng.standard_normal(X[0][:, 1:].shape)).astype(np.float32)
    disc, gam = 0.9, np.float32(1.0)
    gX = np.zeros(X.shape, np.float32)
    for t in range(T):
        gX[:, :, t + 1] = 2 * gam * (X[:, :, t + 1] - Y[None, :, t])
        gam = np.float32(gam * np.float32(disc))
    xseq = np.zeros((B, T, n), np.float32)
    xseq[:, 0] = pb["x0"]
    eng = ero._engine(case)
    try:
        d = eng.to_dev
        mem = ero._members(eng, case)
        _, want = eng.dynamics_ensemble_loss_grad(mem, d(xseq), d(pb["U"]), d(Y), disc, False)
        want = want.cpu().numpy()
        got = _call(eng, mem, X, pb["U"], pb["goal"], gX, None, want=("members",))
    finally:
        eng.close()
    assert np.abs(want).max() > 0
    for p in range(ec.MEMBERS):
        e = gu.rel_err(got["members"][p], want[p])
        print(f"V3 {case} members[{p}]: {e:.3e}")
        assert e <= 1e-4, (p, e)


# ---- V4 ------------------------------------------------------------------------------------------------------------
def _rolled(eng, mem, pb, rows=slice(None)):
    d = eng.to_dev
    return eng.ensemble_rollout(mem, d(pb["x0"][rows]), d(pb["U"][rows]), d(pb["goal"][rows]),
                                want=("X",))["X"].cpu().numpy()


def test_v4_repeats_and_a_problems_place_in_the_batch():
    pb = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ero._problem("tile33").items()}
    for k in ("x0", "U", "goal"):
        pb[k][32] = pb[k][0]                  # the same problem at row 0 of tile 0 and as the 33rd row
    eng = ero._engine("tile33", pb=pb)
    try:
        mem = ero._members(eng, "tile33")
        X = _rolled(eng, mem, pb)
        _same(X[:, 32], X[:, 0])
        gX, gc = _cots(X, "both", 3)
        gX[:, 32], gc[:, 32] = gX[:, 0], gc[:, 0]
        batch = _call(eng, mem, X, pb["U"], pb["goal"], gX, gc)
        for _ in range(2):
            again = _call(eng, mem, X, pb["U"], pb["goal"], gX, gc)
            for k in KEYS:
                _same(again[k], batch[k], f"V4 repeat {k}")
        alone = _call(eng, mem, X[:, :1], pb["U"][:1], pb["goal"][:1], gX[:, :1], gc[:, :1])
    finally:
        eng.close()
    for k in ("x0", "U", "goal"):
        _same(batch[k][0], alone[k][0], f"V4 row 0 {k}")
        _same(batch[k][32], alone[k][0], f"V4 row 32 {k}")
        assert not np.array_equal(batch[k][1], batch[k][0])


def test_v4_a_members_gradient_does_not_depend_on_p_and_zero_cotangents_add_nothing():
    case = "tile33"
    pb = ero._problem(case)
    eng = ero._engine(case)
    try:
        m16 = ero._members(eng, case, tuple(range(16)), count=16)
        X = _rolled(eng, m16, pb)
        gX, gc = _cots(X, "both", 4)
        c = lambda a, sl: np.ascontiguousarray(a[sl])  # noqa: E731
        sixteen = _call(eng, m16, X, pb["U"], pb["goal"], gX, gc)
        three = _call(eng, m16[:3].contiguous(), c(X, slice(0, 3)), pb["U"], pb["goal"], c(gX, slice(0, 3)),
                      c(gc, slice(0, 3)))
        one = _call(eng, m16[:1].contiguous(), c(X, slice(0, 1)), pb["U"], pb["goal"], c(gX, slice(0, 1)),
                    c(gc, slice(0, 1)))
        second = _call(eng, m16[1:2].contiguous(), c(X, slice(1, 2)), pb["U"], pb["goal"], c(gX, slice(1, 2)),
                       c(gc, slice(1, 2)))
        zX, zc = np.zeros_like(gX[:3]), np.zeros_like(gc[:3])
        zX[1], zc[1] = gX[1], gc[1]
        masked = _call(eng, m16[:3].contiguous(), c(X, slice(0, 3)), pb["U"], pb["goal"], zX, zc)
    finally:
        eng.close()
    assert sixteen["members"].shape[0] == 16 and np.isfinite(sixteen["members"]).all()
    _same(one["members"][0], three["members"][0], "V4 P=3 members[0]")
    _same(one["members"][0], sixteen["members"][0], "V4 P=16 members[0]")
    _same(three["members"][2], sixteen["members"][2], "V4 P=16 members[2]")
    assert not np.array_equal(sixteen["members"][15], sixteen["members"][0])
    # P = 1: the member's value; the other members' zero cotangents add exact zeros
    for k in ("x0", "U", "goal"):
        assert np.array_equal(masked[k], second[k]), k
        assert not np.array_equal(three[k], second[k])
    _same(masked["members"][1], second["members"][0])
    assert not masked["members"][0].any() and not masked["members"][2].any()
    # theta sums P B rows in one pass, another grouping than B rows: two differently ordered sums
    e = gu.rel_err(masked["theta"], second["theta"])
    print(f"V4 theta of the masked call against the P = 1 call: {e:.3e}")
    assert e <= 1e-4


def test_v4_any_subset_of_outputs_and_a_null_gcost():
    case = "tile33"
    pb = ero._problem(case)
    X = ero._run(case)["X"]
    gX, gc = _cots(X, "both", 1)
    eng = ero._engine(case)
    try:
        mem = ero._members(eng, case)
        full = _call(eng, mem, X, pb["U"], pb["goal"], gX, gc)
        for mask in range(1, 32):
            want = tuple(k for i, k in enumerate(KEYS) if mask >> i & 1)
            part = _call(eng, mem, X, pb["U"], pb["goal"], gX, gc, want=want)
            assert tuple(part) == want
            for k in want:
                _same(part[k], full[k], f"V4 {k} with {want}")
        nogc = _call(eng, mem, X, pb["U"], pb["goal"], gX, None)
    finally:
        eng.close()
    assert not nogc["theta"].any() and not nogc["goal"].any()
    assert nogc["x0"].any() and nogc["U"].any() and nogc["members"].any()


# ---- V5 ------------------------------------------------------------------------------------------------------------
def test_v5_a_nan_member_poisons_its_own_row_and_the_shared_sums():
    case = "tile33"
    pb = ero._problem(case)
    T = pb["T"]
    layers = [list(mb) for mb in ec.members("base")]
    W, b = layers[1][-1]
    W = W.copy()
    W[0, 0] = np.nan                         # one weight of member 1's output layer: state column 0, from step 1 on
    layers[1][-1] = (W, b)
    eng = ero._engine(case)
    try:
        bad = eng.to_dev(ec.flat(layers))
        good = ero._members(eng, case)
        X = _rolled(eng, bad, pb)
        gX, gc = _cots(X, "both", 8)
        out = _call(eng, bad, X, pb["U"], pb["goal"], gX, gc)
        Xc = X.copy()
        Xc[1] = ero._run(case)["X"][1]
        clean = _call(eng, good, Xc, pb["U"], pb["goal"], gX, gc)
    finally:
        eng.close()
    assert np.isnan(X[1][:, 1:, 0]).all() and np.isfinite(X[0]).all() and np.isfinite(X[2]).all()
    for p in (0, 2):
        _same(out["members"][p], clean["members"][p], f"V5 members[{p}]")
        assert np.isfinite(out["members"][p]).all()
    assert not np.isfinite(out["members"][1]).all()
    # what member 1's NaN states reach: x_t - goal_t of every step t >= 1, so v_1 .. and dL/dx0, dL/dgoal_t, the
    # mpc_w sums, and through v_1 the first step's dL/dU
    assert np.isnan(out["x0"]).all() and np.isnan(out["goal"][:, 1:T]).all() and np.isnan(out["U"][:, 0]).all()
    assert np.isnan(out["theta"][1]) and not out["goal"][:, T].any()


# ---- V6 ------------------------------------------------------------------------------------------------------------
def test_v6_a_held_solution_survives_the_call():
    name = "base"
    pb = ec.problem(name)
    B = pb["B"]
    X = ero._run(name)["X"]
    gX, gc = _cots(X, "both", 2)

    def tail(with_call):
        eng = ero._engine(name)
        try:
            d = eng.to_dev
            sol = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 3})
            if with_call:
                out = _call(eng, ero._members(eng, name), X, pb["U"], pb["goal"], gX, gc)
                assert all(np.isfinite(v).all() for v in out.values())
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return ero._np(sol), loss.cpu().numpy(), grad.cpu().numpy()
        finally:
            eng.close()

    s0, l0, g0 = tail(False)
    s1, l1, g1 = tail(True)
    assert s0.keys() == s1.keys()
    for k in s0:
        _same(s0[k], s1[k], f"V6 held {k}")
    _same(l0, l1)
    _same(g0, g1)


def test_v6_a_solve_under_a_set_ensemble_is_the_same_before_and_after():
    name = "base"
    pb = ec.problem(name)
    eng = ero._engine(name)
    try:
        d = eng.to_dev
        eng.set_sampled_ensemble(ero._members(eng, name))
        eng.set_sampled_ensemble_mode(aggregate="mean_std", risk=0.5)
        eng.set_sampled_precision("bf16")
        args = (d(pb["x0"]), d(pb["U"]), d(pb["goal"]), ec.LO, ec.HI, ec.engine_kwargs("cem", name, 2))
        before = ero._np(eng.cem_solve(*args, want=("costs", "elites", "samples")))
        other = ero._members(eng, name, (3, 4), count=5)
        X = _rolled(eng, other, pb)
        gX, gc = _cots(X, "both", 2)
        mid = _call(eng, other, X, pb["U"], pb["goal"], gX, gc)
        after = ero._np(eng.cem_solve(*args, want=("costs", "elites", "samples")))
    finally:
        eng.close()
    assert before.keys() == after.keys()
    for k in before:
        _same(before[k], after[k], f"V6 {k}")
    assert all(np.isfinite(v).all() and v.any() for v in mid.values())


def test_v6_the_shared_call_workspace_carries_nothing_over():
    case = "tile33"
    pb = ero._problem(case)
    B, T, n = pb["B"], pb["T"], pb["n"]
    X = ero._run(case)["X"]
    gX, gc = _cots(X, "both", 9)
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((B, T, n)).astype(np.float32)
    xseq = np.ascontiguousarray(X[0][:, :T])

    def run(eng, op, Bq):
        d = lambda a: eng.to_dev(np.ascontiguousarray(a[:Bq]))  # noqa: E731
        dp = lambda a: eng.to_dev(np.ascontiguousarray(a[:, :Bq]))  # noqa: E731
        mem = ero._members(eng, case)
        if op == "ens_vjp":
            out = eng.ensemble_rollout_vjp(mem, dp(X), d(pb["U"]), d(pb["goal"]), dp(gX), dp(gc))
        elif op == "rollout_vjp":
            out = eng.rollout_vjp(d(X[0]), d(pb["U"]), d(pb["goal"]), d(gX[0]), d(gc[0]))
        elif op == "ens_fit":
            out = dict(zip(("loss", "grad"), eng.dynamics_ensemble_loss_grad(mem, d(xseq), d(pb["U"]), d(Y), 0.9,
                                                                             True)))
        else:
            out = eng.ensemble_rollout(mem, d(pb["x0"]), d(pb["U"]), want=("mean", "var"))     # planes in the workspace
        return {k: v.cpu().numpy() for k, v in out.items()}

    ops = ("ens_vjp", "rollout_vjp", "ens_fit", "ens_rollout")
    fresh = {}
    for op, Bq in itertools.product(ops, (B, 5)):
        eng = ero._engine(case)
        try:
            fresh[op, Bq] = run(eng, op, Bq)
        finally:
            eng.close()
    big, small = [(op, B) for op in ops], [(op, 5) for op in ops]
    eng = ero._engine(case)
    try:
        for step, (op, Bq) in enumerate(big + small[::-1] + big[::-1] + small + big[:1]):
            got = run(eng, op, Bq)
            for key, want in fresh[op, Bq].items():
                _same(got[key], want, f"V6 step {step}: {op} B={Bq} {key}")
    finally:
        eng.close()


# ---- V7 ------------------------------------------------------------------------------------------------------------
def test_v7_refused_arguments_at_the_c_abi():
    from gan_mpc_amd.engine import Engine
    name = "m1"
    pb = ec.problem(name)
    (n, m, T, B, _, _), _ = ec.CASES[name]
    eng = ero._engine(name)
    try:
        lib, d = eng.lib, eng.to_dev
        mem, U, goal = ero._members(eng, name), d(pb["U"]), d(pb["goal"])
        X = d(ero._run(name)["X"])
        gX, gc = (d(a) for a in _cots(ero._run(name)["X"], "both"))
        gx0, gU = eng.new(B, n), eng.new(B, T, m)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        good = dict(ctx=eng.ctx, B=B, P=3, mem=mem, X=X, U=U, goal=goal, gX=gX, gc=gc, gx0=gx0, gU=gU, ggoal=None,
                    gtheta=None, gmem=None)

        def call(**change):
            a = dict(good, **change)
            return lib.gmpc_ensemble_rollout_vjp(a["ctx"], a["B"], a["P"], p(a["mem"]), p(a["X"]), p(a["U"]),
                                                 p(a["goal"]), p(a["gX"]), p(a["gc"]), p(a["gx0"]), p(a["gU"]),
                                                 p(a["ggoal"]), p(a["gtheta"]), p(a["gmem"]), None)

        assert call() == 0
        torch.cuda.synchronize()
        first = gU.cpu().numpy().copy()
        for change in (dict(ctx=None), dict(mem=None), dict(X=None), dict(U=None), dict(goal=None), dict(B=0),
                       dict(B=B + 1), dict(P=0), dict(P=17), dict(gX=None, gc=None), dict(gx0=None, gU=None)):
            assert call(**change) == -1, change                      # GMPC_EINVAL
            assert lib.gmpc_last_error().startswith(b"ensemble rollout vjp: "), (change, lib.gmpc_last_error())
        assert b"B = 8" in (call(B=B + 1), lib.gmpc_last_error())[1]
        assert b"B = 0" in (call(B=0), lib.gmpc_last_error())[1]
        assert b"P = 17" in (call(P=17), lib.gmpc_last_error())[1]
        assert b"both null" in (call(gX=None, gc=None), lib.gmpc_last_error())[1]
        assert b"every output is null" in (call(gx0=None, gU=None), lib.gmpc_last_error())[1]
        # what is allowed: one cotangent, one output
        assert call(gX=None) == 0 and call(gc=None) == 0 and call(gx0=None) == 0
        assert call(gx0=None, gU=None, gmem=eng.new(3, eng.dyn_count)) == 0
        assert call() == 0
        torch.cuda.synchronize()
        _same(gU.cpu().numpy(), first)
        fresh = Engine(n, m, T, [n + m, 8, n], [n, 8, 2], max_batch=B)       # no parameters set
        try:
            assert lib.gmpc_ensemble_rollout_vjp(fresh.ctx, B, 1, p(eng.new(1, fresh.dyn_count)), p(X), p(U), p(goal),
                                                 p(gX), None, p(gx0), None, None, None, None, None) != 0
            assert lib.gmpc_last_error().startswith(b"ensemble rollout vjp: "), lib.gmpc_last_error()
            assert b"gmpc_set_params" in lib.gmpc_last_error()
        finally:
            fresh.close()
    finally:
        eng.close()


def test_v7_refusals_through_the_engine():
    name = "m1"
    pb = ec.problem(name)
    B, T, n, m = pb["B"], pb["T"], pb["n"], pb["m"]
    eng = ero._engine(name)
    try:
        d = eng.to_dev
        mem, U, goal = ero._members(eng, name), d(pb["U"]), d(pb["goal"])
        X = d(ero._run(name)["X"])
        with pytest.raises(GmpcError, match="ensemble rollout vjp: .*unknown entries"):
            eng.ensemble_rollout_vjp(mem, X, U, goal, gX=X, want=("x0", "dyn"))
        with pytest.raises(GmpcError, match="ensemble rollout vjp: .*both None"):
            eng.ensemble_rollout_vjp(mem, X, U, goal)
        with pytest.raises(GmpcError, match="ensemble rollout vjp: P = 17"):
            eng.ensemble_rollout_vjp(torch.zeros(17, eng.dyn_count, device=eng.device), X, U, goal, gX=X)
        z = lambda *s: d(np.zeros(s, np.float32))  # noqa: E731
        with pytest.raises(GmpcError, match="error -1: ensemble rollout vjp: B = 8"):       # the library's own
            eng.ensemble_rollout_vjp(mem, z(3, B + 1, T + 1, n), z(B + 1, T, m), z(B + 1, T + 1, n),
                                     gX=z(3, B + 1, T + 1, n))
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300"])
def test_v7_refused_shapes_carry_the_prefix(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        X = torch.zeros(2, 2, 4, eng.n, device=eng.device)
        with pytest.raises(GmpcError, match="error -1: ensemble rollout vjp: "):
            eng.ensemble_rollout_vjp(torch.zeros(2, eng.dyn_count, device=eng.device), X, d(pb["U"]),
                                     torch.zeros(2, 4, eng.n, device=eng.device), gX=X, want=("U",))
    finally:
        eng.close()


# ---- V8 / V9: the layer and the policy ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _policy(N, M, with_ensemble=True):
    import copy

    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    build = lambda **more: mirror._build(functools.partial(  # noqa: E731
        l2_policy.L2MPC, solver="icem", control_bounds=(-1.0, 1.0),
        icem_kwargs=dict(num_samples=64, max_iter=2, seed=7), **more), N=N, M=M)
    config, plain, params, data = build()
    if not with_ensemble:
        return plain, params, data, None
    rng = np.random.default_rng(3)
    trees = []
    for scale in (0.3, 0.05, 0.1):
        tree = copy.deepcopy(params["dynamics_params"])
        for layer in tree["params"].values():
            layer["kernel"] = (np.asarray(layer["kernel"]) * rng.uniform(1 - scale, 1 + scale,
                                                                         np.shape(layer["kernel"]))).astype(np.float32)
        trees.append(tree)
    _, policy, params2, _ = build(dynamics_ensemble=trees)
    return policy, params2, data, [params_lib.tree_to_layers(t) for t in trees]


def _policy_problem(N, M, B):
    """The policy, its parameters and the first B problems whose rollouts are away from every member's kinks."""
    import test_gpu_mirror as mirror
    policy, params, data, members = _policy(N, M)
    idx = np.arange(12)
    pb = mirror._oracle_problem(params, data, idx, np.float32)
    pb["T"] = pb["U"].shape[1]
    Xm, _ = policy.plan_spread(params, pb["x0"], pb["U"])
    mem64 = [[(W.astype(np.float64), b.astype(np.float64)) for W, b in layers] for layers in members]
    ok = _kept(orc.cast_problem(pb, np.float64), mem64, Xm.cpu().numpy().astype(np.float64))
    assert ok.sum() >= B
    keep = np.flatnonzero(ok)[:B]
    for k in ("x0", "U", "goal"):
        pb[k] = np.ascontiguousarray(pb[k][keep])
    return policy, params, pb, members


def test_v8_the_layers_forward_and_backward():
    from gan_mpc_amd.policy import differentiable as dl
    policy, params, pb, members = _policy_problem(17, 6, 6)
    dparams = policy.to_device_params(params)
    dev = policy.device()
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    flat = dparams.flat.requires_grad_(True)
    x0, U, goal = (t(pb[k]).requires_grad_(True) for k in ("x0", "U", "goal"))
    mem = t(ec.flat(members)).requires_grad_(True)
    try:
        X, costs = dl.ensemble_rollout_layer(policy, dparams, x0, U, goal, members=mem)
        eng = policy._rollout_eng[1]
        direct = eng.ensemble_rollout(mem.detach(), x0.detach(), U.detach(), goal.detach(), want=("X", "costs"))
        _same(X.detach().cpu().numpy(), direct["X"].cpu().numpy(), "V8 forward X")
        _same(costs.detach().cpu().numpy(), direct["costs"].cpu().numpy(), "V8 forward costs")

        def loss(X, costs):
            J = costs.sum(-1)
            return J.mean(0).sum() + 0.5 * J.std(0, unbiased=False).sum() + 0.1 * X.var(0, unbiased=False).sum()

        loss(X, costs).backward()
        got = dict(x0=x0.grad, U=U.grad, goal=goal.grad, members=mem.grad)
        lo, cnt = dparams.range_of(("mpc_weights", "cost_params"))
        got["theta"] = flat.grad[lo:lo + cnt]
        dlo, dcnt = dparams.range_of(("dynamics_params",))
        assert not flat.grad[dlo:dlo + dcnt].any()               # the nominal network rolls nothing out here
        got = {k: v.cpu().numpy() for k, v in got.items()}
        # a member tensor that does not require grad gets none (and the policy's own ensemble is the default)
        mem2 = mem.detach().clone()
        U2 = U.detach().clone().requires_grad_(True)
        X2, c2 = dl.ensemble_rollout_layer(policy, dparams, x0.detach(), U2, goal.detach(), members=mem2)
        loss(X2, c2).backward()
        assert mem2.grad is None
        _same(U2.grad.cpu().numpy(), got["U"], "V8 U without the members' gradient")
        X3, _ = dl.ensemble_rollout_layer(policy, dparams, x0.detach(), U.detach(), goal.detach())
        _same(X3.detach().cpu().numpy(), X.detach().cpu().numpy(), "V8 the policy's ensemble")
    finally:
        flat.requires_grad_(False)
        flat.grad = None
    # The cotangents of the loss at the GPU's (X, costs) through the reference: everything in fp64 for the arbiter,
    # everything in fp32 for the fp32 oracle -- the loss's own backward too, as the layer's caller runs it: x_p - mean_p
    # and J_p - mean_p cancel among members a few per cent apart, which no fp32 evaluation of this loss escapes.
    Xn, cn = X.detach().cpu().numpy(), costs.detach().cpu().numpy()
    cots = {}
    for dt in (np.float32, np.float64):
        Xt = torch.as_tensor(Xn.astype(dt)).requires_grad_(True)
        ct = torch.as_tensor(cn.astype(dt)).requires_grad_(True)
        loss(Xt, ct).backward()
        cots[dt] = (Xt.grad.numpy(), ct.grad.numpy())
    r32 = vr.reference(pb, members, Xn, pb["U"], pb["goal"], *cots[np.float32])
    r64 = vr.reference(orc.cast_problem(pb, np.float64), members, Xn.astype(np.float64), pb["U"].astype(np.float64),
                       pb["goal"].astype(np.float64), *cots[np.float64])
    gu.set_config("ensemble rollout layer n=17 m=6")
    for key in KEYS:
        e = gu.assert_parity(f"ensemble rollout layer {key}", got[key], r32[key], r64[key], **_tol(key))
        print(f"V8 {key}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")


@pytest.mark.parametrize("aggregate,risk", [("mean", 0.0), ("mean_std", 0.5), ("max", 0.0)])
def test_v9_plan_risk_and_its_gradient_against_the_reference(aggregate, risk):
    policy, params, pb, members = _policy_problem(17, 6, 6)
    R, g = policy.plan_risk(params, pb["x0"], pb["U"], pb["goal"], aggregate=aggregate, risk=risk, grad=True)
    only = policy.plan_risk(params, pb["x0"], pb["U"], pb["goal"], aggregate=aggregate, risk=risk)
    _same(only.cpu().numpy(), R.cpu().numpy(), "V9 R with and without the gradient")
    X = policy.plan_spread(params, pb["x0"], pb["U"])[0].cpu().numpy()
    refs = {}
    for dt in (np.float32, np.float64):
        p = orc.cast_problem(pb, dt)
        costs = np.stack([orc.evaluate(p["cmlp"], p["mpc_w"], p["goal"], X[q].astype(dt), p["U"])
                          for q in range(len(members))])
        Rr, w = vr.risk(costs.sum(-1), aggregate, dt(risk))
        gc = np.ascontiguousarray(np.broadcast_to(w[:, :, None], costs.shape))
        refs[dt] = (Rr, vr.reference(p, members, X.astype(dt), p["U"], p["goal"], None, gc)["U"])
    gu.set_config(f"plan_risk {aggregate}")
    e = gu.assert_parity(f"plan_risk R {aggregate}", R.cpu().numpy(), refs[np.float32][0], refs[np.float64][0])
    f = gu.assert_parity(f"plan_risk dR/dU {aggregate}", g.cpu().numpy(), refs[np.float32][1], refs[np.float64][1])
    print(f"V9 {aggregate}: R HIP {e[0]:.3e} / fp32 {e[1]:.3e}, dR/dU HIP {f[0]:.3e} / fp32 {f[1]:.3e}")


@pytest.mark.parametrize("N,M", [(17, 6), (5, 2)])
def test_v9_refine_plan_lowers_the_risk_inside_the_bounds(N, M):
    policy, params, pb, _ = _policy_problem(N, M, 6)
    args = (params, pb["x0"], pb["U"], pb["goal"])
    U1, R0, R1 = policy.refine_plan(*args, steps=3, aggregate="mean_std", risk=0.5)
    R0, R1, U1 = R0.cpu().numpy(), R1.cpu().numpy(), U1.cpu().numpy()
    print(f"V9 refine_plan n={N}: R {R0} -> {R1}")
    assert np.all(R1 <= R0) and np.any(R1 < R0)
    assert U1.shape == pb["U"].shape and np.all(np.abs(U1) <= 1.0)
    again = policy.plan_risk(*args[:2], U1, pb["goal"], aggregate="mean_std", risk=0.5).cpu().numpy()
    _same(again, R1, "V9 R_after is the forward call's value at U'")
    U0, Ra, Rb = policy.refine_plan(*args, steps=0, aggregate="mean_std", risk=0.5)
    _same(U0.cpu().numpy(), pb["U"], "V9 steps=0")
    _same(Ra.cpu().numpy(), R0)
    _same(Rb.cpu().numpy(), R0)


def test_v9_both_raise_without_an_ensemble():
    plain, params, data, _ = _policy(5, 2, with_ensemble=False)
    x, U, goal = data["hist"][:2, -1], data["init_U"][:2], data["goal"][:2]
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        plain.plan_risk(params, x, U, goal)
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        plain.refine_plan(params, x, U, goal)
