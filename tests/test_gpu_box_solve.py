"""gmpc_ilqr_solve_box -- the one-launch iLQR solve under box bounds on the controls -- on the GPU, on the
inputs tests/box_cases.py fixes (checked on the CPU by tests/test_box_ilqr_host.py):

  G1  bounds that are never active (NULL, +-inf, +-1e30) give gmpc_ilqr_solve_fused bit for bit;
  G2  active bounds: feasibility, X / obj are the rollout of U, clamped rows of K are 0.0, k within the shifted bounds,
      no QP at its iteration cap;
  G3  one iteration under the decided protocol against the fp64 reference (tests/box_ilqr_ref.py);
  G4  the backward pass teacher-forced at the kernel's own iterate, against box_backward in fp32 and fp64;
  G5  the whole solve under the reference kwargs, cheetah T 5 at B 7 and B 128;
  G6  edges: lo == hi, one-sided bounds, a NaN start;
  G7  refusals;
  G8  determinism, alone and interleaved with the other two solves on the same ctx;
  G9  the policy interface."""

import functools

import numpy as np
import pytest
import torch

import box_cases as bc
import box_ilqr_ref as br
import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_control_flow as cf
import test_gpu_mirror as mirror
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.engine import TRAJAX_iLQR_KWARGS
from gan_mpc_amd.norm import l2_policy

pytestmark = pytest.mark.gpu
KEYS = ("X", "U", "obj", "grad", "adjoints", "iterations")


def _np(out):
    return {k: out[k].cpu().numpy().copy() for k in KEYS}


def _args(eng, pb, U=None):
    d = eng.to_dev
    return d(pb["x0"]), d(pb["U"] if U is None else U), d(pb["goal"])


def _box(eng, pb, lo, hi, kw, U=None):
    return _np(eng.ilqr_solve_box(*_args(eng, pb, U), lo, hi, kw))


def _qp_reports(eng, pb):
    B, T, m = pb["B"], pb["T"], pb["m"]
    return (eng.debug_buffer(15, (B, 2)).cpu().numpy(), eng.debug_buffer(16, (B, T)).cpu().numpy(),
            eng.debug_buffer(17, (B, T, m)).cpu().numpy() != 0)


# ---- G1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "cheetah", "wide_m"])
def test_g1_inactive_bounds_are_the_fused_solve_bit_for_bit(name):
    pb = bc.problem(name)
    kw = {"maxiter": bc.MAXITER}
    eng = gu.engine_for(pb, critic=False)
    try:
        fused = _np(eng.ilqr_solve_fused(*_args(eng, pb), kw))
        alpha = eng.debug_buffer(8, (pb["B"],)).cpu().numpy()
        assert (fused["iterations"] > 1).any()
        m = pb["m"]
        for lo, hi in ((None, None), (-np.inf, np.inf), (-1e30, 1e30), (np.full(m, -np.inf), None)):
            box = _box(eng, pb, lo, hi, kw)
            for k in KEYS:
                np.testing.assert_array_equal(box[k], fused[k], err_msg=f"{name} bounds {lo}/{hi}: {k}")
            np.testing.assert_array_equal(eng.debug_buffer(8, (pb["B"],)).cpu().numpy(), alpha)
            count, _, clamped = _qp_reports(eng, pb)
            assert (count[:, 0] == 0).all() and not clamped.any()
    finally:
        eng.close()


# ---- G2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.TABLE)
def test_g2_active_bounds_feasible_and_consistent(name):
    pb, b = bc.problem(name), bc.bound(name)
    pb64 = orc.cast_problem(pb, np.float64)
    B, T, n, m = pb["B"], pb["T"], pb["n"], pb["m"]
    gu.set_config(f"box G2 {name} n={n} m={m} T={T} B={B}")
    eng = gu.engine_for(pb, critic=False)
    try:
        out = _box(eng, pb, -b, b, {"maxiter": bc.MAXITER})
        count, qp_iters, clamped = _qp_reports(eng, pb)
        K = eng.debug_buffer(6, (B, T, m, n)).cpu().numpy()
        k = eng.debug_buffer(7, (B, T, m)).cpu().numpy()
        U = out["U"]
        lo, hi = np.float32(-b), np.float32(b)
        assert (U >= lo).all() and (U <= hi).all()
        assert ((U == lo) | (U == hi)).mean() > 0.1
        # X and obj are the rollout of U and the sum of its costs
        Xd, costs = eng.rollout_cost(eng.to_dev(pb["x0"]), eng.to_dev(U), eng.to_dev(pb["goal"]))
        U64 = U.astype(np.float64)
        X64 = orc.rollout(pb64["dyn"], U64, pb64["x0"])
        gu.assert_parity(f"box X vs rollout_cost {name}", out["X"], Xd.cpu().numpy(), X64)
        gu.assert_parity(f"box obj vs rollout_cost {name}", out["obj"], costs.cpu().numpy().sum(1),
                         orc.evaluate(pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X64, U64).sum(1))
        # the gains the ctx holds were computed at the final U and not applied yet
        assert clamped.any()
        assert (K[clamped] == 0.0).all()
        assert (k >= lo - U).all() and (k <= hi - U).all()
        assert (count[:, 0] == 0).all(), count
        assert (qp_iters >= 1).all() and (qp_iters <= br.QP_ITERS).all()
    finally:
        eng.close()


# ---- G3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.TABLE)
def test_g3_one_iteration_under_the_decided_protocol(name):
    pb, b = bc.problem(name), bc.bound(name)
    B = pb["B"]
    gu.set_config(f"box G3 {name} n={pb['n']} m={pb['m']} T={pb['T']} B={B}")
    agree = bc.decided(name, 1)
    min_agree = bc.MIN_AGREE[name]
    gu._record(dict(stage=f"box {name}: share of trajectories whose control flow is decided (required {min_agree})",
                    config=gu.CURRENT_CONFIG[0], e_hip=float(agree.mean()), e_o32=None, tol=min_agree,
                    tol_used=min_agree, branch="info", entries=int(B), passed=bool(agree.mean() >= min_agree)))
    assert agree.mean() >= min_agree
    ref = bc.reference(name, 1)
    (r64, t64), (r32, _) = ref["o64"], ref["o32"]
    eng = gu.engine_for(pb, critic=False)
    try:
        out = _box(eng, pb, -b, b, {"maxiter": 1})
        alpha = eng.debug_buffer(8, (B,)).cpu().numpy()
        np.testing.assert_array_equal(out["iterations"][agree], r64[6][agree])
        a64 = cf._alphas(t64, B)
        for i in np.nonzero(agree)[0]:
            if len(a64[i]) >= 1:
                assert alpha[i] == np.float32(a64[i][0]), (name, i, alpha[i], a64[i])
        np.testing.assert_array_equal(bc.at_bound(out["U"], np.float32(-b), np.float32(b))[agree],
                                      bc.at_bound(r64[1], -b, b)[agree])
        fin = agree & np.isfinite(r64[2])
        if fin.any():
            for key, j in (("U", 1), ("X", 0)):
                gu.assert_parity(f"box {name} {key} (1 iteration)", out[key][fin], r32[j][fin], r64[j][fin], tol=1e-4,
                                 ceiling=gu.GAIN_CEILING, el_tol=1.0)
            gu.assert_parity(f"box {name} obj (1 iteration)", out["obj"][fin], r32[2][fin], r64[2][fin], tol=1e-4,
                             ceiling=gu.GAIN_CEILING)
    finally:
        eng.close()


# ---- G4 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxiter", [1, 3])
@pytest.mark.parametrize("name", ["base", "m1", "cheetah"])
def test_g4_teacher_forced_backward_pass(name, maxiter):
    pb, b = bc.problem(name), bc.bound(name)
    pb64 = orc.cast_problem(pb, np.float64)
    B, T, n, m = pb["B"], pb["T"], pb["n"], pb["m"]
    gu.set_config(f"box G4 {name} maxiter={maxiter}")
    eng = gu.engine_for(pb, critic=False)
    try:
        out = _box(eng, pb, -b, b, {"maxiter": maxiter})
        _, _, clamped = _qp_reports(eng, pb)
        K = eng.debug_buffer(6, (B, T, m, n)).cpu().numpy()
        k = eng.debug_buffer(7, (B, T, m)).cpu().numpy()
    finally:
        eng.close()
    X, U = out["X"], out["U"]
    X64, U64 = X.astype(np.float64), U.astype(np.float64)
    l32 = orc.get_lqr_params(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], X, U)
    l64 = orc.get_lqr_params(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X64, U64)
    b32 = br.box_backward(l32, U, np.float32(-b), np.float32(b))
    b64 = br.box_backward(l64, U64, -b, b)
    ok = ~(gu.dyn_near_kink(pb64["dyn"], X64, U64).any(1) | gu.near_kink(pb64["cmlp"], X64[:, T]))
    ok &= (clamped == b64["clamped"]).all(axis=(1, 2)) & (b32["clamped"] == b64["clamped"]).all(axis=(1, 2))
    ok &= ((b64["margin_mult"] > bc.MARGIN) & (b64["margin_clear"] > bc.MARGIN) & ~b64["capped"]).all(axis=1)
    assert ok.sum() * 2 >= B, (name, maxiter, ok)
    g32, a32 = orc.adjoint(l32[5], l32[6], l32[1], l32[3])
    g64, a64 = orc.adjoint(l64[5], l64[6], l64[1], l64[3])
    gu.assert_parity(f"box grad {name}", out["grad"][ok], g32[ok], g64[ok])
    gu.assert_parity(f"box adjoints {name}", out["adjoints"][ok], a32[ok], a64[ok])
    gu.assert_parity(f"box K {name}", K[ok], b32["K"][ok], b64["K"][ok], ceiling=gu.GAIN_CEILING, el_tol=1.0)
    gu.assert_parity(f"box k {name}", k[ok], b32["k"][ok], b64["k"][ok], ceiling=gu.GAIN_CEILING, el_tol=1.0)


@pytest.mark.parametrize("name", sorted(bc.STEP_MIN_AGREE))
def test_g4_first_backward_pass_step_by_step(name):
    """maxiter 0: one backward pass at clamp(U_init), no control flow -- the check of the m = 32 QP that does not need a
    whole trajectory to be decided (tests/box_cases.py: first_pass)."""
    pb, b = bc.problem(name), bc.bound(name)
    B, T, n, m = pb["B"], pb["T"], pb["n"], pb["m"]
    gu.set_config(f"box G4 first pass {name} n={n} m={m} T={T} B={B}")
    fp = bc.first_pass(name)
    b32, b64, dec = fp["b32"], fp["b64"], fp["decided"]
    gu._record(dict(stage=f"box {name}: share of steps of the first backward pass that are decided "
                          f"(required {bc.STEP_MIN_AGREE[name]})", config=gu.CURRENT_CONFIG[0],
                    e_hip=float(dec.mean()), e_o32=None, tol=bc.STEP_MIN_AGREE[name], tol_used=bc.STEP_MIN_AGREE[name],
                    branch="info", entries=int(dec.size), passed=bool(dec.mean() >= bc.STEP_MIN_AGREE[name])))
    assert dec.mean() >= bc.STEP_MIN_AGREE[name]
    eng = gu.engine_for(pb, critic=False)
    try:
        out = _box(eng, pb, -b, b, {"maxiter": 0})
        count, qp_iters, clamped = _qp_reports(eng, pb)
        K = eng.debug_buffer(6, (B, T, m, n)).cpu().numpy()
        k = eng.debug_buffer(7, (B, T, m)).cpu().numpy()
    finally:
        eng.close()
    assert (out["iterations"] == 0).all() and (count[:, 0] == 0).all()
    np.testing.assert_array_equal(out["U"], br.clamp(pb["U"], np.float32(-b), np.float32(b)))
    # the minimiser is continuous in the data: every step
    gu.assert_parity(f"box first pass k {name}", k, b32["k"], b64["k"], ceiling=gu.GAIN_CEILING, el_tol=1.0)
    # the clamped set, the QP's iteration count and the gains: the decided steps
    np.testing.assert_array_equal(clamped[dec], b64["clamped"][dec])
    same_count = dec & (b32["qp_iters"] == b64["qp_iters"])
    assert same_count.any()
    np.testing.assert_array_equal(qp_iters[same_count], b64["qp_iters"][same_count])
    assert (K[dec][b64["clamped"][dec]] == 0.0).all()
    gu.assert_parity(f"box first pass K {name}", K[dec], b32["K"][dec], b64["K"][dec], ceiling=gu.GAIN_CEILING,
                     el_tol=1.0)


# ---- G5 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cheetah", "cheetah128"])
def test_g5_whole_solve_under_the_reference_kwargs(name):
    pb, b = bc.problem(name), bc.bound(name)
    ref = bc.whole_solve_reference(name)
    gu.set_config(f"box G5 {name} B={pb['B']}")
    eng = gu.engine_for(pb, critic=False)
    try:
        out = _box(eng, pb, -b, b, dict(TRAJAX_iLQR_KWARGS))
        count, _, _ = _qp_reports(eng, pb)
    finally:
        eng.close()
    fin = np.isfinite(ref["obj64"])
    assert fin.any()
    assert np.isfinite(out["obj"][fin]).all()
    assert (np.abs(out["U"][fin]) <= np.float32(b)).all()
    assert (count[:, 0] == 0).all()
    e_hip = float((np.abs(out["obj"][fin] - ref["obj64"][fin]) / np.abs(ref["obj64"][fin])).max())
    e_o32 = float((np.abs(ref["obj32"][fin] - ref["obj64"][fin]) / np.abs(ref["obj64"][fin])).max())
    gu._record(dict(stage=f"box whole solve obj {name} (max relative difference to the fp64 reference)",
                    config=gu.CURRENT_CONFIG[0], e_hip=e_hip, e_o32=e_o32, tol=4 * e_o32, tol_used=4 * e_o32,
                    branch="slack", entries=int(fin.sum()), passed=bool(e_hip <= 4 * e_o32)))
    print(f"G5 {name}: kernel vs fp64 {e_hip:.3e}, fp32 reference vs fp64 {e_o32:.3e}")
    assert e_hip <= 4 * e_o32, (name, e_hip, e_o32)


# ---- G6 --------------------------------------------------------------------------------------------------------------
def test_g6_equal_bounds_pin_the_controls():
    pb = bc.problem("base")
    B, T, n, m = pb["B"], pb["T"], pb["n"], pb["m"]
    v = np.array([0.05, -0.02], np.float32)
    eng = gu.engine_for(pb, critic=False)
    try:
        out = _box(eng, pb, v, v, {"maxiter": 3})
        assert (out["U"] == v).all()
        assert (eng.debug_buffer(6, (B, T, m, n)).cpu().numpy() == 0.0).all()
        assert (eng.debug_buffer(7, (B, T, m)).cpu().numpy() == 0.0).all()
        assert np.isfinite(out["obj"]).all()
    finally:
        eng.close()


@pytest.mark.parametrize("side", ["lower", "upper"])
def test_g6_one_sided_bounds(side):
    pb, b = bc.problem("base"), bc.bound("base")
    lo, hi = (-b, None) if side == "lower" else (None, b)
    eng = gu.engine_for(pb, critic=False)
    try:
        out = _box(eng, pb, lo, hi, {"maxiter": bc.MAXITER})
        U = out["U"]
        if side == "lower":
            assert (U >= np.float32(-b)).all() and (U == np.float32(-b)).any()
        else:
            assert (U <= np.float32(b)).all() and (U == np.float32(b)).any()
        one = _box(eng, pb, lo, hi, {"maxiter": 1})
        assert (one["obj"] < _box(eng, pb, lo, hi, {"maxiter": 0})["obj"]).all()
    finally:
        eng.close()


def test_g6_nan_start_never_iterates_and_neighbours_do():
    pb, b = bc.problem("base"), bc.bound("base")
    U = pb["U"].copy()
    U[1, 2, 0] = np.nan
    eng = gu.engine_for(pb, critic=False)
    try:
        out = _box(eng, pb, -b, b, {"maxiter": 4}, U=U)
        ref = _box(eng, pb, -b, b, {"maxiter": 4})
        it = out["iterations"]
        assert it[1] == 0 and it[0] > 0 and it[2] > 0
        assert np.isnan(out["obj"][1])
        for k in KEYS:
            np.testing.assert_array_equal(out[k][[0, 2]], ref[k][[0, 2]])
    finally:
        eng.close()


# ---- G7 --------------------------------------------------------------------------------------------------------------
def _solve_box(pb, kw=None, B=None, lo=-0.5, hi=0.5):
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        B = pb["B"] if B is None else B
        x0 = np.resize(pb["x0"], (B,) + pb["x0"].shape[1:])
        U = np.resize(pb["U"], (B,) + pb["U"].shape[1:])
        goal = np.resize(pb["goal"], (B,) + pb["goal"].shape[1:])
        return eng.ilqr_solve_box(d(x0), d(U), d(goal), lo, hi, kw)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n65", "m33", "T33"])
def test_g7_refused_shapes(case):
    args = dict(lstm=dict(n=3, m=1, T=5, dyn_hidden=(16,), dyn_lstm=8), n65=dict(n=65, m=2, T=3),
                m33=dict(n=4, m=33, T=3), T33=dict(n=3, m=1, T=33))[case]
    n, m, T = args.pop("n"), args.pop("m"), args.pop("T")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, T, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    with pytest.raises(GmpcError, match="box solve"):
        _solve_box(pb, {"maxiter": 2})


def test_g7_refused_options_batch_and_bounds():
    pb = gu.problem(3, 1, 5, 2, seed=1, dyn_hidden=(32, 32), cost_hidden=(16,), cost_fout=4)
    with pytest.raises(GmpcError, match="make_psd"):
        _solve_box(pb, {"make_psd": True})
    with pytest.raises(GmpcError, match="box solve"):
        _solve_box(pb, {"alpha_0": 1.0, "alpha_min": 1e-6})     # 20 halvings
    with pytest.raises(GmpcError, match="max_batch"):
        _solve_box(pb, {"maxiter": 2}, B=3)
    with pytest.raises(GmpcError, match="u_lo must be <= u_hi"):
        _solve_box(pb, {"maxiter": 2}, lo=0.2, hi=0.1)


def test_g7_no_bilevel_tail_after_a_box_solve():
    pb = bc.problem("m1")
    B = pb["B"]
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        eng.ilqr_solve_fused(*_args(eng, pb), {"maxiter": 1})          # a held solution the box solve has to drop
        eng.ilqr_solve_box(*_args(eng, pb), -0.1, 0.1, {"maxiter": 1})
        with pytest.raises(GmpcError, match="must precede"):
            eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
        with pytest.raises(GmpcError, match="must precede"):
            eng.upper_loss(B, 0, desired=d(pb["true_seq"]))
        with pytest.raises(GmpcError, match="must precede"):
            eng.bilevel_grad_cotangent(B, lx=d(np.zeros((B, pb["T"] + 1, pb["n"]), np.float32)))
    finally:
        eng.close()


# ---- G8 --------------------------------------------------------------------------------------------------------------
def test_g8_deterministic_and_independent_of_the_other_solves():
    pb, b = bc.problem("cheetah"), bc.bound("cheetah")
    kw = {"maxiter": bc.MAXITER}

    def run(seq):
        eng = gu.engine_for(pb, critic=False)
        try:
            a = _args(eng, pb)
            call = {"b": lambda: eng.ilqr_solve_box(*a, -b, b, kw), "f": lambda: eng.ilqr_solve_fused(*a, kw),
                    "r": lambda: eng.ilqr_solve(*a, kw)}
            return [_np(call[s]()) for s in seq]
        finally:
            eng.close()

    def equal(x, y, what):
        for k in KEYS:
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{what}: {k}")

    b1, b2 = run("bb")
    equal(b1, b2, "two box solves")
    f1, b3, f2 = run("fbf")
    equal(f2, f1, "fused after a box solve")
    equal(b3, b1, "box after a fused solve")
    r1, b4, r2 = run("rbr")
    equal(r2, r1, "round-based after a box solve")
    equal(b4, b1, "box after a round-based solve")
    torch.cuda.synchronize()


# ---- G9 --------------------------------------------------------------------------------------------------------------
def test_g9_policy_action_is_the_first_control_of_the_box_solve():
    config, policy, params, data = mirror._build(functools.partial(l2_policy.L2MPC, solver="box",
                                                                   control_bounds=(-0.3, 0.3)))
    assert policy.solver == "box"
    policy.expert_model.select(np.array([2]))
    a = policy.get_optimal_action(params, data["hist"][2])
    eng = policy._engine
    U = eng.debug_buffer(1, (1, eng.T, eng.m)).cpu().numpy()
    a = a.cpu().numpy()
    np.testing.assert_array_equal(a, U[0, 0])
    assert (a >= np.float32(-0.3)).all() and (a <= np.float32(0.3)).all()
    count = eng.debug_buffer(15, (1, 2)).cpu().numpy()
    assert count[0, 0] == 0 and count[0, 1] >= eng.T
    # (this problem's optimal controls are ~1e-2: under +-0.3 no bound is active at the solution; a tight box is)
    tight = np.float32(1e-3)
    config, policy, params, data = mirror._build(functools.partial(l2_policy.L2MPC, solver="box",
                                                                   control_bounds=(-float(tight), float(tight))))
    policy.expert_model.select(np.array([2]))
    a = policy.get_optimal_action(params, data["hist"][2]).cpu().numpy()
    U = policy._engine.debug_buffer(1, (1, eng.T, eng.m)).cpu().numpy()
    np.testing.assert_array_equal(a, U[0, 0])
    assert (np.abs(U) <= tight).all() and (np.abs(U) == tight).any()
