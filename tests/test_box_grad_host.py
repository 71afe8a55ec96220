"""Bilevel gradients through box-constrained iLQR solutions (gmpc_ilqr_solve_box_held) without a device:

  1. the structured masked solve of tests/box_grad_ref.py against the dense one, in fp64;
  2. the implicit-function formula with the masked solve against central differences of Newton-polished fp64 box
     solutions (the helper and tolerances of tests/test_input_grads_host.py, the polish on the free set);
  3. the C ABI, the ctypes table, the Engine and the solver dispatch of the new entry point;
  4. the inputs of tests/test_gpu_box_grad.py: the share of clamped controls of the reference solutions."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import box_cases as bc
import box_grad_ref as bg
import gan_mpc_oracle as orc
import torch_ref as tr
from gan_mpc_amd import _lib
from gan_mpc_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. masked solve against the dense solve -----------------------------------------------------------------------
def _lq(name):
    pb = orc.cast_problem(bc.problem(name), np.float64)
    X = orc.rollout(pb["dyn"], pb["U"], pb["x0"])
    lqr = orc.get_lqr_params(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], X, pb["U"])
    rng = np.random.default_rng(4)
    return pb, lqr, rng.standard_normal(pb["U"].shape)


@pytest.mark.parametrize("name", ["base", "m1"])
def test_masked_solve_equals_the_dense_solve_on_the_free_set(name):
    pb, lqr, Bv = _lq(name)
    B, T, m = Bv.shape
    rng = np.random.default_rng(11)
    for share in (0.25, 0.5, 0.75):
        cl = rng.random((B, T, m)) < share
        cl[0, T - 1] = True         # an all-clamped and an all-free step in every draw
        cl[0, 0] = False
        assert cl.any() and not cl.all()
        H, dX = bg.masked_hessian_solve(lqr, Bv, cl)
        Hd = bg.dense_masked_solve(lqr, Bv, cl)
        assert (H[cl] == 0).all()
        np.testing.assert_allclose(H, Hd, rtol=0, atol=1e-9 * np.abs(Hd).max())
        assert bg.free_residual(lqr, H, Bv, cl).max() < 1e-10
        # dX is the tangent roll of H
        dx = np.zeros_like(dX)
        for t in range(T):
            dx[:, t + 1] = (np.einsum("bij,bj->bi", lqr[5][:, t], dx[:, t])
                            + np.einsum("bnm,bm->bn", lqr[6][:, t], H[:, t]))
        np.testing.assert_allclose(dX, dx, rtol=0, atol=1e-12 * max(np.abs(dx).max(), 1.0))


@pytest.mark.parametrize("name", ["base", "m1"])
def test_all_free_is_the_oracles_solve_and_all_clamped_is_zero(name):
    pb, lqr, Bv = _lq(name)
    H0, dX0 = orc.hessian_solve(lqr, Bv)
    H, dX = bg.masked_hessian_solve(lqr, Bv, np.zeros(Bv.shape, bool))
    np.testing.assert_allclose(H, H0, rtol=0, atol=1e-12 * np.abs(H0).max())
    np.testing.assert_allclose(dX, dX0, rtol=0, atol=1e-12 * np.abs(dX0).max())
    cl = np.zeros(Bv.shape, bool)
    cl[1] = True                    # one trajectory all clamped
    H, dX = bg.masked_hessian_solve(lqr, Bv, cl)
    assert (H[1] == 0).all() and (dX[1] == 0).all()
    np.testing.assert_allclose(H[0], H0[0], rtol=0, atol=1e-12 * np.abs(H0).max())


def test_clamped_set_and_its_words():
    U = np.array([[[-1.0, 0.5, 1.0], [1.0, -1.0, np.nan]]], np.float32)
    g = np.array([[[2.0, 1.0, -1.0], [1.0, -1.0, 1.0]]], np.float32)
    cl = bg.clamped_set(U, g, -1.0, 1.0)
    # at lo with g > 0; free; at hi with g < 0 / at hi with g > 0: free; at lo with g < 0: free; NaN: free
    np.testing.assert_array_equal(cl, [[[True, False, True], [False, False, False]]])
    np.testing.assert_array_equal(bg.words(cl), [[0b101, 0]])
    np.testing.assert_array_equal(bg.clamped_set(U, g, None, 1.0), [[[False, False, True], [False, False, False]]])
    g[0, 0, 0] = np.nan
    assert not bg.clamped_set(U, g, -1.0, 1.0)[0, 0, 0]
    wide = np.ones((1, 1, 32), bool)
    assert bg.words(wide)[0, 0] == 0xFFFFFFFF


# ---- 2. the implicit-function formula against central differences --------------------------------------------------
def _polish(pb, x0, goal, U, cl):
    """Newton steps on J over the free controls, the clamped ones left on their bounds (test_input_grads_host._solve
    on the free set).  -> (X, U, full gradient dJ/dU) as arrays; the free gradient below 1e-12."""
    T, m = pb["T"], pb["m"]
    dyn, cm, mw = tr.layers64(pb["dyn"]), tr.layers64(pb["cmlp"]), tr.t64(pb["mpc_w"])
    x0t, gt = tr.t64(x0), tr.t64(goal)
    J = lambda u: tr.objective(dyn, cm, mw, gt, u.reshape(T, m), x0t)  # noqa: E731
    u = tr.t64(U).reshape(-1).clone()
    f = torch.as_tensor(~cl.reshape(-1))
    for _ in range(4):
        if not bool(f.any()):
            break
        A = torch.autograd.functional.hessian(J, u)
        g = torch.autograd.functional.jacobian(J, u)
        u[f] = u[f] - torch.linalg.solve(A[f][:, f], g[f])
    g = torch.autograd.functional.jacobian(J, u)
    assert float(g[f].norm()) < 1e-12 if bool(f.any()) else True
    Un = u.reshape(T, m)
    return tr.rollout(dyn, Un, x0t).numpy(), Un.numpy(), g.reshape(T, m).numpy()


def _set_is_valid(U, g, cl, b):
    """strict complementarity: clamped controls on a bound with a multiplier pushing against it, free ones inside"""
    at_lo, at_hi = cl & (U == -b), cl & (U == b)
    return bool((at_lo | at_hi)[cl].all() and (g[at_lo] > 0).all() and (g[at_hi] < 0).all()
                and (np.abs(U[~cl]) < b).all())


# trajectories the fp64 box solve brings to a smooth stationary point (the others stall at a relu kink, as most tiny
# relu problems do -- test_input_grads_host._problem): 4 of 7 and 1 of 3
@pytest.mark.parametrize("name,min_count", [("m1", 4), ("base", 1)])
def test_masked_formula_matches_finite_differences_of_the_box_solution(name, min_count):
    pb = orc.cast_problem(bc.problem(name), np.float64)
    b = float(bc.bound(name))
    T, n = pb["T"], pb["n"]
    r, _ = bc.run(pb, np.float64, -b, b, {"maxiter": 300, "grad_norm_threshold": 1e-12})
    U0, grad0 = r[1], r[3]
    cl0 = bg.clamped_set(U0, grad0, -b, b)
    free_norm = np.sqrt((np.where(cl0, 0.0, grad0) ** 2).sum((1, 2)))
    idx = np.nonzero(free_norm < 1e-6)[0]
    assert len(idx) >= min_count, free_norm
    seen_free = seen_clamped = 0
    seen_goal = False
    for i in idx:
        x0, goal, des, cl = pb["x0"][i], pb["goal"][i], pb["true_seq"][i], cl0[i]
        X, U, g = _polish(pb, x0, goal, U0[i], cl)
        # strict complementarity, with room for the perturbed solves
        assert _set_is_valid(U, g, cl, b)
        assert np.abs(g[cl]).min() > 1e-3 and (b - np.abs(U[~cl])).min() > 1e-3 * b
        seen_free += int((~cl).sum())
        seen_clamped += int(cl.sum())
        one = dict(pb, x0=x0[None], goal=goal[None], true_seq=des[None], B=1)
        lx = orc.l2_loss_grad_x(X[None], des[None])
        ref = bg.gradients(one, X[None], U[None], lx, None, cl[None])
        assert (ref["H"][0][cl] == 0).all()

        def L_at(p=pb, x0_=x0, goal_=goal):
            Xp, Up, gp = _polish(p, x0_, goal_, U, cl)
            assert _set_is_valid(Up, gp, cl, b)
            return float(orc.l2_loss(Xp[None], des[None])[0])

        eps = 1e-5

        def fd(plus, minus):
            return (L_at(**plus) - L_at(**minus)) / (2 * eps)

        # mpc_w (every entry): dL/dw = -d/dw [H . grad_U J]
        for j in range(3):
            e = np.zeros(3)
            e[j] = eps
            d = fd(dict(p=dict(pb, mpc_w=pb["mpc_w"] + e)), dict(p=dict(pb, mpc_w=pb["mpc_w"] - e)))
            np.testing.assert_allclose(-ref["theta"][j], d, rtol=1e-5, atol=1e-9, err_msg=f"{name}[{i}] mpc_w[{j}]")
        # one x0 entry and one goal entry (the tolerances of test_input_grads_host)
        e = np.zeros(n)
        e[0] = eps
        d = fd(dict(x0_=x0 + e), dict(x0_=x0 - e))
        np.testing.assert_allclose(ref["x0"][0, 0], d, rtol=0, atol=1e-6 * abs(d) + 1e-9, err_msg=f"{name}[{i}] x0")
        # (goal row t reaches L through dX_t only: the row behind the first free control, where dX is not 0)
        tg = min(int(np.nonzero((~cl).any(-1))[0][0]) + 1, T - 1)
        e = np.zeros_like(goal)
        e[tg, 0] = eps
        d = fd(dict(goal_=goal + e), dict(goal_=goal - e))
        np.testing.assert_allclose(ref["goal"][0, tg, 0], d, rtol=0, atol=1e-4 * abs(d) + 1e-9,
                                   err_msg=f"{name}[{i}] goal")
        seen_goal = seen_goal or abs(d) > 1e-6
        # one dynamics weight: the last layer's, from the hidden unit most active at step 0 to output 0 (a weight
        # behind an inactive unit has a zero gradient whatever the formula)
        a = np.concatenate([X[0], U[0]])
        for W, bias in pb["dyn"][:-1]:
            a = np.maximum(a @ W + bias, 0.0)
        k = int(np.argmax(a))
        assert a[k] > 0

        def with_weight(delta):
            dyn = [(W.copy(), bias.copy()) for W, bias in pb["dyn"]]
            dyn[-1][0][k, 0] += delta
            return dict(pb, dyn=dyn)

        d = fd(dict(p=with_weight(eps)), dict(p=with_weight(-eps)))
        off = sum(W.size + bias.size for W, bias in pb["dyn"][:-1])
        got = ref["dyn"][off + k * pb["dyn"][-1][0].shape[1]]
        np.testing.assert_allclose(got, d, rtol=1e-5, atol=1e-8, err_msg=f"{name}[{i}] dynamics weight")
    assert seen_free > 0 and seen_clamped > 0
    assert seen_goal or name == "base"       # (base: the one free control is the last step's)


# ---- 3. the C ABI, the ctypes table, the Engine, the dispatch ------------------------------------------------------
def _header_params(name):
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1) for p in m.group(1).split(",")]


def test_library_exports_the_held_box_solve():
    assert re.fullmatch(r"gmpc_[a-z_]+", "gmpc_ilqr_solve_box_held")
    assert hasattr(_lib.load(), "gmpc_ilqr_solve_box_held")


def test_header_signature_and_engine_agree_on_the_argument_order():
    assert _header_params("gmpc_ilqr_solve_box_held") == _header_params("gmpc_ilqr_solve_box")
    assert _lib.SIGNATURES["gmpc_ilqr_solve_box_held"] == _lib.SIGNATURES["gmpc_ilqr_solve_box"]
    assert _lib.SIGNATURES["gmpc_ilqr_solve_box_held"][0] is C.c_int
    assert (list(inspect.signature(Engine.ilqr_solve_box_held).parameters)
            == list(inspect.signature(Engine.ilqr_solve_box).parameters)
            == ["self", "x0", "U", "goal", "u_lo", "u_hi", "kwargs"])

    class Lib:      # records what the engine hands to the entry points
        def __init__(self):
            self.calls = []

        def gmpc_ilqr_solve_box(self, *a):
            self.calls.append(("box", a))
            return 0

        def gmpc_ilqr_solve_box_held(self, *a):
            self.calls.append(("held", a))
            return 0

    eng = object.__new__(Engine)
    eng.lib, eng.ctx, eng.n, eng.m, eng.T, eng.solve_count = Lib(), None, 3, 2, 4, 0
    eng.new = lambda *shape, dtype=None: None
    uploads = []
    eng.to_dev = lambda a: uploads.append(1) or tuple(float(v) for v in a)
    eng._stream = lambda: "stream"
    import gan_mpc_amd.engine as engine_mod
    orig = engine_mod._ptr
    engine_mod._ptr = lambda t: t
    try:
        eng.ilqr_solve_box_held(np.zeros((5, 3)), "U", "goal", -0.5, [1.0, np.inf])
        eng.ilqr_solve_box(np.zeros((5, 3)), "U", "goal", -0.5, [1.0, np.inf])
    finally:
        engine_mod._ptr = orig
    (k0, a), (k1, a1) = eng.lib.calls
    assert (k0, k1) == ("held", "box") and len(a) == len(a1) and a[12:] == a1[12:]
    assert len(a) == len(_lib.SIGNATURES["gmpc_ilqr_solve_box_held"][1])
    assert a[1] == 5 and a[3] == "U" and a[4] == "goal" and a[12] == "stream"
    assert a[13] == (-0.5, -0.5) and a[14] == (1.0, float("inf"))
    assert len(uploads) == 2 and eng.solve_count == 2      # one cache of device bounds serves both


def test_engine_refuses_bad_bounds_before_any_launch():
    eng = object.__new__(Engine)
    eng.m = 2
    eng.lib = None          # any call through the ABI would fail
    with pytest.raises(_lib.GmpcError, match="u_lo must be <= u_hi"):
        eng.ilqr_solve_box_held(None, None, None, 0.3, -0.3)
    with pytest.raises(_lib.GmpcError, match="2 values"):
        eng.ilqr_solve_box_held(None, None, None, [0.0, 0.0, 0.0], None)


def test_solver_dispatch_holds_only_when_asked():
    from gan_mpc_amd.policy import optimizers as opt

    class Eng:
        def ilqr_solve_box(self, x0, U, goal, lo, hi, kwargs=None):
            return ("box", x0, U, goal, lo, hi, kwargs)

        def ilqr_solve_box_held(self, x0, U, goal, lo, hi, kwargs=None):
            return ("held", x0, U, goal, lo, hi, kwargs)

        ilqr_solve = ilqr_solve_fused = None

    class Policy:
        solver, control_bounds = "box", (-0.3, 0.4)

    assert list(inspect.signature(opt._solver).parameters) == ["policy", "eng", "hold"]
    assert inspect.signature(opt._solver).parameters["hold"].default is False
    want = ("x0", "U", "goal", -0.3, 0.4, {"maxiter": 2})
    assert opt._solver(Policy(), Eng())("x0", "U", "goal", {"maxiter": 2}) == ("box",) + want
    assert opt._solver(Policy(), Eng(), hold=True)("x0", "U", "goal", {"maxiter": 2}) == ("held",) + want
    Policy.solver = "fused"
    assert opt._solver(Policy(), Eng(), hold=True) is None       # the other solvers always hold: nothing to select
    assert inspect.signature(opt.ilqr_solve).parameters["hold"].default is False
    from gan_mpc_amd.policy.eval import EvalMPC
    assert inspect.signature(EvalMPC._solve).parameters["hold"].default is False


def test_training_calls_hold_and_the_action_path_does_not():
    """bilevel_optimization, ILQRFunction.forward and batch_loss select the held solve; get_optimal_values the plain."""
    from gan_mpc_amd.policy import base, differentiable, eval as ev, optimizers as opt
    assert "hold=True" in inspect.getsource(opt.bilevel_optimization)
    assert "hold=True" in inspect.getsource(differentiable.ILQRFunction.forward)
    assert "hold=True" in inspect.getsource(base.BaseMPC.batch_loss)
    assert "hold" not in inspect.getsource(ev.EvalMPC.get_optimal_values)


# ---- 4. the inputs of the GPU tests --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.TABLE)
def test_gpu_inputs_are_fixed_here(name):
    """The clamped-set share of the fp32 and the fp64 reference solution of every case lies in [0.2, 0.8] (measured:
    base 0.58 / 0.60, m1 0.46, cheetah 0.51 / 0.52, wide_m 0.38, wide_n 0.67)."""
    b = bc.bound(name)
    ref = bc.reference(name)
    for tag, dt in (("o32", np.float32), ("o64", np.float64)):
        r = ref[tag][0]
        cl = bg.clamped_set(r[1], r[3], dt(-b), dt(b))
        share = float(cl.mean())
        assert 0.2 <= share <= 0.8, (name, tag, share)
        if name == "m1":
            per_step = cl.reshape(-1, cl.shape[-1])
            assert per_step.all(-1).any() and (~per_step).all(-1).any()
