"""CPU side of gmpc_bilevel_grad_inputs (dL/dx0 and dL/dgoal through the iLQR solution): the ABI entry against the
header and _lib.SIGNATURES, the Engine method and the torch layer, and the derivation itself -- the dense fp64 formula

    dL/dp = dL/dp|_(U fixed) - d/dp [ H . grad_U J ],   H = (d^2 J / dU^2)^{-1} dL/dU  (held fixed)

built with torch autograd, against central finite differences of L at the fp64 oracle's iLQR solution."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import torch_ref as tr
from gan_mpc_amd import _lib
from gan_mpc_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_exported_and_its_signature_matches_the_header():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert hasattr(lib, "gmpc_bilevel_grad_inputs")
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    decl = re.search(r"int gmpc_bilevel_grad_inputs\(([^)]*)\);", hdr)
    assert decl, "gmpc_bilevel_grad_inputs is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["gmpc_ctx* ctx", "int B", "const float* lx", "float* grad_x0", "float* grad_goal",
                      "void* stream"]
    want = {"gmpc_ctx*": C.c_void_p, "int": C.c_int, "const float*": C.c_void_p, "float*": C.c_void_p,
            "void*": C.c_void_p}
    res, args = _lib.SIGNATURES["gmpc_bilevel_grad_inputs"]
    assert res is C.c_int
    assert args == [want[p.rsplit(" ", 1)[0]] for p in params]


def test_engine_method_and_torch_layer_exist():
    assert callable(getattr(Engine, "bilevel_grad_inputs", None))
    from gan_mpc_amd.policy import differentiable
    assert issubclass(differentiable.ILQRFunction, torch.autograd.Function)
    assert callable(differentiable.ilqr_layer)


# ---- the derivation, in fp64 -------------------------------------------------------------------------------------
def _upper_loss(X, U, des):
    """A loss of X and U: squared error of the x columns, a control penalty."""
    return 0.5 * ((X[:, : des.shape[-1]] - des) ** 2).sum() + 0.1 * (U * U).sum() + 0.3 * X[-1].sum()


def _problem(kind):
    if kind == "mlp":
        # (a relu problem whose iLQR reaches a smooth stationary point: most tiny ones stall at a kink)
        pb = orc.make_problem(3, 1, 5, 1, seed=17, dtype=np.float64, dyn_hidden=(16, 16), cost_hidden=(16,),
                              cost_fout=4, bias_scale=1.0)
        dyn = tr.layers64(pb["dyn"])
    else:
        pb = orc.make_problem(3, 1, 5, 1, seed=5, dtype=np.float64, dyn_hidden=(16,), cost_hidden=(16,),
                              cost_fout=4, bias_scale=0.1, dyn_lstm=2)
        dyn = tr.lstm_dynamics64(pb["dyn"])
    pb["mpc_w"] = np.array([-1.0, 1.0, -1.5])
    return pb, dyn


_KW = {"maxiter": 500, "grad_norm_threshold": 1e-13}


def _solve(pb, x0, goal, U, dyn):
    """The oracle's fp64 iLQR, then exact Newton steps on J (the LSTM dynamics' iLQR converges linearly and stalls
    near 1e-9 in the gradient norm, too coarse for central differences)."""
    X, U, _, grad, _, _, _ = orc.ilqr(pb["dyn"], pb["cmlp"], pb["mpc_w"], goal[None], x0[None], U[None], _KW)
    assert np.sqrt((grad ** 2).sum()) < 1e-6
    T, m = pb["T"], pb["m"]
    cm, mw, x0t, gt = tr.layers64(pb["cmlp"]), tr.t64(pb["mpc_w"]), tr.t64(x0), tr.t64(goal)
    J = lambda u: tr.objective(dyn, cm, mw, gt, u.reshape(T, m), x0t)  # noqa: E731
    u = tr.t64(U[0]).reshape(-1)
    for _ in range(4):
        u = u - torch.linalg.solve(torch.autograd.functional.hessian(J, u),
                                   torch.autograd.functional.jacobian(J, u))
    assert float(torch.autograd.functional.jacobian(J, u).norm()) < 1e-12
    U = u.reshape(T, m)
    return tr.rollout(dyn, U, x0t).numpy(), U.numpy()


@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_dense_formula_matches_finite_differences_of_the_solution(kind):
    pb, dyn = _problem(kind)
    T, m = pb["T"], pb["m"]
    x0, goal, des = pb["x0"][0], pb["goal"][0], pb["true_seq"][0]
    X, U = _solve(pb, x0, goal, pb["U"][0], dyn)
    cm, mw = tr.layers64(pb["cmlp"]), tr.t64(pb["mpc_w"])
    dest = tr.t64(des)

    # the formula: A = d^2 J / dU^2, Bvec = dL/dU (through the rollout), H = A^{-1} Bvec, then the mixed VJP
    x0t = tr.t64(x0).requires_grad_(True)
    gt = tr.t64(goal).requires_grad_(True)
    Uf = tr.t64(U).reshape(-1).requires_grad_(True)

    def J(u, x0_, g_):
        return tr.objective(dyn, cm, mw, g_, u.reshape(T, m), x0_)

    A = torch.autograd.functional.hessian(lambda u: J(u, x0t.detach(), gt.detach()), Uf.detach())
    L = _upper_loss(tr.rollout(dyn, Uf.reshape(T, m), x0t), Uf.reshape(T, m), dest)
    dL_dU, dL_dx0 = torch.autograd.grad(L, [Uf, x0t])
    H = torch.linalg.solve(A, dL_dU)
    gU = torch.autograd.grad(J(Uf, x0t, gt), Uf, create_graph=True)[0]
    mx0, mg = torch.autograd.grad(torch.dot(H, gU), [x0t, gt])
    gx0, ggoal = (dL_dx0 - mx0).numpy(), (-mg).numpy()
    assert np.all(ggoal[T] == 0)                     # the terminal cost does not read g_T

    # central differences of L(solution(x0, goal)), each perturbed solve warm-started at the solution
    def L_at(x0_, g_):
        Xp, Up = _solve(pb, x0_, g_, U[None][0], dyn)
        return float(_upper_loss(tr.t64(Xp), tr.t64(Up), dest))

    eps = 1e-5
    fd_x0 = np.zeros_like(x0)
    for i in range(x0.size):
        e = np.zeros_like(x0)
        e[i] = eps
        fd_x0[i] = (L_at(x0 + e, goal) - L_at(x0 - e, goal)) / (2 * eps)
    fd_g = np.zeros_like(goal)
    for t in range(T):
        for i in range(goal.shape[1]):
            e = np.zeros_like(goal)
            e[t, i] = eps
            fd_g[t, i] = (L_at(x0, goal + e) - L_at(x0, goal - e)) / (2 * eps)
    scale_x0, scale_g = np.abs(fd_x0).max(), np.abs(fd_g).max()
    assert scale_x0 > 1e-3 and scale_g > 1e-6
    # central differences at eps 1e-5 of solutions exact to ~1e-13: error ~1e-10 absolute
    np.testing.assert_allclose(gx0, fd_x0, rtol=0, atol=1e-6 * scale_x0 + 1e-9)
    np.testing.assert_allclose(ggoal, fd_g, rtol=0, atol=1e-4 * scale_g + 1e-9)


@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_recursions_equal_the_dense_formula(kind):
    """The kernel's form -- mu / nu recursions over the oracle's LQ model (second-order for the LSTM dynamics), goal
    gradient (Q_t dX_t)[:nx] -- against the dense autograd formula, at the same solution."""
    pb, dyn = _problem(kind)
    T, m = pb["T"], pb["m"]
    x0, goal, des = pb["x0"][0], pb["goal"][0], pb["true_seq"][0]
    X, U = _solve(pb, x0, goal, pb["U"][0], dyn)
    gx0, ggoal = recursions(pb, X[None], U[None], lambda X_, U_: _cot(X_[0], U_[0], des))
    cm, mw = tr.layers64(pb["cmlp"]), tr.t64(pb["mpc_w"])
    x0t, gt = tr.t64(x0).requires_grad_(True), tr.t64(goal).requires_grad_(True)
    Uf = tr.t64(U).reshape(-1).requires_grad_(True)
    J = lambda u, a, g: tr.objective(dyn, cm, mw, g, u.reshape(T, m), a)  # noqa: E731
    A = torch.autograd.functional.hessian(lambda u: J(u, x0t.detach(), gt.detach()), Uf.detach())
    L = _upper_loss(tr.rollout(dyn, Uf.reshape(T, m), x0t), Uf.reshape(T, m), tr.t64(des))
    dL_dU, dL_dx0 = torch.autograd.grad(L, [Uf, x0t])
    H = torch.linalg.solve(A, dL_dU)
    mx0, mg = torch.autograd.grad(torch.dot(H, torch.autograd.grad(J(Uf, x0t, gt), Uf, create_graph=True)[0]),
                                  [x0t, gt])
    np.testing.assert_allclose(gx0[0], (dL_dx0 - mx0).numpy(), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(ggoal[0], (-mg).numpy(), rtol=1e-9, atol=1e-11)


def _cot(X, U, des):
    Xt, Ut = tr.t64(X).requires_grad_(True), tr.t64(U).requires_grad_(True)
    lx, lu = torch.autograd.grad(_upper_loss(Xt, Ut, tr.t64(des)), [Xt, Ut])
    return lx.numpy()[None], lu.numpy()[None]


def recursions(pb, X, U, cot):
    """dL/dx0 (B, n) and dL/dgoal (B, T+1, nx) in the kernel's form, on the oracle's LQ model at (X, U) in X's dtype:
    Bvec = loss adjoint + lu, (H, dX) = hessian_solve, mu_t = lx_t + A^T mu_{t+1}, nu_t = Q~_t dX_t + M~_t H_t +
    A^T nu_{t+1} (Q~, M~ with the LSTM dynamics' curvature), goal: (Q_t dX_t)[:nx].  cot(X, U) -> (lx, lu).  Also
    used by the GPU tests."""
    dt = X.dtype
    p = orc.cast_problem(pb, dt)
    lqr = orc.get_lqr_params(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], X, U)
    Q0 = lqr[0]
    lx, lu = cot(X, U)
    Bv = orc.loss_grad_wrt_control(lqr[5], lqr[6], lx) + lu
    lq = orc.second_order_lqr(p["dyn"], lqr, orc.adjoint(lqr[5], lqr[6], lqr[1], lqr[3])[1], X, U)
    H, dX = orc.hessian_solve(lq, Bv)
    return recursions_from(lq, Q0, lx, H, dX, p["goal"].shape[-1])


def recursions_from(lq, Q0, lx, H, dX, nx):
    Q, M, A = lq[0], lq[4], lq[5]
    T = H.shape[1]
    mu, nu = lx[:, T].copy(), np.einsum("bij,bj->bi", Q[:, T], dX[:, T])
    for t in range(T - 1, -1, -1):
        mu = lx[:, t] + np.einsum("bij,bi->bj", A[:, t], mu)
        nu = (np.einsum("bij,bj->bi", Q[:, t], dX[:, t]) + np.einsum("bnm,bm->bn", M[:, t], H[:, t])
              + np.einsum("bij,bi->bj", A[:, t], nu))
    gg = np.einsum("btij,btj->bti", Q0[:, :, :nx, :nx], dX[:, :, :nx])
    gg[:, T] = 0
    return mu - nu, gg
