"""NumPy restatement (fp32 or fp64, the dtype of its inputs) of the bilevel gradient through a box-constrained iLQR
solution (gmpc_ilqr_solve_box_held), built on the oracle's pieces and on the per-row / recursion forms of
tests/test_input_grads_host.py and tests/test_dynamics_grads_host.py.  TEST INFRASTRUCTURE.

With the active set held fixed the clamped controls sit on bounds that depend on no parameter and the free gradient
vanishes, so the implicit-function formula is §12's with the masked solve

    H_C = 0,  H_F = A_FF^-1 Bvec_F   (A = d^2 J / dU^2),  dX the tangent roll of H.

  clamped_set           the set C of a solution, from U, the full gradient and the bounds;
  words                 C as the kernel's [B][T] words (bit j = control j);
  masked_hessian_solve  orc.hessian_solve with each step's m x m system solved on its free rows;
  dense_masked_solve    the same H from the dense A (orc.hessian_apply on unit vectors): the check of the former;
  gradients             every output of the tail at (X, U) for given cotangents and set."""

import numpy as np

import box_ilqr_ref as br
import gan_mpc_oracle as orc
import gpu_util as gu
from test_dynamics_grads_host import row_form
from test_input_grads_host import recursions_from


def clamped_set(U, grad, lo, hi):
    """(B, T, m) bool: (U == lo and grad > 0) or (U == hi and grad < 0), compared in U's dtype; lo / hi None, a scalar
    or m values.  A NaN compares false: free.  The complement of what box_ilqr_ref.projected keeps."""
    lo, hi = br._bounds(lo, hi, U.shape[-1], U.dtype)
    return br.projected(grad.astype(U.dtype), U, lo, hi)[1]


def words(clamped):
    """(B, T, m) bool -> (B, T) uint32, bit j = control j (m <= 32)."""
    m = clamped.shape[-1]
    assert m <= 32
    return (clamped.astype(np.uint64) << np.arange(m, dtype=np.uint64)).sum(-1).astype(np.uint32)


def masked_hessian_solve(lqr, Bvec, clamped):
    """orc.hessian_solve with the per-step free-set solve: rows of K_t, k_t of clamped controls are 0, the others solve
    G_FF [K k]_F = -[H h]_F.  With K of that form K^T G K = -K^T H and K^T (G k + h) = 0, so the value recursions keep
    orc.hessian_solve's short form.  -> (H (B, T, m), dX (B, T+1, n)); an empty set gives orc.hessian_solve's result."""
    Q, _, R, _, M, A, Bm = lqr
    Bsz, T1, n, _ = Q.shape
    T = T1 - 1
    m = R.shape[-1]
    dt = Q.dtype
    P = Q[:, T].copy()
    p = np.zeros((Bsz, n), dt)
    K = np.zeros((Bsz, T, m, n), dt)
    k = np.zeros((Bsz, T, m), dt)
    for t in range(T - 1, -1, -1):
        At = np.swapaxes(A[:, t], -1, -2)
        Bt = np.swapaxes(Bm[:, t], -1, -2)
        BtP = Bt @ P
        G = orc._sym(R[:, t] + BtP @ Bm[:, t])
        H = BtP @ A[:, t] + np.swapaxes(M[:, t], -1, -2)
        h = -Bvec[:, t] + np.einsum("bnm,bn->bm", Bm[:, t], p)
        rhs = np.concatenate([H, h[..., None]], -1)
        Kk = np.zeros((Bsz, m, n + 1), dt)
        for b in range(Bsz):
            fi = np.nonzero(~clamped[b, t])[0]
            if len(fi):
                Kk[b, fi] = -orc.solve_sym_indef(G[b][np.ix_(fi, fi)], rhs[b, fi])
        K[:, t], k[:, t] = Kk[..., :-1], Kk[..., -1]
        Kt = np.swapaxes(K[:, t], -1, -2)
        P = orc._sym(Q[:, t] + At @ P @ A[:, t] + Kt @ H)
        p = np.einsum("bij,bj->bi", At, p) + np.einsum("bmn,bm->bn", H, k[:, t])
    dX = np.zeros((Bsz, T + 1, n), dt)
    H_out = np.zeros((Bsz, T, m), dt)
    for t in range(T):
        H_out[:, t] = k[:, t] + np.einsum("bmn,bn->bm", K[:, t], dX[:, t])
        dX[:, t + 1] = np.einsum("bij,bj->bi", A[:, t], dX[:, t]) + np.einsum("bnm,bm->bn", Bm[:, t], H_out[:, t])
    return H_out, dX


def dense_hessian(lqr):
    """A = d^2 J / dU^2 of the LQ model, (B, T m, T m): orc.hessian_apply on the unit vectors."""
    Bsz, T, m = lqr[6].shape[0], lqr[6].shape[1], lqr[6].shape[-1]
    A = np.zeros((Bsz, T * m, T * m), lqr[0].dtype)
    for e in range(T * m):
        V = np.zeros((Bsz, T * m), lqr[0].dtype)
        V[:, e] = 1
        A[:, :, e] = orc.hessian_apply(lqr, V.reshape(Bsz, T, m)).reshape(Bsz, T * m)
    return A


def dense_masked_solve(lqr, Bvec, clamped):
    """H with H_C = 0, H_F = A_FF^-1 Bvec_F from the dense A.  -> (B, T, m)."""
    A = dense_hessian(lqr)
    Bsz, T, m = Bvec.shape
    H = np.zeros((Bsz, T * m), A.dtype)
    for b in range(Bsz):
        fi = np.nonzero(~clamped[b].reshape(-1))[0]
        if len(fi):
            H[b, fi] = np.linalg.solve(A[b][np.ix_(fi, fi)], Bvec[b].reshape(-1)[fi])
    return H.reshape(Bsz, T, m)


def free_residual(lqr64, H, Bvec64, clamped):
    """(B,) |(A H - Bvec)_F| / |Bvec_F| with fp64 A and Bvec (0 for a trajectory without a free control)."""
    r = np.where(clamped, 0.0, orc.hessian_apply(lqr64, H.astype(np.float64)) - Bvec64)
    den = np.where(clamped, 0.0, Bvec64)
    den = np.sqrt((den ** 2).sum((1, 2)))
    return np.sqrt((r ** 2).sum((1, 2))) / np.where(den > 0, den, 1.0)


def gradients(pb, X, U, lx, lu, clamped, noise=None, H_dX=None):
    """The tail's outputs at (X, U), in X's dtype, for the cotangents lx (B, T+1, n), lu (B, T, m) or None and the
    clamped set: dict(lqr, Bv, H, dX, theta: d/d(mpc_w, cost params) of H . grad_U J per gu.pack_grads_cost, SUMMED
    over the batch (the tail's grad_sum at sign +1), x0 (B, n), goal (B, T+1, nx), dyn: dL/dtheta_dyn summed).
    noise: added to the solve's right-hand side.  H_dX: (H, dX) to use instead of the masked solve's (stage checks)."""
    dt = X.dtype
    p = orc.cast_problem(pb, dt)
    lqr = orc.get_lqr_params(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], X, U)
    Q, q, R, r, M, A, Bm = lqr
    Bv = orc.loss_grad_wrt_control(A, Bm, lx) + (0 if lu is None else lu)
    if H_dX is None:
        H, dX = masked_hessian_solve(lqr, Bv if noise is None else Bv + noise, clamped)
    else:
        H, dX = (a.astype(dt) for a in H_dX)
    g_mpc, g_cost = orc.cost_vjp(p["cmlp"], p["mpc_w"], p["goal"], X, U, H, dX)
    theta = gu.pack_grads_cost(g_mpc.sum(0), [(a.sum(0), b.sum(0)) for a, b in g_cost])
    gx0, gg = recursions_from(lqr, Q, lx, H, dX, p["goal"].shape[-1])
    T = U.shape[1]
    lam = orc.adjoint(A, Bm, q, r)[1]
    mu, nu = lx[:, T].copy(), np.einsum("bij,bj->bi", Q[:, T], dX[:, T])
    w = np.zeros((X.shape[0], T, X.shape[-1]), dt)
    for t in range(T - 1, -1, -1):
        w[:, t] = mu - nu
        mu = lx[:, t] + np.einsum("bij,bi->bj", A[:, t], mu)
        nu = np.einsum("bij,bj->bi", Q[:, t], dX[:, t]) + np.einsum("bij,bi->bj", A[:, t], nu)
    dyn = [(np.asarray(W, dt), np.asarray(b, dt)) for W, b in p["dyn"]]
    gdyn = row_form(dyn, X, U, dX, H, w, lam[:, 1:])
    return dict(lqr=lqr, Bv=Bv, H=H, dX=dX, theta=theta, x0=gx0, goal=gg, dyn=gdyn)
