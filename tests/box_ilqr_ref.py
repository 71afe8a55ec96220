"""NumPy restatement (fp32 or fp64, the dtype of its inputs) of the control-limited iLQR of gmpc_ilqr_solve_box
(control-limited DDP, Tassa, Mansard and Todorov 2014), built on the oracle's pieces (get_lqr_params,
rollout, evaluate, adjoint, cholesky_lower, cho_solve):

  box_qp        min 1/2 y^T G y + h^T y, lb <= y <= ub, by projected Newton from y = 0;
  box_backward  the Riccati sweep whose gains come from one box_qp per step;
  box_ilqr      the solve: clamped start, clamped candidate rollouts, trajax's line-search rule, the continuation test
                on the projected gradient; `trace` like orc.ilqr's.

With no bound active every operation is the one orc.tvlqr / orc.ilqr perform (the Newton step is the last column of the
same cho_solve of [H | g] that yields the gains), so box_ilqr equals orc.ilqr exactly.  One QP at a time: this is
a checker, not a fast path."""

import numpy as np

import gan_mpc_oracle as orc

QP_ITERS = 40          # projected-Newton iterations per QP at most (GMPC_BOX_QP_ITERS)
ARMIJO = 0.1           # sufficient-decrease constant (GMPC_BOX_ARMIJO)
QP_HALVINGS = 16       # step sizes 1, 1/2, ... tried per iteration (GMPC_BOX_QP_HALVINGS)
DELTA = 1e-8           # lqr_step's regulariser


def clamp(v, lo, hi):
    """NaN-propagating clamp (np.clip would do; written out as the kernel's two selects)."""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(v.dtype)


def _clamped(y, g, lb, ub):
    with np.errstate(invalid="ignore"):
        return ((y == lb) & (g > 0)) | ((y == ub) & (g < 0))


def box_qp(G, h, lb, ub, H=None):
    """G (m, m) symmetric INCLUDING the regulariser, h, lb, ub (m,).  -> dict(y, clamped (m,) bool: the complement of
    the free set the last factorisation used, iters, capped, K: -G_ff^-1 H_f on the free rows / 0.0 on the clamped ones
    when H (m, n) is given, margin_mult: the smallest |g| over the clamped set, margin_clear: the smallest distance of
    a free component to its bounds (inf where there is none))."""
    dt = G.dtype
    m = h.shape[0]
    lb, ub = np.asarray(lb, dt), np.asarray(ub, dt)
    Hm = np.zeros((m, 0), dt) if H is None else H
    y = np.zeros(m, dt)
    g = h.copy()
    cl = _clamped(y, g, lb, ub)
    it, capped = 0, True
    free = ~cl
    Kf = np.zeros((0, Hm.shape[1]), dt)
    half, sigma = np.asarray(0.5, dt), np.asarray(ARMIJO, dt)
    with np.errstate(all="ignore"):
        while it < QP_ITERS:
            free = ~cl
            fi = np.nonzero(free)[0]
            d = np.zeros(m, dt)
            if len(fi):
                L = orc.cholesky_lower(G[np.ix_(fi, fi)])
                Kk = -orc.cho_solve(L, np.concatenate([Hm[fi], g[fi][:, None]], axis=-1))
                Kf, d[fi] = Kk[:, :-1], Kk[:, -1]
            else:
                Kf = np.zeros((0, Hm.shape[1]), dt)
            s = np.asarray(1.0, dt)
            found = False
            for _ in range(QP_HALVINGS):
                yt = clamp(y + s * d, lb, ub)
                D = yt - y
                gd = g @ D
                quad = D @ (G @ D)
                if not (gd + half * quad > sigma * gd):
                    found = True
                    break
                s = s * half
            if not found:
                break
            it += 1
            y = yt
            g = h + G @ y
            new = _clamped(y, g, lb, ub)
            changed = bool((new != cl).any())
            cl = new
            if s == 1.0 and not changed:
                capped = False
                break
    K = np.zeros_like(Hm)
    K[free] = Kf
    clamped = ~free
    with np.errstate(invalid="ignore"):
        mult = np.abs(g[clamped]).min() if clamped.any() else np.inf
        clear = np.minimum(y - lb, ub - y)[free].min() if free.any() else np.inf
    return dict(y=y, clamped=clamped, iters=it, capped=capped, K=K, margin_mult=float(mult), margin_clear=float(clear),
                g=g)


def _bounds(lo, hi, m, dt):
    lo = np.full(m, -np.inf, dt) if lo is None else np.broadcast_to(np.asarray(lo, dt), (m,)).copy()
    hi = np.full(m, np.inf, dt) if hi is None else np.broadcast_to(np.asarray(hi, dt), (m,)).copy()
    return lo, hi


def box_backward(lqr, U, lo, hi):
    """The backward pass at the iterate whose LQR data is lqr = orc.get_lqr_params(...) and whose controls are U
    (B, T, m): lqr_step with the gains of the box QP.  -> dict(K (B,T,m,n), k (B,T,m), clamped (B,T,m) bool,
    qp_iters (B,T), capped (B,T) bool, margin_mult (B,T), margin_clear (B,T)); the margins are relative to the
    largest |h| / |k| of their step (tests/box_cases.py: margins_ok)."""
    Q, q, R, r, M, A, Bm = lqr
    B, T, m = U.shape
    n = Q.shape[-1]
    dt = Q.dtype
    lo, hi = _bounds(lo, hi, m, dt)
    out = dict(K=np.zeros((B, T, m, n), dt), k=np.zeros((B, T, m), dt), clamped=np.zeros((B, T, m), bool),
               qp_iters=np.zeros((B, T), int), capped=np.zeros((B, T), bool), margin_mult=np.zeros((B, T)),
               margin_clear=np.zeros((B, T)))
    with np.errstate(all="ignore"):
        P, p = Q[:, T], q[:, T]
        for t in range(T - 1, -1, -1):
            # (the expressions of orc.lqr_step on the whole batch, so that the result is its result, bit for bit,
            # whenever the QPs return the unconstrained gains)
            At = np.swapaxes(A[:, t], -1, -2)
            Bt = np.swapaxes(Bm[:, t], -1, -2)
            AtP = At @ P
            AtPA = orc._sym(AtP @ A[:, t])
            BtP = Bt @ P
            BtPA = BtP @ A[:, t]
            G = orc._sym(R[:, t] + BtP @ Bm[:, t])
            H = BtPA + np.swapaxes(M[:, t], -1, -2)
            h = r[:, t] + np.einsum("...nm,...n->...m", Bm[:, t], p)
            Gd = G + np.asarray(DELTA, dt) * np.eye(m, dtype=dt)
            K, k = np.zeros((B, m, n), dt), np.zeros((B, m), dt)
            for b in range(B):
                qp = box_qp(Gd[b], h[b], lo - U[b, t], hi - U[b, t], H[b])
                K[b], k[b], out["clamped"][b, t] = qp["K"], qp["y"], qp["clamped"]
                out["qp_iters"][b, t], out["capped"][b, t] = qp["iters"], qp["capped"]
                # margins relative to the step's own scales: multipliers to max |h|, clearances to max |y|
                out["margin_mult"][b, t] = qp["margin_mult"] / max(float(np.abs(h[b]).max()), 1e-300)
                out["margin_clear"][b, t] = qp["margin_clear"] / max(float(np.abs(k[b]).max()), 1e-300)
            H_GK = H + G @ K
            Kt = np.swapaxes(K, -1, -2)
            Pn = orc._sym(Q[:, t] + AtPA + np.swapaxes(H_GK, -1, -2) @ K + Kt @ H)
            pn = (
                q[:, t]
                + np.einsum("...ij,...j->...i", At, p)
                + np.einsum("...mn,...m->...n", H_GK, k)
                + np.einsum("...mn,...m->...n", K, h)
            )
            P, p = Pn, pn
            out["K"][:, t], out["k"][:, t] = K, k
    return out


def box_rollout(dyn, X, U, K, k, alpha, lo, hi):
    """orc.ddp_rollout with every control clamped."""
    B, T, m = U.shape
    Xn, Un = np.empty_like(X), np.empty_like(U)
    Xn[:, 0] = X[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            du = alpha[:, None] * k[:, t] + np.einsum("bmn,bn->bm", K[:, t], Xn[:, t] - X[:, t])
            Un[:, t] = clamp(U[:, t] + du, lo, hi)
            Xn[:, t + 1], _ = orc.dynamics_predict(dyn, Xn[:, t], Un[:, t])
    return Xn, Un


def _line_search(dyn, cmlp, mpc_w, goal, X, U, K, k, obj, alpha_0, alpha_min, active, lo, hi):
    """orc.line_search_ddp on box_rollout."""
    B = X.shape[0]
    dt = X.dtype
    obj = np.where(np.isnan(obj), np.inf, obj).astype(dt)
    Xr, Ur = X.copy(), U.copy()
    objr = obj.copy()
    alpha = np.full((B,), alpha_0, dt)
    run = active.copy()
    run &= alpha > alpha_min
    while run.any():
        Xn, Un = box_rollout(dyn, X, U, K, k, alpha, lo, hi)
        with np.errstate(invalid="ignore", over="ignore"):
            on = np.sum(orc.evaluate(cmlp, mpc_w, goal, Xn, Un), axis=1)
        on = np.where(np.isnan(on), obj, on).astype(dt)
        acc = run & (on < obj)
        Xr[acc], Ur[acc] = Xn[acc], Un[acc]
        objr = np.where(run, np.minimum(on, obj), objr).astype(dt)
        alpha = np.where(run, 0.5 * alpha, alpha).astype(dt)
        run = run & (objr >= obj) & (alpha > alpha_min)
    return Xr, Ur, objr, alpha


def projected(grad, U, lo, hi):
    """grad with the components a bound holds back set to zero."""
    with np.errstate(invalid="ignore"):
        held = ((U == lo) & (grad > 0)) | ((U == hi) & (grad < 0))
    return np.where(held, 0, grad).astype(grad.dtype), held


def box_ilqr(dyn, cmlp, mpc_w, goal, x0, U, lo, hi, kwargs=None, trace=None):
    """orc.ilqr under lo <= u <= hi.  Returns X, U, obj, gradient (the full one), adjoints, lqr, iteration; trace
    entries as orc.ilqr's plus `backward` (box_backward's dict of the pass about to be applied) and `U`."""
    kw = dict(orc.ILQR_KWARGS)
    if kwargs:
        kw.update(kwargs)
    if kw["make_psd"]:
        raise NotImplementedError("make_psd=True is not on the reference path")
    B, T, m = U.shape
    dt = x0.dtype
    lo, hi = _bounds(lo, hi, m, dt)
    U = clamp(U.astype(dt), lo, hi)
    X = orc.rollout(dyn, U, x0)
    obj = np.sum(orc.evaluate(cmlp, mpc_w, goal, X, U), axis=1)
    lqr = list(orc.get_lqr_params(dyn, cmlp, mpc_w, goal, X, U))
    grad, adj = orc.adjoint(lqr[5], lqr[6], lqr[1], lqr[3])
    alpha = np.full((B,), kw["alpha_0"], dt)
    it = np.zeros((B,), np.int32)
    obj_step = np.full((B,), np.inf, dt)
    U_step = np.full((B,), np.inf, dt)
    crit = {}

    def cont():
        pg, _ = projected(grad, U, lo, hi)
        with np.errstate(invalid="ignore", over="ignore"):
            gn = np.sqrt(np.sum(pg * pg, axis=(1, 2)))
        gn = np.where(np.isnan(gn), np.inf, gn)
        aobj = np.abs(obj) + 1.0
        un = np.sqrt(np.sum(U * U, axis=(1, 2))) + 1.0
        progressing = (obj_step > kw["obj_step_threshold"] * aobj) & (U_step > kw["inputs_step_threshold"] * un)
        potential = (gn > kw["grad_norm_threshold"]) & (gn > kw["relative_grad_norm_threshold"] * aobj)
        crit.update(gn=gn.copy(), aobj=aobj.copy(), un=un.copy(), obj_step=obj_step.copy(), U_step=U_step.copy())
        return (it < kw["maxiter"]) & progressing & potential & (alpha > kw["alpha_min"])

    while True:
        act = cont()
        if trace is not None:
            trace.append(dict(active=act.copy(), obj=obj.copy(), alpha=alpha.copy(), crit=dict(crit), U=U.copy()))
        if not act.any():
            break
        bw = box_backward(lqr, U, lo, hi)
        if trace is not None:
            trace[-1]["backward"] = bw
        Xn, Un, objn, alphan = _line_search(dyn, cmlp, mpc_w, goal, X, U, bw["K"], bw["k"], obj, kw["alpha_0"],
                                            kw["alpha_min"], act, lo, hi)
        a3 = act[:, None, None]
        U_step = np.where(act, np.sqrt(np.sum((Un - U) ** 2, axis=(1, 2))), U_step).astype(dt)
        obj_step = np.where(act, np.abs(objn - obj), obj_step).astype(dt)
        X = np.where(a3, Xn, X)
        U = np.where(a3, Un, U)
        obj = np.where(act, objn, obj).astype(dt)
        alpha = np.where(act, alphan, alpha).astype(dt)
        new = orc.get_lqr_params(dyn, cmlp, mpc_w, goal, X, U)
        for i in range(7):
            sel = act.reshape((B,) + (1,) * (new[i].ndim - 1))
            lqr[i] = np.where(sel, new[i], lqr[i])
        g2, a2 = orc.adjoint(lqr[5], lqr[6], lqr[1], lqr[3])
        grad = np.where(a3, g2, grad)
        adj = np.where(a3, a2, adj)
        it = it + act.astype(np.int32)
    return X, U, obj, grad, adj, tuple(lqr), it
