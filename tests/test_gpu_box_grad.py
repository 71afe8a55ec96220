"""gmpc_ilqr_solve_box_held and the bilevel tail behind it -- the implicit gradient through a box-constrained iLQR
solution with its active set held fixed -- on the GPU, on the inputs tests/box_cases.py fixes (checked on
the CPU by tests/test_box_grad_host.py).  Every parity check is teacher-forced: the reference (tests/box_grad_ref.py,
NumPy fp32 and fp64) is evaluated at the GPU's own X, U and grad, and the clamped set is rebuilt from those in NumPy,
so no fp32 / fp64 flip of the set can enter.

  G1  debug buffer 18 is clamped_set of the GPU's U and grad bit for bit, a fair share of it is set, H == 0 on it;
  G2  Bvec, the masked Hessian solve (residual on the free entries), the tangent roll, the cost stage, grad_sum,
      grad_x0, grad_goal and grad_dyn_sum under the protocol and bars of test_gpu_bilevel_cotangent /
      test_gpu_input_grads / test_gpu_dynamics_grads, for the L2 loss and a Huber + control loss;
  G3  bounds that are never active: held box solve + tail is fused solve + tail bit for bit;
  G4  the held state: the plain box solve still holds nothing, what drops a held solution drops this one, determinism;
  G5  the policy layer: L2MPC under bounds trains, ilqr_layer's backward, one GAN_MPC generator step."""

import functools

import numpy as np
import pytest
import torch

import box_cases as bc
import box_grad_ref as bg
import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_bilevel_cotangent as cot
import test_gpu_critic_vjp as tv
import test_gpu_input_grads as ig
import test_gpu_mirror as mirror
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.gan import gan_policy
from gan_mpc_amd.norm import l2_policy
from gan_mpc_amd.policy import differentiable as dl
from gan_mpc_amd.policy import optimizers as opt

pytestmark = pytest.mark.gpu
KW = {"maxiter": bc.MAXITER}


def _args(eng, pb, U=None):
    d = eng.to_dev
    return d(pb["x0"]), d(pb["U"] if U is None else U), d(pb["goal"])


def _mask(eng, B):
    """debug buffer 18 as (B, T) uint32 words"""
    return eng.debug_buffer(18, (B, eng.T)).view(torch.int32).cpu().numpy().view(np.uint32)


def _tail(eng, B, lx, lu, sign=1.0):
    """every output of the tail for the cotangents (lx, lu) -> dict of host arrays"""
    g = eng.bilevel_grad_cotangent(B, lx, lu, sign=sign).cpu().numpy()
    st = cot._ctx_state(eng, B)
    gx0, gg = eng.bilevel_grad_inputs(B, lx)
    gdyn = eng.bilevel_grad_dynamics(B, lx)
    return dict(grad_sum=g, H=st["H"], dX=st["dX"], Bvec=st["Bvec"], gx0=gx0.cpu().numpy(), ggoal=gg.cpu().numpy(),
                gdyn=gdyn.cpu().numpy())


# ---- G1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.TABLE)
def test_g1_mask_is_the_clamped_set_of_the_solution(name):
    pb, b = bc.problem(name), bc.bound(name)
    B, T, m = pb["B"], pb["T"], pb["m"]
    eng = gu.engine_for(pb, critic=False)
    try:
        out = eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        U, grad = out["U"].cpu().numpy(), out["grad"].cpu().numpy()
        cl = bg.clamped_set(U, grad, np.float32(-b), np.float32(b))
        np.testing.assert_array_equal(_mask(eng, B), bg.words(cl))
        share = float(cl.mean())
        assert 0.2 <= share <= 0.8, share
        # the plain box solve gives the same solution (the held variant is the same launch)
        plain = eng.ilqr_solve_box(*_args(eng, pb), -b, b, KW)
        for k in ("X", "U", "obj", "grad", "adjoints", "iterations"):
            np.testing.assert_array_equal(plain[k].cpu().numpy(), out[k].cpu().numpy(), err_msg=k)
        eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        eng.bilevel_grad(B, 0, desired=eng.to_dev(pb["true_seq"]))
        st = cot._ctx_state(eng, B)
        assert (st["H"][cl] == 0).all() and np.abs(st["H"][~cl]).max() > 0
        # one-sided bounds: only that side's entries are in the set
        out = eng.ilqr_solve_box_held(*_args(eng, pb), None, b, KW)
        cl_hi = bg.clamped_set(out["U"].cpu().numpy(), out["grad"].cpu().numpy(), None, np.float32(b))
        np.testing.assert_array_equal(_mask(eng, B), bg.words(cl_hi))
        assert cl_hi.any() and (out["U"].cpu().numpy()[cl_hi] == np.float32(b)).all()
    finally:
        eng.close()


# ---- G2 --------------------------------------------------------------------------------------------------------------
def _held_at_the_iterate(name):
    """The case solved under its bounds, the trajectories at a relu kink dropped, the kept ones re-solved with maxiter 0
    from the solution so that the ctx holds exactly them (test_gpu_bilevel_cotangent._solved)."""
    pb, b = dict(bc.problem(name)), bc.bound(name)
    pb64 = orc.cast_problem(pb, np.float64)
    eng = gu.engine_for(pb, critic=False)
    T = pb["T"]
    out = eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
    Xf, Uf = out["X"].cpu().numpy().astype(np.float64), out["U"].cpu().numpy()
    ok = ~(gu.dyn_near_kink(pb64["dyn"], Xf, Uf.astype(np.float64)).any(1) | gu.near_kink(pb64["cmlp"], Xf[:, T]))
    assert ok.sum() >= max(1, pb["B"] // 2)
    for p_ in (pb, pb64):
        for key in ("x0", "goal", "true_seq"):
            p_[key] = p_[key][ok]
        p_["B"] = int(ok.sum())
    out = eng.ilqr_solve_box_held(*_args(eng, pb, Uf[ok]), -b, b, {"maxiter": 0})
    np.testing.assert_array_equal(out["U"].cpu().numpy(), Uf[ok])
    return pb, pb64, eng, out, int(ok.sum()), b


def _check(name, pb, pb64, X, U, cl, cot_fn, loss, got):
    """got: _tail's dict at sign +1.  The stages under their own bars, then the end-to-end figures under the bars HIP's
    own Hessian-solve residual sets (4 x what a right-hand-side perturbation of that size does in fp64)."""
    B, T, n = X.shape[0], U.shape[1], X.shape[-1]
    lv, lx32, lu32 = cot_fn(np.float32)
    lv64, lx64, lu64 = cot_fn(np.float64)
    X64, U64 = X.astype(np.float64), U.astype(np.float64)
    s32, s64 = bg.gradients(pb, X, U, lx32, lu32, cl), bg.gradients(pb64, X64, U64, lx64, lu64, cl)
    if loss is not None:
        gu.assert_parity(f"box grad {name}: loss", loss, lv, lv64)
    gu.assert_parity(f"box grad {name}: Bvec", got["Bvec"], s32["Bv"], s64["Bv"])
    Hd, dXd = got["H"], got["dX"]
    assert (Hd[cl] == 0).all()
    lq, Bv64 = s64["lqr"], s64["Bv"]
    r_hip, r_o32 = bg.free_residual(lq, Hd, Bv64, cl), bg.free_residual(lq, s32["H"], Bv64, cl)
    bar_med, bar_max = max(1e-4, 10 * float(np.median(r_o32))), max(1e-4, 10 * float(r_o32.max()))
    ok = bool(np.median(r_hip) <= bar_med and r_hip.max() <= bar_max)
    gu._record(dict(stage=f"box grad {name}: masked Hessian solve residual |(A H - B)_F| / |B_F| (fp64 A, B; max over "
                    "trajectories)", config=gu.CURRENT_CONFIG[0], e_hip=float(r_hip.max()), e_o32=float(r_o32.max()),
                    tol=1e-4, tol_used=bar_max, branch="tol" if r_hip.max() <= 1e-4 else "slack",
                    entries=int((~cl).sum()), el_hip=float(np.median(r_hip)), el_o32=float(np.median(r_o32)),
                    el_used=bar_med, passed=ok))
    assert ok, (r_hip, r_o32)
    dx = np.zeros((B, T + 1, n))
    Hk = Hd.astype(np.float64)
    for t in range(T):
        dx[:, t + 1] = np.einsum("bij,bj->bi", lq[5][:, t], dx[:, t]) + np.einsum("bnm,bm->bn", lq[6][:, t], Hk[:, t])
    assert gu.rel_err(dXd, dx) < 1e-4
    st32 = bg.gradients(pb, X, U, lx32, lu32, cl, H_dX=(Hd, dXd))
    st64 = bg.gradients(pb64, X64, U64, lx64, lu64, cl, H_dX=(Hd, dXd))
    gu.assert_parity(f"box grad {name}: cost_vjp stage", got["grad_sum"], st32["theta"], st64["theta"])
    # what a backward error of HIP's size does to each output, in fp64
    rng = np.random.default_rng(7)
    keys = dict(theta="grad_sum", x0="gx0", goal="ggoal", dyn="gdyn")
    pert = {k: (0.0, 0.0) for k in keys}
    bf = np.sqrt((np.where(cl, 0.0, Bv64) ** 2).sum((1, 2)))
    for _ in range(4):
        noise = np.where(cl, 0.0, rng.standard_normal(Bv64.shape))
        nn = np.sqrt((noise ** 2).sum((1, 2)))
        noise *= (r_hip * bf / np.where(nn > 0, nn, 1.0))[:, None, None]
        sp = bg.gradients(pb64, X64, U64, lx64, lu64, cl, noise=noise)
        for k in keys:
            e, el = pert[k]
            pert[k] = (max(e, gu.rel_err(sp[k], s64[k])), max(el, gu.el_err(sp[k], s64[k])[0]))
    e, el = pert["theta"]
    gu.assert_parity(f"box grad {name}: grad_sum end-to-end", got["grad_sum"], s32["theta"], s64["theta"],
                     tol=min(max(1e-4, 4.0 * e), gu.SLACK_CEILING), slack=10.0, el_tol=max(1e-3, 4.0 * el))
    for k in ("x0", "goal", "dyn"):
        e, el = pert[k]
        assert np.all(np.isfinite(got[keys[k]]))
        gu.assert_parity(f"box grad {name}: {keys[k]} at the iterate", got[keys[k]], s32[k], s64[k],
                         tol=min(max(1e-4, 4.0 * e), gu.GAIN_CEILING), slack=10.0, ceiling=gu.GAIN_CEILING,
                         el_tol=max(1e-3, 4.0 * el))
    assert np.abs(s64["theta"]).max() > 0 and np.abs(s64["x0"]).max() > 0 and np.abs(s64["dyn"]).max() > 0


@pytest.mark.parametrize("loss", ["l2", "huber"])
@pytest.mark.parametrize("case", list(bc.TABLE) + ["cheetah/valu", "cheetah_T2"])
def test_g2_tail_against_the_masked_reference_at_the_iterate(case, loss, monkeypatch):
    name = cot._case(case, monkeypatch)
    pb, pb64, eng, out, B, b = _held_at_the_iterate(name)
    gu.set_config(f"box grad {case} {loss} n={pb['n']} m={pb['m']} T={pb['T']} B={B}")
    try:
        d = eng.to_dev
        T, m = pb["T"], pb["m"]
        X, U, grad = (out[k].cpu().numpy() for k in ("X", "U", "grad"))
        cl = bg.clamped_set(U, grad, np.float32(-b), np.float32(b))
        np.testing.assert_array_equal(_mask(eng, B), bg.words(cl))
        assert cl.any() and not cl.all()
        des = pb["true_seq"]
        if loss == "l2":
            lossd, g = eng.bilevel_grad(B, 0, desired=d(des), sign=1.0)
            st = cot._ctx_state(eng, B)
            gx0, gg = eng.bilevel_grad_inputs(B, None)
            got = dict(grad_sum=g.cpu().numpy(), H=st["H"], dX=st["dX"], Bvec=st["Bvec"], gx0=gx0.cpu().numpy(),
                       ggoal=gg.cpu().numpy(), gdyn=eng.bilevel_grad_dynamics(B, None).cpu().numpy())
            cot_fn = lambda dt: (orc.l2_loss(X.astype(dt), des.astype(dt)),  # noqa: E731
                                 orc.l2_loss_grad_x(X.astype(dt), des.astype(dt)), np.zeros((B, T, m), dt))
            np.testing.assert_array_equal(eng.upper_loss(B, 0, desired=d(des)).cpu().numpy(), lossd.cpu().numpy())
        else:
            lossd, lx, lu = opt.loss_cotangents(cot.huber_u_loss, out["X"], out["U"], None, (des,))
            assert float(lu.abs().max()) > 0
            got = _tail(eng, B, lx, lu)
            cot_fn = lambda dt: cot._cot_host(cot.huber_u_loss, X, U, des, dt)  # noqa: E731
        assert np.all(got["ggoal"][:, T] == 0)
        _check(case, pb, pb64, X, U, cl, cot_fn, lossd.cpu().numpy(), got)
    finally:
        eng.close()


# ---- G3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "cheetah", "wide_m"])
def test_g3_inactive_bounds_give_the_fused_tail_bit_for_bit(name):
    pb = bc.problem(name)
    B, m = pb["B"], pb["m"]
    eng = gu.engine_for(pb, critic=False)
    try:
        sol = eng.ilqr_solve_fused(*_args(eng, pb), KW)
        _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, sol["X"], sol["U"], None, (pb["true_seq"],))
        want = _tail(eng, B, lx, lu)
        assert np.abs(want["H"]).max() > 0
        for lo, hi in ((None, None), (-np.inf, np.inf), (-1e30, 1e30), (np.full(m, -np.inf), None)):
            held = eng.ilqr_solve_box_held(*_args(eng, pb), lo, hi, KW)
            np.testing.assert_array_equal(held["U"].cpu().numpy(), sol["U"].cpu().numpy())
            assert not _mask(eng, B).any()
            got = _tail(eng, B, lx, lu)
            for k in ("grad_sum", "H", "dX", "gx0", "ggoal", "gdyn"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} bounds {lo}/{hi}: {k}")
    finally:
        eng.close()


# ---- G4 --------------------------------------------------------------------------------------------------------------
def test_g4_held_state():
    pb, b = bc.problem("cheetah"), bc.bound("cheetah")
    B = pb["B"]
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        des = d(pb["true_seq"])
        # the plain box solve holds nothing, whatever was held before it
        eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        eng.ilqr_solve_box(*_args(eng, pb), -b, b, KW)
        for call in (lambda: eng.bilevel_grad(B, 0, desired=des), lambda: eng.upper_loss(B, 0, desired=des),
                     lambda: eng.bilevel_grad_cotangent(B, lx=d(np.zeros((B, pb["T"] + 1, pb["n"]), np.float32)))):
            with pytest.raises(GmpcError, match="must precede"):
                call()
        # held -> fused -> held: the same bits; the fused solve in between gets the unmasked tail
        sol = eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, sol["X"], sol["U"], None, (pb["true_seq"],))
        first = _tail(eng, B, lx, lu)
        mask = _mask(eng, B)
        assert mask.any()
        # repeated tail calls on the held solution
        again = _tail(eng, B, lx, lu)
        for k in first:
            np.testing.assert_array_equal(again[k], first[k], err_msg=f"repeated tail: {k}")
        fsol = eng.ilqr_solve_fused(*_args(eng, pb), KW)
        _, flx, flu = opt.loss_cotangents(cot.huber_u_loss, fsol["X"], fsol["U"], None, (pb["true_seq"],))
        fused = _tail(eng, B, flx, flu)
        eng2 = gu.engine_for(pb, critic=False)       # a ctx that never saw a box solve
        try:
            eng2.ilqr_solve_fused(*_args(eng2, pb), KW)
            clean = _tail(eng2, B, flx.to(eng2.device), flu.to(eng2.device))
        finally:
            eng2.close()
        for k in fused:
            np.testing.assert_array_equal(fused[k], clean[k], err_msg=f"fused tail after a held box solve: {k}")
        eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        np.testing.assert_array_equal(_mask(eng, B), mask)
        third = _tail(eng, B, lx, lu)
        for k in first:
            np.testing.assert_array_equal(third[k], first[k], err_msg=f"held -> fused -> held: {k}")
        # the inputs / dynamics calls need the tail of THIS solution
        eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        with pytest.raises(GmpcError, match="must precede"):
            eng.bilevel_grad_inputs(B, lx)
        # set_params, a rollout and a round-based solve drop the held solution (the last one holds its own, unmasked)
        eng.set_params(*eng._bound)
        with pytest.raises(GmpcError, match="must precede"):
            eng.bilevel_grad(B, 0, desired=des)
        eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        eng.rollout_cost(*_args(eng, pb))
        with pytest.raises(GmpcError, match="must precede"):
            eng.upper_loss(B, 0, desired=des)
        eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        eng.ilqr_solve(*_args(eng, pb, sol["U"].cpu().numpy()), {"maxiter": 0})
        rounds = _tail(eng, B, lx, lu)
        cl = (mask[..., None] >> np.arange(pb["m"], dtype=np.uint32)) & 1 != 0
        assert (first["H"][cl] == 0).all() and (rounds["H"][cl] != 0).all()
        # a solve refused before any launch touches nothing: the held solution and its set stay usable
        eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, KW)
        with pytest.raises(GmpcError, match="make_psd"):
            eng.ilqr_solve_box_held(*_args(eng, pb), -b, b, {"make_psd": True})
        kept = _tail(eng, B, lx, lu)
        for k in first:
            np.testing.assert_array_equal(kept[k], first[k], err_msg=f"after a refused solve: {k}")
    finally:
        eng.close()


def test_g4_refusals_are_the_box_solves():
    pb = gu.problem(3, 1, 33, 2, seed=1, dyn_hidden=(32, 32), cost_hidden=(16,), cost_fout=4)
    eng = gu.engine_for(pb, critic=False)
    try:
        with pytest.raises(GmpcError, match="box solve"):
            eng.ilqr_solve_box_held(*_args(eng, pb), -0.1, 0.1, {"maxiter": 1})
        with pytest.raises(GmpcError, match="u_lo must be <= u_hi"):
            eng.ilqr_solve_box_held(*_args(eng, pb), 0.2, 0.1, {"maxiter": 1})
    finally:
        eng.close()


# ---- G5 --------------------------------------------------------------------------------------------------------------
TIGHT = 1e-3      # the mirror problem's bound: about half of the controls of its 2-iteration solution sit on it


def _box_policy(cls=l2_policy.L2MPC):
    config, policy, params, data = mirror._build(functools.partial(cls, solver="box", control_bounds=(-TIGHT, TIGHT)))
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    return config, policy, params, data


def test_g5_l2mpc_under_bounds_trains():
    config, policy, params, data = _box_policy()
    idx = np.arange(8)
    B = len(idx)
    policy.expert_model.select(idx)
    loss, grads = policy.loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
    eng = policy._engine
    T, n, m = eng.T, eng.n, eng.m
    X = eng.debug_buffer(0, (B, T + 1, n)).cpu().numpy()
    U = eng.debug_buffer(1, (B, T, m)).cpu().numpy()
    mask = _mask(eng, B)
    st = cot._ctx_state(eng, B)
    p32 = mirror._oracle_problem(params, data, idx, np.float32)
    p64 = mirror._oracle_problem(params, data, idx, np.float64)
    X64, U64 = X.astype(np.float64), U.astype(np.float64)
    cl = (mask[..., None] >> np.arange(m, dtype=np.uint32)) & 1 != 0
    # (the set is the kernel's own; that it is clamped_set of the solve's grad is G1's business -- here every clamped
    # control sits on a bound and a fair share is clamped)
    assert (np.abs(U[cl]) == np.float32(TIGHT)).all() and 0.2 <= cl.mean() <= 0.8, cl.mean()
    assert (st["H"][cl] == 0).all()
    keep = ~(gu.dyn_near_kink(p64["dyn"], X64, U64).any(1) | gu.near_kink(p64["cmlp"], X64[:, T]))
    assert keep.sum() >= B // 2
    res = {}
    for dt, p, Xa, Ua in ((np.float32, p32, X, U), (np.float64, p64, X64, U64)):
        pk = dict(p, **{k: p[k][keep] for k in ("x0", "goal", "true_seq")})
        lx = orc.l2_loss_grad_x(Xa[keep], pk["true_seq"])
        s = bg.gradients(pk, Xa[keep], Ua[keep], lx, None, cl[keep])
        res[dt] = (orc.l2_loss(Xa, p["true_seq"]).mean(), s["theta"] / B)
    gu.assert_parity("box policy: loss", float(loss), res[np.float32][0], res[np.float64][0], tol=1e-4, slack=10)
    if keep.all():
        gu.assert_parity("box policy: grads (batch mean) at the iterate", grads.cpu().numpy(), res[np.float32][1],
                         res[np.float64][1], tol=1e-3, slack=10)
    assert np.abs(grads.cpu().numpy()).max() > 0
    policy.expert_model.select(np.arange(8, 16))
    bl = policy.batch_loss(policy.to_device_params(params), data["hist"][8:16], data["Y"][8:16])
    assert np.isfinite(float(bl)) and float(bl) > 0
    # the action path still runs the plain solve: nothing is held behind it
    policy.expert_model.select(np.array([2]))
    policy.get_optimal_action(params, data["hist"][2])
    with pytest.raises(GmpcError, match="must precede"):
        policy._engine.upper_loss(1, 0, desired=policy._engine.to_dev(data["Y"][2:3]))


def test_g5_layer_backward_on_a_box_policy_gives_the_entry_points():
    config, policy, params, data = _box_policy()
    idx = np.arange(8)
    B = len(idx)
    dparams, x0, goal, init_U = ig._layer_inputs(policy, params, data, idx)
    des = torch.as_tensor(np.asarray(data["Y"][idx], np.float32), device=x0.device)
    flat = dparams.flat.requires_grad_(True)
    x0r, goalr = x0.clone().requires_grad_(True), goal.clone().requires_grad_(True)
    X, U = dl.ilqr_layer(policy, dparams, x0r, goalr, init_U)
    loss = ((X[..., : des.shape[-1]] - des) ** 2).mean(1).sum() + 0.05 * (U * U).sum()
    loss.backward()
    eng = policy._engine
    assert _mask(eng, B).any()
    lx = (2 * (X.detach()[..., : des.shape[-1]] - des) / X.shape[1]).contiguous()
    lu = (0.1 * U.detach()).contiguous()
    g = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0)
    gx0, gg = eng.bilevel_grad_inputs(B, lx)
    lo, cnt = dparams.range_of(("mpc_weights", "cost_params"))
    torch.testing.assert_close(flat.grad[lo:lo + cnt], g, rtol=1e-5, atol=1e-6 * float(g.abs().max()))
    assert float(flat.grad[lo + cnt:].abs().max()) == 0
    torch.testing.assert_close(x0r.grad, gx0, rtol=1e-5, atol=1e-6 * float(gx0.abs().max()))
    torch.testing.assert_close(goalr.grad, gg, rtol=1e-5, atol=1e-6 * float(gg.abs().max()))
    assert float(g.abs().max()) > 0 and float(gx0.abs().max()) > 0 and float(gg.abs().max()) > 0
    flat.requires_grad_(False)


def test_g5_gan_mpc_generator_step_under_bounds():
    config, policy, params, data = tv._build(gan_policy.GAN_MPC, N=4, M=2, T=6, hidden=16, ndata=8, objective="wgan",
                                             solver="box", control_bounds=(-TIGHT, TIGHT))
    idx = np.arange(4)
    policy.expert_model.select(idx)
    gl, gg = policy.generator_loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
    assert np.isfinite(float(gl)) and np.all(np.isfinite(gg.cpu().numpy())) and float(gg.abs().max()) > 0
    U = policy._engine.debug_buffer(1, (len(idx), policy._engine.T, policy._engine.m)).cpu().numpy()
    assert (np.abs(U) <= np.float32(TIGHT)).all() and _mask(policy._engine, len(idx)).any()
