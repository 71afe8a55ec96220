"""gmpc_bilevel_grad_cotangent -- the bilevel gradient of a caller-defined upper-level loss L(X, U), from the caller's
cotangents lx = dL/dX, lu = dL/dU -- on the GPU (reference policy/optimizers.py:34-83: `loss` is any callable, and
jax.grad sees its dependence on U as well).

The cases reach every Bvec producer: k_riccati_w2 in its Hessian form (trained-like, w2-T*), k_bvec (tiny-ragged, trained-like under
GMPC_RICCATI=valu, dynl-small with the curvature term), k_big_step mode 1 (big-70, m40-n24, lowrank-1h, dynl-big).

  1. with the lx gmpc_bilevel_grad computes and no lu: the same bits as gmpc_bilevel_grad (grad_sum, Bvec, H, dX);
  2. a loss of X and U against the fp64 oracle's stages at the GPU's iterate, Bvec = loss_grad_wrt_control + lu;
  3. the reference formula literally (dense Hessian, dense solve, mixed VJP in fp64 torch);
  4. lu alone, and linearity in (lx, lu);
  5. the policy layer: a BaseMPC subclass with a torch loss;
  6. refusals and determinism."""

import functools

import numpy as np
import pytest
import torch
from torch.func import grad_and_value, vmap

import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_mirror as mirror
import test_gpu_parity as par
import torch_ref as tr
from gan_mpc_amd import optim
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.norm import cost_trainer, l2_policy
from gan_mpc_amd.policy import base
from gan_mpc_amd.policy import optimizers as opt

pytestmark = pytest.mark.gpu


def huber_u_loss(x, u, params, desired):
    """A loss of X and U: per-step weighted Huber error of the x columns (delta 0.5), time-weighted control
    penalty."""
    del params
    T = u.shape[0]
    d = x[:, : desired.shape[-1]] - desired
    a = d.abs()
    hub = torch.where(a < 0.5, 0.5 * d * d, 0.5 * a - 0.125)
    sw = 1.0 + 0.1 * torch.arange(T + 1, dtype=x.dtype, device=x.device)
    tw = 0.05 * (1.0 + torch.arange(T, dtype=x.dtype, device=x.device) / T)
    return (sw[:, None] * hub).mean(0).sum() + (tw[:, None] * u * u).sum()


def _cot_host(loss, X, U, desired, dt):
    """(loss [B], lx, lu) in dtype dt on the host, torch.func per trajectory."""
    t = functools.partial(torch.as_tensor, dtype=torch.float64 if dt == np.float64 else torch.float32)
    (lx, lu), v = vmap(grad_and_value(loss, argnums=(0, 1)), in_dims=(0, 0, None, 0))(t(X), t(U), None, t(desired))
    return v.numpy(), lx.numpy(), lu.numpy()


def _check_at_iterate(pb, pb64, X, U, cot, loss, grad, Hd, dXd, Bvd, batch_mean=False, keep=None, end_to_end=True):
    """gpu_util.check_bilevel_at_iterate's protocol for a caller-defined loss: cot(dtype) -> (loss or None, lx, lu)
    at the GPU's iterate (X, U); Bvec = loss_grad_wrt_control(A, B, lx) + lu.  Bvec and the cost_vjp stage under
    assert_parity, the Hessian solve by its fp64 residual, the tangent roll, then the end-to-end bar."""
    B, T, n = X.shape[0], U.shape[1], X.shape[-1]
    keep = np.ones(B, bool) if keep is None else np.asarray(keep, bool)
    red = (lambda a: a.mean(0)) if batch_mean else (lambda a: a.sum(0))

    def pack(g_mpc, g_cost):
        return gu.pack_grads_cost(red(g_mpc), [(red(a), red(b)) for a, b in g_cost])

    def stages(p, dt):
        Xa, Ua = X.astype(dt), U.astype(dt)
        lqr = orc.get_lqr_params(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], Xa, Ua)
        lv, lx, lu = cot(dt)
        Bv = orc.loss_grad_wrt_control(lqr[5], lqr[6], lx) + lu
        lqr = orc.second_order_lqr(p["dyn"], lqr, orc.adjoint(lqr[5], lqr[6], lqr[1], lqr[3])[1], Xa, Ua)
        Hc, dX = orc.hessian_solve(lqr, Bv)
        g_stage = pack(*orc.cost_vjp(p["cmlp"], p["mpc_w"], p["goal"], Xa, Ua, Hd.astype(dt), dXd.astype(dt)))
        g_full = pack(*orc.cost_vjp(p["cmlp"], p["mpc_w"], p["goal"], Xa, Ua, Hc, dX))
        lval = None if lv is None else (lv.mean() if batch_mean else lv)
        return dict(lqr=lqr, loss=lval, Bv=Bv, H=Hc, g_stage=g_stage, g_full=g_full)

    s32, s64 = stages(pb, np.float32), stages(pb64, np.float64)
    if loss is not None:
        gu.assert_parity("cotangent loss", loss, s32["loss"], s64["loss"])
    gu.assert_parity("cotangent Bvec", Bvd[keep], s32["Bv"][keep], s64["Bv"][keep])
    lq = [a[keep] for a in s64["lqr"]]
    Bv64 = s64["Bv"][keep]

    def resid(H):
        r = orc.hessian_apply(lq, H[keep].astype(np.float64)) - Bv64
        return np.sqrt((r ** 2).sum((1, 2)) / (Bv64 ** 2).sum((1, 2)))
    r_hip, r_o32 = resid(Hd), resid(s32["H"])
    # The residual of an fp32 solve is ~ eps x cond(A) in the directions B excites.  The L2 / JS right-hand sides of
    # check_bilevel_at_iterate stay below 1e-4; the Huber + control and random-lu right-hand sides reach the
    # ill-conditioned directions of the 17 x 6 problems (T 10 and 50), where the fp32 oracle's own residual is
    # 2e-4 .. 1.4e-3 per trajectory -- so one fp32 draw per trajectory is no yardstick there.  The bar: median and
    # max over the trajectories each within 1e-4 or 10 x the fp32 oracle's median / max.
    bar_med, bar_max = max(1e-4, 10 * float(np.median(r_o32))), max(1e-4, 10 * float(r_o32.max()))
    ok = bool(np.median(r_hip) <= bar_med and r_hip.max() <= bar_max)
    gu._record(dict(stage="cotangent Hessian solve residual |A H - B| / |B| (fp64 A, B; max over trajectories)",
                    config=gu.CURRENT_CONFIG[0], e_hip=float(r_hip.max()), e_o32=float(r_o32.max()), tol=1e-4,
                    tol_used=bar_max, branch="tol" if r_hip.max() <= 1e-4 else "slack", entries=int(Hd[keep].size),
                    el_hip=float(np.median(r_hip)), el_o32=float(np.median(r_o32)), el_used=bar_med, passed=ok))
    assert ok, (r_hip, r_o32)
    Hk = Hd[keep].astype(np.float64)
    dx = np.zeros((Hk.shape[0], T + 1, n))
    for t in range(T):
        dx[:, t + 1] = np.einsum("bij,bj->bi", lq[5][:, t], dx[:, t]) + np.einsum("bnm,bm->bn", lq[6][:, t], Hk[:, t])
    assert gu.rel_err(dXd[keep], dx) < 1e-4
    gu.assert_parity("cotangent cost_vjp stage", grad, s32["g_stage"], s64["g_stage"])
    if not end_to_end:
        return s32, s64
    # the end-to-end bar of check_bilevel_at_iterate: 1e-4, 10 x the fp32 oracle's error, or 4 x what a backward
    # error of HIP's size does to the gradient in fp64; never above 1e-3
    assert keep.all()
    rng = np.random.default_rng(7)
    e_pert, el_pert = 0.0, 0.0
    for _ in range(4):
        noise = rng.standard_normal(Bv64.shape)
        noise *= (r_hip * np.sqrt((Bv64 ** 2).sum((1, 2)) / (noise ** 2).sum((1, 2))))[:, None, None]
        Hp, dXp = orc.hessian_solve(lq, Bv64 + noise)
        gp = pack(*orc.cost_vjp(pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X.astype(np.float64),
                                U.astype(np.float64), Hp, dXp))
        e_pert = max(e_pert, gu.rel_err(gp, s64["g_full"]))
        el_pert = max(el_pert, gu.el_err(gp, s64["g_full"])[0])
    gu.assert_parity("cotangent bilevel grad end-to-end", grad, s32["g_full"], s64["g_full"],
                     tol=min(max(1e-4, 4.0 * e_pert), gu.SLACK_CEILING), slack=10.0, el_tol=max(1e-3, 4.0 * el_pert))
    return s32, s64


# The two-wave sweep's Hessian form (17 x 6 only) at the horizons where its double buffering (t & 1), the one-step-ahead
# helper wave and the tangent roll can go wrong: nothing prepared inside the loop (T 1), each buffer used once (T 2),
# an odd horizon that wraps the buffers (T 3).  name: T (B 4, the seed and out_scale of trained-like)
SHORT = {"w2-T1": 1, "w2-T2": 2, "w2-T3": 3}


def _solved(name, critic=False, fused=False):
    """A problem of test_gpu_parity's table solved on the GPU (3 iterations), the trajectories at a relu kink
    dropped, and the kept ones re-solved with maxiter 0 so that the ctx holds exactly them (test_bilevel_grad)."""
    if name == "fused-17x6" or name in SHORT:
        T, B = (10, 16) if name == "fused-17x6" else (SHORT[name], 4)
        pb = gu.problem(17, 6, T, B, seed=11, out_scale=0.1)
        gu.set_config(f"{'fused' if name == 'fused-17x6' else 'short'} bilevel n=17 m=6 T={T} B={B}")
        pb64, eng = orc.cast_problem(pb, np.float64), gu.engine_for(pb, critic=critic)
    else:
        pb, pb64, eng = par._setup(name, critic=critic)
    solve = eng.ilqr_solve_fused if fused else eng.ilqr_solve
    d = eng.to_dev
    T = pb["T"]
    out = solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 3})
    Xf = out["X"].cpu().numpy().astype(np.float64)
    Uf = out["U"].cpu().numpy()
    ok = ~(gu.dyn_near_kink(pb64["dyn"], Xf, Uf.astype(np.float64)).any(1) | gu.near_kink(pb64["cmlp"], Xf[:, T]))
    assert ok.sum() >= max(1, pb["B"] // 2)
    for p_ in (pb, pb64):
        for key in ("x0", "goal", "true_seq"):
            p_[key] = p_[key][ok]
    out = solve(d(pb["x0"]), d(Uf[ok]), d(pb["goal"]), {"maxiter": 0})
    return pb, pb64, eng, out, int(ok.sum())


def _ctx_state(eng, B):
    T, n, m = eng.T, eng.n, eng.m
    return dict(H=eng.debug_buffer(2, (B, T, m)).cpu().numpy(), dX=eng.debug_buffer(3, (B, T + 1, n)).cpu().numpy(),
                Bvec=eng.debug_buffer(4, (B, T, m)).cpu().numpy())


BVEC_CASES = ["trained-like", "trained-like/valu", "tiny-ragged", "m40-n24", "dynl-small", "big-70", "lowrank-1h",
              "dynl-big"] + [c + form for c in SHORT for form in ("", "/valu")]


def _case(case, monkeypatch):
    name, _, form = case.partition("/")
    if form == "valu":
        monkeypatch.setenv("GMPC_RICCATI", "valu")
    return name


# ---- 1. same machinery, same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("case,loss_kind", [(c, 0) for c in BVEC_CASES] + [("trained-like", 1), ("dynl-small", 1),
                                                                          ("fused-17x6", 0), ("fused-tiny", 1)])
def test_same_cotangent_gives_the_same_bits(case, loss_kind, monkeypatch):
    fused = case.startswith("fused-")
    name = {"fused-tiny": "tiny-ragged"}.get(case, _case(case, monkeypatch))
    pb, pb64, eng, out, B = _solved(name, critic=loss_kind == 1, fused=fused)
    d = eng.to_dev
    T, n = pb["T"], pb["n"]
    crit = d(gu.critic_flat(pb)) if loss_kind == 1 else None
    _, g_ref = eng.bilevel_grad(B, loss_kind, desired=d(pb["true_seq"]), critic=crit, sign=1.0)
    g_ref = g_ref.cpu().numpy()
    ref = _ctx_state(eng, B)
    lx = eng.debug_buffer(11, (B, T + 1, n)).contiguous()
    assert float(lx.abs().max()) > 0
    g = eng.bilevel_grad_cotangent(B, lx, None, sign=1.0).cpu().numpy()
    np.testing.assert_array_equal(g, g_ref)
    got = _ctx_state(eng, B)
    for key in ref:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


# ---- 2. a loss of X and U against fp64 at the GPU's iterate ------------------------------------------------------
@pytest.mark.parametrize("case", BVEC_CASES + ["fused-17x6"])
def test_loss_of_states_and_controls_against_the_oracle(case, monkeypatch):
    fused = case.startswith("fused-")
    pb, pb64, eng, out, B = _solved(_case(case, monkeypatch), fused=fused)
    d = eng.to_dev
    T, n, m = pb["T"], pb["n"], pb["m"]
    Xd, Ud = out["X"], out["U"]
    loss, lx, lu = opt.loss_cotangents(huber_u_loss, Xd, Ud, None, (pb["true_seq"],))
    g = eng.bilevel_grad_cotangent(B, lx, lu, sign=1.0).cpu().numpy()
    st = _ctx_state(eng, B)
    X, U = Xd.cpu().numpy(), Ud.cpu().numpy()
    assert float(lu.abs().max()) > 0 and np.abs(g).max() > 0
    _check_at_iterate(pb, pb64, X, U, lambda dt: _cot_host(huber_u_loss, X, U, pb["true_seq"], dt),
                      loss.cpu().numpy(), g, st["H"], st["dX"], st["Bvec"])


# ---- 3. the reference formula, literally -------------------------------------------------------------------------
def test_reference_formula_dense_hessian_solve():
    """policy/optimizers.py:61-71 as written, in fp64 torch on the host for each trajectory: B = grad_U
    loss(rollout(U), U), the dense A = hessian(objective), H = solve(A, B), grad_theta (H . grad_U J).  Independent of
    the structured solve (hessian_solve) the other checks go through."""
    pb, pb64, eng, out, B = _solved("tiny-ragged")
    T, m = pb["T"], pb["m"]
    Xd, Ud = out["X"], out["U"]
    _, lx, lu = opt.loss_cotangents(huber_u_loss, Xd, Ud, None, (pb["true_seq"],))
    g = eng.bilevel_grad_cotangent(B, lx, lu).cpu().numpy()
    U = Ud.cpu().numpy().astype(np.float64)
    dyn, cm, mw = tr.layers64(pb["dyn"]), tr.layers64(pb["cmlp"]), tr.t64(pb["mpc_w"])
    total = None
    for b in range(B):
        x0, goal, des = tr.t64(pb64["x0"][b]), tr.t64(pb64["goal"][b]), tr.t64(pb64["true_seq"][b])
        Ub = tr.t64(U[b]).requires_grad_(True)
        Bv = torch.autograd.grad(huber_u_loss(tr.rollout(dyn, Ub, x0), Ub, None, des), Ub)[0].reshape(-1)

        def J(Uf, cmlp, mpc_w):
            return tr.objective(dyn, cmlp, mpc_w, goal, Uf.reshape(T, m), x0)

        A = torch.autograd.functional.hessian(lambda Uf: J(Uf, cm, mw), tr.t64(U[b]).reshape(-1))
        H = torch.linalg.solve(A, Bv)
        leaves = [mw.clone().requires_grad_(True)]
        cml = []
        for W, bb in cm:
            W, bb = W.clone().requires_grad_(True), bb.clone().requires_grad_(True)
            cml.append((W, bb))
            leaves += [W, bb]
        Uf = tr.t64(U[b]).reshape(-1).requires_grad_(True)
        gU = torch.autograd.grad(J(Uf, cml, leaves[0]), Uf, create_graph=True)[0]
        grads = torch.autograd.grad(torch.dot(H.detach(), gU), leaves, allow_unused=True)
        flat = torch.cat([(torch.zeros_like(l) if gr is None else gr).reshape(-1) for l, gr in zip(leaves, grads)])
        total = flat if total is None else total + flat
    X = Xd.cpu().numpy()
    s32, _ = _check_at_iterate(pb, pb64, X, Ud.cpu().numpy(),
                               lambda dt: _cot_host(huber_u_loss, X, Ud.cpu().numpy(), pb["true_seq"], dt),
                               None, g, *(_ctx_state(eng, B)[k] for k in ("H", "dX", "Bvec")), end_to_end=False)
    # the fp32 oracle's structured route measured against the same dense fp64 figure sets the slack branch
    gu.assert_parity("cotangent grad vs the dense reference formula (fp64 torch)", g, s32["g_full"], total.numpy(),
                     tol=1e-4, slack=10.0)


# ---- 4. lu is not ignored; linearity -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trained-like", "tiny-ragged", "big-70"])
def test_control_cotangent_alone_and_linearity(name):
    pb, pb64, eng, out, B = _solved(name)
    d = eng.to_dev
    T, n, m = pb["T"], pb["n"], pb["m"]
    rng = np.random.default_rng(21)
    lu = rng.standard_normal((B, T, m)).astype(np.float32) * 0.1
    g_u = eng.bilevel_grad_cotangent(B, None, d(lu)).cpu().numpy()
    st = _ctx_state(eng, B)
    assert np.abs(g_u).max() > 0
    X, U = out["X"].cpu().numpy(), out["U"].cpu().numpy()
    # (trained-like, T 50: white-noise lu reaches the solve's least stable directions, where the end-to-end forward
    # error of an fp32 solve is cond(A)-sized, 1.5e-3; the Huber + control loss of test 2 holds the end-to-end bar on
    # the same shape.  Every stage is still checked here.)
    _check_at_iterate(pb, pb64, X, U, lambda dt: (None, np.zeros((B, T + 1, n), dt), lu.astype(dt)), None, g_u,
                      st["H"], st["dX"], st["Bvec"], end_to_end=name != "trained-like")
    _, lx, _ = opt.loss_cotangents(huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
    g_x = eng.bilevel_grad_cotangent(B, lx, None).cpu().numpy()
    g_xu = eng.bilevel_grad_cotangent(B, lx, d(lu)).cpu().numpy()
    scale = (np.abs(g_x) + np.abs(g_u)).max()
    err = np.abs(g_xu - (g_x + g_u)).max() / scale
    gu._record(dict(stage="g(lx, lu) - g(lx, 0) - g(0, lu), relative to max |g(lx, 0)| + |g(0, lu)|",
                    config=gu.CURRENT_CONFIG[0], e_hip=float(err), e_o32=0.0, tol=1e-5, tol_used=1e-5,
                    branch="tol", entries=int(g_xu.size), passed=bool(err <= 1e-5)))
    assert err <= 1e-5, err


# ---- 5. the policy layer -----------------------------------------------------------------------------------------
class TorchL2MPC(base.BaseMPC):
    """L2MPC's loss written in torch: no LOSS_KIND, so the policy differentiates it per trajectory."""

    def loss(self, xcseq, useq, params, desired_xseq):
        del useq, params
        d = xcseq[:, : desired_xseq.shape[-1]] - desired_xseq
        return (d * d).mean(0).sum()


class HuberUMPC(base.BaseMPC):
    def loss(self, xcseq, useq, params, desired_xseq):
        return huber_u_loss(xcseq, useq, params, desired_xseq)


@pytest.mark.parametrize("solver", ["rounds", "fused"])
def test_torch_l2_policy_reproduces_l2mpc(solver):
    res = {}
    for cls in (l2_policy.L2MPC, TorchL2MPC):
        config, policy, params, data = mirror._build(functools.partial(cls, solver=solver))
        policy.trajax_ilqr_kwargs["maxiter"] = 2
        idx = np.arange(8)
        policy.expert_model.select(idx)
        loss, grads = policy.loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
        policy.expert_model.select(np.arange(8, 16))
        bl = policy.batch_loss(policy.to_device_params(params), data["hist"][8:16], data["Y"][8:16])
        res[cls] = (float(loss), grads.cpu().numpy().astype(np.float64), float(bl))
    (l0, g0, b0), (l1, g1, b1) = res[l2_policy.L2MPC], res[TorchL2MPC]
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l0, l1)
    assert abs(b1 - b0) <= 1e-5 * abs(b0), (b0, b1)
    assert gu.rel_err(g1, g0) <= 1e-5, gu.rel_err(g1, g0)


@pytest.mark.parametrize("solver", ["rounds", "fused"])
def test_control_dependent_policy_against_the_oracle_batch_mean(solver):
    config, policy, params, data = mirror._build(functools.partial(HuberUMPC, solver=solver))
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    idx = np.arange(8)
    policy.expert_model.select(idx)
    loss, grads = policy.loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
    eng = policy._engine
    B, T, n, m = len(idx), eng.T, eng.n, eng.m
    X = eng.debug_buffer(0, (B, T + 1, n)).cpu().numpy()
    U = eng.debug_buffer(1, (B, T, m)).cpu().numpy()
    st = _ctx_state(eng, B)
    p32 = mirror._oracle_problem(params, data, idx, np.float32)
    p64 = mirror._oracle_problem(params, data, idx, np.float64)
    X64, U64 = X.astype(np.float64), U.astype(np.float64)
    keep = ~(gu.dyn_near_kink(p64["dyn"], X64, U64).any(1) | gu.near_kink(p64["cmlp"], X64[:, T]))
    assert keep.sum() >= B // 2
    _check_at_iterate(p32, p64, X, U, lambda dt: _cot_host(huber_u_loss, X, U, data["Y"][idx], dt),
                      np.float32(float(loss)), grads.cpu().numpy(), st["H"], st["dX"], st["Bvec"], batch_mean=True,
                      keep=keep, end_to_end=bool(keep.all()))


def test_cost_trainer_update_with_a_torch_loss():
    config, policy, params, data = mirror._build(HuberUMPC)
    policy.trajax_ilqr_kwargs["maxiter"] = 1
    tc = config.mpc.train.cost
    optimizer = optim.get_optimizer(list(params.keys()), tc.no_grads, tc.learning_rate)
    dparams = policy.to_device_params(params)
    before = dparams.clone()
    opt_state = optimizer.init(dparams)
    train = (data["hist"][:16], data["Y"][:16])
    test = (data["hist"][16:], data["Y"][16:])
    new_params, opt_state, train_losses, test_losses, _ = cost_trainer.train(
        (policy, optimizer), opt_state, dparams, (train, test), num_updates=1, batch_size=8,
        polyak_factor=tc.polyak_factor, key=7, id=0)
    assert opt_state["count"] == 2 and np.isfinite(train_losses[0]) and np.isfinite(test_losses[0])
    moved = (new_params.view("cost_params") - before.view("cost_params")).abs().max()
    assert float(moved) > 0


# ---- 6. refusals, determinism ------------------------------------------------------------------------------------
def test_refusals():
    pb, _, eng = par._setup("tiny-ragged")
    d = eng.to_dev
    B, T, n, m = pb["B"], pb["T"], pb["n"], pb["m"]
    lx = d(np.zeros((B, T + 1, n), np.float32))
    with pytest.raises(GmpcError, match="must precede"):
        eng.bilevel_grad_cotangent(B, lx)
    eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 1})
    with pytest.raises(GmpcError, match="must precede"):
        eng.bilevel_grad_cotangent(B - 1, lx[:B - 1].contiguous())
    with pytest.raises(GmpcError, match="both null"):
        eng.bilevel_grad_cotangent(B)
    with pytest.raises(GmpcError, match="lx must be"):
        eng.bilevel_grad_cotangent(B, d(np.zeros((B, T, n), np.float32)))
    with pytest.raises(GmpcError, match="lu must be"):
        eng.bilevel_grad_cotangent(B, lx, d(np.zeros((B, T, m + 1), np.float32)))
    eng.bilevel_grad_cotangent(B, lx)          # the refusals left the held solution usable


@pytest.mark.parametrize("name", ["trained-like", "tiny-ragged", "big-70"])
def test_repeated_calls_are_bitwise_deterministic(name):
    pb, _, eng, out, B = _solved(name)
    _, lx, lu = opt.loss_cotangents(huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
    first = eng.bilevel_grad_cotangent(B, lx, lu).cpu().numpy()
    s1 = _ctx_state(eng, B)
    for _ in range(2):
        np.testing.assert_array_equal(eng.bilevel_grad_cotangent(B, lx, lu).cpu().numpy(), first)
        s2 = _ctx_state(eng, B)
        for key in s1:
            np.testing.assert_array_equal(s2[key], s1[key], err_msg=key)
