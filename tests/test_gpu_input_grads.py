"""gmpc_bilevel_grad_inputs -- dL/dx0 and dL/dgoal through the iLQR solution -- and the torch layer built on it
(gan_mpc_amd/policy/differentiable.py), on the GPU.

  1. at the GPU's own iterate, against the fp64 recursions on the oracle's LQ model (tests/test_input_grads_host.py
     shows those equal the dense autograd formula and finite differences of the solution); the bars follow
     check_bilevel_at_iterate: HIP's Hessian-solve residual decides how far the gradient may move;
  2. linearity in lx, determinism, and that the call leaves grad_sum, Bvec, H and dX as they were;
  3. refusals;
  4. the torch layer: its gradients are the entry points', a stale backward raises, an expert-like goal model
     trains through it."""

import functools

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_bilevel_cotangent as cot
import test_gpu_mirror as mirror
import test_gpu_parity as par
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.norm import l2_policy
from gan_mpc_amd.policy import differentiable as dl
from gan_mpc_amd.policy import optimizers as opt
from test_input_grads_host import recursions_from

pytestmark = pytest.mark.gpu


def _solved(spec, fused=False):
    """cot._solved for a parity-table name or a (label, n, m, T, B, kw) tuple: solved (3 iterations), trajectories at
    a relu kink dropped, the rest re-solved with maxiter 0 so that the ctx holds exactly them."""
    if isinstance(spec, str):
        return cot._solved(spec, fused=fused)
    label, n, m, T, B, kw = spec
    pb = gu.problem(n, m, T, B, seed=11, **kw)
    gu.set_config(f"{label} n={n} m={m} T={T} B={B}")
    pb64, eng = orc.cast_problem(pb, np.float64), gu.engine_for(pb, critic=False)
    solve = eng.ilqr_solve_fused if fused else eng.ilqr_solve
    d = eng.to_dev
    out = solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 3})
    Xf, Uf = out["X"].cpu().numpy().astype(np.float64), out["U"].cpu().numpy()
    ok = ~(gu.dyn_near_kink(pb64["dyn"], Xf, Uf.astype(np.float64)).any(1) | gu.near_kink(pb64["cmlp"], Xf[:, T]))
    assert ok.sum() >= max(1, B // 2)
    for p_ in (pb, pb64):
        for key in ("x0", "goal", "true_seq"):
            p_[key] = p_[key][ok]
    out = solve(d(pb["x0"]), d(Uf[ok]), d(pb["goal"]), {"maxiter": 0})
    return pb, pb64, eng, out, int(ok.sum())


def _stages(p, X, U, cot_fn, dt):
    Xa, Ua = X.astype(dt), U.astype(dt)
    lqr = orc.get_lqr_params(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], Xa, Ua)
    lx, lu = cot_fn(dt)
    Bv = orc.loss_grad_wrt_control(lqr[5], lqr[6], lx) + lu
    lq = orc.second_order_lqr(p["dyn"], lqr, orc.adjoint(lqr[5], lqr[6], lqr[1], lqr[3])[1], Xa, Ua)
    H, dX = orc.hessian_solve(lq, Bv)
    gx0, gg = recursions_from(lq, lqr[0], lx, H, dX, p["goal"].shape[-1])
    return dict(lq=lq, Q0=lqr[0], lx=lx, Bv=Bv, gx0=gx0, gg=gg)


def _check_inputs(pb, pb64, X, U, cot_fn, Hd, gx0, gg):
    """gx0 (None on the step-major pipeline) and gg against fp64 at the GPU's iterate.  The bar: 1e-4, 10 x the fp32
    oracle's error, or 4 x what a right-hand-side perturbation of the size of HIP's Hessian-solve residual does to
    the fp64 gradient; never above the slack ceiling."""
    s32, s64 = _stages(pb, X, U, cot_fn, np.float32), _stages(pb64, X, U, cot_fn, np.float64)
    lq, Bv64, nx = s64["lq"], s64["Bv"], pb["goal"].shape[-1]
    r = orc.hessian_apply(lq, Hd.astype(np.float64)) - Bv64
    r_hip = np.sqrt((r ** 2).sum((1, 2)) / (Bv64 ** 2).sum((1, 2)))
    r32 = orc.hessian_apply(lq, orc.hessian_solve(s32["lq"], s32["Bv"])[0].astype(np.float64)) - Bv64
    r_o32 = np.sqrt((r32 ** 2).sum((1, 2)) / (Bv64 ** 2).sum((1, 2)))
    assert r_hip.max() <= max(1e-4, 10 * r_o32.max()), (r_hip, r_o32)
    rng = np.random.default_rng(7)
    pert = {"x0": (0.0, 0.0), "goal": (0.0, 0.0)}
    for _ in range(4):
        noise = rng.standard_normal(Bv64.shape)
        noise *= (r_hip * np.sqrt((Bv64 ** 2).sum((1, 2)) / (noise ** 2).sum((1, 2))))[:, None, None]
        Hp, dXp = orc.hessian_solve(lq, Bv64 + noise)
        px0, pg = recursions_from(lq, s64["Q0"], s64["lx"], Hp, dXp, nx)
        for key, a, ref in (("x0", px0, s64["gx0"]), ("goal", pg, s64["gg"])):
            e, el = pert[key]
            pert[key] = (max(e, gu.rel_err(a, ref)), max(el, gu.el_err(a, ref)[0]))
    for key, hip in (("x0", gx0), ("goal", gg)):
        if hip is None:
            continue
        ref32, ref64 = (s32["gx0"], s64["gx0"]) if key == "x0" else (s32["gg"], s64["gg"])
        e, el = pert[key]
        assert np.abs(ref64).max() > 0
        # (downstream of the Hessian solve, whose fp32 accuracy is conditioning-limited on the 17 x 6 shapes with the
        # Huber + control right-hand side -- see test_gpu_bilevel_cotangent._check_at_iterate: the fp32 oracle's own
        # error reaches 7e-4 there -- so the slack branch takes the gain ceiling)
        gu.assert_parity(f"input grad {key} at the iterate", hip, ref32, ref64,
                         tol=min(max(1e-4, 4.0 * e), gu.GAIN_CEILING), slack=10.0, ceiling=gu.GAIN_CEILING,
                         el_tol=max(1e-3, 4.0 * el))


def _state(eng, B):
    s = cot._ctx_state(eng, B)
    s["lx"] = eng.debug_buffer(11, (B, eng.T + 1, eng.n)).cpu().numpy()
    return s


PEND5 = ("pendulum-T5", 3, 1, 5, 7, {})
PEND5_B1 = ("pendulum-T5-B1", 3, 1, 5, 1, {})
CHEETAH5 = ("cheetah-T5", 17, 6, 5, 128, dict(out_scale=0.1))
# n > 32 over several chunks of the adjoint sweep with a ragged last one (out_scale: at 1.0 the random dynamics reach
# |x| ~ 3.5e3 over 20 steps)
WIDE20 = ("wide-T20", 40, 9, 20, 4, dict(dyn_hidden=(256, 64), cost_hidden=(256, 100), cost_fout=32, out_scale=0.1))
CASES = {
    "pendulum-B1/l2": (PEND5_B1, False, "l2"),
    "pendulum-B7/cot": (PEND5, False, "cot"),
    "cheetah/rounds/cot": (CHEETAH5, False, "cot"),
    "cheetah/fused/cot": (CHEETAH5, True, "cot"),
    "cheetah/fused/l2": (CHEETAH5, True, "l2"),
    "c3-w2h/l2": ("trained-like", False, "l2"),
    "c3-w2h/js": ("trained-like", False, "js"),
    "c3-valu/cot": ("trained-like", False, "cot"),
    "tiny-ragged/cot": ("tiny-ragged", False, "cot"),
    "dynl-small/cot": ("dynl-small", False, "cot"),
    "dynl-small/l2": ("dynl-small", False, "l2"),
    "big-70/cot": ("big-70", False, "cot"),
    "m40-n24/l2": ("m40-n24", False, "l2"),
    "wide/cot": ("wide", False, "cot"),
    "wide-T20/cot": (WIDE20, False, "cot"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_input_grads_against_fp64_at_the_iterate(case, monkeypatch):
    spec, fused, loss = CASES[case]
    if "valu" in case:
        monkeypatch.setenv("GMPC_RICCATI", "valu")
    pb, pb64, eng, out, B = cot._solved(spec, critic=True) if loss == "js" else _solved(spec, fused=fused)
    d = eng.to_dev
    T, n, m = eng.T, eng.n, eng.m
    X, U = out["X"].cpu().numpy(), out["U"].cpu().numpy()
    if loss == "l2":
        eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]), sign=-1.0)
        cot_fn = lambda dt: (orc.l2_loss_grad_x(X.astype(dt), pb["true_seq"].astype(dt)),  # noqa: E731
                             np.zeros((B, T, m), dt))
        lx = None
    elif loss == "js":
        eng.bilevel_grad(B, 1, critic=d(gu.critic_flat(pb)), sign=-1.0)
        cot_fn = lambda dt: (orc.generator_loss_grad_x(orc.cast_problem(pb, dt)["critic"], X.astype(dt)),  # noqa: E731
                             np.zeros((B, T, m), dt))
        lx = None
    else:
        _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
        eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0)
        cot_fn = lambda dt: cot._cot_host(cot.huber_u_loss, X, U, pb["true_seq"], dt)[1:]  # noqa: E731
    Hd = cot._ctx_state(eng, B)["H"]
    gx0, gg = eng.bilevel_grad_inputs(B, lx, want_x0=not eng.big)
    assert gg.shape == (B, T + 1, eng.nx) and (gx0 is None) == eng.big
    gg = gg.cpu().numpy()
    assert np.all(gg[:, T] == 0)
    _check_inputs(pb, pb64, X, U, cot_fn, Hd, None if gx0 is None else gx0.cpu().numpy(), gg)
    if eng.big:
        with pytest.raises(GmpcError, match="step-major"):
            eng.bilevel_grad_inputs(B, lx, want_goal=False)
    else:
        # the goal-only kernel and the x0 sweep's goal output agree
        _, gg2 = eng.bilevel_grad_inputs(B, lx, want_x0=False)
        np.testing.assert_allclose(gg2.cpu().numpy(), gg, rtol=1e-5, atol=1e-6 * np.abs(gg).max())


@pytest.mark.parametrize("name", ["trained-like", "tiny-ragged", "dynl-small", "big-70"])
def test_linear_in_lx_deterministic_and_read_only(name):
    pb, _, eng, out, B = _solved(name)
    d = eng.to_dev
    T, n = eng.T, eng.n
    want_x0 = not eng.big
    _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
    g_sum = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy()
    before = _state(eng, B)
    first = [None if a is None else a.cpu().numpy() for a in eng.bilevel_grad_inputs(B, lx, want_x0=want_x0)]
    for _ in range(2):
        again = [None if a is None else a.cpu().numpy() for a in eng.bilevel_grad_inputs(B, lx, want_x0=want_x0)]
        for a, b in zip(again, first):
            if b is not None:
                np.testing.assert_array_equal(a, b)
    after = _state(eng, B)
    for key in before:
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)
    np.testing.assert_array_equal(eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy(), g_sum)
    if want_x0:
        # mu depends on lx linearly, nu on H (fixed here): x0(lx + dl) - x0(lx) = x0(dl) - x0(0)
        rng = np.random.default_rng(3)
        dlx = d(rng.standard_normal((B, T + 1, n)).astype(np.float32) * 0.1)
        z = d(np.zeros((B, T + 1, n), np.float32))
        g = {k: eng.bilevel_grad_inputs(B, v, want_goal=False)[0].cpu().numpy().astype(np.float64)
             for k, v in (("a", lx), ("ab", (lx + dlx).contiguous()), ("b", dlx), ("0", z))}
        lhs, rhs = g["ab"] - g["a"], g["b"] - g["0"]
        assert gu.rel_err(lhs, rhs) <= 1e-5, gu.rel_err(lhs, rhs)


def test_refusals():
    pb, _, eng = par._setup("tiny-ragged")
    d = eng.to_dev
    B, T, n = pb["B"], pb["T"], pb["n"]
    lx = d(np.zeros((B, T + 1, n), np.float32))
    with pytest.raises(GmpcError, match="must precede"):
        eng.bilevel_grad_inputs(B)
    eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 1})
    with pytest.raises(GmpcError, match="must precede"):       # a solve, but no bilevel tail
        eng.bilevel_grad_inputs(B)
    eng.bilevel_grad_cotangent(B, lx)
    with pytest.raises(GmpcError, match="must precede"):
        eng.bilevel_grad_inputs(B - 1)
    with pytest.raises(GmpcError, match="both null"):
        eng.bilevel_grad_inputs(B, want_x0=False, want_goal=False)
    with pytest.raises(GmpcError, match="lx must be"):
        eng.bilevel_grad_inputs(B, d(np.zeros((B, T, n), np.float32)))
    eng.bilevel_grad_inputs(B)                                   # the refusals left the state usable
    eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 1})
    with pytest.raises(GmpcError, match="must precede"):       # a solve in between
        eng.bilevel_grad_inputs(B)
    pbb, _, engb = par._setup("big-70")
    db = engb.to_dev
    engb.ilqr_solve(db(pbb["x0"]), db(pbb["U"]), db(pbb["goal"]), {"maxiter": 1})
    engb.bilevel_grad(pbb["B"], 0, desired=db(pbb["true_seq"]))
    with pytest.raises(GmpcError, match="step-major"):
        engb.bilevel_grad_inputs(pbb["B"])
    engb.bilevel_grad_inputs(pbb["B"], want_x0=False)


# ---- the torch layer ---------------------------------------------------------------------------------------------
def _layer_inputs(policy, params, data, idx):
    dparams = policy.to_device_params(params)
    hx = np.asarray(data["hist"][idx], np.float32)
    policy.expert_model.select(idx)
    goal, init_U = policy.get_goal_states_init_actions(hx, dparams)
    eng = policy.engine_for(len(idx), dparams)
    d = eng.to_dev
    x0 = d(hx[:, -1])
    if eng.n > eng.nx:
        x0 = torch.cat([x0, d(policy.get_dynamics_carry(hx))], dim=1).contiguous()
    return dparams, x0, d(goal), d(init_U)


@pytest.mark.parametrize("solver", ["rounds", "fused"])
def test_layer_gradients_are_the_entry_points(solver):
    config, policy, params, data = mirror._build(functools.partial(l2_policy.L2MPC, solver=solver))
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    idx = np.arange(8)
    dparams, x0, goal, init_U = _layer_inputs(policy, params, data, idx)
    des = torch.as_tensor(np.asarray(data["Y"][idx], np.float32), device=x0.device)
    flat = dparams.flat.requires_grad_(True)
    x0r, goalr = x0.clone().requires_grad_(True), goal.clone().requires_grad_(True)
    X, U = dl.ilqr_layer(policy, dparams, x0r, goalr, init_U)
    loss = ((X[..., : des.shape[-1]] - des) ** 2).mean(1).sum() + 0.05 * (U * U).sum()
    loss.backward()
    eng = policy._engine
    B = len(idx)
    lx = (2 * (X.detach()[..., : des.shape[-1]] - des) / X.shape[1])
    lx = torch.cat([lx, torch.zeros_like(X[..., des.shape[-1]:])], -1).contiguous()
    lu = (0.1 * U.detach()).contiguous()
    g = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0)
    gx0, gg = eng.bilevel_grad_inputs(B, lx)
    lo, cnt = dparams.range_of(("mpc_weights", "cost_params"))
    torch.testing.assert_close(flat.grad[lo:lo + cnt], g, rtol=1e-5, atol=1e-6 * float(g.abs().max()))
    assert float(flat.grad[lo + cnt:].abs().max()) == 0
    torch.testing.assert_close(x0r.grad, gx0, rtol=1e-5, atol=1e-6 * float(gx0.abs().max()))
    torch.testing.assert_close(goalr.grad, gg, rtol=1e-5, atol=1e-6 * float(gg.abs().max()))
    assert float(gx0.abs().max()) > 0 and float(gg.abs().max()) > 0
    flat.requires_grad_(False)


def test_stale_backward_raises():
    config, policy, params, data = mirror._build(l2_policy.L2MPC)
    policy.trajax_ilqr_kwargs["maxiter"] = 1
    dparams, x0, goal, init_U = _layer_inputs(policy, params, data, np.arange(8))
    goalr = goal.clone().requires_grad_(True)
    X, U = dl.ilqr_layer(policy, dparams, x0, goalr, init_U)
    dl.ilqr_layer(policy, dparams, x0, goal, init_U)            # another solve on the same engine
    with pytest.raises(RuntimeError, match="another iLQR solve"):
        X.sum().backward()


def test_goal_model_trains_through_the_layer():
    """A torch.nn.Linear maps the current state to the goal sequence; a few Adam steps through the layer lower an L2
    imitation loss of the solved states."""
    config, policy, params, data = mirror._build(l2_policy.L2MPC)
    policy.trajax_ilqr_kwargs["maxiter"] = 3
    idx = np.arange(8)
    dparams, x0, goal, init_U = _layer_inputs(policy, params, data, idx)
    eng = policy.engine_for(len(idx), dparams)
    B, T, nx = len(idx), eng.T, eng.nx
    des = torch.as_tensor(np.asarray(data["Y"][idx], np.float32), device=x0.device)
    torch.manual_seed(0)
    lin = torch.nn.Linear(nx, (T + 1) * nx).to(x0.device)
    with torch.no_grad():
        lin.weight.mul_(0.1)
        lin.bias.copy_(goal.mean(0).reshape(-1))
    adam = torch.optim.Adam(lin.parameters(), lr=0.05)
    losses = []
    for _ in range(6):
        g = lin(x0[:, :nx]).reshape(B, T + 1, nx)
        X, U = dl.ilqr_layer(policy, dparams, x0, g, init_U)
        loss = ((X[..., :nx] - des) ** 2).mean()
        adam.zero_grad()
        loss.backward()
        assert lin.weight.grad is not None and float(lin.weight.grad.abs().max()) > 0
        adam.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses


def test_x0_gradient_refused_at_forward_on_a_large_state_shape():
    pb, _, eng = par._setup("big-70")

    class _P:                        # the policy surface ilqr_layer touches
        solver, trajax_ilqr_kwargs = "rounds", {"maxiter": 1}

        def to_device_params(self, p):
            return p

        def bind(self, dparams, B):
            return eng

    class _DP:
        flat = torch.zeros(1, device=eng.device)

        def range_of(self, keys):
            return 0, 1
    d = eng.to_dev
    with pytest.raises(GmpcError, match="step-major"):
        dl.ilqr_layer(_P(), _DP(), d(pb["x0"]).requires_grad_(True), d(pb["goal"]), d(pb["U"]))
