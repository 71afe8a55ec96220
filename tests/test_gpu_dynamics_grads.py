"""gmpc_bilevel_grad_dynamics -- dL/dtheta_dyn through the iLQR solution -- and ilqr_layer(..., dynamics_grad=True),
on the GPU.

  1. at the GPU's own iterate, against the fp64 per-row form on the oracle's LQ model (tests/test_dynamics_grads_host.py
     shows it equals the dense autograd formula and finite differences of the solution), under the protocol of
     test_gpu_input_grads._check_inputs: HIP's Hessian-solve residual decides how far the gradient may move;
  2. linearity in lx, determinism, and that the call leaves grad_sum, Bvec, H, dX and the inputs call as they were;
  3. refusals;
  4. the torch layer: its dynamics range is the entry point's, the rest is the default call's, a dynamics model
     trains through it."""

import functools

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_bilevel_cotangent as cot
import test_gpu_input_grads as ig
import test_gpu_mirror as mirror
import test_gpu_parity as par
from gan_mpc_amd import _lib
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.norm import l2_policy
from gan_mpc_amd.policy import differentiable as dl
from gan_mpc_amd.policy import optimizers as opt
from test_dynamics_grads_host import reference

pytestmark = pytest.mark.gpu


def _check_dyn(pb, pb64, X, U, cot_fn, Hd, g):
    """g against fp64 at the GPU's iterate.  The bar: 1e-4, 10 x the fp32 oracle's error, or 4 x what a
    right-hand-side perturbation of the size of HIP's Hessian-solve residual does to the fp64 gradient; never above
    the slack ceiling."""
    X64, U64 = X.astype(np.float64), U.astype(np.float64)
    lx64, lu64 = cot_fn(np.float64)
    lx32, lu32 = cot_fn(np.float32)
    p64 = orc.cast_problem(pb64, np.float64)
    lqr = orc.get_lqr_params(p64["dyn"], p64["cmlp"], p64["mpc_w"], p64["goal"], X64, U64)
    Bv64 = orc.loss_grad_wrt_control(lqr[5], lqr[6], lx64) + lu64
    p32 = orc.cast_problem(pb, np.float32)
    lqr32 = orc.get_lqr_params(p32["dyn"], p32["cmlp"], p32["mpc_w"], p32["goal"], X.astype(np.float32),
                               U.astype(np.float32))
    Bv32 = orc.loss_grad_wrt_control(lqr32[5], lqr32[6], lx32) + lu32
    r = orc.hessian_apply(lqr, Hd.astype(np.float64)) - Bv64
    r_hip = np.sqrt((r ** 2).sum((1, 2)) / (Bv64 ** 2).sum((1, 2)))
    r32 = orc.hessian_apply(lqr, orc.hessian_solve(lqr32, Bv32)[0].astype(np.float64)) - Bv64
    r_o32 = np.sqrt((r32 ** 2).sum((1, 2)) / (Bv64 ** 2).sum((1, 2)))
    assert r_hip.max() <= max(1e-4, 10 * r_o32.max()), (r_hip, r_o32)
    ref64 = reference(pb64, X64, U64, lx64, lu64)
    ref32 = reference(p32, X.astype(np.float32), U.astype(np.float32), lx32, lu32)
    rng = np.random.default_rng(7)
    e = el = 0.0
    for _ in range(4):
        noise = rng.standard_normal(Bv64.shape)
        noise *= (r_hip * np.sqrt((Bv64 ** 2).sum((1, 2)) / (noise ** 2).sum((1, 2))))[:, None, None]
        gp = reference(pb64, X64, U64, lx64, lu64, noise=noise)
        e, el = max(e, gu.rel_err(gp, ref64)), max(el, gu.el_err(gp, ref64)[0])
    assert np.abs(ref64).max() > 0 and np.all(np.isfinite(g))
    gu.assert_parity("dynamics grad at the iterate", g, ref32, ref64, tol=min(max(1e-4, 4.0 * e), gu.GAIN_CEILING),
                     slack=10.0, ceiling=gu.GAIN_CEILING, el_tol=max(1e-3, 4.0 * el))


CASES = {
    "pendulum-B1/l2": (ig.PEND5_B1, False, "l2"),
    "pendulum-B7/cot": (ig.PEND5, False, "cot"),
    "cheetah/rounds/cot": (ig.CHEETAH5, False, "cot"),
    "cheetah/fused/cot": (ig.CHEETAH5, True, "cot"),
    "c3-w2h/l2": ("trained-like", False, "l2"),
    "c3-w2h/js": ("trained-like", False, "js"),
    "c3-w2h/cot": ("trained-like", False, "cot"),
    "tiny-ragged/cot": ("tiny-ragged", False, "cot"),
    "rw-128/cot": ("rw-128", False, "cot"),
    "rw-64/l2": ("rw-64", False, "l2"),
    "wide/cot": ("wide", False, "cot"),
    "wide-T20/cot": (ig.WIDE20, False, "cot"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_dynamics_grads_against_fp64_at_the_iterate(case):
    spec, fused, loss = CASES[case]
    pb, pb64, eng, out, B = cot._solved(spec, critic=True) if loss == "js" else ig._solved(spec, fused=fused)
    d = eng.to_dev
    T, m = eng.T, eng.m
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
    g = eng.bilevel_grad_dynamics(B, lx)
    assert g.shape == (eng.dyn_count,)
    _check_dyn(pb, pb64, X, U, cot_fn, Hd, g.cpu().numpy())


@pytest.mark.parametrize("name", ["trained-like", "tiny-ragged"])
def test_linear_in_lx_deterministic_and_read_only(name):
    pb, _, eng, out, B = ig._solved(name)
    d = eng.to_dev
    T, n = eng.T, eng.n
    _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
    g_sum = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy()
    before = ig._state(eng, B)
    # the inputs call first, then the dynamics call, then the inputs call again: same bits everywhere
    inputs = [a.cpu().numpy() for a in eng.bilevel_grad_inputs(B, lx)]
    first = eng.bilevel_grad_dynamics(B, lx).cpu().numpy()
    assert np.abs(first).max() > 0
    for _ in range(2):
        np.testing.assert_array_equal(eng.bilevel_grad_dynamics(B, lx).cpu().numpy(), first)
    for a, b in zip(eng.bilevel_grad_inputs(B, lx), inputs):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    after = ig._state(eng, B)
    for key in before:
        np.testing.assert_array_equal(after[key], before[key], err_msg=key)
    np.testing.assert_array_equal(eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy(), g_sum)
    # the dynamics call first this time: the inputs call still gives the same bits
    eng.bilevel_grad_dynamics(B, lx)
    for a, b in zip(eng.bilevel_grad_inputs(B, lx), inputs):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    # mu depends on lx linearly, lam and nu not at all (H fixed here): g(lx + dl) - g(lx) = g(dl) - g(0)
    rng = np.random.default_rng(3)
    dlx = d(rng.standard_normal((B, T + 1, n)).astype(np.float32) * 0.1)
    z = d(np.zeros((B, T + 1, n), np.float32))
    g = {k: eng.bilevel_grad_dynamics(B, v).cpu().numpy().astype(np.float64)
         for k, v in (("a", lx), ("ab", (lx + dlx).contiguous()), ("b", dlx), ("0", z))}
    lhs, rhs = g["ab"] - g["a"], g["b"] - g["0"]
    # (each side is a difference of two fp32 sums over 2 B T rows: 1.2e-4 measured at trained-like; a term that is
    # not linear in lx would show at O(1))
    assert gu.rel_err(lhs, rhs) <= 1e-3, gu.rel_err(lhs, rhs)


def test_refusals():
    pb, _, eng = par._setup("tiny-ragged")
    d = eng.to_dev
    B, T, n = pb["B"], pb["T"], pb["n"]
    lx = d(np.zeros((B, T + 1, n), np.float32))
    with pytest.raises(GmpcError, match="must precede"):
        eng.bilevel_grad_dynamics(B)
    eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 1})
    with pytest.raises(GmpcError, match="must precede"):       # a solve, but no bilevel tail
        eng.bilevel_grad_dynamics(B)
    eng.bilevel_grad_cotangent(B, lx)
    with pytest.raises(GmpcError, match="must precede"):
        eng.bilevel_grad_dynamics(B - 1)
    with pytest.raises(GmpcError, match="grad_dyn_sum is null"):
        _lib.check(eng.lib.gmpc_bilevel_grad_dynamics(eng.ctx, B, None, None, eng._stream()))
    with pytest.raises(GmpcError, match="lx must be"):
        eng.bilevel_grad_dynamics(B, d(np.zeros((B, T, n), np.float32)))
    eng.bilevel_grad_dynamics(B)                                 # the refusals left the state usable
    eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 1})
    with pytest.raises(GmpcError, match="must precede"):       # a new solve in between
        eng.bilevel_grad_dynamics(B)
    for name, match in (("dynl-small", "dyn_lstm_features"), ("big-70", "step-major")):
        pbx, _, engx = par._setup(name)
        dx = engx.to_dev
        engx.ilqr_solve(dx(pbx["x0"]), dx(pbx["U"]), dx(pbx["goal"]), {"maxiter": 1})
        engx.bilevel_grad(pbx["B"], 0, desired=dx(pbx["true_seq"]))
        with pytest.raises(GmpcError, match=match):
            engx.bilevel_grad_dynamics(pbx["B"])


# ---- the torch layer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["rounds", "fused"])
def test_layer_dynamics_gradient_is_the_entry_point(solver):
    config, policy, params, data = mirror._build(functools.partial(l2_policy.L2MPC, solver=solver))
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    idx = np.arange(8)
    dparams, x0, goal, init_U = ig._layer_inputs(policy, params, data, idx)
    des = torch.as_tensor(np.asarray(data["Y"][idx], np.float32), device=x0.device)
    flat = dparams.flat.requires_grad_(True)

    def run(dynamics_grad):
        flat.grad = None
        X, U = dl.ilqr_layer(policy, dparams, x0, goal, init_U, dynamics_grad=dynamics_grad)
        loss = ((X[..., : des.shape[-1]] - des) ** 2).mean(1).sum() + 0.05 * (U * U).sum()
        loss.backward()
        return X.detach(), U.detach(), flat.grad.clone()

    _, _, g_default = run(False)
    X, U, g = run(True)
    eng = policy._engine
    B = len(idx)
    lx = (2 * (X[..., : des.shape[-1]] - des) / X.shape[1])
    lx = torch.cat([lx, torch.zeros_like(X[..., des.shape[-1]:])], -1).contiguous()
    lu = (0.1 * U).contiguous()
    eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0)
    gdyn = eng.bilevel_grad_dynamics(B, lx)
    lo, cnt = dparams.range_of(("mpc_weights", "cost_params"))
    dlo, dcnt = dparams.range_of(("dynamics_params",))
    torch.testing.assert_close(g[dlo:dlo + dcnt], gdyn, rtol=1e-5, atol=1e-6 * float(gdyn.abs().max()))
    assert float(gdyn.abs().max()) > 0
    torch.testing.assert_close(g[lo:lo + cnt], g_default[lo:lo + cnt], rtol=1e-5,
                               atol=1e-6 * float(g_default.abs().max()))
    assert float(g_default[dlo:dlo + dcnt].abs().max()) == 0        # the default call leaves the range alone
    rest = g[dlo + dcnt:]                                            # the critic range (if any)
    assert rest.numel() == 0 or float(rest.abs().max()) == 0
    flat.requires_grad_(False)


@pytest.mark.parametrize("name,match", [("dynl-small", "dyn_lstm_features"), ("big-70", "n <= 64")])
def test_layer_refuses_dynamics_grad_at_forward(name, match):
    pb, _, eng = par._setup(name)

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
    solves = eng.solve_count
    with pytest.raises(GmpcError, match=match):
        dl.ilqr_layer(_P(), _DP(), d(pb["x0"]), d(pb["goal"]), d(pb["U"]), dynamics_grad=True)
    assert eng.solve_count == solves                                 # refused before any solve


def test_dynamics_model_trains_through_the_layer():
    """A few Adam steps on the dynamics range alone, through the layer, lower an L2 imitation loss of the solved
    states (the model fitted to a task loss on the planned trajectory)."""
    config, policy, params, data = mirror._build(l2_policy.L2MPC)
    policy.trajax_ilqr_kwargs["maxiter"] = 3
    idx = np.arange(8)
    dparams, x0, goal, init_U = ig._layer_inputs(policy, params, data, idx)
    nx = policy.engine_for(len(idx), dparams).nx
    des = torch.as_tensor(np.asarray(data["Y"][idx], np.float32), device=x0.device)
    flat = dparams.flat.requires_grad_(True)
    dlo, dcnt = dparams.range_of(("dynamics_params",))
    theta0 = flat.detach().clone()
    adam = torch.optim.Adam([flat], lr=2e-3)
    losses = []
    for _ in range(6):
        X, U = dl.ilqr_layer(policy, dparams, x0, goal, init_U, dynamics_grad=True)
        loss = ((X[..., :nx] - des) ** 2).mean()
        adam.zero_grad()
        loss.backward()
        with torch.no_grad():
            assert float(flat.grad[dlo:dlo + dcnt].abs().max()) > 0
            flat.grad[:dlo] = 0
            flat.grad[dlo + dcnt:] = 0
        adam.step()
        losses.append(float(loss.detach()))
    flat.requires_grad_(False)
    moved = (flat.detach() - theta0).abs()
    assert float(moved[:dlo].max()) == 0 and float(moved[dlo:dlo + dcnt].max()) > 0
    assert losses[-1] < losses[0], losses
