"""gmpc_rollout_vjp -- the VJP of the rollout and its per-step costs -- and policy.differentiable.rollout_layer, on the
GPU.

  1. every output against the fp64 per-step reference (tests/test_rollout_vjp_host.py shows it equals torch autograd
     and central differences) at the GPU's own fp32 (X, U), trajectories near a relu kink left out;
  2. cross-checks against verified kernels that work differently: gmpc_lqr_backward's grad / adjoints (Jacobians,
     Riccati sweep) for gX = 0, gc = 1, and gmpc_dynamics_loss_grad for the discounted-MSE cotangents;
  3. linearity in (gX, gc), determinism, NULL outputs;
  4. the call is read-only between a solve, its bilevel calls and the inputs / dynamics calls, and the one call
     workspace it shares with gmpc_expert_vjp, gmpc_expert_loss_grad and gmpc_bilevel_grad_dynamics carries nothing from
     one call into the next;
  5. refusals;
  6. the torch layer."""

import functools
import itertools

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_input_grads as ig
import test_gpu_mirror as mirror
import test_gpu_parity as par
from gan_mpc_amd import _lib
from gan_mpc_amd import params as P
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.engine import Engine, make_expert_shape
from gan_mpc_amd.norm import l2_policy
from gan_mpc_amd.policy import differentiable as dl
from test_rollout_vjp_host import reference

pytestmark = pytest.mark.gpu

SHAPES = {
    "pendulum-T5-B1": (3, 1, 5, 1, {}),
    "pendulum-T5-B7": (3, 1, 5, 7, {}),
    "cheetah-T5-B128": (17, 6, 5, 128, dict(out_scale=0.1)),
    "C3": (17, 6, 50, 1024, dict(out_scale=0.1)),
    "h128-one-layer": (9, 3, 12, 10, dict(dyn_hidden=(128,), cost_hidden=(32,), cost_fout=4, out_scale=0.3)),
    "h64-ragged": (6, 2, 9, 7, dict(dyn_hidden=(64, 37), cost_hidden=(16,), cost_fout=3, out_scale=0.3)),
    "tiny-ragged": (5, 2, 8, 7, dict(dyn_hidden=(33, 47), cost_hidden=(24,), cost_fout=6)),
    "big-70": (70, 7, 6, 5, dict(dyn_hidden=(128, 96), cost_hidden=(64,), cost_fout=12, out_scale=0.3)),
    "m40-n24": (24, 40, 5, 4, dict(dyn_hidden=(64, 48), cost_hidden=(32,), cost_fout=6, out_scale=0.3)),
    "c4-n376": (376, 17, 4, 3, dict(out_scale=0.3)),
}
KEYS = ("x0", "U", "goal", "theta", "dyn")


def _setup(name):
    n, m, T, B, kw = SHAPES[name]
    pb = gu.problem(n, m, T, B, seed=11, **kw)
    gu.set_config(f"rollout-vjp {name} n={n} m={m} T={T} B={B}")
    eng = gu.engine_for(pb, critic=False)
    d = eng.to_dev
    X, _ = eng.rollout_cost(d(pb["x0"]), d(pb["U"]), d(pb["goal"]))
    return pb, eng, X


def _cots(X, which, seed=5):
    rng = np.random.default_rng(seed)
    gX = rng.standard_normal(tuple(X.shape)).astype(np.float32) if which in ("gX", "both") else None
    gc = rng.standard_normal(tuple(X.shape[:2])).astype(np.float32) if which in ("gc", "both") else None
    return gX, gc


def _call(eng, X, U, goal, gX, gc, **want):
    d = lambda a: None if a is None else eng.to_dev(a)  # noqa: E731
    out = eng.rollout_vjp(X, d(U), d(goal), d(gX), d(gc), **want)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name,which", list(itertools.product(SHAPES, ("gX", "gc", "both"))))
def test_against_fp64_at_the_gpus_trajectory(name, which):
    pb, eng, Xd = _setup(name)
    pb64 = orc.cast_problem(pb, np.float64)
    X = Xd.cpu().numpy()
    T = pb["T"]
    X64, U64 = X.astype(np.float64), pb["U"].astype(np.float64)
    bad = gu.dyn_near_kink(pb64["dyn"], X64, U64).any(1) | gu.near_kink(pb64["cmlp"], X64[:, T])
    ok = ~bad
    assert ok.sum() >= max(1, pb["B"] // 2)
    X, U, goal = np.ascontiguousarray(X[ok]), np.ascontiguousarray(pb["U"][ok]), np.ascontiguousarray(pb["goal"][ok])
    gX, gc = _cots(X, which)
    got = _call(eng, eng.to_dev(X), U, goal, gX, gc)
    p32 = dict(pb, goal=goal)
    ref32 = reference(p32, X, U, goal, gX, gc)
    ref64 = reference(dict(pb64, goal=goal.astype(np.float64)), X.astype(np.float64), U.astype(np.float64),
                      goal.astype(np.float64), gX, gc)
    for key in KEYS:
        if which == "gX" and key in ("goal", "theta"):
            assert np.abs(got[key]).max() == 0, key       # no cost cotangent: nothing reaches these
            continue
        sums = key in ("theta", "dyn")
        gu.assert_parity(f"rollout vjp {key} ({which})", got[key], ref32[key], ref64[key],
                         tol=1e-4 if sums else gu.TOL, slack=10.0 if sums else 4.0,
                         el_tol=1e-2 if sums else 1e-3)


@pytest.mark.parametrize("name", list(SHAPES))
def test_cost_cotangent_of_ones_is_lqr_backwards_gradient(name):
    """gX = 0, gc = 1: dL/dU is the objective's gradient and dL/dx0 the first adjoint, which gmpc_lqr_backward forms
    from [A_t | B_t] and its adjoint sweep (step-major shapes: the large-state pipeline)."""
    pb, eng, X = _setup(name)
    B, T = pb["B"], pb["T"]
    d = eng.to_dev
    out = eng.lqr_backward(X, d(pb["U"]), d(pb["goal"]))
    got = _call(eng, X, pb["U"], pb["goal"], None, np.ones((B, T + 1), np.float32), want_theta=False,
                want_dyn=False)
    gU, adj = out["grad"].cpu().numpy(), out["adjoints"].cpu().numpy()
    assert gu.rel_err(got["U"], gU) <= 1e-4, gu.rel_err(got["U"], gU)
    assert gu.rel_err(got["x0"], adj[:, 0]) <= 1e-4, gu.rel_err(got["x0"], adj[:, 0])


@pytest.mark.parametrize("name", ["tiny-ragged", "cheetah-T5-B128", "h64-ragged"])
def test_discounted_mse_cotangent_is_the_dynamics_regression_gradient(name):
    """loss = sum_t discount^t |X_{t+1} - Y_t|^2 without teacher forcing (S = T) is gmpc_dynamics_loss_grad's loss of
    the sequences xseq[:, 0] = x0, useq = U: its dynamics gradient is the VJP's for gX_{t+1} = 2 discount^t (X_{t+1}
    - Y_t)."""
    pb, eng, Xd = _setup(name)
    B, T, n = pb["B"], pb["T"], pb["n"]
    d = eng.to_dev
    X = Xd.cpu().numpy()
    rng = np.random.default_rng(2)
    Y = (X[:, 1:] + 0.1 * rng.standard_normal(X[:, 1:].shape)).astype(np.float32)
    disc, gam = 0.9, np.float32(1.0)
    gX = np.zeros(X.shape, np.float32)
    for t in range(T):
        gX[:, t + 1] = 2 * gam * (X[:, t + 1] - Y[:, t])
        gam = np.float32(gam * np.float32(disc))
    xseq = np.zeros((B, T, n), np.float32)
    xseq[:, 0] = pb["x0"]
    _, want = eng.dynamics_loss_grad(d(xseq), d(pb["U"]), d(Y), disc, False)
    got = _call(eng, Xd, pb["U"], pb["goal"], gX, None, want_x0=False, want_U=False, want_goal=False,
                want_theta=False)
    want = want.cpu().numpy()
    assert np.abs(want).max() > 0
    assert gu.rel_err(got["dyn"], want) <= 1e-4, gu.rel_err(got["dyn"], want)


@pytest.mark.parametrize("name", ["tiny-ragged", "C3", "big-70"])
def test_linear_deterministic_and_null_outputs(name):
    pb, eng, X = _setup(name)
    U, goal = pb["U"], pb["goal"]
    gX1, gc1 = _cots(X, "both", 1)
    gX2, gc2 = _cots(X, "both", 2)
    full = _call(eng, X, U, goal, gX1, gc1)
    for _ in range(2):
        again = _call(eng, X, U, goal, gX1, gc1)
        for key in KEYS:
            np.testing.assert_array_equal(again[key], full[key], err_msg=key)
    # every combination of wanted outputs writes the same bits in what it does write
    flags = ("want_x0", "want_U", "want_goal", "want_theta", "want_dyn")
    for mask in range(1, 32):
        want = {f: bool(mask >> i & 1) for i, f in enumerate(flags)}
        part = _call(eng, X, U, goal, gX1, gc1, **want)
        for key, f in zip(KEYS, flags):
            if want[f]:
                np.testing.assert_array_equal(part[key], full[key], err_msg=f"{key} with {want}")
            else:
                assert part[key] is None
    # linear in (gX, gc)
    two = _call(eng, X, U, goal, gX2, gc2)
    both = _call(eng, X, U, goal, gX1 + gX2, gc1 + gc2)
    for key in KEYS:
        assert gu.rel_err(both[key], full[key].astype(np.float64) + two[key]) <= 1e-4, key


@pytest.mark.parametrize("name", ["trained-like", "tiny-ragged"])
def test_read_only_between_solve_and_bilevel_calls(name):
    from gan_mpc_amd.policy import optimizers as opt
    import test_gpu_bilevel_cotangent as cot
    pb, _, eng, out, B = ig._solved(name)
    d = eng.to_dev
    _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
    X, U, goal = out["X"], out["U"], d(pb["goal"])
    gX, gc = _cots(X, "both", 3)

    def vjp():
        return _call(eng, X, U.cpu().numpy(), pb["goal"], gX, gc)

    def chain(with_vjp):
        res = {}
        if with_vjp:
            vjp()
        res["cot"] = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy()
        if with_vjp:
            vjp()
        res["x0"], res["goal"] = [a.cpu().numpy() for a in eng.bilevel_grad_inputs(B, lx)]
        res["dyn"] = eng.bilevel_grad_dynamics(B, lx).cpu().numpy()
        if with_vjp:
            vjp()
        res["cot2"] = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy()
        res["state"] = ig._state(eng, B)
        return res

    plain = chain(False)
    first = vjp()
    mixed = chain(True)
    for key in ("cot", "x0", "goal", "dyn", "cot2"):
        np.testing.assert_array_equal(mixed[key], plain[key], err_msg=key)
    for key in plain["state"]:
        np.testing.assert_array_equal(mixed["state"][key], plain["state"][key], err_msg=key)
    for key in KEYS:
        np.testing.assert_array_equal(vjp()[key], first[key], err_msg=key)
    del goal


def test_call_workspace_is_shared_safely():
    """gmpc_rollout_vjp, gmpc_expert_vjp, gmpc_expert_loss_grad and gmpc_bilevel_grad_dynamics fill one call workspace
    of the context.  Each of them, for two expert variants and at B = 7 and B = 3, first on a fresh engine (nothing
    else has touched the workspace), then interleaved in two orders on a single engine, where a later call finds the
    buffers as an earlier, larger call with another row stride left them (dynamics rows 87 floats, cost rows 30,
    LSTM expert rows 133, MLP expert rows 118): every output has the fresh engine's bytes."""
    n, m, T, B, kw = SHAPES["tiny-ragged"]
    pb = gu.problem(n, m, T, B, seed=11, **kw)
    gu.set_config(f"call workspace tiny-ragged n={n} m={m} T={T} B={B}")
    rng = np.random.default_rng(9)
    experts = {}
    for name, F, layers in (("lstm", 13, 2), ("mlp", 0, 3)):     # F 13, one hidden head layer of 37; Y 37
        flat, F_, dx, du = P.pack_expert(orc.make_expert(rng, n, m, lstm_features=F, num_layers=layers,
                                                         num_hidden_units=37))
        experts[name] = (flat, make_expert_shape(F_, dx, du))
    hist, S = 1, 3
    rnd = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    first = gu.engine_for(pb, critic=False)
    X = first.rollout_cost(*(first.to_dev(pb[k]) for k in ("x0", "U", "goal")))[0].cpu().numpy()
    first.close()
    data = dict(gX=rnd(B, T + 1, n), gc=rnd(B, T + 1), history=rnd(B, hist + 1, n), g_goal=rnd(B, T + 1, n),
                g_U=rnd(B, T, m), xseq=rnd(B, S, n), useq=np.tanh(rnd(B, S, m)), yseq=rnd(B, S, n),
                lx=rnd(B, T + 1, n), lu=rnd(B, T, m))

    def run(eng, op, Bq):
        d = lambda a: eng.to_dev(np.ascontiguousarray(a[:Bq]))  # noqa: E731
        kind, _, variant = op.partition("/")
        if kind == "rollout_vjp":
            out = eng.rollout_vjp(d(X), d(pb["U"]), d(pb["goal"]), d(data["gX"]), d(data["gc"]))
        elif kind == "expert_vjp":
            flat, es = experts[variant]
            out = eng.expert_vjp(d(data["history"]), eng.to_dev(flat), es, d(data["g_goal"]), d(data["g_U"]))
        elif kind == "expert_loss_grad":
            flat, es = experts[variant]
            out = dict(zip(("loss", "grad"), eng.expert_loss_grad(d(data["xseq"]), d(data["useq"]), d(data["yseq"]),
                                                                  eng.to_dev(flat), es, 0.9, False)))
        else:
            eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 1})
            lx = d(data["lx"])
            out = dict(cot=eng.bilevel_grad_cotangent(Bq, lx, d(data["lu"]), sign=-1.0),
                       dyn=eng.bilevel_grad_dynamics(Bq, lx))
        return {k: v.cpu().numpy() for k, v in out.items()}

    ops = ("rollout_vjp", "expert_vjp/lstm", "expert_vjp/mlp", "expert_loss_grad/lstm", "expert_loss_grad/mlp",
           "bilevel_grad_dynamics")
    fresh = {}
    for op, Bq in itertools.product(ops, (B, 3)):
        eng = gu.engine_for(pb, critic=False)
        fresh[op, Bq] = run(eng, op, Bq)
        eng.close()
        assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in fresh[op, Bq].values()), (op, Bq)
    big = [(op, B) for op in ops]
    small = [(op, 3) for op in ops]
    orders = (big + small[::2] + big[::-1] + small[1::2],
              big[::-1] + small[::-1] + big[3:] + big[:3])
    eng = gu.engine_for(pb, critic=False)
    for i, order in enumerate(orders):
        for step, (op, Bq) in enumerate(order):
            got = run(eng, op, Bq)
            for key, want in fresh[op, Bq].items():
                np.testing.assert_array_equal(got[key], want, err_msg=f"order {i} step {step}: {op} B={Bq} {key}")
    eng.close()


def test_refusals():
    pb, eng, X = _setup("tiny-ragged")
    d = eng.to_dev
    B, T, n = pb["B"], pb["T"], pb["n"]
    U, goal = d(pb["U"]), d(pb["goal"])
    gX = d(np.ones((B, T + 1, n), np.float32))
    out = eng.new(B, n)
    lib, s = eng.lib, eng._stream()
    P = lambda t: None if t is None else _lib.C.c_void_p(t.data_ptr())  # noqa: E731

    def call(Bc=B, X_=X, U_=U, goal_=goal, gX_=gX, gc_=None, o=out, e=eng):
        _lib.check(e.lib.gmpc_rollout_vjp(e.ctx, Bc, P(X_), P(U_), P(goal_), P(gX_), P(gc_), P(o), None, None,
                                          None, None, s))

    with pytest.raises(GmpcError, match="both null"):
        call(gX_=None)
    with pytest.raises(GmpcError, match="every output is null"):
        call(o=None)
    for kw in (dict(X_=None), dict(U_=None), dict(goal_=None)):
        with pytest.raises(GmpcError, match="must not be null"):
            call(**kw)
    for Bc in (0, eng.max_batch + 1):
        with pytest.raises(GmpcError, match="outside"):
            call(Bc=Bc)
    call()                                            # the refusals left the ctx usable
    fresh = Engine(pb["n"], pb["m"], T, [n + pb["m"], 33, 47, n], [n, 24, 6], max_batch=B)
    with pytest.raises(GmpcError, match="gmpc_set_params has not been called"):
        call(e=fresh)
    fresh.close()
    pbl, _, engl = par._setup("dynl-small")
    dl_ = engl.to_dev
    Xl, _ = engl.rollout_cost(dl_(pbl["x0"]), dl_(pbl["U"]), dl_(pbl["goal"]))
    with pytest.raises(GmpcError, match="dyn_lstm_features"):
        engl.rollout_vjp(Xl, dl_(pbl["U"]), dl_(pbl["goal"]), gcost=dl_(np.ones(Xl.shape[:2], np.float32)))
    del lib


# ---- the torch layer ---------------------------------------------------------------------------------------------
def _layer_setup(maxiter=2):
    config, policy, params, data = mirror._build(l2_policy.L2MPC)
    policy.trajax_ilqr_kwargs["maxiter"] = maxiter
    idx = np.arange(8)
    dparams, x0, goal, init_U = ig._layer_inputs(policy, params, data, idx)
    return policy, dparams, x0, goal, init_U, data, idx


def test_layer_gradients_are_the_entry_points():
    policy, dparams, x0, goal, init_U, _, _ = _layer_setup()
    flat = dparams.flat.requires_grad_(True)
    x0 = x0.clone().requires_grad_(True)
    U = init_U.clone().requires_grad_(True)
    goal = goal.clone().requires_grad_(True)
    X, costs = dl.rollout_layer(policy, dparams, x0, U, goal)
    loss = 0.1 * (X * X).sum() + costs.sum()
    loss.backward()
    eng = policy._rollout_eng[1]
    ref = eng.rollout_vjp(X.detach(), U.detach(), goal.detach(), (0.2 * X.detach()).contiguous(),
                          torch.ones_like(costs))
    # (autograd forms dL/dX as 0.1 * (2 X): the same cotangent up to rounding)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))  # noqa: E731
    for got, key in ((x0.grad, "x0"), (U.grad, "U"), (goal.grad, "goal")):
        close(got, ref[key])
    lo, cnt = dparams.range_of(("mpc_weights", "cost_params"))
    dlo, dcnt = dparams.range_of(("dynamics_params",))
    close(flat.grad[lo:lo + cnt], ref["theta"])
    close(flat.grad[dlo:dlo + dcnt], ref["dyn"])
    assert float(ref["dyn"].abs().max()) > 0
    flat.requires_grad_(False)


def test_gradient_descent_on_U_lowers_the_cost():
    policy, dparams, x0, goal, init_U, _, _ = _layer_setup()
    U = init_U.clone().requires_grad_(True)
    costs = []
    for _ in range(10):
        X, c = dl.rollout_layer(policy, dparams, x0, U, goal, dynamics_grad=False)
        tot = c.sum()
        U.grad = None
        tot.backward()
        with torch.no_grad():
            U -= 0.01 * U.grad / U.grad.abs().max()
        costs.append(float(tot.detach()))
    assert costs[-1] < costs[0], costs


def test_dynamics_model_trains_on_a_multi_step_loss():
    policy, dparams, x0, goal, init_U, data, idx = _layer_setup()
    nx = dparams.sizes_of_state()[2]
    des = torch.as_tensor(np.asarray(data["Y"][idx], np.float32), device=x0.device)
    flat = dparams.flat.requires_grad_(True)
    dlo, dcnt = dparams.range_of(("dynamics_params",))
    theta0 = flat.detach().clone()
    adam = torch.optim.Adam([flat], lr=2e-3)
    losses = []
    for _ in range(6):
        X, _ = dl.rollout_layer(policy, dparams, x0, init_U, goal)
        w = torch.linspace(1.0, 0.5, X.shape[1] - 1, device=X.device)[None, :, None]
        loss = (w * (X[:, 1:, :nx] - des[:, 1:]) ** 2).mean()
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


@pytest.mark.parametrize("solver", ["rounds", "fused"])
def test_ilqr_layer_then_rollout_layer_backpropagates(solver):
    """The plan of ilqr_layer evaluated by rollout_layer: one backward through both equals the hand-composed entry
    points (the rollout VJP, its dL/dU into the bilevel cotangent call and the inputs call)."""
    config, policy, params, data = mirror._build(functools.partial(l2_policy.L2MPC, solver=solver))
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    idx = np.arange(8)
    dparams, x0, goal, init_U = ig._layer_inputs(policy, params, data, idx)
    flat = dparams.flat.requires_grad_(True)
    x0 = x0.clone().requires_grad_(True)
    goal = goal.clone().requires_grad_(True)
    Xs, Us = dl.ilqr_layer(policy, dparams, x0, goal, init_U)
    X, costs = dl.rollout_layer(policy, dparams, x0, Us, goal)
    loss = costs.sum() + 0.1 * (X * X).sum()
    loss.backward()
    B = len(idx)
    reng, eng = policy._rollout_eng[1], policy._engine
    r = reng.rollout_vjp(X.detach(), Us.detach(), goal.detach(), (0.2 * X.detach()).contiguous(),
                         torch.ones_like(costs))
    lx = torch.zeros_like(Xs)
    g_sum = eng.bilevel_grad_cotangent(B, lx, r["U"], sign=-1.0)
    gx0, ggoal = eng.bilevel_grad_inputs(B, lx)
    tol = dict(rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(x0.grad, r["x0"] + gx0, **tol)
    torch.testing.assert_close(goal.grad, r["goal"] + ggoal, **tol)
    lo, cnt = dparams.range_of(("mpc_weights", "cost_params"))
    dlo, dcnt = dparams.range_of(("dynamics_params",))
    torch.testing.assert_close(flat.grad[lo:lo + cnt], r["theta"] + g_sum,
                               rtol=1e-5, atol=1e-6 * float(g_sum.abs().max()))
    torch.testing.assert_close(flat.grad[dlo:dlo + dcnt], r["dyn"], rtol=1e-5, atol=1e-6 * float(r["dyn"].abs().max()))
    assert float(gx0.abs().max()) > 0 and float(r["x0"].abs().max()) > 0
    flat.requires_grad_(False)
