"""gmpc_expert_vjp -- the VJP of the expert sequence model's rollout -- and policy.differentiable.expert_layer, on the
GPU: against the torch restatement of the rollout schedule (tests/expert_vjp_ref.py) in fp32 and fp64, against
gmpc_expert_loss_grad for the cotangents of its own loss, the structure of the backward pass, statelessness between
a solve and its bilevel calls, the refusals, and the layer alone and composed with ilqr_layer / rollout_layer."""

import functools
import itertools

import numpy as np
import pytest
import torch

import expert_fit_ref as R
import expert_vjp_ref as V
import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_input_grads as ig
import test_gpu_mirror as mirror
from gan_mpc_amd import params as P
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.engine import Engine, make_expert_shape
from gan_mpc_amd.norm import l2_policy
from gan_mpc_amd.policy import differentiable as dl

pytestmark = pytest.mark.gpu

# name: (x_size, m, F (0 = MLP variant), num_layers, num_hidden_units, B, hist, T)
CASES = {
    "lstm-pendulum": (3, 1, 128, 3, 128, 7, 3, 5),
    "mlp-pendulum": (3, 1, 0, 3, 128, 7, 3, 5),
    "lstm-cheetah": (17, 6, 128, 3, 128, 64, 3, 5),
    "mlp-cheetah": (17, 6, 0, 3, 128, 64, 1, 5),
    "lstm-ragged": (5, 3, 13, 2, 37, 7, 1, 4),
    "mlp-ragged": (7, 5, 0, 3, 37, 9, 3, 3),
    "lstm-T50": (17, 6, 64, 3, 128, 16, 2, 50),
    "lstm-wide": (376, 17, 64, 3, 128, 8, 2, 4),
    "lstm-B1": (3, 1, 16, 2, 24, 1, 2, 5),
    "lstm-T1": (3, 1, 16, 2, 24, 5, 2, 1),
    "lstm-1layer": (4, 2, 8, 1, 16, 5, 2, 3),
    "mlp-1layer": (4, 2, 0, 2, 16, 5, 2, 3),
}
WHICH = ("goal", "U", "both")


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's model, its history with the windows at a relu kink left out, and the cotangents (read-only)."""
    n, m, F, layers, hidden, B, hist, T = CASES[name]
    rng = np.random.default_rng(7)
    ex = orc.make_expert(rng, n, m, lstm_features=F, num_layers=layers, num_hidden_units=hidden)
    W, b = ex["head_x"][-1]
    ex["head_x"][-1] = ((0.3 * W).astype(np.float32), (0.3 * b).astype(np.float32))
    flat, F_, dx, du = P.pack_expert(ex)
    history = rng.standard_normal((B, hist + 1, n)).astype(np.float32)
    keep = ~V.near_kink(flat, F_, dx, du, history, T)
    assert keep.sum() >= 0.75 * B, f"{name}: only {keep.sum()} of {B} windows away from a relu kink"
    history = np.ascontiguousarray(history[keep])
    Bk = int(keep.sum())
    rc = np.random.default_rng(5)
    g_goal = rc.standard_normal((Bk, T + 1, n)).astype(np.float32)
    g_U = rc.standard_normal((Bk, T, m)).astype(np.float32)
    for a in (flat, history, g_goal, g_U):
        a.setflags(write=False)
    return dict(n=n, m=m, T=T, B=B, Bk=Bk, hist=hist, model=(flat, F_, dx, du), history=history, g_goal=g_goal, g_U=g_U)


@functools.lru_cache(maxsize=None)
def _reference(name, which):
    cs = _case(name)
    gg = cs["g_goal"] if which in ("goal", "both") else None
    gu_ = cs["g_U"] if which in ("U", "both") else None
    return tuple(V.vjp(*cs["model"], cs["history"], cs["T"], gg, gu_, dtype=dt) for dt in (np.float32, np.float64))


def _engine(cs):
    n, m = cs["n"], cs["m"]
    return Engine(n, m, cs["T"], [n + m, 8, n], [n, 1], max_batch=cs["B"])


def _call(eng, cs, g_goal, g_U, history=None, **want):
    d = lambda a: None if a is None else eng.to_dev(a)  # noqa: E731
    flat, F, dx, du = cs["model"]
    out = eng.expert_vjp(d(cs["history"] if history is None else history), d(flat), make_expert_shape(F, dx, du),
                         d(g_goal), d(g_U), **want)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name,which", list(itertools.product(CASES, WHICH)))
def test_against_fp32_and_fp64_autograd(name, which):
    cs = _case(name)
    gu.set_config(f"expert-vjp {name} cotangent={which} kept {cs['Bk']}/{cs['B']}")
    (p32, h32), (p64, h64) = _reference(name, which)
    eng = _engine(cs)
    out = _call(eng, cs, cs["g_goal"] if which in ("goal", "both") else None,
                cs["g_U"] if which in ("U", "both") else None)
    eng.close()
    for key, got, o32, o64 in (("params", out["params"], p32, p64), ("history", out["history"], h32, h64)):
        print(f"{name} {which} {key}: hip {gu.rel_err(got, o64):.3e} fp32 ref {gu.rel_err(o32, o64):.3e}")
        gu.assert_parity(f"expert vjp grad_{key} {name} {which}", got, o32, o64)


@pytest.mark.parametrize("name", ["mlp-cheetah", "mlp-ragged"])
def test_mse_cotangents_give_expert_loss_grads_gradient(name):
    """The cotangents of the discounted MSE at the GPU's own rollout: the parameter gradient is the one
    gmpc_expert_loss_grad computes (teacher forcing off, S = T) -- two fp32 sums in different orders."""
    cs = _case(name)
    flat, F, dx, du = cs["model"]
    n, m, T, Bk, hist = cs["n"], cs["m"], cs["T"], cs["Bk"], cs["hist"]
    eng = _engine(cs)
    d = eng.to_dev
    es = make_expert_shape(F, dx, du)
    goal, U = (a.cpu().numpy() for a in eng.expert_rollout(d(cs["history"]), d(flat), es))
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((Bk, T, n)).astype(np.float32)
    A = np.tanh(rng.standard_normal((Bk, T, m))).astype(np.float32)
    gamma = 0.9
    disc = R.discounts(T, gamma, np.float32)[None, :, None]
    g_goal = np.zeros_like(goal)
    g_goal[:, 1:] = 2 * disc * (goal[:, 1:] - Y)
    g_U = (2 * disc * (U - A)).astype(np.float32)
    got = _call(eng, cs, g_goal, g_U, want_history=False)["params"]
    xseq = np.zeros((Bk, T, n), np.float32)
    xseq[:, 0] = cs["history"][:, hist]
    _, want = eng.expert_loss_grad(d(xseq), d(A), d(Y), d(flat), es, gamma, False)
    want = want.cpu().numpy()
    eng.close()
    assert np.abs(want).max() > 1e-3
    print(f"{name}: vjp vs expert_loss_grad {gu.rel_err(got, want):.3e}")
    assert gu.rel_err(got, want) <= 1e-4


@pytest.mark.parametrize("name", ["lstm-ragged", "mlp-ragged", "lstm-cheetah", "mlp-cheetah", "lstm-B1"])
def test_structure_linearity_determinism_and_null_arguments(name):
    cs = _case(name)
    n, T, Bk, hist = cs["n"], cs["T"], cs["Bk"], cs["hist"]
    eng = _engine(cs)
    g1, u1 = cs["g_goal"], cs["g_U"]
    full = _call(eng, cs, g1, u1)
    for _ in range(2):
        again = _call(eng, cs, g1, u1)
        for key in ("params", "history"):
            np.testing.assert_array_equal(again[key], full[key], err_msg=key)
    # a NULL output leaves the other one's bits alone
    only_p = _call(eng, cs, g1, u1, want_history=False)
    only_h = _call(eng, cs, g1, u1, want_params=False)
    assert only_p["history"] is None and only_h["params"] is None
    np.testing.assert_array_equal(only_p["params"], full["params"])
    np.testing.assert_array_equal(only_h["history"], full["history"])
    # a NULL cotangent is a zero one
    for gg, uu, zg, zu in ((g1, None, g1, np.zeros_like(u1)), (None, u1, np.zeros_like(g1), u1)):
        null, zero = _call(eng, cs, gg, uu), _call(eng, cs, zg, zu)
        for key in ("params", "history"):
            np.testing.assert_array_equal(null[key], zero[key], err_msg=key)
    # MLP variant: no carry, the teacher-forced rows reach nothing
    if cs["model"][1] == 0:
        assert np.abs(full["history"][:, :hist]).max() == 0
    else:
        assert np.abs(full["history"][:, :hist]).max() > 0
    assert np.abs(full["history"][:, hist]).max() > 0 and np.abs(full["params"]).max() > 0
    # goal[0] = history[hist]: its cotangent passes straight through and reaches no parameter
    g0 = np.zeros_like(g1)
    g0[:, 0] = g1[:, 0]
    first = _call(eng, cs, g0, None)
    np.testing.assert_array_equal(first["history"][:, hist], g0[:, 0])
    assert np.abs(first["history"][:, :hist]).max() == 0 and np.abs(first["params"]).max() == 0
    # linear in (g_goal, g_U)
    rng = np.random.default_rng(9)
    g2 = rng.standard_normal(g1.shape).astype(np.float32)
    u2 = rng.standard_normal(u1.shape).astype(np.float32)
    two, both = _call(eng, cs, g2, u2), _call(eng, cs, g1 + g2, u1 + u2)
    for key in ("params", "history"):
        assert gu.rel_err(both[key], full[key].astype(np.float64) + two[key]) <= 1e-4, key
    eng.close()


@pytest.mark.parametrize("name", ["tiny-ragged", "trained-like"])
def test_read_only_between_solve_and_bilevel_calls(name):
    from gan_mpc_amd.policy import optimizers as opt
    import test_gpu_bilevel_cotangent as cot
    pb, _, eng, out, B = ig._solved(name)
    _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
    n, m, T, hist = eng.nx, eng.m, eng.T, 2
    rng = np.random.default_rng(7)
    ex = orc.make_expert(rng, n, m, lstm_features=16, num_layers=2, num_hidden_units=24)
    flat, F, dx, du = P.pack_expert(ex)
    cs = dict(model=(flat, F, dx, du), history=rng.standard_normal((B, hist + 1, n)).astype(np.float32))
    g_goal = rng.standard_normal((B, T + 1, n)).astype(np.float32)
    g_U = rng.standard_normal((B, T, m)).astype(np.float32)

    def vjp():
        return _call(eng, cs, g_goal, g_U)

    def chain(where):
        res = {}
        if where == "before":
            vjp()
        res["cot"] = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy()
        if where == "between":
            vjp()
        res["x0"], res["goal"] = [a.cpu().numpy() for a in eng.bilevel_grad_inputs(B, lx)]
        res["dyn"] = eng.bilevel_grad_dynamics(B, lx).cpu().numpy()
        if where == "between":
            vjp()
        res["cot2"] = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy()
        res["state"] = ig._state(eng, B)
        return res

    plain = chain(None)
    first = vjp()
    for where in ("between", "before"):
        mixed = chain(where)
        for key in ("cot", "x0", "goal", "dyn", "cot2"):
            np.testing.assert_array_equal(mixed[key], plain[key], err_msg=f"{key} ({where})")
        for key in plain["state"]:
            np.testing.assert_array_equal(mixed["state"][key], plain["state"][key], err_msg=f"{key} ({where})")
    after = vjp()
    for key in ("params", "history"):
        np.testing.assert_array_equal(after[key], first[key], err_msg=key)


def test_refusals():
    n, m, T, B, hist = 5, 2, 4, 4, 2
    eng = Engine(n, m, T, [n + m, 8, n], [n, 1], max_batch=B)
    d = eng.to_dev
    rng = np.random.default_rng(0)
    history = d(rng.standard_normal((B, hist + 1, n)).astype(np.float32))
    g_goal = d(rng.standard_normal((B, T + 1, n)).astype(np.float32))
    g_U = d(rng.standard_normal((B, T, m)).astype(np.float32))
    good = make_expert_shape(16, [16, 16, n], [16, 16, m])
    gflat = d(P.pack_expert(orc.make_expert(rng, n, m, lstm_features=16, num_layers=2, num_hidden_units=16))[0])

    def ok():
        out = eng.expert_vjp(history, gflat, good, g_goal, g_U)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["params"]).all()) and bool(torch.isfinite(out["history"]).all())
        return out

    want = ok()
    bad = [make_expert_shape(129, [129, 16, n], [129, 16, m]),       # F > 128
           make_expert_shape(0, [513, 16, n], [513, 16, m]),         # MLP first width > 512
           make_expert_shape(16, [16, 1025, n], [16, 1025, m])]      # head width > 1024
    for es in bad:
        zeros = torch.zeros(eng.lib.gmpc_expert_param_count(n, es), device=eng.device)
        with pytest.raises(GmpcError):
            eng.expert_vjp(history, zeros, es, g_goal, g_U)
        ok()
    with pytest.raises(GmpcError, match="hist=0"):
        eng.expert_vjp(history[:, :1].contiguous(), gflat, good, g_goal, g_U)
    ok()
    with pytest.raises(GmpcError, match="outside"):                   # B > max_batch
        eng.expert_vjp(torch.cat([history, history]), gflat, good, torch.cat([g_goal, g_goal]),
                       torch.cat([g_U, g_U]))
    ok()
    with pytest.raises(GmpcError, match="both null"):
        eng.expert_vjp(history, gflat, good, None, None)
    ok()
    with pytest.raises(GmpcError, match="every output is null"):
        eng.expert_vjp(history, gflat, good, g_goal, g_U, want_params=False, want_history=False)
    again = ok()
    for key in ("params", "history"):
        assert torch.equal(again[key], want[key])
    eng.close()


# ---- the torch layer ---------------------------------------------------------------------------------------------
def _layer_setup(maxiter=2):
    config, policy, params, data = mirror._build(l2_policy.L2MPC)
    policy.trajax_ilqr_kwargs["maxiter"] = maxiter
    idx = np.arange(8)
    dparams, x0, goal, init_U = ig._layer_inputs(policy, params, data, idx)
    eng = policy.engine_for(len(idx), dparams)
    rng = np.random.default_rng(13)
    ex = orc.make_expert(rng, eng.nx, eng.m, lstm_features=16, num_layers=2, num_hidden_units=24)
    W, b = ex["head_x"][-1]
    ex["head_x"][-1] = ((0.3 * W).astype(np.float32), (0.3 * b).astype(np.float32))
    flat, F, dx, du = P.pack_expert(ex)
    history = eng.to_dev(np.asarray(data["hist"][idx], np.float32))
    des = eng.to_dev(np.asarray(data["Y"][idx], np.float32))
    return policy, dparams, x0, goal, eng.to_dev(flat), make_expert_shape(F, dx, du), history, des


def test_layer_gradients_are_the_entry_point():
    policy, dparams, _, _, flat, es, history, _ = _layer_setup()
    eng = policy._engine
    flat.requires_grad_(True)
    hist_r = history.clone().requires_grad_(True)
    goal, init_U = dl.expert_layer(policy, flat, es, hist_r)
    want_goal, want_U = eng.expert_rollout(history, flat.detach(), es)
    assert torch.equal(goal, want_goal) and torch.equal(init_U, want_U)
    gen = torch.Generator(device="cpu").manual_seed(1)
    wg = torch.randn(goal.shape, generator=gen).to(goal.device)
    wu = torch.randn(init_U.shape, generator=gen).to(goal.device)
    ((goal * wg).sum() + (init_U * wu).sum()).backward()
    ref = eng.expert_vjp(history, flat.detach(), es, wg, wu)
    assert torch.equal(flat.grad, ref["params"]) and torch.equal(hist_r.grad, ref["history"])
    assert float(ref["params"].abs().max()) > 0
    # one cotangent only
    flat.grad = None
    goal, init_U = dl.expert_layer(policy, flat, es, history)
    (init_U * wu).sum().backward()
    assert torch.equal(flat.grad, eng.expert_vjp(history, flat.detach(), es, None, wu, want_history=False)["params"])


def test_expert_layer_then_ilqr_layer_backpropagates():
    """The goal generator trained through the controller: dL/dgoal of ilqr_layer goes into the expert's VJP (init_U
    gets no cotangent: the NULL-g_U path), and the held solution survives the expert layer's forward and backward."""
    policy, dparams, x0, _, flat, es, history, des = _layer_setup()
    flat.requires_grad_(True)
    loss_of = lambda X: ((X[..., : des.shape[-1]] - des) ** 2).mean(1).sum()  # noqa: E731
    goal, init_U = dl.expert_layer(policy, flat, es, history)
    X, U = dl.ilqr_layer(policy, dparams, x0, goal, init_U)
    dl.expert_layer(policy, flat, es, history)        # another forward on the engine that holds the solution
    loss_of(X).backward()                             # (raises "another iLQR solve" if the solution was dropped)
    got = flat.grad.clone()
    goal_leaf = goal.detach().clone().requires_grad_(True)
    X2, _ = dl.ilqr_layer(policy, dparams, x0, goal_leaf, init_U.detach())
    loss_of(X2).backward()
    assert torch.equal(X2, X)
    ref = policy._engine.expert_vjp(history, flat.detach(), es, goal_leaf.grad.contiguous(), None, want_history=False)
    assert torch.equal(got, ref["params"])
    assert float(got.abs().max()) > 0 and bool(torch.isfinite(got).all())


def test_expert_layer_then_rollout_layer_backpropagates():
    """The action head trained through the learned dynamics: dL/dU of rollout_layer goes into the expert's VJP."""
    policy, dparams, x0, goal_data, flat, es, history, _ = _layer_setup()
    flat.requires_grad_(True)
    loss_of = lambda X, costs: costs.sum() + 0.1 * (X * X).sum()  # noqa: E731
    _, init_U = dl.expert_layer(policy, flat, es, history)
    X, costs = dl.rollout_layer(policy, dparams, x0, init_U, goal_data)
    loss_of(X, costs).backward()
    got = flat.grad.clone()
    U_leaf = init_U.detach().clone().requires_grad_(True)
    X2, costs2 = dl.rollout_layer(policy, dparams, x0, U_leaf, goal_data)
    loss_of(X2, costs2).backward()
    ref = policy._engine.expert_vjp(history, flat.detach(), es, None, U_leaf.grad.contiguous(), want_history=False)
    assert torch.equal(got, ref["params"])
    assert float(got.abs().max()) > 0 and bool(torch.isfinite(got).all())
