"""gmpc_critic_vjp (the VJP of the critic's scores for a caller's output delta) on the GPU: every dispatch cell of
critic_forward_backward (tests/critic_cases.py) against the fp32 and fp64 torch reference (tests/critic_vjp_ref.py)
under test_critic_sweep's protocol; bits against the two hard-wired entry points, under linear scaling, reuse and the
side stream; the ordering contract (it drops no held solution and no bilevel tail); the refusals; critic_layer alone and
behind ilqr_layer / expert_layer; GAN_MPC's critic and generator steps and one CriticTrainer update."""

import os

import numpy as np
import pytest
import torch

import critic_cases as cc
import critic_vjp_ref as V
import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_bilevel_cotangent as cot
import test_gpu_critic_sweep as sweep
import test_gpu_input_grads as ig
from gan_mpc_amd import optim, params as P, utils
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.engine import make_expert_shape
from gan_mpc_amd.expert.expert_model import TableExpert
from gan_mpc_amd.gan import critic_trainer, gan_policy, js_policy
from gan_mpc_amd.policy import differentiable as dl

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(__file__), "golden", "mirror_config.yaml")


def _vjp(eng, crit, xseq, g, **kw):
    out = eng.critic_vjp(eng.to_dev(xseq), crit, eng.to_dev(g), **kw)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b, what):
    assert np.isfinite(a).all(), f"{what}: not finite"
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (
        f"{what}: differs in {int((a != b).sum())} of {a.size} entries")


# ---- 1. parity on every dispatch cell ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_critic_vjp_sweep(case):
    n, F, T, Bc, head, _ = case
    pb, xseq, _, _ = cc.make_case(case)
    cr64 = orc.cast_problem(pb, np.float64)["critic"]
    g = V.case_g(case)
    gu.set_config(f"critic vjp {cc.case_id(case)}")
    x64, g64 = xseq.astype(np.float64), g.astype(np.float64)
    assert np.abs(orc.critic_forward(cr64, x64)).max() < cc.SCORE_MAX
    assert not cc.head_kinks(cr64, x64).any(), "a head row sits at a relu kink"
    eng = gu.engine_for(pb)
    assert eng.max_batch == (Bc + 1) // 2
    try:
        out = _vjp(eng, eng.to_dev(gu.critic_flat(pb)), xseq, g)       # one call, all three outputs
    finally:
        eng.close()
    dims = (F,) + tuple(head) + (1,)
    s32, p32, d32 = V.vjp(gu.critic_flat(pb), n, F, dims, xseq, g, dtype=np.float32)
    s64, p64, d64 = V.vjp(V.flat_of(cr64), n, F, dims, x64, g64)
    gu.assert_parity("score", out["score"], s32, s64)
    gu.assert_parity("critic vjp grad", out["params"] / Bc, p32 / Bc, p64 / Bc)
    sens = V.sensitivity(case, g)
    blocks = [gu.split_critic_flat(v, n, F, dims) for v in (out["params"] / Bc, p32 / Bc, p64 / Bc)]
    for (name, a), (_, b32), (_, b64) in zip(*blocks):
        gu.assert_parity(f"critic vjp grad {name}", a, b32, b64, el_tol=max(1e-3, 4 * sens[name]))
    dx = out["dx"]
    gu.assert_parity("g dscore/dx", dx, d32, d64, el_tol=max(1e-3, 4 * sens["dx"]))
    gu.assert_parity("g dscore/dx t=0", dx[:, 0], d32[:, 0], d64[:, 0], el_tol=max(1e-3, 4 * sens["dx t=0"]))
    gu.assert_parity("g dscore/dx t=T1-1", dx[:, -1], d32[:, -1], d64[:, -1],
                     el_tol=max(1e-3, 4 * sens["dx t=T1-1"]))


# ---- 2. bits against the existing entry points ---------------------------------------------------------------------
ROUTE_BC = [(r, 7) for r in sweep.ROUTE_CASES] + [("gen2", 3), ("gen2", 9)]


@pytest.mark.parametrize("route,Bc", ROUTE_BC, ids=[f"{r}-Bc{b}" for r, b in ROUTE_BC])
def test_bits_against_the_existing_entry_points(route, Bc):
    n, F, T, head = sweep.ROUTE_CASES[route]
    assert cc.critic_route(n, F)[0] == route
    pb = sweep._small_problem(n, F, T, (Bc + 1) // 2, head, seed=60)
    gu.set_config(f"critic vjp bits {route} n={n} F={F} T={T} Bc={Bc}")
    rng = np.random.default_rng(61)
    x = rng.standard_normal((Bc, T + 1, n)).astype(np.float32)
    g = rng.standard_normal(Bc).astype(np.float32)
    g[1] = 0.0
    eng = gu.engine_for(pb)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        score, dx1 = [a.cpu().numpy() for a in eng.critic_score_vjp(eng.to_dev(x), crit)]
        ones = _vjp(eng, crit, x, np.ones(Bc, np.float32))
        both = _vjp(eng, crit, x, g)
        dx_only = _vjp(eng, crit, x, g, want_params=False)
        par_only = _vjp(eng, crit, x, g, want_dx=False)
        twice = _vjp(eng, crit, x, 2 * g)
        again = _vjp(eng, crit, x, g)
    finally:
        eng.close()
    _same_bits(ones["score"], score, "score against critic_score_vjp")
    _same_bits(ones["dx"], dx1, "dx at g = 1 against critic_score_vjp")
    assert dx_only["params"] is None and par_only["dx"] is None
    _same_bits(both["dx"], dx_only["dx"], "dx: both outputs against dx only")
    _same_bits(both["params"], par_only["params"], "params: both outputs against params only")
    for key in ("score", "dx", "params"):
        _same_bits(again[key], both[key], f"{key}: two identical calls")
    _same_bits(twice["dx"], 2 * both["dx"], "dx at 2 g")
    _same_bits(twice["params"], 2 * both["params"], "params at 2 g")
    assert np.abs(both["dx"][1]).max() == 0 and np.abs(both["dx"][0]).max() > 0
    assert np.abs(both["params"]).max() > 0


# ---- 3. reuse and scheduling ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(sweep.ROUTE_CASES))
def test_engine_reuse_with_a_smaller_batch(route):
    n, F, T, head = sweep.ROUTE_CASES[route]
    M = 9
    pb = sweep._small_problem(n, F, T, M, head, seed=70)
    gu.set_config(f"critic vjp reuse {route} n={n} F={F} T={T} max_batch={M}")
    rng = np.random.default_rng(72)
    data = {Bc: (rng.standard_normal((Bc, T + 1, n)).astype(np.float32), rng.standard_normal(Bc).astype(np.float32))
            for Bc in (2 * M, 3)}
    eng = gu.engine_for(pb, max_batch=M)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        _vjp(eng, crit, *data[2 * M])
        reused = _vjp(eng, crit, *data[3])
    finally:
        eng.close()
    fresh = gu.engine_for(pb, max_batch=M)
    try:
        ref = _vjp(fresh, fresh.to_dev(gu.critic_flat(pb)), *data[3])
    finally:
        fresh.close()
    for key in ("score", "dx", "params"):
        _same_bits(reused[key], ref[key], f"{key}: Bc=3 after Bc={2 * M}")


@pytest.mark.parametrize("n,Bc", [(3, 4), (3, 9), (32, 4), (32, 9)])
def test_side_stream_schedule_changes_no_bit(n, Bc, monkeypatch):
    T, head = 5, (129, 65)
    assert cc.critic_route(n, 64)[0] == "gen2"
    pb = sweep._small_problem(n, 64, T, (Bc + 1) // 2, head, seed=80 + n)
    gu.set_config(f"critic vjp side stream n={n} Bc={Bc}")
    rng = np.random.default_rng(82)
    x, g = rng.standard_normal((Bc, T + 1, n)).astype(np.float32), rng.standard_normal(Bc).astype(np.float32)
    eng = gu.engine_for(pb)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        monkeypatch.delenv("GMPC_CRITIC_SIDE", raising=False)
        side = _vjp(eng, crit, x, g)
        monkeypatch.setenv("GMPC_CRITIC_SIDE", "0")
        one = _vjp(eng, crit, x, g)
    finally:
        eng.close()
    for key in ("score", "dx", "params"):
        _same_bits(one[key], side[key], f"{key}: GMPC_CRITIC_SIDE=0 against the side stream")


# ---- 4. ordering contract ------------------------------------------------------------------------------------------
def test_read_only_between_solve_and_bilevel_calls():
    from gan_mpc_amd.policy import optimizers as opt
    pb, _, eng, out, B = cot._solved("tiny-ragged", critic=True)
    _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
    crit = eng.to_dev(gu.critic_flat(pb))
    xs = out["X"][..., :eng.nx].contiguous()
    g = eng.to_dev(np.random.default_rng(5).standard_normal(B).astype(np.float32))

    def vjp():
        return {k: v.cpu().numpy() for k, v in eng.critic_vjp(xs, crit, g).items()}

    def chain(where):
        res = {}
        if where == "before":
            vjp()
        res["cot"] = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy()
        if where == "between":
            vjp()
        res["x0"], res["goal"] = [a.cpu().numpy() for a in eng.bilevel_grad_inputs(B, lx)]
        if where == "between":
            vjp()
        res["loss"], res["js"] = [a.cpu().numpy() for a in eng.bilevel_grad(B, 1, critic=crit, sign=-1.0)]
        res["state"] = ig._state(eng, B)
        return res

    try:
        plain = chain(None)
        first = vjp()
        for where in ("between", "before"):
            mixed = chain(where)
            for key in ("cot", "x0", "goal", "loss", "js"):
                np.testing.assert_array_equal(mixed[key], plain[key], err_msg=f"{key} ({where})")
            for key in plain["state"]:
                np.testing.assert_array_equal(mixed["state"][key], plain["state"][key], err_msg=f"{key} ({where})")
        after = vjp()
    finally:
        eng.close()
    for key in ("score", "dx", "params"):
        np.testing.assert_array_equal(after[key], first[key], err_msg=key)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def test_refusals():
    n, F, T, M = 5, 64, 3, 4
    pb = sweep._small_problem(n, F, T, M, (17,), seed=50)
    eng = gu.engine_for(pb)
    d = eng.to_dev
    rng = np.random.default_rng(51)
    Bc = 2 * M
    x = d(rng.standard_normal((Bc, T + 1, n)).astype(np.float32))
    g = d(rng.standard_normal(Bc).astype(np.float32))
    crit = d(gu.critic_flat(pb))
    score, dx, gs = eng.new(Bc), eng.new(Bc, T + 1, n), eng.new(eng.critic_count)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def raw(Bc_, x_, crit_, g_, dx_, gs_, ctx=None):
        rc = eng.lib.gmpc_critic_vjp(ctx or eng.ctx, Bc_, ptr(x_), ptr(crit_), ptr(g_), ptr(score), ptr(dx_), ptr(gs_),
                                     None)
        assert rc == -1, rc                   # GMPC_EINVAL
        return eng.lib.gmpc_last_error().decode()

    def ok():
        out = eng.critic_vjp(x, crit, g)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in out.values())
        return out

    want = ok()
    assert "xseq is null" in raw(Bc, None, crit, g, dx, gs)
    assert "critic is null" in raw(Bc, x, None, g, dx, gs)
    assert "g_score is null" in raw(Bc, x, crit, None, dx, gs)
    assert "grad_xseq and grad_critic_sum are both null" in raw(Bc, x, crit, g, None, None)
    for bad in (0, Bc + 1):
        msg = raw(bad, x, crit, g, dx, gs)
        assert f"Bc={bad} outside" in msg and f"2*max_batch={Bc}" in msg
    with pytest.raises(GmpcError, match="both null"):
        eng.critic_vjp(x, crit, g, want_dx=False, want_params=False)
    with pytest.raises(GmpcError, match="g_score must be"):
        eng.critic_vjp(x, crit, g[:-1].contiguous())
    with pytest.raises(GmpcError, match="xseq must be"):
        eng.critic_vjp(x[:, :-1].contiguous(), crit, g)
    again = ok()
    for key in want:
        assert torch.equal(again[key], want[key]), key
    bare = gu.engine_for(pb, critic=False)
    try:
        assert "without a critic" in raw(Bc, x, crit, g, dx, gs, ctx=bare.ctx)
    finally:
        bare.close()
        eng.close()


# ---- 6. the torch layer --------------------------------------------------------------------------------------------
def _build(policy_cls, N=3, M=1, T=5, F=64, hidden=17, ndata=10, seed=3, **policy_kw):
    """test_gpu_mirror._build with the critic's and the problem's shape as arguments."""
    config = utils.get_config(CFG)
    config.mpc.horizon = T
    config.mpc.model.critic.lstm.lstm_features = F
    config.mpc.model.critic.lstm.num_hidden_units = hidden
    cost, _ = utils.get_cost_model(config)
    dynamics, _ = utils.get_dynamics_model(config, N)
    critic, _ = utils.get_critic_model(config)
    rng = np.random.default_rng(seed)
    hist = rng.standard_normal((ndata, config.mpc.history + 1, N)).astype(np.float32)
    goal = rng.standard_normal((ndata, T + 1, N)).astype(np.float32)
    goal[:, 0] = hist[:, -1]
    init_U = np.tanh(rng.standard_normal((ndata, T, M))).astype(np.float32)
    Y = rng.standard_normal((ndata, T + 1, N)).astype(np.float32)
    policy = policy_cls(config=config, cost_model=cost, dynamics_model=dynamics, expert_model=TableExpert(goal, init_U),
                        critic_model=critic, **policy_kw)
    mpc_weights = tuple(config.mpc.model.cost.weights.to_dict().values())
    params = policy.init(mpc_weights, (config.seed, N), (config.seed, M), (True,), (config.seed, N))
    dc = config.mpc.model.dynamics.mlp
    params["dynamics_params"]["params"][f"Dense_{dc.num_layers - 1}"]["kernel"] *= 0.1
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    return config, policy, params, dict(hist=hist, goal=goal, init_U=init_U, Y=Y)


def test_critic_layer_behind_ilqr_layer_gives_the_entry_points_bits():
    """ilqr_layer -> critic_layer -> (-score).sum().backward(): the generator step as one autograd graph."""
    B = 5
    config, policy, params, data = _build(js_policy.JS_MPC)
    dparams, x0, goal, init_U = ig._layer_inputs(policy, params, data, np.arange(B))
    dparams.flat.requires_grad_(True)
    X, U = dl.ilqr_layer(policy, dparams, x0, goal, init_U)
    score = dl.critic_layer(policy, dparams, X)
    (-score).sum().backward()
    eng = policy._engine
    assert (eng.n, eng.m, eng.T, eng.shape.lstm_features) == (3, 1, 5, 64)
    grad = dparams.flat.grad.clone()
    crit = dparams.view("critic_params").detach()
    _, want_theta = eng.bilevel_grad(B, 1, critic=crit, sign=-1.0)
    want_crit = eng.critic_vjp(X.detach(), crit, -torch.ones(B, device=X.device), want_dx=False)["params"]
    lo, cnt = dparams.range_of(("mpc_weights", "cost_params"))
    assert torch.equal(grad[lo:lo + cnt], want_theta) and float(want_theta.abs().max()) > 0
    clo, ccnt = dparams.range_of(("critic_params",))
    assert torch.equal(grad[clo:clo + ccnt], want_crit) and float(want_crit.abs().max()) > 0
    rest = torch.ones_like(grad, dtype=torch.bool)
    rest[lo:lo + cnt] = False
    rest[clo:clo + ccnt] = False
    assert float(grad[rest].abs().max()) == 0
    assert torch.equal(score.detach(), eng.critic_score_vjp(X.detach(), crit, want_dx=False)[0])


def test_expert_layer_ilqr_layer_critic_layer_backpropagate_in_one_call():
    B = 5
    config, policy, params, data = _build(js_policy.JS_MPC)
    dparams, x0, _, _ = ig._layer_inputs(policy, params, data, np.arange(B))
    eng = policy._engine
    ex = orc.make_expert(np.random.default_rng(13), eng.nx, eng.m, lstm_features=16, num_layers=2, num_hidden_units=24)
    W, b = ex["head_x"][-1]
    ex["head_x"][-1] = ((0.3 * W).astype(np.float32), (0.3 * b).astype(np.float32))
    flat, Fe, dx, du = P.pack_expert(ex)
    eflat = eng.to_dev(flat).requires_grad_(True)
    history = eng.to_dev(np.asarray(data["hist"][:B], np.float32))
    dparams.flat.requires_grad_(True)
    goal, init_U = dl.expert_layer(policy, eflat, make_expert_shape(Fe, dx, du), history)
    X, _ = dl.ilqr_layer(policy, dparams, x0, goal, init_U)
    torch.relu(1.0 - dl.critic_layer(policy, dparams, X)).sum().backward()
    clo, ccnt = dparams.range_of(("critic_params",))
    for name, gr in (("expert", eflat.grad), ("critic", dparams.flat.grad[clo:clo + ccnt])):
        assert bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, name


def test_critic_layer_refuses_instead_of_rebuilding_the_engine():
    config, policy, params, data = _build(js_policy.JS_MPC)
    dparams = policy.to_device_params(params)
    xs = torch.zeros(4, 6, 3, device=policy.device())
    with pytest.raises(GmpcError, match="bind its parameters first"):
        dl.critic_layer(policy, dparams, xs)
    eng = policy.bind(dparams, 2)
    big = torch.zeros(2 * eng.max_batch + 1, 6, 3, device=policy.device())
    with pytest.raises(GmpcError, match=f"{2 * eng.max_batch + 1}.*{2 * eng.max_batch}"):
        dl.critic_layer(policy, dparams, big)
    assert policy._engine is eng and eng.ctx is not None
    xs.requires_grad_(True)
    score = dl.critic_layer(policy, dparams, xs)
    eng.close()
    with pytest.raises(RuntimeError, match="has been closed"):
        score.sum().backward()


# ---- 7. GAN_MPC ----------------------------------------------------------------------------------------------------
def _critic_batch(policy, params, n, T, Bc, seed):
    rng = np.random.default_rng(seed)
    xs = rng.standard_normal((Bc, T + 1, n)).astype(np.float32)
    lab = np.where(rng.permutation(Bc) % 2 == 0, 1.0, -1.0).astype(np.float32)
    cr = P.critic_tree_to_dict(params["critic_params"])
    cr64 = orc.cast_problem(dict(c=cr), np.float64)["c"]
    assert np.abs(orc.critic_forward(cr64, xs.astype(np.float64))).max() < cc.SCORE_MAX
    assert not cc.head_kinks(cr64, xs.astype(np.float64)).any()
    return xs, lab, cr, cr64


@pytest.mark.parametrize("route", list(sweep.ROUTE_CASES))
def test_gan_mpc_js_critic_step_against_the_oracle(route):
    n, F, T, head = sweep.ROUTE_CASES[route]
    Bc = 7
    config, policy, params, _ = _build(gan_policy.GAN_MPC, N=n, T=T, F=F, hidden=head[0], ndata=2, objective="js")
    xs, lab, cr, cr64 = _critic_batch(policy, params, n, T, Bc, seed=40)
    gu.set_config(f"GAN_MPC js critic step {route}")
    loss, grads = policy.critic_loss_and_grad(xs, lab, params)
    assert cc.critic_route(policy._engine.nx, policy._engine.shape.lstm_features)[0] == route
    grads = grads.cpu().numpy()
    x64, lab64 = xs.astype(np.float64), lab.astype(np.float64)
    l32, g32 = orc.critic_loss_and_grad(cr, xs, lab)
    l64, g64 = orc.critic_loss_and_grad(cr64, x64, lab64)
    gu.assert_parity("critic loss", float(loss), l32, l64)
    p32, p64 = gu.pack_grads_critic(g32), gu.pack_grads_critic(g64)
    gu.assert_parity("critic grad", grads, p32, p64)
    dims = (F,) + tuple(head) + (1,)
    bce = lambda s: np.where(lab64 > 0, -(1 - orc.sigmoid(s)), orc.sigmoid(s))  # noqa: E731
    sens = V.sensitivity_at(V.flat_of(cr64), n, F, head, x64, bce, seed=41)
    for (name, a), (_, b32), (_, b64) in zip(*[gu.split_critic_flat(v, n, F, dims) for v in (grads, p32, p64)]):
        gu.assert_parity(f"critic grad {name}", a, b32, b64, el_tol=max(1e-3, 4 * sens[name]))


def test_gan_mpc_wgan_critic_step_is_critic_vjp():
    n, F, T, head = sweep.ROUTE_CASES["gen2"]
    Bc = 7
    config, policy, params, _ = _build(gan_policy.GAN_MPC, N=n, T=T, F=F, hidden=head[0], ndata=2, objective="wgan")
    xs, lab, cr, cr64 = _critic_batch(policy, params, n, T, Bc, seed=42)
    gu.set_config("GAN_MPC wgan critic step")
    dparams = policy.to_device_params(params)
    loss, grads = policy.critic_loss_and_grad(xs, lab, dparams)
    eng = policy._engine
    ref = eng.critic_vjp(eng.to_dev(xs), dparams.view("critic_params"), eng.to_dev(-lab))
    # the policy's mean is parallel.allreduce_finish's: the sums divided by the count held on the device (a true
    # division; torch turns a division by a Python scalar into a multiplication by its reciprocal)
    assert torch.equal(grads, ref["params"] / torch.full((), float(Bc), device=grads.device))
    dims = (F,) + tuple(head) + (1,)
    s32, p32, _ = V.vjp(V.flat_of(cr, np.float32), n, F, dims, xs, -lab / Bc, dtype=np.float32)
    s64, p64, _ = V.vjp(V.flat_of(cr64), n, F, dims, xs.astype(np.float64), -lab.astype(np.float64) / Bc)
    gu.assert_parity("wgan critic loss", float(loss), np.mean(-lab * s32), np.mean(-lab * s64))
    gu.assert_parity("wgan critic grad", grads.cpu().numpy(), p32, p64)


def test_gan_mpc_js_generator_step_is_js_mpcs():
    B = 5
    res = {}
    for cls, kw in ((js_policy.JS_MPC, {}), (gan_policy.GAN_MPC, dict(objective="js"))):
        config, policy, params, data = _build(cls, **kw)
        idx = np.arange(B)
        policy.expert_model.select(idx)
        loss, grads = policy.generator_loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
        policy.expert_model.select(idx)
        test_loss = policy.batch_loss(policy.to_device_params(params), data["hist"][idx], data["Y"][idx])
        xc, *_ = policy.get_optimal_values(params, data["hist"][idx])
        res[cls] = (float(loss), grads.cpu().numpy(), float(test_loss), xc.cpu().numpy(), params)
    (l_js, g_js, t_js, X_js, params), (l_gan, g_gan, t_gan, X_gan, _) = res[js_policy.JS_MPC], res[gan_policy.GAN_MPC]
    _same_bits(g_gan, g_js, "generator gradient: GAN_MPC(js) against JS_MPC")
    assert np.abs(g_js).max() > 0
    np.testing.assert_array_equal(X_gan, X_js)
    cr = P.critic_tree_to_dict(params["critic_params"])
    cr64 = orc.cast_problem(dict(c=cr), np.float64)["c"]
    want32 = orc.generator_loss(cr, X_js).mean()
    want64 = orc.generator_loss(cr64, X_js.astype(np.float64)).mean()
    gu.set_config("GAN_MPC js generator step")
    for name, got in (("JS_MPC loss", l_js), ("GAN_MPC loss", l_gan), ("JS_MPC test loss", t_js),
                      ("GAN_MPC test loss", t_gan)):
        gu.assert_parity(name, got, want32, want64)


def test_critic_trainer_update_with_a_gan_mpc():
    config, policy, params, data = _build(gan_policy.GAN_MPC, N=4, M=2, T=6, hidden=16, ndata=24, objective="hinge")
    opt = optim.get_optimizer(list(params.keys()), config.mpc.train.critic.no_grads, 1e-2)
    dparams = policy.to_device_params(params)
    before = dparams.view("critic_params").clone()
    other = dparams.flat[:dparams.offsets["critic_params"]].clone()
    ntr = 16
    ds = ((data["hist"][:ntr], data["Y"][:ntr]), (data["hist"][ntr:], data["Y"][ntr:]))
    new_params, _, tl, te, _ = critic_trainer.train((policy, opt), opt.init(dparams), dparams, ds, num_updates=1,
                                                    batch_size=8, key=1, id=0)
    assert len(tl) == 1 and len(te) == 1 and np.isfinite(tl).all() and np.isfinite(te).all()
    assert not torch.equal(before, new_params.view("critic_params"))
    assert torch.equal(other, new_params.flat[:new_params.offsets["critic_params"]])
