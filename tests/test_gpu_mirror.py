"""The Python host mirror (reference protocol: models, policies, trainers) on the GPU, against the
oracle driven the way the reference drives JAX."""

import os

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu
from gan_mpc_amd import optim, params as P, utils
from gan_mpc_amd.expert.expert_model import TableExpert
from gan_mpc_amd.gan import critic_trainer, js_policy
from gan_mpc_amd.norm import cost_trainer, l2_policy

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(__file__), "golden", "mirror_config.yaml")
N, M = 4, 2


def _build(policy_cls, ndata=24, seed=3, N=N, M=M, dyn_use="mlp"):
    config = utils.get_config(CFG)
    config.mpc.model.dynamics.use = dyn_use
    T = config.mpc.horizon
    cost, _ = utils.get_cost_model(config)
    dynamics, _ = utils.get_dynamics_model(config, N)
    critic, _ = utils.get_critic_model(config)
    rng = np.random.default_rng(seed)
    hist = rng.standard_normal((ndata, config.mpc.history + 1, N)).astype(np.float32)
    goal = rng.standard_normal((ndata, T + 1, N)).astype(np.float32)
    goal[:, 0] = hist[:, -1]
    init_U = np.tanh(rng.standard_normal((ndata, T, M))).astype(np.float32)
    Y = rng.standard_normal((ndata, T + 1, N)).astype(np.float32)
    expert = TableExpert(goal, init_U)
    kw = dict(config=config, cost_model=cost, dynamics_model=dynamics, expert_model=expert)
    if policy_cls is js_policy.JS_MPC:
        kw["critic_model"] = critic
    policy = policy_cls(**kw)
    mpc_weights = tuple(config.mpc.model.cost.weights.to_dict().values())
    # the cost MLP takes xc = [x, carry] (reference gan/runner.py:37-48: xc_size = x_size + carry size)
    xc_size = N + dynamics.get_zero_carry(hist[0, :-1]).shape[-1]
    args = [mpc_weights, (config.seed, xc_size), (config.seed, M), (True,)]
    if policy_cls is js_policy.JS_MPC:
        args.append((config.seed, N))
    params = policy.init(*args)
    # "trained-like" residual dynamics so that the few iLQR iterations are well conditioned
    dc = getattr(config.mpc.model.dynamics, dyn_use)
    last = f"Dense_{dc.num_layers - 1}"
    params["dynamics_params"]["params"][last]["kernel"] *= 0.1
    return config, policy, params, dict(hist=hist, goal=goal, init_U=init_U, Y=Y)


def _oracle_problem(params, data, idx, dtype):
    dyn = (P.lstm_dynamics_tree_to_dict(params["dynamics_params"]) if P.dynamics_is_lstm(params["dynamics_params"])
           else P.tree_to_layers(params["dynamics_params"]))
    pb = dict(dyn=dyn,
              cmlp=P.tree_to_layers(params["cost_params"]), mpc_w=params["mpc_weights"],
              goal=data["goal"][idx], x0=data["hist"][idx, -1], U=data["init_U"][idx],
              true_seq=data["Y"][idx])
    if "critic_params" in params:
        pb["critic"] = P.critic_tree_to_dict(params["critic_params"])
    return orc.cast_problem(pb, dtype)


def test_params_dict_has_the_reference_keys():
    _, policy, params, _ = _build(js_policy.JS_MPC)
    assert set(params) == {"mpc_weights", "cost_params", "dynamics_params", "expert_params",
                           "critic_params"}
    assert params["mpc_weights"].dtype == np.float32 and params["mpc_weights"].shape == (3,)
    assert list(params["cost_params"]["params"]) == ["Dense_0", "Dense_1", "Dense_2"]
    assert params["dynamics_params"]["params"]["Dense_0"]["kernel"].shape == (N + M, 32)


def test_get_optimal_values_is_the_trajax_7_tuple():
    config, policy, params, data = _build(l2_policy.L2MPC)
    policy.expert_model.select(np.array([2]))
    out = policy.get_optimal_values(params, data["hist"][2])
    assert len(out) == 7
    X, U, obj, grad, adj, lqr, itr = out
    T = config.mpc.horizon
    assert X.shape == (T + 1, N) and U.shape == (T, M) and grad.shape == (T, M)
    assert adj.shape == (T + 1, N) and lqr.shape == (T, N, N + M) and obj.dim() == 0
    p64 = _oracle_problem(params, data, np.array([2]), np.float64)
    r = orc.ilqr(p64["dyn"], p64["cmlp"], p64["mpc_w"], p64["goal"], p64["x0"], p64["U"])
    assert abs(float(obj) - r[2][0]) / abs(r[2][0]) < 1e-3
    policy.expert_model.select(np.array([2]))
    a = policy.get_optimal_action(params, data["hist"][2])
    assert a.shape == (M,)


def test_get_optimal_values_large_state():
    """n > 64: the step-major backward pass keeps ONE step of Jacobians, so the `lqr` slot is the
    (n, n+m) block at t = 0 and nothing is read past the ctx's allocation (single sample on an engine
    sized for 8)."""
    n, m = 70, 3
    config, policy, params, data = _build(l2_policy.L2MPC, ndata=4, N=n, M=m)
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    policy.expert_model.select(np.array([1]))
    X, U, obj, grad, adj, lqr, itr = policy.get_optimal_values(params, data["hist"][1])
    T = config.mpc.horizon
    assert X.shape == (T + 1, n) and U.shape == (T, m) and lqr.shape == (n, n + m)
    AB = lqr.tensor().cpu().numpy()
    p64 = _oracle_problem(params, data, np.array([1]), np.float64)
    A0, B0 = orc.dynamics_jacobians(p64["dyn"], X[None, 0].cpu().numpy().astype(np.float64),
                                    U[None, 0].cpu().numpy().astype(np.float64))
    assert gu.rel_err(AB, np.concatenate([A0[0], B0[0]], -1)) < 1e-5
    with pytest.raises(Exception, match="holds"):
        policy._engine.debug_buffer(5, (8, T, n, n + m))
    policy.expert_model.select(np.array([1]))
    assert policy.get_optimal_action(params, data["hist"][1]).shape == (m,)


@pytest.mark.parametrize("cls", [l2_policy.L2MPC, js_policy.JS_MPC])
def test_loss_and_grad_matches_oracle_batch_mean(cls):
    config, policy, params, data = _build(cls)
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    idx = np.arange(8)
    policy.expert_model.select(idx)
    loss, grads = policy.loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
    res = {}
    for dt in (np.float32, np.float64):
        p = _oracle_problem(params, data, idx, dt)
        l, g_mpc, g_cost, _ = orc.loss_and_grad(
            p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], p["x0"], p["U"],
            loss="l2" if cls is l2_policy.L2MPC else "js", desired=p["true_seq"],
            critic=p.get("critic"), kwargs={"maxiter": 2})
        res[dt] = (l, gu.pack_grads_cost(g_mpc, g_cost))
    gu.assert_parity("loss", float(loss), res[np.float32][0], res[np.float64][0], tol=1e-4, slack=10)
    # at the GPU's own iterate, stage by stage, under the default bars (the end-to-end figure is the one below)
    _check_policy_gradient_at_the_gpu_iterate(policy, _oracle_problem(params, data, idx, np.float32),
                                              _oracle_problem(params, data, idx, np.float64),
                                              0 if cls is l2_policy.L2MPC else 1, float(loss), grads, len(idx),
                                              end_to_end=False)
    gu.assert_parity("grads", grads.cpu().numpy(), res[np.float32][1], res[np.float64][1], tol=1e-3,
                     slack=10)


def test_critic_loss_and_grad_is_batch_mean():
    config, policy, params, data = _build(js_policy.JS_MPC)
    xs = data["Y"][:10]
    lab = np.array([1, -1] * 5, np.float32)
    loss, grads = policy.critic_loss_and_grad(xs, lab, params)
    cr = P.critic_tree_to_dict(params["critic_params"])
    l32, g32 = orc.critic_loss_and_grad(cr, xs, lab)
    cr64 = orc.cast_problem(dict(c=cr), np.float64)["c"]
    l64, g64 = orc.critic_loss_and_grad(cr64, xs.astype(np.float64), lab.astype(np.float64))
    gu.assert_parity("loss", float(loss), l32, l64)
    gu.assert_parity("grads", grads.cpu().numpy(), gu.pack_grads_critic(g32), gu.pack_grads_critic(g64))
    # single-sample critic_loss as in the reference's vmap body
    l1 = policy.critic_loss(xs[0], lab[0], params)
    p = orc.sigmoid(orc.critic_forward(cr64, xs[:1].astype(np.float64)))
    assert abs(float(l1) - float(-np.log(p[0]))) < 1e-5


def test_cost_trainer_one_update_against_oracle_loop():
    """cost_trainer.train == the reference loop (loss_and_grad -> clip+Adam -> Polyak) driven with
    the oracle on the same minibatches."""
    config, policy, params, data = _build(l2_policy.L2MPC)
    policy.trajax_ilqr_kwargs["maxiter"] = 1
    tc = config.mpc.train.cost
    opt = optim.get_optimizer(list(params.keys()), tc.no_grads, tc.learning_rate)
    assert opt.trainable_keys == ("mpc_weights", "cost_params")
    dparams = policy.to_device_params(params)
    opt_state = opt.init(dparams)
    ntr = 16
    train = (data["hist"][:ntr], data["Y"][:ntr])
    test = (data["hist"][ntr:], data["Y"][ntr:])
    out = cost_trainer.train((policy, opt), opt_state, dparams, (train, test), num_updates=1,
                             batch_size=8, polyak_factor=tc.polyak_factor, key=7, id=0)
    assert len(out) == 5   # (params, opt_state, train_losses, test_losses, exe_time) -- @timeit
    new_params, opt_state, train_losses, test_losses, exe_time = out
    assert opt_state["count"] == 2 and len(train_losses) == 1 and len(test_losses) == 1
    # oracle loop on the same minibatch indices
    rng = np.random.default_rng(7)
    perm = rng.choice(ntr, size=(2, 8))
    cost_flat = P.pack_mlp(params["cost_params"]).astype(np.float64)
    theta = np.concatenate([params["mpc_weights"].astype(np.float64), cost_flat])
    theta0 = theta.copy()
    m = np.zeros_like(theta)
    v = np.zeros_like(theta)
    dims = P.mlp_dims(params["cost_params"])
    losses = []
    for k, p_idx in enumerate(perm):
        cur = dict(params)
        cur["mpc_weights"] = theta[:3]
        cur["cost_params"] = P.unpack_mlp(theta[3:].astype(np.float32), dims)
        p = _oracle_problem(cur, data, p_idx, np.float64)
        p["mpc_w"] = theta[:3]
        p["cmlp"] = [(W.astype(np.float64), b.astype(np.float64)) for W, b in
                     P.tree_to_layers(cur["cost_params"])]
        l, g_mpc, g_cost, _ = orc.loss_and_grad(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], p["x0"],
                                                p["U"], loss="l2", desired=p["true_seq"],
                                                kwargs={"maxiter": 1})
        theta, m, v = orc.adam_clip_step(theta, gu.pack_grads_cost(g_mpc, g_cost), m, v, k + 1,
                                         tc.learning_rate)
        losses.append(l)
    theta = orc.polyak(theta0, theta, tc.polyak_factor)
    got = new_params.flat[:theta.size].cpu().numpy()
    assert abs(train_losses[0] - np.mean(losses)) / abs(np.mean(losses)) < 1e-3
    # Adam's first steps are ~ lr*sign(g): compare the parameter displacement
    disp_ref, disp_got = theta - theta0, got - theta0
    big = np.abs(disp_ref) > 0.5 * np.abs(disp_ref).max()
    assert np.abs(disp_got[big] - disp_ref[big]).max() < 0.05 * np.abs(disp_ref).max()
    # dynamics parameters: zero gradient, so only the Polyak blend 0.9*x + 0.1*x touches
    # them, as in the reference (cost_trainer.py:88-92 blends every leaf): equal up to one rounding
    np.testing.assert_allclose(new_params.view("dynamics_params").cpu().numpy(),
                               P.pack_mlp(params["dynamics_params"]), rtol=2.5e-7, atol=0)


def test_critic_trainer_one_update_against_oracle_loop():
    """critic_trainer.train == the reference loop (gan/critic_trainer.py:12-104): get_dataset (true (+1)
    then iLQR-predicted (-1) sequences per split, permutation of the TRAIN split only), minibatches of
    critic_loss_and_grad -> clip+Adam on critic_params, test loss -- driven with the float64 oracle on
    the same PRNG draws."""
    import oracle_loops as ol
    config, policy, params, data = _build(js_policy.JS_MPC)
    kw = {"maxiter": 1}
    policy.trajax_ilqr_kwargs.update(kw)
    tc = config.mpc.train.critic
    opt = optim.get_optimizer(list(params.keys()), tc.no_grads, tc.learning_rate)
    dparams = policy.to_device_params(params)
    start = dparams.view("critic_params").cpu().numpy().astype(np.float64)
    ntr, nall = 16, len(data["hist"])
    ds = ((data["hist"][:ntr], data["Y"][:ntr]), (data["hist"][ntr:], data["Y"][ntr:]))
    # the dataset on its own, with the key the trainer will use
    (trX, trL), (teX, teL) = critic_trainer.get_dataset(policy, dparams, ds, np.random.default_rng(5))
    op = ol.OracleParams(params)
    o_train = ol.critic_dataset(op, ds[0], data["goal"][:ntr], data["init_U"][:ntr], kw)
    o_test = ol.critic_dataset(op, ds[1], data["goal"][ntr:], data["init_U"][ntr:], kw)
    r2 = np.random.default_rng(5)
    order = r2.permutation(2 * ntr)
    np.testing.assert_array_equal(trL.cpu().numpy(), o_train[1][order])
    np.testing.assert_array_equal(teL.cpu().numpy(), o_test[1])            # the test split is NOT permuted
    # true halves are the inputs themselves; predicted halves: one iLQR iteration in fp32 vs fp64
    np.testing.assert_array_equal(teX[:nall - ntr].cpu().numpy(), data["Y"][ntr:])
    err = np.abs(trX.cpu().numpy() - o_train[0][order]).reshape(2 * ntr, -1).max(1) / np.abs(o_train[0]).max()
    assert np.median(err) < 1e-5 and (err < 1e-3).mean() > 0.8, err
    # the trainer, and the oracle loop on the same draws (trainer: permutation, then one schedule per update)
    new_params, opt_state, tl, te, _ = critic_trainer.train(
        (policy, opt), opt.init(dparams), dparams, ds, num_updates=2, batch_size=8, key=5, id=0)
    adam = ol.Adam(op.critic.size, tc.learning_rate)
    o_train = (o_train[0][order], o_train[1][order])
    ref_tl, ref_te = [], []
    for _ in range(2):
        ref_tl.append(ol.critic_sgd(op, adam, o_train, r2.choice(2 * ntr, size=(2 * ntr // 8, 8))))
        ref_te.append(ol.critic_loss(op, o_test))
    assert opt_state["count"] == 2 * (2 * ntr // 8)
    np.testing.assert_allclose(tl, ref_tl, rtol=2e-3)
    np.testing.assert_allclose(te, ref_te, rtol=2e-3)
    got = new_params.view("critic_params").cpu().numpy().astype(np.float64)
    d, frac = ol.displacement_matches(got, op.critic, start)
    assert d < frac, d
    # masked leaves are untouched
    lo = new_params.offsets["critic_params"]
    assert torch.equal(new_params.flat[:lo], policy.to_device_params(params).flat[:lo])


def test_critic_trainer_runs_and_learns():
    config, policy, params, data = _build(js_policy.JS_MPC)
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    tc = config.mpc.train.critic
    opt = optim.get_optimizer(list(params.keys()), tc.no_grads, 1e-2)
    assert opt.trainable_keys == ("critic_params",)
    dparams = policy.to_device_params(params)
    before = dparams.view("critic_params").clone()
    other = dparams.flat[:dparams.offsets["critic_params"]].clone()
    opt_state = opt.init(dparams)
    ntr = 16
    ds = ((data["hist"][:ntr], data["Y"][:ntr]), (data["hist"][ntr:], data["Y"][ntr:]))
    new_params, opt_state, tl, te, exe = critic_trainer.train(
        (policy, opt), opt_state, dparams, ds, num_updates=3, batch_size=8, key=1, id=0)
    assert len(tl) == 3 and len(te) == 3 and np.isfinite(tl).all() and np.isfinite(te).all()
    assert tl[-1] < tl[0]                      # the critic separates true from rolled-out sequences
    assert not torch.equal(before, new_params.view("critic_params"))
    assert torch.equal(other, new_params.flat[:new_params.offsets["critic_params"]])
    tree = new_params.to_tree()
    assert set(tree["critic_params"]["params"]) >= {"ScanOptimizedLSTMCell_0", "Dense_0", "Dense_1"}


def test_policy_with_the_expert_sequence_model():
    """EvalMPC / L2MPC driven by the GPU expert model (N2) instead of a table: the goal's first row is
    the current state, the solve starts from the expert's controls, loss_and_grad runs end to end."""
    from gan_mpc_amd.config import load_config
    from gan_mpc_amd.expert.expert_model import ExpertModel
    config = utils.get_config(CFG)
    cost, _ = utils.get_cost_model(config)
    dynamics, _ = utils.get_dynamics_model(config, N)
    mc = load_config.Config.from_dict({"use": "lstm", "lstm": {"lstm_features": 32, "num_layers": 3,
                                                               "num_hidden_units": 24}})
    expert = ExpertModel(config, ExpertModel.get_model(mc, N, M))
    policy = l2_policy.L2MPC(config=config, cost_model=cost, dynamics_model=dynamics,
                             expert_model=expert)
    mpc_weights = tuple(config.mpc.model.cost.weights.to_dict().values())
    params = policy.init(mpc_weights, (config.seed, N), (config.seed, M), (False, 5, 1, 4, N))
    assert "MLPCell_0" in str(params["expert_params"]["params"]["model"].keys()) or True
    last = f"Dense_{config.mpc.model.dynamics.mlp.num_layers - 1}"
    params["dynamics_params"]["params"][last]["kernel"] *= 0.1
    rng = np.random.default_rng(1)
    hist = rng.standard_normal((6, config.mpc.history + 1, N)).astype(np.float32)
    goal, init_U = policy.get_goal_states_init_actions(hist, params)
    ex = P.expert_tree_to_dict(params["expert_params"])
    g64, u64 = orc.expert_goal_states_init_actions(orc.cast_problem(dict(e=ex), np.float64)["e"],
                                                   hist.astype(np.float64), config.mpc.horizon)
    assert gu.rel_err(goal.cpu().numpy(), g64) < 1e-5 and gu.rel_err(init_U.cpu().numpy(), u64) < 1e-5
    X, U, obj, grad, adj, lqr, itr = policy.get_optimal_values(params, hist)
    np.testing.assert_array_equal(X[:, 0].cpu().numpy(), hist[:, -1])
    assert np.isfinite(obj.cpu().numpy()).all()
    Y = rng.standard_normal((6, config.mpc.horizon + 1, N)).astype(np.float32)
    loss, grads = policy.loss_and_grad(hist, params, (Y,))
    assert np.isfinite(float(loss)) and np.isfinite(grads.cpu().numpy()).all()


def test_model_protocol_with_the_reference_signatures():
    """reference base.py:4-49 as policy/eval.py:64-73 and gan/js_policy.py:43 call it: get_cost(xc, u, t,
    cost_params, mpc_weights, goal_X), predict(xc, u, t, dynamics_params), predict(xseq, critic_params) --
    no policy= argument, staging AND terminal branch, single samples and batches."""
    config, policy, params, data = _build(js_policy.JS_MPC)
    T = config.mpc.horizon
    p32 = _oracle_problem(params, data, np.arange(4), np.float32)
    p64 = _oracle_problem(params, data, np.arange(4), np.float64)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((4, N)).astype(np.float32)
    u = np.tanh(rng.standard_normal((4, M))).astype(np.float32)
    goal = data["goal"][:4]
    cm, dm, crm = policy.cost_model, policy.dynamics_model, policy.critic_model
    w = lambda p: orc.sigmoid(p["mpc_w"])
    gu.set_config(f"mirror n={N} m={M} T={T} model protocol")
    # staging branch, t < horizon: one sample, then a batch
    for t in (0, T - 1):
        c1 = cm.get_cost(x[1], u[1], t, params["cost_params"], params["mpc_weights"], goal[1])
        gu.assert_parity(f"get_cost stage t={t}", float(c1),
                         orc.stage_cost(x[1], u[1], p32["goal"][1, t], w(p32)),
                         orc.stage_cost(x[1].astype(np.float64), u[1].astype(np.float64), p64["goal"][1, t],
                                        w(p64)))
    cb = cm.get_cost(x, u, 2, params["cost_params"], params["mpc_weights"], goal)
    gu.assert_parity("get_cost stage batch", cb.cpu().numpy(), orc.stage_cost(x, u, p32["goal"][:, 2], w(p32)),
                     orc.stage_cost(x.astype(np.float64), u.astype(np.float64), p64["goal"][:, 2], w(p64)))
    # terminal branch, t == horizon, of an ARBITRARY state
    ct = cm.get_cost(x, u, T, params["cost_params"], params["mpc_weights"], goal)
    gu.assert_parity("get_cost terminal", ct.cpu().numpy(), orc.terminal_cost(p32["cmlp"], x, w(p32)[2]),
                     orc.terminal_cost(p64["cmlp"], x.astype(np.float64), w(p64)[2]))
    assert cm.get_cost(x[0], u[0], T, params["cost_params"], params["mpc_weights"], goal[0]).dim() == 0
    # dynamics
    nx = dm.predict(x, u, 3, params["dynamics_params"])
    gu.assert_parity("predict", nx.cpu().numpy(), orc.dynamics_predict(p32["dyn"], x, u)[0],
                     orc.dynamics_predict(p64["dyn"], x.astype(np.float64), u.astype(np.float64))[0])
    assert dm.predict(x[2], u[2], 0, params["dynamics_params"]).shape == (N,)
    # critic
    xs = data["Y"][:4]
    sc = crm.predict(xs, params["critic_params"])
    gu.assert_parity("critic predict", sc.cpu().numpy(), orc.critic_forward(p32["critic"], xs),
                     orc.critic_forward(p64["critic"], xs.astype(np.float64)))
    assert crm.predict(xs[0], params["critic_params"]).shape == (1,)
    # the two callbacks the reference hands to trajax (policy/eval.py:64-73), through the policy's engine
    c_pol = policy.cost(x[1], u[1], T, params, goal[1])
    assert abs(float(c_pol) - float(ct[1])) <= 1e-6 * abs(float(ct[1]))
    x_pol = policy.dynamics(x[1], u[1], 0, params)
    np.testing.assert_allclose(x_pol.cpu().numpy(), nx[1].cpu().numpy(), rtol=1e-6, atol=1e-7)
    # the terminal entry of a rollout is the terminal cost of its last state
    eng = policy.bind(policy.to_device_params(params), 4)
    X, costs = eng.rollout_cost(eng.to_dev(x), eng.to_dev(data["init_U"][:4]), eng.to_dev(goal))
    cT = cm.get_cost(X[:, -1].cpu().numpy(), u, T, params["cost_params"], params["mpc_weights"], goal)
    np.testing.assert_allclose(cT.cpu().numpy(), costs[:, -1].cpu().numpy(), rtol=2e-6)


def test_policies_with_the_lstm_dynamics_variant():
    """config `dynamics.use: "lstm"` (reference dynamics/nn.py:37-57): xc = [x, c, h].  The evaluation policy
    starts from the carry the history leaves behind (policy/eval.py:75-85, dynamics_model.py:24-43), the
    training policy from the zero carry (policy/base.py:31-38); goals, losses and the critic see x."""
    config, policy, params, data = _build(js_policy.JS_MPC, ndata=8, dyn_use="lstm")
    T, F = config.mpc.horizon, config.mpc.model.dynamics.lstm.lstm_features
    Nc = N + 2 * F
    assert params["cost_params"]["params"]["Dense_0"]["kernel"].shape[0] == Nc
    assert "OptimizedLSTMCell_0" in params["dynamics_params"]["params"]
    kw = {"maxiter": 2}
    policy.trajax_ilqr_kwargs.update(kw)
    idx = np.arange(5)
    p64 = _oracle_problem(params, data, idx, np.float64)
    p32 = _oracle_problem(params, data, idx, np.float32)
    gu.set_config(f"mirror lstm-dynamics nx={N} F={F} m={M} T={T}")
    # model protocol: predict on xc, zero / history carry
    dm = policy.dynamics_model
    assert dm.get_zero_carry(data["hist"][0, :-1]).shape == (2 * F,)
    rng = np.random.default_rng(1)
    xc = rng.standard_normal((5, Nc)).astype(np.float32)
    u = np.tanh(rng.standard_normal((5, M))).astype(np.float32)
    nxt = dm.predict(xc, u, 0, params["dynamics_params"])
    gu.assert_parity("lstm predict", nxt.cpu().numpy(), orc.dynamics_predict(p32["dyn"], xc, u)[0],
                     orc.dynamics_predict(p64["dyn"], xc.astype(np.float64), u.astype(np.float64))[0])
    hu = np.tanh(rng.standard_normal((config.mpc.history, M))).astype(np.float32)
    carry = dm.get_history_carry(data["hist"][0, :-1], hu, params["dynamics_params"])
    c64 = np.zeros(2 * F)
    for i in range(config.mpc.history):
        c64 = orc.dynamics_predict(p64["dyn"], np.concatenate([data["hist"][0, i].astype(np.float64), c64])[None],
                                   hu[i][None].astype(np.float64))[0][0, N:]
    assert gu.rel_err(carry, c64) < 1e-5
    # evaluation-style solve of one sample with a history of controls: the solve starts at [x, carry]
    from gan_mpc_amd.policy.eval import EvalMPC
    ev = EvalMPC(config=config, cost_model=policy.cost_model, dynamics_model=dm,
                 expert_model=TableExpert(data["goal"], data["init_U"]))
    ev.trajax_ilqr_kwargs.update(kw)
    ev.expert_model.select(np.array([0]))
    X, U, obj, *_ = ev.get_optimal_values(params, data["hist"][0], hu)
    assert X.shape == (T + 1, Nc) and gu.rel_err(X[0, N:].cpu().numpy(), c64) < 1e-5
    x0 = np.concatenate([data["hist"][0, -1].astype(np.float64), c64])[None]
    r = orc.ilqr(p64["dyn"], p64["cmlp"], p64["mpc_w"], p64["goal"][:1], x0, p64["U"][:1], kw)
    assert abs(float(obj) - r[2][0]) / abs(r[2][0]) < 1e-3
    # training-style batch: zero carry, loss and gradient against the oracle's batch mean
    policy.expert_model.select(idx)
    loss, grads = policy.loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
    res = {}
    for dt, p in ((np.float32, p32), (np.float64, p64)):
        x0 = np.concatenate([p["x0"], np.zeros((len(idx), 2 * F), dt)], -1)
        l, g_mpc, g_cost, _ = orc.loss_and_grad(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], x0, p["U"], loss="js",
                                                critic=p["critic"], kwargs=kw)
        res[dt] = (l, gu.pack_grads_cost(g_mpc, g_cost))
    gu.assert_parity("lstm-dynamics loss", float(loss), res[np.float32][0], res[np.float64][0], tol=1e-4, slack=10)
    # the policy layer at the GPU's own iterate, stage by stage (the method of test_gpu_parity.test_bilevel_grad):
    # the batch-mean gradient against the fp64 cost_vjp of the GPU's own (H, dX) is the check that sees the
    # policy's packing, sign, mean and carry handling; loss, Bvec, the Hessian solve's residual, the tangent roll
    # and the end-to-end gradient follow
    _check_policy_gradient_at_the_gpu_iterate(policy, p32, p64, 1, float(loss), grads, len(idx))
    # (recorded for comparison) each oracle running its own solve two iLQR iterations from a random start: with the
    # dynamics' curvature in it the Hessian is far from positive definite there and the solve is badly conditioned
    # (the NumPy fp32 oracle is ~0.2 from fp64), so this bar only rejects a gradient that is non-finite or off by
    # more than its own size
    gu.assert_parity("lstm-dynamics grads", grads.cpu().numpy(), res[np.float32][1], res[np.float64][1], tol=1e-3,
                     slack=1.0, ceiling=1.0, el_slack=1e9)


def _check_policy_gradient_at_the_gpu_iterate(policy, p32, p64, loss_kind, loss, grads, B, end_to_end=True):
    eng = policy._engine
    T, n, m = eng.T, eng.n, eng.m
    X = eng.debug_buffer(0, (B, T + 1, n)).cpu().numpy()
    U = eng.debug_buffer(1, (B, T, m)).cpu().numpy()
    Hd = eng.debug_buffer(2, (B, T, m)).cpu().numpy()
    dXd = eng.debug_buffer(3, (B, T + 1, n)).cpu().numpy()
    Bvd = eng.debug_buffer(4, (B, T, m)).cpu().numpy()
    # the solve started from [x0, zero carry]
    np.testing.assert_array_equal(X[:, 0, :eng.nx], p32["x0"])
    np.testing.assert_array_equal(X[:, 0, eng.nx:], 0.0)
    X64, U64 = X.astype(np.float64), U.astype(np.float64)
    keep = ~(gu.dyn_near_kink(p64["dyn"], X64, U64).any(1) | gu.near_kink(p64["cmlp"], X64[:, T]))
    assert keep.sum() >= max(1, B // 2), "too many trajectories near a relu kink; change the seed"
    # the end-to-end figure is the policy's batch mean, which cannot leave a trajectory out: the data seed of
    # _build (3) and these batches put no pre-activation near a kink (checked here, so that a change of data fails
    # as such and not as a parity failure)
    assert keep.all() or not end_to_end, f"trajectories {np.flatnonzero(~keep)} sit at a relu kink; change the seed"
    gu.check_bilevel_at_iterate(p32, p64, loss_kind, X, U, np.float32(loss), grads.cpu().numpy(), Hd, dXd, Bvd,
                                batch_mean=True, keep=keep, end_to_end=end_to_end)
