"""The stand-alone model calls -- gmpc_get_cost (k_get_cost) and gmpc_predict (a horizon-1 rollout on the ctx's
line-search scratch) -- against the oracle on every rollout family, and the rules they keep with a held solution.
Reached from the host through cost_model.get_cost / dynamics_model.predict / critic_model.predict (model_eval.py)
with the reference's own signatures (reference base.py:4-49)."""

import numpy as np
import pytest

import gan_mpc_oracle as orc
import gpu_util as gu
from gan_mpc_amd import GmpcError, model_eval
from gan_mpc_amd.gan import js_policy
from test_gpu_mirror import _build, _oracle_problem
from test_gpu_parity import SHAPES

pytestmark = pytest.mark.gpu

N, M = 4, 2      # test_gpu_mirror's sizes
MAX_BATCH = 8      # two workgroups of the 4-slot rollout kernels; B = 1 and 5 leave slots empty

CALL_SHAPES = {name: SHAPES[name] for name in (
    "tiny-ragged",       # the generic trajectory kernel
    "c2-cheetah",        # register weights, width 200
    "rw-128", "rw-64",   # register weights, widths 128 / 64
    "wide",              # cost hidden widths of 256 (one entry per thread, every wave)
    "big-70",            # the large-state context
    "c4-humanoid",       # n = 376: two entries per thread in k_get_cost, data in all four waves
    "c5-synthetic",      # n = 1024: four entries per thread
    "lowrank-1h",        # large state, low-rank dynamics
    "dynl-small", "dynl-big")}   # the LSTM dynamics kernel, both sizes
# n above 256 into three cost layers of the widest hidden width the engine builds (256): the terminal branch
# runs several layers, each thread owning two inputs of layer 0
CALL_SHAPES["cost-deep-n300"] = (300, 5, 3, 5, dict(dyn_hidden=(64,), cost_hidden=(256, 200, 256), cost_fout=32,
                                                      out_scale=0.3))


def _setup(name, T=None):
    n, m, T0, _, kw = CALL_SHAPES[name]
    pb = gu.problem(n, m, T0 if T is None else T, MAX_BATCH, seed=11, **kw)
    gu.set_config(f"model calls {name} n={pb['n']} m={m} T={pb['T']}")
    return pb, orc.cast_problem(pb, np.float64), gu.engine_for(pb, critic=False)


def _inputs(pb, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((MAX_BATCH, pb["n"])).astype(np.float32)
    u = np.tanh(rng.standard_normal((MAX_BATCH, pb["m"]))).astype(np.float32)
    return x, u


@pytest.mark.parametrize("name", list(CALL_SHAPES))
def test_get_cost_and_predict_against_oracle(name):
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    T, nx = pb["T"], pb.get("nx", pb["n"])
    x, u = _inputs(pb)
    xs = x.copy()
    if nx < pb["n"]:
        # the staging cost reads x only: a read of the carry columns would show at this size
        xs[:, nx:] = 1e3 * np.random.default_rng(6).standard_normal((MAX_BATCH, pb["n"] - nx))
    w32, w64 = orc.sigmoid(pb["mpc_w"]), orc.sigmoid(pb64["mpc_w"])
    for B in (1, 5, MAX_BATCH):
        for t in (0, T - 1):
            g = pb["goal"][:B, t]
            c = eng.get_cost(d(xs[:B]), d(u[:B]), d(g), False).cpu().numpy()
            gu.assert_parity(f"get_cost staging t={t} B={B}", c, orc.stage_cost(xs[:B], u[:B], g, w32),
                             orc.stage_cost(xs[:B].astype(np.float64), u[:B].astype(np.float64),
                                            g.astype(np.float64), w64))
        c = eng.get_cost(d(x[:B]), d(u[:B]), None, True).cpu().numpy()
        gu.assert_parity(f"get_cost terminal B={B}", c, orc.terminal_cost(pb["cmlp"], x[:B], w32[2]),
                         orc.terminal_cost(pb64["cmlp"], x[:B].astype(np.float64), w64[2]))
        nxt = eng.predict(d(x[:B]), d(u[:B])).cpu().numpy()
        gu.assert_parity(f"predict B={B}", nxt, orc.dynamics_predict(pb["dyn"], x[:B], u[:B])[0],
                         orc.dynamics_predict(pb64["dyn"], x[:B].astype(np.float64), u[:B].astype(np.float64))[0])


@pytest.mark.parametrize("name", ["tiny-ragged", "c2-cheetah", "rw-128", "big-70", "dynl-small", "dynl-big"])
def test_predict_does_not_depend_on_the_engine_horizon(name):
    """predict is a horizon-1 rollout whatever the engine's T: an engine built for T = 5 returns the bits of one built
    for T = 1 with the same weights (the policy's own engine, with the config's horizon, serves predict)."""
    out = {}
    for T in (1, 5):
        pb, pb64, eng = _setup(name, T=T)
        x, u = _inputs(pb)
        out[T] = eng.predict(eng.to_dev(x), eng.to_dev(u)).cpu().numpy()
        eng.close()
    gu.assert_parity("predict (T = 5 engine)", out[5], orc.dynamics_predict(pb["dyn"], x, u)[0],
                     orc.dynamics_predict(pb64["dyn"], x.astype(np.float64), u.astype(np.float64))[0])
    np.testing.assert_array_equal(out[5], out[1])


@pytest.mark.parametrize("name", ["tiny-ragged", "c2-cheetah", "big-70", "dynl-small"])
def test_model_calls_and_the_held_solution(name):
    """gmpc_predict overwrites the relu masks and objectives of a held solution, so bilevel_grad / upper_loss refuse
    after it; gmpc_get_cost touches none of that state, so a get_cost between the solve and bilevel_grad changes no
    bit of the loss or the gradient."""
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    B = MAX_BATCH
    x, u = _inputs(pb)
    args = (d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 2})
    desired = d(pb["true_seq"])

    eng.ilqr_solve(*args)
    loss, g = eng.bilevel_grad(B, 0, desired=desired)
    ref = (loss.cpu().numpy(), g.cpu().numpy())
    eng.ilqr_solve(*args)
    c0 = eng.get_cost(d(x), d(u), d(pb["goal"][:, 0]), False)
    c1 = eng.get_cost(d(x), d(u), None, True)
    loss, g = eng.bilevel_grad(B, 0, desired=desired)
    np.testing.assert_array_equal(loss.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(g.cpu().numpy(), ref[1])
    assert np.isfinite(c0.cpu().numpy()).all() and np.isfinite(c1.cpu().numpy()).all()

    eng.ilqr_solve(*args)
    eng.predict(d(x), d(u))
    with pytest.raises(GmpcError, match="must precede"):
        eng.bilevel_grad(B, 0, desired=desired)
    with pytest.raises(GmpcError, match="must precede"):
        eng.upper_loss(B, 0, desired=desired)
    # a new solve holds a solution again
    eng.ilqr_solve(*args)
    loss, g = eng.bilevel_grad(B, 0, desired=desired)
    np.testing.assert_array_equal(g.cpu().numpy(), ref[1])


def test_a_cost_hidden_width_above_256_is_refused():
    """k_get_cost (and every cost kernel) gives one thread per unit of a 256-thread workgroup: wider cost layers
    are refused when the engine is built, not computed wrongly."""
    from gan_mpc_amd.engine import Engine
    with pytest.raises(GmpcError, match="cost hidden width"):
        Engine(40, 9, 6, [49, 64, 40], [40, 300, 40, 8], max_batch=2)


def test_model_protocol_with_the_lstm_dynamics_variant():
    """cost_model.get_cost with the LSTM dynamics: xc = [x, c, h] is N + 2F wide, the goal N wide.  The staging
    branch reads xc[:, :N] (reference cost_model.py:24-25) on an engine model_eval builds for it; the terminal
    branch is the cost MLP of the whole xc."""
    config, policy, params, data = _build(js_policy.JS_MPC, ndata=8, dyn_use="lstm")
    T, F = config.mpc.horizon, config.mpc.model.dynamics.lstm.lstm_features
    Nc = N + 2 * F
    gu.set_config(f"model calls lstm-dynamics nx={N} F={F} T={T}")
    p32 = _oracle_problem(params, data, np.arange(5), np.float32)
    p64 = _oracle_problem(params, data, np.arange(5), np.float64)
    rng = np.random.default_rng(2)
    xc = rng.standard_normal((5, Nc)).astype(np.float32)
    xc[:, N:] *= 1e3          # a read of the carry by the staging branch would show
    u = np.tanh(rng.standard_normal((5, M))).astype(np.float32)
    goal = data["goal"][:5]
    cm = policy.cost_model
    w32, w64 = orc.sigmoid(p32["mpc_w"]), orc.sigmoid(p64["mpc_w"])
    x64, u64 = xc.astype(np.float64), u.astype(np.float64)
    for t in (0, T - 1):
        c = cm.get_cost(xc, u, t, params["cost_params"], params["mpc_weights"], goal)
        gu.assert_parity(f"lstm get_cost staging t={t}", c.cpu().numpy(), orc.stage_cost(xc, u, p32["goal"][:, t], w32),
                         orc.stage_cost(x64, u64, p64["goal"][:, t], w64))
        c1 = cm.get_cost(xc[3], u[3], t, params["cost_params"], params["mpc_weights"], goal[3])
        assert c1.dim() == 0
        np.testing.assert_array_equal(c1.cpu().numpy(), c[3].cpu().numpy())
    xt = rng.standard_normal((5, Nc)).astype(np.float32)
    ct = cm.get_cost(xt, u, T, params["cost_params"], params["mpc_weights"], goal)
    gu.assert_parity("lstm get_cost terminal", ct.cpu().numpy(), orc.terminal_cost(p32["cmlp"], xt, w32[2]),
                     orc.terminal_cost(p64["cmlp"], xt.astype(np.float64), w64[2]))


def test_model_calls_rebuild_the_cached_engine_for_a_larger_batch():
    """model_eval keeps one engine per shape, sized for 8; a batch of 20 after a batch of 4 rebuilds it.  Every row
    of the large batch equals the single-sample call, bit for bit."""
    for eng in model_eval._ENGINES.values():
        eng.close()
    model_eval._ENGINES.clear()
    config, policy, params, data = _build(js_policy.JS_MPC)
    T = config.mpc.horizon
    rng = np.random.default_rng(3)
    x = rng.standard_normal((20, N)).astype(np.float32)
    u = np.tanh(rng.standard_normal((20, M))).astype(np.float32)
    goal = rng.standard_normal((20, T + 1, N)).astype(np.float32)
    cm, dm = policy.cost_model, policy.dynamics_model
    cp, w, dp = params["cost_params"], params["mpc_weights"], params["dynamics_params"]
    single_c = [cm.get_cost(x[i], u[i], 2, cp, w, goal[i]).cpu().numpy() for i in range(20)]
    single_t = [cm.get_cost(x[i], u[i], T, cp, w, goal[i]).cpu().numpy() for i in range(20)]
    single_p = [dm.predict(x[i], u[i], 0, dp).cpu().numpy() for i in range(20)]
    small = cm.get_cost(x[:4], u[:4], 2, cp, w, goal[:4]).cpu().numpy()
    np.testing.assert_array_equal(small, np.stack(single_c[:4]))
    assert max(e.max_batch for e in model_eval._ENGINES.values()) == 8
    big_c = cm.get_cost(x, u, 2, cp, w, goal).cpu().numpy()
    big_t = cm.get_cost(x, u, T, cp, w, goal).cpu().numpy()
    big_p = dm.predict(x, u, 0, dp).cpu().numpy()
    assert max(e.max_batch for e in model_eval._ENGINES.values()) >= 20
    np.testing.assert_array_equal(big_c, np.stack(single_c))
    np.testing.assert_array_equal(big_t, np.stack(single_t))
    np.testing.assert_array_equal(big_p, np.stack(single_p))
    p64 = _oracle_problem(params, data, np.arange(1), np.float64)
    p32 = _oracle_problem(params, data, np.arange(1), np.float32)
    gu.set_config(f"model calls mirror n={N} m={M} T={T} B=20")
    gu.assert_parity("get_cost staging B=20", big_c,
                     orc.stage_cost(x, u, goal[:, 2], orc.sigmoid(p32["mpc_w"])),
                     orc.stage_cost(x.astype(np.float64), u.astype(np.float64), goal[:, 2].astype(np.float64),
                                    orc.sigmoid(p64["mpc_w"])))
    gu.assert_parity("predict B=20", big_p, orc.dynamics_predict(p32["dyn"], x, u)[0],
                     orc.dynamics_predict(p64["dyn"], x.astype(np.float64), u.astype(np.float64))[0])


@pytest.mark.parametrize("count", [1, 3, 17])
def test_critic_predict_on_odd_counts(count):
    """critic_model.predict sizes its engine by (count + 1) // 2 sequences; odd counts leave the last pair half
    used."""
    config, policy, params, data = _build(js_policy.JS_MPC, ndata=24)
    xs = data["Y"][:count]
    p32 = _oracle_problem(params, data, np.arange(count), np.float32)
    p64 = _oracle_problem(params, data, np.arange(count), np.float64)
    gu.set_config(f"model calls critic predict count={count}")
    sc = policy.critic_model.predict(xs if count > 1 else xs[0], params["critic_params"])
    assert sc.shape == (count,)
    gu.assert_parity(f"critic predict count={count}", sc.cpu().numpy(), orc.critic_forward(p32["critic"], xs),
                     orc.critic_forward(p64["critic"], xs.astype(np.float64)))
