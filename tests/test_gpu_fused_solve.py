"""gmpc_ilqr_solve_fused -- the whole iLQR solve of every trajectory in one kernel launch -- on the GPU:

  a. the control-flow scenarios of tests/test_gpu_control_flow.py under its _run protocol and bars, with the engine's
     solve pointed at the fused entry point;
  b. the reference regime (horizon 5, pendulum and cheetah, default nets, maxiter 100; B = 1, 7, 128) against the
     oracle under the same protocol, and against gmpc_ilqr_solve on the same inputs;
  c. grad, adjoints and the [A | B] block the solve leaves in the ctx against the oracle at its own final iterate;
  d. gmpc_bilevel_grad behind a fused solve (L2 and JS losses);
  e. the policy interface: EvalMPC / L2MPC with solver="fused";
  f. what the entry point refuses, and maxiter = 0;
  g. determinism, alone and interleaved with round-based solves on the same ctx.
Reference: trajax ilqr_base / line_search_ddp as called from policy/optimizers.py:19-21, policy/eval.py:10-20;
restated at oracle/gan_mpc_oracle.py:ilqr."""

import functools

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_control_flow as cf
import test_gpu_mirror as mirror
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.engine import TRAJAX_iLQR_KWARGS, Engine
from gan_mpc_amd.norm import l2_policy

pytestmark = pytest.mark.gpu


@pytest.fixture
def fused_engines(monkeypatch):
    """Engines built by gu.engine_for solve through gmpc_ilqr_solve_fused."""
    make = gu.engine_for

    def engine_for(*args, **kw):
        eng = make(*args, **kw)
        eng.ilqr_solve = eng.ilqr_solve_fused
        return eng

    monkeypatch.setattr(gu, "engine_for", engine_for)


# ---- a. control-flow scenarios ---------------------------------------------------------------------------------
def test_full_steps_on_a_tame_problem(fused_engines):
    cf.test_full_steps_on_a_tame_problem()


def test_deep_backtracking(fused_engines):
    cf.test_deep_backtracking()


def test_nan_start_never_iterates_and_neighbours_do(fused_engines):
    cf.test_nan_start_never_iterates_and_neighbours_do()


@pytest.mark.parametrize("kw", [
    {"grad_norm_threshold": 0.6},
    {"relative_grad_norm_threshold": 0.03},
    {"obj_step_threshold": 0.005},
    {"inputs_step_threshold": 0.3},
    {"alpha_min": 0.01},
    {"alpha_0": 0.6, "alpha_min": 0.01},
])
def test_each_threshold_of_the_continuation_criterion(kw, fused_engines):
    cf.test_each_threshold_of_the_continuation_criterion(kw)


def test_members_stop_at_different_iterations(fused_engines):
    cf.test_members_stop_at_different_iterations_and_the_enqueued_tail_is_a_no_op()


def test_headline_widths_heterogeneous_stops(fused_engines, monkeypatch):
    cf.test_headline_shape_heterogeneous_stops(False, monkeypatch)


# ---- b. the reference regime -----------------------------------------------------------------------------------
REF = {"pendulum": (3, 1), "cheetah": (17, 6)}
# Under the reference kwargs two fp32 solves (the fp32 oracle against its own 1e-6 perturbations) stop agreeing on
# the control flow after a few iterations: over all 100 the _run protocol finds 0 - 1 % of the trajectories decided.
# From the second iteration on, line searches accept at halvings 10 - 12, where "strictly smaller objective" is decided
# by the summation order of the objective (fp32, 6 terms; the protocol's perturbed runs do not vary that order): one
# trajectory of 128 took a different halving there.  The protocol therefore runs the first iteration; the whole solve
# is compared with gmpc_ilqr_solve.
PROTO_ITERS = 1
MIN_AGREE = {1: 0.0, 7: 0.4, 128: 0.4}


def _ref_problem(name, B):
    n, m = REF[name]
    return gu.problem(n, m, 5, B, seed=5, out_scale=0.1)


@pytest.mark.parametrize("B", [1, 7, 128])
@pytest.mark.parametrize("name", list(REF))
def test_reference_regime(name, B, fused_engines):
    pb = _ref_problem(name, B)
    kw = dict(TRAJAX_iLQR_KWARGS, maxiter=PROTO_ITERS)
    eng, out, r64, agree = cf._run(pb, kw, label=f"fused reference {name} B={B}", min_agree=MIN_AGREE[B],
                                   tol=1e-3, tol_obj=3e-4)
    try:
        d = eng.to_dev
        args = (d(pb["x0"]), d(pb["U"]), d(pb["goal"]))
        # the round-based solve on the same ctx and inputs: equal iteration counts and step sizes where decided
        fused = {k: v.cpu().numpy() for k, v in eng.ilqr_solve_fused(*args, kw).items()}
        alpha_f = eng.debug_buffer(8, (B,)).cpu().numpy()
        rounds = {k: v.cpu().numpy() for k, v in Engine._solve(eng, eng.lib.gmpc_ilqr_solve, *args, kw).items()}
        alpha_r = eng.debug_buffer(8, (B,)).cpu().numpy()
        np.testing.assert_array_equal(fused["iterations"][agree], rounds["iterations"][agree])
        np.testing.assert_array_equal(alpha_f[agree], alpha_r[agree])
        fin = agree & np.isfinite(r64[2])
        if fin.any():
            gu.assert_parity(f"fused vs rounds obj {name} B={B}", fused["obj"][fin], rounds["obj"][fin], r64[2][fin],
                             tol=3e-4, ceiling=gu.GAIN_CEILING)
        # the whole solve (maxiter 100): where the round-based objective is finite the fused one is too, and both end
        # at the same objective -- in the median to 1e-4, every trajectory to 1e-2 (after 100 fp32 iterations whose
        # control flow is not decided, a trajectory may settle a little elsewhere: 2e-3 for one of pendulum's 128)
        full = dict(TRAJAX_iLQR_KWARGS)
        f100 = {k: v.cpu().numpy() for k, v in eng.ilqr_solve_fused(*args, full).items()}
        r100 = {k: v.cpu().numpy() for k, v in Engine._solve(eng, eng.lib.gmpc_ilqr_solve, *args, full).items()}
        assert (f100["iterations"] <= 100).all() and (f100["iterations"] >= 1).all()
        ok = np.isfinite(r100["obj"])
        assert np.isfinite(f100["obj"][ok]).all()
        rel = np.abs(f100["obj"][ok] - r100["obj"][ok]) / np.maximum(np.abs(r100["obj"][ok]), 1e-6)
        gu._record(dict(stage=f"fused vs rounds obj after 100 iterations {name} B={B} (max relative difference)",
                        config=gu.CURRENT_CONFIG[0], e_hip=float(rel.max()), e_o32=float(np.median(rel)), tol=1e-4,
                        tol_used=1e-2, branch="info", entries=int(ok.sum()),
                        passed=bool(np.median(rel) <= 1e-4 and rel.max() <= 1e-2)))
        assert np.median(rel) <= 1e-4 and rel.max() <= 1e-2, (name, B, np.median(rel), rel.max())
    finally:
        eng.close()


# ---- c. final outputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(REF))
def test_final_outputs_at_the_fused_iterate(name):
    pb = _ref_problem(name, 16)
    pb64 = orc.cast_problem(pb, np.float64)
    gu.set_config(f"fused final outputs {name} B=16")
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        B, T, n, m = pb["B"], pb["T"], pb["n"], pb["m"]
        out = eng.ilqr_solve_fused(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 4})
        X, U = out["X"].cpu().numpy(), out["U"].cpu().numpy()
        AB = eng.debug_buffer(5, (B, T, n, n + m)).cpu().numpy()
        X64, U64 = X.astype(np.float64), U.astype(np.float64)
        ok = ~(gu.dyn_near_kink(pb64["dyn"], X64, U64).any(1) | gu.near_kink(pb64["cmlp"], X64[:, T]))
        assert ok.sum() >= B // 2
        l32 = orc.get_lqr_params(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], X, U)
        l64 = orc.get_lqr_params(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X64, U64)
        g32, a32 = orc.adjoint(l32[5], l32[6], l32[1], l32[3])
        g64, a64 = orc.adjoint(l64[5], l64[6], l64[1], l64[3])
        gu.assert_parity("fused grad", out["grad"].cpu().numpy()[ok], g32[ok], g64[ok])
        gu.assert_parity("fused adjoints", out["adjoints"].cpu().numpy()[ok], a32[ok], a64[ok])
        ab32 = np.concatenate([l32[5][:, :T], l32[6][:, :T]], -1)
        ab64 = np.concatenate([l64[5][:, :T], l64[6][:, :T]], -1)
        gu.assert_parity("fused [A|B]", AB[ok], ab32[ok], ab64[ok])
    finally:
        eng.close()


# ---- d. bilevel gradient after a fused solve -------------------------------------------------------------------
@pytest.mark.parametrize("loss_kind", [0, 1])
def test_bilevel_grad_after_a_fused_solve(loss_kind):
    pb = gu.problem(17, 6, 10, 16, seed=11, out_scale=0.1)
    pb64 = orc.cast_problem(pb, np.float64)
    gu.set_config("fused bilevel n=17 m=6 T=10 B=16")
    eng = gu.engine_for(pb, critic=True)
    try:
        d = eng.to_dev
        T, n, m = pb["T"], pb["n"], pb["m"]
        out = eng.ilqr_solve_fused(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 3})
        Xf = out["X"].cpu().numpy().astype(np.float64)
        Uf = out["U"].cpu().numpy()
        bad = gu.dyn_near_kink(pb64["dyn"], Xf, Uf.astype(np.float64)).any(1) | gu.near_kink(pb64["cmlp"], Xf[:, T])
        ok = ~bad
        assert ok.sum() >= max(1, pb["B"] // 2)
        for p_ in (pb, pb64):
            for key in ("x0", "goal", "true_seq"):
                p_[key] = p_[key][ok]
        B = int(ok.sum())
        out = eng.ilqr_solve_fused(d(pb["x0"]), d(Uf[ok]), d(pb["goal"]), {"maxiter": 0})
        loss, gsum = eng.bilevel_grad(B, loss_kind, desired=d(pb["true_seq"]), critic=d(gu.critic_flat(pb)), sign=1.0)
        X = out["X"].cpu().numpy()
        U = out["U"].cpu().numpy()
        Hd = eng.debug_buffer(2, (B, T, m)).cpu().numpy()
        dXd = eng.debug_buffer(3, (B, T + 1, n)).cpu().numpy()
        Bvd = eng.debug_buffer(4, (B, T, m)).cpu().numpy()
        gu.check_bilevel_at_iterate(pb, pb64, loss_kind, X, U, loss.cpu().numpy(), gsum.cpu().numpy(), Hd, dXd, Bvd)
    finally:
        eng.close()


# ---- e. policy level ---------------------------------------------------------------------------------------------
def _count_fused(monkeypatch):
    calls = []
    orig = Engine.ilqr_solve_fused

    def counted(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    monkeypatch.setattr(Engine, "ilqr_solve_fused", counted)
    return calls


def test_eval_policy_action_is_the_first_control_of_the_fused_solve(monkeypatch):
    calls = _count_fused(monkeypatch)
    config, policy, params, data = mirror._build(functools.partial(l2_policy.L2MPC, solver="fused"))
    assert policy.solver == "fused"
    policy.expert_model.select(np.array([2]))
    a = policy.get_optimal_action(params, data["hist"][2])
    assert calls, "the fused entry point was not called"
    eng = policy._engine
    T, n, m = eng.T, eng.n, eng.m
    U = eng.debug_buffer(1, (1, T, m)).cpu().numpy()
    np.testing.assert_array_equal(a.cpu().numpy(), U[0, 0])
    policy.expert_model.select(np.array([2]))
    X, U, obj, grad, adj, lqr, itr = policy.get_optimal_values(params, data["hist"][2])
    assert lqr.shape == (T, n, n + m)
    p64 = mirror._oracle_problem(params, data, np.array([2]), np.float64)
    r = orc.ilqr(p64["dyn"], p64["cmlp"], p64["mpc_w"], p64["goal"], p64["x0"], p64["U"])
    assert abs(float(obj) - r[2][0]) / abs(r[2][0]) < 1e-3


def test_l2_policy_loss_and_grad_through_the_fused_solve(monkeypatch):
    calls = _count_fused(monkeypatch)
    config, policy, params, data = mirror._build(functools.partial(l2_policy.L2MPC, solver="fused"))
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    idx = np.arange(8)
    policy.expert_model.select(idx)
    loss, grads = policy.loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
    assert calls, "the fused entry point was not called"
    res = {}
    for dt in (np.float32, np.float64):
        p = mirror._oracle_problem(params, data, idx, dt)
        l, g_mpc, g_cost, _ = orc.loss_and_grad(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], p["x0"], p["U"],
                                                loss="l2", desired=p["true_seq"], kwargs={"maxiter": 2})
        res[dt] = (l, gu.pack_grads_cost(g_mpc, g_cost))
    gu.assert_parity("fused policy loss", float(loss), res[np.float32][0], res[np.float64][0], tol=1e-4, slack=10)
    mirror._check_policy_gradient_at_the_gpu_iterate(policy, mirror._oracle_problem(params, data, idx, np.float32),
                                                     mirror._oracle_problem(params, data, idx, np.float64), 0,
                                                     float(loss), grads, len(idx), end_to_end=False)
    gu.assert_parity("fused policy grads", grads.cpu().numpy(), res[np.float32][1], res[np.float64][1], tol=1e-3,
                     slack=10)


# ---- f. refusals -------------------------------------------------------------------------------------------------
def _solve_fused(pb, kw=None, B=None):
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        B = pb["B"] if B is None else B
        x0 = np.resize(pb["x0"], (B,) + pb["x0"].shape[1:])
        U = np.resize(pb["U"], (B,) + pb["U"].shape[1:])
        goal = np.resize(pb["goal"], (B,) + pb["goal"].shape[1:])
        return eng.ilqr_solve_fused(d(x0), d(U), d(goal), kw)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n65", "m33", "T33"])
def test_refused_shapes(case):
    args = dict(lstm=dict(n=3, m=1, T=5, dyn_hidden=(16,), dyn_lstm=8), n65=dict(n=65, m=2, T=3),
                m33=dict(n=4, m=33, T=3), T33=dict(n=3, m=1, T=33))[case]
    n, m, T = args.pop("n"), args.pop("m"), args.pop("T")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, T, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    with pytest.raises(GmpcError, match="fused"):
        _solve_fused(pb, {"maxiter": 2})


def test_refused_options_and_batch():
    pb = gu.problem(3, 1, 5, 2, seed=1, dyn_hidden=(32, 32), cost_hidden=(16,), cost_fout=4)
    with pytest.raises(GmpcError, match="make_psd"):
        _solve_fused(pb, {"make_psd": True})
    with pytest.raises(GmpcError, match="fused"):
        _solve_fused(pb, {"alpha_0": 1.0, "alpha_min": 1e-6})     # 20 halvings
    with pytest.raises(GmpcError, match="max_batch"):
        _solve_fused(pb, {"maxiter": 2}, B=3)


def test_maxiter_zero_returns_the_initial_rollout():
    pb = _ref_problem("cheetah", 7)
    pb64 = orc.cast_problem(pb, np.float64)
    gu.set_config("fused maxiter=0 cheetah T=5 B=7")
    out = _solve_fused(pb, {"maxiter": 0})
    assert (out["iterations"].cpu().numpy() == 0).all()
    gu.assert_parity("fused maxiter=0 X", out["X"].cpu().numpy(), orc.rollout(pb["dyn"], pb["U"], pb["x0"]),
                     orc.rollout(pb64["dyn"], pb64["U"], pb64["x0"]))
    np.testing.assert_array_equal(out["U"].cpu().numpy(), pb["U"])
    o32 = orc.objective(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], pb["U"], pb["x0"])
    o64 = orc.objective(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], pb64["U"], pb64["x0"])
    gu.assert_parity("fused maxiter=0 obj", out["obj"].cpu().numpy(), o32, o64)


# ---- g. determinism ----------------------------------------------------------------------------------------------
KEYS = ("X", "U", "obj", "grad", "adjoints", "iterations")


def _snap(out):
    return {k: out[k].cpu().numpy().copy() for k in KEYS}


def _equal(a, b, what):
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def test_fused_solve_is_deterministic_and_independent_of_round_based_solves():
    pb = _ref_problem("cheetah", 7)
    kw = {"maxiter": 6}

    def run(seq):
        eng = gu.engine_for(pb, critic=False)
        try:
            d = eng.to_dev
            args = (d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
            return [_snap(eng.ilqr_solve_fused(*args) if s == "f" else eng.ilqr_solve(*args)) for s in seq]
        finally:
            eng.close()

    f1, f2 = run("ff")
    _equal(f1, f2, "two fused solves")
    (r_fresh,) = run("r")
    _, f_after_r = run("rf")
    _equal(f_after_r, f1, "fused after a round-based solve")
    _, r_after_f = run("fr")
    _equal(r_after_f, r_fresh, "round-based after a fused solve")
    torch.cuda.synchronize()
