"""The ensemble rollout's VJP without a GPU (gmpc_ensemble_rollout_vjp): the NumPy reference's
sums in fp32 and fp64 (H1); the reference against central differences, in fp64, of ensemble_rollout_ref.rollout (H2);
the risk aggregates' gradients against differences of plan_risk's definition (H3); the entry point's declaration,
binding and argument order (H4); every Engine, layer and policy refusal raised before the library is called (H5)."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ensemble_rollout_ref as rr
import ensemble_rollout_vjp_ref as vr
import gan_mpc_oracle as orc
import sampled_ensemble_cases as ec
import sampled_ensemble_ref as er
from gan_mpc_amd._lib import GmpcError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ctx", "B", "P", "dyn_members", "X", "U", "goal", "gX", "gcost", "grad_x0", "grad_U", "grad_goal",
        "grad_theta_sum", "grad_members", "stream"]


def _cots(X, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(X.shape).astype(dtype), rng.standard_normal(X.shape[:3]).astype(dtype)


# ---- H1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "ragged"])
def test_h1_the_reference_loops_the_members_and_sums_in_member_order(name):
    pb, members = ec.problem(name), ec.members(name)
    from test_rollout_vjp_host import reference as one
    for dt in (np.float32, np.float64):
        p = orc.cast_problem(pb, dt)
        X = rr.rollout(p, members)["X"]
        gX, gc = _cots(X, 1, dt)
        ref = vr.reference(p, members, X, p["U"], p["goal"], gX, gc)
        assert all(ref[k].dtype == dt for k in vr.KEYS)
        per = [one(dict(p, dyn=layers), X[q], p["U"], p["goal"], gX[q], gc[q])
               for q, layers in enumerate(er.cast_members(members, dt))]
        for k in ("x0", "U", "goal", "theta"):
            np.testing.assert_array_equal(ref[k], ((per[0][k] + per[1][k]).astype(dt) + per[2][k]).astype(dt))
        for q in range(3):
            np.testing.assert_array_equal(ref["members"][q], per[q]["dyn"])
        assert not ref["goal"][:, -1].any()
        # one member: its value comes through bit for bit
        alone = vr.reference(p, members[1:2], X[1:2], p["U"], p["goal"], gX[1:2], gc[1:2])
        for k in ("x0", "U", "goal", "theta"):
            np.testing.assert_array_equal(alone[k], per[1][k])
        # no cost cotangent: nothing reaches the goals or the costs' parameters
        nogc = vr.reference(p, members, X, p["U"], p["goal"], gX, None)
        assert not nogc["goal"].any() and not nogc["theta"].any() and nogc["members"].any()


# ---- H2 ------------------------------------------------------------------------------------------------------------
def _flat(layers):
    return np.concatenate([np.concatenate([W.reshape(-1), b]) for W, b in layers])


def _unflat(like, v):
    out, o = [], 0
    for W, b in like:
        out.append((v[o:o + W.size].reshape(W.shape), v[o + W.size:o + W.size + b.size]))
        o += W.size + b.size
    return out


@pytest.mark.parametrize("name", ["base", "ragged"])
def test_h2_the_reference_matches_central_differences_of_the_ensemble_rollout(name):
    pb = orc.cast_problem(ec.problem(name), np.float64)
    members = er.cast_members(ec.members(name), np.float64)
    X = rr.rollout(pb, members)["X"]
    gX, gc = _cots(X, 2)
    ref = vr.reference(pb, members, X, pb["U"], pb["goal"], gX, gc)
    theta = np.concatenate([pb["mpc_w"], _flat(pb["cmlp"])])
    mem = np.stack([_flat(layers) for layers in members])
    assert ref["theta"].shape == theta.shape and ref["members"].shape == mem.shape

    def L(x0, U, goal, th, mv):
        p = dict(pb, x0=x0, U=U, goal=goal, mpc_w=th[:3], cmlp=_unflat(pb["cmlp"], th[3:]))
        out = rr.rollout(p, [_unflat(members[0], v) for v in mv])
        return float(np.sum(gX * out["X"]) + np.sum(gc * out["costs"]))

    rng = np.random.default_rng(4)
    # A relu unit whose kink lies inside [-eps, eps] along the direction adds an error of the order of its own share
    # of the derivative, whatever eps is; only their number shrinks with eps.  base has 3 members x 72 rows x 600
    # units, and every weight moves: at eps = 1e-6 one of them crosses (2.5e-5 off), at 1e-8 none does, and fp64
    # rounding (1e-16 |L| / eps) is still 1e-8 of the difference.
    eps = 1e-8
    for _ in range(3):
        d = [rng.standard_normal(a.shape) for a in (pb["x0"], pb["U"], pb["goal"], theta, mem)]
        d[2][:, -1] = 0    # the terminal row of the goal is not read
        at = (pb["x0"], pb["U"], pb["goal"], theta, mem)
        fd = (L(*(a + eps * e for a, e in zip(at, d))) - L(*(a - eps * e for a, e in zip(at, d)))) / (2 * eps)
        lin = sum(float(np.sum(ref[k] * e)) for k, e in zip(vr.KEYS, d))
        assert abs(fd) > 1e-3
        np.testing.assert_allclose(lin, fd, rtol=1e-6)


# ---- H3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggregate,risk", [("mean", 0.0), ("mean_std", 0.7), ("mean_std", -0.3), ("max", 0.0)])
def test_h3_the_risk_aggregates_and_their_gradients(aggregate, risk):
    rng = np.random.default_rng(7)
    J = rng.standard_normal((5, 6)) + 3.0
    R, w = vr.risk(J, aggregate, risk)
    want = dict(mean=J.mean(0), mean_std=J.mean(0) + risk * J.std(0), max=J.max(0))[aggregate]
    np.testing.assert_allclose(R, want, rtol=1e-14)
    eps = 1e-6
    for p in range(5):
        for b in range(6):
            e = np.zeros_like(J)
            e[p, b] = eps
            fd = (vr.risk(J + e, aggregate, risk)[0] - vr.risk(J - e, aggregate, risk)[0]) / (2 * eps)
            np.testing.assert_allclose(fd[b], w[p, b], rtol=1e-7, atol=1e-9)
            assert not np.delete(fd, b).any()
    # the policy's torch restatement is the same definition
    from gan_mpc_amd.policy.base import BaseMPC
    Rt, wt = BaseMPC._risk(torch.as_tensor(J), aggregate, risk)
    np.testing.assert_allclose(Rt.numpy(), R, rtol=1e-14)
    np.testing.assert_allclose(wt.numpy(), w, rtol=1e-13, atol=1e-15)
    # identical members: no spread, the mean's weights
    same = np.broadcast_to(J[:1], J.shape).copy()
    R0, w0 = vr.risk(same, "mean_std", 0.5)
    np.testing.assert_array_equal(R0, same[0])
    np.testing.assert_array_equal(w0, np.full_like(same, 0.2))


# ---- H4 ------------------------------------------------------------------------------------------------------------
def test_h4_the_entry_point_is_declared_and_bound():
    from gan_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    m = re.search(r"\bint\s+gmpc_ensemble_rollout_vjp\s*\(([^)]*)\)\s*;", header)
    assert m, "gmpc_ensemble_rollout_vjp is not declared in the header"
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in decl] == ARGS
    kinds = [C.c_void_p if "*" in a else C.c_int for a in decl]
    assert _lib.SIGNATURES["gmpc_ensemble_rollout_vjp"] == (C.c_int, kinds)
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "gmpc_ensemble_rollout_vjp")


class _Lib:
    def __init__(self):
        self.calls = []

    def gmpc_ensemble_rollout_vjp(self, *args):
        self.calls.append(args)
        return 0


def _engine(n=5, m=2, T=8, dyn_count=10, cost_count=7):
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.dyn_count, eng.cost_count = _Lib(), "ctx", dyn_count, cost_count
    eng.n, eng.m, eng.T, eng.device = n, m, T, "cpu"
    eng._stream = lambda: "stream"
    eng.to_dev = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    eng.new = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)
    return eng


def test_h4_the_engine_passes_the_arguments_in_the_headers_order(monkeypatch):
    import gan_mpc_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "_ptr", lambda t: t)
    eng = _engine()
    z = torch.zeros
    mem, X, U, goal, gX, gc = z(3, 10), z(3, 4, 9, 5), z(4, 8, 2), z(4, 9, 5), z(3, 4, 9, 5), z(3, 4, 9)
    out = eng.ensemble_rollout_vjp(mem, X, U, goal, gX, gc)
    assert list(out) == ["x0", "U", "goal", "theta", "members"]
    assert [tuple(out[k].shape) for k in out] == [(4, 5), (4, 8, 2), (4, 9, 5), (10,), (3, 10)]
    (call,) = eng.lib.calls
    assert len(call) == len(ARGS) and call[:3] == ("ctx", 4, 3) and call[14] == "stream"
    assert call[4] is X and call[5] is U and call[6] is goal and call[7] is gX and call[8] is gc
    for i, k in enumerate(out):
        assert call[9 + i] is out[k]
    part = eng.ensemble_rollout_vjp(mem, X, U, goal, gcost=gc, want=("members", "U"))
    assert list(part) == ["U", "members"]
    call = eng.lib.calls[1]
    assert call[7] is None and call[8] is gc
    assert call[9] is None and call[10] is part["U"] and call[11] is None and call[12] is None
    assert call[13] is part["members"]
    lone = eng.ensemble_rollout_vjp(mem, X, U, goal, gX, want="x0")
    assert list(lone) == ["x0"]


# ---- H5 ------------------------------------------------------------------------------------------------------------
def test_h5_the_engine_refuses_before_the_library_is_called():
    eng = _engine()
    z = torch.zeros
    good = dict(members=z(3, 10), X=z(3, 4, 9, 5), U=z(4, 8, 2), goal=z(4, 9, 5), gX=z(3, 4, 9, 5), gcost=z(3, 4, 9))
    cases = [
        (dict(members=z(3, 11)), "members must be"),
        (dict(members=z(17, 10)), "P = 17"),
        (dict(members=z(0, 10)), "P = 0"),
        (dict(members=z(3, 10, dtype=torch.float64)), "float32"),
        (dict(want=("x0", "dyn")), "unknown entries"),
        (dict(want=()), "want is empty"),
        (dict(gX=None, gcost=None), "gX and gcost are both None"),
        (dict(X=z(2, 4, 9, 5)), "X must be (3, B, 9, 5)"),
        (dict(X=z(3, 4, 8, 5)), "X must be"),
        (dict(X=z(3, 4, 9, 5, dtype=torch.float64)), "X must be a float32 tensor"),
        (dict(U=z(3, 8, 2)), "U must be (4, 8, 2)"),
        (dict(U=z(4, 7, 2)), "U must be"),
        (dict(U=np.zeros((4, 8, 2), np.float32)), "U must be a float32 tensor"),
        (dict(goal=z(4, 8, 5)), "goal must be"),
        (dict(gX=z(3, 4, 9, 4)), "gX must be"),
        (dict(gcost=z(3, 4, 8)), "gcost must be (3, 4, 9)"),
        (dict(gcost=z(4, 9)), "gcost must be"),
    ]
    for change, msg in cases:
        with pytest.raises(GmpcError, match="ensemble rollout vjp: .*" + re.escape(msg)):
            eng.ensemble_rollout_vjp(**dict(good, **change))
    assert eng.lib.calls == []


def test_h5_the_policys_methods_and_the_layer_raise_without_an_ensemble():
    from gan_mpc_amd.policy import differentiable as dl
    from gan_mpc_amd.policy.base import BaseMPC
    policy = BaseMPC.__new__(BaseMPC)
    policy.dynamics_ensemble = None
    x, U, goal = np.zeros((2, 5), np.float32), np.zeros((2, 8, 2), np.float32), np.zeros((2, 9, 5), np.float32)
    with pytest.raises(ValueError, match="plan_risk needs a dynamics_ensemble"):
        policy.plan_risk(None, x, U, goal)
    with pytest.raises(ValueError, match="refine_plan needs a dynamics_ensemble"):
        policy.refine_plan(None, x, U, goal)
    policy.dynamics_ensemble = np.zeros((2, 10), np.float32)
    with pytest.raises(ValueError, match="plan_risk: aggregate must be one of"):
        policy.plan_risk(None, x, U, goal, aggregate="cvar")
    with pytest.raises(ValueError, match="plan_risk: x must be"):
        policy.plan_risk(None, x[0], U, goal)
    with pytest.raises(ValueError, match="refine_plan: x must be"):
        policy.refine_plan(None, x, U, goal[:1])
    assert callable(dl.ensemble_rollout_layer)
