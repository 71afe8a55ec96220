"""The closed-loop ensemble rollout without a GPU (gmpc_ensemble_rollout_feedback): the entry
point's declaration, binding and the Engine's argument order (H1); the NumPy reference against the oracle's ddp_rollout
-- an independent transcription of trajax's forward pass -- under every member, against the open-loop reference with
K = 0, and what the clamp and x0 do to it (H2); every Engine refusal and the policy's, raised before the library is
called (H3)."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ensemble_feedback_ref as fr
import ensemble_rollout_ref as rr
import gan_mpc_oracle as orc
import sampled_ensemble_cases as ec
from gan_mpc_amd._lib import GmpcError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ctx", "B", "S", "P", "dyn_members", "x0", "X_ref", "U_ref", "K", "k", "alpha", "u_lo", "u_hi", "goal", "X",
        "U", "costs", "obj", "x_mean", "x_var", "stream"]


# ---- H1 ------------------------------------------------------------------------------------------------------------
def test_h1_the_entry_point_is_declared_and_bound():
    from gan_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    m = re.search(r"\bint\s+gmpc_ensemble_rollout_feedback\s*\(([^)]*)\)\s*;", header)
    assert m
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in decl] == ARGS
    kinds = [C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int for a in decl]
    assert kinds.count(C.c_float) == 1 and kinds[ARGS.index("alpha")] is C.c_float
    assert _lib.SIGNATURES["gmpc_ensemble_rollout_feedback"] == (C.c_int, kinds)


class _Lib:
    def __init__(self):
        self.calls = []

    def gmpc_ensemble_rollout_feedback(self, *args):
        self.calls.append(args)
        return 0


def _engine(n=5, m=2, T=8, dyn_count=10, max_batch=4):
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.dyn_count, eng.n, eng.m, eng.T, eng.device = _Lib(), "ctx", dyn_count, n, m, T, "cpu"
    eng.max_batch = max_batch
    eng._stream = lambda: "stream"
    eng.to_dev = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    eng.new = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)
    return eng


def _good():
    z = torch.zeros
    return dict(members=z(3, 10), X_ref=z(4, 9, 5), U_ref=z(4, 8, 2), K=z(4, 8, 2, 5), goal=z(4, 9, 5))


def test_h1_the_engine_passes_the_arguments_in_the_headers_order(monkeypatch):
    import gan_mpc_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "_ptr", lambda t: t)
    eng = _engine()
    a = _good()
    x0, k = torch.zeros(4, 5), torch.zeros(4, 8, 2)
    out = eng.ensemble_rollout_feedback(a["members"], a["X_ref"], a["U_ref"], a["K"], a["goal"], x0=x0, k=k, alpha=0.25,
                                        u_lo=-1.0, u_hi=[1.0, 2.0], want=("var", "obj", "U", "X"))
    assert list(out) == ["X", "U", "obj", "var"]
    assert tuple(out["X"].shape) == (3, 4, 9, 5) and tuple(out["U"].shape) == (3, 4, 8, 2)
    assert tuple(out["obj"].shape) == (3, 4) and tuple(out["var"].shape) == (4, 9, 5)
    (call,) = eng.lib.calls
    assert len(call) == len(ARGS)
    got = dict(zip(ARGS, call))
    assert (got["ctx"], got["B"], got["S"], got["P"], got["stream"]) == ("ctx", 4, 8, 3, "stream")
    assert got["x0"] is x0 and got["X_ref"] is a["X_ref"] and got["U_ref"] is a["U_ref"] and got["K"] is a["K"]
    assert got["k"] is k and got["alpha"] == 0.25 and isinstance(got["alpha"], float) and got["goal"] is a["goal"]
    assert got["u_lo"].tolist() == [-1.0, -1.0] and got["u_hi"].tolist() == [1.0, 2.0]
    assert got["X"] is out["X"] and got["U"] is out["U"] and got["costs"] is None and got["obj"] is out["obj"]
    assert got["x_mean"] is None and got["x_var"] is out["var"]
    # the defaults: no x0, no k, no bounds, the goal unread; S from U_ref, a lone key as a string
    short = eng.ensemble_rollout_feedback(a["members"], a["X_ref"][:, :4].contiguous(), a["U_ref"][:, :3].contiguous(),
                                          a["K"][:, :3].contiguous(), want="U")
    assert list(short) == ["U"] and tuple(short["U"].shape) == (3, 4, 3, 2)
    got = dict(zip(ARGS, eng.lib.calls[1]))
    assert got["S"] == 3 and got["alpha"] == 1.0
    assert all(got[key] is None for key in ("x0", "k", "u_lo", "u_hi", "goal", "X", "costs", "obj", "x_mean", "x_var"))
    assert eng.ensemble_rollout_feedback.__defaults__ == (None, None, None, 1.0, None, None, ("X", "U", "obj"))


# ---- H2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "ragged", "cheetah"])
def test_h2_the_reference_is_trajax_forward_pass_under_every_member(name):
    pb, members = ec.problem(name), ec.members(name)
    X_ref, K, k, _, _ = fr.gains_at(pb)
    B = pb["B"]
    a64 = fr.cast_inputs(np.float64, X_ref=X_ref, U_ref=pb["U"], K=K, k=k)
    for alpha in (0.5, 1.0):
        r64 = fr.rollout(pb, members, a64["X_ref"], a64["U_ref"], a64["K"], k=a64["k"], alpha=alpha)
        r32 = fr.rollout(pb, members, X_ref, pb["U"], K, k=k, alpha=alpha)
        assert r64["X"].dtype == np.float64 and r32["X"].dtype == np.float32 and r32["U"].dtype == np.float32
        for p, layers in enumerate(members):
            dyn = [(W.astype(np.float64), b.astype(np.float64)) for W, b in layers]
            Xd, Ud = orc.ddp_rollout(dyn, a64["X_ref"], a64["U_ref"], a64["K"], a64["k"], np.full(B, alpha))
            np.testing.assert_allclose(r64["X"][p], Xd, rtol=1e-11, atol=1e-12)
            np.testing.assert_allclose(r64["U"][p], Ud, rtol=1e-11, atol=1e-12)
            np.testing.assert_allclose(r32["X"][p], Xd, rtol=1e-3, atol=1e-4)
            costs = orc.evaluate(orc.cast_problem(pb, np.float64)["cmlp"], pb["mpc_w"].astype(np.float64),
                                 pb["goal"].astype(np.float64), Xd, Ud)
            np.testing.assert_allclose(r64["costs"][p], costs, rtol=1e-11, atol=1e-12)
            np.testing.assert_allclose(r64["obj"][p], costs.sum(1), rtol=1e-11, atol=1e-12)
    # the feedback is there: without k the members still leave the open-loop rollout, and they differ
    fb = fr.rollout(pb, members, a64["X_ref"], a64["U_ref"], a64["K"])
    ol = rr.rollout(orc.cast_problem(pb, np.float64), members)
    assert np.abs(fb["X"] - ol["X"]).max() > 1e-4 * np.abs(ol["X"]).max()
    assert np.abs(fb["U"][0] - fb["U"][1]).max() > 1e-4 * np.abs(fb["U"]).max()


@pytest.mark.parametrize("name", ["base", "ragged"])
def test_h2_without_gains_the_reference_is_the_open_loop_reference(name):
    pb, members = ec.problem(name), ec.members(name)
    X_ref, K, _, _, _ = fr.gains_at(pb)
    x0 = fr.perturbed_x0(pb, 0.1)
    for dt in (np.float32, np.float64):
        a = fr.cast_inputs(dt, X_ref=X_ref, U_ref=pb["U"], K=np.zeros_like(K), x0=x0)
        fb = fr.rollout(pb, members, a["X_ref"], a["U_ref"], a["K"], x0=a["x0"])
        ol = rr.rollout(dict(orc.cast_problem(pb, dt), x0=a["x0"]), members)
        np.testing.assert_array_equal(fb["X"], ol["X"])
        np.testing.assert_array_equal(fb["U"], np.broadcast_to(a["U_ref"], fb["U"].shape))
        np.testing.assert_array_equal(fb["costs"], ol["costs"])
        np.testing.assert_allclose(fb["obj"], ol["obj"], rtol=1e-6 if dt is np.float32 else 1e-14)
    short = fr.rollout(pb, members, X_ref[:, :4], pb["U"][:, :3], K[:, :3], x0=x0)
    whole = fr.rollout(pb, members, X_ref, pb["U"], K, x0=x0)
    assert set(short) == {"X", "U"}
    np.testing.assert_array_equal(short["X"], whole["X"][:, :, :4])
    np.testing.assert_array_equal(short["U"], whole["U"][:, :, :3])


def test_h2_the_clamp_and_the_start():
    name = "base"
    pb, members = ec.problem(name), ec.members(name)
    X_ref, K, k, _, _ = fr.gains_at(pb)
    x0 = fr.perturbed_x0(pb, 0.02)
    free = fr.rollout(pb, members, X_ref, pb["U"], K, x0=x0)
    tight = fr.rollout(pb, members, X_ref, pb["U"], K, x0=x0, lo=-1.0, hi=1.0)
    loose = fr.rollout(pb, members, X_ref, pb["U"], K, x0=x0, lo=-1e30, hi=1e30)
    for key in free:
        np.testing.assert_array_equal(free[key], loose[key])
    assert np.abs(free["U"]).max() > 1 and np.abs(tight["U"]).max() == 1
    at = np.abs(tight["U"]) == 1
    assert 0.02 < at.mean() < 0.5
    # up to its first saturated step a (member, problem) pair is the unclamped run
    first = np.where(at.any(-1), np.arange(at.shape[2]), at.shape[2]).min(-1)
    for p, b in np.ndindex(first.shape):
        np.testing.assert_array_equal(tight["X"][p, b, :first[p, b] + 1], free["X"][p, b, :first[p, b] + 1])
    np.testing.assert_array_equal(free["X"][:, :, 0], np.broadcast_to(x0, free["X"][:, :, 0].shape))
    default = fr.rollout(pb, members, X_ref, pb["U"], K)
    np.testing.assert_array_equal(default["X"][:, :, 0], np.broadcast_to(pb["x0"], default["X"][:, :, 0].shape))
    # a member that reproduces the reference gets the reference's controls back: the nominal network
    own = fr.rollout(pb, [pb["dyn"]], X_ref, pb["U"], K)
    np.testing.assert_array_equal(own["X"][0], X_ref)
    np.testing.assert_array_equal(own["U"][0], pb["U"])


# ---- H3 ------------------------------------------------------------------------------------------------------------
def test_h3_the_engine_refuses_before_the_library_is_called(monkeypatch):
    import gan_mpc_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "_ptr", lambda t: t)         # (the accepted neighbours reach the fake library)
    eng = _engine()
    z = torch.zeros
    cases = [
        (dict(members=z(3, 11)), "members must be"),
        (dict(members=z(17, 10)), "P = 17"),
        (dict(members=z(0, 10)), "P = 0"),
        (dict(members=z(3, 10, dtype=torch.float64)), "float32"),
        (dict(want=("X", "spread")), "unknown entries"),
        (dict(want=()), "want is empty"),
        (dict(goal=None), '"costs" and "obj" need goal'),              # the default want asks for obj
        (dict(goal=None, want=("costs",)), '"costs" and "obj" need goal'),
        (dict(X_ref=None), "X_ref must not be None"),
        (dict(U_ref=None), "U_ref must not be None"),
        (dict(K=None), "K must not be None"),
        (dict(X_ref=z(4, 9, 5, dtype=torch.float64)), "X_ref must be a float32 tensor"),
        (dict(K=np.zeros((4, 8, 2, 5), np.float32)), "K must be a float32 tensor"),
        (dict(U_ref=z(4, 8, 3)), "U_ref must be"),
        (dict(U_ref=z(4, 8)), "U_ref must be"),
        (dict(X_ref=z(4, 8, 5)), "X_ref must be"),
        (dict(X_ref=z(3, 9, 5)), "X_ref must be"),
        (dict(K=z(4, 8, 5, 2)), "K must be"),
        (dict(goal=z(4, 8, 5)), "goal must be"),
        (dict(x0=z(4, 6)), "x0 must be"),
        (dict(x0=z(5, 4).t()), "x0 must be contiguous"),
        (dict(k=z(4, 8, 3)), "k must be"),
        (dict(k=z(4, 8, 2, dtype=torch.float64)), "k must be a float32 tensor"),
        (dict(alpha=float("nan")), "alpha must be a finite number"),
        (dict(alpha=float("inf")), "alpha must be a finite number"),
        (dict(alpha="half"), "alpha must be a finite number"),
        (dict(u_lo=-1.0), "u_lo and u_hi must both be given"),
        (dict(u_hi=1.0), "u_lo and u_hi must both be given"),
        (dict(u_lo=1.0, u_hi=-1.0), "u_lo must be <= u_hi"),
        (dict(u_lo=[0.0, 0.0, 0.0], u_hi=1.0), "u_lo must be a scalar or 2 values"),
        (dict(u_lo=float("nan"), u_hi=1.0), "NaN"),
        (dict(X_ref=z(5, 9, 5), U_ref=z(5, 8, 2), K=z(5, 8, 2, 5), goal=z(5, 9, 5)), "B = 5 outside"),
        (dict(X_ref=z(4, 10, 5), U_ref=z(4, 9, 2), K=z(4, 9, 2, 5)), "S = 9 outside"),
        (dict(X_ref=z(4, 4, 5), U_ref=z(4, 3, 2), K=z(4, 3, 2, 5)), "S = 3 is not T = 8"),
        (dict(X_ref=z(4, 4, 5), U_ref=z(4, 3, 2), K=z(4, 3, 2, 5), want=("X", "costs")), "S = 3 is not T = 8"),
    ]
    for change, msg in cases:
        with pytest.raises(GmpcError, match="^ensemble feedback: .*" + re.escape(msg)):
            eng.ensemble_rollout_feedback(**dict(_good(), **change))
    assert eng.lib.calls == []
    # the accepted neighbours
    eng.ensemble_rollout_feedback(**dict(_good(), X_ref=z(4, 4, 5), U_ref=z(4, 3, 2), K=z(4, 3, 2, 5), want=("X", "U")))
    eng.ensemble_rollout_feedback(**dict(_good(), u_lo=-float("inf"), u_hi=1.0, alpha=0))
    assert len(eng.lib.calls) == 2


def test_h3_closed_loop_spread_raises_the_policys_errors_before_anything_is_bound():
    from gan_mpc_amd.policy.base import BaseMPC
    policy = BaseMPC.__new__(BaseMPC)
    policy.dynamics_ensemble = None
    x, U, goal = np.zeros((2, 5), np.float32), np.zeros((2, 8, 2), np.float32), np.zeros((2, 9, 5), np.float32)
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        policy.closed_loop_spread(None, x, U, goal)
    with pytest.raises(ValueError, match="closed_loop_spread: members must hold at least one"):
        policy.closed_loop_spread(None, x, U, goal, members=[])
    policy.dynamics_ensemble = np.zeros((2, 10), np.float32)
    with pytest.raises(ValueError, match="closed_loop_spread: x must be"):
        policy.closed_loop_spread(None, x[0], U, goal)
    with pytest.raises(ValueError, match="closed_loop_spread: x must be"):
        policy.closed_loop_spread(None, x, U, goal[:1])
    with pytest.raises(ValueError, match="closed_loop_spread: x0 must be"):
        policy.closed_loop_spread(None, x, U, goal, x0=np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError, match="closed_loop_spread: x must be"):
        policy.closed_loop_spread(None, x, U[:1], goal, members=np.zeros((2, 10), np.float32))
