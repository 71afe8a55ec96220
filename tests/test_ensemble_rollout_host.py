"""The ensemble rollout without a GPU (gmpc_ensemble_rollout): the entry point's declaration,
binding and argument order (H1); the NumPy reference against an independent sample-by-sample loop in fp64, and its
moments against np.mean / np.var (H2); elite_members' order and ties (H3); holdout_errors' chunking on a fake engine
(H4); every Engine, trainer and policy refusal that is raised before the library is called (H5)."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ensemble_rollout_ref as rr
import gan_mpc_oracle as orc
import sampled_ensemble_cases as ec
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.norm import ensemble_trainer as et

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ctx", "B", "S", "P", "dyn_members", "x0", "U", "goal", "X", "costs", "obj", "x_mean", "x_var", "stream"]


# ---- H1 ------------------------------------------------------------------------------------------------------------
def test_h1_the_entry_point_is_declared_and_bound():
    from gan_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    m = re.search(r"\bint\s+gmpc_ensemble_rollout\s*\(([^)]*)\)\s*;", header)
    assert m
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in decl] == ARGS
    kinds = [C.c_void_p if "*" in a else C.c_int for a in decl]
    assert _lib.SIGNATURES["gmpc_ensemble_rollout"] == (C.c_int, kinds)


class _Lib:
    def __init__(self):
        self.calls = []

    def gmpc_ensemble_rollout(self, *args):
        self.calls.append(args)
        return 0


def _engine(n=5, m=2, T=8, dyn_count=10):
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.dyn_count, eng.n, eng.m, eng.T, eng.device = _Lib(), "ctx", dyn_count, n, m, T, "cpu"
    eng._stream = lambda: "stream"
    eng.to_dev = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    eng.new = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)
    return eng


def test_h1_the_engine_passes_the_arguments_in_the_headers_order(monkeypatch):
    import gan_mpc_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "_ptr", lambda t: t)
    eng = _engine()
    z = torch.zeros
    mem, x0, U, goal = z(3, 10), z(4, 5), z(4, 8, 2), z(4, 9, 5)
    out = eng.ensemble_rollout(mem, x0, U, goal, want=("obj", "var", "X"))
    assert list(out) == ["X", "obj", "var"]
    assert tuple(out["X"].shape) == (3, 4, 9, 5) and tuple(out["obj"].shape) == (3, 4)
    assert tuple(out["var"].shape) == (4, 9, 5)
    (call,) = eng.lib.calls
    assert call[:4] == ("ctx", 4, 8, 3) and call[13] == "stream"
    assert call[5] is x0 and call[6] is U and call[7] is goal
    assert call[8] is out["X"] and call[9] is None and call[10] is out["obj"] and call[11] is None
    assert call[12] is out["var"]
    short = eng.ensemble_rollout(mem, x0, U[:, :3].contiguous(), want="X")        # S from U, a lone key as a string
    assert tuple(short["X"].shape) == (3, 4, 4, 5) and eng.lib.calls[1][2] == 3 and eng.lib.calls[1][7] is None


# ---- H2 ------------------------------------------------------------------------------------------------------------
def _plain_loop(pb, members):
    """Sample by sample, step by step, in fp64: nothing shared with the oracle but the constants."""
    pb = orc.cast_problem(pb, np.float64)
    w = 1.0 / (1.0 + np.exp(-pb["mpc_w"]))
    a = float(orc.ALPHA)
    B, T, _ = pb["U"].shape
    n = pb["x0"].shape[1]

    def mlp(layers, q):
        for W, b in layers[:-1]:
            q = np.maximum(q @ W.astype(np.float64) + b.astype(np.float64), 0.0)
        W, b = layers[-1]
        return q @ W.astype(np.float64) + b.astype(np.float64)

    X = np.zeros((len(members), B, T + 1, n))
    costs = np.zeros((len(members), B, T + 1))
    for p, layers in enumerate(members):
        for b in range(B):
            x = pb["x0"][b]
            for t in range(T):
                u = pb["U"][b, t]
                X[p, b, t] = x
                costs[p, b, t] = (w[0] * (np.sqrt(u @ u + a * a) - a)
                                  + w[1] * (np.sqrt((x - pb["goal"][b, t]) @ (x - pb["goal"][b, t]) + a * a) - a))
                x = x + mlp(layers, np.concatenate([x, u]))
            X[p, b, T] = x
            y = mlp(pb["cmlp"], x)
            costs[p, b, T] = w[2] * (y @ y)
    return X, costs, costs.sum(-1)


@pytest.mark.parametrize("name", ["base", "ragged"])
def test_h2_the_reference_is_the_plain_loop(name):
    pb, members = ec.problem(name), ec.members(name)
    X, costs, obj = _plain_loop(pb, members)
    r64 = rr.rollout(orc.cast_problem(pb, np.float64), members)
    r32 = rr.rollout(pb, members)
    assert r32["X"].dtype == np.float32 and r64["obj"].dtype == np.float64
    for k, want in (("X", X), ("costs", costs), ("obj", obj)):
        assert r64[k].shape == want.shape
        np.testing.assert_allclose(r64[k], want, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(r32[k], want, rtol=2e-5, atol=1e-5)
    assert np.abs(X[0] - X[1]).max() > 1e-3 * np.abs(X).max()          # the members differ
    short = rr.rollout(pb, members, S=3)
    assert set(short) == {"X"}
    np.testing.assert_array_equal(short["X"], r32["X"][:, :, :4])


def test_h2_the_moments_are_numpys_in_fp64_and_exact_where_they_must_be():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((5, 3, 4, 2))
    mean, var = rr.moments(X)
    np.testing.assert_allclose(mean, X.mean(0), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(var, X.var(0), rtol=1e-13, atol=1e-15)            # ddof = 0: the population variance
    X32 = X.astype(np.float32)
    m32, v32 = rr.moments(X32)
    assert m32.dtype == np.float32 and v32.dtype == np.float32
    np.testing.assert_allclose(m32, X.mean(0), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v32, X.var(0), rtol=1e-5, atol=1e-6)
    one_m, one_v = rr.moments(X32[:1])
    np.testing.assert_array_equal(one_m, X32[0])
    assert not one_v.any()
    two_m, two_v = rr.moments(np.stack([X32[1], X32[1]]))
    np.testing.assert_array_equal(two_m, X32[1])
    assert not two_v.any()
    X32[2, 0, 0, 0] = np.nan
    bad_m, bad_v = rr.moments(X32)
    assert np.isnan(bad_m[0, 0, 0]) and np.isnan(bad_v[0, 0, 0]) and np.isfinite(bad_m).sum() == bad_m.size - 1


# ---- H3 ------------------------------------------------------------------------------------------------------------
def test_h3_elite_members_orders_by_the_summed_error_and_breaks_ties_downwards():
    e = np.array([[3.0, 1.0], [0.5, 0.5], [2.0, 2.0], [0.25, 0.75], [9.0, 0.0]], np.float32)
    assert et.elite_members(e, 5).tolist() == [1, 3, 0, 2, 4]                     # 1 and 3 tie at 1, 0 and 2 at 4
    assert et.elite_members(torch.as_tensor(e), 2).tolist() == [1, 3]
    got = et.elite_members(e, 1)
    assert got.dtype == torch.int64 and got.tolist() == [1]
    e[1, 0] = np.nan
    e[3, 1] = np.inf
    assert et.elite_members(e, 5).tolist() == [0, 2, 4, 1, 3]                     # non-finite last, in index order
    members = torch.arange(5.0)[:, None] * torch.ones(5, 3)
    assert members[et.elite_members(e, 2)][:, 0].tolist() == [0.0, 2.0]
    for k in (0, 6, 1.5, True):
        with pytest.raises(ValueError, match="ensemble trainer: k"):
            et.elite_members(e, k)
    with pytest.raises(ValueError, match="ensemble trainer: errors"):
        et.elite_members(e[0], 1)


# ---- H4 ------------------------------------------------------------------------------------------------------------
class _FakeEngine:
    """ensemble_rollout for linear members x' = x + a_p u.sum(): enough to see which rows each chunk was given."""

    def __init__(self, max_batch):
        self.max_batch = max_batch
        self.batches = []

    def ensemble_rollout(self, members, x0, U, goal=None, want=("X", "obj")):
        assert want == ("X",) and goal is None and x0.is_contiguous() and U.is_contiguous()
        assert x0.shape[0] == U.shape[0] <= self.max_batch
        self.batches.append(int(x0.shape[0]))
        X = [x0[None].expand(members.shape[0], -1, -1)]
        for t in range(U.shape[1]):
            X.append(X[-1] + members[:, :1, None] * U[None, :, t].sum(-1, keepdim=True))
        return dict(X=torch.stack(X, dim=2))


def test_h4_holdout_errors_chunks_by_max_batch_and_averages_over_all_rows():
    rng = np.random.default_rng(1)
    D, S, n, m, P = 11, 4, 3, 2, 3
    xseq = torch.as_tensor(rng.standard_normal((D, S, n)), dtype=torch.float32)
    useq = torch.as_tensor(rng.standard_normal((D, S, m)), dtype=torch.float32)
    nxt = torch.as_tensor(rng.standard_normal((D, S, n)), dtype=torch.float32)
    members = torch.as_tensor([[0.5], [1.0], [-2.0]])
    whole = _FakeEngine(16)
    want = whole.ensemble_rollout(members, xseq[:, 0].contiguous(), useq, want=("X",))["X"][:, :, 1:]
    want = ((want - nxt[None]).double() ** 2).mean(dim=(1, 3))
    e16 = et.holdout_errors(whole, members, xseq, useq, nxt)
    assert tuple(e16.shape) == (P, S) and e16.dtype == torch.float32 and whole.batches == [11, 11]
    np.testing.assert_allclose(e16.numpy(), want.numpy(), rtol=1e-6)
    for mb, batches in ((4, [4, 4, 3]), (11, [11]), (1, [1] * 11)):
        eng = _FakeEngine(mb)
        np.testing.assert_allclose(et.holdout_errors(eng, members, xseq, useq, nxt).numpy(), want.numpy(), rtol=1e-6)
        assert eng.batches == batches
    for bad in ((xseq[0], useq, nxt), (xseq, useq[:5], nxt), (xseq, useq, nxt[:, :2]), (xseq[:0], useq[:0], nxt[:0])):
        with pytest.raises(ValueError, match="ensemble trainer: holdout data"):
            et.holdout_errors(whole, members, *bad)


# ---- H5 ------------------------------------------------------------------------------------------------------------
def test_h5_the_engine_refuses_before_the_library_is_called():
    eng = _engine()
    z = torch.zeros
    good = dict(members=z(3, 10), x0=z(4, 5), U=z(4, 8, 2), goal=z(4, 9, 5))
    cases = [
        (dict(members=z(3, 11)), "members must be"),
        (dict(members=z(17, 10)), "P = 17"),
        (dict(members=z(0, 10)), "P = 0"),
        (dict(members=z(3, 10, dtype=torch.float64)), "float32"),
        (dict(want=("X", "spread")), "unknown entries"),
        (dict(want=()), "want is empty"),
        (dict(goal=None), '"costs" and "obj" need goal'),              # the default want asks for obj
        (dict(goal=None, want=("costs",)), '"costs" and "obj" need goal'),
        (dict(x0=z(4, 6)), "x0 must be"),
        (dict(x0=z(4, 5, dtype=torch.float64)), "x0 must be a float32 tensor"),
        (dict(U=z(3, 8, 2)), "U must be"),
        (dict(U=z(4, 8, 3)), "U must be"),
        (dict(U=np.zeros((4, 8, 2), np.float32)), "U must be a float32 tensor"),
        (dict(goal=z(4, 8, 5)), "goal must be"),
    ]
    for change, msg in cases:
        with pytest.raises(GmpcError, match="ensemble rollout: .*" + re.escape(msg)):
            eng.ensemble_rollout(**dict(good, **change))
    assert eng.lib.calls == []


def test_h5_plan_spread_raises_the_policys_error_without_an_ensemble():
    from gan_mpc_amd.policy.base import BaseMPC
    policy = BaseMPC.__new__(BaseMPC)
    policy.dynamics_ensemble = None
    with pytest.raises(ValueError, match="dynamics_ensemble"):
        policy.plan_spread(None, np.zeros((2, 5), np.float32), np.zeros((2, 8, 2), np.float32))
    policy.dynamics_ensemble = np.zeros((2, 10), np.float32)
    with pytest.raises(ValueError, match="plan_spread: x must be"):
        policy.plan_spread(None, np.zeros(5, np.float32), np.zeros((2, 8, 2), np.float32))
