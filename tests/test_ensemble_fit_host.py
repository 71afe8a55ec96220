"""The ensemble fit without a GPU (gmpc_dynamics_ensemble_loss_grad): the entry point's
declaration, binding and argument order (H1), every Engine, trainer and policy refusal, raised before any library call
(H2), the trainer's host pieces -- trees, index tensors (H3) -- and the trainer's schedule on the fp64 oracle with a
NumPy clip+Adam: the reference alone meets the condition the GPU test F8 asserts, with the same updates and rate (H4)."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ensemble_fit_cases as fc
import gan_mpc_oracle as orc
import sampled_ensemble_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ctx", "P", "dyn_members", "D", "B", "S", "xseq", "useq", "next_xseq", "rows", "discount", "teacher_forcing",
        "loss_sum", "grad_sum", "stream"]


# ---- H1 ------------------------------------------------------------------------------------------------------------
def test_h1_the_entry_point_is_declared_and_bound():
    from gan_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    m = re.search(r"\bint\s+gmpc_dynamics_ensemble_loss_grad\s*\(([^)]*)\)\s*;", header)
    assert m
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in decl] == ARGS
    kinds = [C.c_void_p if "*" in a else C.c_double if a.startswith("double") else C.c_int for a in decl]
    assert _lib.SIGNATURES["gmpc_dynamics_ensemble_loss_grad"] == (C.c_int, kinds)
    assert decl[9] == "const int* rows" and decl[2] == "const float* dyn_members"


class _Lib:
    def __init__(self):
        self.calls = []

    def gmpc_dynamics_ensemble_loss_grad(self, *args):
        self.calls.append(args)
        return 0


def _engine(n=5, m=2, dyn_count=10):
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.dyn_count, eng.n, eng.m, eng.device = _Lib(), "ctx", dyn_count, n, m, "cpu"
    eng._stream = lambda: "stream"
    eng.to_dev = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    return eng


def _good(P=3, D=6, S=4, n=5, m=2, dyn_count=10):
    z = lambda *s: torch.zeros(*s)
    return dict(members=z(P, dyn_count), xseq=z(D, S, n), useq=z(D, S, m), next_xseq=z(D, S, n))


def test_h1_the_engine_passes_the_arguments_in_the_headers_order():
    import gan_mpc_amd.engine as engine_mod
    eng = _engine()
    a = _good()
    rows = np.array([[0, 5, 5], [1, 2, 3], [4, 4, 4]], np.int32)      # P = 3, B = 3
    real = engine_mod._ptr
    engine_mod._ptr = lambda t: None if t is None else ("ptr", t.data_ptr())
    try:
        loss, grad = eng.dynamics_ensemble_loss_grad(a["members"], a["xseq"], a["useq"], a["next_xseq"], 0.9, True,
                                                     rows=rows)
        eng.dynamics_ensemble_loss_grad(a["members"], a["xseq"], a["useq"], a["next_xseq"], 0.9, False)
    finally:
        engine_mod._ptr = real
    p = lambda t: ("ptr", t.data_ptr())
    first, second = eng.lib.calls
    assert first[:9] == ("ctx", 3, p(a["members"]), 6, 3, 4, p(a["xseq"]), p(a["useq"]), p(a["next_xseq"]))
    assert first[9] is not None and first[10:12] == (0.9, 1) and first[12:] == (p(loss), p(grad), "stream")
    assert tuple(loss.shape) == (3,) and tuple(grad.shape) == (3, 10)
    assert second[3:6] == (6, 6, 4) and second[9] is None and second[11] == 0        # rows = None: D = B, the identity
    assert len(first) == len(ARGS)


# ---- H2 ------------------------------------------------------------------------------------------------------------
def _bad_engine_calls():
    z = lambda *s: torch.zeros(*s)
    i32 = lambda a: np.asarray(a, np.int32)
    return {
        "members rank": dict(members=z(10)),
        "members width": dict(members=z(3, 9)),
        "members dtype": dict(members=z(3, 10).double()),
        "members array": dict(members=np.zeros((3, 10), np.float32)),
        "P0": dict(members=z(0, 10)),
        "P17": dict(members=z(17, 10)),
        "xseq rank": dict(xseq=z(6, 5)),
        "xseq width": dict(xseq=z(6, 4, 4)),
        "useq width": dict(useq=z(6, 4, 3)),
        "useq steps": dict(useq=z(6, 3, 2)),
        "next_xseq rows": dict(next_xseq=z(5, 4, 5)),
        "xseq dtype": dict(xseq=z(6, 4, 5).double()),
        "rows rank": dict(rows=i32([0, 1, 2])),
        "rows members": dict(rows=i32([[0, 1], [2, 3]])),
        "rows dtype": dict(rows=np.zeros((3, 2), np.int64)),
        "rows negative": dict(rows=i32([[0, 1], [2, -1], [0, 0]])),
        "rows past D": dict(rows=i32([[0, 1], [2, 6], [0, 0]])),
        "rows past D, tensor": dict(rows=torch.tensor([[0, 1], [2, 6], [0, 0]], dtype=torch.int32)),
        "loss_sum shape": dict(loss_sum=z(1)),
        "grad_sum shape": dict(grad_sum=z(10)),
    }


@pytest.mark.parametrize("what", list(_bad_engine_calls()))
def test_h2_the_engine_refuses_before_the_library(what):
    from gan_mpc_amd._lib import GmpcError
    eng = _engine()
    kw = dict(_good(), discount=0.9, teacher_forcing=True)
    kw.update(_bad_engine_calls()[what])
    with pytest.raises(GmpcError, match="^ensemble fit: "):
        eng.dynamics_ensemble_loss_grad(**kw)
    assert eng.lib.calls == []


class _NoEnginePolicy:
    """A policy whose engine must not be asked for: the trainer's refusals come first."""
    _bound = True

    def device(self):
        return torch.device("cpu")

    def engine_for(self, *a, **k):
        raise AssertionError("the trainer reached the engine")


def test_h2_the_trainer_refuses_before_the_engine(monkeypatch):
    from gan_mpc_amd import optim, parallel
    from gan_mpc_amd.norm import ensemble_trainer as et
    X, U, Y = fc.train_dataset()
    args = ((_NoEnginePolicy(), optim.ClipAdam(1e-2)), None)
    tail = (2, 16, 0.95, 0.5, 0, 0)
    mem = torch.zeros(3, 10)
    for bad_members in (torch.zeros(10), torch.zeros(0, 10), torch.zeros(17, 10), np.zeros((3, 10), np.float32)):
        with pytest.raises(ValueError, match="^ensemble trainer: "):
            et.train_params(*args, bad_members, (X, U, Y), *tail)
    for bad_data in ((X, U), (X, U, Y[:, :3]), (X, U[:5], Y), (X[0], U[0], Y[0])):
        with pytest.raises(ValueError, match="^ensemble trainer: "):
            et.train_params(*args, mem, bad_data, *tail)
    with pytest.raises(ValueError, match="^ensemble trainer: batch_size"):
        et.train_params(*args, mem, (X, U, Y), 2, 0, 0.95, 0.5, 0, 0)
    with pytest.raises(ValueError, match="^ensemble trainer: opt_state"):
        et.train_params(args[0], [{}], mem, (X, U, Y), *tail)
    unbound = _NoEnginePolicy()
    unbound._bound = None
    with pytest.raises(ValueError, match="^ensemble trainer: bind the policy"):
        et.train_params((unbound, args[0][1]), None, mem, (X, U, Y), *tail)
    for P in (0, 17, 2.5):
        with pytest.raises(ValueError, match="^ensemble trainer: P"):
            et.init_members(_NoEnginePolicy(), (0, 2), P, 0)
    # fewer windows than a batch: nothing to do, as dynamics_trainer.train_params
    out = et.train_params(*args, mem, (X[:4], U[:4], Y[:4]), *tail)
    assert out[0] is mem and len(out[1]) == 3 and out[2].shape == (0, 3)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="one rank"):
        et.train_params(*args, mem, (X, U, Y), *tail)


class _Eng:
    device = torch.device("cpu")

    def __init__(self):
        self.sets = []

    def to_dev(self, a):
        return torch.as_tensor(np.ascontiguousarray(a))

    def set_sampled_ensemble(self, members):
        self.sets.append(members)


def test_h2_the_policy_method_follows_the_constructors_rule():
    from gan_mpc_amd import params as P
    from gan_mpc_amd.gan.js_policy import JS_MPC
    from gan_mpc_amd.norm.l2_policy import L2MPC
    from gan_mpc_amd.policy.base import BaseMPC
    from gan_mpc_amd.policy.eval import EvalMPC
    trees = [P.layers_to_tree(layers) for layers in ec.members("base")]
    flat = ec.flat(ec.members("base"))
    for solver, more in (("rounds", {}), ("fused", {}), ("box", dict(control_bounds=(-1.0, 1.0)))):
        p = EvalMPC(None, None, None, None, solver=solver, **more)
        with pytest.raises(ValueError, match="dynamics_ensemble"):
            p.set_dynamics_ensemble(trees)
        p.set_dynamics_ensemble(None)                                 # nothing to take away: allowed
    kw = dict(solver="icem", control_bounds=(-1.0, 1.0))
    for cls, args in ((EvalMPC, (None,) * 4), (BaseMPC, (None,) * 4), (L2MPC, (None,) * 4), (JS_MPC, (None,) * 5)):
        p = cls(*args, **kw)
        for bad in ([], np.zeros(10, np.float32), np.zeros((0, 10), np.float32), np.zeros((17, 10), np.float32),
                    np.zeros((2, 10), np.float64), torch.zeros(2, 10, dtype=torch.float64)):
            with pytest.raises(ValueError, match="dynamics_ensemble"):
                p.set_dynamics_ensemble(bad)
        assert p.dynamics_ensemble is None
        for given in (trees, tuple(trees), flat, torch.as_tensor(flat)):
            p.set_dynamics_ensemble(given)                            # no engine yet: kept for the next bind
            np.testing.assert_array_equal(p.dynamics_ensemble, flat)
            assert p._ensemble_dev is None
        p._engine = _Eng()
        p.set_dynamics_ensemble(flat[:2])                             # replaces the stored one, and sets it at once
        np.testing.assert_array_equal(p._engine.sets[-1].numpy(), flat[:2])
        assert p.dynamics_ensemble.shape == (2, flat.shape[1])
        p.set_dynamics_ensemble(None)
        assert p._engine.sets[-1] is None and p.dynamics_ensemble is None and p._ensemble_dev is None


# ---- H3 ------------------------------------------------------------------------------------------------------------
def test_h3_members_round_trip_through_trees():
    from gan_mpc_amd import params as P
    from gan_mpc_amd.norm import ensemble_trainer as et
    flat = ec.flat(ec.members("ragged"))
    like = P.layers_to_tree(ec.problem("ragged")["dyn"])
    for given in (flat, torch.as_tensor(flat)):
        trees = et.members_to_trees(given, like)
        assert len(trees) == 3 and list(trees[0]["params"]) == list(like["params"])
        np.testing.assert_array_equal(np.stack([P.pack_mlp(t) for t in trees]), flat)
        for k, layer in like["params"].items():
            assert trees[1]["params"][k]["kernel"].shape == np.shape(layer["kernel"])
    with pytest.raises(ValueError, match="^ensemble trainer: members"):
        et.members_to_trees(flat[:, :-1], like)


def test_h3_the_index_tensor():
    from gan_mpc_amd.norm import ensemble_trainer as et
    idx = et.draw_indices(np.random.default_rng(1), 64, 4, 3, 16, True)
    assert idx.shape == (4, 3, 16) and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < 64
    assert idx.flags["C_CONTIGUOUS"] and not np.array_equal(idx[:, 0], idx[:, 1])
    np.testing.assert_array_equal(idx, np.random.default_rng(1).choice(64, size=(4, 3, 16)))      # one draw
    one = et.draw_indices(np.random.default_rng(1), 64, 4, 3, 16, False)
    assert one.shape == (4, 3, 16) and one.dtype == np.int32 and one.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(one[:, 0], one[:, 1])
    np.testing.assert_array_equal(one[:, 0], one[:, 2])
    np.testing.assert_array_equal(one[:, 0], np.random.default_rng(1).choice(64, size=(4, 16)))


# ---- H4 ------------------------------------------------------------------------------------------------------------
def _adam(p, g, m, v, count, lr, max_norm, b1, b2, eps):
    """optax.chain(clip_by_global_norm(max_norm), adam(lr)) on one flat vector, fp64."""
    norm = np.sqrt(np.sum(g * g))
    if not norm < max_norm:
        g = g / norm * max_norm
    m[:] = b1 * m + (1 - b1) * g
    v[:] = b2 * v + (1 - b2) * g * g
    p += -lr * (m / (1 - b1 ** count)) / (np.sqrt(v / (1 - b2 ** count)) + eps)


def test_h4_the_schedule_lowers_every_members_loss_on_the_reference():
    from gan_mpc_amd import trainer_common as tc
    from gan_mpc_amd.norm import ensemble_trainer as et
    t = fc.TRAIN
    X, U, Y = (a.astype(np.float64) for a in fc.train_dataset())
    assert X.shape == (t["windows"], t["S"], t["n"]) and np.array_equal(X[:, 1:], Y[:, :-1])
    dims = fc.train_dims()
    members = fc.students().astype(np.float64)
    P_, steps = t["P"], t["windows"] // t["batch_size"]
    m, v, count = np.zeros_like(members), np.zeros_like(members), 0
    rng = tc.as_rng(t["key"])
    losses = np.zeros((t["num_updates"], P_))
    for up in range(1, t["num_updates"] + 1):
        idx = et.draw_indices(rng, t["windows"], steps, P_, t["batch_size"], True)
        tf = up <= t["num_updates"] * t["teacher_forcing_factor"]
        for s in range(steps):
            count += 1
            for p in range(P_):
                layers = _unrounded(members[p], dims)
                r = idx[s, p]
                loss, g = orc.dynamics_fit_loss_and_grad(layers, X[r], U[r], Y[r], fc.DISCOUNT, tf)
                losses[up - 1, p] += loss / steps
                _adam(members[p], fc.flat_grad(g), m[p], v[p], count, t["lr"], **fc.ADAM)
    print("H4 losses, first and last update:", losses[0], losses[-1])
    assert np.all(np.isfinite(losses)) and np.all(losses[-1] < losses[0])


def _unrounded(flat, dims):
    """The layers of a flat fp64 vector, kept in fp64 (params.unpack_mlp rounds to fp32)."""
    out, off = [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        out.append((flat[off:off + a * b].reshape(a, b), flat[off + a * b:off + a * b + b]))
        off += a * b + b
    return out
