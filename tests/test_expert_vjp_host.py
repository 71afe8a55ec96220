"""CPU side of gmpc_expert_vjp (the VJP of the expert sequence model's rollout): the torch reference the GPU tests use
(tests/expert_vjp_ref.py) against the oracle's forward, against central differences of it and against the training
loss's gradient (tests/expert_fit_ref.py); the structure of the backward pass; the ABI entry against the header and
_lib.SIGNATURES, the Engine method and the torch layer."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import expert_fit_ref as R
import expert_vjp_ref as V
import gan_mpc_oracle as orc
from gan_mpc_amd import _lib, params as P
from gan_mpc_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (x_size, m, F (0 = MLP variant), num_layers, num_hidden_units, B, hist, T)
CASES = {
    "lstm": (5, 3, 13, 2, 17, 3, 2, 4),
    "mlp": (4, 2, 0, 3, 19, 3, 2, 3),
    "lstm-hist1": (3, 1, 8, 3, 12, 2, 1, 5),
}


def _setup(name, seed=0):
    n, m, F, layers, hidden, B, hist, T = CASES[name]
    rng = np.random.default_rng(seed)
    ex = orc.make_expert(rng, n, m, lstm_features=F, num_layers=layers, num_hidden_units=hidden, dtype=np.float64)
    W, b = ex["head_x"][-1]
    ex["head_x"][-1] = (W * 0.3, b * 0.3)
    _, F_, dx, du = P.pack_expert(ex)
    flat = V.flat_of_tree(ex)
    history = rng.standard_normal((B, hist + 1, n))
    return ex, (flat, F_, dx, du), history, T


def _unflatten_np(flat, F, dx, du):
    import torch
    ex = R.unflatten(torch.as_tensor(flat), F, dx, du)
    out = {}
    if "lstm" in ex:
        out["lstm"] = {k: v.numpy() for k, v in ex["lstm"].items()}
    else:
        out["first"] = tuple(v.numpy() for v in ex["first"])
    for key in ("head_x", "head_u"):
        out[key] = [(W.numpy(), b.numpy()) for W, b in ex[key]]
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_reference_forward_is_the_oracles(name):
    ex, model, history, T = _setup(name)
    goal, U = V.forward(*model, history, T)
    g64, u64 = orc.expert_goal_states_init_actions(ex, history, T)
    assert g64.dtype == np.float64
    assert np.abs(goal - g64).max() <= 1e-12 and np.abs(U - u64).max() <= 1e-12
    # the flat vector is pack_expert's order
    flat32 = P.pack_expert(ex)[0]
    np.testing.assert_array_equal(flat32, model[0].astype(np.float32))


@pytest.mark.parametrize("name", list(CASES))
def test_reference_matches_central_differences(name):
    ex, model, history, T = _setup(name, seed=1)
    flat, F, dx, du = model
    rng = np.random.default_rng(2)
    goal, U = V.forward(*model, history, T)
    g_goal, g_U = rng.standard_normal(goal.shape), rng.standard_normal(U.shape)
    gp, gh = V.vjp(*model, history, T, g_goal, g_U)

    def L(v, hx):
        g, u = orc.expert_goal_states_init_actions(_unflatten_np(v, F, dx, du), hx, T)
        return float(np.sum(g_goal * g) + np.sum(g_U * u))

    eps = 1e-6
    for _ in range(3):
        dv, dh = rng.standard_normal(flat.shape), rng.standard_normal(history.shape)
        fd = (L(flat + eps * dv, history + eps * dh) - L(flat - eps * dv, history - eps * dh)) / (2 * eps)
        lin = gp @ dv + np.sum(gh * dh)
        assert abs(fd) > 1e-3
        np.testing.assert_allclose(lin, fd, rtol=1e-6)


def test_mse_cotangents_give_the_training_gradient():
    """MLP variant: with the discounted-MSE cotangents built from the rollout itself, the parameter gradient is the
    training loss's (teacher forcing off, S = T, xseq[:, 0] = history[:, hist])."""
    ex, model, history, T = _setup("mlp", seed=3)
    flat, F, dx, du = model
    B, hist = history.shape[0], history.shape[1] - 1
    rng = np.random.default_rng(4)
    n, m = dx[-1], du[-1]
    Y, A = rng.standard_normal((B, T, n)), np.tanh(rng.standard_normal((B, T, m)))
    gamma = 0.9
    goal, U = V.forward(*model, history, T)
    d = R.discounts(T, gamma, np.float64)[None, :, None]
    g_goal = np.zeros_like(goal)
    g_goal[:, 1:] = 2 * d * (goal[:, 1:] - Y)
    g_U = 2 * d * (U - A)
    gp, gh = V.vjp(*model, history, T, g_goal, g_U)
    xseq = np.zeros((B, T, n))
    xseq[:, 0] = history[:, hist]
    _, want = R.loss_and_grad(flat, F, dx, du, xseq, A, Y, gamma, False)
    np.testing.assert_allclose(gp, want, rtol=1e-12, atol=1e-14 * np.abs(want).max())
    assert np.abs(want).max() > 1e-3
    # no carry: the teacher-forced rows reach nothing
    assert np.abs(gh[:, :hist]).max() == 0 and np.abs(gh[:, hist]).max() > 0


@pytest.mark.parametrize("name", ["lstm", "mlp"])
def test_first_goal_row_passes_straight_through(name):
    ex, model, history, T = _setup(name, seed=5)
    B, h1, n = history.shape
    g_goal = np.zeros((B, T + 1, n))
    g_goal[:, 0] = np.random.default_rng(6).standard_normal((B, n))
    gp, gh = V.vjp(*model, history, T, g_goal, None)
    assert np.abs(gp).max() == 0
    np.testing.assert_array_equal(gh[:, h1 - 1], g_goal[:, 0])
    assert np.abs(gh[:, :h1 - 1]).max() == 0


def test_lstm_history_rows_get_gradient_through_the_carry():
    ex, model, history, T = _setup("lstm", seed=7)
    goal, U = V.forward(*model, history, T)
    rng = np.random.default_rng(8)
    _, gh = V.vjp(*model, history, T, rng.standard_normal(goal.shape), rng.standard_normal(U.shape))
    assert np.abs(gh[:, 0]).max() > 1e-6


def test_entry_point_is_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert hasattr(lib, "gmpc_expert_vjp")
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    decl = re.search(r"int gmpc_expert_vjp\(([^)]*)\);", hdr)
    assert decl, "gmpc_expert_vjp is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["gmpc_ctx* ctx", "int B", "int hist", "const gmpc_expert_shape* es", "const float* expert",
                      "const float* history", "const float* g_goal", "const float* g_U", "float* grad_expert_sum",
                      "float* grad_history", "void* stream"]
    want = {"gmpc_ctx*": C.c_void_p, "int": C.c_int, "const float*": C.c_void_p, "float*": C.c_void_p,
            "void*": C.c_void_p, "const gmpc_expert_shape*": C.POINTER(_lib.ExpertShape)}
    res, args = _lib.SIGNATURES["gmpc_expert_vjp"]
    assert res is C.c_int
    assert args == [want[p.rsplit(" ", 1)[0]] for p in params]


def test_engine_method_and_layer_exist():
    p = inspect.signature(Engine.expert_vjp).parameters
    assert list(p) == ["self", "history", "expert_flat", "expert_shape", "g_goal", "g_U", "want_params",
                       "want_history"]
    assert p["g_goal"].default is None and p["g_U"].default is None
    assert p["want_params"].default is True and p["want_history"].default is True
    from gan_mpc_amd.expert.expert_model import ExpertModel
    from gan_mpc_amd.policy import differentiable
    assert list(inspect.signature(differentiable.expert_layer).parameters) == [
        "policy", "expert_flat", "expert_shape", "history"]
    assert list(inspect.signature(ExpertModel.device_params).parameters) == ["self", "expert_params", "engine"]
