"""CPU side of gmpc_rollout_vjp (the VJP of the rollout and its per-step costs): the ABI entry against the header and
_lib.SIGNATURES, the Engine method and the torch layer, and the fp64 per-step reference the GPU tests use -- against
torch fp64 autograd through tests/torch_ref.py (rollout, cost) and against central differences of the oracle's
rollout / evaluate."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import torch_ref as tr
from gan_mpc_amd import _lib
from gan_mpc_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference(pb, X, U, goal, gX=None, gc=None):
    """The kernels' per-step form in X's dtype: the terminal-cost VJP through the cost MLP, then for t = T-1 .. 0 the
    backward pass of v_{t+1} through the dynamics MLP at (X_t, U_t) and the staging-cost terms in closed form.
    -> dict(x0 (B, n), U (B, T, m), goal (B, T+1, n), theta [3 + cost count] and dyn [dyn count], both summed over the
    batch, in the flat layouts of gmpc_bilevel_grad's grad_sum and gmpc_set_params' dyn vector)."""
    dt = X.dtype
    p = orc.cast_problem(pb, dt)
    dyn, cm = p["dyn"], p["cmlp"]
    goal = np.asarray(goal, dt)
    B, T, m = U.shape
    n = X.shape[-1]
    gX = np.zeros(X.shape, dt) if gX is None else np.asarray(gX, dt)
    gc = np.zeros(X.shape[:2], dt) if gc is None else np.asarray(gc, dt)
    w = orc.sigmoid(np.asarray(p["mpc_w"], dt))
    a = dt.type(orc.ALPHA)
    gm = np.zeros(3, dt)
    # terminal: c_T = w2 |MLP_c(x_T)|^2
    acts = [X[:, T]]
    for W, b in cm[:-1]:
        acts.append(np.maximum(acts[-1] @ W + b, 0))
    y = acts[-1] @ cm[-1][0] + cm[-1][1]
    gm[2] = np.sum(gc[:, T] * w[2] * (1 - w[2]) * np.sum(y * y, -1))
    e = 2 * w[2] * gc[:, T, None] * y
    gcost = [None] * len(cm)
    for li in range(len(cm) - 1, -1, -1):
        gcost[li] = (acts[li].T @ e, e.sum(0))
        e = e @ cm[li][0].T
        if li > 0:
            e = np.where(acts[li] > 0, e, 0)
    v = gX[:, T] + e
    gU = np.zeros(U.shape, dt)
    ggoal = np.zeros((B, T + 1, goal.shape[-1]), dt)
    gdyn = [(np.zeros_like(W), np.zeros_like(b)) for W, b in dyn]
    for t in range(T - 1, -1, -1):
        da = [np.concatenate([X[:, t], U[:, t]], -1)]
        for W, b in dyn[:-1]:
            da.append(np.maximum(da[-1] @ W + b, 0))
        e = v
        for li in range(len(dyn) - 1, -1, -1):
            gdyn[li] = (gdyn[li][0] + da[li].T @ e, gdyn[li][1] + e.sum(0))
            e = e @ dyn[li][0].T
            if li > 0:
                e = np.where(da[li] > 0, e, 0)
        px, pu = e[:, :n], e[:, n:]
        d = X[:, t, :goal.shape[-1]] - goal[:, t]
        sx = np.sqrt(np.sum(d * d, -1) + a * a)
        su = np.sqrt(np.sum(U[:, t] ** 2, -1) + a * a)
        g = gc[:, t]
        gU[:, t] = (g * w[0] / su)[:, None] * U[:, t] + pu
        gxc = (g * w[1] / sx)[:, None] * d
        ggoal[:, t] = -gxc
        v = gX[:, t] + v + px
        v[:, :goal.shape[-1]] += gxc
        gm[0] += np.sum(g * w[0] * (1 - w[0]) * (su - a))
        gm[1] += np.sum(g * w[1] * (1 - w[1]) * (sx - a))
    flat = lambda layers: np.concatenate([np.concatenate([W.reshape(-1), b]) for W, b in layers])  # noqa: E731
    return dict(x0=v, U=gU, goal=ggoal, theta=np.concatenate([gm, flat(gcost)]), dyn=flat(gdyn))


def _problem(name):
    if name == "pendulum":
        return orc.make_problem(3, 1, 5, 3, seed=2, dtype=np.float64, dyn_hidden=(16, 16), cost_hidden=(8,),
                                cost_fout=3)
    return orc.make_problem(5, 2, 4, 3, seed=5, dtype=np.float64, dyn_hidden=(33, 47), cost_hidden=(24,),
                            cost_fout=6)


def _cots(pb, X, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(X.shape), rng.standard_normal(X.shape[:2])


@pytest.mark.parametrize("name", ["pendulum", "ragged"])
def test_reference_equals_torch_autograd(name):
    pb = _problem(name)
    X = orc.rollout(pb["dyn"], pb["U"], pb["x0"])
    gX, gc = _cots(pb, X, 1)
    ref = reference(pb, X, pb["U"], pb["goal"], gX, gc)
    B, T, m = pb["U"].shape
    mw = tr.t64(pb["mpc_w"]).requires_grad_(True)
    cm = [(W.requires_grad_(True), b.requires_grad_(True)) for W, b in tr.layers64(pb["cmlp"])]
    dy = [(W.requires_grad_(True), b.requires_grad_(True)) for W, b in tr.layers64(pb["dyn"])]
    theta = [mw] + [p for wb in cm for p in wb]
    dleaves = [p for wb in dy for p in wb]
    gt_sum = [torch.zeros_like(p) for p in theta]
    gd_sum = [torch.zeros_like(p) for p in dleaves]
    for b in range(B):
        x0 = tr.t64(pb["x0"][b]).requires_grad_(True)
        U = tr.t64(pb["U"][b]).requires_grad_(True)
        goal = tr.t64(pb["goal"][b]).requires_grad_(True)
        Xt = tr.rollout(dy, U, x0)
        zero = torch.zeros(m, dtype=torch.float64)
        costs = torch.stack([tr.cost(cm, mw, goal, Xt[t], U[t] if t < T else zero, t, T) for t in range(T + 1)])
        L = (tr.t64(gX[b]) * Xt).sum() + (tr.t64(gc[b]) * costs).sum()
        g = torch.autograd.grad(L, [x0, U, goal] + theta + dleaves)
        for key, gg in zip(("x0", "U", "goal"), g[:3]):
            np.testing.assert_allclose(ref[key][b], gg.numpy(), rtol=1e-10, atol=1e-12)
        gt_sum = [s + x for s, x in zip(gt_sum, g[3:3 + len(theta)])]
        gd_sum = [s + x for s, x in zip(gd_sum, g[3 + len(theta):])]
    want_theta = np.concatenate([x.reshape(-1).numpy() for x in gt_sum])
    want_dyn = np.concatenate([x.reshape(-1).numpy() for x in gd_sum])
    np.testing.assert_allclose(ref["theta"], want_theta, rtol=1e-10, atol=1e-12 * np.abs(want_theta).max())
    np.testing.assert_allclose(ref["dyn"], want_dyn, rtol=1e-10, atol=1e-12 * np.abs(want_dyn).max())
    assert np.abs(ref["goal"][:, T]).max() == 0


def _pack(pb):
    return np.concatenate([np.asarray(pb["mpc_w"], np.float64)] +
                          [np.concatenate([W.reshape(-1), b]) for W, b in pb["cmlp"]] +
                          [np.concatenate([W.reshape(-1), b]) for W, b in pb["dyn"]])


def _unpack(pb, v):
    out, o = dict(pb), 3
    out["mpc_w"] = v[:3]
    for key in ("cmlp", "dyn"):
        layers = []
        for W, b in pb[key]:
            Wn = v[o:o + W.size].reshape(W.shape)
            o += W.size
            layers.append((Wn, v[o:o + b.size]))
            o += b.size
        out[key] = layers
    return out


@pytest.mark.parametrize("name", ["pendulum", "ragged"])
def test_reference_matches_central_differences(name):
    pb = _problem(name)
    X = orc.rollout(pb["dyn"], pb["U"], pb["x0"])
    gX, gc = _cots(pb, X, 2)
    ref = reference(pb, X, pb["U"], pb["goal"], gX, gc)
    th = _pack(pb)

    def L(x0, U, goal, v):
        p = _unpack(pb, v)
        Xp = orc.rollout(p["dyn"], U, x0)
        return float(np.sum(gX * Xp) + np.sum(gc * orc.evaluate(p["cmlp"], p["mpc_w"], goal, Xp, U)))

    rng = np.random.default_rng(4)
    eps = 1e-6
    for _ in range(3):
        d = [rng.standard_normal(a.shape) for a in (pb["x0"], pb["U"], pb["goal"], th)]
        d[2][:, -1] = 0    # the terminal row of the goal is not read
        plus = L(pb["x0"] + eps * d[0], pb["U"] + eps * d[1], pb["goal"] + eps * d[2], th + eps * d[3])
        minus = L(pb["x0"] - eps * d[0], pb["U"] - eps * d[1], pb["goal"] - eps * d[2], th - eps * d[3])
        fd = (plus - minus) / (2 * eps)
        lin = (np.sum(ref["x0"] * d[0]) + np.sum(ref["U"] * d[1]) + np.sum(ref["goal"] * d[2]) +
               ref["theta"] @ d[3][:ref["theta"].size] + ref["dyn"] @ d[3][ref["theta"].size:])
        assert abs(fd) > 1e-3
        np.testing.assert_allclose(lin, fd, rtol=1e-6)


def test_entry_point_is_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert hasattr(lib, "gmpc_rollout_vjp")
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    decl = re.search(r"int gmpc_rollout_vjp\(([^)]*)\);", hdr)
    assert decl, "gmpc_rollout_vjp is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["gmpc_ctx* ctx", "int B", "const float* X", "const float* U", "const float* goal",
                      "const float* gX", "const float* gcost", "float* grad_x0", "float* grad_U",
                      "float* grad_goal", "float* grad_theta_sum", "float* grad_dyn_sum", "void* stream"]
    want = {"gmpc_ctx*": C.c_void_p, "int": C.c_int, "const float*": C.c_void_p, "float*": C.c_void_p,
            "void*": C.c_void_p}
    res, args = _lib.SIGNATURES["gmpc_rollout_vjp"]
    assert res is C.c_int
    assert args == [want[p.rsplit(" ", 1)[0]] for p in params]


def test_engine_method_and_layer_exist():
    assert list(inspect.signature(Engine.rollout_vjp).parameters) == [
        "self", "X", "U", "goal", "gX", "gcost", "want_x0", "want_U", "want_goal", "want_theta", "want_dyn"]
    from gan_mpc_amd.policy import differentiable
    p = inspect.signature(differentiable.rollout_layer).parameters
    assert list(p)[:5] == ["policy", "params", "x0", "U", "goal"]
    assert p["dynamics_grad"].default is True
