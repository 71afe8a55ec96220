"""The Jacobian chain over each sample's active relu units (k_linearize_sparse) returns the dense chain's bits.

Every case runs the same inputs through the default route and through GMPC_LIN=dense (k_linearize_regs alone) and
compares with assert_array_equal: the parity shapes with 200-wide hidden layers, the full-shape C3 problems, relu
masks forced to edge cases through the biases (a layer with no active unit, every unit active, one active unit,
counts that are not a multiple of 4 or 16, only tail units 192..199), and five iterations of the iLQR solve (its
later iterations run the chain with the `active` trajectory filter)."""
import numpy as np
import pytest
import torch

import gpu_util as gu
import test_gpu_fullshape as fs
from test_gpu_parity import SHAPES

SPARSE_SHAPES = [k for k, (n, m, T, B, kw) in SHAPES.items()
                 if kw.get("dyn_hidden", (200, 200, 200)) == (200, 200, 200) and n + m <= 32]


def _both(eng, fn, monkeypatch):
    out = {}
    for route in ("sparse", "dense"):
        if route == "dense":
            monkeypatch.setenv("GMPC_LIN", "dense")
        else:
            monkeypatch.delenv("GMPC_LIN", raising=False)
        res = fn()
        torch.cuda.synchronize()
        out[route] = ({k: v.cpu().numpy().copy() for k, v in res.items() if torch.is_tensor(v)},
                      eng.profile_kernel_name("linearize"))
    monkeypatch.delenv("GMPC_LIN", raising=False)
    return out


def _backward(eng, pb):
    d = eng.to_dev
    x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])

    def run():
        X, _ = eng.rollout_cost(x0, U, goal)
        return eng.lqr_backward(X, U, goal, after_rollout=True)
    return run


def _check_backward(eng, pb, monkeypatch):
    eng.profile_enable(True)
    out = _both(eng, _backward(eng, pb), monkeypatch)
    eng.profile_enable(False)
    (sp, name_sp), (de, name_de) = out["sparse"], out["dense"]
    assert name_sp.startswith("k_linearize_sparse"), name_sp
    assert name_de.startswith("k_linearize_regs"), name_de
    assert np.isfinite(de["AB"]).all()
    for key in ("AB", "K", "k", "grad", "adjoints"):
        np.testing.assert_array_equal(sp[key], de[key], err_msg=key)
    return de["AB"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SPARSE_SHAPES)
def test_parity_shapes(name, monkeypatch):
    n, m, T, B, kw = SHAPES[name]
    pb = gu.problem(n, m, T, B, seed=11, **kw)
    eng = gu.engine_for(pb, critic=False)
    _check_backward(eng, pb, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3-bench", "c3-trained"])
def test_full_shape(name, monkeypatch):
    pb, _ = fs._problem(name)
    eng = gu.engine_for(pb, critic=False)
    _check_backward(eng, pb, monkeypatch)


def _force(pb, layer, on):
    """Hidden layer `layer`: units in `on` forced active, the rest inactive, for every input of the test."""
    W, b = pb["dyn"][layer]
    b = np.full_like(b, -1e4)
    b[list(on)] = 1e4
    pb["dyn"][layer] = (W, b.astype(np.float32))


EDGE = {
    "layer2-dead": {1: []},
    "all-active": {0: range(200), 1: range(200), 2: range(200)},
    "one-active": {0: [7], 1: [199], 2: [100]},
    "ragged-counts": {0: range(3, 200, 5), 1: list(range(37)) + [193, 196], 2: range(1, 200, 2)},
    "tail-only": {0: range(192, 200), 1: [192, 195, 198], 2: range(190, 200)},
    "last-dead": {2: []},
}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 12])
@pytest.mark.parametrize("case", list(EDGE))
def test_forced_masks(case, n, monkeypatch):
    pb = gu.problem(n, 6, 2, 9, seed=4)
    for layer, on in EDGE[case].items():
        _force(pb, layer, on)
    eng = gu.engine_for(pb, critic=False)
    AB = _check_backward(eng, pb, monkeypatch)
    if any(len(list(on)) == 0 for on in EDGE[case].values()):
        # a layer without an active unit: the chain is zero and [A | B] = [I | 0]
        eye = np.zeros_like(AB)
        eye[..., np.arange(n), np.arange(n)] = 1.0
        np.testing.assert_array_equal(AB, eye)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3-trained", "c2-cheetah"])
def test_solve_routes_agree(name, monkeypatch):
    if name in SHAPES:
        n, m, T, B, kw = SHAPES[name]
        pb = gu.problem(n, m, T, B, seed=11, **kw)
    else:
        pb, _ = fs._problem(name)
    eng = gu.engine_for(pb, critic=False)
    d = eng.to_dev
    B, n, m, T = pb["B"], pb["n"], pb["m"], pb["T"]

    def run():
        out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 5})
        out["AB"] = eng.debug_buffer(5, (B, T, n, n + m)).clone()
        return out
    out = _both(eng, run, monkeypatch)
    sp, de = out["sparse"][0], out["dense"][0]
    for key in ("X", "U", "obj", "grad", "iterations", "AB"):
        np.testing.assert_array_equal(sp[key], de[key], err_msg=key)
