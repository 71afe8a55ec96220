"""CPU side of gmpc_critic_vjp (the VJP of the critic's scores for a caller's output delta): the torch reference the GPU
tests use (tests/critic_vjp_ref.py) against the oracle's forward, against the oracle's two hard-wired gradients and
against central differences of its forward; the sensitivity helper; the ABI entry against the header and
_lib.SIGNATURES, the Engine method and the torch layer; GAN_MPC's named objectives against their closed forms."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import critic_cases as cc
import critic_vjp_ref as V
import gan_mpc_oracle as orc
import gpu_util as gu
from gan_mpc_amd import _lib
from gan_mpc_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one short and one long case per route of the table
HOST_CASES = [c for c in cc.CASES if c[5] in (1, 4, 12, 18, 22, 23, 28, 130, 31, 34)]


def _setup(case):
    n, F, T, Bc, head, seed = case
    pb, xseq, label, xs = cc.make_case(case)
    cr = orc.cast_problem(pb, np.float64)["critic"]
    return cr, V.flat_of(cr), (F,) + tuple(head) + (1,), xseq.astype(np.float64), label.astype(np.float64)


def _close(a, b, tol):
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


def test_host_cases_reach_every_route():
    assert {cc.critic_route(c[0], c[1])[0] for c in HOST_CASES} == set(cc.ROUTES) and len(HOST_CASES) == 10


@pytest.mark.parametrize("case", HOST_CASES, ids=cc.case_id)
def test_reference_forward_is_the_oracles(case):
    n, F = case[0], case[1]
    cr, flat, dims, x, _ = _setup(case)
    want = orc.critic_forward(cr, x)
    assert want.dtype == np.float64
    assert np.abs(V.forward(flat, n, F, dims, x) - want).max() <= 1e-12
    # the flat vector is pack_critic's order
    np.testing.assert_array_equal(gu.critic_flat(cc.make_case(case)[0]), flat.astype(np.float32))


@pytest.mark.parametrize("case", HOST_CASES, ids=cc.case_id)
def test_reference_gives_the_oracles_two_gradients(case):
    """g = the BCE output delta / Bc: critic_loss_and_grad's gradient; g = -1: the generator loss's dx."""
    n, F, Bc = case[0], case[1], case[3]
    cr, flat, dims, x, label = _setup(case)
    p = orc.sigmoid(orc.critic_forward(cr, x))
    g = np.where(label > 0, -(1 - p), p) / Bc
    _, gp, _ = V.vjp(flat, n, F, dims, x, g)
    want = gu.pack_grads_critic(orc.critic_loss_and_grad(cr, x, label)[1])
    _close(gp, want, 1e-10)
    assert np.abs(want).max() > 1e-6
    _, _, dx = V.vjp(flat, n, F, dims, x, -np.ones(Bc))
    _close(dx, orc.generator_loss_grad_x(cr, x), 1e-10)


def _cr_of_flat(flat, n, F, dims):
    Wx, Wh, b, head = V.unflatten(torch.as_tensor(flat), n, F, dims)
    return dict(Wx=Wx.numpy(), Wh=Wh.numpy(), b=b.numpy(), head=[(W.numpy(), bb.numpy()) for W, bb in head])


@pytest.mark.parametrize("case", HOST_CASES, ids=cc.case_id)
def test_reference_matches_central_differences(case):
    n, F, Bc, seed = case[0], case[1], case[3], case[5]
    cr, flat, dims, x, _ = _setup(case)
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(Bc)
    _, gp, gx = V.vjp(flat, n, F, dims, x, g)

    def L(v, xx):
        return float(g @ orc.critic_forward(_cr_of_flat(v, n, F, dims), xx))

    eps = 1e-6
    for _ in range(3):
        dv, dxx = rng.standard_normal(flat.shape), rng.standard_normal(x.shape)
        fd = (L(flat + eps * dv, x + eps * dxx) - L(flat - eps * dv, x - eps * dxx)) / (2 * eps)
        lin = gp @ dv + np.sum(gx * dxx)
        assert abs(fd) > 1e-3
        np.testing.assert_allclose(lin, fd, rtol=1e-6)


def test_vjp_is_linear_in_g_and_per_sequence():
    case = HOST_CASES[1]
    n, F, Bc = case[0], case[1], case[3]
    cr, flat, dims, x, _ = _setup(case)
    g = V.case_g(case).astype(np.float64)
    g[2] = 0.0
    _, gp, gx = V.vjp(flat, n, F, dims, x, g)
    _, gp2, gx2 = V.vjp(flat, n, F, dims, x, 2 * g)
    _close(gp2, 2 * gp, 1e-13)
    _close(gx2, 2 * gx, 1e-13)
    assert np.abs(gx[2]).max() == 0 and np.abs(gx[0]).max() > 0


def test_sensitivity_names_every_compared_block():
    case = HOST_CASES[0]
    n, F, T, Bc, head, _ = case
    sens = V.sensitivity(case, V.case_g(case), trials=2)
    names = [f"head{l}.{k}" for l in range(len(head) + 1) for k in ("W", "b")]
    assert list(sens) == ["Wx", "Wh", "b"] + names + ["dx", "dx t=0", "dx t=T1-1"]
    assert all(np.isfinite(v) and v >= 0 for v in sens.values()) and max(sens.values()) > 0, sens


# ---- ABI ---------------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert hasattr(lib, "gmpc_critic_vjp")
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    decl = re.search(r"int gmpc_critic_vjp\(([^)]*)\);", hdr)
    assert decl, "gmpc_critic_vjp is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["gmpc_ctx* ctx", "int Bc", "const float* xseq", "const float* critic", "const float* g_score",
                      "float* score", "float* grad_xseq", "float* grad_critic_sum", "void* stream"]
    want = {"gmpc_ctx*": C.c_void_p, "int": C.c_int, "const float*": C.c_void_p, "float*": C.c_void_p,
            "void*": C.c_void_p}
    res, args = _lib.SIGNATURES["gmpc_critic_vjp"]
    assert res is C.c_int
    assert args == [want[p.rsplit(" ", 1)[0]] for p in params]


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    comment = hdr[:hdr.index("int gmpc_critic_vjp(")].rsplit("/*", 1)[1]
    for phrase in ("g_score", "SUMMED over the batch", "true derivative", "GMPC_EINVAL", "Stateless", "Deterministic",
                   "not both gradients"):
        assert phrase in comment, phrase


def test_engine_method_and_layer_exist():
    p = inspect.signature(Engine.critic_vjp).parameters
    assert list(p) == ["self", "xseq", "critic", "g_score", "want_dx", "want_params", "grad_sum"]
    assert p["want_dx"].default is True and p["want_params"].default is True and p["grad_sum"].default is None
    from gan_mpc_amd.policy import base, differentiable, optimizers
    assert list(inspect.signature(differentiable.critic_layer).parameters) == ["policy", "params", "xseq"]
    assert "critic_layer" in differentiable.__doc__
    assert inspect.signature(optimizers.bilevel_optimization).parameters["cotangents"].default is None
    assert hasattr(base.BaseMPC, "batch_cotangents")


# ---- GAN_MPC's objectives ------------------------------------------------------------------------------------------
SCORE = np.array([-2.5, -0.3, 0.0, 0.4, 1.0, 3.0])
LABEL = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])


def _closed_forms(name):
    s, y = SCORE, LABEL
    p = 1.0 / (1.0 + np.exp(-s))
    if name == "js":         # the BCE of gan/js_policy.py and -log p + log(1 - p) = -score
        return -np.log(np.where(y > 0, p, 1 - p)), -np.log(p) + np.log(1 - p)
    if name == "wgan":
        return -y * s, -s
    if name == "lsgan":
        return 0.5 * (s - (y > 0)) ** 2, 0.5 * (s - 1) ** 2
    return np.maximum(0.0, 1 - y * s), -s


@pytest.mark.parametrize("name", ["js", "wgan", "lsgan", "hinge"])
def test_named_objectives_are_their_closed_forms(name):
    from gan_mpc_amd.gan import gan_policy
    critic_obj, gen_obj = gan_policy.get_objective(name)
    s, y = torch.as_tensor(SCORE), torch.as_tensor(LABEL)
    want_c, want_g = _closed_forms(name)
    got_c, got_g = critic_obj(s, y), gen_obj(s)
    assert tuple(got_c.shape) == (6,) and tuple(got_g.shape) == (6,)
    np.testing.assert_allclose(got_c.numpy(), want_c, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(got_g.numpy(), want_g, rtol=1e-14, atol=1e-15)


def test_objective_argument_is_checked():
    from gan_mpc_amd.gan import gan_policy
    pair = (lambda s, y: s * y, lambda s: s)
    assert gan_policy.get_objective(pair) == pair
    assert issubclass(gan_policy.GAN_MPC, gan_policy.js_policy.JS_MPC)
    for bad in ("ns", ("js",), (1, 2), None):
        with pytest.raises(ValueError):
            gan_policy.get_objective(bad)
