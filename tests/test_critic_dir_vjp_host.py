"""CPU side of gmpc_critic_dir_vjp (the second-order VJP of the critic's scores): the torch double-backward reference the
GPU tests use (tests/critic_dir_ref.py) against the oracle's input gradient, against central differences of it, and its
symmetry; the exactly-zero head-bias blocks; the sensitivity helper; GAN_MPC's gradient_penalty spec; the ABI entry
against the header and _lib.SIGNATURES, the Engine method and the layer."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import critic_cases as cc
import critic_dir_ref as D
import critic_vjp_ref as V
import gan_mpc_oracle as orc
import gpu_util as gu
from gan_mpc_amd import _lib
from gan_mpc_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ten cases off the wide-input route: the register-weight shapes (every NX), run-time n at F = 64, other F
HOST_CASES = [c for c in cc.CASES if c[5] in (1, 4, 7, 12, 13, 18, 23, 28, 29, 130)]


def _setup(case):
    n, F, T, Bc, head, seed = case
    pb, xseq, _, _ = cc.make_case(case)
    cr = orc.cast_problem(pb, np.float64)["critic"]
    return (cr, V.flat_of(cr), (F,) + tuple(head) + (1,), xseq.astype(np.float64), D.case_v(case).astype(np.float64),
            D.case_gdir(case).astype(np.float64))


def _cr_of_flat(flat, n, F, dims):
    Wx, Wh, b, head = V.unflatten(torch.as_tensor(flat), n, F, dims)
    return dict(Wx=Wx.numpy(), Wh=Wh.numpy(), b=b.numpy(), head=[(W.numpy(), bb.numpy()) for W, bb in head])


def _close(a, b, tol):
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


def test_host_cases_reach_the_three_routes():
    assert {cc.critic_route(c[0], c[1])[0] for c in HOST_CASES} == {"gen2", "gen1", "generic"}
    assert len(HOST_CASES) == 10
    assert {cc.critic_route(c[0], c[1])[1] for c in HOST_CASES if cc.critic_route(c[0], c[1])[0] == "gen2"} == set(cc.NXS)


@pytest.mark.parametrize("case", HOST_CASES, ids=cc.case_id)
def test_sdot_is_the_oracles_input_gradient_along_v(case):
    n, F = case[0], case[1]
    cr, flat, dims, x, v, g = _setup(case)
    score, sdot, _, _ = D.dir_vjp(flat, n, F, dims, x, v, g)
    _close(score, orc.critic_forward(cr, x), 1e-12)
    want = np.sum(-orc.generator_loss_grad_x(cr, x) * v, axis=(1, 2))       # the generator loss is -score
    assert np.abs(want).max() > 1e-6
    _close(sdot, want, 1e-10)


@pytest.mark.parametrize("case", HOST_CASES, ids=cc.case_id)
def test_gradients_match_central_differences_of_the_oracle(case):
    n, F, seed = case[0], case[1], case[5]
    cr, flat, dims, x, v, g = _setup(case)
    _, _, gp, gx = D.dir_vjp(flat, n, F, dims, x, v, g)

    def L(fl, xx):
        return float(g @ np.sum(-orc.generator_loss_grad_x(_cr_of_flat(fl, n, F, dims), xx) * v, axis=(1, 2)))

    def sides(fl, xx):
        c = _cr_of_flat(fl, n, F, dims)
        _, (_, hT, _) = orc.critic_forward(c, xx, keep=True)
        return np.concatenate([(z > 0).ravel() for z in orc.mlp_forward(c["head"], hT)[1]])

    # A central difference is the derivative only where sdot is smooth between its two points: sdot jumps where a head
    # unit changes side (the derivative of the relu mask is a delta there, which the VJP rightly leaves out).  Directions
    # along which a unit changes side within +-h are not used; two valid ones per variable are required.
    rng = np.random.default_rng(seed)
    h = 1e-5
    done_p = done_x = 0
    for _ in range(24):
        w, wx = rng.standard_normal(flat.shape), rng.standard_normal(x.shape)
        if done_p < 2 and np.array_equal(sides(flat + h * w, x), sides(flat - h * w, x)):
            fd_p = (L(flat + h * w, x) - L(flat - h * w, x)) / (2 * h)
            np.testing.assert_allclose(gp @ w, fd_p, rtol=1e-6, atol=1e-9 * np.abs(gp).max())
            done_p += 1
        if done_x < 2 and np.array_equal(sides(flat, x + h * wx), sides(flat, x - h * wx)):
            fd_x = (L(flat, x + h * wx) - L(flat, x - h * wx)) / (2 * h)
            np.testing.assert_allclose(np.sum(gx * wx), fd_x, rtol=1e-6, atol=1e-9 * np.abs(gx).max())
            done_x += 1
    assert done_p == 2 and done_x == 2, (done_p, done_x)


@pytest.mark.parametrize("case", HOST_CASES, ids=cc.case_id)
def test_second_derivative_in_x_is_symmetric(case):
    n, F, Bc, seed = case[0], case[1], case[3], case[5]
    cr, flat, dims, x, v, _ = _setup(case)
    w = np.random.default_rng(5000 + seed).standard_normal(x.shape)
    one = np.ones(Bc)
    gx_v = D.dir_vjp(flat, n, F, dims, x, v, one)[3]
    gx_w = D.dir_vjp(flat, n, F, dims, x, w, one)[3]
    a, b = np.sum(gx_v * w, axis=(1, 2)), np.sum(gx_w * v, axis=(1, 2))
    _close(a, b, 1e-10)


@pytest.mark.parametrize("case", HOST_CASES, ids=cc.case_id)
def test_head_bias_blocks_are_exactly_zero(case):
    n, F = case[0], case[1]
    cr, flat, dims, x, v, g = _setup(case)
    for dtype in (np.float64, np.float32):
        gp = D.dir_vjp(flat, n, F, dims, x, v, g, dtype)[2]
        blocks = dict(gu.split_critic_flat(gp, n, F, dims))
        for name, blk in blocks.items():
            if name.startswith("head") and name.endswith(".b"):
                assert np.abs(blk).max() == 0, name
        assert np.abs(blocks["b"]).max() > 0 and np.abs(blocks["head0.W"]).max() > 0


def test_call_is_linear_in_v_and_in_g_and_per_sequence():
    case = HOST_CASES[1]
    n, F = case[0], case[1]
    cr, flat, dims, x, v, g = _setup(case)
    v[2] = 0.0
    g[3] = 0.0
    _, sd, gp, gx = D.dir_vjp(flat, n, F, dims, x, v, g)
    _, sd2, gp2, gx2 = D.dir_vjp(flat, n, F, dims, x, 2 * v, g)
    _close(sd2, 2 * sd, 1e-13), _close(gp2, 2 * gp, 1e-13), _close(gx2, 2 * gx, 1e-13)
    _, sd3, gp3, gx3 = D.dir_vjp(flat, n, F, dims, x, v, 2 * g)
    _close(sd3, sd, 1e-13), _close(gp3, 2 * gp, 1e-13), _close(gx3, 2 * gx, 1e-13)
    assert sd[2] == 0 and np.abs(gx[2]).max() == 0 and np.abs(gx[3]).max() == 0 and np.abs(gx[0]).max() > 0


def test_sensitivity_names_every_compared_block():
    case = HOST_CASES[0]
    n, F, T, Bc, head, _ = case
    sens = D.sensitivity(case, D.case_v(case), D.case_gdir(case), trials=2)
    names = [f"head{l}.{k}" for l in range(len(head) + 1) for k in ("W", "b")]
    assert list(sens) == ["sdot", "Wx", "Wh", "b"] + names + ["dx", "dx t=0", "dx t=T1-1"]
    assert all(np.isfinite(s) and s >= 0 for s in sens.values()) and max(sens.values()) > 0, sens


def test_penalty_reference_is_mean_objective_plus_weighted_mean_penalty():
    case = HOST_CASES[1]
    n, F, T, Bc, head, seed = case
    cr, flat, dims, x, _, _ = _setup(case)
    lab = np.where(np.arange(Bc) % 2 == 0, 1.0, -1.0)
    eps = np.random.default_rng(seed).random(Bc)
    score = orc.critic_forward(cr, x)
    for at, target in (("true", 0.0), ("mixed", 1.0)):
        loss, grad, norms = D.penalty_loss_grad(flat, n, F, dims, x, lab, 10.0, target, at, eps)
        xhat = D.penalty_points(x, lab, at, eps)
        assert len(norms) == len(xhat) == ((Bc + 1) // 2 if at == "true" else Bc // 2)
        want = np.sqrt(np.sum(orc.generator_loss_grad_x(cr, xhat) ** 2, axis=(1, 2)))
        _close(norms, want, 1e-10)
        np.testing.assert_allclose(loss, np.mean(-lab * score) + 10.0 * np.mean((want - target) ** 2), rtol=1e-12)
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    # no penalty point: the objective alone
    loss, grad, norms = D.penalty_loss_grad(flat, n, F, dims, x, -np.ones(Bc), 10.0, 1.0, "mixed", eps)
    assert len(norms) == 0
    np.testing.assert_allclose(loss, np.mean(score), rtol=1e-12)


# ---- GAN_MPC's gradient_penalty argument -----------------------------------------------------------------------------
def test_gradient_penalty_spec_is_checked():
    from gan_mpc_amd.gan import gan_policy
    assert gan_policy.get_gradient_penalty(None) is None
    assert gan_policy.get_gradient_penalty(dict(weight=10)) == dict(weight=10.0, target=1.0, at="mixed", seed=0)
    assert gan_policy.get_gradient_penalty(dict(weight=0.5, target=0, at="true", seed=7)) == dict(
        weight=0.5, target=0.0, at="true", seed=7)
    for bad in (10.0, "mixed", dict(), dict(target=1.0), dict(weight=-1.0), dict(weight="1"), dict(weight=True),
                dict(weight=float("nan")), dict(weight=1.0, target=-0.5), dict(weight=1.0, target=float("inf")),
                dict(weight=1.0, at="fake"), dict(weight=1.0, seed=-1), dict(weight=1.0, seed=0.5),
                dict(weight=1.0, lam=2.0)):
        with pytest.raises(ValueError):
            gan_policy.get_gradient_penalty(bad)
    p = inspect.signature(gan_policy.gradient_penalty).parameters
    assert list(p)[:5] == ["policy", "dparams", "flat", "xhat", "target"]
    assert inspect.signature(gan_policy.GAN_MPC.__init__).parameters["gradient_penalty"].default is None


# ---- ABI ---------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_bound():
    """(fails without the feature)"""
    assert "gmpc_critic_dir_vjp" in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    decl = re.search(r"int gmpc_critic_dir_vjp\(([^)]*)\);", hdr)
    assert decl, "gmpc_critic_dir_vjp is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["gmpc_ctx* ctx", "int Bc", "const float* xseq", "const float* critic", "const float* v_xseq",
                      "const float* g_dir", "float* score", "float* sdot", "float* grad_xseq", "float* grad_critic_sum",
                      "void* stream"]
    want = {"gmpc_ctx*": C.c_void_p, "int": C.c_int, "const float*": C.c_void_p, "float*": C.c_void_p,
            "void*": C.c_void_p}
    res, args = _lib.SIGNATURES["gmpc_critic_dir_vjp"]
    assert res is C.c_int
    assert args == [want[p.rsplit(" ", 1)[0]] for p in params]
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "gmpc_critic_dir_vjp")


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    comment = hdr[:hdr.index("int gmpc_critic_dir_vjp(")].rsplit("/*", 1)[1]
    for phrase in ("g_dir", "sdot", "SUMMED over the batch", "head-bias", "zeros", "GMPC_EINVAL", "unsupported shape",
                   "Stateless", "deterministic", "no Hessian"):
        assert phrase in comment, phrase


def test_engine_method_and_layer_exist():
    p = inspect.signature(Engine.critic_dir_vjp).parameters
    assert list(p) == ["self", "xseq", "critic", "v", "g_dir", "want_dx", "want_params", "grad_sum"]
    assert p["g_dir"].default is None and p["want_dx"].default is True and p["want_params"].default is True
    assert p["grad_sum"].default is None
    from gan_mpc_amd.policy import differentiable
    assert hasattr(differentiable, "CriticGradFunction") and "gmpc_critic_dir_vjp" in differentiable.__doc__
