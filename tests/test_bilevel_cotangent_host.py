"""CPU side of gmpc_bilevel_grad_cotangent (the bilevel gradient of a caller-defined upper-level loss): the ABI entry,
the per-trajectory cotangent helper (optimizers.loss_cotangents) against a plain autograd loop, and the policy's
refusal when there is no loss at all."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gan_mpc_amd import _lib
from gan_mpc_amd.policy import base
from gan_mpc_amd.policy import optimizers as opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_exported_and_its_signature_matches_the_header():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert hasattr(lib, "gmpc_bilevel_grad_cotangent")
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    decl = re.search(r"int gmpc_bilevel_grad_cotangent\(([^)]*)\);", hdr)
    assert decl, "gmpc_bilevel_grad_cotangent is not declared in the header"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["gmpc_ctx* ctx", "int B", "const float* lx", "const float* lu", "float sign",
                      "float* grad_sum", "void* stream"]
    want = {"gmpc_ctx*": C.c_void_p, "int": C.c_int, "float": C.c_float, "const float*": C.c_void_p,
            "float*": C.c_void_p, "void*": C.c_void_p}
    res, args = _lib.SIGNATURES["gmpc_bilevel_grad_cotangent"]
    assert res is C.c_int
    assert args == [want[p.rsplit(" ", 1)[0]] for p in params]


def _huber_u_loss(x, u, params, desired, w):
    """X and U dependent: a per-step weighted Huber state error (mapped `desired`), a time-weighted control penalty
    (unmapped weights `w`)."""
    del params
    d = x[:, : desired.shape[-1]] - desired
    a = d.abs()
    hub = torch.where(a < 0.5, 0.5 * d * d, 0.5 * (a - 0.25))
    steps = torch.arange(x.shape[0], dtype=x.dtype)
    return ((1.0 + 0.1 * steps)[:, None] * hub).mean(0).sum() + (w[:, None] * u * u).sum()


def test_vmap_helper_matches_a_per_sample_autograd_loop():
    rng = np.random.default_rng(4)
    B, T, n, m, nx = 5, 6, 7, 3, 4
    X = torch.as_tensor(rng.standard_normal((B, T + 1, n)), dtype=torch.float32)
    U = torch.as_tensor(rng.standard_normal((B, T, m)), dtype=torch.float32)
    desired = rng.standard_normal((B, T + 1, nx)).astype(np.float32)       # numpy, mapped: moved to X's device
    w = torch.as_tensor(rng.random(T) + 0.5, dtype=torch.float32)          # unmapped
    params = object()                                                       # passed through, never differentiated
    loss, lx, lu = opt.loss_cotangents(_huber_u_loss, X, U, params, (desired, w), (0, None))
    assert loss.shape == (B,) and lx.shape == (B, T + 1, n) and lu.shape == (B, T, m)
    assert lx.is_contiguous() and lu.is_contiguous() and lx.dtype == torch.float32
    for b in range(B):
        x = X[b].clone().requires_grad_(True)
        u = U[b].clone().requires_grad_(True)
        v = _huber_u_loss(x, u, params, torch.as_tensor(desired[b]), w)
        gx, gu = torch.autograd.grad(v, (x, u))
        torch.testing.assert_close(loss[b], v.detach(), rtol=1e-6, atol=0)
        torch.testing.assert_close(lx[b], gx, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(lu[b], gu, rtol=1e-6, atol=1e-7)
    assert float(lx[:, :, nx:].abs().max()) == 0.0        # columns the loss does not read
    assert float(lu.abs().max()) > 0.0
    # the value alone (batch_loss), and the default in_dims: 0 for every loss argument
    v_only, none_x, none_u = opt.loss_cotangents(lambda x, u, p, dsr: ((x[:, :nx] - dsr) ** 2).mean(0).sum(),
                                                 X, U, params, (desired,), want_grad=False)
    assert none_x is None and none_u is None
    ref = ((X[:, :, :nx] - torch.as_tensor(desired)) ** 2).mean(1).sum(-1)
    torch.testing.assert_close(v_only, ref, rtol=1e-6, atol=0)


def test_vmap_helper_refusals():
    X, U = torch.zeros(2, 3, 2), torch.zeros(2, 2, 1)
    with pytest.raises(ValueError, match="loss_vmap"):
        opt.loss_cotangents(lambda x, u, p, a: x.sum(), X, U, None, (np.zeros((2, 3)),), (0, None))
    with pytest.raises(ValueError, match="scalar per trajectory"):
        opt.loss_cotangents(lambda x, u, p: x.sum(0), X, U, None, want_grad=False)
    with pytest.raises(RuntimeError, match="scalar"):        # (torch.func's own refusal under grad)
        opt.loss_cotangents(lambda x, u, p: x.sum(0), X, U, None)


class _NoLoss(base.BaseMPC):
    pass


class _WithLoss(base.BaseMPC):
    def loss(self, xcseq, useq, params, desired):
        return ((xcseq - desired) ** 2).sum()


def test_policy_without_loss_kind_or_loss_refuses_before_any_device_work():
    pol = _NoLoss.__new__(_NoLoss)          # no models, no engine, no device: nothing may be touched
    with pytest.raises(NotImplementedError):
        pol.loss_and_grad(np.zeros((2, 3, 4), np.float32), None, (None,))
    with pytest.raises(NotImplementedError):
        pol.batch_loss(None, np.zeros((2, 3, 4), np.float32), None)
    assert base.BaseMPC.LOSS_KIND is None
    assert _WithLoss.__new__(_WithLoss)._custom_loss() is True
