"""The one-step disagreement's VJP without a GPU (gmpc_ensemble_disagreement_vjp): the fp64
reference against torch autograd of a torch transcription of disagreement_ref.plan (H1); the two exact properties -- an
equal member gives exact zeros, a member's row depends on neither P nor the other members' cotangents -- in the fp32
reference, bit for bit (H2); the kink filter's cap and the conditioning cap on the fp64 reference for every case and the
seeds the GPU test draws from (H3); the entry point's declaration, binding and argument order, and every Engine refusal
raised before the library is called (H4)."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import disagreement_ref as dr
import disagreement_vjp_cases as vc
import disagreement_vjp_ref as vr
import gpu_util as gu
import sampled_ensemble_cases as ec
from gan_mpc_amd._lib import GmpcError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ctx", "B", "P", "dyn_members", "X", "U", "gd", "gD", "grad_x0", "grad_U", "grad_nominal", "grad_members",
        "stream"]


# ---- H1 ------------------------------------------------------------------------------------------------------------
def _torch_plan(nominal, members, x0, U):
    """disagreement_ref.plan in torch: -> (d (P, B, T), D (P, B))."""
    def mlp(layers, q):
        for W, b in layers[:-1]:
            q = torch.relu(q @ W + b)
        W, b = layers[-1]
        return q @ W + b

    x, d = x0, []
    for t in range(U.shape[1]):
        q = torch.cat([x, U[:, t]], -1)
        o0 = mlp(nominal, q)
        d.append(torch.stack([((mlp(layers, q) - o0) ** 2).sum(-1) for layers in members]))
        x = o0 + x
    d = torch.stack(d, -1)
    return d, d.sum(-1)


def _flat(layers):
    return np.concatenate([np.concatenate([np.asarray(W).reshape(-1), np.asarray(b)]) for W, b in layers])


@pytest.mark.parametrize("which", vc.WHICH)
@pytest.mark.parametrize("name", ["base", "m1", "ragged"])
def test_h1_the_fp64_reference_is_torch_autograd_of_the_plan(name, which):
    pb = ec.problem(name)
    nominal, members = vc.f64(pb["dyn"]), [vc.f64(layers) for layers in ec.members(name)]
    x0, U = pb["x0"].astype(np.float64), pb["U"].astype(np.float64)
    plan = dr.plan(nominal, members, x0, U)
    P, (B, T, _) = len(members), U.shape
    gd, gD = vc.cots(P, B, T, which, 3, np.float64)
    ref = vr.reference(nominal, members, plan["X"], U, gd, gD)
    leaf = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)  # noqa: E731
    tn = [(leaf(W), leaf(b)) for W, b in nominal]
    tm = [[(leaf(W), leaf(b)) for W, b in layers] for layers in members]
    tx, tU = leaf(x0), leaf(U)
    d, D = _torch_plan(tn, tm, tx, tU)
    np.testing.assert_allclose(d.detach().numpy(), plan["d"], rtol=1e-12, atol=1e-300)
    loss = 0.0
    if gd is not None:
        loss = loss + (torch.as_tensor(gd) * d).sum()
    if gD is not None:
        loss = loss + (torch.as_tensor(gD) * D).sum()
    loss.backward()
    want = dict(x0=tx.grad.numpy(), U=tU.grad.numpy(), nominal=_flat([(W.grad, b.grad) for W, b in tn]),
                members=np.stack([_flat([(W.grad, b.grad) for W, b in layers]) for layers in tm]))
    for k in vr.KEYS:
        assert ref[k].dtype == np.float64 and ref[k].shape == want[k].shape, k
        e = gu.rel_err(ref[k], want[k])
        print(f"H1 {name} {which} {k}: {e:.3e}")
        assert np.abs(want[k]).max() > 0 and e <= 1e-9, (k, e)
    # the parts are the terms of the sums
    n = pb["n"]
    r = ref["q"].sum(0) + ref["qN"]
    np.testing.assert_allclose(ref["U"], r[..., n:] + ref["chain"][..., n:], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ref["x0"], r[:, 0, :n] + ref["lam"][:, 1] + ref["chain"][:, 0, :n], rtol=1e-12,
                               atol=1e-14)
    assert not ref["lam"][:, -1].any()


# ---- H2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "ragged"])
def test_h2_the_exact_properties_hold_in_the_fp32_reference(name):
    pb = ec.problem(name)
    nominal, members = pb["dyn"], list(ec.members(name))
    X = dr.plan(nominal, members, pb["x0"], pb["U"])["X"]
    P, (B, T, _) = 3, pb["U"].shape
    gd, gD = vc.cots(P, B, T, "both", 4)
    full = vr.reference(nominal, members, X, pb["U"], gd, gD)
    assert all(full[k].dtype == np.float32 for k in vr.KEYS)
    # every member equal to the nominal network: every output is exactly zero
    zero = vr.reference(nominal, [nominal] * 3, X, pb["U"], gd, gD)
    for k in vr.KEYS:
        assert not zero[k].any(), k
    # one equal member among three: its row and its q are exact zeros, the others' rows stay
    mixed = vr.reference(nominal, [members[0], nominal, members[2]], X, pb["U"], gd, gD)
    assert not mixed["members"][1].any() and not mixed["q"][1].any()
    for p in (0, 2):
        np.testing.assert_array_equal(mixed["members"][p], full["members"][p])
    # a member's row depends on neither P nor the other members' cotangents
    one = vr.reference(nominal, members[1:2], X, pb["U"], gd[1:2], gD[1:2])
    np.testing.assert_array_equal(one["members"][0], full["members"][1])
    zd, zD = np.zeros_like(gd), np.zeros_like(gD)
    zd[1], zD[1] = gd[1], gD[1]
    masked = vr.reference(nominal, members, X, pb["U"], zd, zD)
    np.testing.assert_array_equal(masked["members"][1], full["members"][1])
    assert not masked["members"][0].any() and not masked["members"][2].any()
    for k in ("x0", "U", "nominal"):
        np.testing.assert_array_equal(masked[k], one[k])
    # gD alone is gd = 0 plus gD
    a = vr.reference(nominal, members, X, pb["U"], None, gD)
    b = vr.reference(nominal, members, X, pb["U"], np.zeros_like(gd), gD)
    for k in vr.KEYS:
        np.testing.assert_array_equal(a[k], b[k])


# ---- H3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vc.CASES)
def test_h3_the_kink_filter_and_the_conditioning_cap_hold_on_the_reference(case):
    pb = vc.problem(case)
    B = pb["B"]
    x0, U = pb["x0"].astype(np.float64), pb["U"].astype(np.float64)
    X = dr.plan(vc.f64(pb["dyn"]), [vc.f64(layers) for layers in vc.members(case)], x0, U)["X"]
    ok = vc.kept(case, X, pb["U"])
    print(f"H3 {case}: {ok.sum()} of {B} problems kept")
    assert ok.sum() >= max(1, B // 2) and ok.sum() >= B - B // 2
    X, Uk = np.ascontiguousarray(X[ok]), np.ascontiguousarray(pb["U"][ok])
    for which in vc.WHICH:
        seed, _, _, _, tried = vc.pick_seed(case, X, Uk, which)
        print(f"H3 {case} {which}: seed {seed}, kappa of the seeds tried " + " ".join(f"{k:.3g}" for k in tried))
        assert seed is not None, (case, which, tried)


# ---- H4 ------------------------------------------------------------------------------------------------------------
def test_h4_the_entry_point_is_declared_and_bound():
    from gan_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    m = re.search(r"\bint\s+gmpc_ensemble_disagreement_vjp\s*\(([^)]*)\)\s*;", header)
    assert m, "gmpc_ensemble_disagreement_vjp is not declared in the header"
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in decl] == ARGS
    kinds = [C.c_void_p if "*" in a else C.c_int for a in decl]
    assert _lib.SIGNATURES["gmpc_ensemble_disagreement_vjp"] == (C.c_int, kinds)
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "gmpc_ensemble_disagreement_vjp")


class _Lib:
    def __init__(self):
        self.calls = []

    def gmpc_ensemble_disagreement_vjp(self, *args):
        self.calls.append(args)
        return 0


def _engine(n=5, m=2, T=8, dyn_count=10):
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx, eng.dyn_count = _Lib(), "ctx", dyn_count
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
    mem, X, U, gd, gD = z(3, 10), z(4, 9, 5), z(4, 8, 2), z(3, 4, 8), z(3, 4)
    out = eng.ensemble_disagreement_vjp(mem, X, U, gd, gD)
    assert list(out) == ["x0", "U", "nominal", "members"]
    assert [tuple(out[k].shape) for k in out] == [(4, 5), (4, 8, 2), (10,), (3, 10)]
    (call,) = eng.lib.calls
    assert len(call) == len(ARGS) and call[:3] == ("ctx", 4, 3) and call[12] == "stream"
    assert call[4] is X and call[5] is U and call[6] is gd and call[7] is gD
    for i, k in enumerate(out):
        assert call[8 + i] is out[k]
    part = eng.ensemble_disagreement_vjp(mem, X, U, gD=gD, want=("members", "U"))
    assert list(part) == ["U", "members"]
    call = eng.lib.calls[1]
    assert call[6] is None and call[7] is gD
    assert call[8] is None and call[9] is part["U"] and call[10] is None and call[11] is part["members"]
    assert list(eng.ensemble_disagreement_vjp(mem, X, U, gd, want="nominal")) == ["nominal"]


def test_h4_the_engine_refuses_before_the_library_is_called():
    eng = _engine()
    z = torch.zeros
    good = dict(members=z(3, 10), X=z(4, 9, 5), U=z(4, 8, 2), gd=z(3, 4, 8), gD=z(3, 4))
    cases = [
        (dict(members=z(3, 11)), "members must be"),
        (dict(members=z(17, 10)), "P = 17"),
        (dict(members=z(0, 10)), "P = 0"),
        (dict(members=z(3, 10, dtype=torch.float64)), "float32"),
        (dict(want=("x0", "theta")), "unknown entries"),
        (dict(want=()), "want is empty"),
        (dict(gd=None, gD=None), "gd and gD are both None"),
        (dict(X=z(3, 4, 9, 5)), "X must be (B, 9, 5)"),
        (dict(X=z(4, 8, 5)), "X must be"),
        (dict(X=z(4, 9, 5, dtype=torch.float64)), "X must be a float32 tensor"),
        (dict(U=z(3, 8, 2)), "U must be (4, 8, 2)"),
        (dict(U=z(4, 7, 2)), "U must be"),
        (dict(U=np.zeros((4, 8, 2), np.float32)), "U must be a float32 tensor"),
        (dict(gd=z(3, 4, 9)), "gd must be (3, 4, 8)"),
        (dict(gd=z(2, 4, 8)), "gd must be"),
        (dict(gD=z(3, 5)), "gD must be (3, 4)"),
        (dict(gD=z(3, 4, dtype=torch.float64)), "gD must be a float32 tensor"),
    ]
    for change, msg in cases:
        with pytest.raises(GmpcError, match="ensemble disagreement vjp: .*" + re.escape(msg)):
            eng.ensemble_disagreement_vjp(**dict(good, **change))
    assert eng.lib.calls == []
