"""gmpc_critic_dir_vjp (the second-order VJP of the critic's scores) on the GPU: every case of tests/critic_cases.py off
the wide-input route against the fp32 and fp64 double-backward reference (tests/critic_dir_ref.py) under
test_critic_vjp_sweep's protocol; bits under repetition, linear scaling, zero rows and skipped outputs; consistency with
gmpc_critic_score_vjp and the symmetry of the second derivative; engine reuse; the ordering contract; the refusals;
critic_layer differentiated twice; GAN_MPC's gradient penalties and one CriticTrainer update with one.

The call recomputes the primal forward in its own sweep (it reuses none of the other critic kernels' forwards), so
`score` is compared with gmpc_critic_score_vjp's to parity on every route, not bit for bit."""

import numpy as np
import pytest
import torch

import critic_cases as cc
import critic_dir_ref as D
import critic_vjp_ref as V
import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_bilevel_cotangent as cot
import test_gpu_critic_sweep as sweep
import test_gpu_critic_vjp as tv
import test_gpu_input_grads as ig
from gan_mpc_amd import optim, params as P
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.gan import critic_trainer, gan_policy, js_policy
from gan_mpc_amd.policy import differentiable as dl

pytestmark = pytest.mark.gpu

NARROW = [c for c in cc.CASES if cc.critic_route(c[0], c[1])[0] != "wide"]
ROUTES = ("gen2", "gen1", "generic")
_same_bits = tv._same_bits


def _dir(eng, crit, xseq, v, g=None, **kw):
    out = eng.critic_dir_vjp(eng.to_dev(xseq), crit, eng.to_dev(v), None if g is None else eng.to_dev(g), **kw)
    return {k: None if t is None else t.cpu().numpy() for k, t in out.items()}


# ---- 1. parity on every case off the wide-input route --------------------------------------------------------------
def test_the_sweep_has_every_narrow_case():
    """Every case of the table that is off the wide-input route: 17 gen2, 5 gen1 and 8 generic ones, 30 in all."""
    wide = [c for c in cc.CASES if cc.critic_route(c[0], c[1])[0] == "wide"]
    assert len(NARROW) == 30 and len(NARROW) + len(wide) == len(cc.CASES)
    assert {cc.critic_route(c[0], c[1])[0] for c in NARROW} == set(ROUTES)


@pytest.mark.parametrize("case", NARROW, ids=cc.case_id)
def test_critic_dir_vjp_sweep(case):
    n, F, T, Bc, head, _ = case
    pb, xseq, _, _ = cc.make_case(case)
    cr64 = orc.cast_problem(pb, np.float64)["critic"]
    v, g = D.case_v(case), D.case_gdir(case)
    gu.set_config(f"critic dir vjp {cc.case_id(case)}")
    x64, v64, g64 = xseq.astype(np.float64), v.astype(np.float64), g.astype(np.float64)
    assert np.abs(orc.critic_forward(cr64, x64)).max() < cc.SCORE_MAX
    assert not cc.head_kinks(cr64, x64).any(), "a head row sits at a relu kink"
    eng = gu.engine_for(pb)
    assert eng.max_batch == (Bc + 1) // 2
    try:
        out = _dir(eng, eng.to_dev(gu.critic_flat(pb)), xseq, v, g)       # one call, all four outputs
    finally:
        eng.close()
    dims = (F,) + tuple(head) + (1,)
    s32, sd32, p32, d32 = D.dir_vjp(gu.critic_flat(pb), n, F, dims, xseq, v, g, dtype=np.float32)
    s64, sd64, p64, d64 = D.dir_vjp(V.flat_of(cr64), n, F, dims, x64, v64, g64)
    sens = D.sensitivity(case, v, g)
    gu.assert_parity("score", out["score"], s32, s64)
    gu.assert_parity("sdot", out["sdot"], sd32, sd64, el_tol=max(1e-3, 4 * sens["sdot"]))
    gu.assert_parity("critic dir vjp grad", out["params"] / Bc, p32 / Bc, p64 / Bc)
    blocks = [gu.split_critic_flat(a, n, F, dims) for a in (out["params"] / Bc, p32 / Bc, p64 / Bc)]
    for (name, a), (_, b32), (_, b64) in zip(*blocks):
        if name.startswith("head") and name.endswith(".b"):
            assert np.abs(b64).max() == 0 and np.abs(b32).max() == 0
            assert np.array_equal(a, np.zeros_like(a)), f"{name}: the head biases reach sdot through the masks only"
            continue
        gu.assert_parity(f"critic dir vjp grad {name}", a, b32, b64, el_tol=max(1e-3, 4 * sens[name]))
    dx = out["dx"]
    gu.assert_parity("g dsdot/dx", dx, d32, d64, el_tol=max(1e-3, 4 * sens["dx"]))
    gu.assert_parity("g dsdot/dx t=0", dx[:, 0], d32[:, 0], d64[:, 0], el_tol=max(1e-3, 4 * sens["dx t=0"]))
    gu.assert_parity("g dsdot/dx t=T1-1", dx[:, -1], d32[:, -1], d64[:, -1],
                     el_tol=max(1e-3, 4 * sens["dx t=T1-1"]))


# ---- 2. bits -------------------------------------------------------------------------------------------------------
ROUTE_BC = [(r, 7) for r in ROUTES] + [("gen2", 3), ("gen2", 9)]


@pytest.mark.parametrize("route,Bc", ROUTE_BC, ids=[f"{r}-Bc{b}" for r, b in ROUTE_BC])
def test_bits(route, Bc):
    n, F, T, head = sweep.ROUTE_CASES[route]
    assert cc.critic_route(n, F)[0] == route
    pb = sweep._small_problem(n, F, T, (Bc + 1) // 2, head, seed=60)
    gu.set_config(f"critic dir vjp bits {route} n={n} F={F} T={T} Bc={Bc}")
    rng = np.random.default_rng(62)
    x = rng.standard_normal((Bc, T + 1, n)).astype(np.float32)
    v = rng.standard_normal((Bc, T + 1, n)).astype(np.float32)
    g = rng.standard_normal(Bc).astype(np.float32)
    v[1] = 0.0
    g[2] = 0.0
    eng = gu.engine_for(pb)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        both = _dir(eng, crit, x, v, g)
        again = _dir(eng, crit, x, v, g)
        dx_only = _dir(eng, crit, x, v, g, want_params=False)
        par_only = _dir(eng, crit, x, v, g, want_dx=False)
        fwd = _dir(eng, crit, x, v)
        v2 = _dir(eng, crit, x, 2 * v, g)
        g2 = _dir(eng, crit, x, v, 2 * g)
    finally:
        eng.close()
    for key in ("score", "sdot", "dx", "params"):
        _same_bits(again[key], both[key], f"{key}: two identical calls")
    assert dx_only["params"] is None and par_only["dx"] is None and fwd["dx"] is None and fwd["params"] is None
    _same_bits(dx_only["dx"], both["dx"], "dx: dx only against both outputs")
    _same_bits(par_only["params"], both["params"], "params: params only against both outputs")
    for key in ("score", "sdot"):
        for name, other in (("dx only", dx_only), ("params only", par_only), ("forward only", fwd)):
            _same_bits(other[key], both[key], f"{key}: {name} against both outputs")
    _same_bits(v2["score"], both["score"], "score at 2 v")
    for key in ("sdot", "dx", "params"):
        _same_bits(v2[key], 2 * both[key], f"{key} at 2 v")
    _same_bits(g2["sdot"], both["sdot"], "sdot at 2 g_dir")
    for key in ("dx", "params"):
        _same_bits(g2[key], 2 * both[key], f"{key} at 2 g_dir")
    assert both["sdot"][1] == 0 and np.abs(both["dx"][1]).max() == 0, "v_b = 0"
    assert both["sdot"][2] != 0 and np.abs(both["dx"][2]).max() == 0, "g_dir_b = 0"
    assert np.abs(both["dx"][0]).max() > 0 and np.abs(both["params"]).max() > 0


# ---- 3. consistency ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_sdot_is_the_score_vjps_input_gradient_along_v_and_the_second_derivative_is_symmetric(route):
    n, F, T, head = sweep.ROUTE_CASES[route]
    Bc = 7
    pb = sweep._small_problem(n, F, T, (Bc + 1) // 2, head, seed=60)
    gu.set_config(f"critic dir vjp consistency {route}")
    rng = np.random.default_rng(63)
    x, v, w = (rng.standard_normal((Bc, T + 1, n)).astype(np.float32) for _ in range(3))
    one = np.ones(Bc, np.float32)
    eng = gu.engine_for(pb)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        score1, dx1 = [a.cpu().numpy() for a in eng.critic_score_vjp(eng.to_dev(x), crit)]
        at_v, at_w = _dir(eng, crit, x, v, one, want_params=False), _dir(eng, crit, x, w, one, want_params=False)
    finally:
        eng.close()
    flat32, dims = gu.critic_flat(pb), (F,) + tuple(head) + (1,)
    flat64 = V.flat_of(orc.cast_problem(pb, np.float64)["critic"])
    x64, v64, w64 = (a.astype(np.float64) for a in (x, v, w))
    s32, sd32, _, dv32 = D.dir_vjp(flat32, n, F, dims, x, v, one, dtype=np.float32)
    s64, sd64, _, dv64 = D.dir_vjp(flat64, n, F, dims, x64, v64, one.astype(np.float64))
    gu.assert_parity("score against critic_score_vjp's", at_v["score"], score1, s64)
    gu.assert_parity("sdot = <dx1, v>", at_v["sdot"], np.sum(dx1.astype(np.float64) * v64, axis=(1, 2)), sd64)
    dw32 = D.dir_vjp(flat32, n, F, dims, x, w, one, dtype=np.float32)[3]

    def asym(dv, dw):
        a = np.sum(dv.astype(np.float64) * w64, axis=(1, 2))
        b = np.sum(dw.astype(np.float64) * v64, axis=(1, 2))
        return float(np.abs(a - b).max() / np.abs(a).max())
    bar = max(1e-5, 4 * asym(dv32, dw32))
    got = asym(at_v["dx"], at_w["dx"])
    assert got <= bar, f"<dx(v), w> against <dx(w), v>: {got:.3e}, bar {bar:.3e}"


# ---- 4. engine reuse -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_engine_reuse_with_a_smaller_batch(route):
    n, F, T, head = sweep.ROUTE_CASES[route]
    M = 9
    pb = sweep._small_problem(n, F, T, M, head, seed=70)
    gu.set_config(f"critic dir vjp reuse {route} n={n} F={F} T={T} max_batch={M}")
    rng = np.random.default_rng(73)
    data = {Bc: (rng.standard_normal((Bc, T + 1, n)).astype(np.float32),
                 rng.standard_normal((Bc, T + 1, n)).astype(np.float32), rng.standard_normal(Bc).astype(np.float32))
            for Bc in (2 * M, 3)}
    eng = gu.engine_for(pb, max_batch=M)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        small_first = _dir(eng, crit, *data[3])             # the call workspace starts small and grows
        _dir(eng, crit, *data[2 * M])
        reused = _dir(eng, crit, *data[3])
    finally:
        eng.close()
    fresh = gu.engine_for(pb, max_batch=M)
    try:
        ref = _dir(fresh, fresh.to_dev(gu.critic_flat(pb)), *data[3])
    finally:
        fresh.close()
    for key in ("score", "sdot", "dx", "params"):
        _same_bits(reused[key], ref[key], f"{key}: Bc=3 after Bc={2 * M}")
        _same_bits(small_first[key], ref[key], f"{key}: Bc=3 first")


# ---- 5. ordering contract ------------------------------------------------------------------------------------------
def test_read_only_between_solve_and_bilevel_calls():
    from gan_mpc_amd.policy import optimizers as opt
    pb, _, eng, out, B = cot._solved("tiny-ragged", critic=True)
    _, lx, lu = opt.loss_cotangents(cot.huber_u_loss, out["X"], out["U"], None, (pb["true_seq"],))
    crit = eng.to_dev(gu.critic_flat(pb))
    xs = out["X"][..., :eng.nx].contiguous()
    rng = np.random.default_rng(5)
    v = eng.to_dev(rng.standard_normal(tuple(xs.shape)).astype(np.float32))
    g = eng.to_dev(rng.standard_normal(B).astype(np.float32))

    def vjp():
        return {k: t.cpu().numpy() for k, t in eng.critic_dir_vjp(xs, crit, v, g).items()}

    def chain(where):
        res = {}
        if where == "before":
            vjp()
        res["cot"] = eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0).cpu().numpy()
        if where == "between":
            vjp()
        res["x0"], res["goal"] = [a.cpu().numpy() for a in eng.bilevel_grad_inputs(B, lx)]
        if where == "between":
            vjp()
        res["loss"], res["js"] = [a.cpu().numpy() for a in eng.bilevel_grad(B, 1, critic=crit, sign=-1.0)]
        res["state"] = ig._state(eng, B)
        return res

    try:
        plain = chain(None)
        first = vjp()
        for where in ("between", "before"):
            mixed = chain(where)
            for key in ("cot", "x0", "goal", "loss", "js"):
                np.testing.assert_array_equal(mixed[key], plain[key], err_msg=f"{key} ({where})")
            for key in plain["state"]:
                np.testing.assert_array_equal(mixed["state"][key], plain["state"][key], err_msg=f"{key} ({where})")
        after = vjp()
    finally:
        eng.close()
    for key in ("score", "sdot", "dx", "params"):
        np.testing.assert_array_equal(after[key], first[key], err_msg=key)
    assert np.abs(first["params"]).max() > 0


# ---- 6. refusals ---------------------------------------------------------------------------------------------------
def test_refusals():
    n, F, T, M = 5, 64, 3, 4
    pb = sweep._small_problem(n, F, T, M, (17,), seed=50)
    eng = gu.engine_for(pb)
    d = eng.to_dev
    rng = np.random.default_rng(52)
    Bc = 2 * M
    x = d(rng.standard_normal((Bc, T + 1, n)).astype(np.float32))
    v = d(rng.standard_normal((Bc, T + 1, n)).astype(np.float32))
    g = d(rng.standard_normal(Bc).astype(np.float32))
    crit = d(gu.critic_flat(pb))
    score, sdot, dx, gs = eng.new(Bc), eng.new(Bc), eng.new(Bc, T + 1, n), eng.new(eng.critic_count)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def raw(Bc_, x_, crit_, v_, g_, sdot_, dx_, gs_, e=None):
        e = e or eng
        rc = e.lib.gmpc_critic_dir_vjp(e.ctx, Bc_, ptr(x_), ptr(crit_), ptr(v_), ptr(g_), ptr(score), ptr(sdot_),
                                       ptr(dx_), ptr(gs_), None)
        assert rc == -1, rc                   # GMPC_EINVAL
        return e.lib.gmpc_last_error().decode()

    def ok():
        out = eng.critic_dir_vjp(x, crit, v, g)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in out.values())
        return out

    try:
        want = ok()
        assert "xseq is null" in raw(Bc, None, crit, v, g, sdot, dx, gs)
        assert "critic is null" in raw(Bc, x, None, v, g, sdot, dx, gs)
        assert "v_xseq is null" in raw(Bc, x, crit, None, g, sdot, dx, gs)
        assert "sdot is null" in raw(Bc, x, crit, v, g, None, dx, gs)
        for dx_, gs_ in ((dx, gs), (dx, None), (None, gs)):
            assert "g_dir is null" in raw(Bc, x, crit, v, None, sdot, dx_, gs_)
        for bad in (0, Bc + 1):
            msg = raw(bad, x, crit, v, g, sdot, dx, gs)
            assert f"Bc={bad} outside" in msg and f"2*max_batch={Bc}" in msg
        with pytest.raises(GmpcError, match="v must be"):
            eng.critic_dir_vjp(x, crit, v[:, :-1].contiguous(), g)
        with pytest.raises(GmpcError, match="g_dir must be"):
            eng.critic_dir_vjp(x, crit, v, g[:-1].contiguous())
        with pytest.raises(GmpcError, match="xseq must be"):
            eng.critic_dir_vjp(x[:, :-1].contiguous(), crit, v, g)
        with pytest.raises(GmpcError, match="grad_sum must be"):
            eng.critic_dir_vjp(x, crit, v, None, grad_sum=gs)
        bare = gu.engine_for(pb, critic=False)
        try:
            assert "without a critic" in raw(Bc, x, crit, v, g, sdot, dx, gs, e=bare)
        finally:
            bare.close()
        # the wide-input route is this call's stated limit
        wn, wT = 193, 2
        wide = gu.engine_for(sweep._small_problem(wn, F, wT, M, (17,), seed=53))
        try:
            assert cc.critic_route(wn, F)[0] == "wide"
            wx = wide.new(Bc, wT + 1, wn).zero_()
            msg = raw(Bc, wx, wide.new(wide.critic_count).zero_(), wx, g, sdot, None, None, e=wide)
            assert "unsupported shape" in msg and "193" in msg and "64" in msg
        finally:
            wide.close()
        again = ok()
        for key in want:
            assert torch.equal(again[key], want[key]), key
    finally:
        eng.close()


# ---- 7. the torch layer --------------------------------------------------------------------------------------------
def _layer_setup(Bc=5, seed=90):
    config, policy, params, data = tv._build(js_policy.JS_MPC)
    dparams = policy.to_device_params(params)
    eng = policy.bind(dparams, Bc)
    n, T = eng.nx, eng.T
    x = np.random.default_rng(seed).standard_normal((Bc, T + 1, n)).astype(np.float32)
    cr = P.critic_tree_to_dict(params["critic_params"])
    cr64 = orc.cast_problem(dict(c=cr), np.float64)["c"]
    assert np.abs(orc.critic_forward(cr64, x.astype(np.float64))).max() < cc.SCORE_MAX
    assert not cc.head_kinks(cr64, x.astype(np.float64)).any()
    return policy, dparams, eng, x, cr, cr64


def _penalty_ref(flat, n, F, dims, x, target, dtype):
    fl = torch.as_tensor(np.asarray(flat, dtype)).requires_grad_(True)
    xs = torch.as_tensor(np.asarray(x, dtype)).requires_grad_(True)
    g, = torch.autograd.grad(V.forward_t(fl, n, F, dims, xs).sum(), xs, create_graph=True)
    nrm = torch.linalg.vector_norm(g.reshape(len(x), -1), dim=1)
    gp, gx = torch.autograd.grad(((nrm - target) ** 2).sum(), (fl, xs))
    return nrm.detach().numpy(), gp.numpy(), gx.numpy()


def test_critic_layer_differentiates_twice():
    policy, dparams, eng, x, cr, cr64 = _layer_setup()
    Bc, n, F = x.shape[0], eng.nx, eng.shape.lstm_features
    dims = tuple(eng.shape.head_dims[:eng.shape.head_layers + 1])
    gu.set_config("critic_layer twice")
    dparams.flat.requires_grad_(True)
    xs = eng.to_dev(x).requires_grad_(True)
    score = dl.critic_layer(policy, dparams, xs)
    g, = torch.autograd.grad(score.sum(), xs, create_graph=True)
    assert g.requires_grad and g.grad_fn is not None
    nrm = torch.linalg.vector_norm(g.reshape(Bc, -1), dim=1)
    ((nrm - 1.0) ** 2).sum().backward()
    grad, gx = dparams.flat.grad.cpu().numpy(), xs.grad.cpu().numpy()
    lo, cnt = dparams.range_of(("critic_params",))
    rest = np.ones(grad.shape, bool)
    rest[lo:lo + cnt] = False
    assert np.abs(grad[rest]).max() == 0
    n32, p32, x32 = _penalty_ref(V.flat_of(cr, np.float32), n, F, dims, x, 1.0, np.float32)
    n64, p64, x64 = _penalty_ref(V.flat_of(cr64), n, F, dims, x.astype(np.float64), 1.0, np.float64)
    assert n64.min() >= 1e-3
    gu.assert_parity("|dscore/dx|", nrm.detach().cpu().numpy(), n32, n64)
    gu.assert_parity("d penalty / d critic", grad[lo:lo + cnt], p32, p64)
    gu.assert_parity("d penalty / d xseq", gx, x32, x64)
    assert np.abs(p64).max() > 0 and np.abs(x64).max() > 0


def test_critic_layer_refuses_what_it_cannot_differentiate():
    policy, dparams, eng, x, _, _ = _layer_setup()
    dparams.flat.requires_grad_(True)
    xs = eng.to_dev(x).requires_grad_(True)
    gf, = torch.autograd.grad(dl.critic_layer(policy, dparams, xs).sum(), dparams.flat, create_graph=True)
    with pytest.raises(NotImplementedError, match="parameter gradient"):
        gf.sum().backward()
    # third derivatives
    g, = torch.autograd.grad(dl.critic_layer(policy, dparams, xs).sum(), xs, create_graph=True)
    h, = torch.autograd.grad((g ** 2).sum(), xs, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        h.sum().backward()


def test_critic_layer_without_create_graph_gives_critic_vjps_bits():
    policy, dparams, eng, x, _, _ = _layer_setup()
    Bc = x.shape[0]
    dparams.flat.requires_grad_(True)
    xs = eng.to_dev(x).requires_grad_(True)
    gs = eng.to_dev(np.random.default_rng(91).standard_normal(Bc).astype(np.float32))
    score = dl.critic_layer(policy, dparams, xs)
    score.backward(gs)
    assert xs.grad.grad_fn is None and not xs.grad.requires_grad
    crit = dparams.view("critic_params").detach()
    want = eng.critic_vjp(xs.detach(), crit, gs)
    lo, cnt = dparams.range_of(("critic_params",))
    assert torch.equal(dparams.flat.grad[lo:lo + cnt], want["params"]) and float(want["params"].abs().max()) > 0
    assert torch.equal(xs.grad, want["dx"]) and torch.equal(score.detach(), want["score"])


# ---- 8. GAN_MPC ----------------------------------------------------------------------------------------------------
PEN_SEED = {"gen2": 44, "generic": 44}


@pytest.mark.parametrize("route", ["gen2", "generic"])
@pytest.mark.parametrize("at,target", [("true", 0.0), ("mixed", 1.0)])
def test_gan_mpc_gradient_penalty_against_the_reference(route, at, target):
    n, F, T, head = sweep.ROUTE_CASES[route]
    Bc, weight = 7, 10.0
    config, policy, params, _ = tv._build(gan_policy.GAN_MPC, N=n, T=T, F=F, hidden=head[0], ndata=2, objective="wgan",
                                          gradient_penalty=dict(weight=weight, target=target, at=at, seed=5))
    xs, lab, cr, cr64 = tv._critic_batch(policy, params, n, T, Bc, seed=PEN_SEED[route])
    gu.set_config(f"GAN_MPC wgan + gradient penalty at {at} {route}")
    P_ = int(min((lab > 0).sum(), (lab <= 0).sum()))
    replay = torch.Generator(device=policy.device())
    replay.set_state(policy.penalty_generator.get_state())
    eps = torch.rand(P_, generator=replay, device=policy.device(), dtype=torch.float32).cpu().numpy()
    loss, grads = policy.critic_loss_and_grad(xs, lab, params)
    assert cc.critic_route(policy._engine.nx, policy._engine.shape.lstm_features)[0] == route
    dims = (F,) + tuple(head) + (1,)
    l32, g32, _ = D.penalty_loss_grad(V.flat_of(cr, np.float32), n, F, dims, xs, lab, weight, target, at, eps,
                                      dtype=np.float32)
    l64, g64, norms = D.penalty_loss_grad(V.flat_of(cr64), n, F, dims, xs, lab, weight, target, at, eps)
    xhat = D.penalty_points(xs.astype(np.float64), lab.astype(np.float64), at, eps)
    assert len(norms) == len(xhat) == ((lab > 0).sum() if at == "true" else P_) and len(xhat) >= 3
    assert norms.min() >= 1e-3, norms
    assert not cc.head_kinks(cr64, xhat).any(), "a penalty point sits at a relu kink"
    plain = D.penalty_loss_grad(V.flat_of(cr64), n, F, dims, xs, lab, 0.0, target, at, eps)
    assert abs(l64 - plain[0]) > 1e-3 * abs(plain[0]) and np.abs(g64 - plain[1]).max() > 1e-3 * np.abs(g64).max(), \
        "the penalty must show in the loss and in the gradient"
    gu.assert_parity("wgan-gp critic loss", float(loss), l32, l64)
    gu.assert_parity("wgan-gp critic grad", grads.cpu().numpy(), g32, g64)


def test_gan_mpc_without_penalty_points_and_generator_step_are_unchanged():
    n, F, T, head = sweep.ROUTE_CASES["gen2"]
    Bc, B = 6, 2
    res = {}
    for spec in (None, dict(weight=10.0, at="mixed")):
        config, policy, params, data = tv._build(gan_policy.GAN_MPC, N=n, T=T, F=F, hidden=head[0], ndata=2,
                                                 objective="wgan", gradient_penalty=spec)
        xs, _, _, _ = tv._critic_batch(policy, params, n, T, Bc, seed=45)
        lab = -np.ones(Bc, np.float32)                       # predicted sequences only: P = 0
        loss, grads = policy.critic_loss_and_grad(xs, lab, params)
        idx = np.arange(B)
        policy.expert_model.select(idx)
        gl, gg = policy.generator_loss_and_grad(data["hist"][idx], params, (data["Y"][idx],))
        res[spec is None] = [a.cpu().numpy() for a in (loss, grads, gl, gg)]
    for name, a, b in zip(("critic loss", "critic grad", "generator loss", "generator grad"), res[False], res[True]):
        _same_bits(np.atleast_1d(a), np.atleast_1d(b), f"{name}: with a penalty spec against gradient_penalty=None")
    assert np.abs(res[True][1]).max() > 0 and np.abs(res[True][3]).max() > 0


def test_critic_trainer_update_with_a_gradient_penalty():
    config, policy, params, data = tv._build(gan_policy.GAN_MPC, N=4, M=2, T=6, hidden=16, ndata=24, objective="wgan",
                                             gradient_penalty=dict(weight=10.0))
    opt = optim.get_optimizer(list(params.keys()), config.mpc.train.critic.no_grads, 1e-2)
    dparams = policy.to_device_params(params)
    before = dparams.view("critic_params").clone()
    other = dparams.flat[:dparams.offsets["critic_params"]].clone()
    state0 = policy.penalty_generator.get_state().clone()
    ntr = 16
    ds = ((data["hist"][:ntr], data["Y"][:ntr]), (data["hist"][ntr:], data["Y"][ntr:]))
    new_params, _, tl, te, _ = critic_trainer.train((policy, opt), opt.init(dparams), dparams, ds, num_updates=1,
                                                    batch_size=8, key=1, id=0)
    assert len(tl) == 1 and len(te) == 1 and np.isfinite(tl).all() and np.isfinite(te).all()
    assert not torch.equal(before, new_params.view("critic_params"))
    assert torch.equal(other, new_params.flat[:new_params.offsets["critic_params"]])
    assert not torch.equal(state0, policy.penalty_generator.get_state()), "the update drew no eps: no penalty point?"
