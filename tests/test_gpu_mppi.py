"""gmpc_mppi_solve and gmpc_mppi_vjp on the GPU against tests/mppi_ref.py.  Forward: one update
at the GPU's own costs and samples (F1), three free-running iterations (F2), chaining and the traces bit for bit (F3),
independence from B and an untouched std (F4), a NaN problem (F5), the temperature's two limits (F6), the bounds (F7),
sequencing with a held iLQR solution (F8).  Backward: gmpc_mppi_vjp against float64 autograd of the torch
transcription (B1), chunking, determinism and NULL arguments (B2), policy.differentiable.mppi_layer (B3).  Then the
policy (P1) and the refusals (R).  Parity goes through gpu_util.assert_parity at its defaults: fp64 is the arbiter, the
fp32 restatement the yardstick."""

import functools

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu
import mppi_cases as mc
import mppi_ref as mr
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

ALL = ("costs", "weights", "samples")
LINKS = 5
NAMES = list(mc.CASES)
GRADS = ("x0", "U", "goal", "theta", "dyn")


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _args(eng, pb, B=None):
    d = eng.to_dev
    B = pb["B"] if B is None else B
    return d(pb["x0"][:B]), d(pb["U"][:B]), d(pb["goal"][:B])


def _solve(eng, name, x0, U, goal, K, lo=mc.LO, hi=mc.HI, **more):
    want = more.pop("want", ALL)
    off = more.pop("iter_offset", 0)
    return eng.mppi_solve(x0, U, goal, lo, hi, mc.kwargs(name, K, **more), init_std=mc.INIT_STD, want=want,
                          iter_offset=off, trace=True)


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Per case, computed once: LINKS chained calls of one iteration (each with the mean it started from), and the
    whole solves of 3 and of LINKS iterations."""
    pb = mc.problem(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        links, mean = [], U
        for i in range(LINKS):
            out = _solve(eng, name, x0, mean, goal, 1, iter_offset=i)
            rec = _np(out)
            rec["mean_in"] = mean.cpu().numpy()
            links.append(rec)
            mean = out["U"]
        whole = {K: _np(_solve(eng, name, x0, U, goal, K)) for K in (3, LINKS)}
        torch.cuda.synchronize()
    finally:
        eng.close()
    return links, whole


def _clip_objective(name):
    """The fp64 objective of clip(U_init) per problem."""
    p = orc.cast_problem(mc.problem(name), np.float64)
    return orc.objective(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], np.clip(p["U"], mc.LO, mc.HI), p["x0"])


# ---- F1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_f1_one_update_at_the_gpu_costs_and_samples(name):
    links, _ = _runs(name)
    for i, lk in enumerate(links[:3]):
        ref = {dt: mr.update(lk["samples"], lk["costs"], lk["mean_in"], mc.TEMPERATURE[name], 0.0, dt)
               for dt in (np.float32, np.float64)}
        e = gu.assert_parity(f"mppi weights link {i}", lk["weights"], ref[np.float32][1], ref[np.float64][1])
        f = gu.assert_parity(f"mppi mean link {i}", lk["U"], ref[np.float32][0], ref[np.float64][0])
        print(f"F1 {name} link {i}: weights HIP {e[0]:.3e} / fp32 {e[1]:.3e}, mean HIP {f[0]:.3e} / fp32 {f[1]:.3e}")
        np.testing.assert_allclose(lk["weights"].sum(axis=1), 1.0, rtol=1e-5)


def test_f1_update_with_more_elements_than_threads():
    """T m = 288 >= 256: k_mppi_update takes one element per thread (two for the first 32 threads) instead of staging
    blocks of samples, the path of every case above (T m <= 96)."""
    n, m, T, B, N = 4, 32, 9, 2, 40
    pb = gu.problem(n, m, T, B, seed=5, dyn_hidden=(32, 32), cost_hidden=(16,), cost_fout=4)
    kw = dict(num_samples=N, seed=mc.SEED, temperature=0.5, evolution_smoothing=0.2)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        one = eng.mppi_solve(x0, U, goal, mc.LO, mc.HI, dict(kw, max_iter=1), init_std=0.5, want=ALL)
        two = _np(eng.mppi_solve(x0, one["U"], goal, mc.LO, mc.HI, dict(kw, max_iter=1), init_std=0.5, want=ALL,
                                 iter_offset=1))
        whole = _np(eng.mppi_solve(x0, U, goal, mc.LO, mc.HI, dict(kw, max_iter=2), init_std=0.5, want=ALL))
        one = _np(one)
    finally:
        eng.close()
    ref = {dt: mr.update(one["samples"], one["costs"], pb["U"], 0.5, 0.2, dt) for dt in (np.float32, np.float64)}
    gu.assert_parity("mppi weights, T m = 288", one["weights"], ref[np.float32][1], ref[np.float64][1])
    gu.assert_parity("mppi mean, T m = 288", one["U"], ref[np.float32][0], ref[np.float64][0])
    for k in two:
        np.testing.assert_array_equal(whole[k], two[k], err_msg=k)


# ---- F2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_f2_three_free_running_iterations(name):
    _, whole = _runs(name)
    r32, _, r64, _ = mc.traces(name)
    for k in ("U", "X", "obj"):
        e = gu.assert_parity(f"mppi free run {k}", whole[3][k], r32[k], r64[k])
        print(f"F2 {name} {k}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")
    assert (whole[3]["obj"] < _clip_objective(name)).all()


# ---- F3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("K", [3, LINKS])
def test_f3_one_call_is_the_chain_of_single_iterations(name, K):
    links, whole = _runs(name)
    w, last = whole[K], links[K - 1]
    for k in ("U", "X", "obj", "costs", "weights", "samples"):
        np.testing.assert_array_equal(w[k], last[k], err_msg=k)
    for i in range(K):
        np.testing.assert_array_equal(w["means_trace"][i], links[i]["mean_in"], err_msg=f"means_trace {i}")
        np.testing.assert_array_equal(w["costs_trace"][i], links[i]["costs"], err_msg=f"costs_trace {i}")
        np.testing.assert_array_equal(links[i]["means_trace"][0], links[i]["mean_in"])


# ---- F4 / F5 ---------------------------------------------------------------------------------------------------------
def test_f4_a_problems_mean_does_not_depend_on_b_and_std_is_untouched():
    name = "m1"
    pb = mc.problem(name)
    _, whole = _runs(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb, 3)
        std = eng.to_dev(np.random.default_rng(0).uniform(0.3, 0.7, (3,) + U.shape[1:]).astype(np.float32))
        few = _np(_solve(eng, name, x0, U, goal, 3))
        own = eng.mppi_solve(x0, U, goal, mc.LO, mc.HI, mc.kwargs(name, 3), init_std=std)
        np.testing.assert_array_equal(own["std"].cpu().numpy(), std.cpu().numpy())
    finally:
        eng.close()
    for k in ("U", "X", "obj", "costs", "weights", "samples", "std"):
        np.testing.assert_array_equal(few[k], whole[3][k][:3], err_msg=k)
    assert (few["std"] == np.float32(mc.INIT_STD)).all()


def test_f5_a_nan_problem_keeps_its_mean_and_leaves_the_others_alone():
    name = "m1"
    pb = mc.problem(name)
    _, whole = _runs(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        x0 = x0.clone()
        x0[2] = float("nan")
        out = _np(_solve(eng, name, x0, U, goal, 3))
    finally:
        eng.close()
    np.testing.assert_array_equal(out["U"][2], pb["U"][2])
    assert (out["weights"][2] == 0).all() and np.isnan(out["costs"][2]).all()
    keep = [b for b in range(pb["B"]) if b != 2]
    for k in ("U", "X", "obj", "costs", "weights", "samples"):
        np.testing.assert_array_equal(out[k][keep], whole[3][k][keep], err_msg=k)


# ---- F6 --------------------------------------------------------------------------------------------------------------
def _seq_mean(s, dt):
    acc = np.zeros(s.shape[:1] + s.shape[2:], dt)
    for i in range(s.shape[1]):
        acc = acc + s[:, i].astype(dt)
    return acc / dt(s.shape[1])


def test_f6_temperature_limits():
    name = "base"
    pb = mc.problem(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        hot = _np(_solve(eng, name, x0, U, goal, 1, temperature=1e30))
        # the costs do not depend on the temperature: find the one at which the fp64 weights are one-hot
        c64 = hot["costs"].astype(np.float64)
        lam = mc.TEMPERATURE[name]
        while True:
            w, _ = mr.weights(c64, lam, np.float64)
            if ((w / w.sum(axis=1, keepdims=True)).max(axis=1) > 1 - 1e-6).all():
                break
            lam /= 2
        cold = _np(_solve(eng, name, x0, U, goal, 1, temperature=lam))
    finally:
        eng.close()
    gu.assert_parity("mppi mean at temperature 1e30", hot["U"], _seq_mean(hot["samples"], np.float32),
                     _seq_mean(hot["samples"], np.float64))
    np.testing.assert_array_equal(cold["costs"], hot["costs"])
    two = np.sort(c64, axis=1)[:, :2]
    sure = (two[:, 1] - two[:, 0]) / np.abs(two[:, 0]) > 1e-5
    assert sure.any()
    best = np.argmin(c64, axis=1)
    pick = np.stack([cold["samples"][b, best[b]] for b in range(pb["B"])])
    gu.assert_parity("mppi mean at a one-hot temperature", cold["U"][sure], pick[sure], pick[sure].astype(np.float64))


# ---- F7 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_f7_samples_and_mean_inside_the_bounds(name):
    links, whole = _runs(name)
    for rec in links + list(whole.values()):
        assert (rec["samples"] >= np.float32(mc.LO)).all() and (rec["samples"] <= np.float32(mc.HI)).all()
        # gamma = 0: the mean is a convex combination of samples inside the bounds
        assert (rec["U"] >= mc.LO - 1e-6).all() and (rec["U"] <= mc.HI + 1e-6).all()


def test_f7_one_sided_and_absent_bounds_are_the_clamp_of_the_free_samples():
    name = "base"
    pb = mc.problem(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        s = {k: _np(_solve(eng, name, x0, U, goal, 1, lo=lo, hi=hi, want=("samples",)))["samples"]
             for k, (lo, hi) in dict(free=(None, None), lo=(-0.3, None), hi=(None, 0.2), both=(-0.3, 0.2)).items()}
        with pytest.raises(GmpcError, match="mppi: .*init_std"):
            eng.mppi_solve(x0, U, goal, -0.3, None, mc.kwargs(name, 1))
    finally:
        eng.close()
    lo, hi = np.float32(-0.3), np.float32(0.2)
    assert (s["free"] < lo).any() and (s["free"] > hi).any()
    np.testing.assert_array_equal(s["lo"], np.maximum(s["free"], lo))
    np.testing.assert_array_equal(s["hi"], np.minimum(s["free"], hi))
    np.testing.assert_array_equal(s["both"], np.clip(s["free"], lo, hi))


# ---- F8 --------------------------------------------------------------------------------------------------------------
def test_f8_a_held_solution_survives_the_solve():
    name = "base"
    pb = mc.problem(name)
    B = pb["B"]

    def tail(with_mppi):
        eng = gu.engine_for(pb, critic=False)
        try:
            x0, U, goal = _args(eng, pb)
            sol = eng.ilqr_solve(x0, U, goal, {"maxiter": 3})
            out = _np(_solve(eng, name, x0, U, goal, 3)) if with_mppi else None
            loss, grad = eng.bilevel_grad(B, 0, desired=eng.to_dev(pb["true_seq"]))
            return _np(sol), loss.cpu().numpy(), grad.cpu().numpy(), out
        finally:
            eng.close()

    s0, l0, g0, _ = tail(False)
    s1, l1, g1, out = tail(True)
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    np.testing.assert_array_equal(l0, l1)
    np.testing.assert_array_equal(g0, g1)
    _, whole = _runs(name)
    for k in out:       # the same call in another context, after another solve
        np.testing.assert_array_equal(out[k], whole[3][k], err_msg=k)


# ---- B1 / B2 ---------------------------------------------------------------------------------------------------------
def _vjp(gname, max_batch=None, repeat=1, **want):
    name, K, more = mc.GRAD_CASES[gname]
    pb = mc.problem(name)
    (n, m, T, B, N, E), _ = mc.CASES[name]
    eng = gu.engine_for(pb, max_batch=max_batch or B * N, critic=False)
    try:
        d = eng.to_dev
        x0, U, goal = _args(eng, pb)
        kw = mc.kwargs(name, K, **more)
        sol = eng.mppi_solve(x0, U, goal, mc.LO, mc.HI, kw, init_std=mc.INIT_STD, trace=True)
        gX, gU, gobj = (d(a) for a in mc.cotangents(name))
        cot = dict(gX=gX, gU=gU, gobj=gobj)
        cot.update({k: want.pop(k) for k in list(want) if k in cot})
        outs = [eng.mppi_vjp(x0, goal, mc.LO, mc.HI, sol, kwargs=kw, **cot, **want) for _ in range(repeat)]
        outs = [{k: None if v is None else v.cpu().numpy() for k, v in o.items()} for o in outs]
        return outs if repeat > 1 else outs[0], _np(sol)
    finally:
        eng.close()


def _check_grads(gname, got, tag):
    g64, g32, _, _ = mc.grad_refs(gname)
    for k in GRADS:
        if got[k] is None:
            continue
        e = gu.assert_parity(f"mppi vjp {tag} {k}", got[k].reshape(g64[k].shape), g32[k], g64[k])
        print(f"{tag} {gname} {k}: HIP {e[0]:.3e}, torch fp32 {e[1]:.3e}")


@pytest.mark.parametrize("gname", list(mc.GRAD_CASES))
def test_b1_vjp_against_float64_autograd(gname):
    got, sol = _vjp(gname)
    _, _, fwd, _ = mc.grad_refs(gname)
    assert gu.rel_err(sol["U"], fwd[1]) < 1e-4       # the two forwards are the same solve
    _check_grads(gname, got, "B1")


@pytest.mark.parametrize("gname", ["base", "m1_smooth"])
def test_b2_two_chunks_are_the_same_gradient_and_deterministic(gname):
    name = mc.GRAD_CASES[gname][0]
    (n, m, T, B, N, E), _ = mc.CASES[name]
    chunk = (B + 1) // 2
    assert chunk < B
    outs, _ = _vjp(gname, max_batch=chunk * N + N - 1, repeat=2)
    _check_grads(gname, outs[0], "B2")
    for k in GRADS:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)


def test_b2_null_outputs_and_null_cotangents():
    gname = "m1"
    full, _ = _vjp(gname)
    for k in GRADS:
        want = {f"want_{j}": j == k for j in GRADS}
        one, _ = _vjp(gname, **want)
        assert all(one[j] is None for j in GRADS if j != k)
        np.testing.assert_array_equal(one[k], full[k], err_msg=k)
    # the VJP is linear in the cotangents: the three single-cotangent calls add up to the full one
    parts = [_vjp(gname, **{c: None for c in ("gX", "gU", "gobj") if c != keep})[0] for keep in ("gX", "gU", "gobj")]
    for k in GRADS:
        tot = sum(p[k].astype(np.float64) for p in parts)
        assert gu.rel_err(tot, full[k]) < 1e-5, k


# ---- B3 --------------------------------------------------------------------------------------------------------------
def test_b3_mppi_layer_matches_the_arbiter_and_leaves_the_held_solution_usable():
    import test_gpu_input_grads as ig
    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    from gan_mpc_amd.policy import differentiable as dl
    config, policy, params, data = mirror._build(l2_policy.L2MPC)
    policy.trajax_ilqr_kwargs["maxiter"] = 2
    idx = np.arange(3)
    B = len(idx)
    dparams, x0, goal, init_U = ig._layer_inputs(policy, params, data, idx)
    des = torch.as_tensor(np.asarray(data["Y"][idx], np.float32), device=x0.device)
    k = des.shape[-1]
    kw = dict(num_samples=48, max_iter=2, seed=3, temperature=0.5)
    # the policy's own engine holds an iLQR solution across the layer's forward and backward
    sol = policy._solve(dparams, data["hist"][idx])[1]
    eng = policy._engine
    before = eng.bilevel_grad(B, 0, desired=des)[1].cpu().numpy()
    flat = dparams.flat.requires_grad_(True)
    leaves = [t.clone().requires_grad_(True) for t in (x0, goal, init_U)]
    X, U, obj = dl.mppi_layer(policy, dparams, leaves[0], leaves[1], leaves[2], (-1.0, 1.0), kw, init_std=0.5,
                              dynamics_grad=True)
    loss = ((X[..., :k] - des) ** 2).sum() + obj.sum()
    loss.backward()
    after = eng.bilevel_grad(B, 0, desired=des)[1].cpu().numpy()
    np.testing.assert_array_equal(before, after)
    assert policy._rollout_eng[1] is not eng and policy._rollout_eng[1].max_batch >= 48
    pb = mirror._oracle_problem(params, data, idx, np.float32)
    ref = {}
    for dt in (torch.float64, torch.float32):
        lv = mr.leaves(pb, dt)
        Xr, Ur, objr = mr.torch_mppi(lv, -1.0, 1.0, kw, 0.5)
        L = ((Xr[..., :k] - torch.as_tensor(data["Y"][idx], dtype=dt)) ** 2).sum() + objr.sum()
        ref[dt] = mr.torch_grads(lv, L)
    g64, g32 = ref[torch.float64], ref[torch.float32]
    lo, cnt = dparams.range_of(("mpc_weights", "cost_params"))
    dlo, dcnt = dparams.range_of(("dynamics_params",))
    fg = flat.grad.cpu().numpy()
    got = dict(x0=leaves[0].grad, goal=leaves[1].grad, U=leaves[2].grad)
    got = {k_: v.cpu().numpy() for k_, v in got.items()}
    got["theta"], got["dyn"] = fg[lo:lo + cnt], fg[dlo:dlo + dcnt]
    for key in GRADS:
        e = gu.assert_parity(f"mppi_layer {key}", got[key], g32[key], g64[key])
        print(f"B3 {key}: HIP {e[0]:.3e}, torch fp32 {e[1]:.3e}")
    mask = np.ones(fg.shape, bool)
    mask[lo:lo + cnt] = False
    mask[dlo:dlo + dcnt] = False
    assert (fg[mask] == 0).all() and np.abs(got["dyn"]).max() > 0
    flat.grad = None
    X2, _, _ = dl.mppi_layer(policy, dparams, x0, goal, init_U, (-1.0, 1.0), kw, init_std=0.5)
    (X2 * X2).sum().backward()
    fg = flat.grad.cpu().numpy()
    assert (fg[dlo:dlo + dcnt] == 0).all() and np.abs(fg[lo:lo + cnt]).max() > 0      # dynamics_grad=False
    flat.requires_grad_(False)
    del sol


# ---- P1 --------------------------------------------------------------------------------------------------------------
def test_p1_policy_actions_warm_start_and_training_calls():
    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    from gan_mpc_amd.policy import differentiable as diff
    bound = 0.3
    kw = dict(num_samples=64, max_iter=4, seed=7, temperature=0.5)

    def build(**more):
        _, policy, params, data = mirror._build(functools.partial(
            l2_policy.L2MPC, solver="mppi", control_bounds=(-bound, bound), mppi_kwargs=dict(kw, **more)))
        policy.expert_model.select(np.array([2]))
        return policy, params, data

    policy, params, data = build()
    assert policy.solver == "mppi" and policy.mppi_kwargs["num_samples"] == 64
    X, U, obj, grad, adj, lqr, itr = policy.get_optimal_values(params, data["hist"][2])
    assert grad is None and adj is None and lqr is None and int(itr) == 4
    assert tuple(U.shape) == (policy._engine.T, policy._engine.m)
    U = U.cpu().numpy()
    assert (np.abs(U) <= np.float32(bound)).all()
    a = policy.get_optimal_action(params, data["hist"][2]).cpu().numpy()
    assert (np.abs(a) <= np.float32(bound)).all()
    assert policy.mppi_solves == 2 and not np.array_equal(a, U[0])      # the second solve ran under seed + 1
    # warm start: the second call starts from the first one's U shifted, not from the expert's
    warm, wparams, _ = build(warm_start=True)
    U1 = warm.get_optimal_values(wparams, data["hist"][2])[1].cpu().numpy()
    np.testing.assert_array_equal(U1, U)                                # the first solve has nothing to start from
    a_warm = warm.get_optimal_action(wparams, data["hist"][2]).cpu().numpy()
    assert not np.array_equal(a_warm, a)
    warm.mppi_solves = 1
    warm.reset_warm_start()
    np.testing.assert_array_equal(warm.get_optimal_action(wparams, data["hist"][2]).cpu().numpy(), a)
    policy.expert_model.select(np.arange(4))
    with pytest.raises(NotImplementedError, match="mppi_layer"):
        policy.loss_and_grad(data["hist"][:4], params, (data["Y"][:4],))
    with pytest.raises(NotImplementedError, match="mppi_layer"):
        policy.batch_loss(params, data["hist"][:4], data["Y"][:4])
    with pytest.raises(NotImplementedError, match="mppi_layer"):
        diff.ilqr_layer(policy, params, None, None, None)
    assert policy.mppi_solves == 2


# ---- R ---------------------------------------------------------------------------------------------------------------
def _refused(pb, kw, vjp=False, max_batch=None, **more):
    eng = gu.engine_for(pb, max_batch=max_batch, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        if not vjp:
            return eng.mppi_solve(x0, U, goal, mc.LO, mc.HI, kw, init_std=0.5, **more)
        K, N = max(int(kw.get("max_iter", 1)), 0), max(int(kw.get("num_samples", 32)), 0)
        sol = dict(U=U, X=eng.new(pb["B"], pb["T"] + 1, pb["n"]), std=torch.full_like(U, 0.5),
                   means_trace=eng.new(K, *U.shape), costs_trace=eng.new(K, pb["B"], N))
        more.setdefault("gU", torch.ones_like(U))
        return eng.mppi_vjp(x0, goal, mc.LO, mc.HI, sol, kwargs=kw, **more)
    finally:
        eng.close()


@pytest.mark.parametrize("vjp", [False, True])
@pytest.mark.parametrize("case", ["lstm", "n300", "nm257"])
def test_r_refused_shapes(case, vjp):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2),
                nm257=dict(n=250, m=7))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    args.setdefault("cost_hidden", (16,))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_fout=4, **args)
    with pytest.raises(GmpcError, match="mppi: "):
        _refused(pb, dict(num_samples=32, max_iter=1), vjp=vjp, max_batch=64)


@pytest.mark.parametrize("vjp", [False, True])
def test_r_refused_options(vjp):
    pb = mc.problem("m1")
    ok = dict(num_samples=32, max_iter=1)
    for bad in (dict(num_samples=4097), dict(num_samples=0), dict(max_iter=-1), dict(sampling_smoothing=1.0),
                dict(sampling_smoothing=-0.1), dict(evolution_smoothing=1.5), dict(evolution_smoothing=float("nan")),
                dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")),
                dict(temperature=float("inf"))):
        with pytest.raises(GmpcError, match="mppi: "):
            _refused(pb, dict(ok, **bad), vjp=vjp, max_batch=64)
    with pytest.raises(GmpcError, match="mppi: unknown"):
        _refused(pb, dict(ok, elite_portion=0.1), vjp=vjp, max_batch=64)
    if vjp:
        with pytest.raises(GmpcError, match="mppi: .*max_batch"):
            _refused(pb, ok, vjp=True, max_batch=31)
        with pytest.raises(GmpcError, match="mppi: every output"):
            _refused(pb, ok, vjp=True, max_batch=64, **{f"want_{k}": False for k in GRADS})
        with pytest.raises(GmpcError, match="mppi: .*no cotangent"):
            _refused(pb, ok, vjp=True, max_batch=64, gU=None)
    else:
        with pytest.raises(GmpcError, match="mppi: want"):
            _refused(pb, ok, want=("elites",))
        # max_iter = 0 is no refusal: the mean's own rollout, the mean untouched
        out = _refused(pb, dict(ok, max_iter=0))
        np.testing.assert_array_equal(out["U"].cpu().numpy(), pb["U"])
