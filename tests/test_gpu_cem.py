"""gmpc_cem_solve on the GPU against tests/cem_ref.py, link by link: the sampler (G1), the costs
at the GPU's own samples (G2), the elite selection (G3), the update at the GPU's own samples and elites (G4), the
chaining of iterations bit for bit (G5) -- together they pin the whole solve --, then three free-running iterations on
the decided problems (G6), the final mean's rollout (G7), the bounds (G8), independence from N and B (G9),
statelessness and determinism (G10), refusals and the policy (G11).  Parity goes through gpu_util.assert_parity at its
defaults: fp64 is the arbiter, the fp32 NumPy restatement the yardstick."""

import functools

import numpy as np
import pytest
import torch

import cem_cases as cc
import cem_ref as cr
import gan_mpc_oracle as orc
import gpu_util as gu
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

ALL = ("costs", "elites", "samples")
LINKS = 10          # chained one-iteration calls per case; the first CHECKED are checked link by link
CHECKED = 3
NAMES = list(cc.CASES)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _args(eng, pb, B=None):
    d = eng.to_dev
    B = pb["B"] if B is None else B
    return d(pb["x0"][:B]), d(pb["U"][:B]), d(pb["goal"][:B])


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Per case, computed once: `links` -- LINKS chained calls of one iteration (each with the mean / std it started
    from) --, and the whole solves of 3 and of 10 iterations."""
    pb = cc.problem(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        links, mean, std = [], U, None
        for i in range(LINKS):
            out = eng.cem_solve(x0, mean, goal, cc.LO, cc.HI, cc.engine_kwargs(name, 1), init_std=std, want=ALL,
                                iter_offset=i)
            rec = _np(out)
            rec["mean_in"] = mean.cpu().numpy()
            rec["std_in"] = (np.full_like(rec["mean_in"], (cc.HI - cc.LO) / 2) if std is None else std.cpu().numpy())
            links.append(rec)
            mean, std = out["U"], out["std"]
        whole = {K: _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, cc.engine_kwargs(name, K), want=ALL))
                 for K in (3, LINKS)}
        torch.cuda.synchronize()
    finally:
        eng.close()
    return links, whole


def _pb64(name):
    return orc.cast_problem(cc.problem(name), np.float64)


# ---- G1 --------------------------------------------------------------------------------------------------------------
def test_g1_samples_are_the_box_muller_of_the_philox_integers():
    name = "base"
    pb = cc.problem(name)
    (n, m, T, B, N, E), _ = cc.CASES[name]
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        zero = torch.zeros_like(U)
        outs = [_np(eng.cem_solve(x0, zero, goal, None, None, cc.engine_kwargs(name, 1), init_std=1.0,
                                  want=("samples",), iter_offset=it)) for it in (0, 1)]
    finally:
        eng.close()
    for it, out in enumerate(outs):
        z32 = np.stack([cr.normals(cc.CEM_SEED, it, b, np.arange(N), T * m, np.float32) for b in range(B)])
        z64 = np.stack([cr.normals(cc.CEM_SEED, it, b, np.arange(N), T * m, np.float64) for b in range(B)])
        e = gu.assert_parity(f"cem samples it={it}", out["samples"].reshape(B, N, T * m), z32, z64)
        print(f"G1 it={it}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")
    s0, s1 = outs[0]["samples"], outs[1]["samples"]
    assert not np.array_equal(s0, s1), "the stream does not depend on the iteration"
    assert not np.array_equal(s0[0], s0[1]), "the stream does not depend on the problem"
    assert not np.array_equal(s0[:, 0], s0[:, 1]), "the stream does not depend on the sample"
    flat = s0.reshape(-1)
    assert np.unique(flat).size > 0.99 * flat.size


def test_g1_smoothing_along_time_in_both_callers_of_the_helper():
    """sampling_smoothing > 0 takes the helper's recurrence from step 0: the samples against the smoothed normals,
    and the update -- which regenerates the elites' controls through the same helper -- at those samples."""
    name, beta = "base", 0.6
    pb = cc.problem(name)
    (n, m, T, B, N, E), _ = cc.CASES[name]
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        kw = cc.engine_kwargs(name, 1, sampling_smoothing=beta)
        free = _np(eng.cem_solve(x0, torch.zeros_like(U), goal, None, None, kw, init_std=1.0, want=("samples",)))
        one = eng.cem_solve(x0, U, goal, cc.LO, cc.HI, kw, want=ALL)
        two = _np(eng.cem_solve(x0, one["U"], goal, cc.LO, cc.HI, kw, init_std=one["std"], want=ALL, iter_offset=1))
        whole = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, cc.engine_kwargs(name, 2, sampling_smoothing=beta),
                                  want=ALL))
        one = _np(one)
    finally:
        eng.close()
    z = {dt: np.stack([cr.smooth(cr.normals(cc.CEM_SEED, 0, b, np.arange(N), T * m, dt).reshape(N, T, m), beta, dt)
                       for b in range(B)]) for dt in (np.float32, np.float64)}
    e = gu.assert_parity("cem smoothed samples", free["samples"], z[np.float32], z[np.float64])
    print(f"G1 smoothed: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")
    plain = np.stack([cr.normals(cc.CEM_SEED, 0, b, np.arange(N), T * m).reshape(N, T, m) for b in range(B)])
    assert gu.rel_err(free["samples"][:, :, 0], plain[:, :, 0]) < 1e-6          # step 0 is z_0 itself,
    assert gu.rel_err(free["samples"][:, :, 1:], plain[:, :, 1:]) > 0.1         # the later steps are not z_t
    for dt in (np.float32, np.float64):
        s = cr.draw(one["U"].astype(dt), one["std"].astype(dt), np.full(m, cc.LO), np.full(m, cc.HI), cc.CEM_SEED, 1,
                    N, beta, dt)
        z[dt] = s
    gu.assert_parity("cem smoothed clamped samples", two["samples"], z[np.float32], z[np.float64])
    ref = {dt: cr.update(two["samples"].astype(dt), two["costs"], one["U"].astype(dt), one["std"].astype(dt), E, 0.1,
                         dt, elites=two["elites"]) for dt in (np.float32, np.float64)}
    np.testing.assert_array_equal(two["elites"], cr.elites_of(two["costs"], E))
    gu.assert_parity("cem mean under smoothing", two["U"], ref[np.float32][0], ref[np.float64][0])
    gu.assert_parity("cem std under smoothing", two["std"], ref[np.float32][1], ref[np.float64][1])
    for k in two:
        np.testing.assert_array_equal(whole[k], two[k], err_msg=k)


# ---- G2 - G4: every link of the chain --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_g2_costs_at_the_gpu_samples(name):
    pb, pb64 = cc.problem(name), _pb64(name)
    links, _ = _runs(name)
    for i, lk in enumerate(links[:CHECKED]):
        c32, c64 = cr.sample_costs(pb, lk["samples"]), cr.sample_costs(pb64, lk["samples"].astype(np.float64))
        e = gu.assert_parity(f"cem costs link {i}", lk["costs"], c32, c64)
        print(f"G2 {name} link {i}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")


@pytest.mark.parametrize("name", NAMES)
def test_g3_elites_are_the_stable_argsort_of_the_gpu_costs(name):
    (n, m, T, B, N, E), _ = cc.CASES[name]
    links, _ = _runs(name)
    for lk in links:
        np.testing.assert_array_equal(lk["elites"], cr.elites_of(lk["costs"], E))


def test_g3_equal_costs_and_nan_costs():
    name = "base"
    pb = cc.problem(name)
    (n, m, T, B, N, E), _ = cc.CASES[name]
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        flat = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, cc.engine_kwargs(name, 1), init_std=0.0, want=ALL))
        ref = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, cc.engine_kwargs(name, 2), want=ALL))
        bad = x0.clone()
        bad[1, 0] = float("nan")
        nan = _np(eng.cem_solve(bad, U, goal, cc.LO, cc.HI, cc.engine_kwargs(name, 2), want=ALL))
    finally:
        eng.close()
    # std 0: every sample is the (clamped) mean, every cost equal, the order is the index
    assert (flat["costs"] == flat["costs"][:, :1]).all()
    np.testing.assert_array_equal(flat["elites"], np.tile(np.arange(E), (B, 1)))
    # a NaN x0: that problem's costs are NaN, its elites the first E, its mean finite; the others do not notice
    assert np.isnan(nan["costs"][1]).all()
    np.testing.assert_array_equal(nan["elites"][1], np.arange(E))
    assert np.isfinite(nan["U"][1]).all() and np.isfinite(nan["std"][1]).all()
    for k in ("X", "U", "obj", "std", "costs", "elites", "samples"):
        np.testing.assert_array_equal(nan[k][[0, 2]], ref[k][[0, 2]], err_msg=k)


@pytest.mark.parametrize("name", NAMES)
def test_g4_update_at_the_gpu_samples_and_elites(name):
    (n, m, T, B, N, E), _ = cc.CASES[name]
    links, _ = _runs(name)
    for i, lk in enumerate(links[:CHECKED]):
        ref = {}
        for dt in (np.float32, np.float64):
            ref[dt] = cr.update(lk["samples"].astype(dt), lk["costs"], lk["mean_in"].astype(dt),
                                lk["std_in"].astype(dt), E, 0.1, dt, elites=lk["elites"])
        e = gu.assert_parity(f"cem mean link {i}", lk["U"], ref[np.float32][0], ref[np.float64][0])
        f = gu.assert_parity(f"cem std link {i}", lk["std"], ref[np.float32][1], ref[np.float64][1])
        print(f"G4 {name} link {i}: mean HIP {e[0]:.3e} / fp32 {e[1]:.3e}, std HIP {f[0]:.3e} / fp32 {f[1]:.3e}")


# ---- G5 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("K", [3, LINKS])
def test_g5_one_call_is_the_chain_of_single_iterations(name, K):
    links, whole = _runs(name)
    for k in ("X", "U", "obj", "std", "costs", "elites", "samples"):
        np.testing.assert_array_equal(whole[K][k], links[K - 1][k], err_msg=f"{name} K={K}: {k}")


# ---- G6 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.DECIDED)
def test_g6_three_free_running_iterations_on_the_decided_problems(name):
    (n, m, T, B, N, E), _ = cc.CASES[name]
    links, whole = _runs(name)
    r32, t32, r64, t64 = cc.traces(name)
    ok = cr.decided(t32, t64, E)[2]
    print(f"G6 {name}: decided {int(ok.sum())} of {B}")
    if not ok.any():
        return
    for i in range(3):
        for b in np.nonzero(ok)[0]:
            assert set(links[i]["elites"][b]) == set(t64[i]["elites"][b]), (name, i, b)
    out = whole[3]
    e = gu.assert_parity("cem mean after 3", out["U"][ok], r32["U"][ok], r64["U"][ok])
    f = gu.assert_parity("cem std after 3", out["std"][ok], r32["std"][ok], r64["std"][ok])
    print(f"G6 {name}: mean HIP {e[0]:.3e} / fp32 {e[1]:.3e}, std HIP {f[0]:.3e} / fp32 {f[1]:.3e}")


# ---- G7 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_g7_rollout_and_objective_of_the_final_mean(name):
    pb, pb64 = cc.problem(name), _pb64(name)
    _, whole = _runs(name)
    out = whole[LINKS]
    U = out["U"]
    X32, X64 = orc.rollout(pb["dyn"], U, pb["x0"]), orc.rollout(pb64["dyn"], U.astype(np.float64), pb64["x0"])
    o32 = orc.objective(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], U, pb["x0"])
    o64 = orc.objective(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], U.astype(np.float64), pb64["x0"])
    gu.assert_parity("cem X of the mean", out["X"], X32, X64)
    gu.assert_parity("cem obj of the mean", out["obj"], o32, o64)
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        Xr, cr_ = eng.rollout_cost(d(pb["x0"]), d(U), d(pb["goal"]))
        Xr, objr = Xr.cpu().numpy(), cr_.cpu().numpy().astype(np.float64).sum(1)
    finally:
        eng.close()
    gu.assert_parity("cem X against rollout_cost", out["X"], Xr, X64)
    gu.assert_parity("cem obj against rollout_cost", out["obj"], objr.astype(np.float32), o64)
    start = orc.objective(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"],
                          np.clip(pb64["U"], cc.LO, cc.HI), pb64["x0"])
    assert (out["obj"] < start).all(), (out["obj"], start)


# ---- G8 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_g8_every_sample_is_inside_the_bounds(name):
    links, _ = _runs(name)
    for lk in links:
        s = lk["samples"]
        assert (s >= np.float32(cc.LO)).all() and (s <= np.float32(cc.HI)).all()
    s = links[0]["samples"]
    assert (s == np.float32(cc.LO)).any() and (s == np.float32(cc.HI)).any()      # std 1 around tanh: both bounds bind


def test_g8_one_sided_and_absent_bounds_need_init_std():
    name = "base"
    pb = cc.problem(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        kw = cc.engine_kwargs(name, 1)
        lo = _np(eng.cem_solve(x0, U, goal, -0.5, None, kw, init_std=1.0, want=ALL))["samples"]
        hi = _np(eng.cem_solve(x0, U, goal, None, [0.25, 0.5], kw, init_std=1.0, want=ALL))["samples"]
        free = _np(eng.cem_solve(x0, U, goal, None, None, kw, init_std=1.0, want=ALL))["samples"]
        for bounds in ((-0.5, None), (None, 0.5), (None, None), (-np.inf, 1.0)):
            with pytest.raises(GmpcError, match="cem: .*init_std"):
                eng.cem_solve(x0, U, goal, bounds[0], bounds[1], kw)
    finally:
        eng.close()
    assert lo.min() == np.float32(-0.5) and lo.max() > 1.0
    assert hi[..., 0].max() == np.float32(0.25) and hi[..., 1].max() == np.float32(0.5) and hi.min() < -1.0
    assert free.min() < -1.0 and free.max() > 1.0
    np.testing.assert_array_equal(lo, np.maximum(free, np.float32(-0.5)))
    np.testing.assert_array_equal(hi, np.minimum(free, np.array([0.25, 0.5], np.float32)))


# ---- G9 --------------------------------------------------------------------------------------------------------------
def test_g9_a_samples_cost_depends_on_neither_n_nor_b():
    pb = cc.problem("base")
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        kw = dict(max_iter=1, seed=cc.CEM_SEED, elite_portion=0.1)
        a = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, dict(kw, num_samples=40), want=ALL))
        b = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, dict(kw, num_samples=72), want=ALL))
    finally:
        eng.close()
    np.testing.assert_array_equal(a["samples"], b["samples"][:, :40])
    np.testing.assert_array_equal(a["costs"], b["costs"][:, :40])
    pb = cc.problem("m1")
    eng = gu.engine_for(pb, critic=False)
    try:
        kw = cc.engine_kwargs("m1", 3)
        full = _np(eng.cem_solve(*_args(eng, pb), cc.LO, cc.HI, kw, want=ALL))
        part = _np(eng.cem_solve(*_args(eng, pb, 3), cc.LO, cc.HI, kw, want=ALL))
    finally:
        eng.close()
    for k in full:
        np.testing.assert_array_equal(part[k], full[k][:3], err_msg=k)


# ---- G10 -------------------------------------------------------------------------------------------------------------
def test_g10_stateless_and_deterministic():
    name = "base"
    pb = cc.problem(name)
    B = pb["B"]
    kw = cc.engine_kwargs(name, 3)

    def tail(with_cem):
        eng = gu.engine_for(pb, critic=False)
        try:
            d = eng.to_dev
            x0, U, goal = _args(eng, pb)
            sol = eng.ilqr_solve(x0, U, goal, {"maxiter": 3})
            cem = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, kw, want=ALL)) if with_cem else None
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return _np(sol), loss.cpu().numpy(), grad.cpu().numpy(), cem
        finally:
            eng.close()

    s0, l0, g0, _ = tail(False)
    s1, l1, g1, c1 = tail(True)
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    np.testing.assert_array_equal(l0, l1)
    np.testing.assert_array_equal(g0, g1)
    links, whole = _runs(name)
    for k in c1:       # the same call in another context, after another solve
        np.testing.assert_array_equal(c1[k], whole[3][k], err_msg=k)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        again = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, kw, want=ALL))
        other = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, dict(kw, seed=cc.CEM_SEED + 1), want=ALL))
        high = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, dict(kw, seed=cc.CEM_SEED + (1 << 32)), want=ALL))
    finally:
        eng.close()
    for k in again:
        np.testing.assert_array_equal(again[k], c1[k], err_msg=k)
    assert not np.array_equal(other["samples"], c1["samples"]) and not np.array_equal(other["U"], c1["U"])
    assert not np.array_equal(high["samples"], c1["samples"])      # the seed's high word is part of the key


# ---- G11 -------------------------------------------------------------------------------------------------------------
def _refused(pb, kw, B=None, **more):
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb, B)
        return eng.cem_solve(x0, U, goal, cc.LO, cc.HI, kw, **more)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300", "nm257"])
def test_g11_refused_shapes(case):
    # (a ctx takes no hidden width above 256: the widths that can pass the cap are n and n + m)
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2),
                nm257=dict(n=250, m=7))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    args.setdefault("cost_hidden", (16,))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_fout=4, **args)
    with pytest.raises(GmpcError, match="cem: "):
        _refused(pb, dict(num_samples=32, max_iter=1))


def test_g11_refused_options():
    pb = cc.problem("m1")
    ok = dict(num_samples=32, max_iter=1)
    for bad in (dict(num_samples=4097), dict(num_samples=0), dict(elite_portion=0.0), dict(elite_portion=1.5),
                dict(max_iter=-1), dict(sampling_smoothing=1.0), dict(sampling_smoothing=-0.1),
                dict(evolution_smoothing=1.5), dict(evolution_smoothing=-0.5), dict(evolution_smoothing=float("nan"))):
        with pytest.raises(GmpcError, match="cem: "):
            _refused(pb, dict(ok, **bad))
    with pytest.raises(GmpcError, match="cem: "):
        _refused(pb, dict(ok, bogus=1))
    with pytest.raises(GmpcError, match="cem: "):
        _refused(pb, ok, want=("noise",))
    pb2 = gu.problem(3, 1, 5, 2, seed=1, dyn_hidden=(32, 32), cost_hidden=(16,), cost_fout=4)
    eng = gu.engine_for(pb2, critic=False)
    try:
        d = eng.to_dev
        with pytest.raises(GmpcError, match="max_batch"):
            eng.cem_solve(d(np.zeros((3, 3))), d(np.zeros((3, 5, 1))), d(np.zeros((3, 6, 3))), cc.LO, cc.HI, ok)
        with pytest.raises(GmpcError, match="cem: U_init"):
            eng.cem_solve(d(pb2["x0"]), d(np.zeros((2, 4, 1))), d(pb2["goal"]), cc.LO, cc.HI, ok)
        with pytest.raises(GmpcError, match="u_lo must be <= u_hi"):
            eng.cem_solve(d(pb2["x0"]), d(pb2["U"]), d(pb2["goal"]), 0.2, 0.1, ok)
        # max_iter = 0 is no refusal: the mean's own rollout, mean and std untouched
        out = eng.cem_solve(d(pb2["x0"]), d(pb2["U"]), d(pb2["goal"]), cc.LO, cc.HI, dict(ok, max_iter=0))
        np.testing.assert_array_equal(out["U"].cpu().numpy(), pb2["U"])
        Xr, _ = eng.rollout_cost(d(pb2["x0"]), d(pb2["U"]), d(pb2["goal"]))
        assert gu.rel_err(out["X"].cpu().numpy(), Xr.cpu().numpy()) < 1e-5
    finally:
        eng.close()


def test_g11_policy_actions_are_inside_the_bounds_and_training_calls_raise():
    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    from gan_mpc_amd.policy import differentiable as diff
    bound = 0.3             # (the expert's start is tanh-sized: the policy clamps it into the bounds)
    kw = dict(num_samples=64, max_iter=4, seed=7)
    config, policy, params, data = mirror._build(functools.partial(
        l2_policy.L2MPC, solver="cem", control_bounds=(-bound, bound), cem_kwargs=kw))
    assert policy.solver == "cem" and policy.cem_kwargs["num_samples"] == 64
    policy.expert_model.select(np.array([2]))
    X, U, obj, grad, adj, lqr, itr = policy.get_optimal_values(params, data["hist"][2])
    assert grad is None and adj is None and lqr is None and int(itr) == 4
    assert tuple(U.shape) == (policy._engine.T, policy._engine.m)
    U = U.cpu().numpy()
    assert (np.abs(U) <= np.float32(bound)).all()
    a = policy.get_optimal_action(params, data["hist"][2]).cpu().numpy()
    assert (np.abs(a) <= np.float32(bound)).all()
    assert policy.cem_solves == 2
    assert not np.array_equal(a, U[0])          # the second solve ran under seed + 1
    # the same two solves again from a fresh policy: the seed advances deterministically
    _, policy2, params2, _ = mirror._build(functools.partial(
        l2_policy.L2MPC, solver="cem", control_bounds=(-bound, bound), cem_kwargs=kw))
    policy2.expert_model.select(np.array([2]))
    np.testing.assert_array_equal(policy2.get_optimal_values(params2, data["hist"][2])[1].cpu().numpy(), U)
    policy.expert_model.select(np.arange(4))
    with pytest.raises(NotImplementedError, match="cem"):
        policy.loss_and_grad(data["hist"][:4], params, (data["Y"][:4],))
    with pytest.raises(NotImplementedError, match="cem"):
        policy.batch_loss(params, data["hist"][:4], data["Y"][:4])
    with pytest.raises(NotImplementedError, match="cem"):
        diff.ilqr_layer(policy, params, None, None, None)
    assert policy.cem_solves == 2
