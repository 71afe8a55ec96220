"""gmpc_icem_solve on the GPU against tests/icem_ref.py, link by link: the tie to gmpc_cem_solve
(I1), the coloured samples on both of the rollout's paths (I2), the costs at the GPU's own pool (I3), one update at the
GPU's own costs and rows (I4), the chaining of iterations bit for bit (I5) -- together they pin the whole solve --, then
independence from N and B (I6), a problem without a finite cost (I7), three free-running iterations on the decided
problems (I8), the bounds (I9), statelessness and determinism (I10), refusals (I11) and the policy (I12).  Parity goes
through gpu_util.assert_parity at its defaults: fp64 is the arbiter, the fp32 NumPy restatement the yardstick."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cem_cases as cc
import cem_ref as cr
import gan_mpc_oracle as orc
import gpu_util as gu
import icem_cases as ic
import icem_ref as ir
from gan_mpc_amd import engine as E_
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

ALL = ("costs", "elites", "samples")
NAMES = list(ic.CASES)
GAMMA = 0.1
OUT = ("X", "U", "obj", "mean", "std", "costs", "elites", "samples")
STATE = ("keep", "best_U", "best_cost")


def _np(out):
    return {k: ({s: t.cpu().numpy() for s, t in v.items()} if isinstance(v, dict) else v.cpu().numpy())
            for k, v in out.items()}


def _args(eng, pb, B=None):
    d = eng.to_dev
    B = pb["B"] if B is None else B
    return d(pb["x0"][:B]), d(pb["U"][:B]), d(pb["goal"][:B])


def _same(a, b, what=""):
    for k in OUT:
        if k in a or k in b:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    for k in STATE:
        np.testing.assert_array_equal(a["state"][k], b["state"][k], err_msg=f"{what}: state {k}")


def _chain(eng, name, x0, U, goal, K):
    """K chained calls of one iteration (add_mean in the last only), each with what it started from."""
    nk = ic.NUM_KEEP[name]
    links, mean, std, state = [], U, ic.INIT_STD, None
    for i in range(K):
        last = i == K - 1
        out = eng.icem_solve(x0, mean, goal, ic.LO, ic.HI, ic.engine_kwargs(name, 1, add_mean=last), init_std=std,
                             want=ALL, iter_offset=i, state=state)
        rec = _np(out)
        rec["mean_in"] = mean.cpu().numpy()
        rec["std_in"] = np.full_like(rec["mean_in"], ic.INIT_STD) if i == 0 else std.cpu().numpy()
        rec["carry"], rec["add_mean"] = (0 if state is None else nk), last
        rec["state_in"] = None if state is None else {k: v.cpu().numpy() for k, v in state.items()}
        links.append(rec)
        mean, std, state = out["mean"], out["std"], out["state"]
    return links


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Per case, computed once: the chains of 3 and of 5 one-iteration calls and the whole solves of 3 and 5."""
    pb = ic.problem(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        chains = {K: _chain(eng, name, x0, U, goal, K) for K in (3, 5)}
        whole = {K: _np(eng.icem_solve(x0, U, goal, ic.LO, ic.HI, ic.engine_kwargs(name, K), init_std=ic.INIT_STD,
                                       want=ALL)) for K in (3, 5)}
        torch.cuda.synchronize()
    finally:
        eng.close()
    return chains, whole


def _pool(lk, dt):
    """The pool of a link as the kernel saw it: the GPU's fresh rows, the carried rows, the mean."""
    lo, hi = dt(ic.LO), dt(ic.HI)
    rows = [lk["samples"].astype(dt)]
    if lk["carry"]:
        rows.append(ir.clamp(lk["state_in"]["keep"][:, :lk["carry"]].astype(dt), lo, hi))
    if lk["add_mean"]:
        rows.append(ir.clamp(lk["mean_in"].astype(dt), lo, hi)[:, None])
    return np.concatenate(rows, axis=1)


def _pb64(name):
    return orc.cast_problem(ic.problem(name), np.float64)


# ---- I1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_i1_tie_settings_are_cem_bit_for_bit(name):
    pb = ic.problem(name)
    (n, m, T, B, N, E), _ = ic.CASES[name]
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        tie = dict(cc.engine_kwargs(name, 3), keep_portion=0.0, decay=1.0, noise_beta=0.0, add_mean=False,
                   return_best=False)
        a = _np(eng.icem_solve(x0, U, goal, cc.LO, cc.HI, tie, want=ALL))
        c = _np(eng.cem_solve(x0, U, goal, cc.LO, cc.HI, cc.engine_kwargs(name, 3), want=ALL))
    finally:
        eng.close()
    assert a["costs"].shape == (B, N) and a["samples"].shape == (B, N, T, m)
    for k in ("X", "obj", "std", "costs", "elites", "samples"):
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    np.testing.assert_array_equal(a["mean"], c["U"])
    np.testing.assert_array_equal(a["U"], c["U"])           # without return_best the returned sequence is the mean


# ---- I2 --------------------------------------------------------------------------------------------------------------
def _free_samples(pb, N, E, nk, beta):
    """Samples around mean 0 with std 1 and no bounds -- the coloured normals themselves --, and the kept rows."""
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        kw = dict(num_samples=N, elite_portion=(E + 0.5) / N, keep_portion=(nk + 0.5) / E, max_iter=1, seed=ic.ICEM_SEED,
                  noise_beta=beta, add_mean=False, decay=1.0)
        outs = [_np(eng.icem_solve(x0, torch.zeros_like(U), goal, None, None, kw, init_std=1.0, want=ALL,
                                   iter_offset=it)) for it in (0, 1)]
    finally:
        eng.close()
    return outs


@pytest.mark.parametrize("path", ["lds", "element"])
def test_i2_coloured_samples_on_both_paths(path):
    """The rollout forms a tile's normals once in LDS where 32 m T floats fit beside the operand block (m T <= 252:
    "lds", base's m T = 16) and per element otherwise ("element": m T = 256).  The update always regenerates per
    element, so the kept rows -- bitwise the elites' sample rows -- show the two evaluations equal at base, where both
    are legal."""
    if path == "lds":
        pb = ic.problem("base")
        (n, m, T, B, N, E), _ = ic.CASES["base"]
        nk = 3
    else:
        n, m, T, B, N, E, nk = 4, 32, 8, 2, 33, 4, 2
        pb = gu.problem(n, m, T, B, seed=5, bias_scale=0.1, dyn_hidden=(32, 32), cost_hidden=(16,), cost_fout=4)
    assert (m * T <= 252) == (path == "lds")
    outs = _free_samples(pb, N, E, nk, ic.NOISE_BETA)
    cw = ir.colour_weights(T, ic.NOISE_BETA).astype(np.float32)
    for it, out in enumerate(outs):
        z = {dt: np.stack([ir.colour(cr.normals(ic.ICEM_SEED, it, b, np.arange(N), T * m, dt).reshape(N, T, m), cw, dt)
                           for b in range(B)]) for dt in (np.float32, np.float64)}
        e = gu.assert_parity(f"icem coloured samples {path} it={it}", out["samples"], z[np.float32], z[np.float64])
        print(f"I2 {path} it={it}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")
        for b in range(B):
            np.testing.assert_array_equal(out["state"]["keep"][b], out["samples"][b][out["elites"][b, :nk]])
        var = (out["samples"].astype(np.float64) ** 2).mean()
        assert abs(var - 1) < 4 * np.sqrt(2.0 / (B * N * m))      # (T steps of one row are not independent draws)
    white = _free_samples(pb, N, E, nk, 0.0)[0]["samples"]
    plain = np.stack([cr.normals(ic.ICEM_SEED, 0, b, np.arange(N), T * m, np.float32).reshape(N, T, m) for b in range(B)])
    assert gu.rel_err(white, plain) < 1e-5 and gu.rel_err(outs[0]["samples"], plain) > 0.1
    assert not np.array_equal(outs[0]["samples"], outs[1]["samples"])


# ---- I3, I4: every link of the chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_i3_costs_at_the_gpu_pool(name):
    pb, pb64 = ic.problem(name), _pb64(name)
    chains, _ = _runs(name)
    nk = ic.NUM_KEEP[name]
    want = ir.sample_counts(ic.CASES[name][0][4], ic.CASES[name][0][5], ic.DECAY, 3)
    for i, lk in enumerate(chains[3]):
        assert lk["samples"].shape[1] == want[i] and lk["costs"].shape[1] == want[i] + lk["carry"] + lk["add_mean"]
        c32, c64 = cr.sample_costs(pb, _pool(lk, np.float32)), cr.sample_costs(pb64, _pool(lk, np.float64))
        e = gu.assert_parity(f"icem costs link {i}", lk["costs"], c32, c64)
        print(f"I3 {name} link {i}: pool {lk['costs'].shape[1]} rows, HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")
    if nk:
        # a carried row costs what it cost as a sample: the same controls, rolled out again
        a, b = chains[3][0], chains[3][1]
        for p in range(a["costs"].shape[0]):
            np.testing.assert_array_equal(b["costs"][p, want[1]:want[1] + nk], a["costs"][p, a["elites"][p, :nk]])


@pytest.mark.parametrize("name", NAMES)
def test_i4_update_at_the_gpu_costs_and_rows(name):
    (n, m, T, B, N, E), _ = ic.CASES[name]
    nk = ic.NUM_KEEP[name]
    chains, _ = _runs(name)
    for i, lk in enumerate(chains[3]):
        np.testing.assert_array_equal(lk["elites"], cr.elites_of(lk["costs"], E))
        ref = {}
        for dt in (np.float32, np.float64):
            ref[dt] = cr.update(_pool(lk, dt), lk["costs"], lk["mean_in"].astype(dt), lk["std_in"].astype(dt), E, GAMMA,
                                dt, elites=lk["elites"])
        e = gu.assert_parity(f"icem mean link {i}", lk["mean"], ref[np.float32][0], ref[np.float64][0])
        f = gu.assert_parity(f"icem std link {i}", lk["std"], ref[np.float32][1], ref[np.float64][1])
        print(f"I4 {name} link {i}: mean HIP {e[0]:.3e} / fp32 {e[1]:.3e}, std HIP {f[0]:.3e} / fp32 {f[1]:.3e}")
        pool = _pool(lk, np.float32)
        old = np.full(B, np.inf, np.float32) if lk["state_in"] is None else lk["state_in"]["best_cost"]
        for b in range(B):
            np.testing.assert_array_equal(lk["state"]["keep"][b], pool[b][lk["elites"][b, :nk]])
            top = lk["costs"][b, lk["elites"][b, 0]]
            if top < old[b]:
                assert lk["state"]["best_cost"][b] == top
                np.testing.assert_array_equal(lk["state"]["best_U"][b], pool[b][lk["elites"][b, 0]])
            else:
                assert lk["state"]["best_cost"][b] == old[b]
                np.testing.assert_array_equal(lk["state"]["best_U"][b], lk["state_in"]["best_U"][b])
        np.testing.assert_array_equal(lk["U"], lk["state"]["best_U"])        # return_best, and every best is finite
    assert all((lk["state"]["best_cost"] < np.inf).all() for lk in chains[3])


# ---- I5 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("K", [3, 5])
def test_i5_one_call_is_the_chain_of_single_iterations(name, K):
    chains, whole = _runs(name)
    _same(whole[K], chains[K][-1], f"{name} K={K}")


# ---- I6 --------------------------------------------------------------------------------------------------------------
def test_i6_a_rows_cost_depends_on_neither_n_nor_b():
    pb = ic.problem("base")
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        kw = dict(max_iter=1, seed=ic.ICEM_SEED, elite_portion=0.1)
        a = _np(eng.icem_solve(x0, U, goal, ic.LO, ic.HI, dict(kw, num_samples=40), init_std=ic.INIT_STD, want=ALL))
        b = _np(eng.icem_solve(x0, U, goal, ic.LO, ic.HI, dict(kw, num_samples=72), init_std=ic.INIT_STD, want=ALL))
    finally:
        eng.close()
    np.testing.assert_array_equal(a["samples"], b["samples"][:, :40])
    np.testing.assert_array_equal(a["costs"][:, :40], b["costs"][:, :40])
    pb = ic.problem("m1")
    eng = gu.engine_for(pb, critic=False)
    try:
        kw = ic.engine_kwargs("m1", 3)
        full = _np(eng.icem_solve(*_args(eng, pb), ic.LO, ic.HI, kw, init_std=ic.INIT_STD, want=ALL))
        part = _np(eng.icem_solve(*_args(eng, pb, 3), ic.LO, ic.HI, kw, init_std=ic.INIT_STD, want=ALL))
    finally:
        eng.close()
    for k in OUT:
        np.testing.assert_array_equal(part[k], full[k][:3], err_msg=k)
    for k in STATE:
        np.testing.assert_array_equal(part["state"][k], full["state"][k][:3], err_msg=k)


# ---- I6 (no finite cost), I7 -----------------------------------------------------------------------------------------
def test_i7_a_problem_without_a_finite_cost_keeps_mean_and_std_and_returns_the_mean():
    name = "base"
    pb = ic.problem(name)
    chains, whole = _runs(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        bad = x0.clone()
        bad[1, 0] = float("nan")
        nan = _np(eng.icem_solve(bad, U, goal, ic.LO, ic.HI, ic.engine_kwargs(name, 3), init_std=ic.INIT_STD, want=ALL))
    finally:
        eng.close()
    assert np.isnan(nan["costs"][1]).all() and np.isinf(nan["state"]["best_cost"][1])
    np.testing.assert_array_equal(nan["std"][1], np.full_like(nan["std"][1], ic.INIT_STD))        # untouched
    np.testing.assert_array_equal(nan["mean"][1], pb["U"][1])
    np.testing.assert_array_equal(nan["U"][1], nan["mean"][1])
    assert np.isfinite(nan["state"]["keep"][1]).all()
    ref = whole[3]
    for k in OUT:
        np.testing.assert_array_equal(nan[k][[0, 2]], ref[k][[0, 2]], err_msg=k)
    for k in STATE:
        np.testing.assert_array_equal(nan["state"][k][[0, 2]], ref["state"][k][[0, 2]], err_msg=k)


# ---- I8 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.DECIDED)
def test_i8_three_free_running_iterations_on_the_decided_problems(name):
    (n, m, T, B, N, E), _ = ic.CASES[name]
    nk = ic.NUM_KEEP[name]
    pb, pb64 = ic.problem(name), _pb64(name)
    chains, whole = _runs(name)
    r32, t32, r64, t64 = ic.traces(name)
    ok = ir.decided(t32, t64, E, nk)[2]
    print(f"I8 {name}: decided {int(ok.sum())} of {B}")
    out = whole[3]
    if ok.any():
        for i in range(3):
            for b in np.nonzero(ok)[0]:
                assert set(chains[3][i]["elites"][b]) == set(t64[i]["elites"][b]), (name, i, b)
                assert list(chains[3][i]["elites"][b, :nk]) == list(t64[i]["elites"][b, :nk]), (name, i, b)
        e = gu.assert_parity("icem mean after 3", out["mean"][ok], r32["mean"][ok], r64["mean"][ok])
        f = gu.assert_parity("icem std after 3", out["std"][ok], r32["std"][ok], r64["std"][ok])
        gu.assert_parity("icem keep after 3", out["state"]["keep"][ok], r32["state"]["keep"][ok],
                         r64["state"]["keep"][ok])
        print(f"I8 {name}: mean HIP {e[0]:.3e} / fp32 {e[1]:.3e}, std HIP {f[0]:.3e} / fp32 {f[1]:.3e}")
    # the returned sequence, its rollout and objective: every problem
    U = out["U"]
    X64 = orc.rollout(pb64["dyn"], U.astype(np.float64), pb64["x0"])
    o32 = orc.objective(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], U, pb["x0"])
    o64 = orc.objective(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], U.astype(np.float64), pb64["x0"])
    gu.assert_parity("icem X of the returned U", out["X"], orc.rollout(pb["dyn"], U, pb["x0"]), X64)
    gu.assert_parity("icem obj of the returned U", out["obj"], o32, o64)
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        Xr, cr_ = eng.rollout_cost(d(pb["x0"]), d(U), d(pb["goal"]))
        Xr, objr = Xr.cpu().numpy(), cr_.cpu().numpy().astype(np.float64).sum(1)
    finally:
        eng.close()
    gu.assert_parity("icem X against rollout_cost", out["X"], Xr, X64)
    gu.assert_parity("icem obj against rollout_cost", out["obj"], objr.astype(np.float32), o64)
    # the objective is the best cost: the same controls through the same arithmetic, to the rounding of another tile
    best = out["state"]["best_cost"]
    assert (out["obj"] <= best * (1 + 1e-5)).all(), (out["obj"], best)
    start = orc.objective(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"],
                          np.clip(pb64["U"], ic.LO, ic.HI), pb64["x0"])
    assert (out["obj"] < start).all(), (out["obj"], start)


# ---- I9 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_i9_every_row_and_the_returned_controls_are_inside_the_bounds(name):
    chains, whole = _runs(name)
    lo, hi = np.float32(ic.LO), np.float32(ic.HI)
    for lk in chains[5] + [whole[3], whole[5]]:
        for a in (lk["samples"], lk["state"]["keep"], lk["state"]["best_U"], lk["U"]):
            assert (a >= lo).all() and (a <= hi).all()
    if name == "cheetah":       # 84 000 controls with std 0.5 around a tanh-sized start: both bounds bind
        s = chains[5][0]["samples"]
        assert (s == lo).any() and (s == hi).any()


def test_i9_one_sided_and_absent_bounds_are_the_clamp_of_the_free_samples():
    name = "base"
    pb = ic.problem(name)
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        kw = ic.engine_kwargs(name, 1)
        lo = _np(eng.icem_solve(x0, U, goal, -0.5, None, kw, init_std=1.0, want=ALL))["samples"]
        hi = _np(eng.icem_solve(x0, U, goal, None, [0.25, 0.5], kw, init_std=1.0, want=ALL))["samples"]
        free = _np(eng.icem_solve(x0, U, goal, None, None, kw, init_std=1.0, want=ALL))["samples"]
        for bounds in ((-0.5, None), (None, 0.5), (None, None), (-np.inf, 1.0)):
            with pytest.raises(GmpcError, match="icem: .*init_std"):
                eng.icem_solve(x0, U, goal, bounds[0], bounds[1], kw)
    finally:
        eng.close()
    assert lo.min() == np.float32(-0.5) and lo.max() > 1.0
    assert hi[..., 0].max() == np.float32(0.25) and hi[..., 1].max() == np.float32(0.5) and hi.min() < -1.0
    assert free.min() < -1.0 and free.max() > 1.0
    np.testing.assert_array_equal(lo, np.maximum(free, np.float32(-0.5)))
    np.testing.assert_array_equal(hi, np.minimum(free, np.array([0.25, 0.5], np.float32)))


# ---- I10 -------------------------------------------------------------------------------------------------------------
def test_i10_stateless_and_deterministic():
    name = "base"
    pb = ic.problem(name)
    B = pb["B"]
    kw = ic.engine_kwargs(name, 3)

    def tail(with_icem):
        eng = gu.engine_for(pb, critic=False)
        try:
            d = eng.to_dev
            x0, U, goal = _args(eng, pb)
            sol = eng.ilqr_solve(x0, U, goal, {"maxiter": 3})
            icem = (_np(eng.icem_solve(x0, U, goal, ic.LO, ic.HI, kw, init_std=ic.INIT_STD, want=ALL))
                    if with_icem else None)
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return {k: v.cpu().numpy() for k, v in sol.items()}, loss.cpu().numpy(), grad.cpu().numpy(), icem
        finally:
            eng.close()

    s0, l0, g0, _ = tail(False)
    s1, l1, g1, c1 = tail(True)
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    np.testing.assert_array_equal(l0, l1)
    np.testing.assert_array_equal(g0, g1)
    _, whole = _runs(name)
    _same(c1, whole[3], "another context, after another solve")
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb)
        again = _np(eng.icem_solve(x0, U, goal, ic.LO, ic.HI, kw, init_std=ic.INIT_STD, want=ALL))
        beta = _np(eng.icem_solve(x0, U, goal, ic.LO, ic.HI, dict(kw, noise_beta=1.0), init_std=ic.INIT_STD, want=ALL))
        back = _np(eng.icem_solve(x0, U, goal, ic.LO, ic.HI, kw, init_std=ic.INIT_STD, want=ALL))
        other = _np(eng.icem_solve(x0, U, goal, ic.LO, ic.HI, dict(kw, seed=ic.ICEM_SEED + (1 << 32)),
                                   init_std=ic.INIT_STD, want=ALL))
    finally:
        eng.close()
    _same(again, c1, "repeated")
    _same(back, c1, "after a call with another noise_beta")       # (the weights on the device follow noise_beta)
    assert not np.array_equal(beta["samples"], c1["samples"])
    assert not np.array_equal(other["samples"], c1["samples"])    # the seed's high word is part of the key


# ---- I11 -------------------------------------------------------------------------------------------------------------
def _refused(pb, kw, B=None, **more):
    eng = gu.engine_for(pb, critic=False)
    try:
        x0, U, goal = _args(eng, pb, B)
        return eng.icem_solve(x0, U, goal, ic.LO, ic.HI, kw, **more)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300", "nm257"])
def test_i11_refused_shapes(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2),
                nm257=dict(n=250, m=7))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    args.setdefault("cost_hidden", (16,))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_fout=4, **args)
    with pytest.raises(GmpcError, match="icem: "):
        _refused(pb, dict(num_samples=32, max_iter=1))


def test_i11_refused_options_and_arguments():
    pb = ic.problem("m1")
    ok = dict(num_samples=32, max_iter=1)
    for bad in (dict(num_samples=4097), dict(num_samples=0), dict(elite_portion=0.0), dict(elite_portion=1.5),
                dict(keep_portion=1.5), dict(keep_portion=-1.0), dict(num_samples=4090, keep_portion=0.05),
                dict(max_iter=-1), dict(decay=0.9), dict(decay=float("inf")), dict(noise_beta=-1.0),
                dict(noise_beta=float("nan")), dict(evolution_smoothing=1.5), dict(evolution_smoothing=float("nan"))):
        with pytest.raises(GmpcError, match="icem: "):
            _refused(pb, dict(ok, **bad))
    with pytest.raises(GmpcError, match="icem: "):
        _refused(pb, dict(ok, bogus=1))
    with pytest.raises(GmpcError, match="icem: "):
        _refused(pb, ok, want=("weights",))
    with pytest.raises(GmpcError, match="icem: iter_offset"):
        _refused(pb, ok, iter_offset=-1)
    eng = gu.engine_for(pb, critic=False)
    try:
        d = eng.to_dev
        x0, U, goal = _args(eng, pb)
        B, T, m, n = pb["B"], pb["T"], pb["m"], pb["n"]
        with pytest.raises(GmpcError, match="max_batch"):
            eng.icem_solve(d(np.zeros((B + 1, n))), d(np.zeros((B + 1, T, m))), d(np.zeros((B + 1, T + 1, n))), ic.LO,
                           ic.HI, ok)
        with pytest.raises(GmpcError, match="icem: U_init"):
            eng.icem_solve(x0, d(np.zeros((B, T + 1, m))), goal, ic.LO, ic.HI, ok)
        with pytest.raises(GmpcError, match="u_lo must be <= u_hi"):
            eng.icem_solve(x0, U, goal, 0.2, 0.1, ok)
        with pytest.raises(GmpcError, match="icem: carry_in"):
            eng.icem_solve(x0, U, goal, ic.LO, ic.HI, dict(ok, keep_portion=0.4), state=dict(
                keep=torch.zeros(B, 1, T, m), best_U=torch.zeros(B, T, m), best_cost=torch.zeros(B), carry=2))
        # the pointers the entry point itself refuses: through the C ABI
        opts = E_.make_icem_opts(dict(ok, keep_portion=0.4))           # E = 3, num_keep = 1
        std, keep, bU, bc, Uo = (d(np.full((B, T, m), 0.5)), d(np.zeros((B, 1, T, m))), d(np.zeros((B, T, m))),
                                 d(np.full(B, np.inf)), eng.new(B, T, m))
        P = E_._ptr

        def raw(o, x0=x0, goal=goal, mean=U.clone(), std=std, keep=keep, bU=bU, bc=bc, Uo=Uo):
            return eng.lib.gmpc_icem_solve(eng.ctx, B, P(x0), P(goal), None, None, C.byref(o), P(mean), P(std), P(keep),
                                           P(bU), P(bc), P(Uo), None, None, None, None, None, eng._stream())

        for change in (dict(keep=None), dict(bU=None), dict(bc=None), dict(Uo=None), dict(bU=None, bc=None),
                       dict(x0=None), dict(goal=None), dict(mean=None), dict(std=None)):
            assert raw(opts, **change) == -1, change
            assert eng.lib.gmpc_last_error().startswith(b"icem: "), (change, eng.lib.gmpc_last_error())
        assert eng.lib.gmpc_icem_solve(eng.ctx, B, P(x0), P(goal), None, None, None, P(U), P(std), P(keep), P(bU), P(bc),
                                       P(Uo), None, None, None, None, None, eng._stream()) == -1
        # without return_best the best buffers and U_out may be absent; max_iter = 0 returns the mean's rollout
        o2 = E_.make_icem_opts(dict(ok, keep_portion=0.0, return_best=False))
        assert raw(o2, keep=None, bU=None, bc=None, Uo=None) == 0
        out = eng.icem_solve(x0, U, goal, ic.LO, ic.HI, dict(ok, max_iter=0))
        np.testing.assert_array_equal(out["U"].cpu().numpy(), pb["U"])
        np.testing.assert_array_equal(out["mean"].cpu().numpy(), pb["U"])
        Xr, _ = eng.rollout_cost(x0, U, goal)
        assert gu.rel_err(out["X"].cpu().numpy(), Xr.cpu().numpy()) < 1e-5
        torch.cuda.synchronize()
    finally:
        eng.close()


# ---- I12 -------------------------------------------------------------------------------------------------------------
def test_i12_policy_actions_are_inside_the_bounds_elites_are_carried_and_training_calls_raise():
    import test_gpu_mirror as mirror
    from gan_mpc_amd.norm import l2_policy
    from gan_mpc_amd.policy import differentiable as diff
    bound = 0.3
    kw = dict(num_samples=64, max_iter=3, seed=7)
    build = lambda **more: mirror._build(functools.partial(                                     # noqa: E731
        l2_policy.L2MPC, solver="icem", control_bounds=(-bound, bound), icem_kwargs=dict(kw, **more)))
    config, policy, params, data = build()
    assert policy.solver == "icem" and policy.icem_kwargs["num_samples"] == 64 and policy.icem_kwargs["shift_elites"]
    policy.expert_model.select(np.array([2]))
    X, U, obj, grad, adj, lqr, itr = policy.get_optimal_values(params, data["hist"][2])
    assert grad is None and adj is None and lqr is None and int(itr) == 3
    assert tuple(U.shape) == (policy._engine.T, policy._engine.m)
    U = U.cpu().numpy()
    assert (np.abs(U) <= np.float32(bound)).all()
    keep1 = policy._icem_state["keep"].clone()
    assert tuple(keep1.shape)[:2] == (1, 1) and bool((keep1.abs() <= bound).all())                # E = 6, num_keep = 1
    a = policy.get_optimal_action(params, data["hist"][2]).cpu().numpy()
    assert (np.abs(a) <= np.float32(bound)).all()
    assert policy.icem_solves == 2
    assert not np.array_equal(a, U[0])          # the second solve ran under seed + 1, with the shifted row in its pool
    # the same two solves from fresh policies: deterministic; without shift_elites the second one differs
    _, policy2, params2, _ = build()
    policy2.expert_model.select(np.array([2]))
    np.testing.assert_array_equal(policy2.get_optimal_values(params2, data["hist"][2])[1].cpu().numpy(), U)
    np.testing.assert_array_equal(policy2._icem_state["keep"].cpu().numpy(), keep1.cpu().numpy())
    np.testing.assert_array_equal(policy2.get_optimal_action(params2, data["hist"][2]).cpu().numpy(), a)
    # reset drops the kept rows (what the next solve then passes on is checked with a stubbed engine in
    # test_icem_host.py); a policy without shift_elites never holds any
    policy2.reset_warm_start()
    assert policy2._icem_state is None
    _, policy3, params3, _ = build(shift_elites=False)
    policy3.expert_model.select(np.array([2]))
    np.testing.assert_array_equal(policy3.get_optimal_values(params3, data["hist"][2])[1].cpu().numpy(), U)
    assert policy3._icem_state is None and policy3.icem_solves == 1
    policy.expert_model.select(np.arange(4))
    with pytest.raises(NotImplementedError, match="icem"):
        policy.loss_and_grad(data["hist"][:4], params, (data["Y"][:4],))
    with pytest.raises(NotImplementedError, match="icem"):
        policy.batch_loss(params, data["hist"][:4], data["Y"][:4])
    with pytest.raises(NotImplementedError, match="icem"):
        diff.ilqr_layer(policy, params, None, None, None)
    assert policy.icem_solves == 2
