"""Control-limited iLQR (gmpc_ilqr_solve_box) without a device:

  * the NumPy restatement tests/box_ilqr_ref.py -- its box QP against brute force over all 3^m faces, its solve against
    orc.ilqr with no bound active (exactly, fp64), feasibility / monotonicity / the KKT conditions with active bounds;
  * the C ABI, the ctypes table and the Engine agree on the argument order; the host-side refusals;
  * the inputs of tests/test_gpu_box_solve.py (tests/box_cases.py): share of controls at a bound, share of trajectories
    whose control flow is decided, the recorded whole-solve reference."""

import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import box_cases as bc
import box_ilqr_ref as br
import gan_mpc_oracle as orc
import test_gpu_control_flow as cf
from gan_mpc_amd import _lib
from gan_mpc_amd._lib import GmpcError
from gan_mpc_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- box_qp against brute force ------------------------------------------------------------------------------------
def _brute_force(G, h, lb, ub):
    """The minimiser by enumeration: every component at its lower bound, free or at its upper bound; the feasible
    stationary point of the lowest objective (G positive definite: it is the KKT point)."""
    m = len(h)
    best = None
    for face in itertools.product((-1, 0, 1), repeat=m):
        face = np.array(face)
        if (np.isinf(lb[face < 0])).any() or (np.isinf(ub[face > 0])).any():
            continue
        y = np.where(face < 0, lb, np.where(face > 0, ub, 0.0))
        f = face == 0
        if f.any():
            y[f] = np.linalg.solve(G[np.ix_(f, f)], -(h[f] + G[np.ix_(f, ~f)] @ y[~f]))
        if (y < lb).any() or (y > ub).any():
            continue
        val = 0.5 * y @ G @ y + h @ y
        if best is None or val < best[0]:
            best = (val, y, face)
    return best


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_box_qp_against_brute_force(m):
    rng = np.random.default_rng(100 + m)
    seen = set()
    for trial in range(60):
        A = rng.standard_normal((m, m + 2))
        G = A @ A.T / m + 0.05 * np.eye(m)
        G = (G + G.T) / 2
        h = rng.standard_normal(m)
        y_free = np.linalg.solve(G, -h)
        # bounds placed so that none, some and all of the components clamp
        width = (4.0, 0.7, 0.05)[trial % 3] * np.abs(y_free).max()
        centre = (0.0, 0.3, 0.0)[trial % 3] * width * rng.standard_normal(m)
        lb, ub = np.minimum(centre - width, 0.0), np.maximum(centre + width, 0.0)    # y = 0 is feasible
        if trial % 5 == 4:
            lb[rng.integers(m)] = -np.inf
        qp = br.box_qp(G, h, lb, ub)
        val, y, face = _brute_force(G, h, lb, ub)
        assert not qp["capped"] and qp["iters"] <= m + 3
        np.testing.assert_allclose(qp["y"], y, rtol=0, atol=1e-10)
        if min(qp["margin_mult"], qp["margin_clear"]) > 1e-8:
            np.testing.assert_array_equal(qp["clamped"], face != 0)
        seen.add(int(qp["clamped"].sum()))
    assert {0, m} <= seen and (m == 1 or len(seen) > 2), seen


def test_box_qp_gains_vanish_on_the_clamped_rows_and_solve_the_free_block():
    rng = np.random.default_rng(7)
    m, n = 4, 3
    A = rng.standard_normal((m, m + 2))
    G = A @ A.T / m + 0.05 * np.eye(m)
    h, H = rng.standard_normal(m), rng.standard_normal((m, n))
    w = 0.5 * np.abs(np.linalg.solve(G, -h))
    w[0] *= 4
    qp = br.box_qp(G, h, -w, w, H)
    c = qp["clamped"]
    assert c.any() and not c.all()
    assert (qp["K"][c] == 0.0).all()
    np.testing.assert_allclose(G[np.ix_(~c, ~c)] @ qp["K"][~c], -H[~c], atol=1e-12)


def test_the_kernels_qp_routine_on_the_host_against_the_numpy_qp():
    """gmpc_box_qp_host is the routine the kernel runs on one lane, compiled for the host: same minimiser as the fp64
    NumPy QP to fp32 accuracy, the iteration count of the fp32 NumPy QP, the same clamped set where the margins hold."""
    lib = _lib.load()
    rng = np.random.default_rng(0)
    active = 0
    for trial, m in enumerate([1, 2, 3, 6, 6, 13, 32, 32] * 12):
        A = rng.standard_normal((m, m + 2)).astype(np.float32)
        G = (A @ A.T / m + 0.05 * np.eye(m)).astype(np.float32)
        G = ((G + G.T) / 2).astype(np.float32)
        h = rng.standard_normal(m).astype(np.float32)
        c = (0.05, 0.3, 1.0, np.inf)[trial % 4]
        lo, hi = np.full(m, -c, np.float32), np.full(m, c, np.float32)
        if trial % 5 == 4:
            lo[:] = -np.inf
        u = np.clip(0.3 * rng.standard_normal(m), lo, hi).astype(np.float32)
        y, cl, it = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(2, np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        assert lib.gmpc_box_qp_host(m, ptr(G), ptr(h), ptr(u), ptr(lo), ptr(hi), ptr(y), ptr(cl), ptr(it)) == 0
        Gd = G + np.float32(br.DELTA) * np.eye(m, dtype=np.float32)
        r64 = br.box_qp(Gd.astype(np.float64), h.astype(np.float64), (lo - u).astype(np.float64),
                        (hi - u).astype(np.float64))
        r32 = br.box_qp(Gd, h, lo - u, hi - u)
        assert it[1] == 0 and not r64["capped"]
        assert it[0] == r32["iters"]
        assert (y >= lo - u).all() and (y <= hi - u).all()
        # (cond(G) <= ~1e3 here: 1e-3 relative is three orders above fp32 rounding through the factorisation)
        assert np.abs(y - r64["y"]).max() <= 1e-3 * max(np.abs(r64["y"]).max(), 1e-6)
        if min(r64["margin_mult"], r64["margin_clear"]) > 1e-4:
            np.testing.assert_array_equal(cl.astype(bool), r64["clamped"])
        active += bool(cl.any())
    assert active > 30
    assert lib.gmpc_box_qp_host(33, ptr(G), ptr(h), ptr(u), ptr(lo), ptr(hi), ptr(y), ptr(cl), ptr(it)) != 0


# ---- box_ilqr ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 3, 7])
def test_without_active_bounds_it_is_the_unconstrained_solve_exactly(seed):
    pb = orc.cast_problem(cf._problem(seed), np.float64)
    kw = {"maxiter": 6}
    args = (pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], pb["x0"], pb["U"])
    with np.errstate(all="ignore"):
        t0, t1 = [], []
        r0 = orc.ilqr(*args, kw, trace=t0)
        for lo, hi in ((-np.inf, np.inf), (None, None), (-1e30, 1e30)):
            t1.clear()
            r1 = br.box_ilqr(*args, lo, hi, kw, trace=t1)
            for i in (0, 1, 2, 3, 4, 6):
                np.testing.assert_array_equal(r1[i], r0[i])
            assert [tuple(t["alpha"]) for t in t1] == [tuple(t["alpha"]) for t in t0]
    assert (r0[6] > 1).any()


@pytest.mark.parametrize("name", ["base", "m1", "cheetah"])
def test_active_bounds_feasible_iterates_and_monotone_objective(name):
    b = bc.bound(name)
    r, trace = bc.reference(name)["o64"]
    for tr in trace:
        assert (np.abs(tr["U"]) <= b).all()
    objs = np.array([tr["obj"] for tr in trace])
    assert (np.diff(objs, axis=0) <= 0).all()
    assert (objs[-1] < objs[0]).all()
    assert (np.abs(r[1]) <= b).all()


def test_kkt_conditions_at_a_solve_stopped_by_the_gradient_criterion():
    pb = bc.problem("m1")
    b = bc.bound("m1")
    thr = 1e-5
    r, trace = bc.run(pb, np.float64, -b, b, {"maxiter": 500, "grad_norm_threshold": thr})
    stopped = (r[6] < 500) & (trace[-1]["crit"]["gn"] <= thr)
    assert stopped.sum() >= 3, (r[6], trace[-1]["crit"]["gn"])
    U, g = r[1][stopped], r[3][stopped]
    lower, upper = U == -b, U == b
    assert (lower | upper).any()
    free = ~(lower | upper)
    assert np.sqrt((g[free] ** 2).sum()) <= thr * np.sqrt(stopped.sum())
    # a bound's multiplier has the sign that pushes against it; entries the projection kept are inside the threshold
    assert (g[lower] > -thr).all() and (g[upper] < thr).all()


# ---- the C ABI, the ctypes table, the Engine -----------------------------------------------------------------------
def _header_params(name):
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1) for p in m.group(1).split(",")]


def test_library_exports_the_box_solve():
    assert hasattr(_lib.load(), "gmpc_ilqr_solve_box")


def test_header_signature_and_engine_agree_on_the_argument_order():
    box, fused = _header_params("gmpc_ilqr_solve_box"), _header_params("gmpc_ilqr_solve_fused")
    assert box[:len(fused)] == fused
    assert box[len(fused):] == [["const float*", "u_lo"], ["const float*", "u_hi"]]
    res, args = _lib.SIGNATURES["gmpc_ilqr_solve_box"]
    res0, args0 = _lib.SIGNATURES["gmpc_ilqr_solve_fused"]
    assert res is res0 is C.c_int
    assert args == args0 + [C.c_void_p, C.c_void_p]
    assert list(inspect.signature(Engine.ilqr_solve_box).parameters) == ["self", "x0", "U", "goal", "u_lo", "u_hi",
                                                                         "kwargs"]

    class Lib:      # records what the engine hands to the entry point
        def gmpc_ilqr_solve_box(self, *a):
            self.args = a
            return 0

    eng = object.__new__(Engine)
    eng.lib, eng.ctx, eng.n, eng.m, eng.T, eng.solve_count = Lib(), None, 3, 2, 4, 0
    made = []
    eng.new = lambda *shape, dtype=None: made.append(shape) or None
    eng.to_dev = lambda a: tuple(float(v) for v in a)
    eng._stream = lambda: "stream"
    import gan_mpc_amd.engine as engine_mod
    orig = engine_mod._ptr
    engine_mod._ptr = lambda t: t
    try:
        eng.ilqr_solve_box(np.zeros((5, 3)), "U", "goal", -0.5, [1.0, np.inf])
    finally:
        engine_mod._ptr = orig
    a = eng.lib.args
    assert len(a) == len(args)
    assert a[1] == 5 and a[3] == "U" and a[4] == "goal" and a[12] == "stream"
    assert a[13] == (-0.5, -0.5) and a[14] == (1.0, float("inf"))


def test_engine_refuses_bad_bounds_before_any_launch():
    eng = object.__new__(Engine)
    eng.m = 2
    eng.lib = None          # any call through the ABI would fail
    for lo, hi in (([0.0, 1.0], [1.0, 0.5]), (0.3, -0.3), ([0.0, np.nan], None), (None, [np.nan, 1.0])):
        with pytest.raises(GmpcError, match="u_lo must be <= u_hi"):
            eng.ilqr_solve_box(None, None, None, lo, hi)
    with pytest.raises(GmpcError, match="2 values"):
        eng.ilqr_solve_box(None, None, None, [0.0, 0.0, 0.0], None)


def test_policy_wants_bounds_and_the_box_solver_together():
    from gan_mpc_amd.policy.eval import EvalMPC
    none = dict(config=None, cost_model=None, dynamics_model=None, expert_model=None)
    with pytest.raises(ValueError, match="control_bounds"):
        EvalMPC(**none, control_bounds=(-1.0, 1.0))
    with pytest.raises(ValueError, match="control_bounds"):
        EvalMPC(**none, solver="fused", control_bounds=(-1.0, 1.0))
    with pytest.raises(ValueError, match="control_bounds"):
        EvalMPC(**none, solver="box")
    p = EvalMPC(**none, solver="box", control_bounds=(-1.0, None))
    assert p.solver == "box" and p.control_bounds == (-1.0, None)
    from gan_mpc_amd.norm.l2_policy import L2MPC
    assert L2MPC(**none, solver="box", control_bounds=(-0.3, 0.3)).control_bounds == (-0.3, 0.3)


def test_solver_dispatch_hands_the_bounds_to_the_box_entry_point():
    from gan_mpc_amd.policy import optimizers as opt

    class Eng:
        def ilqr_solve_box(self, x0, U, goal, lo, hi, kwargs=None):
            return ("box", x0, U, goal, lo, hi, kwargs)

    class Policy:
        solver, control_bounds = "box", (-0.3, 0.4)

    assert opt._solver(Policy(), Eng())("x0", "U", "goal", {"maxiter": 2}) == ("box", "x0", "U", "goal", -0.3, 0.4,
                                                                             {"maxiter": 2})


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.TABLE)
def test_gpu_inputs_are_fixed_here(name):
    pb, b = bc.problem(name), bc.bound(name)
    r64 = bc.reference(name)["o64"][0]
    share = float((np.abs(r64[1]) == b).mean())
    assert 0.2 <= share <= 0.8, share
    assert np.isfinite(r64[2]).all()
    assert not any(tr["backward"]["capped"].any() for tr in bc.reference(name)["o64"][1] if "backward" in tr)
    decided = bc.decided(name, 1)
    assert decided.mean() >= bc.MIN_AGREE[name], (name, decided)
    # (the recorded share is the one this run shows, not a floor far below it)
    assert decided.mean() - bc.MIN_AGREE[name] < 1.0 / pb["B"], (name, decided)


@pytest.mark.parametrize("name", sorted(bc.STEP_MIN_AGREE))
def test_first_pass_steps_are_fixed_here(name):
    fp = bc.first_pass(name)
    share = float(fp["decided"].mean())
    assert share >= bc.STEP_MIN_AGREE[name], (name, fp["decided"])
    assert share - bc.STEP_MIN_AGREE[name] < 1.0 / fp["decided"].size, (name, share)
    assert fp["b64"]["clamped"][fp["decided"]].any() and not fp["b64"]["clamped"][fp["decided"]].all()
    assert (fp["b64"]["qp_iters"] > 1).any()


def test_whole_solve_reference_of_the_large_batch_is_the_recorded_one():
    pb, b = bc.problem("cheetah128"), bc.bound("cheetah128")
    ref = bc.whole_solve_reference("cheetah128")
    assert np.isfinite(ref["obj64"]).all()
    share = float((ref["atb64"] != 0).mean())
    assert 0.2 <= share <= 0.8, share
    idx = np.array([0, 37, 127])
    r = bc.whole_solve(bc.take(pb, idx), b, np.float64)
    np.testing.assert_allclose(r[2], ref["obj64"][idx], rtol=1e-9)
    np.testing.assert_array_equal(bc.at_bound(r[1], -b, b), ref["atb64"][idx])
