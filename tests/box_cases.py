"""The problems, bounds and fp64 / fp32 reference runs shared by tests/test_box_ilqr_host.py (which fixes and checks
them on the CPU) and tests/test_gpu_box_solve.py (which runs gmpc_ilqr_solve_box on them).  TEST INFRASTRUCTURE.

Bounds are +-c x the median |U| of the fp64 UNCONSTRAINED solution (orc.ilqr, maxiter 6), c per case, chosen so that a
fair share of the fp64 box solution's controls sits at a bound (asserted between 20 % and 80 % by the host test)."""

import functools
import os
import sys

import numpy as np

if __name__ == "__main__":      # `python tests/box_cases.py` (the golden writer): what conftest.py sets up under pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import box_ilqr_ref as br
import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_control_flow as cf

MAXITER = 6
MARGIN = cf.MARGIN      # 2e-2: relative size of one step's fp32 uncertainty (tests/gpu_util.py GAIN_CEILING x 2)

# name -> (builder, c)
CASES = {
    "base": (lambda: cf._problem(11, out_scale=1.0), 0.5),
    "m1": (lambda: gu.problem(3, 1, 5, 7, seed=5), 0.5),
    "cheetah": (lambda: gu.problem(17, 6, 5, 7, seed=5), 0.5),
    "wide_m": (lambda: gu.problem(4, 32, 3, 2, seed=1, dyn_hidden=(32, 32), cost_hidden=(16,), cost_fout=4), 0.5),
    "wide_n": (lambda: gu.problem(64, 2, 3, 2, seed=5, dyn_hidden=(32, 32), cost_hidden=(16,), cost_fout=4), 0.5),
    "cheetah128": (lambda: gu.problem(17, 6, 5, 128, seed=5), 0.5),     # the whole-solve test only
    # the tail test only: the two-wave Hessian solve with each of its two clamped-word buffers used once (the CPU run:
    # 10 of step 0's 42 controls on a bound, none of step 1's -- swapping the buffers would move the set)
    "cheetah_T2": (lambda: gu.problem(17, 6, 2, 7, seed=5), 0.5),
}
SHAPES = {"base": (5, 2, 8, 3), "m1": (3, 1, 5, 7), "cheetah": (17, 6, 5, 7), "wide_m": (4, 32, 3, 2),
          "wide_n": (64, 2, 3, 2), "cheetah128": (17, 6, 5, 128), "cheetah_T2": (17, 6, 2, 7)}
TABLE = ("base", "m1", "cheetah", "wide_m", "wide_n")       # the case table of the GPU tests
# min_agree of the one-iteration protocol (decided(name, 1)): what the CPU run shows -- 2 of 3, 4 of 7, 3 of 7, 0 of 2,
# 2 of 2 trajectories -- rounded down; asserted by test_box_ilqr_host.test_gpu_inputs_are_fixed_here.  wide_m: with 32
# controls on 3 steps some multiplier or clearance of every trajectory lies inside the 2e-2 margin.
MIN_AGREE = {"base": 0.66, "m1": 0.57, "cheetah": 0.42, "wide_m": 0.0, "wide_n": 1.0}


@functools.lru_cache(maxsize=None)
def problem(name):
    pb = CASES[name][0]()
    assert (pb["n"], pb["m"], pb["T"], pb["B"]) == SHAPES[name]
    return pb


@functools.lru_cache(maxsize=None)
def bound(name):
    """The scalar b of the case's bounds [-b, b] (fp32, the value the kernel and both references see)."""
    pb = orc.cast_problem(problem(name), np.float64)
    with np.errstate(all="ignore"):
        r = orc.ilqr(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], pb["x0"], pb["U"], {"maxiter": MAXITER})
    return float(np.float32(CASES[name][1] * np.median(np.abs(r[1]))))


def run(pb, dt, lo, hi, kw, U=None, x0=None):
    """box_ilqr in dtype dt -> (result 7-tuple, trace)."""
    q = orc.cast_problem(pb, dt)
    trace = []
    with np.errstate(all="ignore"):
        r = br.box_ilqr(q["dyn"], q["cmlp"], q["mpc_w"], q["goal"], q["x0"] if x0 is None else x0.astype(dt),
                        (q["U"] if U is None else U).astype(dt), lo, hi, kw, trace=trace)
    return r, trace


@functools.lru_cache(maxsize=None)
def reference(name, maxiter=MAXITER):
    """fp64 and fp32 box_ilqr of the case under its bounds: dict(o64=(result, trace), o32=...)."""
    pb, b = problem(name), bound(name)
    kw = {"maxiter": maxiter}
    return dict(o64=run(pb, np.float64, -b, b, kw), o32=run(pb, np.float32, -b, b, kw))


def at_bound(U, lo, hi):
    """+1 where U == hi, -1 where U == lo, 0 elsewhere."""
    return (U == hi).astype(int) - (U == lo).astype(int)


def _flow(r, trace, B, lo, hi):
    """what has to be equal between two runs for a trajectory's control flow to count as the same"""
    alphas = cf._alphas(trace, B)
    return [(int(r[6][b]), tuple(cf._f32(alphas[b])), at_bound(r[1][b], lo, hi).tobytes(),
             tuple(tr["backward"]["clamped"][b].tobytes() for i, tr in enumerate(trace)
                   if "backward" in tr and tr["active"][b])) for b in range(B)]


def margins_ok(trace, B):
    """(B,) bool: in every backward pass a trajectory ran, every clamped control's multiplier and every free control's
    clearance from its bounds exceed MARGIN (relative to the step's largest |h| / |k|) and no QP hit its cap."""
    ok = np.ones(B, bool)
    for tr in trace:
        if "backward" not in tr:
            continue
        bw = tr["backward"]
        good = ((bw["margin_mult"] > MARGIN) & (bw["margin_clear"] > MARGIN) & ~bw["capped"]).all(axis=1)
        ok &= good | ~tr["active"]
    return ok


@functools.lru_cache(maxsize=None)
def decided(name, maxiter=1):
    """(B,) bool -- the protocol of test_gpu_control_flow._run for the box solve: the fp32 and the fp64 reference and
    cf.NPERT fp32 runs from starts perturbed by 1e-6 agree on the iteration count, every accepted step size, the set
    {U == bound} and the clamped set of every backward pass; no continuation check within MARGIN of its threshold; the
    fp64 run's multiplier and clearance margins above MARGIN."""
    pb, b = problem(name), bound(name)
    B = pb["B"]
    kw = {"maxiter": maxiter}
    ref = reference(name, maxiter)
    (r64, t64), (r32, t32) = ref["o64"], ref["o32"]
    f64 = _flow(r64, t64, B, -b, b)
    agree = np.array([a == c for a, c in zip(_flow(r32, t32, B, np.float32(-b), np.float32(b)), f64)])
    rng = np.random.default_rng(1234)
    for _ in range(cf.NPERT):
        Up = (pb["U"] * (1 + 1e-6 * rng.standard_normal(pb["U"].shape))).astype(np.float32)
        xp = (pb["x0"] * (1 + 1e-6 * rng.standard_normal(pb["x0"].shape))).astype(np.float32)
        rp, tp = run(pb, np.float32, -b, b, kw, U=Up, x0=xp)
        agree &= np.array([a == c for a, c in zip(_flow(rp, tp, B, np.float32(-b), np.float32(b)), f64)])
    agree &= ~cf._near_threshold(t64, kw, B)
    agree &= margins_ok(t64, B)
    return agree


# ---- the first backward pass, step by step ------------------------------------------------------------------------
# With maxiter 0 the solve is one backward pass at clamp(U_init): no line search, no control flow.  A STEP (b, t) of it
# is decided when the fp32 and the fp64 reference agree on its clamped set and the fp64 margins exceed MARGIN, at this
# step and at every later one of the trajectory (the sweep runs from t = T - 1 down, and a clamped set that flips
# changes the value function every earlier step sees).  The minimiser k itself is continuous in the data, so it is
# compared on every step.  Share of decided steps the CPU run shows: 3 of 6 at m = 32, 28 of 35 for cheetah (asserted
# by test_box_ilqr_host.test_first_pass_steps_are_fixed_here); the GPU test requires it.
STEP_MIN_AGREE = {"wide_m": 0.5, "cheetah": 0.8}


@functools.lru_cache(maxsize=None)
def first_pass(name):
    """dict(b32, b64: box_backward at clamp(U_init) in fp32 / fp64, decided (B, T) bool)."""
    pb, b = problem(name), bound(name)
    out = {}
    for tag, dt in (("b32", np.float32), ("b64", np.float64)):
        q = orc.cast_problem(pb, dt)
        U = br.clamp(q["U"], dt(-b), dt(b))
        X = orc.rollout(q["dyn"], U, q["x0"])
        lqr = orc.get_lqr_params(q["dyn"], q["cmlp"], q["mpc_w"], q["goal"], X, U)
        out[tag] = br.box_backward(lqr, U, dt(-b), dt(b))
    b32, b64 = out["b32"], out["b64"]
    ok = (b32["clamped"] == b64["clamped"]).all(-1)
    ok &= (b64["margin_mult"] > MARGIN) & (b64["margin_clear"] > MARGIN) & ~b64["capped"] & ~b32["capped"]
    out["decided"] = np.logical_and.accumulate(ok[:, ::-1], axis=1)[:, ::-1]
    return out


# ---- the whole solve under the reference kwargs (cheetah T 5 at B 7 and B 128) ------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_whole_solve_cheetah128.npz")


def take(pb, idx):
    """the trajectories idx of a problem (the networks are shared)"""
    q = dict(pb)
    for key in ("x0", "U", "goal", "true_seq"):
        if key in q:
            q[key] = pb[key][idx]
    q["B"] = len(idx)
    return q


def whole_solve(pb, b, dt):
    from gan_mpc_amd.engine import TRAJAX_iLQR_KWARGS
    return run(pb, dt, -b, b, dict(TRAJAX_iLQR_KWARGS))[0]


@functools.lru_cache(maxsize=None)
def whole_solve_reference(name):
    """dict(obj64, obj32 (B,), atb64 (B, T, m) int8: at_bound of the fp64 solution) of box_ilqr under the reference
    kwargs.  B = 7 is computed here; B = 128 takes a minute in NumPy and is read from tests/golden (written by
    `python tests/box_cases.py`, spot-checked against a recomputation by the host test)."""
    if name == "cheetah128":
        z = np.load(GOLDEN)
        assert float(z["b"]) == bound(name)
        return dict(obj64=z["obj64"], obj32=z["obj32"], atb64=z["atb64"])
    pb, b = problem(name), bound(name)
    r64, r32 = whole_solve(pb, b, np.float64), whole_solve(pb, b, np.float32)
    return dict(obj64=r64[2], obj32=r32[2], atb64=at_bound(r64[1], -b, b).astype(np.int8))


if __name__ == "__main__":
    pb, b = problem("cheetah128"), bound("cheetah128")
    r64, r32 = whole_solve(pb, b, np.float64), whole_solve(pb, b, np.float32)
    np.savez(GOLDEN, b=np.float64(b), obj64=r64[2], obj32=r32[2].astype(np.float32),
             atb64=at_bound(r64[1], -b, b).astype(np.int8))
