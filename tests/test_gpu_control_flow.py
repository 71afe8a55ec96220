"""The iLQR control flow ON THE GPU (gmpc_ilqr_solve: k_ls_place / k_ls_decide / the continuation test at the end
of the Riccati sweep / the host's four-deep polling of the continuation flags) against the fp64 oracle -- the
scenarios tests/test_ilqr_control_flow.py pins between the two CPU restatements, run through the C ABI:

  * iteration counts EQUAL to the oracle's and the step size accepted by every line search EQUAL (powers of two),
    wherever the control flow is DECIDED: the fp32 and the fp64 oracle agree, and so do four more fp32 runs from
    starts perturbed by 1e-6 (a branch that flips under a perturbation of the size by which any two fp32
    implementations of the Riccati sweep differ is not a parity failure), and no check of the continuation
    criterion came within 2 % of its threshold; the share of trajectories left out is bounded by an assertion;
  * full steps, deep backtracking, a NaN start, each threshold of the continuation criterion, an exhausted line
    search, a batch whose members stop at different iterations;
  * the iterations the host enqueues after the last trajectory stopped (it looks at the flags GMPC_POLL_DEPTH = 4
    iterations late) are exact no-ops: maxiter = last stop + 4 and + 20 give bit-identical X, U, obj;
  * the same on the headline shape (n = 17, m = 6, three hidden layers of 200: register-weight rollout, one-wave
    Riccati sweep, and with GMPC_LS16_SPLIT=1 the 16-candidate line search).
Per-iteration step sizes are read by re-solving with maxiter = 1, 2, ... (the solve is deterministic) and reading
the ctx's alpha buffer.  Reference: trajax ilqr_base / line_search_ddp as called from policy/optimizers.py:19-21,
policy/eval.py:10-20; restated at oracle/gan_mpc_oracle.py:ilqr."""

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu

pytestmark = pytest.mark.gpu
POLL_DEPTH = 4


def _problem(seed, out_scale=1.0, B=3, n=5, m=2, T=8, hidden=(16, 16), cost_hidden=(12,), fout=4):
    pb = orc.make_problem(n, m, T, B, seed=seed, dtype=np.float32, dyn_hidden=hidden, cost_hidden=cost_hidden,
                          cost_fout=fout, bias_scale=0.1)
    W, b = pb["dyn"][-1]
    pb["dyn"][-1] = ((W * out_scale).astype(np.float32), (b * out_scale).astype(np.float32))
    return pb


NPERT = 4      # perturbed fp32 runs that a trajectory's control flow has to survive to count as decided


def _oracle(pb, kw, U):
    """fp32 and fp64 oracle runs, plus NPERT fp32 runs from starts perturbed by 1e-6 (relative): through gains of
    condition ~1e4 that is a 1e-3-level change of every step -- the size of the difference between ANY two fp32
    implementations of the sweep (tests/gpu_util.py: GAIN_CEILING), in NPERT random directions."""
    out = {}
    for tag, dt in (("o32", np.float32), ("o64", np.float64)):
        q = orc.cast_problem(pb, dt)
        trace = []
        with np.errstate(all="ignore"):
            r = orc.ilqr(q["dyn"], q["cmlp"], q["mpc_w"], q["goal"], q["x0"], U.astype(dt), kw, trace=trace)
        out[tag] = (r, trace)
    rng = np.random.default_rng(1234)
    q = orc.cast_problem(pb, np.float32)
    out["pert"] = []
    for _ in range(NPERT):
        Up = (U * (1 + 1e-6 * rng.standard_normal(U.shape))).astype(np.float32)
        xp = (q["x0"] * (1 + 1e-6 * rng.standard_normal(q["x0"].shape))).astype(np.float32)
        trace = []
        with np.errstate(all="ignore"):
            r = orc.ilqr(q["dyn"], q["cmlp"], q["mpc_w"], q["goal"], xp, Up, kw, trace=trace)
        out["pert"].append((r, trace))
    return out


def _f32(seq):
    return [np.float32(a) for a in seq]


MARGIN = 2e-2      # = tests/gpu_util.py GAIN_CEILING x 2: the relative size of a step's fp32 uncertainty


def _near_threshold(trace, kw, B):
    """(B,) bool: at some check of the continuation criterion the fp64 oracle decided a trajectory that was still
    running within MARGIN (relative) of a threshold.  obj_step and U_step are differences of iterates that carry the
    gains' conditioning-limited error (two fp32 implementations differ by up to GAIN_CEILING there), so a decision
    that close to its threshold is not a property of the algorithm."""
    full = dict(orc.ILQR_KWARGS)
    full.update(kw)
    near = np.zeros(B, bool)
    for i, tr in enumerate(trace):
        c = tr["crit"]
        running = np.ones(B, bool) if i == 0 else trace[i - 1]["active"]
        pairs = [(c["obj_step"], full["obj_step_threshold"] * c["aobj"]),
                 (c["U_step"], full["inputs_step_threshold"] * c["un"]),
                 (c["gn"], np.full(B, full["grad_norm_threshold"])),
                 (c["gn"], full["relative_grad_norm_threshold"] * c["aobj"])]
        for q, t in pairs:
            with np.errstate(invalid="ignore"):
                close = np.isfinite(q) & (t > 0) & (np.abs(q - t) <= MARGIN * np.maximum(np.abs(q), np.abs(t)))
            near |= close & running
    return near


def _alphas(trace, B):
    """alpha[b][i] = step size trajectory b carries after its (i+1)-th iteration"""
    return [[tr["alpha"][b] for i, tr in enumerate(trace[1:], 1) if trace[i - 1]["active"][b]] for b in range(B)]


def _run(pb, kw, U=None, min_agree=0.6, label="", tol=1e-4, tol_obj=None):
    """tol: bar of the one-step iterates (U, X); tol_obj: bar of the objective (default: tol).  min_agree: the share of
    trajectories whose control flow has to be DECIDED (see the module docstring) -- set per scenario to what the
    scenario shows (the observed share is recorded in the parity log next to the assertions)."""
    tol_obj = tol if tol_obj is None else tol_obj
    U = pb["U"] if U is None else U
    B = U.shape[0]
    gu.set_config(f"control-flow {label} n={pb['n']} m={pb['m']} T={pb['T']} B={B}")
    eng = gu.engine_for(pb, critic=False)
    d = eng.to_dev
    try:
        o = _oracle(pb, kw, U)
        (r32, t32), (r64, t64) = o["o32"], o["o64"]
        a32, a64 = _alphas(t32, B), _alphas(t64, B)
        # (step sizes are alpha_0 / 2^k: compared in fp32, the type the kernels and the fp32 oracle carry them in)
        agree = np.array([r32[6][b] == r64[6][b] and _f32(a32[b]) == _f32(a64[b]) for b in range(B)])
        for rp, tp in o["pert"]:
            ap = _alphas(tp, B)
            agree &= np.array([rp[6][b] == r64[6][b] and _f32(ap[b]) == _f32(a64[b]) for b in range(B)])
        agree &= ~_near_threshold(t64, kw, B)
        gu._record(dict(stage=f"{label}: share of trajectories whose control flow is decided (required {min_agree})",
                        config=gu.CURRENT_CONFIG[0], e_hip=float(agree.mean()), e_o32=None, tol=min_agree,
                        tol_used=min_agree, branch="info", entries=int(B), passed=bool(agree.mean() >= min_agree)))
        assert agree.mean() >= min_agree, f"the control flow of {agree.sum()} of {B} trajectories only is decided"
        out = eng.ilqr_solve(d(pb["x0"]), d(U), d(pb["goal"]), kw)
        it = out["iterations"].cpu().numpy()
        # --- iteration counts
        np.testing.assert_array_equal(it[agree], r64[6][agree])
        # --- the step size after every iteration: re-solve with maxiter = 1 .. and read the ctx's alpha
        kmax = int(r64[6].max())
        for k in range(1, kmax + 1):
            kk = dict(kw, maxiter=k)
            eng.ilqr_solve(d(pb["x0"]), d(U), d(pb["goal"]), kk)
            alpha = eng.debug_buffer(8, (B,)).cpu().numpy()
            for b in np.nonzero(agree)[0]:
                if len(a64[b]) >= k:
                    assert alpha[b] == np.float32(a64[b][k - 1]), (label, "iteration", k, "trajectory", b, alpha[b],
                                                                   a64[b][k - 1])
        # --- the iterate.  A dozen ill-conditioned Newton steps amplify a 1e-3 difference in the gains chaotically
        # (the fp32 oracle is 1e-4 .. 0.6 away from the fp64 one after six iterations, trajectory by trajectory, and
        # so are the kernels): the controls are compared where one step was taken, the objective everywhere
        fin = agree & np.isfinite(r64[2])
        one = fin & (r64[6] <= 1)
        if one.any():
            for key, j in (("U", 1), ("X", 0)):
                # (max-norm only: the per-entry rule on one ill-conditioned step is the business of
                # test_ilqr_single_iteration_teacher_forced, from identical starts)
                gu.assert_parity(f"{label} {key} (<= 1 iteration)", out[key].cpu().numpy()[one], r32[j][one],
                                 r64[j][one], tol=tol, ceiling=gu.GAIN_CEILING, el_tol=1.0)
        if fin.any():
            gu.assert_parity(f"{label} obj", out["obj"].cpu().numpy()[fin], r32[2][fin], r64[2][fin], tol=tol_obj,
                             ceiling=gu.GAIN_CEILING)
        nanb = np.isnan(r64[2])
        assert np.isnan(out["obj"].cpu().numpy()[nanb]).all()
        return eng, out, r64, agree
    except Exception:
        eng.close()
        raise


def test_full_steps_on_a_tame_problem():
    pb = _problem(1, out_scale=0.05)
    pb["U"] = (pb["U"] * 1e-2).astype(np.float32)
    # (|u| ~ a = 1e-2 and two iterations: with |u| << a the tame problem is converged to fp32 rounding after one
    # step and its next line search compares noise -- the CPU test runs that form in fp64, for five iterations)
    eng, out, r64, agree = _run(pb, {"maxiter": 2}, label="full steps", tol=1e-5, min_agree=1.0)
    assert (out["iterations"].cpu().numpy() == 2).all()
    eng.close()


def test_deep_backtracking():
    pb = _problem(3, out_scale=1.0, B=4)
    eng, out, r64, agree = _run(pb, {"maxiter": 6}, label="deep backtracking", tol=1e-4, tol_obj=3e-5, min_agree=0.75)
    eng.close()


def test_nan_start_never_iterates_and_neighbours_do():
    pb = _problem(5, out_scale=0.05)
    U = pb["U"].copy()
    U[1, 2, 0] = np.nan
    eng, out, r64, agree = _run(pb, {"maxiter": 4}, U, label="nan start", min_agree=1.0)
    it = out["iterations"].cpu().numpy()
    assert it[1] == 0 and it[0] > 0 and it[2] > 0
    assert np.isnan(out["obj"].cpu().numpy()[1])
    eng.close()


# thresholds chosen so that the members of the batch stop at DIFFERENT iterations between 1 and 10 (the criterion's
# quantities along the unconstrained solve of this problem are listed in scratch form in the commit message)
@pytest.mark.parametrize("kw", [
    {"grad_norm_threshold": 0.6},                     # has_potential: absolute gradient norm
    {"relative_grad_norm_threshold": 0.03},           # has_potential: relative to |obj| + 1
    {"obj_step_threshold": 0.005},                    # still_improving_obj
    {"inputs_step_threshold": 0.3},                   # still_moving_U
    {"alpha_min": 0.01},                              # line search exhausted: alpha <= alpha_min stops the loop
    {"alpha_0": 0.6, "alpha_min": 0.01},
])
def test_each_threshold_of_the_continuation_criterion(kw):
    pb = _problem(7, out_scale=0.6, B=4)
    kw = dict(kw, maxiter=12)
    # (round 4: 1e-4 where round 3 allowed 1e-3 -- the achieved errors are 1e-8 .. 1e-4, profiles/parity_r04.md)
    eng, out, r64, agree = _run(pb, kw, label="threshold " + "/".join(kw), tol=1e-4, min_agree=0.75)
    with np.errstate(all="ignore"):
        q = orc.cast_problem(pb, np.float64)
        base = orc.ilqr(q["dyn"], q["cmlp"], q["mpc_w"], q["goal"], q["x0"], q["U"], {"maxiter": 12})
    assert (r64[6] < base[6]).any(), "the threshold under test never stopped a trajectory early"
    eng.close()


def _noop_check(eng, pb, kw, stop, more_keys=()):
    """more_keys: outputs of ilqr_solve compared on top of X, U, obj, iterations (e.g. "grad", "adjoints")"""
    d = eng.to_dev
    keys = ("X", "U", "obj", "iterations") + tuple(more_keys)
    ref = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), dict(kw, maxiter=stop))
    snap = {k: ref[k].clone() for k in keys}
    for extra in (POLL_DEPTH, 20):
        more = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), dict(kw, maxiter=stop + extra))
        for k in keys:
            assert torch.equal(more[k], snap[k]), f"maxiter = {stop} + {extra}: {k} changed after the last stop"


def test_members_stop_at_different_iterations_and_the_enqueued_tail_is_a_no_op():
    pb = _problem(9, out_scale=0.6, B=5)
    kw = {"maxiter": 15, "obj_step_threshold": 0.01}
    eng, out, r64, agree = _run(pb, kw, label="heterogeneous stops", tol=1e-4, tol_obj=1e-5, min_agree=0.8)
    it = out["iterations"].cpu().numpy()
    assert len(set(it.tolist())) > 1 and it.max() < 15
    # every trajectory has stopped on the threshold before maxiter: later iterations must change nothing
    _noop_check(eng, pb, kw, int(it.max()))
    eng.close()


@pytest.mark.parametrize("ls16", [False, True, "ls32"])
def test_headline_shape_heterogeneous_stops(ls16, monkeypatch):
    """n = 17, m = 6, hidden 3 x 200 (the register-weight rollout / two-wave Riccati / MFMA chain kernels; ls16: the
    16-candidate line search forced for every round; ls32: the two-group form), 40 trajectories that stop between
    iterations 1 and 6."""
    if ls16:
        monkeypatch.setenv("GMPC_LS16_SPLIT", "1")
        monkeypatch.delenv("GMPC_LS", raising=False)
    if ls16 == "ls32":
        monkeypatch.setenv("GMPC_LS32_SPLIT", "1")
    pb = _problem(21, out_scale=0.1, B=40, n=17, m=6, T=20, hidden=(200, 200, 200), cost_hidden=(128, 128), fout=10)
    kw = {"maxiter": 6, "obj_step_threshold": 0.0007}
    eng, out, r64, agree = _run(pb, kw, label="headline shape" + (f" {ls16 if ls16 == 'ls32' else 'ls16'}" if ls16 else ""),
                                min_agree=0.65, tol=1e-3, tol_obj=3e-4)      # (27 of the 40 trajectories are decided)
    it = out["iterations"].cpu().numpy()
    assert len(set(it.tolist())) > 1
    if it.max() < 6:
        _noop_check(eng, pb, kw, int(it.max()))
    eng.close()

