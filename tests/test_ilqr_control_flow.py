"""The iLQR control flow has two authors' worth of restatements: oracle/gan_mpc_oracle.py (batched NumPy,
hand-derived derivatives, masked "frozen trajectory" updates) and tests/torch_ref.py:ilqr_scalar (one
trajectory, Python while loops, torch autograd), both written from trajax' published algorithm
(optimizers.py ilqr_base / line_search_ddp, tvlqr.py; pinned commit c94a637, reference requirements.txt:51)
and sharing no code.  They must agree on iteration counts, on the step size every line search returns
(exact: powers of two) and on the iterates (fp64 rounding), for: full steps, deep backtracking, a NaN
start, each of the five thresholds of the continuation criterion, an exhausted line search, and a batch
whose members stop at different iterations (frozen members untouched).  Reference call sites:
policy/optimizers.py:19-21,55-57, policy/eval.py:10-20."""

import numpy as np
import pytest
import torch

import control_flow_cases as cfc
import gan_mpc_oracle as orc
import torch_ref as tr


def _problem(seed, out_scale=1.0, B=3, n=5, m=2, T=8):
    pb = orc.make_problem(n, m, T, B, seed=seed, dtype=np.float64, dyn_hidden=(16, 16), cost_hidden=(12,),
                          cost_fout=4, bias_scale=0.1)
    W, b = pb["dyn"][-1]
    pb["dyn"][-1] = (W * out_scale, b * out_scale)
    return pb


def _both(pb, kw, U=None):
    U = pb["U"] if U is None else U
    trace = []
    with np.errstate(all="ignore"):
        r = orc.ilqr(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], pb["x0"], U, kw, trace=trace)
    lstm = isinstance(pb["dyn"], dict)          # the LSTM dynamics variant: dict(Wx, Wh, b, tail)
    dyn = tr.lstm_dynamics64(pb["dyn"]) if lstm else tr.layers64(pb["dyn"])
    cm, w = tr.layers64(pb["cmlp"]), tr.t64(pb["mpc_w"])
    scal = [tr.ilqr_scalar(dyn, cm, w, tr.t64(pb["goal"][b]), tr.t64(pb["x0"][b]), tr.t64(U[b]), kw)
            for b in range(U.shape[0])]
    return r, trace, scal


def _assert_same(r, trace, scal, rtol=1e-8):
    its = np.array([s["iteration"] for s in scal])
    np.testing.assert_array_equal(r[6], its)
    # the alpha each trajectory carries when it stops (returned by its last line search, or alpha_0)
    np.testing.assert_array_equal(trace[-1]["alpha"], np.array([s["alpha"] for s in scal]))
    # ... and after every iteration it took part in
    for b, s in enumerate(scal):
        seen = [tr_["alpha"][b] for i, tr_ in enumerate(trace[1:], 1) if trace[i - 1]["active"][b]]
        assert seen == s["alphas"], (b, seen, s["alphas"])
    for b, s in enumerate(scal):
        if np.isnan(r[2][b]):
            assert bool(torch.isnan(s["obj"]))
            continue
        np.testing.assert_allclose(s["U"].numpy(), r[1][b], rtol=rtol, atol=1e-10)
        np.testing.assert_allclose(s["X"].numpy(), r[0][b], rtol=rtol, atol=1e-10)
        np.testing.assert_allclose(float(s["obj"]), r[2][b], rtol=rtol)
        np.testing.assert_allclose(s["gradient"].numpy(), r[3][b], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(s["adjoints"].numpy(), r[4][b], rtol=1e-6, atol=1e-9)


def test_full_steps_on_a_tame_problem():
    """The smooth-L2 action cost sqrt(|u|^2 + a^2), a = 1e-2, is far from quadratic at |u| ~ 1 (its Newton
    step overshoots by |u|^2 / a^2), so iLQR backtracks deeply on ordinary starts; with |u| << a the
    model is nearly quadratic and the full step alpha_0 is taken."""
    pb = _problem(1, out_scale=0.05)
    pb["U"] = pb["U"] * 1e-3
    r, trace, scal = _both(pb, {"maxiter": 5})
    _assert_same(r, trace, scal)
    assert any(a == 0.5 for s in scal for a in s["alphas"])          # accepted alpha_0 returns alpha_0 / 2


def test_deep_backtracking():
    pb = _problem(3, out_scale=1.0, B=4)
    r, trace, scal = _both(pb, {"maxiter": 6})
    _assert_same(r, trace, scal, rtol=1e-7)
    assert min(a for s in scal for a in s["alphas"]) <= 2.0 ** -6      # several halvings were needed


def test_nan_start_never_iterates_and_neighbours_do():
    pb = _problem(5, out_scale=0.05)
    U = pb["U"].copy()
    U[1, 2, 0] = np.nan
    r, trace, scal = _both(pb, {"maxiter": 4}, U)
    _assert_same(r, trace, scal)
    assert r[6][1] == 0 and np.isnan(r[2][1]) and r[6][0] > 0 and r[6][2] > 0


@pytest.mark.parametrize("kw", [
    {"grad_norm_threshold": 5.0},                     # has_potential: absolute gradient norm
    {"relative_grad_norm_threshold": 0.2},            # has_potential: relative to |obj| + 1
    {"obj_step_threshold": 0.02},                     # still_improving_obj
    {"inputs_step_threshold": 0.3},                   # still_moving_U
    {"alpha_min": 0.2},                               # line search exhausted: alpha <= alpha_min stops the loop
    {"alpha_0": 0.6, "alpha_min": 0.01},
])
def test_each_threshold_of_the_continuation_criterion(kw):
    pb = _problem(7, out_scale=0.6, B=4)
    kw = dict(kw, maxiter=12)
    r, trace, scal = _both(pb, kw)
    _assert_same(r, trace, scal, rtol=1e-5)     # a dozen ill-conditioned Newton steps amplify fp64 rounding
    base = orc.ilqr(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], pb["x0"], pb["U"], {"maxiter": 12})
    assert (r[6] < base[6]).any(), "the threshold under test never stopped a trajectory early"


def test_members_stop_at_different_iterations_and_stay_frozen():
    pb = _problem(9, out_scale=0.6, B=5)
    kw = {"maxiter": 15, "obj_step_threshold": 0.01}
    r, trace, scal = _both(pb, kw)
    _assert_same(r, trace, scal, rtol=1e-5)
    assert len(set(r[6].tolist())) > 1
    # a member solved alone gives the same answer as inside the batch (frozen = untouched)
    b = int(np.argmin(r[6]))
    alone = orc.ilqr(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"][b:b + 1], pb["x0"][b:b + 1],
                     pb["U"][b:b + 1], kw)
    np.testing.assert_allclose(alone[1][0], r[1][b], rtol=1e-10)    # BLAS batch size changes the last bits
    assert alone[6][0] == r[6][b]


# The oracle's ilqr OFF the small-state MLP shapes -- the arbiter of tests/test_gpu_control_flow_paths.py there: the
# LSTM dynamics variant (state [x, c, h], goals with the x columns only) and more controls than states
@pytest.mark.parametrize("name,seed,opts", [
    ("dynl-small", 7, {"obj_step_threshold": 0.003}),
    ("m40", 3, {"alpha_min": 0.01}),
])
def test_the_lstm_variant_and_more_controls_than_states(name, seed, opts):
    pb = orc.cast_problem(cfc.problem(name, seed), np.float64)
    r, trace, scal = _both(pb, dict(opts, maxiter=12))
    _assert_same(r, trace, scal, rtol=1e-5)     # (as the threshold rows above: up to a dozen Newton steps)
    assert len(set(r[6].tolist())) > 1 and r[6].max() < 12
