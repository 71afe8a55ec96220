"""The iLQR control flow of gmpc_ilqr_solve OFF the small-state MLP path, against the fp64 oracle: the protocol of
tests/test_gpu_control_flow.py (its _run: iteration counts and the step size after every iteration EQUAL to the
oracle's wherever the control flow is decided, iterates and objectives through assert_parity) on the code that runs
instead of the small-state kernels there --

  * the step-major large-state pipeline (n > 64, or m > 32), dense and low-rank: backward_pass' c->big branch, the
    continuation test k_big_cont on the gn2 that k_big_init / k_big_step build, the per-trajectory `active` mask in
    k_big_init, every batched GEMM, k_btranspose, k_big_step, k_big_pupdate, k_add_identity, the strided Jacobian
    chains and k_terminal, the side stream's double-buffered Jacobians from one backward pass to the next, the
    line-search candidates through the generic k_traj<true>;
  * the LSTM dynamics variant on both pipelines: candidates by k_dynl_traj<true>, Jacobians by k_dynl_jac, goals with
    nx columns beside a state of nx + 2F, k_ls_decide committing with the tail network's layer count.

The rows (tests/control_flow_cases.py) backtrack 7-12 halvings, so they reach the second and third line-search rounds,
and their members stop at different iterations.  Per row: the path is asserted; thresholds must have stopped a member
early; a NaN start never iterates and its neighbours do; where everything stops below maxiter the iterations the host
enqueues after the last stop are exact no-ops in X, U, obj, iterations AND grad, adjoints; the returned gradient and
adjoints are those of a fresh linearisation AT the returned iterate for every finite trajectory, stopped ones
included (a held gradient rewritten after the stop, or left one iteration stale, shows here).  Without an oracle: the
same solve twice, and the batch in another order, return the same bits."""

import functools

import numpy as np
import pytest
import torch

import control_flow_cases as cfc
import gan_mpc_oracle as orc
import gpu_util as gu
import test_gpu_control_flow as cf

pytestmark = pytest.mark.gpu

# all but one trajectory has to be decided (a cap: the oracle alone reaches 1.0 on every row; the margin of one
# trajectory allows for another NumPy / BLAS build)
MIN_AGREE = {4: 0.75, 5: 0.8, 6: 0.8}
TOL = 1e-4          # iterates and objective: the bar of the one-iteration tests on these shapes
OUT_KEYS = ("X", "U", "obj", "grad", "adjoints", "iterations")


def _assert_path(eng, name):
    """a later dispatch change must not turn these into tests of another path silently"""
    big, lstm = cfc.PROBLEMS[name][5:]
    assert eng.big == big, f"{name}: the step-major pipeline is {'not ' if big else ''}taken"
    assert bool(eng.shape.dyn_lstm_features) == lstm, f"{name}: LSTM dynamics flag {eng.shape.dyn_lstm_features}"


@functools.lru_cache(maxsize=None)
def _unconstrained_iterations(name, seed, maxiter):
    """fp64 oracle, the same solve with every threshold at its default"""
    q = orc.cast_problem(cfc.problem(name, seed), np.float64)
    with np.errstate(all="ignore"):
        return orc.ilqr(q["dyn"], q["cmlp"], q["mpc_w"], q["goal"], q["x0"], q["U"], {"maxiter": maxiter})[6]


def _grad_at_the_returned_iterate(label, pb, out):
    """out["grad"], out["adjoints"] against the oracles' linearisation at the GPU's own (X, U): every finite
    trajectory, whether its control flow is decided or not, away from the relu kinks."""
    pb64 = orc.cast_problem(pb, np.float64)
    T = pb["T"]
    Xg, Ug = out["X"].cpu().numpy(), out["U"].cpu().numpy()
    fin = np.isfinite(out["obj"].cpu().numpy()) & np.isfinite(Xg).all((1, 2)) & np.isfinite(Ug).all((1, 2))
    assert fin.sum() >= pb["B"] - 1
    Xg, Ug = Xg[fin], Ug[fin]
    X64, U64 = Xg.astype(np.float64), Ug.astype(np.float64)
    bad = gu.dyn_near_kink(pb64["dyn"], X64, U64)
    bad[:, -1] |= gu.near_kink(pb64["cmlp"], X64[:, T])
    ok = ~bad.any(axis=1)
    assert 2 * ok.sum() >= fin.sum(), "too many trajectories near a relu kink at the returned iterate"
    l32 = orc.get_lqr_params(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"][fin], Xg, Ug)
    l64 = orc.get_lqr_params(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"][fin], X64, U64)
    g32, a32 = orc.adjoint(l32[5], l32[6], l32[1], l32[3])
    g64, a64 = orc.adjoint(l64[5], l64[6], l64[1], l64[3])
    gu.assert_parity(f"{label} grad at the returned iterate", out["grad"].cpu().numpy()[fin][ok], g32[ok], g64[ok])
    gu.assert_parity(f"{label} adjoints at the returned iterate", out["adjoints"].cpu().numpy()[fin][ok], a32[ok],
                     a64[ok])


def _check_row(row, label):
    name, seed, opts, nan, maxiter = row
    pb = cfc.problem(name, seed)
    U = cfc.start(pb, nan)
    B = pb["B"]
    kw = dict(opts, maxiter=maxiter)
    eng, out, r64, agree = cf._run(pb, kw, U, label=label, tol=TOL, min_agree=MIN_AGREE[B])
    try:
        _assert_path(eng, name)
        assert agree.mean() >= MIN_AGREE[B]
        it = out["iterations"].cpu().numpy()
        if nan:
            assert it[1] == 0 and it[0] > 0 and it[2] > 0
            assert np.isnan(out["obj"].cpu().numpy()[1])
        else:
            assert len(set(it.tolist())) > 1, "the members of the batch stopped at one and the same iteration"
            base = _unconstrained_iterations(name, seed, maxiter)
            assert (r64[6] < base).any(), "the threshold under test never stopped a trajectory early"
        _grad_at_the_returned_iterate(label, pb, out)
        if r64[6].max() < maxiter:
            # every trajectory has stopped before maxiter: later iterations must change nothing
            assert it.max() < maxiter
            cf._noop_check(eng, pb, kw, int(it.max()), more_keys=("grad", "adjoints"))
    finally:
        eng.close()


@pytest.mark.parametrize("row", cfc.ROWS, ids=cfc.row_id)
def test_control_flow_on_the_large_state_and_lstm_paths(row):
    _check_row(row, cfc.row_id(row))


def test_dense_row_with_the_gain_solve_on_the_vector_pipe(monkeypatch):
    """k_big_step's other form of the gain solve (read from the environment once per backward pass)"""
    monkeypatch.setenv("GMPC_BIG_SOLVE", "valu")
    _check_row(cfc.ROWS[0], cfc.row_id(cfc.ROWS[0]) + " valu gain solve")


@pytest.mark.parametrize("row", [next(r for r in cfc.ROWS if r[0] == name) for name in ("dense", "lowrank", "dynl-big")],
                         ids=cfc.row_id)
def test_same_bits_on_a_second_solve_and_in_another_batch_order(row):
    """No oracle: the solve is deterministic, and the trajectories of a batch are independent -- handed over in
    another order they return the same bits in that order (tests/test_gpu_fullshape.py holds this at the headline
    size only).  On the dense problem the Jacobians of step t - 1 are written on the side stream while step t runs: a
    copy overwritten before its last reader, in this backward pass or the next one of the loop, differs from run to
    run."""
    name, seed, opts, nan, maxiter = row
    assert not nan
    pb = cfc.problem(name, seed)
    gu.set_config(f"bit identity {cfc.row_id(row)}")
    kw = dict(opts, maxiter=maxiter)
    eng = gu.engine_for(pb, critic=False)
    try:
        _assert_path(eng, name)
        d = eng.to_dev
        perm = np.random.default_rng(5).permutation(pb["B"])
        assert (perm != np.arange(pb["B"])).any()

        def solve(idx):
            o = eng.ilqr_solve(d(pb["x0"][idx]), d(pb["U"][idx]), d(pb["goal"][idx]), kw)
            torch.cuda.synchronize()
            return {k: o[k].cpu().numpy() for k in OUT_KEYS}
        ident = np.arange(pb["B"])
        first, second, permuted = solve(ident), solve(ident), solve(perm)
        assert len(set(first["iterations"].tolist())) > 1 and np.isfinite(first["obj"]).all()
        for k in OUT_KEYS:
            np.testing.assert_array_equal(second[k], first[k], err_msg=f"{k}: second solve of the same batch")
        for k in OUT_KEYS:
            np.testing.assert_array_equal(permuted[k], first[k][perm], err_msg=f"{k}: permuted batch")
    finally:
        eng.close()
