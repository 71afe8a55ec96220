"""Rows 16..n-1 of the sparse Jacobian chain run inside k_linearize_sparse as group jobs: one tile column per sample
of up to 16 consecutive samples, contracted over the UNION of their active lists, every column zeroed by its own
sample's relu mask at each hand-over.  The result is still the dense chain's, bit for bit.

Every case runs the same inputs through the default route and through GMPC_LIN=dense and compares with
assert_array_equal (test_gpu_linearize_sparse._check_backward).  A wave takes a contiguous chunk of
C = ceil(T B / waves of the grid) samples, and the grid has one wave per sample up to 2048 waves: below 2049 samples
every group has ONE column, so each property is checked at a small shape (C = 1) and at one with T B > 2048 (C > 1,
columns of different samples in one tile)."""
import numpy as np
import pytest

import gpu_util as gu
from test_gpu_linearize_sparse import _both, _check_backward, _force


def _run(n, m, T, B, seed=31, prepare=None):
    pb = gu.problem(n, m, T, B, seed=seed)
    if prepare is not None:
        prepare(pb)
    eng = gu.engine_for(pb, critic=False)
    return eng, pb


# T B below, at and just above 16; chunks of one sample; a chunk that spans trajectories (T = 7: C = 3); T B = 4200 is
# 1400 whole chunks of 3, 4207 leaves a last chunk of one sample; 36000 samples are chunks of 18 = two groups of 9
@pytest.mark.gpu
@pytest.mark.parametrize("T,B", [(1, 1), (3, 5), (16, 1), (17, 1), (33, 2), (50, 3), (7, 600), (7, 601), (50, 720)])
def test_ragged_chunks_and_groups(T, B, monkeypatch):
    eng, pb = _run(17, 6, T, B)
    _check_backward(eng, pb, monkeypatch)


# n = 12, 16: no group jobs; n = 18, 20: two and four rows, each with its own group jobs
@pytest.mark.gpu
@pytest.mark.parametrize("T,B", [(4, 6), (7, 601)])
@pytest.mark.parametrize("n", [12, 16, 18, 20])
def test_no_extra_rows_and_several(n, T, B, monkeypatch):
    eng, pb = _run(n, 6, T, B)
    _check_backward(eng, pb, monkeypatch)


def _complementary(full_upper):
    """Layer 0 sees u_0 only: even units respond to +u_0, odd units to -u_0, and u_0 changes sign every step, so
    consecutive samples have complementary layer-0 masks (union: all 200 units, intersection: none)."""
    def prepare(pb):
        n = pb["n"]
        W, b = pb["dyn"][0]
        W = np.zeros_like(W)
        W[n, 0::2] = 1.0
        W[n, 1::2] = -1.0
        pb["dyn"][0] = (W, np.zeros_like(b))
        sign = np.where(np.arange(pb["T"]) % 2 == 0, 1.0, -1.0).astype(np.float32)
        pb["U"][:, :, 0] = 0.5 * sign[None, :]
        if full_upper:
            _force(pb, 1, range(200))
            _force(pb, 2, range(200))
    return prepare


# (4, 3) is the shape the issue names; (4, 600) and (5, 1300) put two and four consecutive samples into one tile, the
# second with chunks that start at odd steps and span trajectories
@pytest.mark.gpu
@pytest.mark.parametrize("T,B", [(4, 3), (4, 600), (5, 1300)])
@pytest.mark.parametrize("full_upper", [False, True])
def test_columns_that_disagree(full_upper, T, B, monkeypatch):
    eng, pb = _run(17, 6, T, B, prepare=_complementary(full_upper))
    AB = _check_backward(eng, pb, monkeypatch)
    # the inputs do what they are built for: row 16 depends on u_0 alone
    assert np.count_nonzero(AB[:, :, 16, :17] - np.eye(17, dtype=AB.dtype)[16]) == 0


# the later iterations run the chain with the `active` filter: converged trajectories are empty columns of a group
@pytest.mark.gpu
@pytest.mark.parametrize("T,B", [(5, 6), (5, 900)])
def test_active_across_a_group(T, B, monkeypatch):
    eng, pb = _run(17, 6, T, B, seed=11)
    d = eng.to_dev
    n, m = pb["n"], pb["m"]

    def run():
        out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 5})
        out["AB"] = eng.debug_buffer(5, (B, T, n, n + m)).clone()
        return out
    out = _both(eng, run, monkeypatch)
    sp, de = out["sparse"][0], out["dense"][0]
    for key in ("X", "U", "obj", "grad", "iterations", "AB"):
        np.testing.assert_array_equal(sp[key], de[key], err_msg=key)


@pytest.mark.gpu
def test_kernel_name(monkeypatch):
    eng, pb = _run(17, 6, 3, 5)
    eng.profile_enable(True)
    out = _both(eng, lambda: eng.lqr_backward(*_xug(eng, pb), after_rollout=True), monkeypatch)
    eng.profile_enable(False)
    name = out["sparse"][1]
    assert name.startswith("k_linearize_sparse"), name
    assert "k_linearize_regs" not in name, name
    assert out["dense"][1].startswith("k_linearize_regs"), out["dense"][1]


def _xug(eng, pb):
    d = eng.to_dev
    x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
    X, _ = eng.rollout_cost(x0, U, goal)
    return X, U, goal
