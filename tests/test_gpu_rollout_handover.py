"""The register-weight rollout (k_traj_rw<false, ...>, gmpc_traj_rw.hip) hands the state from the output layer to
layer 0 in registers: every wave forms its layer-0 operand from the output layer's partial sums, the old state it
kept and the control it loaded one step ahead.  The additions and their order are the ones of the form that went
through LDS, so nothing may move by a bit.

(a) Bitwise against fixtures recorded from the library of the commit before the hand-over
    (tests/golden/rollout_handover/<case>.npz, written by tests/golden/make_rollout_handover.py): the states, the
    costs, and AB / K / k / grad of the backward pass run after the rollout -- the Jacobian chain reads the relu
    mask words the rollout wrote, so the last four show that the masks did not move.
(b) Against the fp64 oracle at test_gpu_parity.test_rollout_cost's bars, so that the file still means something
    should the fixtures ever be recorded again.

The shapes are the smallest at which the hand-over can go wrong; see CASES."""

import functools
import os

import numpy as np
import pytest

import gan_mpc_oracle as orc
import gpu_util as gu

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "rollout_handover")
SEED = 11
H128 = dict(dyn_hidden=(128, 128, 128), cost_hidden=(32,), cost_fout=4, out_scale=0.3)
H64 = dict(dyn_hidden=(64, 64, 64), cost_hidden=(16,), cost_fout=3, out_scale=0.3)
CASES = {
    # name: (n, m, T, B, kwargs of gpu_util.problem)
    "one-step": (17, 6, 1, 6, {}),                 # the first step is the last: no reload, final state after one step
    "two-steps": (17, 6, 2, 3, {}),                # B = 3 < the 4 slots of a workgroup
    "three-steps": (17, 6, 3, 3, {}),              # the partial-sum buffer is rewritten twice
    "ragged": (17, 6, 9, 7, {}),                   # second workgroup with one unused slot
    "n16-m8": (16, 8, 4, 5, {}),                   # the state fills operand register 0 exactly, the controls register 1
    "wide-io": (22, 9, 5, 6, dict(out_scale=0.3)),  # 8 input groups, the state crosses into register 1, m > 8
    "h128": (9, 3, 12, 10, H128),                  # waves 2-3 hold no neuron
    "h64": (6, 2, 9, 7, H64),                      # waves 1-3 hold no neuron
}
NAN_CASE, NAN_AT = "ragged", (5, 2, 3)             # U[trajectory 5 (slot 1 of workgroup 1), step 2, control 3] = NaN
BACKWARD_KEYS = ("AB", "K", "k", "grad")


def problem(name):
    n, m, T, B, kw = CASES[name]
    return gu.problem(n, m, T, B, seed=SEED, **kw)


def run_case(name, nan=False):
    """The rollout (and, without the NaN, the backward pass after it) of one case on the GPU: name -> array."""
    import torch
    pb = problem(name)
    gu.set_config(f"handover {name} n={pb['n']} m={pb['m']} T={pb['T']} B={pb['B']}")
    U = pb["U"].copy()
    if nan:
        U[NAN_AT] = np.nan
    eng = gu.engine_for(pb, critic=False)
    d = eng.to_dev
    Xd, costs = eng.rollout_cost(d(pb["x0"]), d(U), d(pb["goal"]))
    out = dict(x0=pb["x0"], U=U, X=Xd.cpu().numpy(), costs=costs.cpu().numpy())
    if not nan:
        bw = eng.lqr_backward(Xd, d(U), d(pb["goal"]), after_rollout=True)
        for key in BACKWARD_KEYS:
            out[key] = bw[key].cpu().numpy()
    torch.cuda.synchronize()
    eng.close()
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


_run = functools.lru_cache(maxsize=None)(run_case)   # each case runs once, shared by (a) and (b); read only


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _golden(tag):
    return np.load(os.path.join(GOLDEN, tag + ".npz"))


@pytest.mark.parametrize("name", list(CASES))
def test_bitwise_against_parent(name):
    got, G = _run(name), _golden(name)
    assert int(G["seed"]) == SEED
    for key in ("x0", "U"):        # the seed still makes the inputs the fixture was recorded on
        assert np.array_equal(_bits(got[key]), _bits(G[key])), key
    for key in ("X", "costs") + BACKWARD_KEYS:
        assert got[key].shape == G[key].shape, key
        assert np.array_equal(got[key], G[key]), (key, int((_bits(got[key]) != _bits(G[key])).sum()))


def test_nan_stays_in_its_slot():
    """A NaN in one trajectory's controls: that trajectory's outputs have the parent's bits (NaNs included), and
    every other trajectory -- the other slots of its workgroup among them -- has the bits of the run without it."""
    got, G, clean = _run(NAN_CASE, True), _golden(NAN_CASE + "-nan"), _run(NAN_CASE)
    b, t, _ = NAN_AT
    assert np.array_equal(_bits(got["U"]), _bits(G["U"]))
    for key in ("X", "costs"):
        assert np.array_equal(_bits(got[key]), _bits(G[key])), key
        others = np.arange(got[key].shape[0]) != b
        assert np.array_equal(_bits(got[key][others]), _bits(clean[key][others])), key
        assert np.isfinite(got[key][others]).all(), key
    assert np.isnan(got["costs"][b, t])
    assert np.array_equal(_bits(got["X"][b, :t + 1]), _bits(clean["X"][b, :t + 1]))


@pytest.mark.parametrize("name", list(CASES))
def test_against_fp64_oracle(name):
    got, pb = _run(name), problem(name)
    pb64 = orc.cast_problem(pb, np.float64)
    X32 = orc.rollout(pb["dyn"], pb["U"], pb["x0"])
    X64 = orc.rollout(pb64["dyn"], pb64["U"], pb64["x0"])
    gu.assert_parity("X", got["X"], X32, X64)
    c32 = orc.evaluate(pb["cmlp"], pb["mpc_w"], pb["goal"], X32, pb["U"])
    c64 = orc.evaluate(pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X64, pb64["U"])
    gu.assert_parity("costs", got["costs"], c32, c64)
