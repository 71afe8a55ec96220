"""The cases of the ensemble fit's tests (tests/test_ensemble_fit_host.py, tests/test_gpu_ensemble_fit.py;
gmpc_dynamics_ensemble_loss_grad; TEST INFRASTRUCTURE).

Shapes: cem_cases' base (n 5, m 2), ragged (hidden (7, 9): partial column tiles and a K tail), cheetah (n 17, m 6,
3 x 200), w256 (the width cap) and wide_n (n 64); the members are sampled_ensemble_cases.members'.  The call does not
read the horizon beyond S <= T, and the networks do not depend on it (gu.problem draws them first), so every engine
here has T = 8 and all of S in {1, 5, T} run on every shape.  B in {7, 33, 65}: less than one tile of 32 sequences,
one tile and one row, three tiles with a partial last one.  Inputs as tests/test_gpu_parity.py::test_dynamics_loss_grad
draws them: standard normal x and y, tanh of a standard normal for u, discount 0.95.

The training problem of the trainer's tests: windows rolled out under a fixed teacher network (gu.problem's n 5, m 2,
hidden (7, 9)), 64 windows of S = 4; students from nn_init.dense_tree under seeds STUDENT_SEED + p."""

import functools

import numpy as np

import gan_mpc_oracle as orc
import gpu_util as gu
import sampled_ensemble_cases as ec
from gan_mpc_amd import nn_init, params as P

NAMES = ("base", "ragged", "cheetah", "w256", "wide_n")
T = 8
BATCHES = (7, 33, 65)
STEPS = (1, 5, T)
MAX_BATCH = 65
DISCOUNT = 0.95
DATA_SEED = 21


def dims(name):
    """(n, m, dynamics widths, cost widths) of the case."""
    pb = ec.problem(name)
    dyn = [pb["dyn"][0][0].shape[0]] + [W.shape[1] for W, _ in pb["dyn"]]
    cost = [pb["cmlp"][0][0].shape[0]] + [W.shape[1] for W, _ in pb["cmlp"]]
    return pb["n"], pb["m"], dyn, cost


def new_engine(name, max_batch=MAX_BATCH):
    """An engine of the case's shape with NO parameters bound: the call reads none."""
    from gan_mpc_amd.engine import Engine
    n, m, dyn, cost = dims(name)
    return Engine(n, m, T, dyn, cost, max_batch)


@functools.lru_cache(maxsize=None)
def data(name, D, S):
    n, m, _, _ = dims(name)
    rng = np.random.default_rng(DATA_SEED)
    xseq = rng.standard_normal((D, S, n)).astype(np.float32)
    useq = np.tanh(rng.standard_normal((D, S, m))).astype(np.float32)
    yseq = rng.standard_normal((D, S, n)).astype(np.float32)
    return xseq, useq, yseq


def draw_rows(P_, B, D, seed=0):
    """(P, B) int32 dataset rows, with a duplicate inside every member wherever B > 1."""
    idx = np.random.default_rng(seed).integers(0, D, size=(P_, B)).astype(np.int32)
    if B > 1:
        idx[:, B - 1] = idx[:, 0]
    return idx


def flat_grad(g):
    return np.concatenate([t.ravel() for Wb in g for t in Wb])


def oracle(layers, xseq, useq, yseq, tf, dtype):
    """(mean loss, flat mean gradient) of one member in `dtype`."""
    cast = [(W.astype(dtype), b.astype(dtype)) for W, b in layers]
    l, g = orc.dynamics_fit_loss_and_grad(cast, xseq.astype(dtype), useq.astype(dtype), yseq.astype(dtype), DISCOUNT, tf)
    return l, flat_grad(g)


# ---- the training problem ---------------------------------------------------------------------------------------------
TRAIN = dict(n=5, m=2, hidden=(7, 9), windows=64, S=4, teacher_seed=31, data_seed=32, P=3, batch_size=16,
             num_updates=12, lr=1e-2, teacher_forcing_factor=0.0, key=5)
# (teacher_forcing_factor 0: every update runs free, so the first and the last update's losses are the same quantity
# -- a schedule that switches modes half-way compares a teacher-forced loss with a free-running one -- and the sweep
# back through time is what trains.  On the fp64 reference the three losses fall from 27 / 24 / 37 to 4.6 / 7.4 / 3.7.)
STUDENT_SEED = 40
ADAM = dict(max_norm=100.0, b1=0.9, b2=0.999, eps=1e-8)


def train_dims():
    return [TRAIN["n"] + TRAIN["m"], *TRAIN["hidden"], TRAIN["n"]]


@functools.lru_cache(maxsize=None)
def train_dataset():
    """(xseq, useq, next_xseq), each (64, 4, .): x_{t+1} = x_t + MLP_teacher([x_t; u_t]) in fp64, stored as fp32."""
    n, m, S, D = TRAIN["n"], TRAIN["m"], TRAIN["S"], TRAIN["windows"]
    teacher = gu.problem(n, m, T, 1, seed=TRAIN["teacher_seed"], dyn_hidden=TRAIN["hidden"])["dyn"]
    rng = np.random.default_rng(TRAIN["data_seed"])
    x = rng.standard_normal((D, n))
    useq = np.tanh(rng.standard_normal((D, S, m)))
    xs, ys = [], []
    for t in range(S):
        a = np.concatenate([x, useq[:, t]], axis=1)
        for l, (W, b) in enumerate(teacher):
            a = a @ W.astype(np.float64) + b.astype(np.float64)
            if l < len(teacher) - 1:
                a = np.maximum(a, 0)
        xs.append(x)
        x = x + a
        ys.append(x)
    f = lambda v: np.ascontiguousarray(np.stack(v, axis=1).astype(np.float32))
    return f(xs), useq.astype(np.float32), f(ys)


def students(count=None, same=False):
    """(P, dyn count) fp32: student p from nn_init.dense_tree under seed STUDENT_SEED + p (same: all from member 0's)."""
    count = TRAIN["P"] if count is None else count
    return np.stack([P.pack_mlp(nn_init.dense_tree(np.random.default_rng(STUDENT_SEED + (0 if same else p)),
                                                   train_dims())) for p in range(count)]).astype(np.float32)


class EnginePolicy:
    """What ensemble_trainer asks of a policy, around one engine: device(), engine_for(), a bound marker."""

    def __init__(self, eng):
        self._engine, self._bound = eng, True

    def device(self):
        return self._engine.device

    def engine_for(self, batch, dparams=None):
        assert batch <= self._engine.max_batch
        return self._engine
