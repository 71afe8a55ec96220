"""Host tests of expert-model training: the torch restatement of the loss (tests/expert_fit_ref.py) pinned
against the oracle's expert forward and against finite differences, the minibatch and teacher-forcing
schedules, and the reference's names in gan_mpc_amd.expert.trainer / .runner."""

import importlib
import types

import numpy as np
import pytest
import torch

import expert_fit_ref as R
import gan_mpc_oracle as orc
from gan_mpc_amd import params as P, trainer_common as tc


def _model(rng, n, m, F, layers, hidden, dtype=np.float32):
    ex = orc.make_expert(rng, n, m, lstm_features=F, num_layers=layers, num_hidden_units=hidden, dtype=dtype)
    flat, F_, dx, du = P.pack_expert(ex)
    return ex, flat, F_, dx, du


@pytest.mark.parametrize("F", [16, 0])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forward_matches_oracle_rollout(F, dtype):
    rng = np.random.default_rng(1)
    n, m, B, S = 5, 2, 6, 4
    ex, flat, F_, dx, du = _model(rng, n, m, F, 3, 12)
    xseq, _, _ = R.make_windows(rng, B, S, n, m)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    exd = R.unflatten(torch.as_tensor(flat.astype(dtype), dtype=tdt), F_, dx, du)
    exo = {k: (dict((kk, vv.astype(dtype)) for kk, vv in v.items()) if isinstance(v, dict) else
               (tuple(a.astype(dtype) for a in v) if isinstance(v, tuple) else
                [(W.astype(dtype), b.astype(dtype)) for W, b in v])) for k, v in ex.items()}
    x = xseq.astype(dtype)
    tol = 1e-12 if dtype == np.float64 else 2e-6
    # teacher forcing off: the first state, then S steps on the model's own predictions
    nx, u = (a.numpy() for a in R.forward(exd, torch.as_tensor(x), False))
    goal, U = orc.expert_goal_states_init_actions(exo, x[:, :1], S)
    np.testing.assert_allclose(nx, goal[:, 1:], rtol=tol, atol=tol)
    np.testing.assert_allclose(u, U, rtol=tol, atol=tol)
    # teacher forcing on: every row fed, the last step's prediction
    nx, u = (a.numpy() for a in R.forward(exd, torch.as_tensor(x), True))
    goal, U = orc.expert_goal_states_init_actions(exo, x[:, :S], 1)
    np.testing.assert_allclose(nx[:, -1], goal[:, 1], rtol=tol, atol=tol)
    np.testing.assert_allclose(u[:, -1], U[:, 0], rtol=tol, atol=tol)


@pytest.mark.parametrize("F", [3, 0])
@pytest.mark.parametrize("teacher_forcing", [False, True])
@pytest.mark.parametrize("gamma", [0.9, 1.0])
def test_fp64_gradient_matches_finite_differences(F, teacher_forcing, gamma):
    rng = np.random.default_rng(7)
    n, m, B, S = 3, 2, 2, 3
    _, flat, F_, dx, du = _model(rng, n, m, F, 3, 4, dtype=np.float64)
    xseq, useq, yseq = R.make_windows(rng, B, S, n, m)
    flat = flat.astype(np.float64)
    _, g = R.loss_and_grad(flat, F_, dx, du, xseq, useq, yseq, gamma, teacher_forcing)
    fd = np.zeros_like(flat)
    h = 1e-6
    for i in range(flat.size):
        e = np.zeros_like(flat)
        e[i] = h
        fd[i] = (R.loss_only(flat + e, F_, dx, du, xseq, useq, yseq, gamma, teacher_forcing)
                 - R.loss_only(flat - e, F_, dx, du, xseq, useq, yseq, gamma, teacher_forcing)) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-5, atol=1e-7 * np.abs(fd).max())


def test_discount_by_repeated_multiplication():
    d = R.discounts(12, 0.9, np.float32)
    g = np.float32(0.9)
    acc = np.float32(1.0)
    for t in range(12):
        assert d[t] == acc
        acc = np.float32(acc * g)


def test_minibatch_schedule_draws_with_replacement():
    rng = np.random.default_rng(0)
    perm = tc.minibatch_schedule(rng, 10, 4)
    assert perm.shape == (10 // 4, 4)
    assert perm.min() >= 0 and perm.max() < 10
    big = tc.minibatch_schedule(np.random.default_rng(1), 20, 20)
    assert len(np.unique(big)) < 20          # with replacement: a full-size draw repeats indices


def test_module_names():
    trainer = importlib.import_module("gan_mpc_amd.expert.trainer")
    runner = importlib.import_module("gan_mpc_amd.expert.runner")
    for name in ("calculate_loss", "train_epoch", "train"):
        assert callable(getattr(trainer, name))
    for name in ("get_model", "get_params", "get_optimizer", "get_normalizer", "get_trainstate", "run"):
        assert callable(getattr(runner, name))


def test_train_schedules(monkeypatch):
    """trainer.train's host loop with the GPU calls stubbed out: datasize // batch_size minibatches per
    epoch drawn with replacement, teacher forcing while ep <= num_epochs * factor (reference trainer.py:61-107),
    test loss with teacher forcing off every print_step epochs and at the end."""
    trainer = importlib.import_module("gan_mpc_amd.expert.trainer")
    seen, tested = [], []

    def fake_epoch(state, perm, dataset, discount_factor, teacher_forcing):
        seen.append((np.array(perm), teacher_forcing))
        return state, float(len(seen))

    def fake_loss(state, params, dataset, discount_factor, teacher_forcing):
        tested.append(teacher_forcing)
        return -1.0

    monkeypatch.setattr(trainer, "train_epoch", fake_epoch)
    monkeypatch.setattr(trainer, "calculate_loss", fake_loss)
    data = tuple(np.zeros((23, 4, k), np.float32) for k in (3, 1, 3))
    st = types.SimpleNamespace(params=None)
    state, train_loss, test_loss = trainer.train(st, (data, data), num_epochs=10, batch_size=5, key=3,
                                                 discount_factor=0.9, teacher_forcing_factor=0.7, print_step=4)
    assert state is st and train_loss == 10.0 and test_loss == -1.0
    assert [tf for _, tf in seen] == [True] * 7 + [False] * 3
    assert all(p.shape == (23 // 5, 5) and p.min() >= 0 and p.max() < 23 for p, _ in seen)
    ref = np.random.default_rng(3)
    for p, _ in seen:
        np.testing.assert_array_equal(p, ref.choice(23, size=(4, 5)))
    assert tested == [False, False, False]     # epochs 4 and 8, then the final test loss


def test_unpack_expert_inverts_pack_expert():
    rng = np.random.default_rng(2)
    for F in (8, 0):
        ex = orc.make_expert(rng, 5, 2, lstm_features=F, num_layers=3, num_hidden_units=7)
        flat, F_, dx, du = P.pack_expert(ex)
        back, *_ = P.pack_expert(P.expert_dict_to_tree(P.unpack_expert(flat, F_, dx, du)))
        np.testing.assert_array_equal(back, flat)
