"""Expert-model training on the GPU: gmpc_expert_loss_grad against the torch restatement of reference
expert/nn.py + expert/trainer.py:calculate_loss (tests/expert_fit_ref.py) in fp32 and fp64, determinism,
caps, the trainer against an fp64 loop, the runner's saved artefacts and the environment policy."""

import os

import numpy as np
import pytest
import torch
import yaml

import expert_fit_ref as R
import gan_mpc_oracle as orc
import gpu_util as gu
from gan_mpc_amd import _lib, params as P, utils
from gan_mpc_amd.engine import make_expert_shape
from gan_mpc_amd.expert import expert_model, runner, trainer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (x_size, m, F (0 = MLP variant), num_layers, num_hidden_units, B, S)
CASES = {
    "lstm-pendulum": (3, 1, 128, 3, 128, 64, 10),
    "mlp-pendulum": (3, 1, 0, 3, 128, 64, 10),
    "lstm-cheetah": (17, 6, 128, 3, 128, 64, 10),
    "mlp-cheetah": (17, 6, 0, 3, 128, 64, 10),
    "lstm-ragged": (5, 3, 13, 2, 37, 7, 1),
    "mlp-ragged": (7, 5, 0, 3, 37, 9, 3),
    "lstm-wide": (376, 17, 64, 3, 128, 16, 5),
}


def _setup(name, seed=0):
    n, m, F, layers, hidden, B, S = CASES[name]
    rng = np.random.default_rng(seed)
    ex = orc.make_expert(rng, n, m, lstm_features=F, num_layers=layers, num_hidden_units=hidden)
    flat, F_, dx, du = P.pack_expert(ex)
    xseq, useq, yseq = R.make_windows(rng, B, S, n, m)
    eng = runner.make_engine(n, m, B)
    return eng, (flat, F_, dx, du), (xseq, useq, yseq)


def _gpu(eng, model, data, gamma, tf, want_grad=True):
    flat, F, dx, du = model
    d = eng.to_dev
    loss, grad = eng.expert_loss_grad(d(data[0]), d(data[1]), d(data[2]), d(flat), make_expert_shape(F, dx, du),
                                      gamma, tf, want_grad=want_grad)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), (grad.cpu().numpy() if grad is not None else None)


@pytest.mark.parametrize("tf", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_loss_grad_parity(name, tf):
    gu.set_config(f"expert fit {name} tf={tf}")
    eng, model, data = _setup(name)
    gamma = 0.9
    loss, grad = _gpu(eng, model, data, gamma, tf)
    l32, g32 = R.loss_and_grad(*model, *data, gamma, tf, dtype=np.float32)
    l64, g64 = R.loss_and_grad(*model, *data, gamma, tf, dtype=np.float64)
    gu.assert_parity(f"expert loss {name} tf={tf}", loss.reshape(()), l32, l64)
    gu.assert_parity(f"expert grad {name} tf={tf}", grad, g32, g64)
    eng.close()


def test_deterministic_and_loss_only():
    eng, model, data = _setup("lstm-cheetah", seed=4)
    l1, g1 = _gpu(eng, model, data, 0.9, False)
    l2, g2 = _gpu(eng, model, data, 0.9, False)
    assert l1.tobytes() == l2.tobytes() and g1.tobytes() == g2.tobytes()
    l3, g3 = _gpu(eng, model, data, 0.9, False, want_grad=False)
    assert g3 is None and l3.tobytes() == l1.tobytes()
    eng.close()


def test_out_of_cap_shapes_fail():
    n, m = 5, 2
    eng = runner.make_engine(n, m, 4)
    d = eng.to_dev
    xseq, useq, yseq = (d(a) for a in R.make_windows(np.random.default_rng(0), 4, 3, n, m))
    bad = [make_expert_shape(129, [129, 16, n], [129, 16, m]),       # F > 128
           make_expert_shape(0, [513, 16, n], [513, 16, m]),         # MLP first width > 512
           make_expert_shape(16, [16, 1025, n], [16, 1025, m])]      # head width > 1024
    for es in bad:
        count = eng.lib.gmpc_expert_param_count(n, es)
        with pytest.raises(_lib.GmpcError):
            eng.expert_loss_grad(xseq, useq, yseq, torch.zeros(count, device=eng.device), es, 0.9, False)
    es = make_expert_shape(16, [16, 16, n], [16, 16, m])
    flat = torch.zeros(eng.lib.gmpc_expert_param_count(n, es), device=eng.device)
    with pytest.raises(_lib.GmpcError):                               # S = 0
        eng.expert_loss_grad(xseq[:, :0], useq[:, :0], yseq[:, :0], flat, es, 0.9, False)
    with pytest.raises(_lib.GmpcError):                               # B > max_batch
        eng.expert_loss_grad(torch.cat([xseq, xseq]), torch.cat([useq, useq]), torch.cat([yseq, yseq]), flat,
                             es, 0.9, False)
    eng.close()


def _teacher_windows(rng, n, m, count, S, F=8):
    """Windows of trajectories rolled by a random teacher model (next_x = its prediction, u = its action)."""
    teacher = orc.make_expert(rng, n, m, lstm_features=F, num_layers=2, num_hidden_units=16)
    for W, b in teacher["head_x"][-1:]:
        W *= 0.3
    x0 = rng.standard_normal((count, 1, n)).astype(np.float32)
    goal, U = orc.expert_goal_states_init_actions(teacher, np.concatenate([x0, x0], 1), S)
    return (np.ascontiguousarray(goal[:, :S]), np.ascontiguousarray(U), np.ascontiguousarray(goal[:, 1:]))


def _adam_fp64(p, g, m, v, step, lr, max_norm=100.0, b1=0.9, b2=0.999, eps=1e-8):
    norm = np.sqrt((g * g).sum())
    g = g * min(1.0, max_norm / norm) if norm > 0 else g
    m[:] = b1 * m + (1 - b1) * g
    v[:] = b2 * v + (1 - b2) * g * g
    mh, vh = m / (1 - b1 ** step), v / (1 - b2 ** step)
    p -= lr * mh / (np.sqrt(vh) + eps)


def test_trainer_matches_fp64_loop_and_learns():
    rng = np.random.default_rng(11)
    n, m, S = 3, 1, 4
    train = _teacher_windows(rng, n, m, 48, S)
    test = _teacher_windows(rng, n, m, 16, S)
    ex = orc.make_expert(rng, n, m, lstm_features=8, num_layers=2, num_hidden_units=16)
    flat0, F, dx, du = P.pack_expert(ex)
    tree = P.expert_dict_to_tree(ex)
    lr, epochs, batch, gamma, factor = 1e-2, 6, 8, 0.9, 0.5
    eng = runner.make_engine(n, m, 64)
    st = runner.get_trainstate(None, tree, runner.optim.ClipAdam(lr), eng)
    before = float(trainer.calculate_loss(st, st.params, test, gamma, False))
    st, train_loss, test_loss = trainer.train(st, (train, test), epochs, batch, 5, gamma, factor, print_step=2)
    got = st.params.cpu().numpy()
    # the same minibatches, teacher-forcing schedule and clip+Adam in fp64 (and fp32) on the restatement
    refs = {}
    for dt in (np.float64, np.float32):
        p, mm, vv = flat0.astype(np.float64), np.zeros(flat0.size), np.zeros(flat0.size)
        sched = np.random.default_rng(5)
        step = 0
        for ep in range(1, epochs + 1):
            perm = sched.choice(train[0].shape[0], size=(train[0].shape[0] // batch, batch))
            tf = ep <= epochs * factor
            for idx in perm:
                _, g = R.loss_and_grad(p.astype(dt), F, dx, du, *(a[idx] for a in train), gamma, tf, dtype=dt)
                step += 1
                _adam_fp64(p, g.astype(np.float64) / batch, mm, vv, step, lr)
        refs[dt] = p
    gu.assert_parity("expert trainer params after 6 epochs", got, refs[np.float32], refs[np.float64])
    N = test[0].shape[0]
    l64 = R.loss_only(refs[np.float64], F, dx, du, *test, gamma, False) / N
    l32 = R.loss_only(refs[np.float32], F, dx, du, *test, gamma, False, dtype=np.float32) / N
    gu.assert_parity("expert trainer test loss", np.float32(test_loss), l32, l64)
    assert np.isfinite(train_loss) and test_loss < 0.9 * before, (before, test_loss)
    eng.close()


def _runner_config(tmp_path, use):
    cfg = {
        "seed": 3,
        "env": {"type": "dmcontrol", "expert": {"name": "synthetic_linear"},
                "imitator": {"name": "synthetic_linear", "physics": []}},
        "expert_prediction": {
            "model": {"use": use, "mlp": {"num_layers": 3, "num_hidden_units": 32},
                      "lstm": {"lstm_features": 16, "num_layers": 2, "num_hidden_units": 32}},
            "train": {"num_epochs": 2, "batch_size": 8, "seqlen": 5, "learning_rate": 1e-3,
                      "discount_factor": 0.9, "teacher_forcing_factor": 0.5, "print_step": 1}},
        "mpc": {"normalizer": {"state": "standard_norm", "action": "identity"},
                "train": {"num_trajectories": 3, "trajectory_len": 30}},
    }
    path = tmp_path / f"expert_{use}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def _tree_listing(top):
    out = []
    for dirpath, _, files in os.walk(top):
        if "__pycache__" in dirpath or ".pytest_cache" in dirpath:
            continue
        out += [os.path.join(dirpath, f) for f in files]
    return sorted(out)


@pytest.mark.parametrize("use", ["lstm", "mlp"])
def test_runner_writes_loadable_params(tmp_path, use):
    from test_gpu_runner import LinearEnv, _write_dataset
    data = _write_dataset(tmp_path, ntraj=3, L=30)
    before = _tree_listing(os.path.join(ROOT, "gan_mpc_amd"))
    out_dir = runner.run(_runner_config(tmp_path, use), dataset_path=data, env=LinearEnv(seed=1),
                         save_dir=str(tmp_path / "expert"))
    assert out_dir.startswith(str(tmp_path)) and os.path.exists(os.path.join(out_dir, "params.npz"))
    assert _tree_listing(os.path.join(ROOT, "gan_mpc_amd")) == before
    saved = utils.load_json(os.path.join(out_dir, "config.json"))
    assert saved["model"]["use"] == use and np.isfinite(saved["loss"]["test_loss"])
    flat, F, dx, du = P.pack_expert(utils.load_params(os.path.join(out_dir, "params.npz")))
    assert F == (16 if use == "lstm" else 0) and dx[-1] == 4 and du[-1] == 2


def test_saved_params_roll_out_bitwise(tmp_path):
    rng = np.random.default_rng(2)
    n, m, S = 4, 2, 5
    ex = orc.make_expert(rng, n, m, lstm_features=16, num_layers=2, num_hidden_units=32)
    eng = runner.make_engine(n, m, 16)
    st = runner.get_trainstate(None, P.expert_dict_to_tree(ex), runner.optim.ClipAdam(1e-3), eng)
    data = _teacher_windows(rng, n, m, 16, S)
    st, _ = trainer.train_epoch(st, np.arange(16).reshape(2, 8), data, 0.9, True)
    out_dir = utils.save_all_args(str(tmp_path / "expert"), st.to_tree(), {"model": {}})
    loaded = utils.load_params(os.path.join(out_dir, "params.npz"))
    spec = expert_model.ExpertModel.get_model(utils.load_config.Config.from_dict(
        {"use": "lstm", "lstm": {"lstm_features": 16, "num_layers": 2, "num_hidden_units": 32}}), n, m)
    model = expert_model.ExpertModel(None, spec)
    hist = eng.to_dev(rng.standard_normal((5, 3, n)).astype(np.float32))
    g_mem, u_mem = eng.expert_rollout(hist, st.params, st.shape)
    g_ld, u_ld = model.get_goal_states_init_actions(hist.cpu().numpy(), loaded, engine=eng)
    torch.cuda.synchronize()
    assert g_mem.cpu().numpy().tobytes() == g_ld.cpu().numpy().tobytes()
    assert u_mem.cpu().numpy().tobytes() == u_ld.cpu().numpy().tobytes()
    eng.close()


def test_policy_fn_is_the_teacher_forced_last_action():
    rng = np.random.default_rng(6)
    n, m = 6, 2
    for F in (16, 0):
        ex = orc.make_expert(rng, n, m, lstm_features=F, num_layers=3, num_hidden_units=24)
        flat, F_, dx, du = P.pack_expert(ex)
        eng = runner.make_engine(n, m, 4)
        st = runner.get_trainstate(None, P.expert_dict_to_tree(ex), runner.optim.ClipAdam(1e-3), eng)
        fn = runner.get_policy_fn(st)
        for H in (2, 7):
            hist = rng.standard_normal((H, n)).astype(np.float32)
            u = fn(st.params, hist, None).cpu().numpy()
            refs = []
            for dt, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
                exd = R.unflatten(torch.as_tensor(flat.astype(dt), dtype=tdt), F_, dx, du)
                _, us = R.forward(exd, torch.as_tensor(hist[None].astype(dt)), True)
                refs.append(us[0, -1].numpy())
            gu.assert_parity(f"expert policy_fn F={F} H={H}", u, refs[0], refs[1])
        eng.close()
