"""Entry points of expert-model training with the reference's names (reference expert/runner.py:12-137):
model, parameters, optimiser, normaliser, the expert windows of the trajectory file, training, an optional
evaluation in the environment, and the saved artefacts (params.npz + config.json) that
ExpertModel.init(load_params=True) and utils.get_expert_model read back.

Differences from the reference, as in norm/runner.py: state / action sizes come from the trajectory file,
`dataset_path` names that file, PRNG keys are NumPy generators, and the environment evaluation runs only
when an `env` object with the dm_control protocol is passed in."""

import numpy as np

from gan_mpc_amd import data_buffers, data_loader, optim, params as P, parallel, runner_common, utils
from gan_mpc_amd.engine import Engine, make_expert_shape
from gan_mpc_amd.expert import expert_model, trainer

get_normalizer = runner_common.get_normalizer
EVAL_CHUNK = 256        # windows per loss-only call (test split)


class TrainState:
    """What flax's TrainState carries, on the device: the flat expert vector in the layout of
    gmpc_expert_rollout, its shape, the optimiser and its state, and the engine the calls run on."""

    def __init__(self, engine, params, tx):
        flat, F, dx, du = P.pack_expert(params)
        self.engine, self.tx = engine, tx
        self.dims = (F, list(dx), list(du))
        self.shape = make_expert_shape(F, dx, du)
        self.params = engine.to_dev(flat)
        self.opt_state = tx.init(self.params)

    def apply_gradients(self, grads):
        self.params, self.opt_state = self.tx.update(self.engine, self.params, grads, self.opt_state)
        return self

    def to_dict(self):
        return P.unpack_expert(self.params.detach().cpu().numpy(), *self.dims)

    def to_tree(self):
        return P.expert_dict_to_tree(self.to_dict())


def make_engine(x_size, u_size, max_batch, device=None):
    """A context for the expert calls: they need x_size and u_size only, so the MPC part of the shape is
    a minimal one gmpc_create accepts (horizon 1: the policy's one-step expert rollout)."""
    return Engine(x_size, u_size, 1, [x_size + u_size, 8, x_size], [x_size, 1], max_batch, device=device)


def get_trainstate(model, params, tx, engine):
    del model
    return TrainState(engine, params, tx)


def get_model(config, state_size, action_size):
    expert_model_config = config.expert_prediction.model
    model = expert_model.ExpertModel.get_model(model_config=expert_model_config, x_size=state_size,
                                               u_size=action_size)
    return model, expert_model_config


def get_params(config, model, state_size):
    """reference :30-33: a fresh parameter tree drawn from config.seed."""
    return expert_model.ExpertModel(config, model).init(False, config.seed, 1, 1, state_size)


def get_optimizer(config):
    """reference :36-41: clip_by_global_norm(100) then adam(lr)."""
    return optim.ClipAdam(config.expert_prediction.train.learning_rate, max_norm=100.0)


def get_policy_fn(trainstate):
    """reference :94-100: the teacher-forced pass over the whole state history, last action.  That is
    gmpc_expert_rollout with the history minus its last row as teacher-forced rows and the last row as the
    current state, one step (the ctx's horizon is 1)."""
    eng = trainstate.engine

    def policy_fn(params, history_x, history_u):
        del history_u
        hx = eng.to_dev(np.asarray(history_x, np.float32)[None])
        _, init_U = eng.expert_rollout(hx, params, trainstate.shape)
        return init_U[0, 0]

    return policy_fn


def run(config_path, dataset_path=None, env=None, save_dir=None):
    """Train the expert model, optionally evaluate it in `env`, save it.  Returns the directory written
    (by rank 0; the other ranks get the same path)."""
    from gan_mpc_amd.norm import dynamics_trainer
    rank, world_size, _ = parallel.init_from_env()
    config = utils.get_config(config_path)
    key = np.random.default_rng(config.seed)

    env_type, env_name = config.env.type, config.env.expert.name
    loader = data_loader.DataLoader(config=config, normalizer=get_normalizer(config.mpc.normalizer))
    loader.init(path=dataset_path)
    state_size = loader.expert_trajectories["states"].shape[-1]
    action_size = loader.expert_trajectories["actions"].shape[-1]

    train_config = config.expert_prediction.train
    model, model_config = get_model(config, state_size, action_size)
    params = get_params(config, model, state_size)
    tx = get_optimizer(config)
    engine = make_engine(state_size, action_size, max(int(train_config.batch_size), EVAL_CHUNK))
    trainstate = get_trainstate(model, params, tx, engine)

    key, (subkey,) = runner_common.split_keys(key, 1)
    dataset = loader.get_expert_dataset(subkey)

    trainstate, train_loss, test_loss = trainer.train(
        trainstate=trainstate, dataset=dataset, num_epochs=train_config.num_epochs,
        batch_size=train_config.batch_size, key=key, discount_factor=train_config.discount_factor,
        teacher_forcing_factor=train_config.teacher_forcing_factor, print_step=train_config.print_step)

    avg_reward = 0.0
    if env is not None:
        buffer = data_buffers.Buffer(maxlen=train_config.seqlen, normalizer=loader.normalizer)
        avg_reward = dynamics_trainer.avg_run_policy(env=env, policy_fn=get_policy_fn(trainstate),
                                                     params=trainstate.params, buffer=buffer, num_runs=3,
                                                     max_interactions=1000)

    save_config = {
        "env": config.env.to_dict(),
        "loss": {"train_loss": round(float(train_loss), 5), "test_loss": round(float(test_loss), 5)},
        "model": model_config.to_dict(),
        "train": train_config.to_dict(),
        "avg_reward": round(float(avg_reward), 2),
    }
    where = save_dir or f"trained_models/expert/{env_type}/{env_name}/"
    out_dir = utils.save_all_args(where, trainstate.to_tree(), save_config) if rank == 0 else None
    if world_size > 1:           # the numbered directory is chosen by rank 0 alone; tell the others
        import torch.distributed as dist
        box = [out_dir]
        dist.broadcast_object_list(box, src=0)
        out_dir = box[0]
    return out_dir


if __name__ == "__main__":
    import sys
    run(config_path=sys.argv[1] if len(sys.argv) > 1 else "config/l2_hyperparameters.yaml",
        dataset_path=sys.argv[2] if len(sys.argv) > 2 else None)
