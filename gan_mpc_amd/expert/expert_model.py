"""Where goal_xseq / init_useq come from (reference policy/eval.py:87-107, policy/base.py:41-61).

ExpertModel is the reference's behaviour-cloning sequence model (expert/expert_model.py:10-91,
expert/nn.py:10-163) run on the GPU by gmpc_expert_rollout: the history rows are fed teacher-forced,
then the model rolls `horizon` steps on its own predictions.  No pretrained parameters ship with
either repository, so utils.get_expert_model falls back to HoldExpert unless a saved model is found;
TableExpert serves synthetic workloads and tests."""

import numpy as np

from gan_mpc_amd import nn_init, params as P


class ExpertProtocol:
    needs_engine = False

    def init(self, *args):
        return None

    def get_goal_states_init_actions(self, history_X, expert_params):
        """history_X (B, hist+1, n) -> goal (B, T+1, n) with goal[:, 0] = history_X[:, -1],
        init_U (B, T, m)   (reference policy/base.py:41-61)."""
        raise NotImplementedError


class HoldExpert(ExpertProtocol):
    """Goal = hold the current state, zero initial controls."""

    def __init__(self, horizon, u_size):
        self.T, self.m = int(horizon), int(u_size)

    def get_goal_states_init_actions(self, history_X, expert_params):
        x = np.asarray(history_X, np.float32)[:, -1]
        goal = np.repeat(x[:, None, :], self.T + 1, axis=1)
        return goal, np.zeros((x.shape[0], self.T, self.m), np.float32)


class TableExpert(ExpertProtocol):
    """Goal / initial controls looked up from arrays (synthetic workloads and tests): row i of the
    tables belongs to the sample whose history is history_X[i]."""

    def __init__(self, goal, init_U):
        self.goal = np.asarray(goal, np.float32)
        self.init_U = np.asarray(init_U, np.float32)
        self._cursor = None

    def select(self, idx):
        self._cursor = np.asarray(idx)
        return self

    def get_goal_states_init_actions(self, history_X, expert_params):
        idx = self._cursor if self._cursor is not None else np.arange(len(history_X))
        self._cursor = None
        return self.goal[idx], self.init_U[idx]


class _ModelSpec:
    """What expert_nn.StateAction(ScanLSTM | ScanMLP) carries: the architecture."""

    def __init__(self, use, lstm_features, num_layers, num_hidden_units, x_out, u_out):
        self.use, self.lstm_features = use, int(lstm_features)
        self.num_layers, self.num_hidden_units = int(num_layers), int(num_hidden_units)
        self.x_out, self.u_out = int(x_out), int(u_out)


class ExpertModel(ExpertProtocol):
    needs_engine = True

    def __init__(self, config, model):
        self.config = config
        self.model = model
        self._packed = None        # (id(params), device flat vector, shape struct)

    @staticmethod
    def get_model(model_config, x_size, u_size):
        """reference expert_model.py:15-37"""
        if model_config.use == "lstm":
            c = model_config.lstm
            return _ModelSpec("lstm", c.lstm_features, c.num_layers, c.num_hidden_units, x_size, u_size)
        if model_config.use == "mlp":
            c = model_config.mlp
            return _ModelSpec("mlp", 0, c.num_layers, c.num_hidden_units, x_size, u_size)
        raise ValueError("Choose either mlp or lstm model.")

    def init(self, load_params, *args):
        """reference expert_model.py:39-48.  load_params=True reads the saved parameters of
        trained_models/expert/<env type>/<env name>/<load_id>/ (params.npz; the reference's pickled
        params.npy only with mpc.model.expert.allow_pickle: true); otherwise args = (seed, batch, seqlen, x_size) and a
        fresh flax-style tree is drawn."""
        from gan_mpc_amd import utils
        if load_params:
            config = self.config
            base = (f"trained_models/expert/{config.env.type}/{config.env.expert.name}/"
                    f"{config.mpc.model.expert.load_id}/")
            try:
                return utils.load_params(base + "params.npz")
            except FileNotFoundError:
                # the reference's own artefact is a pickled params.npy: unpickling runs code, so it is
                # read only on an explicit opt-in (config.mpc.model.expert.allow_pickle: true)
                if not getattr(config.mpc.model.expert, "allow_pickle", False):
                    raise FileNotFoundError(
                        f"{base}params.npz not found.  A reference-format params.npy is a pickle and is "
                        "only read with mpc.model.expert.allow_pickle: true in the config; convert it "
                        "once: np.savez('params.npz', **utils.flatten_tree(utils.load_params(path, allow_pickle=True))).")
                return utils.load_params(base + "params.npy", allow_pickle=True)
        seed = args[0]
        rng = np.random.default_rng(seed)
        mdl = self.model
        if mdl.use == "lstm":
            F, L, ywidth = mdl.lstm_features, mdl.num_layers, mdl.lstm_features
            ex = {"lstm": dict(Wx=nn_init.lecun_normal(rng, mdl.x_out, 4 * F),
                               Wh=nn_init.lecun_normal(rng, F, 4 * F), b=np.zeros(4 * F, np.float32))}
        else:
            L, ywidth = mdl.num_layers - 1, mdl.num_hidden_units
            ex = {"first": (nn_init.lecun_normal(rng, mdl.x_out, ywidth), np.zeros(ywidth, np.float32))}
        for key, out in (("head_x", mdl.x_out), ("head_u", mdl.u_out)):
            sizes = [ywidth] + [mdl.num_hidden_units] * (L - 1) + [out]
            ex[key] = [(nn_init.lecun_normal(rng, a, b), np.zeros(b, np.float32))
                       for a, b in zip(sizes[:-1], sizes[1:])]
        return P.expert_dict_to_tree(ex)

    def _device_params(self, expert_params, engine):
        from gan_mpc_amd.engine import make_expert_shape
        if self._packed is None or self._packed[0] is not expert_params:
            flat, F, dx, du = P.pack_expert(expert_params)
            self._packed = (expert_params, engine.to_dev(flat), make_expert_shape(F, dx, du))
        return self._packed[1], self._packed[2]

    def device_params(self, expert_params, engine):
        """(flat, shape): the cached fp32 device vector in params.pack_expert's layout -- the leaf
        policy.differentiable.expert_layer differentiates -- and its gmpc_expert_shape."""
        return self._device_params(expert_params, engine)

    def get_goal_states_init_actions(self, history_X, expert_params, engine=None):
        """Batched policy/eval.py:87-107 on the GPU -> device tensors goal (B, T+1, n), init_U (B, T, m)."""
        if engine is None:
            raise ValueError("ExpertModel runs on the GPU: the policy passes its engine")
        flat, shape = self._device_params(expert_params, engine)
        return engine.expert_rollout(engine.to_dev(np.asarray(history_X, np.float32)), flat, shape)

    # single-sample API of the reference (expert_model.py:78-91), for parity of the protocol
    def get_carry_next_state_and_action_seq(self, history_x, expert_params, engine):
        goal, U = self.get_goal_states_init_actions(np.asarray(history_x, np.float32)[None],
                                                    expert_params, engine)
        return goal[0], U[0]
