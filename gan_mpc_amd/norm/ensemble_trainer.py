"""Training of a dynamics ensemble: the P members of the ensemble the sampling solvers cost
their rows on (Engine.set_sampled_ensemble, section 24), fitted together.

dynamics_trainer.train_params, with the members in place of the one model: the dataset goes to the device once, every
step is ONE call of the member-parallel regression (Engine.dynamics_ensemble_loss_grad) on index rows into it, then the
fused clip+Adam on each member's slice with the member's own moments and norm.  With bootstrap=True every member draws
its own minibatches (with replacement, like the reference's `jax.random.choice`): the members see different data and
differ for that reason as well as for their initial weights.  Relu-MLP dynamics only; one rank only.

Validation: holdout_errors rolls held-out sequences out under every member in one call per chunk
(Engine.ensemble_rollout) and returns each member's open-loop error per step; elite_members picks the best k.

`key` is a NumPy seed / Generator.  `train_args` = (policy, opt): the policy lends its engine (policy.engine_for; it
must have been bound once, its engine takes the shapes from the bound parameters), opt is an optim.ClipAdam."""

import numpy as np
import torch

from gan_mpc_amd import parallel, params as params_lib, trainer_common as tc

MAX_MEMBERS = 16      # Engine.MAX_ENSEMBLE


def _check_count(P):
    if not isinstance(P, (int, np.integer)) or not 1 <= P <= MAX_MEMBERS:
        raise ValueError(f"ensemble trainer: P = {P!r} outside [1, {MAX_MEMBERS}]")


def _single_rank():
    world = parallel.world()[1]
    if world > 1:
        raise NotImplementedError(f"ensemble trainer: one rank only, the world has {world}")


def init_members(policy, dynamics_args, P, seed):
    """(P, dyn_count) float32 device tensor: member p is dynamics_model.init under seed + p (dynamics_args as
    policy.init takes them, its seed replaced)."""
    _check_count(P)
    rows = []
    for p in range(int(P)):
        tree = policy.dynamics_model.init(int(seed) + p, *tuple(dynamics_args)[1:])
        if params_lib.dynamics_is_lstm(tree):
            raise ValueError("ensemble trainer: relu-MLP dynamics only")
        rows.append(params_lib.pack_mlp(tree))
    return torch.as_tensor(np.stack(rows).astype(np.float32)).to(policy.device())


def init_opt_state(opt, members):
    """One optimiser state per member (its own moments and step count)."""
    return [opt.init(members[p]) for p in range(members.shape[0])]


def members_to_trees(members, like):
    """The members as parameter trees shaped like `like` (params["dynamics_params"]): what
    EvalMPC(dynamics_ensemble=...) and set_dynamics_ensemble take."""
    flat = members.detach().cpu().numpy() if torch.is_tensor(members) else np.asarray(members, np.float32)
    dims = params_lib.mlp_dims(like)
    count = sum(a * b + b for a, b in zip(dims[:-1], dims[1:]))
    if flat.ndim != 2 or flat.shape[1] != count:
        raise ValueError(f"ensemble trainer: members must be (P, {count}) for a network of widths {dims}, got "
                         f"{flat.shape}")
    return [params_lib.unpack_mlp(row, dims) for row in flat]


def draw_indices(rng, datasize, steps, P, batch_size, bootstrap=True):
    """The index tensor of one update, (steps, P, batch_size) int32 in [0, datasize): one draw with replacement.
    bootstrap=False: one (steps, batch_size) draw that every member shares."""
    if bootstrap:
        return rng.choice(datasize, size=(steps, P, batch_size)).astype(np.int32)
    one = rng.choice(datasize, size=(steps, batch_size)).astype(np.int32)
    return np.ascontiguousarray(np.broadcast_to(one[:, None, :], (steps, P, batch_size)))


def _check_args(members, dataset, batch_size):
    shape = tuple(getattr(members, "shape", ()))
    if len(shape) != 2:
        raise ValueError(f"ensemble trainer: members must be (P, dyn_count), got shape {shape}")
    _check_count(int(shape[0]))
    if len(dataset) != 3:
        raise ValueError("ensemble trainer: dataset must be (xseq, useq, next_xseq)")
    X, U, Y = (np.asarray(d, np.float32) for d in dataset)
    if X.ndim != 3 or U.ndim != 3 or Y.shape != X.shape or U.shape[:2] != X.shape[:2]:
        raise ValueError(f"ensemble trainer: dataset must be (D, S, n), (D, S, m), (D, S, n), got {X.shape}, {U.shape}, "
                         f"{Y.shape}")
    if not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f"ensemble trainer: batch_size = {batch_size!r} must be a positive integer")
    return X, U, Y


def train_params(train_args, opt_state, members, dataset, num_updates, batch_size, discount_factor,
                 teacher_forcing_factor, key, id, bootstrap=True):
    """dynamics_trainer.train_params for the members (P, dyn_count), a float32 device tensor updated in place.
    opt_state: init_opt_state's list, or None for a fresh one.  -> (members, opt_state, losses (num_updates, P): each
    member's mean loss over the update's steps)."""
    _single_rank()
    policy, opt = train_args
    X, U, Y = _check_args(members, dataset, batch_size)
    if not torch.is_tensor(members):
        raise ValueError("ensemble trainer: members must be a device tensor (init_members)")
    P = int(members.shape[0])
    datasize = X.shape[0]
    steps = datasize // int(batch_size)
    losses = np.zeros((0, P), np.float32)
    if opt_state is None:
        opt_state = init_opt_state(opt, members)
    if len(opt_state) != P:
        raise ValueError(f"ensemble trainer: opt_state holds {len(opt_state)} states for P = {P} members")
    if steps == 0:
        return members, opt_state, losses
    if getattr(policy, "_bound", None) is None:
        raise ValueError("ensemble trainer: bind the policy once first (policy.bind(policy.to_device_params(params))): "
                         "its engine takes the shapes from the bound parameters")
    rng = tc.as_rng(key)
    eng = policy.engine_for(int(batch_size))
    Xd, Ud, Yd = eng.to_dev(X), eng.to_dev(U), eng.to_dev(Y)      # once: the steps address it by index
    loss_sum = eng.new(P)
    grad = eng.new(P, members.shape[1])
    inv = 1.0 / float(batch_size)
    out = []
    for up in range(1, num_updates + 1):
        idx = draw_indices(rng, datasize, steps, P, int(batch_size), bootstrap)
        teacher_forcing = (id + up) <= (num_updates * teacher_forcing_factor)
        total = torch.zeros(P, dtype=torch.float32, device=loss_sum.device)
        for step in range(steps):
            eng.dynamics_ensemble_loss_grad(members, Xd, Ud, Yd, discount_factor, teacher_forcing, rows=idx[step],
                                            loss_sum=loss_sum, grad_sum=grad)
            total += loss_sum
            for p in range(P):
                opt_state[p]["count"] += 1
                eng.adam_clip_step(members[p], grad[p], opt_state[p]["m"], opt_state[p]["v"], opt_state[p]["count"],
                                   opt.lr, inv, opt.max_norm, opt.b1, opt.b2, opt.eps)
        out.append((total * (inv / steps)).cpu().numpy())
    return members, opt_state, np.stack(out).astype(np.float32) if out else losses


def holdout_errors(engine, members, xseq, useq, next_xseq):
    """The members' multi-step open-loop error on recorded sequences: every sequence is rolled
    out from xseq[:, 0] under useq by every member (Engine.ensemble_rollout, in chunks of engine.max_batch sequences)
    and compared with next_xseq.  members (P, dyn_count); xseq, next_xseq (D, S, n), useq (D, S, m), S <= T, tensors
    on the engine's device.  -> (P, S) float32: the mean over sequences and state entries of the squared error of
    member p's prediction of step s + 1.  No gradient, nothing of the engine's state is touched."""
    shapes = tuple(tuple(getattr(t, "shape", ())) for t in (xseq, useq, next_xseq))
    if any(len(s) != 3 for s in shapes) or shapes[2] != shapes[0] or shapes[1][:2] != shapes[0][:2] or shapes[0][0] < 1:
        raise ValueError("ensemble trainer: holdout data must be (D, S, n), (D, S, m), (D, S, n) with D >= 1, got "
                         f"{shapes[0]}, {shapes[1]}, {shapes[2]}")
    D, S, n = shapes[0]
    total = None
    for b0 in range(0, D, int(engine.max_batch)):
        b1 = min(D, b0 + int(engine.max_batch))
        X = engine.ensemble_rollout(members, xseq[b0:b1, 0].contiguous(), useq[b0:b1].contiguous(), want=("X",))["X"]
        err = X[:, :, 1:] - next_xseq[b0:b1].unsqueeze(0)
        part = (err * err).to(torch.float64).sum(dim=(1, 3))           # (P, S): the chunk's sum
        total = part if total is None else total + part
    return (total / float(D * n)).to(torch.float32)


def elite_members(errors, k):
    """The indices of the k members with the smallest holdout error summed over the steps, best first; ties go to the
    lower index, a member with a non-finite error comes last.  errors: holdout_errors' (P, S).  -> int64 tensor (k,)
    that indexes the members (members[elite_members(errors, k)] is what set_dynamics_ensemble takes)."""
    e = errors.detach().cpu().numpy() if torch.is_tensor(errors) else np.asarray(errors)
    if e.ndim != 2 or e.shape[0] < 1:
        raise ValueError(f"ensemble trainer: errors must be (P, S), got shape {e.shape}")
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= e.shape[0]:
        raise ValueError(f"ensemble trainer: k = {k!r} outside [1, P = {e.shape[0]}]")
    total = e.astype(np.float64).sum(axis=1)
    total = np.where(np.isfinite(total), total, np.inf)
    return torch.as_tensor(np.argsort(total, kind="stable")[:int(k)].astype(np.int64))
