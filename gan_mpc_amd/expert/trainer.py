"""Expert-model training (reference expert/trainer.py:10-107, same names and return values): behaviour
cloning of the sequence model on expert windows, with teacher forcing for the first
`teacher_forcing_factor` of the epochs.

The loss and its gradient are one fused GPU call (gmpc_expert_loss_grad); minibatch sampling, the
teacher-forcing schedule and clip+Adam bookkeeping are host code.  `trainstate` is the TrainState of
gan_mpc_amd/expert/runner.py (flat device parameters, their shape, the optimiser and its state).  `key` is
a NumPy seed / Generator.  Under torch.distributed every rank takes its shard of each minibatch and the
sums are averaged over the global batch (parallel.allreduce_mean_from_sums)."""

import numpy as np
import torch

from gan_mpc_amd import parallel, trainer_common as tc


def _sums(trainstate, params, X, U, Y, discount_factor, teacher_forcing, packed, want_grad):
    """Write the loss sum (and gradient sum) of the windows X, U, Y into packed[0] (and packed[1:1+count]),
    in chunks of the engine's max_batch."""
    eng = trainstate.engine
    count = params.numel()
    d = eng.to_dev
    for lo in range(0, X.shape[0], eng.max_batch):
        hi = min(X.shape[0], lo + eng.max_batch)
        first = lo == 0
        loss = packed[:1] if first else eng.new(1)
        grad = (packed[1:1 + count] if first else eng.new(count)) if want_grad else None
        eng.expert_loss_grad(d(X[lo:hi]), d(U[lo:hi]), d(Y[lo:hi]), params, trainstate.shape, discount_factor,
                             teacher_forcing, want_grad=want_grad, loss_sum=loss, grad_sum=grad)
        if not first:
            packed[:1] += loss
            if want_grad:
                packed[1:1 + count] += grad


def _loss_and_grad(trainstate, params, X, U, Y, discount_factor, teacher_forcing, want_grad=True):
    """(mean loss, mean gradient or None over the global batch) for this rank's shard X, U, Y."""
    B = X.shape[0]
    count = params.numel() if want_grad else 0
    packed = parallel.new_packed(1 + count, params.device, B)
    if B > 0:                              # an empty shard still joins the exchange, with count 0
        _sums(trainstate, params, X, U, Y, discount_factor, teacher_forcing, packed, want_grad)
    means = parallel.allreduce_mean_from_sums(packed)
    return means[0], (means[1:] if want_grad else None)


def _shard(dataset):
    lo, hi = parallel.shard_range(dataset[0].shape[0])
    return tuple(np.asarray(d[lo:hi], np.float32) for d in dataset)


def calculate_loss(trainstate, params, dataset, discount_factor, teacher_forcing):
    """reference :10-31: mean over the windows of sum_dims sum_t g^t ((u - a)^2 + (next_x - next_s)^2)
    -> 0-d device tensor."""
    X, U, Y = _shard(dataset)
    loss, _ = _loss_and_grad(trainstate, params, X, U, Y, discount_factor, teacher_forcing, want_grad=False)
    return loss


def train_epoch(trainstate, perm, dataset, discount_factor, teacher_forcing):
    """reference :34-58: one clip+Adam step per row of `perm` -> (trainstate, mean minibatch loss)."""
    s, a, next_s = dataset
    losses = []
    for batch in perm:
        lo, hi = parallel.shard_range(len(batch))
        idx = batch[lo:hi]
        loss, grads = _loss_and_grad(trainstate, trainstate.params, s[idx], a[idx], next_s[idx], discount_factor,
                                     teacher_forcing)
        trainstate = trainstate.apply_gradients(grads=grads)
        losses.append(loss.reshape(1))
    if not losses:               # datasize < batch_size: the reference's mean over an empty scan is NaN
        return trainstate, float("nan")
    return trainstate, float(torch.cat(losses).mean())


def train(trainstate, dataset, num_epochs, batch_size, key, discount_factor, teacher_forcing_factor,
          print_step=10):
    """reference :61-107 -> (trainstate, last epoch's train loss, test loss with teacher forcing off)."""
    rng = tc.as_rng(key)
    train_data, test_data = (tuple(np.asarray(d, np.float32) for d in split) for split in dataset)
    datasize = train_data[0].shape[0]
    epoch_loss = []
    for ep in range(1, num_epochs + 1):
        perm = tc.minibatch_schedule(rng, datasize, batch_size)
        teacher_forcing = ep <= (num_epochs * teacher_forcing_factor)
        trainstate, train_loss = train_epoch(trainstate, perm, train_data, discount_factor, teacher_forcing)
        if (ep % print_step) == 0:
            test_loss = float(calculate_loss(trainstate, trainstate.params, test_data, discount_factor,
                                             teacher_forcing=False))
            print(f"epoch: {ep} training_loss: {train_loss:.4f} test_loss: {test_loss:.4f}")
        epoch_loss.append(train_loss)

    test_loss = float(calculate_loss(trainstate, trainstate.params, test_data, discount_factor,
                                     teacher_forcing=False))
    return trainstate, epoch_loss[-1], test_loss
