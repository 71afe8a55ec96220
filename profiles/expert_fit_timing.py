"""Timing of gmpc_expert_loss_grad at the reference's default expert shape (expert_prediction in
config/l2_hyperparameters.yaml: LSTM F=128, 3 x 128 heads, batch 64, seqlen 10) for x_size / m given on the
command line (default: the cheetah sizes 17 / 6).  30 warm-up calls, then 100 timed calls on one stream;
prints the wall time per call.  Run it under rocprofv3 for the per-kernel figures quoted in DESIGN.md §9:

    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o expert -- python profiles/expert_fit_timing.py 17 6
"""

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gan_mpc_oracle as orc  # noqa: E402
from gan_mpc_amd import params as P  # noqa: E402
from gan_mpc_amd.engine import make_expert_shape  # noqa: E402
from gan_mpc_amd.expert import runner  # noqa: E402


def main(n=17, m=6, B=64, S=10):
    rng = np.random.default_rng(0)
    ex = orc.make_expert(rng, n, m, lstm_features=128, num_layers=3, num_hidden_units=128)
    flat, F, dx, du = P.pack_expert(ex)
    eng = runner.make_engine(n, m, B)
    d = eng.to_dev
    traj = rng.standard_normal((B, S + 1, n)).astype(np.float32)
    x, y = d(np.ascontiguousarray(traj[:, :S])), d(np.ascontiguousarray(traj[:, 1:]))
    u = d(np.tanh(rng.standard_normal((B, S, m))).astype(np.float32))
    fl, es = d(flat), make_expert_shape(F, dx, du)
    loss, grad = eng.new(1), eng.new(flat.size)
    for i in range(30):
        eng.expert_loss_grad(x, u, y, fl, es, 0.9, i % 2 == 0, loss_sum=loss, grad_sum=grad)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(100):
        eng.expert_loss_grad(x, u, y, fl, es, 0.9, False, loss_sum=loss, grad_sum=grad)
    torch.cuda.synchronize()
    print(f"x_size={n} m={m} B={B} S={S}: {1e6 * (time.perf_counter() - t0) / 100:.1f} us per call "
          "(wall, 100 calls)")
    eng.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
