"""Cost of gmpc_critic_dir_vjp (the second-order VJP of the critic's scores, both gradient outputs) against two
yardsticks, neither of them the code under test:

  (a) gmpc_critic_vjp with both outputs on the same sequences: the new call does roughly a forward and a backward of
      twice the width, in a run-time-shape form without register-held weights.  The ratio is recorded, with no bar.
  (b) what a user would otherwise run: torch's fp32 double backward of tests/critic_vjp_ref.forward_t on the same device
      tensors (score -> dscore/dx with create_graph -> <., v> -> gradients w.r.t. parameters and sequences).  The new
      call's median must be below (b)'s p10 at C3.

Engine level: alternating one call each after warm-up, device time per call from a synchronised host clock over `--calls`
calls, in one process.  Shapes: the C3 critic (n 17, F 64, head 3 x 256, T 50, Bc 2048) and the reference regime (same
model, T 5, Bc 256).  Kernel-only times come from a separate `rocprofv3 --kernel-trace --stats` run of this script per
shape (--shape, --no-torch), committed as profiles/critic_dir_vjp_kernel_stats_<shape>.csv.

    python profiles/critic_dir_vjp_timing.py [--calls 30] [--out FILE] [--shape C3|T5-Bc256] [--no-torch]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from cotangent_timing import _mlp, _timed  # noqa: E402
from gan_mpc_amd.engine import Engine  # noqa: E402

# name: (n, F, head hidden widths, T, Bc)
SHAPES = {"C3": (17, 64, (256, 256, 256), 50, 2048), "T5-Bc256": (17, 64, (256, 256, 256), 5, 256)}


def _torch_double_backward(crit, n, F, head, xseq, v, g):
    import critic_vjp_ref as V

    def run():
        fl = crit.detach().requires_grad_(True)
        xs = xseq.detach().requires_grad_(True)
        with torch.device(crit.device):          # forward_t's zero carry follows the default device
            score = V.forward_t(fl, n, F, tuple(head), xs)
        gx, = torch.autograd.grad(score.sum(), xs, create_graph=True)
        sdot = (gx * v).sum((1, 2))
        return torch.autograd.grad((sdot * g).sum(), (fl, xs))
    return run


def engine_level(name, calls, with_torch=True):
    n, F, hidden, T, Bc = SHAPES[name]
    rng = np.random.default_rng(0)
    head = [F, *hidden, 1]
    eng = Engine(n, 6, T, [n + 6, 8, n], [n, 1], max_batch=Bc // 2, lstm_features=F, head_dims=head)
    d = eng.to_dev
    lstm = [rng.standard_normal((n, 4 * F)) / np.sqrt(n), rng.standard_normal((F, 4 * F)) / np.sqrt(F),
            0.1 * rng.standard_normal(4 * F)]
    crit = d(np.concatenate([a.reshape(-1) for a in lstm] + [_mlp(rng, head)]).astype(np.float32))
    xseq = d(rng.standard_normal((Bc, T + 1, n)).astype(np.float32))
    v = d(rng.standard_normal((Bc, T + 1, n)).astype(np.float32))
    g = d(rng.standard_normal(Bc).astype(np.float32))
    calls_ = {"critic_dir_vjp": lambda: eng.critic_dir_vjp(xseq, crit, v, g),
              "critic_dir_vjp_params_only": lambda: eng.critic_dir_vjp(xseq, crit, v, g, want_dx=False),
              "critic_dir_vjp_dx_only": lambda: eng.critic_dir_vjp(xseq, crit, v, g, want_params=False),
              "critic_dir_vjp_forward_only": lambda: eng.critic_dir_vjp(xseq, crit, v),
              "critic_vjp": lambda: eng.critic_vjp(xseq, crit, g)}
    if with_torch:
        calls_["torch_double_backward"] = _torch_double_backward(crit, n, F, head, xseq, v, g)
        # the yardstick computes the same thing
        ours, (tp, tx) = eng.critic_dir_vjp(xseq, crit, v, g), calls_["torch_double_backward"]()
        agree = {"params": float((ours["params"] - tp).abs().max() / tp.abs().max()),
                 "dx": float((ours["dx"] - tx).abs().max() / tx.abs().max())}
    for fn in calls_.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in calls_}
    for _ in range(calls):             # alternate, one call each, so that drift hits all alike
        for k, fn in calls_.items():
            res[k].append(_timed(fn, 1)["median_us"])
    out = {"level": "engine", "shape": name, "n": n, "F": F, "head": list(hidden), "T": T, "Bc": Bc, "calls": calls}
    for k, t in res.items():
        t = np.asarray(t)
        out[k] = {"median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)),
                  "p90_us": float(np.percentile(t, 90))}
    out["dir_over_critic_vjp"] = out["critic_dir_vjp"]["median_us"] / out["critic_vjp"]["median_us"]
    if with_torch:
        out["max_norm_difference_to_torch"] = agree
        out["dir_over_torch"] = out["critic_dir_vjp"]["median_us"] / out["torch_double_backward"]["median_us"]
        out["below_torch_p10"] = bool(out["critic_dir_vjp"]["median_us"] < out["torch_double_backward"]["p10_us"])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=list(SHAPES))
    ap.add_argument("--no-torch", action="store_true", help="leave the torch yardstick out (kernel-trace runs)")
    a = ap.parse_args()
    rows = [engine_level(s, a.calls, not a.no_torch) for s in ([a.shape] if a.shape else SHAPES)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
