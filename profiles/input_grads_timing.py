"""Cost of gmpc_bilevel_grad_inputs (dL/dx0 and dL/dgoal through the iLQR solution) against the bilevel call it follows.

Engine level, after one solve and one gmpc_bilevel_grad_cotangent: the cotangent call, the inputs call with both
outputs (the x0 sweep, k_tail_adjoints) and with the goal only (k_goal_grad), alternating, device time per call from a
synchronised host clock over `--calls` calls.  Shapes: C3 (n 17, m 6, T 50, B 1024) and the reference regime
(cheetah n 17, m 6, T 5, B 128); dynamics 3 x 200 relu, cost 128-128-10.  Kernel-only times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script per shape (--shape), committed as
profiles/input_grads_kernel_stats_<shape>.csv.

    python profiles/input_grads_timing.py [--calls 50] [--out FILE] [--shape C3|cheetah-T5-B128]
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

from cotangent_timing import SHAPES, _mlp, _timed  # noqa: E402
from gan_mpc_amd.engine import Engine  # noqa: E402


def engine_level(name, calls):
    n, m, T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    dyn_dims, cost_dims = [n + m, 200, 200, 200, n], [n, 128, 128, 10]
    eng = Engine(n, m, T, dyn_dims, cost_dims, max_batch=B)
    d = eng.to_dev
    params = (d(np.zeros(3, np.float32)), d(_mlp(rng, dyn_dims, 0.1)), d(_mlp(rng, cost_dims)))
    eng.set_params(*params)
    x0 = rng.standard_normal((B, n)).astype(np.float32)
    U = np.tanh(rng.standard_normal((B, T, m))).astype(np.float32)
    goal = rng.standard_normal((B, T + 1, n)).astype(np.float32)
    goal[:, 0] = x0
    eng.ilqr_solve(d(x0), d(U), d(goal), {"maxiter": 5})
    lx = d(rng.standard_normal((B, T + 1, n)).astype(np.float32))
    lu = d(rng.standard_normal((B, T, m)).astype(np.float32))
    g = eng.new(3 + eng.cost_count)
    eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0, grad_sum=g)
    calls_ = {"bilevel_grad_cotangent": lambda: eng.bilevel_grad_cotangent(B, lx, lu, sign=-1.0, grad_sum=g),
              "inputs_x0_and_goal": lambda: eng.bilevel_grad_inputs(B, lx),
              "inputs_goal_only": lambda: eng.bilevel_grad_inputs(B, lx, want_x0=False)}
    for fn in calls_.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in calls_}
    for _ in range(calls):             # alternate, one call each, so that drift hits all alike
        for k, fn in calls_.items():
            res[k].append(_timed(fn, 1)["median_us"])
    out = {"level": "engine", "shape": name, "n": n, "m": m, "T": T, "B": B, "calls": calls}
    for k, v in res.items():
        v = np.asarray(v)
        out[k] = {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
                  "p90_us": float(np.percentile(v, 90))}
    out["inputs_over_cotangent"] = out["inputs_x0_and_goal"]["median_us"] / out["bilevel_grad_cotangent"]["median_us"]
    # bytes the x0 sweep reads: [A_t | B_t], X, goal, dX, lx, QT (H only with the LSTM dynamics' curvature)
    out["x0_sweep_bytes"] = 4 * B * (T * n * (n + m) + (T + 1) * (4 * n) + n * n)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None, help="one shape only (a rocprofv3 run each)")
    args = ap.parse_args()
    lines = [engine_level(name, args.calls) for name in SHAPES if args.shape in (None, name)]
    for rec in lines:
        print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
