"""Cost of gmpc_rollout_vjp (the VJP of the rollout and its costs) against gmpc_rollout_cost and gmpc_lqr_backward on
the same (X, U).

Engine level: the VJP with and without grad_dyn_sum (gX and gcost both given, every other output wanted), the rollout
and the backward pass, alternating one call each after warm-up, device time per call from a synchronised host clock
over `--calls` calls.  Achieved FLOP/s use 2 x (the dynamics MLP's MACs) per (trajectory, step) for the sweep's
backward pass plus as much again for the forward pass that recomputes the relu masks.  Shapes: C3 (n 17, m 6, T 50,
B 1024), the reference regime (cheetah n 17, m 6, T 5, B 128) and a C4 shard (n 376, m 17, T 50, B 512); dynamics
3 x 200 relu, cost 128-128-10.  Kernel-only times come from a separate `rocprofv3 --kernel-trace --stats` run of this
script per shape (--shape), committed as profiles/rollout_vjp_kernel_stats_<shape>.csv.

    python profiles/rollout_vjp_timing.py [--calls 30] [--out FILE] [--shape C3|cheetah-T5-B128|C4-shard]
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

from cotangent_timing import _mlp, _timed  # noqa: E402
from gan_mpc_amd.engine import Engine  # noqa: E402

SHAPES = {"C3": (17, 6, 50, 1024), "cheetah-T5-B128": (17, 6, 5, 128), "C4-shard": (376, 17, 50, 512)}


def engine_level(name, calls):
    n, m, T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    dyn_dims, cost_dims = [n + m, 200, 200, 200, n], [n, 128, 128, 10]
    eng = Engine(n, m, T, dyn_dims, cost_dims, max_batch=B)
    d = eng.to_dev
    eng.set_params(d(np.zeros(3, np.float32)), d(_mlp(rng, dyn_dims, 0.1)), d(_mlp(rng, cost_dims)))
    x0 = d(rng.standard_normal((B, n)).astype(np.float32))
    U = d(np.tanh(rng.standard_normal((B, T, m))).astype(np.float32))
    goal = d(rng.standard_normal((B, T + 1, n)).astype(np.float32))
    X, costs = eng.rollout_cost(x0, U, goal)
    gX = d(rng.standard_normal((B, T + 1, n)).astype(np.float32))
    gc = d(rng.standard_normal((B, T + 1)).astype(np.float32))
    calls_ = {"rollout_vjp": lambda: eng.rollout_vjp(X, U, goal, gX, gc, want_dyn=False),
              "rollout_vjp_with_dyn": lambda: eng.rollout_vjp(X, U, goal, gX, gc),
              "rollout_cost": lambda: eng.rollout_cost(x0, U, goal, X=X, costs=costs),
              "lqr_backward": lambda: eng.lqr_backward(X, U, goal)}
    for fn in calls_.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in calls_}
    for _ in range(calls):             # alternate, one call each, so that drift hits all alike
        for k, fn in calls_.items():
            res[k].append(_timed(fn, 1)["median_us"])
    macs = sum(a * b for a, b in zip(dyn_dims[:-1], dyn_dims[1:]))
    flop = 2 * 2 * macs * B * T          # backward sweep + mask forward
    out = {"level": "engine", "shape": name, "n": n, "m": m, "T": T, "B": B, "calls": calls,
           "sweep_gflop": flop / 1e9}
    for k, v in res.items():
        v = np.asarray(v)
        out[k] = {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
                  "p90_us": float(np.percentile(v, 90))}
    out["rollout_vjp"]["tflops"] = flop / (out["rollout_vjp"]["median_us"] * 1e-6) / 1e12
    out["vjp_over_lqr_backward"] = out["rollout_vjp"]["median_us"] / out["lqr_backward"]["median_us"]
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=list(SHAPES))
    a = ap.parse_args()
    rows = [engine_level(s, a.calls) for s in ([a.shape] if a.shape else SHAPES)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
