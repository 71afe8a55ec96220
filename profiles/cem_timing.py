"""Wall time of the cross-entropy method solver (gmpc_cem_solve) beside the iLQR solves on the same
inputs, in ONE process with alternating calls:

  cheetah (n 17, m 6), horizon 5, dynamics 3 x 200 relu, cost 128-128-10 (the problem of profiles/mpc_action_timing.py)
  at B = 1 and B = 128: "cem" under trajax' keywords (400 samples, 40 elites, 10 iterations) and bounds of +-1, "rounds"
  (gmpc_ilqr_solve) and "box" (gmpc_ilqr_solve_box, the same bounds) under the reference's iLQR keywords;
  C3 size (the same networks, horizon 50, B = 1024): ONE iteration of each -- "cem" with max_iter 1, "rounds" with
  maxiter 1; the one-launch box solve does not cover T = 50.

Each call = the solve followed by reading the first controls back to the host.  Prints one JSON line per shape: median /
p10 / p90 wall time per call, the iLQR solves' mean / max iterations, the objectives reached (mean over the batch; the
iLQR "rounds" solve is unconstrained), and for "cem" the useful flops of a call (2 x the networks' multiply-adds x
B N T per iteration) over the median time.

    python profiles/cem_timing.py [--calls 200] [--shapes cheetah1,cheetah128,c3] [--out profiles/cem_timing.jsonl]

Kernel times come from a run of their own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/cem_timing.py --calls 20
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import mpc_action_timing as base  # noqa: E402
from gan_mpc_amd.engine import TRAJAX_CEM_KWARGS, TRAJAX_iLQR_KWARGS, Engine  # noqa: E402

N, M = 17, 6
DYN, COST = [N + M, 200, 200, 200, N], [N, 128, 128, 10]
SHAPES = {"cheetah1": (5, 1), "cheetah128": (5, 128), "c3": (50, 1024)}      # name -> (T, B)
BOUND = 1.0


def _engine(T, B, rng):
    eng = Engine(N, M, T, DYN, COST, max_batch=B)
    d = eng.to_dev
    params = (d(np.zeros(3, np.float32)), d(base._mlp(rng, DYN, 0.1)), d(base._mlp(rng, COST)))
    eng.set_params(*params)
    eng._keep = params
    return eng


def _inputs(eng, T, B, rng):
    d = eng.to_dev
    x0 = rng.standard_normal((B, N)).astype(np.float32)
    U = np.tanh(rng.standard_normal((B, T, M))).astype(np.float32)
    goal = rng.standard_normal((B, T + 1, N)).astype(np.float32)
    goal[:, 0] = x0
    return d(x0), d(U), d(goal)


def _mlp_macs(dims):
    return sum(a * b for a, b in zip(dims[:-1], dims[1:]))


def run(name, calls):
    T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    eng = _engine(T, B, rng)
    x0, U, goal = _inputs(eng, T, B, rng)
    one = name == "c3"            # one iteration of each solver
    ckw = dict(TRAJAX_CEM_KWARGS, max_iter=1) if one else dict(TRAJAX_CEM_KWARGS)
    ikw = dict(TRAJAX_iLQR_KWARGS, maxiter=1) if one else dict(TRAJAX_iLQR_KWARGS)
    solvers = {"cem": lambda: eng.cem_solve(x0, U, goal, -BOUND, BOUND, ckw),
               "rounds": lambda: eng.ilqr_solve(x0, U, goal, ikw)}
    if T <= 32:
        solvers["box"] = lambda: eng.ilqr_solve_box(x0, U, goal, -BOUND, BOUND, ikw)
    res = {"shape": name, "n": N, "m": M, "T": T, "B": B, "calls": calls, "bound": BOUND,
           "cem_kwargs": ckw, "ilqr_maxiter": ikw["maxiter"]}
    for fn in solvers.values():          # warm-up (first launches, workspace growth, code objects)
        for _ in range(5):
            fn()["U"][:, 0].cpu()
    times = {k: [] for k in solvers}
    for _ in range(calls):
        for k, fn in solvers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()["U"][:, 0].cpu()
            times[k].append(time.perf_counter() - t0)
    start = eng.rollout_cost(x0, torch.clamp(U, -BOUND, BOUND), goal)[1].sum(1).mean().item()
    res["mean_objective_of_the_clipped_start"] = start
    for k, fn in solvers.items():
        out = fn()
        s = base._stats(times[k])
        s["mean_objective"] = float(out["obj"].mean().item())
        if k == "cem":
            iters = ckw["max_iter"]
            flops = 2.0 * (_mlp_macs(DYN) * T + _mlp_macs(COST)) * B * ckw["num_samples"] * iters
            s["launches"] = 2 * iters + 1
            s["useful_gflop_per_call"] = flops / 1e9
            s["useful_tflops_at_the_median"] = flops / (s["median_us"] * 1e-6) / 1e12
        else:
            it = out["iterations"].float().cpu().numpy()
            s["mean_iterations"], s["max_iterations"] = float(it.mean()), int(it.max())
        res[k] = s
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--shapes", default="cheetah1,cheetah128,c3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name in a.shapes.split(","):
        lines.append(json.dumps(run(name, a.calls)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
