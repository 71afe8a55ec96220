"""Wall time of the batch-1 MPC action (reference policy/eval.py:126-128: one full iLQR solve per control step) on the
two solvers: gmpc_ilqr_solve (the host enqueues every iteration: ~20 launches each, the continuation flags polled four
iterations late) and gmpc_ilqr_solve_fused (the whole solve in one launch).

Per shape (pendulum n 3 / m 1 and cheetah n 17 / m 6, horizon 5, dynamics 4 x 200 relu, cost 128-128-10, the
reference kwargs), after a warm-up: 200 calls per solver, alternating, each call = the solve of one sample followed by
reading its first control back to the host (what EvalMPC.get_optimal_action hands its caller), then one B = 128 solve
per solver.  Prints one JSON line per shape: median / p10 / p90 wall time per call, the mean iteration count and the
time per iteration.

    python profiles/mpc_action_timing.py [--calls 200] [--out FILE]
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

from gan_mpc_amd.engine import TRAJAX_iLQR_KWARGS, Engine  # noqa: E402

SHAPES = {"pendulum": (3, 1), "cheetah": (17, 6)}
T = 5


def _mlp(rng, dims, last_scale=1.0):
    out = []
    for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        W = rng.standard_normal((a, b)) / np.sqrt(a)
        if l == len(dims) - 2:
            W = W * last_scale
        out += [W.reshape(-1), 0.1 * rng.standard_normal(b)]
    return np.concatenate(out).astype(np.float32)


def _engine(n, m, B, rng):
    dyn_dims, cost_dims = [n + m, 200, 200, 200, n], [n, 128, 128, 10]
    eng = Engine(n, m, T, dyn_dims, cost_dims, max_batch=B)
    d = eng.to_dev
    params = (d(np.array([0.0, 0.0, 0.0], np.float32)), d(_mlp(rng, dyn_dims, 0.1)), d(_mlp(rng, cost_dims)))
    eng.set_params(*params)
    eng._keep = params
    return eng


def _inputs(eng, n, m, B, rng):
    d = eng.to_dev
    x0 = rng.standard_normal((B, n)).astype(np.float32)
    U = np.tanh(rng.standard_normal((B, T, m))).astype(np.float32)
    goal = rng.standard_normal((B, T + 1, n)).astype(np.float32)
    goal[:, 0] = x0
    return d(x0), d(U), d(goal)


def _stats(ts):
    ts = np.asarray(ts) * 1e6
    return {"median_us": float(np.median(ts)), "p10_us": float(np.percentile(ts, 10)),
            "p90_us": float(np.percentile(ts, 90))}


def run(name, calls):
    n, m = SHAPES[name]
    rng = np.random.default_rng(0)
    eng = _engine(n, m, 128, rng)
    kw = dict(TRAJAX_iLQR_KWARGS)
    solvers = {"rounds": eng.ilqr_solve, "fused": eng.ilqr_solve_fused}
    one = _inputs(eng, n, m, 1, rng)
    res = {"shape": name, "n": n, "m": m, "T": T, "calls": calls}
    for fn in solvers.values():          # warm-up (first launches, pinned ring, code objects)
        for _ in range(10):
            fn(*one, kw)["U"][:, 0].cpu()
    times = {k: [] for k in solvers}
    iters = {k: [] for k in solvers}
    for _ in range(calls):
        for k, fn in solvers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*one, kw)
            out["U"][:, 0].cpu()
            times[k].append(time.perf_counter() - t0)
            iters[k].append(int(out["iterations"][0]))
    for k in solvers:
        it = float(np.mean(iters[k]))
        s = _stats(times[k])
        s["mean_iterations"] = it
        s["us_per_iteration"] = s["median_us"] / max(it, 1.0)
        res[f"B1_{k}"] = s
    res["B1_speedup_median"] = res["B1_rounds"]["median_us"] / res["B1_fused"]["median_us"]
    big = _inputs(eng, n, m, 128, rng)
    for k, fn in solvers.items():
        fn(*big, kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*big, kw)
        torch.cuda.synchronize()
        res[f"B128_{k}"] = {"wall_us": (time.perf_counter() - t0) * 1e6,
                            "mean_iterations": float(out["iterations"].float().mean()),
                            "max_iterations": int(out["iterations"].max())}
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--shapes", default="pendulum,cheetah")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name in a.shapes.split(","):
        r = run(name, a.calls)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
