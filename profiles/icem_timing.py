"""Wall time and objective of the sample-efficient CEM (gmpc_icem_solve) beside the plain
cross-entropy method (gmpc_cem_solve) on the same inputs, in ONE process with alternating calls, on the problem of
profiles/cem_timing.py: cheetah (n 17, m 6), horizon 5, dynamics 3 x 200 relu, cost 128-128-10, bounds of +-1, at
B = 1 and B = 128.

  tie    icem_solve under the tie settings (no kept rows, decay 1, white noise, no mean row, the mean returned) against
         cem_solve under trajax' keywords: the same samples, costs, elites and update, so the ratio of the medians
         prices the pool's bookkeeping alone.
  paper  icem_solve under ICEM_KWARGS (3 iterations of 100 / 80 / 64 samples, coloured noise, 3 kept rows, the best row
         returned) against cem_solve under TRAJAX_CEM_KWARGS (10 iterations of 400): time per call and the mean
         objective each reaches.
  mpc    20 consecutive MPC steps on the model itself (x <- predict(x, u_0), the start shifted one step): cem, icem with
         the kept rows carried over and shifted (what the policy's shift_elites does) and icem without; per-step time
         and the mean over steps and problems of the objective of the returned sequence.  Repeated --calls / 20 times
         from the same initial state.

Each call = the solve followed by reading the first controls back to the host.  Prints one JSON line per (shape, leg).

    python profiles/icem_timing.py [--calls 200] [--shapes cheetah1,cheetah128] [--legs tie,paper,mpc] [--out FILE]

Kernel times come from a run of their own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/icem_timing.py --calls 20 --legs tie
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

import cem_timing as ct  # noqa: E402
import mpc_action_timing as base  # noqa: E402
from gan_mpc_amd.engine import ICEM_KWARGS, TRAJAX_CEM_KWARGS  # noqa: E402
from gan_mpc_amd.policy.optimizers import shift_warm_start  # noqa: E402

SHAPES = {"cheetah1": (5, 1), "cheetah128": (5, 128)}      # name -> (T, B)
BOUND = ct.BOUND
TIE = dict(keep_portion=0.0, decay=1.0, noise_beta=0.0, add_mean=False, return_best=False)
STEPS = 20


def _alternate(solvers, calls):
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
    out = {}
    for k, fn in solvers.items():
        out[k] = base._stats(times[k])
        out[k]["mean_objective"] = float(fn()["obj"].mean().item())
    return out


def _launches(kw):
    return 2 * kw["max_iter"] + 1


def run_pair(name, leg, calls):
    T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    ckw = dict(TRAJAX_CEM_KWARGS)
    ikw = dict(TRAJAX_CEM_KWARGS, **TIE) if leg == "tie" else dict(ICEM_KWARGS)
    ikw.pop("sampling_smoothing", None)
    res = {"shape": name, "leg": leg, "T": T, "B": B, "calls": calls, "bound": BOUND, "cem_kwargs": ckw,
           "icem_kwargs": ikw}
    res.update(_alternate({"cem": lambda: eng.cem_solve(x0, U, goal, -BOUND, BOUND, ckw),
                           "icem": lambda: eng.icem_solve(x0, U, goal, -BOUND, BOUND, ikw)}, calls))
    res["cem"]["launches"], res["icem"]["launches"] = _launches(ckw), _launches(ikw)
    res["icem_over_cem_median"] = res["icem"]["median_us"] / res["cem"]["median_us"]
    res["mean_objective_of_the_clipped_start"] = eng.rollout_cost(x0, torch.clamp(U, -BOUND, BOUND),
                                                                  goal)[1].sum(1).mean().item()
    eng.close()
    return res


def run_mpc(name, calls):
    T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x_first, U_first, goal = ct._inputs(eng, T, B, rng)
    ckw, ikw = dict(TRAJAX_CEM_KWARGS), dict(ICEM_KWARGS)

    def episode(kind, times, objs, seed):
        x, U, state = x_first, torch.clamp(U_first, -BOUND, BOUND), None
        for k in range(STEPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "cem":
                sol = eng.cem_solve(x, U, goal, -BOUND, BOUND, dict(ckw, seed=seed + k))
            else:
                sol = eng.icem_solve(x, U, goal, -BOUND, BOUND, dict(ikw, seed=seed + k), state=state)
            u0 = torch.clamp(sol["U"], -BOUND, BOUND)[:, 0].contiguous()
            u0.cpu()
            times.append(time.perf_counter() - t0)
            objs.append(float(sol["obj"].mean().item()))
            x = eng.predict(x, u0)
            U = shift_warm_start(torch.clamp(sol["U"], -BOUND, BOUND))
            if kind == "icem_shift":
                st = sol["state"]
                state = dict(keep=shift_warm_start(st["keep"].flatten(0, 1)).reshape(st["keep"].shape),
                             best_U=st["best_U"], best_cost=torch.full_like(st["best_cost"], float("inf")))

    res = {"shape": name, "leg": "mpc", "T": T, "B": B, "steps": STEPS, "episodes": max(calls // STEPS, 1),
           "bound": BOUND, "cem_kwargs": ckw, "icem_kwargs": ikw}
    kinds = ("cem", "icem_shift", "icem")
    for kind in kinds:
        episode(kind, [], [], 0)         # warm-up
    times, objs = {k: [] for k in kinds}, {k: [] for k in kinds}
    for ep in range(res["episodes"]):
        for kind in kinds:
            episode(kind, times[kind], objs[kind], 1000 * ep)
    for kind in kinds:
        res[kind] = base._stats(times[kind])
        res[kind]["mean_objective_over_steps"] = float(np.mean(objs[kind]))
        res[kind]["launches_per_step"] = _launches(ckw if kind == "cem" else ikw)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--shapes", default="cheetah1,cheetah128")
    ap.add_argument("--legs", default="tie,paper,mpc")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name in a.shapes.split(","):
        for leg in a.legs.split(","):
            res = run_mpc(name, a.calls) if leg == "mpc" else run_pair(name, leg, a.calls)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
