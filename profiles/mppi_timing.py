"""Wall time of the path-integral solver (gmpc_mppi_solve / gmpc_mppi_vjp), in ONE process with
alternating calls, on the cheetah networks of profiles/cem_timing.py (n 17, m 6, dynamics 3 x 200 relu, cost
128-128-10), bounds of +-1, init_std 0.5:

  forward     mppi_solve against cem_solve at the same N (400) and iteration count (5), horizon 5, B = 1 and B = 128;
              each call = the solve followed by reading the first controls back to the host.
  train       what policy.differentiable.mppi_layer runs forward + backward (mppi_solve with the traces, then mppi_vjp
              with every output, on an engine of N min(B, 16) rows as the layer sizes it) against what ilqr_layer of a
              "box" policy runs (ilqr_solve_box_held, bilevel_grad_cotangent, bilevel_grad_inputs), horizon 5, B = 128;
              "mppi_1" and "mppi_32" are the same MPPI pair on engines of N and 32 N rows (1 and 32 problems per chunk).
  long        the MPPI pair alone at horizon 50, B = 8, N = 400: the one-launch box solve does not cover that horizon.

Prints one JSON line per shape: median / p10 / p90 wall time per call.

    python profiles/mppi_timing.py [--calls 200] [--shapes fwd1,fwd128,train128,long8]
                                   [--out profiles/mppi_timing.jsonl]

Kernel times come from a run of their own (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \
        python profiles/mppi_timing.py --calls 20 --shapes fwd128
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

import box_grad_timing as base  # noqa: E402
from gan_mpc_amd.engine import MPPI_KWARGS, TRAJAX_CEM_KWARGS, Engine  # noqa: E402

N, M = 17, 6
DYN, COST = [N + M, 200, 200, 200, N], [N, 128, 128, 10]
SHAPES = {"fwd1": (5, 1), "fwd128": (5, 128), "train128": (5, 128), "long8": (50, 8)}      # name -> (T, B)
BOUND, STD, SAMPLES, ITERS = 1.0, 0.5, 400, 5


def _engine(T, rows, flat):
    eng = Engine(N, M, T, DYN, COST, max_batch=rows)
    eng._keep = tuple(eng.to_dev(a) for a in flat)
    eng.set_params(*eng._keep)
    return eng


def run(name, calls):
    T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    flat = (np.zeros(3, np.float32), base._mlp(rng, DYN, 0.1), base._mlp(rng, COST))
    x0 = rng.standard_normal((B, N)).astype(np.float32)
    U = np.tanh(rng.standard_normal((B, T, M))).astype(np.float32)
    goal = rng.standard_normal((B, T + 1, N)).astype(np.float32)
    goal[:, 0] = x0
    desired = rng.standard_normal((B, T + 1, N)).astype(np.float32)
    mkw = dict(MPPI_KWARGS, num_samples=SAMPLES, max_iter=ITERS)
    ckw = dict(TRAJAX_CEM_KWARGS, num_samples=SAMPLES, max_iter=ITERS)
    res = {"shape": name, "n": N, "m": M, "T": T, "B": B, "calls": calls, "bound": BOUND, "init_std": STD,
           "mppi_kwargs": mkw}
    engs = []
    if name.startswith("fwd"):
        eng = _engine(T, B, flat)
        engs.append(eng)
        a = tuple(eng.to_dev(v) for v in (x0, U, goal))
        res.update(base._alternate({
            "mppi": lambda: eng.mppi_solve(*a, -BOUND, BOUND, mkw, init_std=STD)["U"][:, 0].cpu(),
            "cem": lambda: eng.cem_solve(*a, -BOUND, BOUND, ckw, init_std=STD)["U"][:, 0].cpu()}, calls))
        res["mppi_over_cem"] = res["mppi"]["median_us"] / res["cem"]["median_us"]
        res["mean_objective"] = {k: float(f(*a, -BOUND, BOUND, kw, init_std=STD)["obj"].mean().item())
                                 for k, f, kw in (("mppi", eng.mppi_solve, mkw), ("cem", eng.cem_solve, ckw))}
    else:
        def pair(eng):
            a = tuple(eng.to_dev(v) for v in (x0, U, goal))
            des = eng.to_dev(desired)

            def call():
                sol = eng.mppi_solve(*a, -BOUND, BOUND, mkw, init_std=STD, trace=True)
                gX = (2.0 * (sol["X"] - des)).contiguous()
                return eng.mppi_vjp(a[0], a[2], -BOUND, BOUND, sol, gX=gX, gobj=torch.ones_like(sol["obj"]),
                                    kwargs=mkw)["theta"][:1].cpu()
            return call

        fns = {}
        for key, per in (("mppi", 16), ("mppi_1", 1), ("mppi_32", 32)):
            rows = max(B, SAMPLES * min(B, per))
            if any(e.max_batch == rows for e in engs):
                continue
            engs.append(_engine(T, rows, flat))
            fns[key] = pair(engs[-1])
        if T <= 32:
            box = _engine(T, B, flat)
            engs.append(box)
            a = tuple(box.to_dev(v) for v in (x0, U, goal))
            des = box.to_dev(desired)
            kw = {"maxiter": 6}

            def box_call():
                sol = box.ilqr_solve_box_held(*a, -BOUND, BOUND, kw)
                lx = (2.0 * (sol["X"] - des)).contiguous()
                g = box.bilevel_grad_cotangent(B, lx, None, sign=-1.0)
                box.bilevel_grad_inputs(B, lx)
                return g[:1].cpu()
            fns["box"] = box_call
            res["box_maxiter"] = kw["maxiter"]
        res.update(base._alternate(fns, calls))
        if "box" in fns:
            res["mppi_over_box"] = res["mppi"]["median_us"] / res["box"]["median_us"]
    for e in engs:
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
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
