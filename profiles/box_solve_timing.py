"""Wall time of the control-limited one-launch solve (gmpc_ilqr_solve_box) beside gmpc_ilqr_solve_fused on the same
inputs: cheetah (n 17, m 6), horizon 5, dynamics 4 x 200 relu, cost 128-128-10, the reference kwargs, at B = 1 and
B = 128, in ONE process with alternating calls (the problem and its inputs are those of profiles/mpc_action_timing.py).

Three calls alternate: "fused"; "box_inactive" -- bounds of -inf / +inf, the same results bit for bit, what the box
form costs when it does nothing (a compare per control and one QP pass per step); "box_active" -- bounds of +-0.5 x the
median |U| of the fused solution (this problem's optimal controls are ~1e-4, so almost every control ends at a bound
and the solve stops after one or two iterations).  Each call = the solve followed by reading the first controls back
to the host; the box calls include Engine.ilqr_solve_box's host check of the bounds (their device copies are uploaded
once).  Prints one JSON line per batch size: median / p10 / p90 wall time per call, mean and max iterations, the time
per call divided by (max iterations + 1) -- the number of backward passes of the slowest trajectory --, for the
box calls the QP iterations per step (debug buffer 15), and whether the inactive box call's median lies inside the
fused call's own p10 - p90 spread.

    python profiles/box_solve_timing.py [--calls 200] [--out profiles/box_solve_timing.jsonl]
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
from gan_mpc_amd.engine import TRAJAX_iLQR_KWARGS  # noqa: E402

N, M, T = 17, 6, base.T


def run(B, calls):
    rng = np.random.default_rng(0)
    eng = base._engine(N, M, 128, rng)
    kw = dict(TRAJAX_iLQR_KWARGS)
    args = base._inputs(eng, N, M, B, rng)
    ref = eng.ilqr_solve_fused(*args, kw)
    bound = float(np.float32(0.5 * np.median(np.abs(ref["U"].cpu().numpy()))))
    inf = float("inf")
    solvers = {"fused": lambda: eng.ilqr_solve_fused(*args, kw),
               "box_inactive": lambda: eng.ilqr_solve_box(*args, -inf, inf, kw),
               "box_active": lambda: eng.ilqr_solve_box(*args, -bound, bound, kw)}
    res = {"shape": "cheetah", "n": N, "m": M, "T": T, "B": B, "calls": calls, "bound": bound}
    same = solvers["box_inactive"]()
    res["inactive_equals_fused_bitwise"] = bool(all(torch.equal(same[k], ref[k]) for k in ref))
    for fn in solvers.values():
        for _ in range(10):
            fn()["U"][:, 0].cpu()
    times = {k: [] for k in solvers}
    for _ in range(calls):
        for k, fn in solvers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()["U"][:, 0].cpu()
            times[k].append(time.perf_counter() - t0)
    for k, fn in solvers.items():
        out = fn()
        it = out["iterations"].float().cpu().numpy()
        s = base._stats(times[k])
        s["mean_iterations"] = float(it.mean())
        s["max_iterations"] = int(it.max())
        # a call is the launch, the initial rollout / linearisation / backward pass, then per iteration a line search,
        # a linearisation and a backward pass, and the readback: max iterations + 1 backward passes (the slowest
        # workgroup sets the time)
        s["us_per_call_over_iterations_plus_1"] = s["median_us"] / (float(it.max()) + 1.0)
        if k != "fused":
            count = eng.debug_buffer(15, (B, 2)).cpu().numpy()
            U = out["U"].cpu().numpy()
            s["qps_at_the_cap"] = int(count[:, 0].sum())
            s["qp_iterations_per_step"] = float(count[:, 1].sum() / ((it + 1).sum() * T))
            s["share_of_controls_at_a_bound"] = float((np.abs(U) == np.float32(bound)).mean()) if k == "box_active" else 0.0
        res[k] = s
    f = res["fused"]
    res["inactive_median_within_fused_p10_p90"] = bool(f["p10_us"] <= res["box_inactive"]["median_us"] <= f["p90_us"])
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--batches", default="1,128")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for B in a.batches.split(","):
        lines.append(json.dumps(run(int(B), a.calls)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
