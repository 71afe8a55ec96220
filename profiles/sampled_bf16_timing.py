"""Wall time of the cross-entropy method solver with its sampled rollouts in fp32 and in bf16 mode
(gmpc_set_sampled_precision), on ONE engine in ONE process with alternating calls: the same
build, the same box, the same inputs, the mode switched between calls (no device work).

  The three shapes of profiles/cem_timing.py: cheetah (n 17, m 6), dynamics 3 x 200 relu, cost 128-128-10, bounds of
  +-1, trajax' keywords (400 samples, 40 elites): horizon 5 at B = 1 and B = 128 with 10 iterations, and the C3 size
  (horizon 50, B = 1024) with ONE iteration.

Each call = the solve followed by reading the first controls back to the host.  Prints one JSON line per shape: median /
p10 / p90 wall time per call and mode, the useful flops of a call over the median, and the fp32-evaluated objective of
each mode's result (gmpc_cem_solve's obj: always the fp32 rollout of the returned mean) beside the clipped start's.

    python profiles/sampled_bf16_timing.py [--calls 200] [--shapes cheetah1,cheetah128,c3] [--out FILE.jsonl]

Kernel times come from a run of their own (tracing slows the host): k_sampled_rollout<CemDrawn, false, CemOneModel> and
k_sampled_rollout<CemDrawn, true, CemOneModel> (the fp32 and the bf16 form) in
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/sampled_bf16_timing.py --calls 20
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import cem_timing as ct  # noqa: E402
import mpc_action_timing as base  # noqa: E402
import numpy as np  # noqa: E402
from gan_mpc_amd.engine import TRAJAX_CEM_KWARGS  # noqa: E402

MODES = ("fp32", "bf16")


def run(name, calls):
    T, B = ct.SHAPES[name]
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    kw = dict(TRAJAX_CEM_KWARGS, max_iter=1) if name == "c3" else dict(TRAJAX_CEM_KWARGS)

    def solve(mode):
        eng.set_sampled_precision(mode)
        return eng.cem_solve(x0, U, goal, -ct.BOUND, ct.BOUND, kw)

    res = {"shape": name, "n": ct.N, "m": ct.M, "T": T, "B": B, "calls": calls, "bound": ct.BOUND, "cem_kwargs": kw}
    for mode in MODES:                   # warm-up (first launches, workspace growth, code objects, the weight image)
        for _ in range(5):
            solve(mode)["U"][:, 0].cpu()
    times = {mode: [] for mode in MODES}
    for _ in range(calls):
        for mode in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            solve(mode)["U"][:, 0].cpu()
            times[mode].append(time.perf_counter() - t0)
    res["mean_objective_of_the_clipped_start"] = \
        eng.rollout_cost(x0, torch.clamp(U, -ct.BOUND, ct.BOUND), goal)[1].sum(1).mean().item()
    flops = 2.0 * (ct._mlp_macs(ct.DYN) * T + ct._mlp_macs(ct.COST)) * B * kw["num_samples"] * kw["max_iter"]
    for mode in MODES:
        s = base._stats(times[mode])
        s["mean_objective"] = float(solve(mode)["obj"].mean().item())
        s["useful_gflop_per_call"] = flops / 1e9
        s["useful_tflops_at_the_median"] = flops / (s["median_us"] * 1e-6) / 1e12
        res[mode] = s
    res["bf16_over_fp32_median"] = res["bf16"]["median_us"] / res["fp32"]["median_us"]
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
