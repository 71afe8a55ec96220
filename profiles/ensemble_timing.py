"""Wall time of the sampling solvers with their sampled rows costed on a dynamics ensemble (gmpc_set_sampled_ensemble,
DESIGN.md section 24) against the same solve without one, on ONE engine in ONE process with alternating calls: the
same build, the same box, the same inputs, the ensemble switched between calls.

  cheetah (n 17, m 6), horizon 5, dynamics 3 x 200 relu, cost 128-128-10, bounds of +-1, at B = 1 and B = 128;
  icem_solve and cem_solve at their default keywords; no ensemble and P = 1, 3, 5 members; fp32 and bf16 mode.

Each timed call = the solve followed by reading the first controls back to the host.  Switching the ensemble marks the
members' bf16 images stale, so every timed call follows one untimed solve under the same setting (which packs them): the
figures are those of a policy that sets its ensemble once.  Prints one JSON line per (shape, solver, precision): median /
p10 / p90 per setting and the three ratios of DESIGN.md section 24 -- (a) P = 1 over none, (b) time(P) / (P time(none)),
(c) time(P) / time(none).

    python profiles/ensemble_timing.py [--calls 200] [--shapes cheetah1,cheetah128] [--out FILE.jsonl]

Kernel times come from a run of their own (tracing slows the host): k_sampled_rollout<CemDrawn, BF16, CemMember>,
k_sampled_rollout<IcemDrawn, BF16, CemMember> (BF16 false / true) and k_ens_reduce in
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/ensemble_timing.py --calls 20
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
from gan_mpc_amd.engine import ICEM_KWARGS, TRAJAX_CEM_KWARGS  # noqa: E402

MODES = ("fp32", "bf16")
SOLVERS = ("icem", "cem")
MEMBERS = (None, 1, 3, 5)


def run(name, calls):
    T, B = ct.SHAPES[name]
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    nominal = eng._keep[1]
    # the members: the bound dynamics with every parameter moved by a few per cent (the values do not enter the time)
    noise = torch.as_tensor(rng.uniform(0.95, 1.05, (max(MEMBERS[1:]), nominal.numel())).astype(np.float32))
    members = (nominal[None, :] * noise.to(nominal.device)).contiguous()
    sets = {P: None if P is None else members[:P].contiguous() for P in MEMBERS}
    solvers = {"icem": lambda: eng.icem_solve(x0, U, goal, -ct.BOUND, ct.BOUND, dict(ICEM_KWARGS)),
               "cem": lambda: eng.cem_solve(x0, U, goal, -ct.BOUND, ct.BOUND, dict(TRAJAX_CEM_KWARGS))}
    out = []
    for solver in SOLVERS:
        for mode in MODES:
            eng.set_sampled_precision(mode)
            fn = solvers[solver]
            for P in MEMBERS:              # warm-up (first launches, workspace growth, code objects, the images)
                eng.set_sampled_ensemble(sets[P])
                for _ in range(5):
                    fn()["U"][:, 0].cpu()
            times = {P: [] for P in MEMBERS}
            for _ in range(calls):
                for P in MEMBERS:
                    eng.set_sampled_ensemble(sets[P])
                    fn()["U"][:, 0].cpu()          # untimed: packs the members' bf16 images behind the switch
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()["U"][:, 0].cpu()
                    times[P].append(time.perf_counter() - t0)
            res = {"shape": name, "n": ct.N, "m": ct.M, "T": T, "B": B, "calls": calls, "solver": solver,
                   "precision": mode}
            for P in MEMBERS:
                res["none" if P is None else f"P{P}"] = base._stats(times[P])
            t = lambda k: res[k]["median_us"]
            res["a_P1_over_none"] = t("P1") / t("none")
            res["b_time_over_P_times_none"] = {f"P{P}": t(f"P{P}") / (P * t("none")) for P in MEMBERS[1:]}
            res["c_time_over_none"] = {f"P{P}": t(f"P{P}") / t("none") for P in MEMBERS[1:]}
            out.append(res)
            print(json.dumps(res), flush=True)
    eng.set_sampled_ensemble(None)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--shapes", default="cheetah1,cheetah128")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name in a.shapes.split(","):
        lines += [json.dumps(r) for r in run(name, a.calls)]
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
