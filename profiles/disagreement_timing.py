"""Wall time of the sampling solvers under the one-step disagreement penalty (gmpc_set_sampled_disagreement, DESIGN.md
section 28) against the same solve on the same ensemble with the penalty off, on ONE engine in ONE process with
alternating calls: the same build, the same box, the same inputs, the setting switched between calls.

  cheetah (n 17, m 6), horizon 5, dynamics 3 x 200 relu, cost 128-128-10, bounds of +-1, at B = 1 and B = 128;
  icem_solve and cem_solve at their default keywords; fp32 and bf16 mode; P = 3 and P = 5 members; the settings
    none   no ensemble
    mean   P members, fixed propagation, aggregate mean, the penalty off (what this build's parent runs: the baseline)
    dis    the same with the penalty on: every plane rolls the rows out under the nominal model and runs member p's
           layers beside it -- two dynamics passes per step instead of one

Each timed call = the solve followed by reading the first controls back to the host; every timed call follows one
untimed solve under the same setting (switching the ensemble marks the members' bf16 images stale).  Prints one JSON
line per (shape, solver, precision, P): median / p10 / p90 per setting and the ratio dis / mean.

    python profiles/disagreement_timing.py [--calls 200] [--shapes cheetah1,cheetah128] [--out F]

Kernel times come from a run of their own (tracing slows the host): k_sampled_rollout<..., CemDisagree> against
k_sampled_rollout<..., CemMember> in
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/disagreement_timing.py --calls 20
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

PRECISIONS = ("fp32", "bf16")
SOLVERS = ("icem", "cem")
MEMBERS = (3, 5)
PENALTY = 64.0
#            name    ensemble  penalty
SETTINGS = (("none", False,    None),
            ("mean", True,     None),
            ("dis",  True,     PENALTY))


def run(name, calls):
    T, B = ct.SHAPES[name]
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    nominal = eng._keep[1]
    # the members: the bound dynamics with every parameter moved by a few per cent (the values do not enter the time)
    noise = torch.as_tensor(rng.uniform(0.95, 1.05, (max(MEMBERS), nominal.numel())).astype(np.float32))
    members = (nominal[None, :] * noise.to(nominal.device)).contiguous()
    eng.set_sampled_ensemble_mode()

    def switch(setting, P):
        _, ens, penalty = setting
        eng.set_sampled_ensemble(members[:P].contiguous() if ens else None)
        eng.set_sampled_disagreement(penalty)

    solvers = {"icem": lambda: eng.icem_solve(x0, U, goal, -ct.BOUND, ct.BOUND, dict(ICEM_KWARGS)),
               "cem": lambda: eng.cem_solve(x0, U, goal, -ct.BOUND, ct.BOUND, dict(TRAJAX_CEM_KWARGS))}
    out = []
    for solver in SOLVERS:
        for prec in PRECISIONS:
            eng.set_sampled_precision(prec)
            fn = solvers[solver]
            for P in MEMBERS:
                for s in SETTINGS:         # warm-up (first launches, workspace growth, code objects, the images)
                    switch(s, P)
                    for _ in range(5):
                        fn()["U"][:, 0].cpu()
                times = {s[0]: [] for s in SETTINGS}
                for _ in range(calls):
                    for s in SETTINGS:
                        switch(s, P)
                        fn()["U"][:, 0].cpu()          # untimed: packs the members' bf16 images behind the switch
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()["U"][:, 0].cpu()
                        times[s[0]].append(time.perf_counter() - t0)
                res = {"shape": name, "n": ct.N, "m": ct.M, "T": T, "B": B, "P": P, "calls": calls, "solver": solver,
                       "precision": prec, "penalty": PENALTY}
                for s in SETTINGS:
                    res[s[0]] = base._stats(times[s[0]])
                t = lambda k: res[k]["median_us"]
                res["mean_over_none"] = t("mean") / t("none")
                res["dis_over_mean"] = t("dis") / t("mean")
                out.append(res)
                print(json.dumps(res), flush=True)
    eng.set_sampled_ensemble(None)
    eng.set_sampled_disagreement(None)
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
