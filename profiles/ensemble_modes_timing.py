"""Wall time of the sampling solvers under the ensemble modes (gmpc_set_sampled_ensemble_mode)
against the mean over the members and against no ensemble, on ONE engine in ONE process with alternating calls: the
same build, the same box, the same inputs, the setting switched between calls.

  cheetah (n 17, m 6), horizon 5, dynamics 3 x 200 relu, cost 128-128-10, bounds of +-1, at B = 1 and B = 128;
  icem_solve and cem_solve at their default keywords; fp32 and bf16 mode; the settings
    none       no ensemble
    mean       P = 5 members, the default mode (what this build's parent runs under an ensemble)
    mean_std   P = 5, mean + 1 x spread            max   P = 5, the worst member
    ts1q5      P = 5, 5 particles, mean            ts1q1 P = 5, 1 particle, mean

Each timed call = the solve followed by reading the first controls back to the host; every timed call follows one
untimed solve under the same setting (switching the ensemble marks the members' bf16 images stale).  Prints one JSON
line per (shape, solver, precision): median / p10 / p90 per setting and the ratios of DESIGN.md section 26 -- (b)
mean_std and max over mean, (c) ts1q5 over mean and ts1q1 over none.  For (a), the default mode against the parent
build, run this file with --default-only in both trees (it then never calls the new entry point) and compare the
`none` and `mean` columns.

    python profiles/ensemble_modes_timing.py [--calls 200] [--shapes cheetah1,cheetah128] [--default-only]
                                             [--build LABEL] [--out F [--append]]

--build labels every record (which tree ran), --append adds the records to F.  profiles/ensemble_modes_timing.jsonl
holds three runs: all settings on this build, then --default-only on this build and on the parent's:
    python profiles/ensemble_modes_timing.py --build this --out profiles/ensemble_modes_timing.jsonl
    python profiles/ensemble_modes_timing.py --build this --default-only --out profiles/ensemble_modes_timing.jsonl --append
    (in a checkout of the parent commit, with this file copied in) ... --build parent --default-only --out ... --append

Kernel times come from a run of their own (tracing slows the host): k_sampled_rollout<..., CemParticle> and
k_ens_reduce_risk in
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/ensemble_modes_timing.py --calls 20
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
P = 5
#            name        ensemble  mode (None: the entry point is not called)
SETTINGS = (("none",     False,    None),
            ("mean",     True,     None),
            ("mean_std", True,     dict(aggregate="mean_std", risk=1.0)),
            ("max",      True,     dict(aggregate="max")),
            ("ts1q5",    True,     dict(propagation="ts1", particles=5)),
            ("ts1q1",    True,     dict(propagation="ts1", particles=1)))


def run(name, calls, default_only, build):
    T, B = ct.SHAPES[name]
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    nominal = eng._keep[1]
    # the members: the bound dynamics with every parameter moved by a few per cent (the values do not enter the time)
    noise = torch.as_tensor(rng.uniform(0.95, 1.05, (P, nominal.numel())).astype(np.float32))
    members = (nominal[None, :] * noise.to(nominal.device)).contiguous()
    settings = [s for s in SETTINGS if s[2] is None] if default_only else list(SETTINGS)

    def switch(setting):
        _, ens, mode = setting
        eng.set_sampled_ensemble(members if ens else None)
        if not default_only:
            eng.set_sampled_ensemble_mode(**(mode or {}))

    solvers = {"icem": lambda: eng.icem_solve(x0, U, goal, -ct.BOUND, ct.BOUND, dict(ICEM_KWARGS)),
               "cem": lambda: eng.cem_solve(x0, U, goal, -ct.BOUND, ct.BOUND, dict(TRAJAX_CEM_KWARGS))}
    out = []
    for solver in SOLVERS:
        for prec in PRECISIONS:
            eng.set_sampled_precision(prec)
            fn = solvers[solver]
            for s in settings:             # warm-up (first launches, workspace growth, code objects, the images)
                switch(s)
                for _ in range(5):
                    fn()["U"][:, 0].cpu()
            times = {s[0]: [] for s in settings}
            for _ in range(calls):
                for s in settings:
                    switch(s)
                    fn()["U"][:, 0].cpu()          # untimed: packs the members' bf16 images behind the switch
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()["U"][:, 0].cpu()
                    times[s[0]].append(time.perf_counter() - t0)
            res = {"shape": name, "n": ct.N, "m": ct.M, "T": T, "B": B, "P": P, "calls": calls, "solver": solver,
                   "precision": prec, "default_only": bool(default_only), "build": build}
            for s in settings:
                res[s[0]] = base._stats(times[s[0]])
            t = lambda k: res[k]["median_us"]
            res["mean_over_none"] = t("mean") / t("none")
            if not default_only:
                res["b_over_mean"] = {k: t(k) / t("mean") for k in ("mean_std", "max")}
                res["c_ts1q5_over_mean"] = t("ts1q5") / t("mean")
                res["c_ts1q1_over_none"] = t("ts1q1") / t("none")
            out.append(res)
            print(json.dumps(res), flush=True)
    eng.set_sampled_ensemble(None)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--shapes", default="cheetah1,cheetah128")
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--build", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    lines = []
    for name in a.shapes.split(","):
        lines += [json.dumps(r) for r in run(name, a.calls, a.default_only, a.build)]
    if a.out:
        with open(a.out, "a" if a.append else "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
