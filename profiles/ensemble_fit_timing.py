"""Wall time of the dynamics regression for the P members of an ensemble: ONE call of
gmpc_dynamics_ensemble_loss_grad (k_dynfit_rows: matrix cores, members on the grid) against what an ensemble cost
before it, P x (gmpc_set_params + gmpc_dynamics_loss_grad) (k_dynfit: vector ALU, one model per call) -- on ONE engine
in ONE process with alternating calls: the same build, the same box, the same inputs.

  cheetah (n 17, m 6), dynamics 3 x 200 relu, S = 10 and 50, B = 64 and 256, P = 1, 3, 5, free-running and
  teacher-forced.

Each timed call = the launches followed by reading the P losses back to the host.  Prints one JSON line per (S, B,
mode): median / p10 / p90 per path and P, and new / (P x old) with old = the old path at P = 1.

    python profiles/ensemble_fit_timing.py [--calls 200] [--out FILE.jsonl]
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
from gan_mpc_amd import nn_init, params as params_lib  # noqa: E402
from gan_mpc_amd.engine import Engine  # noqa: E402

N, M, T = 17, 6, 50
DYN = [N + M, 200, 200, 200, N]
COST = [N, 128, 128, 10]
STEPS = (10, 50)
BATCHES = (64, 256)
MEMBERS = (1, 3, 5)
DISCOUNT = 0.95


def run(calls):
    rng = np.random.default_rng(0)
    eng = Engine(N, M, T, DYN, COST, max(BATCHES))
    d = eng.to_dev
    pack = lambda dims: params_lib.pack_mlp(nn_init.dense_tree(rng, dims))
    members = d(np.stack([pack(DYN) for _ in range(max(MEMBERS))]))
    mpc_w, cost = d(np.array([-2.0, 3.0, -3.0], np.float32)), d(pack(COST))
    out = []
    for S in STEPS:
        for B in BATCHES:
            x = d(rng.standard_normal((B, S, N)).astype(np.float32))
            u = d(np.tanh(rng.standard_normal((B, S, M))).astype(np.float32))
            y = d(rng.standard_normal((B, S, N)).astype(np.float32))
            for tf in (False, True):
                loss1, grad1 = eng.new(max(MEMBERS)), eng.new(max(MEMBERS), eng.dyn_count)

                def new(P):
                    eng.dynamics_ensemble_loss_grad(members[:P], x, u, y, DISCOUNT, tf, loss_sum=loss1[:P],
                                                    grad_sum=grad1[:P])
                    return loss1[:P].cpu()

                def old(P):
                    for p in range(P):
                        eng.set_params(mpc_w, members[p], cost)
                        eng.dynamics_loss_grad(x, u, y, DISCOUNT, tf, loss_sum=loss1[p:p + 1], grad_sum=grad1[p])
                    return loss1[:P].cpu()

                paths = {"new": new, "old": old}
                for _ in range(5):            # warm-up: first launches, workspace growth, code objects
                    for fn in paths.values():
                        for P in MEMBERS:
                            fn(P)
                times = {(k, P): [] for k in paths for P in MEMBERS}
                for _ in range(calls):
                    for P in MEMBERS:
                        for k, fn in paths.items():
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            fn(P)
                            times[(k, P)].append(time.perf_counter() - t0)
                res = {"n": N, "m": M, "dyn": DYN, "S": S, "B": B, "teacher_forcing": tf, "calls": calls}
                for (k, P), ts in times.items():
                    res[f"{k}_P{P}"] = base._stats(ts)
                t = lambda k: res[k]["median_us"]
                res["new_over_P_times_old"] = {f"P{P}": t(f"new_P{P}") / (P * t("old_P1")) for P in MEMBERS}
                res["new_over_old_same_P"] = {f"P{P}": t(f"new_P{P}") / t(f"old_P{P}") for P in MEMBERS}
                res["new_P_over_new_P1"] = {f"P{P}": t(f"new_P{P}") / t("new_P1") for P in MEMBERS}
                out.append(res)
                print(json.dumps(res), flush=True)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps(r) for r in run(a.calls)]
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
