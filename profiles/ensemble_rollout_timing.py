"""Wall time of one plan's rollout under every member of a dynamics ensemble (gmpc_ensemble_rollout, DESIGN.md section
27) against the two ways there were before it, on ONE engine in ONE process with alternating calls: the same build, the
same box, the same inputs (the protocol of profiles/ensemble_timing.py).

  cheetah (n 17, m 6), horizon 50, dynamics 3 x 200 relu, cost 128-128-10; B = 1, 128, 1024 plans; P = 1, 5, 16 members.

  call      Engine.ensemble_rollout(members[:P], x0, U, goal, want=("X", "obj")): one launch
  rebind    P x (Engine.set_params with member p as the dynamics + Engine.rollout_cost): X and the per-step costs
  cem0      P x (Engine.set_params with member p + Engine.cem_solve(max_iter=0)): X and obj, the sampled rollout's
            one-row-per-problem form

Each timed call = the work followed by reading the last member's costs of the B plans back to the host; the outputs of
the two loops go to preallocated tensors, as the call's do to fresh ones.  Prints one JSON line per (B, P): median / p10
/ p90 per way and the call's time over each loop's.

    python profiles/ensemble_rollout_timing.py [--calls 100] [--batches 1,128,1024] [--out FILE.jsonl]
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

T = 50
MEMBERS = (1, 5, 16)
WAYS = ("call", "rebind", "cem0")


def run(B, calls):
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    mpc_w, nominal, cost = eng._keep
    # the members: the bound dynamics with every parameter moved by a few per cent (the values do not enter the time)
    noise = torch.as_tensor(rng.uniform(0.95, 1.05, (max(MEMBERS), nominal.numel())).astype(np.float32))
    members = (nominal[None, :] * noise.to(nominal.device)).contiguous()
    Xbuf, cbuf = eng.new(max(MEMBERS), B, T + 1, ct.N), eng.new(max(MEMBERS), B, T + 1)
    kw = dict(TRAJAX_CEM_KWARGS, max_iter=0)

    def call(P):
        eng.ensemble_rollout(members[:P], x0, U, goal, want=("X", "obj"))["obj"][P - 1].cpu()

    def rebind(P):
        for p in range(P):
            eng.set_params(mpc_w, members[p], cost)
            eng.rollout_cost(x0, U, goal, X=Xbuf[p], costs=cbuf[p])
        cbuf[P - 1, :, T].cpu()

    def cem0(P):
        for p in range(P):
            eng.set_params(mpc_w, members[p], cost)
            sol = eng.cem_solve(x0, U, goal, -ct.BOUND, ct.BOUND, kw)
        sol["obj"].cpu()

    ways = dict(call=call, rebind=rebind, cem0=cem0)
    for P in MEMBERS:                  # warm-up: first launches, workspace growth, code objects
        for w in WAYS:
            for _ in range(3):
                ways[w](P)
    times = {(w, P): [] for w in WAYS for P in MEMBERS}
    for _ in range(calls):
        for P in MEMBERS:
            for w in WAYS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ways[w](P)
                times[(w, P)].append(time.perf_counter() - t0)
    eng.set_params(mpc_w, nominal, cost)
    out = []
    for P in MEMBERS:
        res = {"shape": "cheetah", "n": ct.N, "m": ct.M, "T": T, "B": B, "P": P, "calls": calls}
        for w in WAYS:
            res[w] = base._stats(times[(w, P)])
        res["call_over_rebind"] = res["call"]["median_us"] / res["rebind"]["median_us"]
        res["call_over_cem0"] = res["call"]["median_us"] / res["cem0"]["median_us"]
        out.append(res)
        print(json.dumps(res), flush=True)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--batches", default="1,128,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for B in a.batches.split(","):
        lines += [json.dumps(r) for r in run(int(B), a.calls)]
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
