"""Wall time of the VJP of a plan's rollout under every member of a dynamics ensemble (gmpc_ensemble_rollout_vjp,
DESIGN.md section 29) against the one route there was before it, on ONE engine in ONE process with alternating calls:
the same build, the same box, the same inputs (the protocol of profiles/ensemble_rollout_timing.py).

  cheetah (n 17, m 6), dynamics 3 x 200 relu, cost 128-128-10; horizon 5 at B = 1, 128 and horizon 50 at B = 8, 128;
  P = 3, 5, 16 members; cotangents of the states and of the costs.

  call         Engine.ensemble_rollout_vjp(members[:P], X, U, goal, gX, gcost): every output
  call_nomem   the same without "members" (no acts / dels rows, no weight-gradient GEMMs of the dynamics)
  loop         P x (Engine.set_params with member p as the dynamics + Engine.rollout_vjp(X[p], ...)): every output
  loop_nodyn   the same with want_dyn=False

The loops leave the sums over the members undone (P per-member results), which favours them.  Each timed call = an
untimed synchronise, the work, and reading dL/dU of the B plans back to the host.  Prints one JSON line per (shape, B,
P): median / p10 / p90 per way and the call's time over the loop's.

    python profiles/ensemble_rollout_vjp_timing.py [--calls 200] [--out FILE.jsonl]
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

SHAPES = ((5, 1), (5, 128), (50, 8), (50, 128))          # (T, B)
MEMBERS = (3, 5, 16)
WAYS = ("call", "call_nomem", "loop", "loop_nodyn")
NOMEM = ("x0", "U", "goal", "theta")


def run(T, B, calls):
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    mpc_w, nominal, cost = eng._keep
    # the members: the bound dynamics with every parameter moved by a few per cent (the values do not enter the time)
    Pmax = max(MEMBERS)
    noise = torch.as_tensor(rng.uniform(0.95, 1.05, (Pmax, nominal.numel())).astype(np.float32))
    members = (nominal[None, :] * noise.to(nominal.device)).contiguous()
    X = eng.ensemble_rollout(members, x0, U, goal, want=("X",))["X"]
    gX = eng.to_dev(rng.standard_normal(tuple(X.shape)).astype(np.float32))
    gc = eng.to_dev(rng.standard_normal(tuple(X.shape[:3])).astype(np.float32))

    def call(P, want=None):
        kw = {} if want is None else dict(want=want)
        eng.ensemble_rollout_vjp(members[:P], X[:P], U, goal, gX[:P], gc[:P], **kw)["U"].cpu()

    def loop(P, dyn=True):
        for p in range(P):
            eng.set_params(mpc_w, members[p], cost)
            out = eng.rollout_vjp(X[p], U, goal, gX[p], gc[p], want_dyn=dyn)
        out["U"].cpu()

    ways = dict(call=call, call_nomem=lambda P: call(P, NOMEM), loop=loop, loop_nodyn=lambda P: loop(P, False))
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
        res["call_over_loop"] = res["call"]["median_us"] / res["loop"]["median_us"]
        res["call_nomem_over_loop_nodyn"] = res["call_nomem"]["median_us"] / res["loop_nodyn"]["median_us"]
        out.append(res)
        print(json.dumps(res), flush=True)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = []
    for T, B in SHAPES:
        lines += [json.dumps(r) for r in run(T, B, a.calls)]
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
