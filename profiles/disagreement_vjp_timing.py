"""Wall time of the VJP of a plan's one-step ensemble disagreement (gmpc_ensemble_disagreement_vjp, DESIGN.md section
30), on ONE engine in ONE process with alternating calls: the same build, the same box, the same inputs (the protocol of
profiles/ensemble_rollout_vjp_timing.py).  There is no earlier route to this gradient, so two existing calls stand
beside it for scale only.

  cheetah (n 17, m 6), dynamics 3 x 200 relu; horizon T = 5, 50 at B = 1, 128; P = 3, 5, 16 members; cotangents of d
  and of D.

  call         Engine.ensemble_disagreement_vjp(members[:P], X, U, gd, gD): every output
  call_nograd  the same without "nominal" and "members" (no acts / dels rows, no weight-gradient GEMMs)
  forward      Engine.ensemble_disagreement(members[:P], x0, U): the forward (X, d, D)
  chain        Engine.ensemble_rollout_vjp at P = 1 on the bound dynamics under gX, no cost cotangent, x0 and U wanted:
               the chain through the nominal rollout alone (it does not depend on P)

Each timed call = an untimed synchronise, the work, and reading one (B, ...) output back to the host.  Prints one JSON
line per (T, B, P): median / p10 / p90 per way.

    python profiles/disagreement_vjp_timing.py [--calls 200] [--out FILE.jsonl]
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

SHAPES = ((5, 1), (5, 128), (50, 1), (50, 128))          # (T, B)
MEMBERS = (3, 5, 16)
WAYS = ("call", "call_nograd", "forward", "chain")


def run(T, B, calls):
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    _, nominal, _ = eng._keep
    # the members: the bound dynamics with every parameter moved by a few per cent (the values do not enter the time)
    Pmax = max(MEMBERS)
    noise = torch.as_tensor(rng.uniform(0.95, 1.05, (Pmax, nominal.numel())).astype(np.float32))
    members = (nominal[None, :] * noise.to(nominal.device)).contiguous()
    X = eng.ensemble_disagreement(members, x0, U, want=("X",))["X"]
    gd = eng.to_dev(rng.standard_normal((Pmax, B, T)).astype(np.float32))
    gD = eng.to_dev(rng.standard_normal((Pmax, B)).astype(np.float32))
    gX = eng.to_dev(rng.standard_normal((1,) + tuple(X.shape)).astype(np.float32))
    X1, nom1 = X[None].contiguous(), nominal[None].contiguous()

    def call(P, want=None):
        kw = {} if want is None else dict(want=want)
        eng.ensemble_disagreement_vjp(members[:P], X, U, gd[:P].contiguous(), gD[:P].contiguous(), **kw)["U"].cpu()

    def forward(P):
        eng.ensemble_disagreement(members[:P], x0, U, want=("X", "d", "D"))["D"].cpu()

    def chain(P):
        eng.ensemble_rollout_vjp(nom1, X1, U, goal, gX, None, want=("x0", "U"))["U"].cpu()

    ways = dict(call=call, call_nograd=lambda P: call(P, ("x0", "U")), forward=forward, chain=chain)
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
    out = []
    for P in MEMBERS:
        res = {"shape": "cheetah", "n": ct.N, "m": ct.M, "T": T, "B": B, "P": P, "calls": calls}
        for w in WAYS:
            res[w] = base._stats(times[(w, P)])
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
