"""Wall time of one plan tracked in closed loop under every member of a dynamics ensemble
(gmpc_ensemble_rollout_feedback) against the open-loop call it extends and against the only way
there was before it, on ONE engine in ONE process with alternating calls: the same build, the same box, the same inputs
(the protocol of profiles/ensemble_rollout_timing.py).

  cheetah (n 17, m 6), horizon 50, dynamics 3 x 200 relu, cost 128-128-10; B = 1, 128, 1024 plans; P = 1, 5, 16 members.
  The reference trajectory is the rollout of U under the bound dynamics, the gains are Engine.lqr_backward's there, the
  members start 0.02 N(0, 1) off x0 and the applied controls are clamped to -1 / +1.

  feedback  Engine.ensemble_rollout_feedback(members[:P], X, U, K, goal, x0=..., u_lo=-1, u_hi=1,
            want=("X", "U", "obj")): one launch
  open      Engine.ensemble_rollout(members[:P], x0, U, goal, want=("X", "obj")): one launch, no feedback
  host      P x (Engine.set_params with member p as the dynamics + T x (a torch matvec for K_t (x_t - X_t), add, clamp,
            Engine.predict)): the members' states and controls, no costs

Each timed call = the work followed by reading the last member's result back to the host; the host loop writes to
preallocated tensors, as the calls do to fresh ones.  Prints one JSON line per (B, P): median / p10 / p90 per way and
the feedback call's time over each of the other two.

    python profiles/ensemble_feedback_timing.py [--calls 100] [--batches 1,128,1024] [--out FILE.jsonl]
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

T = 50
MEMBERS = (1, 5, 16)
WAYS = ("feedback", "open", "host")


def run(B, calls):
    rng = np.random.default_rng(0)
    eng = ct._engine(T, B, rng)
    x0, U, goal = ct._inputs(eng, T, B, rng)
    mpc_w, nominal, cost = eng._keep
    # the members: the bound dynamics with every parameter moved by a few per cent (the values do not enter the time)
    noise = torch.as_tensor(rng.uniform(0.95, 1.05, (max(MEMBERS), nominal.numel())).astype(np.float32))
    members = (nominal[None, :] * noise.to(nominal.device)).contiguous()
    X, _ = eng.rollout_cost(x0, U, goal)
    K = eng.lqr_backward(X, U, goal, after_rollout=True)["K"]
    start = (x0 + 0.02 * torch.as_tensor(rng.standard_normal((B, ct.N)).astype(np.float32)).to(x0.device)).contiguous()
    Xbuf, Ubuf = eng.new(max(MEMBERS), B, T + 1, ct.N), eng.new(max(MEMBERS), B, T, ct.M)

    def feedback(P):
        eng.ensemble_rollout_feedback(members[:P], X, U, K, goal, x0=start, u_lo=-ct.BOUND, u_hi=ct.BOUND,
                                      want=("X", "U", "obj"))["obj"][P - 1].cpu()

    def open_loop(P):
        eng.ensemble_rollout(members[:P], start, U, goal, want=("X", "obj"))["obj"][P - 1].cpu()

    def host(P):
        for p in range(P):
            eng.set_params(mpc_w, members[p], cost)
            x = start
            Xbuf[p, :, 0] = x
            for t in range(T):
                du = torch.bmm(K[:, t], (x - X[:, t]).unsqueeze(-1)).squeeze(-1)
                u = torch.clamp(U[:, t] + du, -ct.BOUND, ct.BOUND)
                x = eng.predict(x, u)
                Ubuf[p, :, t] = u
                Xbuf[p, :, t + 1] = x
        Xbuf[P - 1, :, T].cpu()

    ways = dict(feedback=feedback, open=open_loop, host=host)
    for P in MEMBERS:                  # warm-up: first launches, workspace growth, code objects
        for w in WAYS:
            for _ in range(3 if w != "host" else 1):
                ways[w](P)
    eng.set_params(mpc_w, nominal, cost)
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
        res["feedback_over_open"] = res["feedback"]["median_us"] / res["open"]["median_us"]
        res["feedback_over_host"] = res["feedback"]["median_us"] / res["host"]["median_us"]
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
        if a.out:                      # (after every batch size: a run cut short keeps what it measured)
            with open(a.out, "w") as fp:
                fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
