"""Cost of the caller-defined upper-level loss path (gmpc_bilevel_grad_cotangent) against the kernels' own L2 loss.

Engine level: gmpc_bilevel_grad (loss_kind 0: k_l2loss writes lx, then Bvec, the Hessian solve, cost_vjp) against
gmpc_bilevel_grad_cotangent fed the same lx (the same kernels without k_l2loss), after one solve, alternating, device
time per call from a synchronised host clock over `--calls` calls.  Shapes: C3 (n 17, m 6, T 50, B 1024) and the
reference regime (cheetah n 17, m 6, T 5, B 128); dynamics 3 x 200 relu, cost 128-128-10.

Policy level: loss_and_grad of a BaseMPC subclass whose torch loss is the L2 formula (solve, torch.func vmap + grad of
the loss, the cotangent entry point) against L2MPC.loss_and_grad (solve, gmpc_bilevel_grad), cheetah sizes, T 5,
B 128, maxiter 100 (the reference kwargs), alternating; the solve is in both.

    python profiles/cotangent_timing.py [--calls 50] [--out FILE]
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

from gan_mpc_amd import utils  # noqa: E402
from gan_mpc_amd.engine import Engine  # noqa: E402
from gan_mpc_amd.expert.expert_model import TableExpert  # noqa: E402
from gan_mpc_amd.norm import l2_policy  # noqa: E402
from gan_mpc_amd.policy import base  # noqa: E402

SHAPES = {"C3": (17, 6, 50, 1024), "cheetah-T5-B128": (17, 6, 5, 128)}


def _mlp(rng, dims, last_scale=1.0):
    out = []
    for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        W = rng.standard_normal((a, b)) / np.sqrt(a)
        if l == len(dims) - 2:
            W = W * last_scale
        out += [W.reshape(-1), 0.1 * rng.standard_normal(b)]
    return np.concatenate(out).astype(np.float32)


def _timed(fn, calls):
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts) * 1e6
    return {"median_us": float(np.median(ts)), "p10_us": float(np.percentile(ts, 10)),
            "p90_us": float(np.percentile(ts, 90))}


def engine_level(name, calls):
    n, m, T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    dyn_dims, cost_dims = [n + m, 200, 200, 200, n], [n, 128, 128, 10]
    eng = Engine(n, m, T, dyn_dims, cost_dims, max_batch=B)
    d = eng.to_dev
    params = (d(np.zeros(3, np.float32)), d(_mlp(rng, dyn_dims, 0.1)), d(_mlp(rng, cost_dims)))
    eng.set_params(*params)
    x0 = rng.standard_normal((B, n)).astype(np.float32)
    U = np.tanh(rng.standard_normal((B, T, m))).astype(np.float32)
    goal = rng.standard_normal((B, T + 1, n)).astype(np.float32)
    goal[:, 0] = x0
    desired = d(rng.standard_normal((B, T + 1, n)).astype(np.float32))
    eng.ilqr_solve(d(x0), d(U), d(goal), {"maxiter": 5})
    g = eng.new(3 + eng.cost_count)
    eng.bilevel_grad(B, 0, desired=desired, grad_sum=g)
    lx = eng.debug_buffer(11, (B, T + 1, n)).contiguous()
    g2 = eng.new(3 + eng.cost_count)
    eng.bilevel_grad_cotangent(B, lx, grad_sum=g2)
    torch.cuda.synchronize()
    same = bool(torch.equal(g, g2))
    calls_ = {"bilevel_grad_l2": lambda: eng.bilevel_grad(B, 0, desired=desired, grad_sum=g),
              "bilevel_grad_cotangent": lambda: eng.bilevel_grad_cotangent(B, lx, grad_sum=g2)}
    for fn in calls_.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in calls_}
    for _ in range(calls):             # alternate, one call each, so that drift hits both alike
        for k, fn in calls_.items():
            res[k].append(_timed(fn, 1)["median_us"])
    out = {"level": "engine", "shape": name, "n": n, "m": m, "T": T, "B": B, "calls": calls,
           "grad_sum_bitwise_equal": same}
    for k, v in res.items():
        v = np.asarray(v)
        out[k] = {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
                  "p90_us": float(np.percentile(v, 90))}
    out["cotangent_minus_l2_median_us"] = out["bilevel_grad_cotangent"]["median_us"] - out["bilevel_grad_l2"]["median_us"]
    eng.close()
    return out


class TorchL2MPC(base.BaseMPC):
    def loss(self, xcseq, useq, params, desired_xseq):
        del useq, params
        d = xcseq[:, : desired_xseq.shape[-1]] - desired_xseq
        return (d * d).mean(0).sum()


def _policy(cls, N, M, T, B, rng_seed=3):
    config = utils.get_config(os.path.join(ROOT, "tests", "golden", "mirror_config.yaml"))
    config.mpc.horizon = T
    config.mpc.model.dynamics.mlp.num_hidden_units = 200
    config.mpc.model.cost.mlp.num_hidden_units = 128
    config.mpc.model.cost.mlp.fout = 10
    cost, _ = utils.get_cost_model(config)
    dynamics, _ = utils.get_dynamics_model(config, N)
    rng = np.random.default_rng(rng_seed)
    hist = rng.standard_normal((B, config.mpc.history + 1, N)).astype(np.float32)
    goal = rng.standard_normal((B, T + 1, N)).astype(np.float32)
    goal[:, 0] = hist[:, -1]
    init_U = np.tanh(rng.standard_normal((B, T, M))).astype(np.float32)
    Y = rng.standard_normal((B, T + 1, N)).astype(np.float32)
    policy = cls(config=config, cost_model=cost, dynamics_model=dynamics, expert_model=TableExpert(goal, init_U))
    mpc_weights = tuple(config.mpc.model.cost.weights.to_dict().values())
    params = policy.init(mpc_weights, (config.seed, N), (config.seed, M), (True,))
    last = f"Dense_{config.mpc.model.dynamics.mlp.num_layers - 1}"
    params["dynamics_params"]["params"][last]["kernel"] *= 0.1
    policy.expert_model.select(np.arange(B))
    return policy, policy.to_device_params(params), hist, Y


def policy_level(calls):
    N, M, T, B = 17, 6, 5, 128
    pols = {k: _policy(cls, N, M, T, B) for k, cls in (("L2MPC", l2_policy.L2MPC), ("TorchL2MPC", TorchL2MPC))}

    def step(k):
        policy, dp, hist, Y = pols[k]
        policy.loss_and_grad(hist, dp, (Y,))

    for k in pols:
        for _ in range(3):
            step(k)
    res = {k: [] for k in pols}
    for _ in range(calls):
        for k in pols:
            res[k].append(_timed(lambda: step(k), 1)["median_us"])
    out = {"level": "policy loss_and_grad", "n": N, "m": M, "T": T, "B": B, "calls": calls}
    for k, v in res.items():
        v = np.asarray(v)
        out[k] = {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
                  "p90_us": float(np.percentile(v, 90))}
    out["torch_loss_minus_l2_median_us"] = out["TorchL2MPC"]["median_us"] - out["L2MPC"]["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for r in [engine_level(name, a.calls) for name in SHAPES] + [policy_level(a.calls)]:
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
