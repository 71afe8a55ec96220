"""Cost of gmpc_expert_vjp (the VJP of the expert sequence model's rollout) against gmpc_expert_loss_grad on the same
batch with S = hist + T steps and teacher forcing off: the same forward, BPTT and weight sums, one window per
workgroup there, four per workgroup here.

Engine level: the VJP with both cotangents and both outputs, the VJP without grad_history, the yardstick, and the
forward alone (gmpc_expert_rollout), alternating one call each after warm-up, device time per call from a
synchronised host clock over `--calls` calls.  Shapes: the reference regime (x 17, m 6, LSTM F 128, heads 3 x 128,
hist 1, T 5, B 128) and the C3 horizon (same model, hist 1, T 50, B 1024).  Kernel-only times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script per shape (--shape), committed as
profiles/expert_vjp_kernel_stats_<shape>.csv.

    python profiles/expert_vjp_timing.py [--calls 30] [--out FILE] [--shape cheetah-T5-B128|C3]
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from cotangent_timing import _mlp, _timed  # noqa: E402
from gan_mpc_amd.engine import Engine, make_expert_shape  # noqa: E402

# name: (x_size, m, F, head hidden widths, hist, T, B)
SHAPES = {"cheetah-T5-B128": (17, 6, 128, (128, 128), 1, 5, 128), "C3": (17, 6, 128, (128, 128), 1, 50, 1024)}


def engine_level(name, calls):
    n, m, F, hidden, hist, T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    eng = Engine(n, m, T, [n + m, 8, n], [n, 1], max_batch=B)
    d = eng.to_dev
    dx, du = [F, *hidden, n], [F, *hidden, m]
    lstm = [rng.standard_normal((n, 4 * F)) / np.sqrt(n), rng.standard_normal((F, 4 * F)) / np.sqrt(F),
            0.1 * rng.standard_normal(4 * F)]
    flat = d(np.concatenate([a.reshape(-1) for a in lstm] + [_mlp(rng, dx, 0.3), _mlp(rng, du)]).astype(np.float32))
    es = make_expert_shape(F, dx, du)
    S = hist + T
    history = d(rng.standard_normal((B, hist + 1, n)).astype(np.float32))
    g_goal = d(rng.standard_normal((B, T + 1, n)).astype(np.float32))
    g_U = d(rng.standard_normal((B, T, m)).astype(np.float32))
    xseq = d(rng.standard_normal((B, S, n)).astype(np.float32))
    useq = d(np.tanh(rng.standard_normal((B, S, m))).astype(np.float32))
    yseq = d(rng.standard_normal((B, S, n)).astype(np.float32))
    calls_ = {"expert_vjp": lambda: eng.expert_vjp(history, flat, es, g_goal, g_U),
              "expert_vjp_params_only": lambda: eng.expert_vjp(history, flat, es, g_goal, g_U, want_history=False),
              "expert_loss_grad": lambda: eng.expert_loss_grad(xseq, useq, yseq, flat, es, 0.9, False),
              "expert_rollout": lambda: eng.expert_rollout(history, flat, es)}
    for fn in calls_.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in calls_}
    for _ in range(calls):             # alternate, one call each, so that drift hits all alike
        for k, fn in calls_.items():
            res[k].append(_timed(fn, 1)["median_us"])
    out = {"level": "engine", "shape": name, "n": n, "m": m, "F": F, "hist": hist, "T": T, "B": B, "calls": calls}
    for k, v in res.items():
        v = np.asarray(v)
        out[k] = {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
                  "p90_us": float(np.percentile(v, 90))}
    y = out["expert_loss_grad"]
    out["vjp_over_loss_grad"] = out["expert_vjp"]["median_us"] / y["median_us"]
    # the expectation: the VJP's median is no higher than the yardstick's median plus its own p10-p90 spread
    out["expectation_us"] = y["median_us"] + (y["p90_us"] - y["p10_us"])
    out["expectation_met"] = bool(out["expert_vjp"]["median_us"] <= out["expectation_us"])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=list(SHAPES))
    a = ap.parse_args()
    rows = [engine_level(s, a.calls) for s in ([a.shape] if a.shape else SHAPES)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
