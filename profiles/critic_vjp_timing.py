"""Cost of gmpc_critic_vjp with both gradient outputs against the two calls that give the same two gradients of the
same sequences without it: gmpc_critic_loss_grad (d theta, BCE delta) + gmpc_critic_score_vjp (dx, delta 1) -- two
forward sweeps, two head passes, two backward sweeps against one of each.

Engine level: the VJP with both outputs, with either one alone, and the two yardstick calls, alternating one call each
after warm-up, device time per call from a synchronised host clock over `--calls` calls.  Shapes: the C3 critic (n 17,
F 64, head 3 x 256, T 50, Bc 2048) and the reference regime (same model, T 5, Bc 256).  Kernel-only times come from a
separate `rocprofv3 --kernel-trace --stats` run of this script per shape (--shape), committed as
profiles/critic_vjp_kernel_stats_<shape>.csv: they hold k_lstm_bwd2<17, true, true, 2> (the VJP with both outputs) next
to <17, true, false, 2> (critic_loss_grad, the VJP with parameters only) and <17, false, true, 2> (critic_score_vjp, the
VJP with dx only) of the same run, the comparison that decides the register-weight route's dispatch.

    python profiles/critic_vjp_timing.py [--calls 30] [--out FILE] [--shape C3|T5-Bc256]
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
from gan_mpc_amd.engine import Engine  # noqa: E402

# name: (n, F, head hidden widths, T, Bc)
SHAPES = {"C3": (17, 64, (256, 256, 256), 50, 2048), "T5-Bc256": (17, 64, (256, 256, 256), 5, 256)}


def engine_level(name, calls):
    n, F, hidden, T, Bc = SHAPES[name]
    rng = np.random.default_rng(0)
    head = [F, *hidden, 1]
    eng = Engine(n, 6, T, [n + 6, 8, n], [n, 1], max_batch=Bc // 2, lstm_features=F, head_dims=head)
    d = eng.to_dev
    lstm = [rng.standard_normal((n, 4 * F)) / np.sqrt(n), rng.standard_normal((F, 4 * F)) / np.sqrt(F),
            0.1 * rng.standard_normal(4 * F)]
    crit = d(np.concatenate([a.reshape(-1) for a in lstm] + [_mlp(rng, head)]).astype(np.float32))
    xseq = d(rng.standard_normal((Bc, T + 1, n)).astype(np.float32))
    label = d(np.where(rng.permutation(Bc) % 2 == 0, 1.0, -1.0).astype(np.float32))
    g = d(rng.standard_normal(Bc).astype(np.float32))
    calls_ = {"critic_vjp": lambda: eng.critic_vjp(xseq, crit, g),
              "critic_vjp_params_only": lambda: eng.critic_vjp(xseq, crit, g, want_dx=False),
              "critic_vjp_dx_only": lambda: eng.critic_vjp(xseq, crit, g, want_params=False),
              "critic_loss_grad": lambda: eng.critic_loss_grad(xseq, label, crit),
              "critic_score_vjp": lambda: eng.critic_score_vjp(xseq, crit)}
    for fn in calls_.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in calls_}
    for _ in range(calls):             # alternate, one call each, so that drift hits all alike
        for k, fn in calls_.items():
            res[k].append(_timed(fn, 1)["median_us"])
    out = {"level": "engine", "shape": name, "n": n, "F": F, "head": list(hidden), "T": T, "Bc": Bc, "calls": calls}
    for k, v in res.items():
        v = np.asarray(v)
        out[k] = {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
                  "p90_us": float(np.percentile(v, 90))}
    a, b = out["critic_loss_grad"], out["critic_score_vjp"]
    out["yardstick_us"] = a["median_us"] + b["median_us"]
    out["vjp_over_yardstick"] = out["critic_vjp"]["median_us"] / out["yardstick_us"]
    # the expectation: the VJP's median is no higher than the two yardstick medians plus their p10-p90 spreads
    out["expectation_us"] = out["yardstick_us"] + (a["p90_us"] - a["p10_us"]) + (b["p90_us"] - b["p10_us"])
    out["expectation_met"] = bool(out["critic_vjp"]["median_us"] <= out["expectation_us"])
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
