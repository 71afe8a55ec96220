"""Cost of the bilevel tail behind a held box solve (gmpc_ilqr_solve_box_held) beside the same tail behind
gmpc_ilqr_solve_fused, and of the held solve beside the plain box solve.  Shapes: the reference regime (cheetah n 17,
m 6, T 5, B 128) and the training shape (n 17, m 6, T 32, B 1024); dynamics 3 x 200 relu, cost 128-128-10; solves with
maxiter 6; bounds of +-0.5 x the median |U| of the fused solution under the reference kwargs (as
profiles/box_solve_timing.py: this problem's optimal controls are small, so most controls of the box solution end at a
bound; the share in the final clamped set is printed).  ONE process, alternating calls:

  (a) "tail_box":   bilevel_grad_cotangent (lx and lu of an L2 + control loss) on an engine holding the box solution --
                    k_riccati_w2<17, 6, HESS, LU, BOX> with the clamped words, then the cost stage and the weight sums;
  (b) "tail_fused": the same call on a second engine holding the fused solution of the same problem --
                    k_riccati_w2<17, 6, HESS, LU>, the code the masked form leaves untouched;
  (c) "solve_held" against "solve_box": the solve followed by reading the first controls back; their difference is the
      launch of k_box_clamped.

Each figure is the wall time of one call between two device synchronisations: median / p10 / p90 over `--calls`.

    python profiles/box_grad_timing.py [--calls 200] [--out profiles/box_grad_timing.jsonl]
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

from gan_mpc_amd.engine import TRAJAX_iLQR_KWARGS, Engine  # noqa: E402

SHAPES = {"cheetah-T5-B128": (17, 6, 5, 128), "train-T32-B1024": (17, 6, 32, 1024)}
KW = {"maxiter": 6}


def _mlp(rng, dims, last_scale=1.0):
    out = []
    for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        W = rng.standard_normal((a, b)) / np.sqrt(a)
        if l == len(dims) - 2:
            W = W * last_scale
        out += [W.reshape(-1), 0.1 * rng.standard_normal(b)]
    return np.concatenate(out).astype(np.float32)


def _one(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def _stats(v):
    v = np.asarray(v)
    return {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)),
            "p90_us": float(np.percentile(v, 90))}


def _alternate(fns, calls):
    for fn in fns.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in fns}
    for _ in range(calls):             # one call each in turn, so that drift hits all alike
        for k, fn in fns.items():
            res[k].append(_one(fn))
    return {k: _stats(v) for k, v in res.items()}


def run(name, calls):
    n, m, T, B = SHAPES[name]
    rng = np.random.default_rng(0)
    dyn_dims, cost_dims = [n + m, 200, 200, 200, n], [n, 128, 128, 10]
    flat = (np.zeros(3, np.float32), _mlp(rng, dyn_dims, 0.1), _mlp(rng, cost_dims))
    x0 = rng.standard_normal((B, n)).astype(np.float32)
    U = np.tanh(rng.standard_normal((B, T, m))).astype(np.float32)
    goal = rng.standard_normal((B, T + 1, n)).astype(np.float32)
    goal[:, 0] = x0
    desired = rng.standard_normal((B, T + 1, n)).astype(np.float32)
    engs = []
    for _ in range(2):
        eng = Engine(n, m, T, dyn_dims, cost_dims, max_batch=B)
        eng.set_params(*(eng.to_dev(a) for a in flat))
        engs.append(eng)
    box, fus = engs
    args = tuple(box.to_dev(a) for a in (x0, U, goal))
    ref = fus.ilqr_solve_fused(*args, dict(TRAJAX_iLQR_KWARGS))
    bound = float(np.float32(0.5 * np.median(np.abs(ref["U"].cpu().numpy()))))
    out = {"shape": name, "n": n, "m": m, "T": T, "B": B, "calls": calls, "maxiter": KW["maxiter"], "bound": bound}
    # (c) the solves
    out.update(_alternate({"solve_box": lambda: box.ilqr_solve_box(*args, -bound, bound, KW)["U"][:, 0].cpu(),
                           "solve_held": lambda: box.ilqr_solve_box_held(*args, -bound, bound, KW)["U"][:, 0].cpu()},
                          calls))
    out["held_over_box"] = out["solve_held"]["median_us"] / out["solve_box"]["median_us"]
    # (a) / (b) the tails, each on its own held solution
    sols = {"box": box.ilqr_solve_box_held(*args, -bound, bound, KW), "fused": fus.ilqr_solve_fused(*args, KW)}
    words = box.debug_buffer(18, (B, T)).view(torch.int32).cpu().numpy().view(np.uint32)
    out["share_of_controls_clamped"] = float(np.unpackbits(words.view(np.uint8)).sum() / (B * T * m))
    des = box.to_dev(desired)
    cots = {}
    for k, sol in sols.items():
        lx = (2.0 * (sol["X"] - des) / (T + 1)).contiguous()
        cots[k] = (lx, (0.1 * sol["U"]).contiguous())
    gs = {k: e.new(3 + e.cost_count) for k, e in (("box", box), ("fused", fus))}
    out.update(_alternate({"tail_box": lambda: box.bilevel_grad_cotangent(B, *cots["box"], grad_sum=gs["box"]),
                           "tail_fused": lambda: fus.bilevel_grad_cotangent(B, *cots["fused"], grad_sum=gs["fused"])},
                          calls))
    out["tail_box_over_fused"] = out["tail_box"]["median_us"] / out["tail_fused"]["median_us"]
    out["grads_finite"] = bool(torch.isfinite(gs["box"]).all() and torch.isfinite(gs["fused"]).all())
    for e in engs:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name in a.shapes.split(","):
        lines.append(json.dumps(run(name, a.calls)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
