"""NumPy restatement of the sampled rollouts in bf16 mode (gmpc_set_sampled_precision; TEST
INFRASTRUCTURE).  Per sampled row:

  weights      every weight matrix rounded once to bf16 (round_bf16: to nearest even, a NaN kept); biases fp32
  layer input  [x_t; u_t], every relu output and x_T rounded to bf16 when it becomes a matrix operand
  product      of the rounded operands, accumulated in fp64 and rounded once to fp32 (`matmul`; matmul_f32_blocks is the
               same product accumulated in fp32 in another order: the spread that rounding flips cause)
  the rest     bias add, relu, the residual x += out + b, the stage cost (fp32 x_t, u_t, goal) and the terminal
               w2 |y|^2 of the fp32, unrounded output of the last cost layer: the oracle's fp32 arithmetic

Everything else of the three solvers is cem_ref's, mppi_ref's and icem_ref's: bf16_costs() makes them cost their samples
here (they all go through cem_ref.sample_costs); their final rollout stays the oracle's fp32 one, as in the library."""

import contextlib

import numpy as np

import cem_ref
import gan_mpc_oracle as orc


def round_bf16(a):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32; on the bit pattern: add 0x7FFF + the lowest kept
    bit, clear the low half.  A NaN stays the NaN it was; the largest finite values round to inf."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32)
    return np.where(np.isnan(a), a, r.view(np.float32))


def matmul_f64(a, W):
    """The product of bf16-valued fp32 operands, accumulated in fp64, rounded once to fp32."""
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) @ W.astype(np.float64)).astype(np.float32)


def matmul_f32_blocks(a, W, block=32):
    """The same product accumulated in fp32: blocks of `block` along k, last block first."""
    K = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (W.shape[1],), np.float32)
    with np.errstate(all="ignore"):
        for k0 in reversed(range(0, K, block)):
            acc = acc + a[..., k0:k0 + block] @ W[k0:k0 + block]
    return acc


def _mlp(layers_q, q, matmul, seen):
    """relu MLP on rounded weights layers_q; -> the fp32 output.  seen: a list that receives every operand's largest
    magnitude."""
    for i, (Wq, b) in enumerate(layers_q):
        a = round_bf16(q)
        if seen is not None:
            seen.append(float(np.max(np.abs(a), initial=0.0)))
        with np.errstate(all="ignore"):
            q = matmul(a, Wq) + b
        if i < len(layers_q) - 1:
            q = np.maximum(q, np.float32(0))
    return q


def sample_costs(pb, samples, matmul=matmul_f64, seen=None):
    """The bf16-mode cost of every sample: samples (B, N, T, m) -> (B, N) fp32; pb: the fp32 problem."""
    B, N, T, m = samples.shape
    f32 = lambda layers: [(np.asarray(W, np.float32), np.asarray(b, np.float32)) for W, b in layers]
    dyn = [(round_bf16(W), b) for W, b in f32(pb["dyn"])]
    cmlp = [(round_bf16(W), b) for W, b in f32(pb["cmlp"])]
    U = np.asarray(samples, np.float32).reshape(B * N, T, m)
    x0 = np.repeat(np.asarray(pb["x0"], np.float32), N, axis=0)
    goal = np.repeat(np.asarray(pb["goal"], np.float32), N, axis=0)
    X = np.empty((B * N, T + 1, x0.shape[-1]), np.float32)
    X[:, 0] = x0
    with np.errstate(all="ignore"):
        for t in range(T):
            X[:, t + 1] = _mlp(dyn, np.concatenate([X[:, t], U[:, t]], axis=-1), matmul, seen) + X[:, t]
        w = orc.sigmoid(np.asarray(pb["mpc_w"], np.float32))
        c = np.empty((B * N, T + 1), np.float32)
        c[:, :T] = orc.stage_cost(X[:, :T], U, goal[:, :T], w)
        y = _mlp(cmlp, X[:, T], matmul, seen)
        c[:, T] = w[2] * np.sum(y * y, -1)
        return np.sum(c, axis=1).reshape(B, N)


@contextlib.contextmanager
def bf16_costs(matmul=matmul_f64):
    """Inside: cem_ref.cem, mppi_ref.mppi and icem_ref.icem (run in fp32) cost their samples in bf16 mode."""
    saved = cem_ref.sample_costs
    cem_ref.sample_costs = lambda pb, samples: sample_costs(pb, samples, matmul)
    try:
        yield
    finally:
        cem_ref.sample_costs = saved
