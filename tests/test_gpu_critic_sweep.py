"""The critic step (critic_loss_grad, critic_score_vjp) over every dispatch cell of critic_forward_backward against the
fp64 oracle: the register-weight kernels of gmpc_critic_lstm.hip at each x width NX (exact and padded), short and
long sequences, batches around the backward sweep's groups and the head's 8-row workgroups, the run-time-n F = 64
kernels and the generic-F kernels of gmpc_critic.hip (routes "gen1", "generic"), the wide-input GEMMs, head widths
that leave a wave with one neuron and the deepest head.  The case table and the route mirror are
tests/critic_cases.py (checked without a GPU by tests/test_critic_cases.py).

Then bit-for-bit: an engine reused with a smaller batch after a larger one against a fresh engine, the side-stream
schedule against everything on the caller's stream, and two identical calls."""

import numpy as np
import pytest

import critic_cases as cc
import gan_mpc_oracle as orc
import gpu_util as gu

pytestmark = pytest.mark.gpu


def _small_problem(n, F, T, B, head, seed):
    return orc.make_problem(n, 1, T, B, seed=seed, dtype=np.float32, dyn_hidden=(8,), cost_hidden=(8,), cost_fout=2,
                            lstm_features=F, head_hidden=head, bias_scale=0.1)


def _critic_step(eng, crit, xseq, label, xs):
    """Both calls of the critic step; numpy copies of (loss_sum, grad_sum, score, dx)."""
    d = eng.to_dev
    ls, gs = eng.critic_loss_grad(d(xseq), d(label), crit)
    score, dx = eng.critic_score_vjp(d(xs), crit)
    return [a.cpu().numpy() for a in (ls, gs, score, dx)]


def _assert_same_bits(a, b, what):
    for name, x, y in zip(("loss_sum", "grad_sum", "score", "dx"), a, b):
        assert np.isfinite(x).all(), f"{what}: {name} not finite"
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (
            f"{what}: {name} differs in {int((x != y).sum())} of {x.size} entries")


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_critic_sweep(case):
    n, F, T, Bc, head, _ = case
    pb, xseq, label, xs = cc.make_case(case)
    pb64 = orc.cast_problem(pb, np.float64)
    cr, cr64 = pb["critic"], pb64["critic"]
    gu.set_config(f"critic sweep {cc.case_id(case)}")
    x64, xs64 = xseq.astype(np.float64), xs.astype(np.float64)
    # the fp32 comparison is valid: no saturated sigmoid, no head row at a relu kink
    for x in (x64, xs64):
        assert np.abs(orc.critic_forward(cr64, x)).max() < cc.SCORE_MAX
        assert not cc.head_kinks(cr64, x).any(), "a head row sits at a relu kink"
    eng = gu.engine_for(pb)
    assert eng.max_batch == (Bc + 1) // 2
    try:
        loss, grad, score, dx = _critic_step(eng, eng.to_dev(gu.critic_flat(pb)), xseq, label, xs)
    finally:
        eng.close()
    # critic_loss_grad: sums over the Bc sequences; the oracle's loss and gradient are means
    l32, g32 = orc.critic_loss_and_grad(cr, xseq, label)
    l64, g64 = orc.critic_loss_and_grad(cr64, x64, label.astype(np.float64))
    gu.assert_parity("critic loss", loss / Bc, l32, l64)
    p32, p64 = gu.pack_grads_critic(g32), gu.pack_grads_critic(g64)
    gu.assert_parity("critic grad", grad / Bc, p32, p64)
    # per block, so that a wrong b or a wrong Wx at n = 1 is not hidden under the Wh / head entries.  The max-norm
    # rule keeps its default bar; the elementwise rule's bar also admits 4 x the fp64 result's own change under a
    # one-ulp perturbation of the inputs (critic_cases.sensitivity), as the bilevel end-to-end check does: single small
    # entries of a block are that ill-conditioned, whatever computes them
    sens = cc.sensitivity(case)
    dims = (F,) + tuple(head) + (1,)
    blocks = [gu.split_critic_flat(v, n, F, dims) for v in (grad / Bc, p32, p64)]
    for (name, a), (_, b32), (_, b64) in zip(*blocks):
        gu.assert_parity(f"critic grad {name}", a, b32, b64, el_tol=max(1e-3, 4 * sens[name]))
    # critic_score_vjp: the score and d score / d x (generator_loss_grad_x is d(-score)/dx)
    gu.assert_parity("score", score, orc.critic_forward(cr, xs), orc.critic_forward(cr64, xs64))
    gx32, gx64 = orc.generator_loss_grad_x(cr, xs), orc.generator_loss_grad_x(cr64, xs64)
    gu.assert_parity("dscore/dx", -dx, gx32, gx64, el_tol=max(1e-3, 4 * sens["dx"]))
    # the first and the last step are the sweeps' special steps (prefetch set-up, the image of the last step)
    gu.assert_parity("dscore/dx t=0", -dx[:, 0], gx32[:, 0], gx64[:, 0], el_tol=max(1e-3, 4 * sens["dx t=0"]))
    gu.assert_parity("dscore/dx t=T1-1", -dx[:, -1], gx32[:, -1], gx64[:, -1],
                     el_tol=max(1e-3, 4 * sens["dx t=T1-1"]))


# one case per route: (n, F, T, head)
ROUTE_CASES = {
    "gen2": (17, 64, 4, (65,)),
    "gen1": (40, 64, 3, (129,)),
    "generic": (5, 100, 3, (65,)),
    "wide": (193, 64, 2, (100,)),
}


def _batches(n, T, sizes, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for Bc in sizes:
        x = rng.standard_normal((Bc, T + 1, n)).astype(np.float32)
        lab = np.where(rng.permutation(Bc) % 2 == 0, 1.0, -1.0).astype(np.float32)
        out[Bc] = (x, lab, rng.standard_normal((Bc, T + 1, n)).astype(np.float32))
    return out


@pytest.mark.parametrize("route", list(ROUTE_CASES))
def test_engine_reuse_with_a_smaller_batch(route):
    """Every saved buffer is sized for 2 max_batch sequences: after Bc = 2 max_batch, a smaller Bc on other data must
    read none of the stale rows past it -- the same bits as a fresh engine that only ever ran the smaller Bc."""
    n, F, T, head = ROUTE_CASES[route]
    assert cc.critic_route(n, F)[0] == route
    M = 9
    pb = _small_problem(n, F, T, M, head, seed=70)
    gu.set_config(f"critic reuse {route} n={n} F={F} T={T} max_batch={M}")
    data = _batches(n, T, (2 * M, 9, 3), seed=71)
    eng = gu.engine_for(pb, max_batch=M)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        _critic_step(eng, crit, *data[2 * M])
        reused = {Bc: _critic_step(eng, crit, *data[Bc]) for Bc in (9, 3)}
    finally:
        eng.close()
    for Bc in (9, 3):
        fresh = gu.engine_for(pb, max_batch=M)
        try:
            ref = _critic_step(fresh, fresh.to_dev(gu.critic_flat(pb)), *data[Bc])
        finally:
            fresh.close()
        _assert_same_bits(reused[Bc], ref, f"Bc={Bc} after Bc={2 * M}")


@pytest.mark.parametrize("n,Bc", [(3, 4), (3, 9), (32, 3), (32, 8)])
def test_side_stream_schedule_changes_no_bit(n, Bc, monkeypatch):
    """The register-weight critic step runs the head transposes, the head weight gradients and the loss sum on a side
    stream; GMPC_CRITIC_SIDE=0 (read on every call) puts everything on the caller's stream.  NX 4 and 32, one and two
    groups per workgroup of the backward sweep."""
    T, head = 5, (129, 65)
    assert cc.critic_route(n, 64)[0] == "gen2"
    pb = _small_problem(n, 64, T, (Bc + 1) // 2, head, seed=80 + n)
    gu.set_config(f"critic side stream n={n} Bc={Bc}")
    x, lab, xs = _batches(n, T, (Bc,), seed=81)[Bc]
    eng = gu.engine_for(pb)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        monkeypatch.delenv("GMPC_CRITIC_SIDE", raising=False)
        side = _critic_step(eng, crit, x, lab, xs)
        monkeypatch.setenv("GMPC_CRITIC_SIDE", "0")
        one = _critic_step(eng, crit, x, lab, xs)
    finally:
        eng.close()
    _assert_same_bits(one, side, "GMPC_CRITIC_SIDE=0 against the side stream")


@pytest.mark.parametrize("route", list(ROUTE_CASES))
def test_repeated_critic_step_gives_the_same_bits(route):
    n, F, T, head = ROUTE_CASES[route]
    Bc = 7
    pb = _small_problem(n, F, T, (Bc + 1) // 2, head, seed=90)
    gu.set_config(f"critic repeat {route} n={n} F={F} T={T} Bc={Bc}")
    x, lab, xs = _batches(n, T, (Bc,), seed=91)[Bc]
    eng = gu.engine_for(pb)
    try:
        crit = eng.to_dev(gu.critic_flat(pb))
        a = _critic_step(eng, crit, x, lab, xs)
        b = _critic_step(eng, crit, x, lab, xs)
    finally:
        eng.close()
    _assert_same_bits(a, b, "two identical calls")
