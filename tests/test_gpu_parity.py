"""GPU parity: every C-ABI entry point against the oracle on the same seeded inputs.

The bar (BASELINE.json north_star): 1e-5 relative fp32.  The fp64 oracle is the arbiter; where a
chained fp32 computation cannot itself reach 1e-5 (the oracle's own fp32 run shows that), HIP must
be no worse than 4x the oracle's fp32 error (see gpu_util.assert_parity)."""

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import gpu_util as gu

pytestmark = pytest.mark.gpu

SHAPES = {
    # name: (n, m, T, B, kwargs)
    "tiny-ragged": (5, 2, 8, 7, dict(dyn_hidden=(33, 47), cost_hidden=(24,), cost_fout=6)),
    "c1-pendulum": (3, 1, 20, 32, {}),
    "c2-cheetah": (17, 6, 50, 48, {}),
    "trained-like": (17, 6, 50, 32, dict(out_scale=0.1)),
    # the register-weight MFMA rollout (three hidden layers of 200) off its headline shape: n + m = 31 (the
    # 8-group layer-0 instantiation), 4 m > 32 (controls without the one-step-ahead operands), T > 64 (two
    # chunks of the after-the-horizon cost pass), batch not a multiple of the 4 slots of a workgroup
    "rw-wide-io": (22, 9, 70, 6, dict(out_scale=0.3)),
    "rw-ragged": (17, 6, 9, 7, {}),
    "rw-one-step": (17, 6, 1, 6, {}),          # horizon 1: the first step is the last one
    # the two-wave Riccati sweep's double buffering (t & 1) and one-step-ahead helper wave: each buffer used once
    # (T 2), an odd horizon that wraps the buffers (T 3); at T 1 nothing is prepared inside the loop
    "rw-two-steps": (17, 6, 2, 3, {}),
    "rw-three-steps": (17, 6, 3, 3, {}),
    # the 128- and 64-wide instantiations of the register-weight rollout / line search (round 3; the Jacobian chain
    # has its regs<4, 64> / regs<2, 32> forms for them): waves 2-3 / 1-3 of the workgroup hold no neuron
    "rw-128": (9, 3, 12, 10, dict(dyn_hidden=(128, 128, 128), cost_hidden=(32,), cost_fout=4, out_scale=0.3)),
    "rw-64": (6, 2, 9, 7, dict(dyn_hidden=(64, 64, 64), cost_hidden=(16,), cost_fout=3, out_scale=0.3)),
    # the 16-candidate form of the line search (gmpc_ls16.hip; the tests force it with GMPC_LS16_SPLIT=1): a
    # last workgroup with unused candidates, the three instantiations (layer-0 k-steps 4 / 6, one or two row
    # blocks of the output layer)
    "ls16-ragged": (17, 6, 9, 21, dict(out_scale=0.3)),
    # (round 4) the 128- and 64-wide instantiations of k_ls16: 8 / 4 full row blocks, no K-split block
    "ls16-h128": (9, 3, 12, 18, dict(dyn_hidden=(128, 128, 128), cost_hidden=(32,), cost_fout=4, out_scale=0.3)),
    "ls16-h128-n17": (17, 6, 8, 20, dict(dyn_hidden=(128, 128, 128), cost_hidden=(64, 64), cost_fout=6, out_scale=0.3)),
    "ls16-h64": (6, 2, 9, 19, dict(dyn_hidden=(64, 64, 64), cost_hidden=(16,), cost_fout=3, out_scale=0.3)),
    "ls16-n12": (12, 4, 7, 18, dict(out_scale=0.3)),
    "ls16-n14m8": (14, 8, 5, 17, dict(out_scale=0.3)),
    "wide": (40, 9, 6, 5, dict(dyn_hidden=(256, 64), cost_hidden=(256, 100), cost_fout=32)),
    # equal-width hidden layers of 128 / 64: the other instantiations of the register-resident chain
    "regs-128": (9, 3, 7, 11, dict(dyn_hidden=(128, 128), cost_hidden=(32,), cost_fout=4)),
    "regs-64": (6, 2, 5, 9, dict(dyn_hidden=(64, 64, 64), cost_hidden=(16,), cost_fout=3)),
    # n > 64: the step-major large-state backward pass (gmpc_large.hip)
    "big-70": (70, 7, 6, 5, dict(dyn_hidden=(128, 96), cost_hidden=(64,), cost_fout=12, out_scale=0.3)),
    # control counts that land in the 8- and 16-block instantiations of the matrix-pipe gain solve with rows to
    # spare (big_solve_mfma<8>: m = 30 of 32; <16>: m = 41 of 64)
    "big-m30": (72, 30, 4, 3, dict(dyn_hidden=(96, 80), cost_hidden=(48,), cost_fout=8, out_scale=0.3)),
    "big-m41": (90, 41, 3, 3, dict(dyn_hidden=(96, 80), cost_hidden=(48,), cost_fout=8, out_scale=0.3)),
    # n <= 64 with more than 32 controls (round 4): the step-major pipeline as well (the fused small-state kernels
    # are built for m <= 32)
    "m40-n24": (24, 40, 5, 4, dict(dyn_hidden=(64, 48), cost_hidden=(32,), cost_fout=6, out_scale=0.3)),
    "m64-n10": (10, 64, 4, 3, dict(dyn_hidden=(96, 80), cost_hidden=(24,), cost_fout=5, out_scale=0.3)),
    "c4-humanoid": (376, 17, 4, 3, dict(out_scale=0.3)),
    "c5-synthetic": (1024, 64, 3, 2, dict(out_scale=0.3)),
    # last hidden width h < n / 2: the large-state pass runs on the low-rank form A = I + W_L^T Vx^T (gmpc_large.hip)
    # -- one, two and three hidden layers (the factor V^T is built differently for each)
    "lowrank-1h": (90, 4, 5, 4, dict(dyn_hidden=(30,), cost_hidden=(48,), cost_fout=6, out_scale=0.3)),
    "lowrank-2h": (150, 5, 5, 4, dict(dyn_hidden=(48, 40), cost_hidden=(64,), cost_fout=8, out_scale=0.3)),
    "lowrank-3h": (130, 3, 4, 3, dict(dyn_hidden=(40, 36, 33), cost_hidden=(32,), cost_fout=5, out_scale=0.3)),
    # the LSTM dynamics variant (reference dynamics/nn.py:37-57): the state xc = [x, c, h] has n + 2F entries --
    # 4 + 12 = 16 (small-state path) and 17 + 64 = 81 (step-major large-state path); goals keep n columns
    "dynl-small": (4, 2, 7, 6, dict(dyn_lstm=6, dyn_hidden=(12,), cost_hidden=(16,), cost_fout=4, out_scale=0.5)),
    "dynl-two-layers": (5, 3, 6, 5, dict(dyn_lstm=8, dyn_hidden=(20, 14), cost_hidden=(16,), cost_fout=4,
                                         out_scale=0.25)),
    "dynl-dense-only": (3, 1, 5, 4, dict(dyn_lstm=5, dyn_hidden=(), cost_hidden=(8,), cost_fout=3)),
    "dynl-big": (17, 6, 8, 5, dict(dyn_lstm=32, dyn_hidden=(64, 64), cost_hidden=(64,), cost_fout=8,
                                   out_scale=0.3)),
}


# more shapes for the line-search kernels only (test_linesearch_16_candidate_form)
LS_SHAPES = {
    "ls16-pendulum": (3, 1, 20, 40, dict(out_scale=0.3)),      # one control, one layer-0 k-step of real rows
    "ls16-m8": (8, 8, 30, 16, dict(out_scale=0.3)),            # every thread of the controls phase owns a pair
}


def _setup(name, critic=False, **over):
    n, m, T, B, kw = SHAPES[name] if name in SHAPES else LS_SHAPES[name]
    kw = dict(kw)
    kw.update(over)
    pb = gu.problem(n, m, T, B, seed=11, **kw)
    gu.set_config(f"{name} n={pb['n']} m={m} T={T} B={B}")
    pb64 = orc.cast_problem(pb, np.float64)
    eng = gu.engine_for(pb, critic=critic)
    return pb, pb64, eng


@pytest.mark.parametrize("name", list(SHAPES))
def test_rollout_cost(name):
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    X, costs = eng.rollout_cost(d(pb["x0"]), d(pb["U"]), d(pb["goal"]))
    X32 = orc.rollout(pb["dyn"], pb["U"], pb["x0"])
    X64 = orc.rollout(pb64["dyn"], pb64["U"], pb64["x0"])
    gu.assert_parity("X", X.cpu().numpy(), X32, X64)
    c32 = orc.evaluate(pb["cmlp"], pb["mpc_w"], pb["goal"], X32, pb["U"])
    c64 = orc.evaluate(pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X64, pb64["U"])
    gu.assert_parity("costs", costs.cpu().numpy(), c32, c64)


def test_rollout_batch_not_multiple_of_block():
    """ragged batch: B = 1 and B = 5 (workgroups own 4 trajectories)."""
    pb, pb64, eng = _setup("tiny-ragged")
    d = eng.to_dev
    X64 = orc.rollout(pb64["dyn"], pb64["U"], pb64["x0"])
    for B in (1, 5):
        X, _ = eng.rollout_cost(d(pb["x0"][:B]), d(pb["U"][:B]), d(pb["goal"][:B]))
        assert gu.rel_err(X.cpu().numpy(), X64[:B]) < 1e-5


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("after_rollout", [False, True])
def test_lqr_backward(name, after_rollout):
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    T = pb["T"]
    if after_rollout:
        Xd, _ = eng.rollout_cost(d(pb["x0"]), d(pb["U"]), d(pb["goal"]))
        X = Xd.cpu().numpy()
    else:
        X = orc.rollout(pb["dyn"], pb["U"], pb["x0"])
        Xd = d(X)
    out = eng.lqr_backward(Xd, d(pb["U"]), d(pb["goal"]), after_rollout=after_rollout)
    # both oracles linearise at the SAME trajectory the kernel saw
    X64 = X.astype(np.float64)
    lqr32 = orc.get_lqr_params(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], X, pb["U"])
    lqr64 = orc.get_lqr_params(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X64, pb64["U"])
    B, n, m = pb["B"], pb["n"], pb["m"]
    bad_s = gu.dyn_near_kink(pb64["dyn"], X64, pb64["U"])
    bad_s[:, -1] |= gu.near_kink(pb64["cmlp"], X64[:, T])
    ok_b = ~bad_s.any(axis=1)
    assert ok_b.sum() >= B // 2, "too many trajectories near a relu kink; change the seed"
    AB32 = np.concatenate([lqr32[5][:, :T], lqr32[6][:, :T]], -1)
    AB64 = np.concatenate([lqr64[5][:, :T], lqr64[6][:, :T]], -1)
    ok_s = ~bad_s
    if not eng.big:
        AB = out["AB"].cpu().numpy()
        gu.assert_parity("AB", AB[ok_s], AB32[ok_s], AB64[ok_s])
    else:   # step-major pass: only the Jacobians of the last processed step (t = 0) are left
        AB = eng.debug_buffer(5, (B, n, n + m)).cpu().numpy()
        gu.assert_parity("AB[t=0]", AB[ok_s[:, 0]], AB32[:, 0][ok_s[:, 0]], AB64[:, 0][ok_s[:, 0]])
    K32, k32, _, _ = orc.tvlqr(*lqr32)
    K64, k64, _, _ = orc.tvlqr(*lqr64)
    g32, a32 = orc.adjoint(lqr32[5], lqr32[6], lqr32[1], lqr32[3])
    g64, a64 = orc.adjoint(lqr64[5], lqr64[6], lqr64[1], lqr64[3])
    gu.assert_parity("grad", out["grad"].cpu().numpy()[ok_b], g32[ok_b], g64[ok_b])
    gu.assert_parity("adjoints", out["adjoints"].cpu().numpy()[ok_b], a32[ok_b], a64[ok_b])
    gu.assert_parity("K", out["K"].cpu().numpy()[ok_b], K32[ok_b], K64[ok_b], ceiling=gu.GAIN_CEILING)
    gu.assert_parity("k", out["k"].cpu().numpy()[ok_b], k32[ok_b], k64[ok_b], ceiling=gu.GAIN_CEILING)
    gu.assert_gain_backward_error([a[ok_b] for a in lqr64], out["K"].cpu().numpy()[ok_b],
                                  out["k"].cpu().numpy()[ok_b], K32[ok_b], k32[ok_b])


@pytest.mark.parametrize("name,head", [("tiny-ragged", (12,)), ("c2-cheetah", ()),
                                       ("c2-cheetah", (256, 256, 256)), ("big-70", (32,)),
                                       ("c4-humanoid", (256, 256, 256))])
def test_critic_loss_grad(name, head):
    pb, pb64, eng = _setup(name, critic=True, head_hidden=head)
    d = eng.to_dev
    B = pb["B"]
    rng = np.random.default_rng(5)
    xseq = np.concatenate([pb["true_seq"], pb["goal"]], 0)          # 2B sequences
    label = np.concatenate([np.ones(B), -np.ones(B)]).astype(np.float32)
    perm = rng.permutation(2 * B)
    xseq, label = xseq[perm], label[perm]
    ls, gs = eng.critic_loss_grad(d(xseq), d(label), d(gu.critic_flat(pb)))
    l32, g32 = orc.critic_loss_and_grad(pb["critic"], xseq, label)
    l64, g64 = orc.critic_loss_and_grad(pb64["critic"], xseq.astype(np.float64), label.astype(np.float64))
    gu.assert_parity("critic loss", ls.cpu().numpy() / (2 * B), l32, l64)
    gu.assert_parity("critic grad", gs.cpu().numpy() / (2 * B), gu.pack_grads_critic(g32),
                     gu.pack_grads_critic(g64))


@pytest.mark.parametrize("F,n,head,Bq", [(32, 17, (64, 64), 11), (128, 17, (256,), 9), (24, 5, (), 6), (128, 300, (32,), 5)])
def test_critic_other_lstm_feature_counts(F, n, head, Bq):
    """critic.lstm.lstm_features is a yaml integer in the reference (critic/nn.py:10-14, config/
    gan_hyperparameters.yaml:60-65; its expert model uses 128): 64 runs the register-weight kernels, every other count
    up to 128 the strided k_lstm_fwd_g / k_lstm_bwd_g -- the critic step (loss, BPTT, weight gradients), the score and
    its input gradient (the generator loss's path), ragged batch; (128, 300): the wide-input form, x Wx as a GEMM."""
    m, T = 3, 9
    pb = orc.make_problem(n, m, T, Bq, seed=40 + F, dtype=np.float32, dyn_hidden=(16, 16), cost_hidden=(12,), cost_fout=4,
                          lstm_features=F, head_hidden=head, bias_scale=0.1)
    pb64 = orc.cast_problem(pb, np.float64)
    gu.set_config(f"critic F={F} n={n} T={T} B={Bq} head={head}")
    eng = gu.engine_for(pb)
    d = eng.to_dev
    try:
        xseq = np.concatenate([pb["true_seq"], pb["goal"]], 0)
        rng = np.random.default_rng(F)
        label = np.where(rng.random(2 * Bq) > 0.5, 1.0, -1.0).astype(np.float32)
        crit = d(gu.critic_flat(pb))
        ls, gs = eng.critic_loss_grad(d(xseq), d(label), crit)
        l32, g32 = orc.critic_loss_and_grad(pb["critic"], xseq, label)
        l64, g64 = orc.critic_loss_and_grad(pb64["critic"], xseq.astype(np.float64), label.astype(np.float64))
        gu.assert_parity("critic loss", ls.cpu().numpy() / (2 * Bq), l32, l64)
        gu.assert_parity("critic grad", gs.cpu().numpy() / (2 * Bq), gu.pack_grads_critic(g32), gu.pack_grads_critic(g64))
        score, dx = eng.critic_score_vjp(d(pb["true_seq"]), crit)
        gu.assert_parity("score", score.cpu().numpy(), orc.critic_forward(pb["critic"], pb["true_seq"]),
                         orc.critic_forward(pb64["critic"], pb["true_seq"].astype(np.float64)))
        gu.assert_parity("dscore/dx", -dx.cpu().numpy(), orc.generator_loss_grad_x(pb["critic"], pb["true_seq"]),
                         orc.generator_loss_grad_x(pb64["critic"], pb["true_seq"].astype(np.float64)))
    finally:
        eng.close()


def test_critic_loss_grad_odd_row_count():
    """An odd number of sequences times an odd T + 1: the weight-gradient GEMMs see an odd row count (81 rows,
    chunks of 64), i.e. the clamped last k-step of k_wgrad_batch's 16-byte operand loads."""
    pb, pb64, eng = _setup("tiny-ragged", critic=True, head_hidden=(128,))
    d = eng.to_dev
    rng = np.random.default_rng(9)
    xseq = np.concatenate([pb["true_seq"], pb["goal"]], 0)[:9]      # 9 sequences x (T + 1 = 9) rows
    label = np.where(rng.random(9) > 0.5, 1.0, -1.0).astype(np.float32)
    ls, gs = eng.critic_loss_grad(d(xseq), d(label), d(gu.critic_flat(pb)))
    l32, g32 = orc.critic_loss_and_grad(pb["critic"], xseq, label)
    l64, g64 = orc.critic_loss_and_grad(pb64["critic"], xseq.astype(np.float64), label.astype(np.float64))
    gu.assert_parity("critic loss", ls.cpu().numpy() / 9, l32, l64)
    gu.assert_parity("critic grad", gs.cpu().numpy() / 9, gu.pack_grads_critic(g32), gu.pack_grads_critic(g64))


@pytest.mark.parametrize("name", ["c2-cheetah", "c4-humanoid"])
def test_critic_score_vjp(name):
    """c4-humanoid: n + F > 256, the input projection and dx run as MFMA GEMMs around the LSTM."""
    pb, pb64, eng = _setup(name, critic=True)
    d = eng.to_dev
    xs = pb["true_seq"]
    score, dx = eng.critic_score_vjp(d(xs), d(gu.critic_flat(pb)))
    s32 = orc.critic_forward(pb["critic"], xs)
    s64 = orc.critic_forward(pb64["critic"], xs.astype(np.float64))
    gu.assert_parity("score", score.cpu().numpy(), s32, s64)
    # generator_loss_grad_x is d(-score)/dx
    gu.assert_parity("dscore/dx", -dx.cpu().numpy(), orc.generator_loss_grad_x(pb["critic"], xs),
                     orc.generator_loss_grad_x(pb64["critic"], xs.astype(np.float64)))


def test_adam_clip_step():
    pb, _, eng = _setup("tiny-ragged")
    rng = np.random.default_rng(2)
    cnt = 20109
    p = rng.standard_normal(cnt).astype(np.float32)
    m = np.zeros(cnt, np.float32)
    v = np.zeros(cnt, np.float32)
    pd, md, vd = eng.to_dev(p), eng.to_dev(m), eng.to_dev(v)
    p64, m64, v64 = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for step in range(1, 4):
        # step 2 has a huge gradient so the global-norm clip is active
        g = (rng.standard_normal(cnt) * (1e3 if step == 2 else 1.0)).astype(np.float32)
        eng.adam_clip_step(pd, eng.to_dev(g), md, vd, step, lr=1e-3, grad_scale=0.5)
        p, m, v = orc.adam_clip_step(p, 0.5 * g, m, v, step, 1e-3)
        p64, m64, v64 = orc.adam_clip_step(p64, 0.5 * g.astype(np.float64), m64, v64, step, 1e-3)
        gu.assert_parity(f"adam p step {step}", pd.cpu().numpy(), p, p64)
        gu.assert_parity(f"adam m step {step}", md.cpu().numpy(), m, m64)
        gu.assert_parity(f"adam v step {step}", vd.cpu().numpy(), v, v64)


@pytest.mark.parametrize("name", ["tiny-ragged", "trained-like", "big-70", "rw-wide-io", "rw-ragged", "rw-one-step",
                                  "rw-128", "rw-64", "m40-n24",
                                  "dynl-small", "dynl-two-layers", "dynl-big", "lowrank-2h"])
def test_ilqr_single_iteration_teacher_forced(name):
    """maxiter=1 from the same start: tvlqr + line search + re-linearisation, one iteration."""
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    kw = {"maxiter": 1}
    out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
    r32 = orc.ilqr(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], pb["x0"], pb["U"], kw)
    r64 = orc.ilqr(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], pb64["x0"], pb64["U"], kw)
    it = out["iterations"].cpu().numpy()
    np.testing.assert_array_equal(it, r64[6])
    # trajectories whose accepted step size agrees between fp32 and fp64 oracles (a line-search
    # branch decided by the last bit is not a parity failure)
    same = np.isclose(r32[2], r64[2], rtol=1e-3)
    assert same.mean() > 0.7
    gu.assert_parity("U", out["U"].cpu().numpy()[same], r32[1][same], r64[1][same], tol=1e-4, ceiling=gu.GAIN_CEILING)
    gu.assert_parity("X", out["X"].cpu().numpy()[same], r32[0][same], r64[0][same], tol=1e-4, ceiling=gu.GAIN_CEILING)
    gu.assert_parity("obj", out["obj"].cpu().numpy()[same], r32[2][same], r64[2][same], tol=1e-4, ceiling=gu.GAIN_CEILING)


@pytest.fixture
def wide_linesearch(monkeypatch):
    """every work list goes to k_ls16 (by default only those of 1537 candidates and more do)"""
    monkeypatch.setenv("GMPC_LS16_SPLIT", "1")
    monkeypatch.delenv("GMPC_LS", raising=False)


@pytest.mark.parametrize("name", ["ls16-ragged", "ls16-n12", "ls16-n14m8", "ls16-pendulum", "ls16-m8",
                                  "trained-like", "rw-one-step", "ls16-h128", "ls16-h128-n17", "ls16-h64"])
def test_linesearch_16_candidate_form(name, wide_linesearch, monkeypatch):
    """k_ls16 against the oracle's loop (two iterations: the second line search starts from masks, states and
    controls the first one committed) and against k_traj_rw<true> on the same problem."""
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    # (the other shapes: the second iteration is past the 4x rule for BOTH forms alike, n14m8 3.3e-3 against the
    # fp32 oracle's 5e-4 -- its gains, not the rollouts)
    kw = {"maxiter": 2 if name in ("ls16-ragged", "ls16-n12") else 1}
    out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
    n16 = eng.linesearch_candidates()
    r32 = orc.ilqr(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], pb["x0"], pb["U"], kw)
    r64 = orc.ilqr(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], pb64["x0"], pb64["U"], kw)
    np.testing.assert_array_equal(out["iterations"].cpu().numpy(), r64[6])
    same = np.isclose(r32[2], r64[2], rtol=1e-3)
    assert same.mean() > 0.7
    for key, j in (("U", 1), ("X", 0), ("obj", 2)):
        gu.assert_parity(f"ls16 {key}", out[key].cpu().numpy()[same], r32[j][same], r64[j][same], tol=1e-4,
                         ceiling=gu.GAIN_CEILING)
    # the masks the accepted candidates wrote: Jacobians and gradient of the solve at ITS iterate against the
    # oracles' at the same (X, U), away from the relu kinks
    Xg, Ug = out["X"].cpu().numpy(), out["U"].cpu().numpy()
    B, n, m, T = pb["B"], pb["n"], pb["m"], pb["T"]
    l32 = orc.get_lqr_params(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], Xg, Ug)
    l64 = orc.get_lqr_params(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], Xg.astype(np.float64),
                             Ug.astype(np.float64))
    bad_s = gu.dyn_near_kink(pb64["dyn"], Xg.astype(np.float64), Ug.astype(np.float64))
    bad_s[:, -1] |= gu.near_kink(pb64["cmlp"], Xg[:, T].astype(np.float64))
    ok_b = ~bad_s.any(axis=1)
    assert ok_b.sum() >= B // 2
    AB = eng.debug_buffer(5, (B, T, n, n + m)).cpu().numpy()
    AB32 = np.concatenate([l32[5][:, :T], l32[6][:, :T]], -1)
    AB64 = np.concatenate([l64[5][:, :T], l64[6][:, :T]], -1)
    gu.assert_parity("ls16 AB at the solve's iterate", AB[~bad_s], AB32[~bad_s], AB64[~bad_s])
    g32 = orc.adjoint(l32[5], l32[6], l32[1], l32[3])[0]
    g64 = orc.adjoint(l64[5], l64[6], l64[1], l64[3])[0]
    gu.assert_parity("ls16 grad at the solve's iterate", out["grad"].cpu().numpy()[ok_b], g32[ok_b], g64[ok_b])
    snap = {key: out[key].cpu().numpy().copy() for key in ("U", "X", "obj")}
    monkeypatch.setenv("GMPC_LS", "rw")
    ref = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
    # (the 16-candidate form takes a full first round -- all 8 candidates -- where its pass has room for them, the
    # 4-candidate form one more than was accepted last time and then 4 and 8: the same candidate is accepted, the
    # numbers evaluated on the way differ in either direction)
    assert eng.linesearch_candidates() > 0 and n16 > 0
    for key in ("U", "X", "obj"):
        a, b = snap[key][same], ref[key].cpu().numpy()[same]
        # two fp32 routes through gains of condition ~1e4 (GAIN_CEILING): each is held to the fp64 oracle above
        assert gu.rel_err(a, b.astype(np.float64)) < 1e-3, key


def test_ilqr_converges_on_lq_problem():
    """KAT: linear dynamics (zero hidden->out weights except a linear path is impossible with relu, so
    use zero dynamics weights: x' = x) and the smooth-L2 cost: iLQR must reduce the objective and
    stop; HIP and oracle agree on the optimum."""
    pb, pb64, eng = _setup("tiny-ragged", out_scale=0.05)
    d = eng.to_dev
    out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]))
    obj0 = orc.objective(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], pb64["U"], pb64["x0"])
    r64 = orc.ilqr(pb64["dyn"], pb64["cmlp"], pb64["mpc_w"], pb64["goal"], pb64["x0"], pb64["U"])
    obj = out["obj"].cpu().numpy()
    assert (obj <= obj0 + 1e-6).all()
    # both reached (nearly) the same local optimum value
    assert np.median(np.abs(obj - r64[2]) / np.abs(r64[2])) < 1e-3
    # the returned X is the rollout of the returned U, the objective is its cost
    X64 = orc.rollout(pb64["dyn"], out["U"].cpu().numpy().astype(np.float64), pb64["x0"])
    assert gu.rel_err(out["X"].cpu().numpy(), X64) < 1e-5
    c64 = orc.evaluate(pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X64,
                       out["U"].cpu().numpy().astype(np.float64)).sum(1)
    assert gu.rel_err(obj, c64) < 1e-5


@pytest.mark.parametrize("name", ["c2-cheetah", "rw-one-step", "rw-two-steps", "rw-three-steps"])
def test_riccati_two_wave_form_and_linearize_event(name, monkeypatch):
    """k_riccati_w2 (the default at n=17, m=6) against k_riccati (GMPC_RICCATI=valu) on the same inputs -- each is
    held to the oracle by test_lqr_backward, this pins them to each other --, and gmpc_set_linearize_event: the
    caller's event is recorded inside the backward pass, a second stream that waits for it sees the Jacobians."""
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    Xd, _ = eng.rollout_cost(d(pb["x0"]), d(pb["U"]), d(pb["goal"]))
    ev = torch.cuda.Event()
    ev.record()
    eng.set_linearize_event(ev)
    side = torch.cuda.Stream()
    out = eng.lqr_backward(Xd, d(pb["U"]), d(pb["goal"]), after_rollout=True)
    side.wait_event(ev)
    with torch.cuda.stream(side):
        AB_seen = out["AB"].clone()            # ordered after the Jacobian chain, beside the Riccati sweep
    torch.cuda.synchronize()
    assert ev.query()
    eng.set_linearize_event(None)
    w = {k: out[k].cpu().numpy().copy() for k in ("K", "k", "grad", "adjoints", "AB")}
    np.testing.assert_array_equal(AB_seen.cpu().numpy(), w["AB"])
    monkeypatch.setenv("GMPC_RICCATI", "valu")
    ref = eng.lqr_backward(Xd, d(pb["U"]), d(pb["goal"]), after_rollout=True)
    for k in ("grad", "adjoints"):
        assert gu.rel_err(w[k], ref[k].cpu().numpy().astype(np.float64)) < 1e-5, k
    for k in ("K", "k"):       # gains: two fp32 routes through cond(G) ~ 1e4
        assert gu.rel_err(w[k], ref[k].cpu().numpy().astype(np.float64)) < 1e-3, k


@pytest.mark.parametrize("name", ["big-70", "big-m30", "big-m41", "c4-humanoid", "c5-synthetic", "lowrank-2h"])
def test_gain_solve_matrix_pipe_against_vector_form(name, monkeypatch):
    """k_big_step's gain solve (trajax lqr_step: K, k = -(G + 1e-8 I)^-1 [H, h] by Cholesky substitutions): the
    matrix-pipe form runs the same multiply-subtracts as the vector form kept behind GMPC_BIG_SOLVE=valu (two
    interleaved accumulation chains per row instead of one) -- the gains agree far inside the gains' own fp32
    forward error (1e-3 at these shapes), and the rest of the pass with them."""
    pb, _, eng = _setup(name)
    d = eng.to_dev
    X, _ = eng.rollout_cost(d(pb["x0"]), d(pb["U"]), d(pb["goal"]))
    outs = {}
    for form in ("mfma", "valu"):
        monkeypatch.setenv("GMPC_BIG_SOLVE", form)
        o = eng.lqr_backward(X, d(pb["U"]), d(pb["goal"]), after_rollout=True)
        outs[form] = {k: v.cpu().numpy().astype(np.float64) for k, v in o.items() if k in ("K", "k", "grad", "adjoints")}
    for key in ("K", "k", "grad", "adjoints"):
        a, b = outs["mfma"][key], outs["valu"][key]
        assert np.isfinite(a).all()
        assert gu.rel_err(a, b) < (2e-4 if key in ("K", "k") else 1e-5), (key, gu.rel_err(a, b))


@pytest.mark.parametrize("name,loss_kind", [("trained-like", 0), ("trained-like", 1), ("big-70", 0),
                                            ("big-70", 1), ("c4-humanoid", 0), ("dynl-small", 0),
                                            ("dynl-small", 1), ("dynl-big", 0), ("dynl-big", 1),
                                            ("lowrank-1h", 0), ("lowrank-2h", 1), ("lowrank-3h", 0), ("m40-n24", 0)])
def test_bilevel_grad(name, loss_kind):
    """a8-a11 at the lower-level solution the GPU found.  The Hessian solve is ill-conditioned
    (forward error = cond(A) x backward error), so H is checked by its residual A H - B in fp64;
    the remaining stages are checked stage-by-stage with the GPU's own H, dX as input."""
    pb, pb64, eng = _setup(name, critic=True)
    d = eng.to_dev
    T, n, m = pb["T"], pb["n"], pb["m"]
    out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 3})
    # keep the trajectories whose final iterate has no pre-activation at a relu kink (there the
    # Jacobian is discontinuous and GPU / oracle may legitimately take different sides), then
    # re-linearise exactly those at the solution (maxiter = 0: rollout + backward at the given U)
    Xf = out["X"].cpu().numpy().astype(np.float64)
    Uf = out["U"].cpu().numpy()
    bad = gu.dyn_near_kink(pb64["dyn"], Xf, Uf.astype(np.float64)).any(1) | gu.near_kink(pb64["cmlp"], Xf[:, T])
    ok = ~bad
    assert ok.sum() >= max(1, pb["B"] // 2)
    for p_ in (pb, pb64):
        for key in ("x0", "goal", "true_seq"):
            p_[key] = p_[key][ok]
    B = int(ok.sum())
    out = eng.ilqr_solve(d(pb["x0"]), d(Uf[ok]), d(pb["goal"]), {"maxiter": 0})
    crit = d(gu.critic_flat(pb))
    loss, gsum = eng.bilevel_grad(B, loss_kind, desired=d(pb["true_seq"]), critic=crit, sign=1.0)
    X = out["X"].cpu().numpy()
    U = out["U"].cpu().numpy()
    Hd = eng.debug_buffer(2, (B, T, m)).cpu().numpy()
    dXd = eng.debug_buffer(3, (B, T + 1, n)).cpu().numpy()
    Bvd = eng.debug_buffer(4, (B, T, m)).cpu().numpy()
    gu.check_bilevel_at_iterate(pb, pb64, loss_kind, X, U, loss.cpu().numpy(), gsum.cpu().numpy(), Hd, dXd, Bvd)


@pytest.mark.parametrize("name", ["ls16-ragged", "ls16-n12", "ls16-n14m8", "ls16-pendulum", "ls16-m8", "trained-like",
                                  "c2-cheetah"])
def test_linesearch_two_group_form_is_bit_identical(name, monkeypatch):
    """k_ls32 (two groups of 16 candidates per workgroup, half a step apart, on two teams of four waves; the form long
    work lists run on by default) computes every candidate with k_ls16's operations in k_ls16's order: forced onto
    every work list, a three-iteration solve must return the same bits -- iterate, objective, step sizes, iteration
    counts, candidate count, and the relu masks behind the last Jacobians -- as the solve with k_ls16 on every list."""
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    kw = {"maxiter": 3}
    monkeypatch.setenv("GMPC_LS16_SPLIT", "1")
    monkeypatch.setenv("GMPC_LS", "ls16")
    ref = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
    n16 = eng.linesearch_candidates()
    snap = {key: ref[key].cpu().numpy().copy() for key in ("X", "U", "obj", "grad", "iterations")}
    monkeypatch.delenv("GMPC_LS")
    monkeypatch.setenv("GMPC_LS32_SPLIT", "1")
    out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
    assert eng.linesearch_candidates() == n16
    for key in snap:
        np.testing.assert_array_equal(out[key].cpu().numpy(), snap[key], err_msg=key)
    # and the relu masks the accepted candidates left behind: the Jacobians of the last backward pass
    B, n, m, T = pb["B"], pb["n"], pb["m"], pb["T"]
    AB32 = eng.debug_buffer(5, (B, T, n, n + m)).cpu().numpy()
    monkeypatch.setenv("GMPC_LS", "ls16")
    eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
    np.testing.assert_array_equal(AB32, eng.debug_buffer(5, (B, T, n, n + m)).cpu().numpy())


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_linesearch_two_group_form_is_bit_identical_on_random_shapes(seed, monkeypatch):
    """The same comparison on shapes drawn at random inside k_ls32's limits (n <= 24, m <= 8, n + m <= 24, m n <= 128):
    ragged last groups (batch x candidates not a multiple of 32), both layer-0 depths, one and two output row blocks."""
    rng = np.random.default_rng(1000 + seed)
    while True:
        n, m = int(rng.integers(3, 25)), int(rng.integers(1, 9))
        if n + m <= 24 and m * n <= 128:
            break
    T, B = int(rng.integers(3, 14)), int(rng.integers(5, 40))
    pb = gu.problem(n, m, T, B, seed=seed, out_scale=0.3)
    gu.set_config(f"ls32 random seed={seed} n={n} m={m} T={T} B={B}")
    eng = gu.engine_for(pb, critic=False)
    d = eng.to_dev
    kw = {"maxiter": 3}
    try:
        monkeypatch.setenv("GMPC_LS16_SPLIT", "1")
        monkeypatch.setenv("GMPC_LS", "ls16")
        ref = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
        n16 = eng.linesearch_candidates()
        snap = {key: ref[key].cpu().numpy().copy() for key in ("X", "U", "obj", "grad", "iterations")}
        ab = eng.debug_buffer(5, (B, T, n, n + m)).cpu().numpy().copy()
        monkeypatch.delenv("GMPC_LS")
        monkeypatch.setenv("GMPC_LS32_SPLIT", "1")
        out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
        assert eng.linesearch_candidates() == n16
        for key in snap:
            np.testing.assert_array_equal(out[key].cpu().numpy(), snap[key], err_msg=f"{key} (n={n} m={m} T={T} B={B})")
        np.testing.assert_array_equal(eng.debug_buffer(5, (B, T, n, n + m)).cpu().numpy(), ab)
    finally:
        eng.close()


def test_linesearch_two_group_threshold_never_below_the_16_candidate_forms(monkeypatch):
    """GMPC_LS32_SPLIT=1 alone asks k_ls32 for every work list while k_ls16's threshold stays at 1537: the plan raises
    k_ls32's threshold to k_ls16's, so on this batch (21 x 8 candidates at most) every round is still k_traj_rw's and
    the solve returns the bits of the solve with no variable set.  (Unclamped, k_traj_rw AND k_ls32 evaluated such
    rounds and k_ls32's values -- k_ls16's bits, not k_traj_rw's -- were the ones kept.)"""
    pb, pb64, eng = _setup("ls16-ragged")
    d = eng.to_dev
    kw = {"maxiter": 3}
    for var in ("GMPC_LS", "GMPC_LS16_SPLIT", "GMPC_LS32_SPLIT"):
        monkeypatch.delenv(var, raising=False)
    ref = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
    ncand = eng.linesearch_candidates()
    snap = {key: ref[key].cpu().numpy().copy() for key in ("X", "U", "obj", "grad", "iterations")}
    monkeypatch.setenv("GMPC_LS32_SPLIT", "1")
    out = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), kw)
    assert eng.linesearch_candidates() == ncand
    for key in snap:
        np.testing.assert_array_equal(out[key].cpu().numpy(), snap[key], err_msg=key)


def test_unsupported_shape_fails_loudly():
    from gan_mpc_amd import GmpcError
    from gan_mpc_amd.engine import Engine
    with pytest.raises(GmpcError, match="unsupported shape"):
        Engine(1100, 17, 5, [1117, 200, 200, 200, 1100], [1100, 128, 128, 10], max_batch=2)
    with pytest.raises(GmpcError, match="unsupported shape"):
        Engine(40, 65, 5, [105, 64, 40], [40, 32, 8], max_batch=2)
    with pytest.raises(GmpcError, match="unsupported shape"):       # critic lstm_features above 128
        Engine(5, 2, 5, [7, 16, 5], [5, 8, 4], max_batch=2, lstm_features=192, head_dims=[192, 1])


def test_nan_trajectory_follows_the_trajax_rules_and_is_isolated():
    """A poisoned trajectory (NaN control) has a NaN objective; the continuation test
    `obj_step > obj_step_threshold * (|obj| + 1)` then compares against NaN and is false, so the
    restated trajax loop never starts for it (0 iterations, NaN kept) -- and its neighbours in the
    same workgroup are untouched."""
    pb, pb64, eng = _setup("tiny-ragged", out_scale=0.05)
    d = eng.to_dev
    clean = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 4})
    U = pb["U"].copy()
    U[2, 3, 0] = np.nan
    out = eng.ilqr_solve(d(pb["x0"]), d(U), d(pb["goal"]), {"maxiter": 4})
    with np.errstate(all="ignore"):
        ref = orc.ilqr(pb["dyn"], pb["cmlp"], pb["mpc_w"], pb["goal"], pb["x0"], U, {"maxiter": 4})
    it = out["iterations"].cpu().numpy()
    assert it[2] == ref[6][2] == 0
    assert np.isnan(out["obj"].cpu().numpy()[2])
    keep = np.arange(pb["B"]) != 2
    for key in ("X", "U", "obj"):
        np.testing.assert_array_equal(out[key].cpu().numpy()[keep], clean[key].cpu().numpy()[keep])
    np.testing.assert_array_equal(it[keep], clean["iterations"].cpu().numpy()[keep])


def test_bad_calls_fail_loudly():
    from gan_mpc_amd import GmpcError
    pb, _, eng = _setup("tiny-ragged")
    d = eng.to_dev
    with pytest.raises(GmpcError, match="outside"):
        eng.rollout_cost(d(pb["x0"][:0]), d(pb["U"][:0]), d(pb["goal"][:0]))       # empty batch
    big = np.repeat(pb["x0"], 3, axis=0)
    with pytest.raises(GmpcError, match="outside"):
        eng.rollout_cost(d(big), d(np.repeat(pb["U"], 3, 0)), d(np.repeat(pb["goal"], 3, 0)))
    with pytest.raises(GmpcError, match="must precede"):
        eng.bilevel_grad(3, 0, desired=d(pb["true_seq"][:3]))     # no solve of that batch size yet
    with pytest.raises(GmpcError, match="make_psd"):
        eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"make_psd": True})
    from gan_mpc_amd.engine import Engine
    e2 = Engine(5, 2, 8, [7, 33, 47, 5], [5, 24, 6], max_batch=4)        # created without a critic
    with pytest.raises(GmpcError, match="without a critic"):
        e2.critic_score_vjp(d(pb["true_seq"][:2]), d(np.zeros(8, np.float32)))


@pytest.mark.parametrize("M,N,K,batch", [(376, 376, 376, 3), (17, 376, 376, 2), (376, 17, 17, 2),
                                         (40, 70, 33, 5), (64, 1024, 129, 1),
                                         # the streaming thin-product kernel (k_bthin): wide X / wide Y, rows that
                                         # are not 16-byte aligned, widths that are not multiples of 4 or 128, two
                                         # thin strips, odd K
                                         (376, 17, 376, 3), (17, 393, 376, 3), (130, 5, 33, 7), (7, 131, 35, 6),
                                         (64, 1088, 200, 2), (1024, 64, 200, 2), (33, 257, 21, 4)])
def test_bgemm_tn_matches_float64(M, N, K, batch):
    """building block of the large-state Riccati path: C = alpha X^T Y + beta C"""
    import ctypes as C
    from gan_mpc_amd import _lib
    pb, _, eng = _setup("tiny-ragged")
    rng = np.random.default_rng(4)
    X = rng.standard_normal((batch, K, M)).astype(np.float32)
    Y = np.zeros((batch * K + 8, N), np.float32)           # 8 readable pad rows
    Y[:batch * K] = rng.standard_normal((batch * K, N))
    C0 = rng.standard_normal((batch, M, N)).astype(np.float32)
    Xd, Yd, Cd = eng.to_dev(X), eng.to_dev(Y), eng.to_dev(C0)
    _lib.check(eng.lib.gmpc_bgemm_tn(eng.ctx, batch, M, N, K, C.c_void_p(Xd.data_ptr()),
                                     C.c_void_p(Yd.data_ptr()), C.c_void_p(Cd.data_ptr()), 0.5, -2.0,
                                     eng._stream()))
    Yb = Y[:batch * K].reshape(batch, K, N).astype(np.float64)
    ref = 0.5 * np.einsum("bkm,bkn->bmn", X.astype(np.float64), Yb) - 2.0 * C0
    assert gu.rel_err(Cd.cpu().numpy(), ref) < 1e-5


@pytest.mark.parametrize("name,tf,S", [("tiny-ragged", True, 8), ("tiny-ragged", False, 5),
                                       ("trained-like", True, 50), ("trained-like", False, 50),
                                       ("wide", False, 6), ("c4-humanoid", False, 4), ("c4-humanoid", True, 3),
                                       ("c5-synthetic", False, 3), ("dynl-small", True, 7), ("dynl-small", False, 6),
                                       ("dynl-two-layers", False, 5), ("dynl-big", False, 8)])
def test_dynamics_loss_grad(name, tf, S):
    """N3: batch of multi-step prediction losses + weight gradient (dynamics_trainer.py:14-86)."""
    pb, pb64, eng = _setup(name)
    d = eng.to_dev
    B, n, m = pb["B"], pb.get("nx", pb["n"]), pb["m"]          # the regression runs on x (the LSTM carry starts at 0)
    rng = np.random.default_rng(21)
    xseq = rng.standard_normal((B, S, n)).astype(np.float32)
    useq = np.tanh(rng.standard_normal((B, S, m))).astype(np.float32)
    yseq = rng.standard_normal((B, S, n)).astype(np.float32)
    gamma = 0.95
    ls, gs = eng.dynamics_loss_grad(d(xseq), d(useq), d(yseq), gamma, tf)
    l32, g32 = orc.dynamics_fit_loss_and_grad(pb["dyn"], xseq, useq, yseq, gamma, tf)
    l64, g64 = orc.dynamics_fit_loss_and_grad(pb64["dyn"], xseq.astype(np.float64),
                                              useq.astype(np.float64), yseq.astype(np.float64),
                                              gamma, tf)
    def flat(g):
        if isinstance(g, dict):      # LSTM variant: Wx | Wh | b | the tail's layers
            return np.concatenate([g["Wx"].ravel(), g["Wh"].ravel(), g["b"].ravel()]
                                  + [t.ravel() for Wb in g["tail"] for t in Wb])
        return np.concatenate([t.ravel() for Wb in g for t in Wb])
    gu.assert_parity("dynamics loss", ls.cpu().numpy()[0] / B, l32, l64)
    gu.assert_parity("dynamics grad", gs.cpu().numpy() / B, flat(g32), flat(g64), tol=1e-5)
    from gan_mpc_amd import GmpcError
    with pytest.raises(GmpcError, match="outside"):
        eng.dynamics_loss_grad(d(np.zeros((B, pb["T"] + 1, n), np.float32)),
                               d(np.zeros((B, pb["T"] + 1, m), np.float32)),
                               d(np.zeros((B, pb["T"] + 1, n), np.float32)), gamma, tf)


@pytest.mark.parametrize("name,F,hist,hidden,layers", [("c2-cheetah", 128, 1, 128, 3),
                                                       ("c2-cheetah", 0, 2, 128, 3),
                                                       ("tiny-ragged", 24, 3, 19, 2),
                                                       ("wide", 64, 1, 256, 3),
                                                       ("c4-humanoid", 128, 1, 128, 3),
                                                       ("c5-synthetic", 64, 2, 300, 2),
                                                       ("c4-humanoid", 0, 1, 160, 3)])
def test_expert_rollout(name, F, hist, hidden, layers):
    """N2: goal states / initial controls from the expert sequence model (expert_model.py:60-91)."""
    from gan_mpc_amd import params as P
    from gan_mpc_amd.engine import make_expert_shape
    pb, _, eng = _setup(name)
    B, n, m, T = pb["B"], pb["n"], pb["m"], pb["T"]
    rng = np.random.default_rng(17)
    ex = orc.make_expert(rng, n, m, lstm_features=F, num_layers=layers, num_hidden_units=hidden)
    # trained-like residual head so that 50 free-running steps stay O(1)
    W, b = ex["head_x"][-1]
    ex["head_x"][-1] = ((0.1 * W).astype(np.float32), (0.1 * b).astype(np.float32))
    hx = rng.standard_normal((B, hist + 1, n)).astype(np.float32)
    flat, Fp, dx, du = P.pack_expert(ex)
    goal, U = eng.expert_rollout(eng.to_dev(hx), eng.to_dev(flat), make_expert_shape(Fp, dx, du))
    g32, u32 = orc.expert_goal_states_init_actions(ex, hx, T)
    ex64 = orc.cast_problem(dict(e=ex), np.float64)["e"]
    g64, u64 = orc.expert_goal_states_init_actions(ex64, hx.astype(np.float64), T)
    np.testing.assert_array_equal(goal[:, 0].cpu().numpy(), hx[:, -1])
    gu.assert_parity("goal", goal.cpu().numpy(), g32, g64)
    gu.assert_parity("init_U", U.cpu().numpy(), u32, u64)
    assert np.abs(U.cpu().numpy()).max() <= 1.0
    from gan_mpc_amd import GmpcError
    with pytest.raises(GmpcError, match="history"):
        eng.expert_rollout(eng.to_dev(hx[:, :1]), eng.to_dev(flat), make_expert_shape(Fp, dx, du))


def test_c_abi_exchange_world_of_one():
    """gmpc_allreduce_grads (RCCL bound at run time): without gmpc_comm_init the ctx is a world of one and
    the call is a no-op; with a one-rank communicator the in-place ncclAllReduce(sum) returns the buffer
    unchanged.  (More ranks need more GPUs than the test box has: the N > 1 arithmetic of the exchange is
    covered by tests/test_parallel_gloo.py, the RCCL call itself is exercised here.)"""
    import ctypes as C
    from gan_mpc_amd import _lib
    pb, _, eng = _setup("tiny-ragged")
    lib = eng.lib
    buf = eng.to_dev(np.arange(1, 1001, dtype=np.float32))
    want = buf.clone()
    ws, rk = C.c_int(), C.c_int()
    _lib.check(lib.gmpc_comm_world(eng.ctx, C.byref(ws), C.byref(rk)))
    assert (ws.value, rk.value) == (1, 0)
    _lib.check(lib.gmpc_allreduce_grads(eng.ctx, C.c_void_p(buf.data_ptr()), buf.numel(), eng._stream()))
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
    uid = C.create_string_buffer(128)
    _lib.check(lib.gmpc_comm_unique_id(uid))
    assert any(uid.raw)
    _lib.check(lib.gmpc_comm_init(eng.ctx, 1, 0, uid))
    _lib.check(lib.gmpc_allreduce_grads(eng.ctx, C.c_void_p(buf.data_ptr()), buf.numel(), eng._stream()))
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
    assert lib.gmpc_comm_init(eng.ctx, 2, 5, uid) == -1      # rank outside the world: rejected before RCCL
    eng.close()
