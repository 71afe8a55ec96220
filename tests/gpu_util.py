"""Helpers shared by the GPU parity tests (TEST INFRASTRUCTURE)."""

import json
import os

import numpy as np

import gan_mpc_oracle as orc
from gan_mpc_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-5  # BASELINE.json north_star: 1e-5 relative fp32
SLACK_CEILING = 1e-3  # the "no worse than the fp32 oracle" branch never accepts more than this
# Riccati gains (and what follows from them: the iLQR iterate) are conditioning-limited in fp32: the
# stage cost's R = w0 (I - u u^T / (|u|^2 + a^2)) / sqrt(|u|^2 + a^2) with a = 1e-2 (reference
# cost_model.py:20-28) has condition number (|u|^2 + a^2) / a^2 ~ 1e4 for |u| ~ 1, so G = R + B^T P B is
# solved to ~1e4 x 6e-8 whatever the implementation -- the NumPy fp32 oracle shows the same ~1e-3.  Those
# stages get this ceiling on the slack branch; every other stage keeps SLACK_CEILING.
GAIN_CEILING = 1e-2
EL_FLOOR = 1e-6       # elementwise relative errors are taken against max(|ref|, EL_FLOOR * max|ref|)

# Every assertion appends one record here; tests/parity_report.py turns the file into the table
# committed as profiles/parity_rNN.md, so a stage that passes on the slack branch instead of on 1e-5
# is visible.  gpurun_out/ travels back from the GPU box.
PARITY_LOG = os.environ.get("GMPC_PARITY_LOG", os.path.join(ROOT, "gpurun_out", "parity_records.jsonl"))


def rel_err(a, ref):
    a = np.asarray(a, np.float64)
    ref = np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-300))


def el_err(a, ref):
    """Per-entry relative error with the floor EL_FLOOR * max|ref| under the denominator:
    (max over entries, 99.9th percentile).  Unlike the max-norm figure it sees small entries."""
    a = np.asarray(a, np.float64).ravel()
    ref = np.asarray(ref, np.float64).ravel()
    if ref.size == 0:
        return 0.0, 0.0
    den = np.maximum(np.abs(ref), EL_FLOOR * (np.abs(ref).max() + 1e-300))
    e = np.abs(a - ref) / den
    return float(e.max()), float(np.quantile(e, 0.999))


def _record(rec):
    try:
        os.makedirs(os.path.dirname(PARITY_LOG), exist_ok=True)
        rec["test"] = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(PARITY_LOG, "a") as fp:
            fp.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def assert_parity(name, hip, o32, o64, tol=TOL, slack=4.0, ceiling=SLACK_CEILING, el_tol=1e-3,
                  el_slack=16.0, config=None):
    """HIP fp32 vs the oracle: the fp64 oracle is the arbiter.

    Max-norm rule: pass if HIP is within `tol` (max-norm relative) of fp64, or no worse than `slack` x
    the oracle's own fp32 error -- a chained fp32 computation cannot be asked to beat fp32 -- and in
    that branch never above `ceiling`.
    Elementwise rule (small entries count): the largest per-entry relative error (floored denominator,
    see el_err) is within `el_tol`, or no worse than `el_slack` x the fp32 oracle's.
    Which branch decided, and every achieved error, is recorded."""
    e_hip = rel_err(hip, o64)
    e_o32 = rel_err(o32, o64)
    el_hip, el_hip_q = el_err(hip, o64)
    el_o32, el_o32_q = el_err(o32, o64)
    tol_used = max(tol, min(slack * e_o32, ceiling))
    el_used = max(el_tol, el_slack * el_o32)
    ok = bool(np.isfinite(e_hip) and e_hip <= tol_used and el_hip <= el_used)
    _record(dict(stage=name, config=config or CURRENT_CONFIG[0], e_hip=e_hip, e_o32=e_o32, tol=tol,
                 tol_used=tol_used, branch="tol" if e_hip <= tol else "slack", el_hip=el_hip,
                 el_o32=el_o32, el_hip_p999=el_hip_q, el_o32_p999=el_o32_q, el_used=el_used,
                 entries=int(np.asarray(o64).size), passed=ok))
    assert np.isfinite(e_hip), f"{name}: non-finite"
    assert e_hip <= tol_used, (
        f"{name}: HIP err {e_hip:.3e} vs fp64; oracle-fp32 err {e_o32:.3e}; tol {tol:.1e}, "
        f"slack {slack} capped at {ceiling:.0e}")
    assert el_hip <= el_used, (
        f"{name}: elementwise HIP err {el_hip:.3e} (p99.9 {el_hip_q:.3e}) vs fp64; oracle-fp32 "
        f"{el_o32:.3e} (p99.9 {el_o32_q:.3e})")
    return e_hip, e_o32


def assert_gain_backward_error(lqr64, K_hip, k_hip, K32, k32, tol=TOL, slack=4.0, ceiling=GAIN_CEILING):
    """The Riccati gains in the BACKWARD-error sense: residual of trajax' gain equations
    (G_t + 1e-8 I) K_t = -H_t and (G_t + 1e-8 I) k_t = -h_t with G, H, h formed in fp64 from the fp64 value
    function, max-norm over the horizon relative to |H| / |h|.  The forward error of K carries cond(G)
    (see GAIN_CEILING); this figure does not -- what is left in it is the fp32 propagation of the value
    function (P, p) over the horizon, which the fp32 oracle shows too (3e-3 in k at n = 1024, T = 100)."""
    Q, q, R, r, M, A, Bm = lqr64
    with np.errstate(all="ignore"):
        _, _, P, p = orc.tvlqr(*lqr64)
    T = K_hip.shape[1]
    Bt = np.swapaxes(Bm[:, :T], -1, -2)
    BtP = Bt @ P[:, 1:]
    G = BtP @ Bm[:, :T] + R[:, :T]
    G = (G + np.swapaxes(G, -1, -2)) / 2 + 1e-8 * np.eye(G.shape[-1])
    H = BtP @ A[:, :T] + np.swapaxes(M[:, :T], -1, -2)
    h = r[:, :T] + np.einsum("btnm,btn->btm", Bm[:, :T], p[:, 1:])
    out = {}
    for tag, K, k in (("hip", K_hip, k_hip), ("o32", K32, k32)):
        K, k = np.asarray(K, np.float64), np.asarray(k, np.float64)
        out[tag] = (float(np.abs(G @ K + H).max() / np.abs(H).max()),
                    float(np.abs(np.einsum("btij,btj->bti", G, k) + h).max() / np.abs(h).max()))
    for i, stage in enumerate(("gain equation residual |G K + H| / |H| (fp64 G, H)",
                               "gain equation residual |G k + h| / |h| (fp64 G, h)")):
        e_hip, e_o32 = out["hip"][i], out["o32"][i]
        tol_used = max(tol, min(slack * e_o32, ceiling))
        ok = bool(np.isfinite(e_hip) and e_hip <= tol_used)
        _record(dict(stage=stage, config=CURRENT_CONFIG[0], e_hip=e_hip, e_o32=e_o32, tol=tol,
                     tol_used=tol_used, branch="tol" if e_hip <= tol else "slack",
                     entries=int(K_hip.size if i == 0 else k_hip.size), passed=ok))
        assert ok, f"{stage}: HIP {e_hip:.3e}, oracle-fp32 {e_o32:.3e}, allowed {tol_used:.3e}"
    return out


CURRENT_CONFIG = [""]   # set by the tests' _setup so that the records name the shape


def set_config(label):
    CURRENT_CONFIG[0] = label


def problem(n, m, T, B, seed=0, dyn_hidden=(200, 200, 200), cost_hidden=(128, 128), cost_fout=10,
            head_hidden=(), bias_scale=0.1, out_scale=1.0, dyn_lstm=0):
    """dyn_lstm = F > 0: the LSTM dynamics variant; n is then the x size and pb["n"] = n + 2F the state size."""
    pb = orc.make_problem(n, m, T, B, seed=seed, dtype=np.float32, dyn_hidden=dyn_hidden,
                          cost_hidden=cost_hidden, cost_fout=cost_fout, head_hidden=head_hidden,
                          bias_scale=bias_scale, dyn_lstm=dyn_lstm)
    if out_scale != 1.0:  # "trained-like" residual dynamics: next_x = x + small
        layers = pb["dyn"]["tail"] if dyn_lstm else pb["dyn"]
        W, b = layers[-1]
        layers[-1] = ((W * out_scale).astype(np.float32), (b * out_scale).astype(np.float32))
    return pb


def dyn_tree(dyn):
    return P.lstm_dynamics_dict_to_tree(dyn) if isinstance(dyn, dict) else P.layers_to_tree(dyn)


def engine_for(pb, max_batch=None, critic=True):
    from gan_mpc_amd.engine import Engine
    lstm = isinstance(pb["dyn"], dict)
    layers = pb["dyn"]["tail"] if lstm else pb["dyn"]
    dyn_dims = [layers[0][0].shape[0]] + [W.shape[1] for W, _ in layers]
    cost_dims = [pb["cmlp"][0][0].shape[0]] + [W.shape[1] for W, _ in pb["cmlp"]]
    F = pb["critic"]["Wh"].shape[0]
    head = [F] + [W.shape[1] for W, _ in pb["critic"]["head"]]
    eng = Engine(pb["n"], pb["m"], pb["T"], dyn_dims, cost_dims, max_batch or pb["B"],
                 lstm_features=F if critic else 0, head_dims=head,
                 dyn_lstm=pb["dyn"]["Wh"].shape[0] if lstm else 0, x_size=pb.get("nx", 0) if lstm else 0)
    eng.set_params(eng.to_dev(pb["mpc_w"]), eng.to_dev(P.pack_dynamics(dyn_tree(pb["dyn"]))),
                   eng.to_dev(P.pack_mlp(P.layers_to_tree(pb["cmlp"]))))
    return eng


def dyn_near_kink(dyn, X, U, thresh=3e-6):
    """(B, T) bool: a relu pre-activation of the dynamics network at (X[:, t], U[:, t]) is within `thresh` of
    the kink (MLP variant: every hidden layer; LSTM variant: the relu tail after the cell)."""
    B, T, m = U.shape
    N = X.shape[-1]
    if not isinstance(dyn, dict):
        return near_kink(dyn, np.concatenate([X[:, :T], U], -1).reshape(B * T, N + m), thresh).reshape(B, T)
    _, zs = orc.lstm_dynamics_predict(dyn, X[:, :T].reshape(B * T, N), U.reshape(B * T, m))
    bad = np.zeros(B * T, bool)
    for z in zs:
        bad |= (np.abs(z) < thresh * np.abs(z).max(axis=1, keepdims=True)).any(axis=1)
    return bad.reshape(B, T)


def critic_flat(pb):
    return P.pack_critic(P.critic_dict_to_tree(pb["critic"]))


def split_critic_flat(v, n, F, head_dims):
    """The blocks of a flat critic vector (parameters or gradient) in pack_critic's layout
    Wx[n][4F] | Wh[F][4F] | b[4F] | W[K][N], b[N] per head layer: a list of (name, 1-D view).
    head_dims = (F, hidden..., 1)."""
    v = np.asarray(v).reshape(-1)
    sizes = [("Wx", n * 4 * F), ("Wh", F * 4 * F), ("b", 4 * F)]
    for l, (K, N) in enumerate(zip(head_dims[:-1], head_dims[1:])):
        sizes += [(f"head{l}.W", K * N), (f"head{l}.b", N)]
    assert sum(s for _, s in sizes) == v.size, (v.size, sizes)
    out, o = [], 0
    for name, s in sizes:
        out.append((name, v[o:o + s]))
        o += s
    return out


def near_kink(layers, q, thresh=3e-6):
    """(rows,) bool: some hidden pre-activation is within `thresh` (relative to that sample's layer scale)
    of the relu kink, where the derivative is discontinuous (hard part iii)."""
    _, zs = orc.mlp_forward(layers, q)
    bad = np.zeros(q.shape[0], bool)
    for z in zs:
        bad |= (np.abs(z) < thresh * np.abs(z).max(axis=1, keepdims=True)).any(axis=1)
    return bad


def pack_grads_cost(g_mpc, g_cost):
    out = [np.asarray(g_mpc).reshape(-1)]
    for gW, gb in g_cost:
        out += [np.asarray(gW).reshape(-1), np.asarray(gb).reshape(-1)]
    return np.concatenate(out)


def pack_grads_critic(g):
    out = [g["Wx"].reshape(-1), g["Wh"].reshape(-1), g["b"].reshape(-1)]
    for gW, gb in g["head"]:
        out += [np.asarray(gW).reshape(-1), np.asarray(gb).reshape(-1)]
    return np.concatenate(out)


def check_bilevel_at_iterate(pb, pb64, loss_kind, X, U, loss, grad, Hd, dXd, Bvd, batch_mean=False, keep=None,
                             end_to_end=True):
    """a8-a11 at the lower-level solution the GPU found (X, U), stage by stage.  The Hessian solve is
    ill-conditioned (forward error = cond(A) x backward error), so H is checked by its residual A H - B in fp64;
    the other stages are checked with the GPU's own H, dX as input.  Used by test_gpu_parity.test_bilevel_grad (the
    engine: per-trajectory `loss`, batch-summed `grad`) and by test_gpu_mirror (the policy layer: batch_mean=True,
    `loss` and `grad` are means over the batch, through the policy's packing and its all-reduce mean).

    Hd, dXd, Bvd are the ctx's H, dX, Bvec (debug buffers 2, 3, 4).  `keep` (bool per trajectory, default all)
    selects the trajectories of the per-trajectory checks -- Bvec, the residual, the tangent roll: those with a
    relu pre-activation at a kink may take a different side on the GPU.  The loss, the cost_vjp stage (the GPU's own
    H, dX in, so no conditioning) and the end-to-end gradient are over the whole batch; the end-to-end comparison
    therefore needs every trajectory kept (end_to_end=False leaves it to the caller)."""
    B, T, n = X.shape[0], U.shape[1], X.shape[-1]
    keep = np.ones(B, bool) if keep is None else np.asarray(keep, bool)
    red = (lambda a: a.mean(0)) if batch_mean else (lambda a: a.sum(0))

    def pack(g_mpc, g_cost):
        return pack_grads_cost(red(g_mpc), [(red(a), red(b)) for a, b in g_cost])

    def stages(p, dt):
        Xa, Ua = X.astype(dt), U.astype(dt)
        lqr = orc.get_lqr_params(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], Xa, Ua)
        if loss_kind == 0:
            lv, lx = orc.l2_loss(Xa, p["true_seq"]), orc.l2_loss_grad_x(Xa, p["true_seq"])
        else:
            lv, lx = orc.generator_loss(p["critic"], Xa), orc.generator_loss_grad_x(p["critic"], Xa)
        Bv = orc.loss_grad_wrt_control(lqr[5], lqr[6], lx)
        # the LQ model whose Hessian is the reference's dense one (curvature of smooth dynamics included)
        lqr = orc.second_order_lqr(p["dyn"], lqr, orc.adjoint(lqr[5], lqr[6], lqr[1], lqr[3])[1], Xa, Ua)
        Hc, dX = orc.hessian_solve(lqr, Bv)
        g_mpc, g_cost = orc.cost_vjp(p["cmlp"], p["mpc_w"], p["goal"], Xa, Ua, Hd.astype(dt), dXd.astype(dt))
        g_from_hip_H = pack(g_mpc, g_cost)
        g_mpc, g_cost = orc.cost_vjp(p["cmlp"], p["mpc_w"], p["goal"], Xa, Ua, Hc, dX)
        g_full = pack(g_mpc, g_cost)
        return dict(lqr=lqr, loss=lv.mean() if batch_mean else lv, Bv=Bv, H=Hc, g_stage=g_from_hip_H, g_full=g_full)

    s32, s64 = stages(pb, np.float32), stages(pb64, np.float64)
    assert_parity("loss", loss, s32["loss"], s64["loss"])
    assert_parity("Bvec", Bvd[keep], s32["Bv"][keep], s64["Bv"][keep])
    lq = [a[keep] for a in s64["lqr"]]
    Bv64 = s64["Bv"][keep]

    # residual of the structured solve, per trajectory, in fp64
    def resid(H):
        r = orc.hessian_apply(lq, H[keep].astype(np.float64)) - Bv64
        return np.sqrt((r ** 2).sum((1, 2)) / (Bv64 ** 2).sum((1, 2)))
    r_hip, r_o32 = resid(Hd), resid(s32["H"])
    _record(dict(stage="Hessian solve residual |A H - B| / |B| (fp64 A, B; max over trajectories)",
                 config=CURRENT_CONFIG[0], e_hip=float(r_hip.max()), e_o32=float(r_o32.max()), tol=1e-4,
                 tol_used=float(np.maximum(1e-4, 10 * r_o32).min()), branch="tol" if r_hip.max() <= 1e-4 else "slack",
                 entries=int(Hd[keep].size), passed=bool((r_hip <= np.maximum(1e-4, 10 * r_o32)).all())))
    assert np.median(r_hip) < 1e-4 and (r_hip <= np.maximum(1e-4, 10 * r_o32)).all(), (r_hip, r_o32)
    # tangent roll consistent with H
    Hk = Hd[keep].astype(np.float64)
    dx = np.zeros((Hk.shape[0], T + 1, n))
    for t in range(T):
        dx[:, t + 1] = np.einsum("bij,bj->bi", lq[5][:, t], dx[:, t]) + np.einsum("bnm,bm->bn", lq[6][:, t], Hk[:, t])
    assert rel_err(dXd[keep], dx) < 1e-4
    # a11 given the same (H, dX)
    assert_parity("cost_vjp stage", grad, s32["g_stage"], s64["g_stage"])
    if not end_to_end:
        return s32, s64
    # end to end.  The forward error of the gradient is the Hessian solve's backward error (the residual checked
    # above, fp32-sized) seen through cond(A) -- for a given residual SIZE it varies with the residual's direction
    # (6e-6 .. 6e-4 across the parity configs for the HIP path and for the fp32 oracle alike, uncorrelated), so one
    # draw of the fp32 oracle's own forward error is a poor yardstick.  The bar: 1e-4, or 10 x the fp32 oracle's
    # error, or 4 x what a backward error of HIP's size does to the gradient in fp64 (largest of four random
    # right-hand-side perturbations of relative norm r_hip per trajectory); never above 1e-3.  The elementwise
    # rule gets the same third term.
    assert keep.all(), "the end-to-end gradient is over the whole batch: no trajectory may sit at a relu kink"
    rng = np.random.default_rng(7)
    e_pert, el_pert = 0.0, 0.0
    for _ in range(4):
        noise = rng.standard_normal(Bv64.shape)
        noise *= (r_hip * np.sqrt((Bv64 ** 2).sum((1, 2)) / (noise ** 2).sum((1, 2))))[:, None, None]
        Hp, dXp = orc.hessian_solve(lq, Bv64 + noise)
        g_mpc, g_cost = orc.cost_vjp(pb64["cmlp"], pb64["mpc_w"], pb64["goal"], X.astype(np.float64),
                                     U.astype(np.float64), Hp, dXp)
        gp = pack(g_mpc, g_cost)
        e_pert = max(e_pert, rel_err(gp, s64["g_full"]))
        el_pert = max(el_pert, el_err(gp, s64["g_full"])[0])
    _record(dict(stage="gradient response to a backward error of HIP's size (fp64, 4 random directions)",
                 config=CURRENT_CONFIG[0], e_hip=e_pert, e_o32=float(r_hip.max()), tol=1e-4, tol_used=1e-3,
                 branch="info", el_hip=el_pert, entries=int(s64["g_full"].size), passed=True))
    # (the round-2 bar, fixed 1e-4, kept as a recorded check: profiles/parity_r04.md lists which shapes pass it)
    e_fixed, e_fixed32 = rel_err(grad, s64["g_full"]), rel_err(s32["g_full"], s64["g_full"])
    _record(dict(stage="bilevel grad end-to-end against the round-2 fixed bar 1e-4 (recorded, not asserted)",
                 config=CURRENT_CONFIG[0], e_hip=e_fixed, e_o32=e_fixed32, tol=1e-4, tol_used=1e-4, branch="info",
                 entries=int(s64["g_full"].size), passed=bool(e_fixed <= 1e-4)))
    assert_parity("bilevel grad end-to-end", grad, s32["g_full"], s64["g_full"],
                  tol=min(max(1e-4, 4.0 * e_pert), SLACK_CEILING), slack=10.0, el_tol=max(1e-3, 4.0 * el_pert))
    return s32, s64
