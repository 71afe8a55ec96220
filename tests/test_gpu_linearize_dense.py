"""The dense Jacobian chain k_linearize_mfma<NT, NTF> through gmpc_linearize_ex: all 32 instantiations, the four staging
combinations with one and with several hidden layers, the three input-GEMM bodies, column groups, tiles that straddle
samples, a ragged last tile, the persistent loop's second pass, `active` skipping and strided sample sets -- each case of
tests/linearize_cases.py against the fp64 product of the same fp32 weights under the SAME relu bits (no forward pass, so
no kink and no entry left out): bit for bit on the integer fill, within

    |err_ij| <= gamma_N (|W_L|^T D ... |W_1|^T)_ij + 2^-24 |J_ij|,   gamma_N = N u / (1 - N u),  N = sum_l (K_l + 2)

on the normal one (K_l the contracted widths; derived, not measured).  AB is pre-filled with index-carrying NaNs between
guard words and the biases hold +-1e30; every case launches twice (same bits) and again after a second gmpc_set_params
(the second weights' Jacobians).  Then: the refusals of gmpc_linearize_ex, and lqr_backward on one shape per family.  The table, reference, checker and the fp32 model they are checked against: tests/test_linearize_cases.py."""

import numpy as np
import pytest
import torch

import gpu_util as gu
import linearize_cases as lc
from gan_mpc_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _bits(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy())           # bits, not values: NaN payloads


class _Run:
    """One case's engine and device buffers."""

    def __init__(self, case):
        c = self.case = case
        self.eng = e = Engine(c.n, c.m, c.T, list(c.dims), [c.n, 8, 2], max_batch=min(c.B, 3))
        rng = np.random.default_rng(5)
        self.mpc_w = e.to_dev(np.array([1.0, 0.5, 0.1], np.float32))
        self.cost = e.to_dev(rng.standard_normal(e.cost_count).astype(np.float32))

    def set_params(self, Bf, which):
        self.eng.set_params(self.mpc_w, self.eng.to_dev(Bf.dyn[which]), self.cost)

    def launch(self, Bf):
        c, e = self.case, self.eng
        masks = _bits(Bf.masks).to(e.device)
        active = None if Bf.active is None else torch.from_numpy(Bf.active).to(e.device)
        ab = _bits(Bf.AB0).to(e.device).view(torch.float32)
        e.linearize(masks, ab[lc.GUARD:], c.nsamp, active=active, samp_mul=c.samp_mul, samp_add=c.samp_add)
        torch.cuda.synchronize()
        return ab.view(torch.int32).cpu().numpy().view(np.float32)

    def close(self):
        self.eng.close()


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_linearize_case(case):
    run = _Run(case)
    try:
        r = run.eng.linearize_route(case.nsamp, case.strided)
        assert r["family"] == "mfma" and {k: r[k] for k in case.want} == case.want
        kernel = "k_linearize_mfma<%d, %d>" % (r["NT"], r["NTF"])
        for fill in lc.FILLS:
            Bf = lc.build(case, fill)
            ref = lc.reference(Bf)
            run.set_params(Bf, 0)
            got = run.launch(Bf)
            assert run.eng.profile_kernel_name("linearize") == "k_linearize_mfma"

            def record(fig):
                lim = 0.0 if fill == "exact" else 1.0
                print(f"{case.id} {fill}: {kernel} w1 {r['stage_w1']} wl {r['stage_wl']} {r['body']}: worst error "
                      f"{fig['entry']:.3f} of the bound, max |err| {fig['max_err']:.3e}, {fig['entries']} entries")
                gu._record(dict(stage=f"linearize {kernel} {r['body']}, {fill} fill: per-entry error / bound in el_hip "
                                      "(exact fill: must be 0)", config=case.id, e_hip=fig["max_err"], tol=gu.TOL,
                                tol_used=gu.TOL, branch="tol", el_hip=fig["entry"], el_used=lim,
                                entries=fig["entries"], passed=bool(fig["entry"] <= lim)))

            compared = lc.check(Bf, ref, got, on_figures=record)
            if case.active in ("null", "on"):
                assert compared == case.nsamp * case.n * (case.n + case.m)      # nothing left out
            # no atomics, one wave per tile: the same launch again, from the same pre-fill, gives the same bits
            again = run.launch(Bf)
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
            # other weights on the same engine: the padded operands are rebuilt, nothing of the first set is left
            run.set_params(Bf, 1)
            got2 = run.launch(Bf)
            lc.check(Bf, lc.reference(Bf, which=1), got2)
            if case.active != "off" and fill == "normal":      # (dense weights: some written entry differs)
                assert not np.array_equal(got.view(np.uint32), got2.view(np.uint32))
    finally:
        run.close()


# family, kernel name prefix, n (the x size under LSTM dynamics), m, hidden, dyn_lstm
FAMILY_SHAPES = [("sparse", "k_linearize_sparse", 17, 6, (200, 200), 0), ("regs", "k_linearize_regs", 17, 6, (64, 64), 0),
                 ("mfma", "k_linearize_mfma", 17, 6, (200, 150), 0), ("mfma", "k_linearize_mfma", 33, 1, (200, 200), 0),
                 ("dynl", "k_dynl_jac", 4, 2, (12,), 6),
                 # large state: the dense step on k_linearize_mfma and on the wide register chain, the low-rank form
                 ("mfma", "k_linearize_mfma", 70, 7, (128, 96), 0), ("regs", "k_linearize_regs<6, 100, 8, true>", 90, 10, (200, 200), 0),
                 ("lowrank", "low-rank factors", 90, 4, (30,), 0)]


@pytest.mark.parametrize("family,kernel,n,m,hidden,lstm", FAMILY_SHAPES,
                         ids=["%s-n%dm%d-%s" % (f, n, m, "x".join(map(str, h))) for f, _, n, m, h, _ in FAMILY_SHAPES])
def test_backward_pass_runs_the_family_the_route_names(family, kernel, n, m, hidden, lstm, monkeypatch):
    monkeypatch.delenv("GMPC_LIN", raising=False)
    monkeypatch.delenv("GMPC_BIG_DENSE", raising=False)
    T, B = 3, 3
    pb = gu.problem(n, m, T, B, seed=3, dyn_hidden=hidden, cost_hidden=(8,), cost_fout=2, dyn_lstm=lstm, out_scale=0.3)
    eng = gu.engine_for(pb, critic=False)
    try:
        r = eng.linearize_route(B if eng.big else B * T, strided=eng.big)
        assert r["family"] == family
        d = eng.to_dev
        x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
        X, _ = eng.rollout_cost(x0, U, goal)
        out = eng.lqr_backward(X, U, goal, after_rollout=True)
        torch.cuda.synchronize()
        name = eng.profile_kernel_name("linearize")
        assert name.startswith(kernel), name
        assert all(np.isfinite(v.cpu().numpy()).all() for v in out.values())
    finally:
        eng.close()


def test_linearize_ex_refusals():
    """GMPC_EINVAL, before any launch: LSTM dynamics, the low-rank large-state form, a ctx without parameters, NULL
    masks / AB and counts out of range."""
    from gan_mpc_amd import _lib
    for n, m, hidden, lstm in ((4, 2, (12,), 6), (90, 4, (30,), 0)):
        pb = gu.problem(n, m, 3, 3, seed=3, dyn_hidden=hidden, cost_hidden=(8,), cost_fout=2, dyn_lstm=lstm)
        eng = gu.engine_for(pb, critic=False)
        try:
            assert eng.linearize_route(3, strided=eng.big)["family"] == ("dynl" if lstm else "lowrank")
            masks = torch.zeros(9 * len(hidden) * lc.MW, dtype=torch.int32, device=eng.device)
            AB = eng.new(9 * eng.n * (eng.n + eng.m))
            with pytest.raises(_lib.GmpcError, match="LSTM dynamics and the low-rank form"):
                eng.linearize(masks, AB, 3, samp_mul=3, samp_add=1)
        finally:
            eng.close()
    c = lc.CASES[1]
    eng = Engine(c.n, c.m, c.T, list(c.dims), [c.n, 8, 2], max_batch=3)
    try:
        lib, st = eng.lib, eng._stream()
        masks = torch.zeros(c.smask * c.Lh * lc.MW, dtype=torch.int32, device=eng.device)
        AB = torch.full((c.entries,), float("nan"), device=eng.device)
        mp, ap = masks.data_ptr(), AB.data_ptr()
        assert lib.gmpc_linearize_ex(eng.ctx, c.nsamp, mp, None, ap, 1, 0, st) != 0
        assert b"gmpc_set_params has not been called" in lib.gmpc_last_error()
        Bf = lc.build(c, "normal")
        eng.set_params(eng.to_dev(np.ones(3, np.float32)), eng.to_dev(Bf.dyn[0]), eng.to_dev(np.zeros(eng.cost_count, np.float32)))
        for args in ((c.nsamp, None, None, ap, 1, 0), (c.nsamp, mp, None, None, 1, 0), (0, mp, None, ap, 1, 0),
                     (-1, mp, None, ap, 1, 0), (c.nsamp, mp, None, ap, 0, 0), (c.nsamp, mp, None, ap, 1, -1)):
            assert lib.gmpc_linearize_ex(eng.ctx, *args, st) == -1, args          # GMPC_EINVAL
        with pytest.raises(_lib.GmpcError):
            eng.linearize(masks[:-1], AB, c.nsamp)                                 # too few mask words
        with pytest.raises(_lib.GmpcError):
            eng.linearize(masks, AB[:-1], c.nsamp)
        with pytest.raises(_lib.GmpcError):
            eng.linearize(masks, AB, 2, samp_mul=c.smask, samp_add=1)              # a sample past the masks
        torch.cuda.synchronize()
        assert torch.isnan(AB).all()                                               # nothing was launched
        eng.linearize(masks, AB, c.nsamp)                                          # and the good call goes through
        torch.cuda.synchronize()
        assert torch.isfinite(AB).all()
    finally:
        eng.close()
