"""The one-step disagreement's VJP on the GPU (gmpc_ensemble_disagreement_vjp): every output
against the fp64 reference at the GPU's own X (G1); independence of a problem's outputs from its row and from B, of a
member's row from P and the others' cotangents (G2); exact zeros for members equal to the bound dynamics (G3); subsets of
outputs, and gD alone (G4); statelessness (G5); refusals (G6); a NaN member (G7); ensemble_disagreement_layer (G8);
plan_risk and refine_plan under the penalty (G9).

Cases: disagreement_vjp_cases' -- sampled_ensemble_cases' seven shapes with their three members and the tile cases B = 1,
33, 64 on n 5, m 2, T 8 (B T = 8, 264 and 512 rows of the row kernels' tiles of 32).  Tolerances: those of
test_gpu_ensemble_rollout_vjp -- gpu_util.assert_parity at its defaults for x0 / U, tol=1e-4, slack=10, el_tol=1e-2 for
the sums over the batch (nominal / members).  A problem is left out of G1 / G8 / G9 when the nominal network or a member
is within gpu_util's 3e-6 of a relu kink along the nominal rollout; the cotangents of G1 come from the first seed whose
fp64 reference meets the conditioning cap (disagreement_vjp_cases.pick_seed; test_disagreement_vjp_host's H3 shows there
is one for every case).

Achieved on MI355X (the tests print them): see DESIGN.md section 30."""

import functools
import itertools

import numpy as np
import pytest
import torch

import disagreement_vjp_cases as vc
import disagreement_vjp_ref as vr
import gpu_util as gu
import sampled_ensemble_cases as ec
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

KEYS = vr.KEYS
SUMS = ("nominal", "members")


def _tol(key):
    return dict(tol=1e-4, slack=10.0, el_tol=1e-2) if key in SUMS else {}


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what=""):
    np.testing.assert_array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)), err_msg=what)


def _engine(case, pb=None, **more):
    return gu.engine_for(vc.problem(case) if pb is None else pb, critic=False, **more)


def _members(eng, case, which=(0, 1, 2), count=ec.MEMBERS):
    return eng.to_dev(ec.flat([vc.members(case, count)[p] for p in which]))


def _rolled(eng, mem, x0, U):
    d = eng.to_dev
    return eng.ensemble_disagreement(mem, d(x0), d(U), want=("X",))["X"].cpu().numpy()


def _call(eng, mem, X, U, gd, gD, want=KEYS):
    d = lambda a: None if a is None else eng.to_dev(np.ascontiguousarray(a))  # noqa: E731
    out = eng.ensemble_disagreement_vjp(mem, d(X), d(U), d(gd), d(gD), want=want)
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _nominal_X(case):
    """The GPU's nominal rollout of the case's problems."""
    pb = vc.problem(case)
    eng = _engine(case)
    try:
        X = _rolled(eng, _members(eng, case), pb["x0"], pb["U"])
        torch.cuda.synchronize()
    finally:
        eng.close()
    return X


# ---- G1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,which", list(itertools.product(vc.CASES, vc.WHICH)))
def test_g1_every_output_against_fp64_at_the_gpus_own_states(case, which):
    pb = vc.problem(case)
    members = vc.members(case)
    X = _nominal_X(case)
    ok = vc.kept(case, X.astype(np.float64), pb["U"])
    print(f"G1 {case}: {ok.sum()} of {pb['B']} problems kept")
    assert ok.sum() >= max(1, pb["B"] - pb["B"] // 2)
    X, U = np.ascontiguousarray(X[ok]), np.ascontiguousarray(pb["U"][ok])
    seed, gd, gD, r64, tried = vc.pick_seed(case, X.astype(np.float64), U, which)
    print(f"G1 {case} {which}: cotangents of seed {seed}; kappa " + " ".join(f"{k:.3g}" for k in tried))
    assert seed is not None, f"no well-conditioned draw of the cotangents in 16 seeds: kappa {tried}"
    r32 = vr.reference(pb["dyn"], members, X, U, gd, gD)
    eng = _engine(case)
    try:
        got = _call(eng, _members(eng, case), X, U, gd, gD)
        torch.cuda.synchronize()
    finally:
        eng.close()
    gu.set_config(f"ensemble disagreement vjp {case}")
    assert got["members"].shape == (ec.MEMBERS, r64["members"].shape[1])
    for key in KEYS:
        e = gu.assert_parity(f"ensemble disagreement vjp {key} ({which}) {case}", got[key], r32[key], r64[key],
                             **_tol(key))
        print(f"G1 {case} {which} {key}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")
    if which == "both":
        # the members rolled by one place do not pass: member p + 1 under member p's cotangents
        w = lambda a: a.astype(np.float64)  # noqa: E731
        wrong = vr.reference(pb["dyn"], members[1:] + members[:1], w(X), w(U), w(gd), w(gD))
        for key in KEYS:
            assert gu.rel_err(wrong[key], r64[key]) > 1e-3, key


# ---- G2 ------------------------------------------------------------------------------------------------------------
def test_g2_a_problems_outputs_depend_on_neither_its_row_nor_b():
    pb = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vc.problem("tile33").items()}
    for k in ("x0", "U"):
        pb[k][32] = pb[k][0]                  # the same problem at row 0 of the batch and as its 33rd
    eng = _engine("tile33", pb=pb)
    try:
        mem = _members(eng, "tile33")
        X = _rolled(eng, mem, pb["x0"], pb["U"])
        _same(X[32], X[0])
        gd, gD = vc.cots(3, 33, pb["T"], "both", 3)
        gd[:, 32], gD[:, 32] = gd[:, 0], gD[:, 0]
        batch = _call(eng, mem, X, pb["U"], gd, gD)
        again = _call(eng, mem, X, pb["U"], gd, gD)
        for k in KEYS:
            _same(again[k], batch[k], f"G2 repeat {k}")
        alone = _call(eng, mem, X[:1], pb["U"][:1], gd[:, :1], gD[:, :1])
    finally:
        eng.close()
    for k in ("x0", "U"):
        _same(batch[k][0], alone[k][0], f"G2 row 0 {k}")
        _same(batch[k][32], alone[k][0], f"G2 row 32 {k}")
        assert not np.array_equal(batch[k][1], batch[k][0])


def test_g2_a_members_row_depends_on_neither_p_nor_the_others_cotangents():
    case = "tile33"
    pb = vc.problem(case)
    X = _nominal_X(case)
    eng = _engine(case)
    try:
        m16 = _members(eng, case, tuple(range(16)), count=16)
        gd, gD = vc.cots(16, pb["B"], pb["T"], "both", 4)
        sixteen = _call(eng, m16, X, pb["U"], gd, gD)
        three = _call(eng, m16[:3].contiguous(), X, pb["U"], gd[:3], gD[:3])
        second = _call(eng, m16[1:2].contiguous(), X, pb["U"], gd[1:2], gD[1:2])
        zd, zD = np.zeros_like(gd[:3]), np.zeros_like(gD[:3])
        zd[1], zD[1] = gd[1], gD[1]
        masked = _call(eng, m16[:3].contiguous(), X, pb["U"], zd, zD)
    finally:
        eng.close()
    assert sixteen["members"].shape[0] == 16 and np.isfinite(sixteen["members"]).all()
    _same(second["members"][0], three["members"][1], "G2 P=3 members[1]")
    _same(second["members"][0], sixteen["members"][1], "G2 P=16 members[1]")
    _same(three["members"][2], sixteen["members"][2], "G2 P=16 members[2]")
    assert not np.array_equal(sixteen["members"][15], sixteen["members"][0])
    # the other members' zero cotangents add exact zeros: the P = 1 call's bits
    _same(masked["members"][1], second["members"][0], "G2 masked members[1]")
    assert not masked["members"][0].any() and not masked["members"][2].any()
    for k in ("x0", "U", "nominal"):
        assert np.array_equal(masked[k], second[k]), k
        assert not np.array_equal(three[k], second[k])


# ---- G3 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["base", "ragged", "w256", "tile33"])
def test_g3_members_equal_to_the_bound_dynamics_give_exact_zeros(case):
    pb = vc.problem(case)
    X = _nominal_X(case)
    gd, gD = vc.cots(3, pb["B"], pb["T"], "both", 6)
    nominal = pb["dyn"]
    eng = _engine(case)
    try:
        copies = _call(eng, eng.to_dev(ec.flat([nominal] * 3)), X, pb["U"], gd, gD)
        mem = vc.members(case)
        mixed = _call(eng, eng.to_dev(ec.flat([mem[0], nominal, mem[2]])), X, pb["U"], gd, gD)
        full = _call(eng, _members(eng, case), X, pb["U"], gd, gD)
    finally:
        eng.close()
    for k in KEYS:
        assert not copies[k].any(), k
    assert not mixed["members"][1].any()
    for p in (0, 2):
        _same(mixed["members"][p], full["members"][p], f"G3 members[{p}]")
        assert mixed["members"][p].any()
    assert mixed["x0"].any() and not np.array_equal(mixed["x0"], full["x0"])


# ---- G4 ------------------------------------------------------------------------------------------------------------
def test_g4_any_subset_of_outputs_and_gd_alone():
    case = "tile33"
    pb = vc.problem(case)
    X = _nominal_X(case)
    gd, gD = vc.cots(3, pb["B"], pb["T"], "both", 1)
    eng = _engine(case)
    try:
        mem = _members(eng, case)
        full = _call(eng, mem, X, pb["U"], gd, gD)
        for mask in range(1, 16):
            want = tuple(k for i, k in enumerate(KEYS) if mask >> i & 1)
            part = _call(eng, mem, X, pb["U"], gd, gD, want=want)
            assert tuple(part) == want
            for k in want:
                _same(part[k], full[k], f"G4 {k} with {want}")
        lone = _call(eng, mem, X, pb["U"], None, gD)
        zero = _call(eng, mem, X, pb["U"], np.zeros_like(gd), gD)
        only = _call(eng, mem, X, pb["U"], gd, None)
    finally:
        eng.close()
    for k in KEYS:
        _same(lone[k], zero[k], f"G4 gD alone {k}")
        assert full[k].any() and only[k].any() and not np.array_equal(only[k], full[k])


# ---- G5 ------------------------------------------------------------------------------------------------------------
def test_g5_a_held_solution_survives_the_call():
    name = "base"
    pb = ec.problem(name)
    B = pb["B"]
    X = _nominal_X(name)
    gd, gD = vc.cots(3, B, pb["T"], "both", 2)

    def tail(with_call):
        eng = _engine(name)
        try:
            d = eng.to_dev
            sol = eng.ilqr_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), {"maxiter": 3})
            if with_call:
                out = _call(eng, _members(eng, name), X, pb["U"], gd, gD)
                assert all(np.isfinite(v).all() for v in out.values())
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            return {k: v.cpu().numpy() for k, v in sol.items()}, loss.cpu().numpy(), grad.cpu().numpy()
        finally:
            eng.close()

    s0, l0, g0 = tail(False)
    s1, l1, g1 = tail(True)
    assert s0.keys() == s1.keys()
    for k in s0:
        _same(s0[k], s1[k], f"G5 held {k}")
    _same(l0, l1)
    _same(g0, g1)


def test_g5_a_solve_under_the_penalty_is_the_same_before_and_after():
    name = "base"
    pb = ec.problem(name)
    eng = _engine(name)
    try:
        d = eng.to_dev
        eng.set_sampled_ensemble(_members(eng, name))
        eng.set_sampled_ensemble_mode(aggregate="max")
        eng.set_sampled_disagreement(0.5)
        args = (d(pb["x0"]), d(pb["U"]), d(pb["goal"]), ec.LO, ec.HI, ec.engine_kwargs("cem", name, 2))
        want = ("costs", "elites", "samples")
        before = {k: v.cpu().numpy() for k, v in eng.cem_solve(*args, want=want).items()}
        other = _members(eng, name, (3, 4), count=5)
        gd, gD = vc.cots(2, pb["B"], pb["T"], "both", 2)
        mid = _call(eng, other, _nominal_X(name), pb["U"], gd, gD)
        after = {k: v.cpu().numpy() for k, v in eng.cem_solve(*args, want=want).items()}
    finally:
        eng.close()
    assert before.keys() == after.keys()
    for k in before:
        _same(before[k], after[k], f"G5 {k}")
    assert all(np.isfinite(v).all() and v.any() for v in mid.values())


def test_g5_a_large_call_leaves_nothing_for_a_small_one():
    case = "tile33"
    pb = vc.problem(case)
    X = _nominal_X(case)
    gd, gD = vc.cots(3, pb["B"], pb["T"], "both", 9)

    def run(eng, Bq, P):
        mem = _members(eng, case, tuple(range(P)), count=16)
        return _call(eng, mem, X[:Bq], pb["U"][:Bq], np.resize(gd, (16, 33, pb["T"]))[:P, :Bq],
                     np.resize(gD, (16, 33))[:P, :Bq])

    eng = _engine(case)
    try:
        fresh = run(eng, 5, 2)
    finally:
        eng.close()
    eng = _engine(case)
    try:
        run(eng, 33, 16)
        small = run(eng, 5, 2)
        d = eng.to_dev
        eng.rollout_vjp(d(X), d(pb["U"]), d(pb["goal"]), d(np.ones_like(X)), d(np.ones(X.shape[:2], np.float32)))      # another user of the workspace
        third = run(eng, 5, 2)
    finally:
        eng.close()
    for k in KEYS:
        _same(small[k], fresh[k], f"G5 after a large call: {k}")
        _same(third[k], fresh[k], f"G5 after rollout_vjp: {k}")


# ---- G6 ------------------------------------------------------------------------------------------------------------
def test_g6_refused_arguments_at_the_c_abi():
    from gan_mpc_amd.engine import Engine
    name = "m1"
    pb = ec.problem(name)
    (n, m, T, B, _, _), _ = ec.CASES[name]
    eng = _engine(name)
    try:
        lib, d = eng.lib, eng.to_dev
        mem, U, X = _members(eng, name), d(pb["U"]), d(_nominal_X(name))
        gd, gD = (d(a) for a in vc.cots(3, B, T, "both", 5))
        gx0, gU = eng.new(B, n), eng.new(B, T, m)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        good = dict(ctx=eng.ctx, B=B, P=3, mem=mem, X=X, U=U, gd=gd, gD=gD, gx0=gx0, gU=gU, gnom=None, gmem=None)

        def call(**change):
            a = dict(good, **change)
            return lib.gmpc_ensemble_disagreement_vjp(a["ctx"], a["B"], a["P"], p(a["mem"]), p(a["X"]), p(a["U"]),
                                                      p(a["gd"]), p(a["gD"]), p(a["gx0"]), p(a["gU"]), p(a["gnom"]),
                                                      p(a["gmem"]), None)

        assert call() == 0
        torch.cuda.synchronize()
        first = gU.cpu().numpy().copy()
        for change in (dict(ctx=None), dict(mem=None), dict(X=None), dict(U=None), dict(B=0), dict(B=B + 1), dict(P=0),
                       dict(P=17), dict(gd=None, gD=None), dict(gx0=None, gU=None)):
            assert call(**change) == -1, change                      # GMPC_EINVAL
            assert lib.gmpc_last_error().startswith(b"ensemble disagreement vjp: "), (change, lib.gmpc_last_error())
        assert b"B = 8" in (call(B=B + 1), lib.gmpc_last_error())[1]
        assert b"P = 17" in (call(P=17), lib.gmpc_last_error())[1]
        assert b"both null" in (call(gd=None, gD=None), lib.gmpc_last_error())[1]
        assert b"every output is null" in (call(gx0=None, gU=None), lib.gmpc_last_error())[1]
        # what is allowed: one cotangent, one output
        assert call(gd=None) == 0 and call(gD=None) == 0 and call(gx0=None) == 0
        assert call(gx0=None, gU=None, gmem=eng.new(3, eng.dyn_count)) == 0
        assert call(gx0=None, gU=None, gnom=eng.new(eng.dyn_count)) == 0
        assert call() == 0
        torch.cuda.synchronize()
        _same(gU.cpu().numpy(), first)
        fresh = Engine(n, m, T, [n + m, 8, n], [n, 8, 2], max_batch=B)       # no parameters set
        try:
            assert lib.gmpc_ensemble_disagreement_vjp(fresh.ctx, B, 1, p(eng.new(1, fresh.dyn_count)), p(X), p(U),
                                                      p(gd), None, p(gx0), None, None, None, None) != 0
            assert lib.gmpc_last_error().startswith(b"ensemble disagreement vjp: "), lib.gmpc_last_error()
            assert b"gmpc_set_params" in lib.gmpc_last_error()
        finally:
            fresh.close()
    finally:
        eng.close()


def test_g6_refusals_through_the_engine():
    name = "m1"
    pb = ec.problem(name)
    B, T, n, m = pb["B"], pb["T"], pb["n"], pb["m"]
    eng = _engine(name)
    try:
        d = eng.to_dev
        mem, U, X = _members(eng, name), d(pb["U"]), d(_nominal_X(name))
        gD = d(np.ones((3, B), np.float32))
        with pytest.raises(GmpcError, match="ensemble disagreement vjp: .*unknown entries"):
            eng.ensemble_disagreement_vjp(mem, X, U, gD=gD, want=("x0", "theta"))
        with pytest.raises(GmpcError, match="ensemble disagreement vjp: .*both None"):
            eng.ensemble_disagreement_vjp(mem, X, U)
        with pytest.raises(GmpcError, match="ensemble disagreement vjp: P = 17"):
            eng.ensemble_disagreement_vjp(torch.zeros(17, eng.dyn_count, device=eng.device), X, U, gD=gD)
        z = lambda *s: d(np.zeros(s, np.float32))  # noqa: E731
        with pytest.raises(GmpcError, match="error -1: ensemble disagreement vjp: B = 8"):       # the library's own
            eng.ensemble_disagreement_vjp(mem, z(B + 1, T + 1, n), z(B + 1, T, m), gD=z(3, B + 1))
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300"])
def test_g6_refused_shapes_carry_the_prefix(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    eng = gu.engine_for(pb, critic=False)
    try:
        X = torch.zeros(2, 4, eng.n, device=eng.device)
        with pytest.raises(GmpcError, match="error -1: ensemble disagreement vjp: "):
            eng.ensemble_disagreement_vjp(torch.zeros(2, eng.dyn_count, device=eng.device), X, eng.to_dev(pb["U"]),
                                          gD=torch.ones(2, 2, device=eng.device), want=("U",))
    finally:
        eng.close()


# ---- G7 ------------------------------------------------------------------------------------------------------------
def test_g7_a_nan_member_poisons_its_own_row_alone():
    case = "tile33"
    pb = vc.problem(case)
    X = _nominal_X(case)
    layers = [list(mb) for mb in vc.members(case)]
    W, b = layers[1][-1]
    W = W.copy()
    W[0, 0] = np.nan                         # one weight of member 1's output layer
    layers[1][-1] = (W, b)
    gd, gD = vc.cots(3, pb["B"], pb["T"], "both", 8)
    eng = _engine(case)
    try:
        out = _call(eng, eng.to_dev(ec.flat(layers)), X, pb["U"], gd, gD)
        clean = _call(eng, _members(eng, case), X, pb["U"], gd, gD)
    finally:
        eng.close()
    for p in (0, 2):
        _same(out["members"][p], clean["members"][p], f"G7 members[{p}]")
        assert np.isfinite(out["members"][p]).all()
    assert not np.isfinite(out["members"][1]).all()
    assert np.isfinite(clean["members"]).all()
    # the shared sums carry member 1's e and q
    assert not np.isfinite(out["x0"]).all() and not np.isfinite(out["nominal"]).all()


# ---- G8 / G9: the layer and the policy ----------------------------------------------------------------------------
PENALTY = 0.5


def _policy_problem(N, M, B):
    """test_gpu_ensemble_rollout_vjp's policy with its three-member ensemble, its parameters and the first B problems
    whose nominal rollouts are away from the nominal network's and every member's kinks; X: the GPU's nominal rollout."""
    import test_gpu_ensemble_rollout_vjp as erv
    import test_gpu_mirror as mirror
    policy, params, data, members = erv._policy(N, M)
    pb = mirror._oracle_problem(params, data, np.arange(12), np.float32)
    pb["T"] = pb["U"].shape[1]
    eng = policy.bind(policy.to_device_params(params), 12)
    X = eng.ensemble_disagreement(policy._ensemble_dev, eng.to_dev(pb["x0"]), eng.to_dev(pb["U"]),
                                  want=("X",))["X"].cpu().numpy()
    bad = np.zeros(12, bool)
    for layers in [pb["dyn"]] + list(members):
        bad |= gu.dyn_near_kink(vc.f64(layers), X.astype(np.float64), pb["U"].astype(np.float64)).any(1)
    assert (~bad).sum() >= B
    keep = np.flatnonzero(~bad)[:B]
    for k in ("x0", "U", "goal"):
        pb[k] = np.ascontiguousarray(pb[k][keep])
    return policy, params, pb, members, np.ascontiguousarray(X[keep])


def test_g8_the_layers_forward_and_backward():
    from gan_mpc_amd.policy import differentiable as dl
    policy, params, pb, members, _ = _policy_problem(17, 6, 6)
    dparams = policy.to_device_params(params)
    dev = policy.device()
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    flat = dparams.flat.requires_grad_(True)
    x0, U = (t(pb[k]).requires_grad_(True) for k in ("x0", "U"))
    mem = t(ec.flat(members)).requires_grad_(True)

    def loss(d, D):
        return D.mean(0).sum() + 0.5 * D.std(0, unbiased=False).sum() + 0.1 * (d * d).sum()

    try:
        d, D = dl.ensemble_disagreement_layer(policy, dparams, x0, U, members=mem)
        eng = policy._rollout_eng[1]
        direct = eng.ensemble_disagreement(mem.detach(), x0.detach(), U.detach(), want=("X", "d", "D"))
        _same(d.detach().cpu().numpy(), direct["d"].cpu().numpy(), "G8 forward d")
        _same(D.detach().cpu().numpy(), direct["D"].cpu().numpy(), "G8 forward D")
        loss(d, D).backward()
        lo, cnt = dparams.range_of(("dynamics_params",))
        got = dict(x0=x0.grad, U=U.grad, members=mem.grad, nominal=flat.grad[lo:lo + cnt])
        rest = flat.grad.clone()
        rest[lo:lo + cnt] = 0
        assert not rest.any()                                     # costs and mpc_w do not enter
        got = {k: v.cpu().numpy() for k, v in got.items()}
        # a member tensor that does not require grad gets none (and the policy's own ensemble is the default)
        mem2 = mem.detach().clone()
        U2 = U.detach().clone().requires_grad_(True)
        d2, D2 = dl.ensemble_disagreement_layer(policy, dparams, x0.detach(), U2, members=mem2)
        loss(d2, D2).backward()
        assert mem2.grad is None
        _same(U2.grad.cpu().numpy(), got["U"], "G8 U without the members' gradient")
        d3, _ = dl.ensemble_disagreement_layer(policy, dparams, x0.detach(), U.detach())
        _same(d3.detach().cpu().numpy(), d.detach().cpu().numpy(), "G8 the policy's ensemble")
    finally:
        flat.requires_grad_(False)
        flat.grad = None
    # the loss's own backward at the GPU's (d, D), in fp32 as the layer's caller runs it and in fp64 for the arbiter
    Xn, dn, Dn = direct["X"].cpu().numpy(), d.detach().cpu().numpy(), D.detach().cpu().numpy()
    refs = {}
    for dt in (np.float32, np.float64):
        dt_, Dt_ = (torch.as_tensor(a.astype(dt)).requires_grad_(True) for a in (dn, Dn))
        loss(dt_, Dt_).backward()
        refs[dt] = vr.reference(pb["dyn"], members, Xn.astype(dt), pb["U"].astype(dt), dt_.grad.numpy(),
                                Dt_.grad.numpy())
    gu.set_config("ensemble disagreement layer n=17 m=6")
    for key in KEYS:
        e = gu.assert_parity(f"ensemble disagreement layer {key}", got[key], refs[np.float32][key],
                             refs[np.float64][key], **_tol(key))
        print(f"G8 {key}: HIP {e[0]:.3e}, NumPy fp32 {e[1]:.3e}")


def _risk_refs(pb, members, X, aggregate, risk, penalty):
    """{dtype: (R (B,), dR/dU (B, T, m))} of plan_risk(disagreement=penalty) at the nominal rollout X."""
    import disagreement_ref as dr
    import ensemble_rollout_vjp_ref as rvr
    import gan_mpc_oracle as orc
    from test_rollout_vjp_host import reference as rollout_reference
    refs = {}
    for dt in (np.float32, np.float64):
        p = orc.cast_problem(pb, dt)
        Xd = X.astype(dt)
        costs = orc.evaluate(p["cmlp"], p["mpc_w"], p["goal"], Xd, p["U"])
        D = dr.plan(p["dyn"], members, p["x0"], p["U"])["D"]
        J = np.stack([dr.penalised(costs.sum(-1).astype(dt), penalty, D[q]) for q in range(len(members))])
        R, w = rvr.risk(J, aggregate, dt(risk))
        gc = np.ascontiguousarray(np.broadcast_to(w.sum(0)[:, None], costs.shape)).astype(dt)
        g0 = rollout_reference(p, Xd, p["U"], p["goal"], None, gc)["U"]
        gD = (dt(np.float32(penalty)) * w).astype(dt)
        g1 = vr.reference(p["dyn"], members, Xd, p["U"], None, gD)["U"]
        refs[dt] = (R.astype(dt), (g0 + g1).astype(dt))
    return refs


@pytest.mark.parametrize("aggregate,risk", [("mean", 0.0), ("mean_std", 0.5), ("max", 0.0)])
def test_g9_plan_risk_under_the_penalty_against_the_reference(aggregate, risk):
    policy, params, pb, members, X = _policy_problem(17, 6, 6)
    args = (params, pb["x0"], pb["U"], pb["goal"])
    R, g = policy.plan_risk(*args, aggregate=aggregate, risk=risk, grad=True, disagreement=PENALTY)
    only = policy.plan_risk(*args, aggregate=aggregate, risk=risk, disagreement=PENALTY)
    _same(only.cpu().numpy(), R.cpu().numpy(), "G9 R with and without the gradient")
    refs = _risk_refs(pb, members, X, aggregate, risk, PENALTY)
    gu.set_config(f"plan_risk disagreement {aggregate}")
    e = gu.assert_parity(f"plan_risk disagreement R {aggregate}", R.cpu().numpy(), refs[np.float32][0],
                         refs[np.float64][0])
    f = gu.assert_parity(f"plan_risk disagreement dR/dU {aggregate}", g.cpu().numpy(), refs[np.float32][1],
                         refs[np.float64][1])
    print(f"G9 {aggregate}: R HIP {e[0]:.3e} / fp32 {e[1]:.3e}, dR/dU HIP {f[0]:.3e} / fp32 {f[1]:.3e}")
    plain = policy.plan_risk(*args, aggregate=aggregate, risk=risk).cpu().numpy()
    assert gu.rel_err(plain, refs[np.float64][0]) > 1e-3          # the members' own objectives are another quantity
    # disagreement=None is the call without the keyword
    a, ga = policy.plan_risk(*args, aggregate=aggregate, risk=risk, grad=True, disagreement=None)
    b, gb = policy.plan_risk(*args, aggregate=aggregate, risk=risk, grad=True)
    _same(a.cpu().numpy(), b.cpu().numpy(), "G9 disagreement=None R")
    _same(ga.cpu().numpy(), gb.cpu().numpy(), "G9 disagreement=None dR/dU")
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="plan_risk: disagreement must be"):
            policy.plan_risk(*args, disagreement=bad)
        with pytest.raises(ValueError, match="refine_plan: disagreement must be"):
            policy.refine_plan(*args, disagreement=bad)


def test_g9_r_is_the_aggregate_of_the_solvers_plane_costs():
    """The plan as the mean row of Engine.cem_solve(max_iter=0): its obj is the nominal objective J_0 of the sampled
    rollout's arithmetic; with Engine.ensemble_disagreement's D the planes are section 28's J_0 + penalty * D_p (the
    product rounded, then the sum) and R their aggregate -- what a solve under this penalty and aggregate costs the
    row at."""
    import disagreement_ref as dr
    import ensemble_modes_ref as mr
    policy, params, pb, members, _ = _policy_problem(17, 6, 6)
    eng = policy.bind(policy.to_device_params(params), 6)
    d = eng.to_dev
    sol = eng.cem_solve(d(pb["x0"]), d(pb["U"]), d(pb["goal"]), -1.0, 1.0, dict(num_samples=16, elite_portion=0.25, max_iter=0))
    D = eng.ensemble_disagreement(policy._ensemble_dev, d(pb["x0"]), d(pb["U"]), want=("D",))["D"].cpu().numpy()
    _same(sol["U"].cpu().numpy(), pb["U"])
    J0 = sol["obj"].cpu().numpy()
    for aggregate, risk in (("mean", 0.0), ("mean_std", 0.5), ("max", 0.0)):
        want = mr.aggregate([dr.penalised(J0, PENALTY, D[p]) for p in range(3)], aggregate, risk)
        R = policy.plan_risk(params, pb["x0"], pb["U"], pb["goal"], aggregate=aggregate, risk=risk,
                             disagreement=PENALTY).cpu().numpy()
        e = gu.rel_err(R, want)
        print(f"G9 {aggregate}: R against the solver's plane costs {e:.3e}")
        assert e <= 1e-5, (aggregate, e)           # two fp32 evaluations of one sum over T + 1 costs and P planes


@pytest.mark.parametrize("N,M", [(17, 6), (5, 2)])
def test_g9_refine_plan_under_the_penalty_lowers_r_inside_the_bounds(N, M):
    policy, params, pb, _, _ = _policy_problem(N, M, 6)
    args = (params, pb["x0"], pb["U"], pb["goal"])
    kw = dict(aggregate="mean_std", risk=0.5, disagreement=PENALTY)
    U1, R0, R1 = policy.refine_plan(*args, steps=3, **kw)
    R0, R1, U1 = R0.cpu().numpy(), R1.cpu().numpy(), U1.cpu().numpy()
    print(f"G9 refine_plan n={N}: R {R0} -> {R1}")
    assert np.all(R1 <= R0) and np.any(R1 < R0)
    assert U1.shape == pb["U"].shape and np.all(np.abs(U1) <= 1.0)
    again = policy.plan_risk(*args[:2], U1, pb["goal"], **kw).cpu().numpy()
    _same(again, R1, "G9 R_after is the forward call's value at U'")
    U0, Ra, Rb = policy.refine_plan(*args, steps=0, **kw)
    _same(U0.cpu().numpy(), pb["U"], "G9 steps=0")
    _same(Ra.cpu().numpy(), R0)
    _same(Rb.cpu().numpy(), R0)
    # disagreement=None is the call without the keyword
    a = policy.refine_plan(*args, steps=2, aggregate="mean_std", risk=0.5, disagreement=None)
    b = policy.refine_plan(*args, steps=2, aggregate="mean_std", risk=0.5)
    for x, y in zip(a, b):
        _same(x.cpu().numpy(), y.cpu().numpy(), "G9 refine_plan disagreement=None")
