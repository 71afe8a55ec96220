"""The path-integral solver without a GPU: the references of tests/mppi_ref.py against brute
force, the conditions the GPU tests rest on (temperatures that leave the weights non-degenerate, a solve that lowers
the objective, no sample on a bound), the arbiter of the gradient -- float64 autograd of the torch transcription --
against central differences of the NumPy fp64 solve, and the host plumbing: header, ctypes, Engine, policy."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
import mppi_cases as mc
import mppi_ref as mr
from gan_mpc_amd import _lib, engine as E_
from gan_mpc_amd._lib import GmpcError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the references ----------------------------------------------------------------------------------------------
def test_weights_against_a_brute_force_softmax():
    nan, inf = float("nan"), float("inf")
    costs = np.array([[3.0, 1.0, 2.0, 1.0, 7.5],          # a tie at the minimum
                      [nan, 4.0, inf, 2.0, 2.0],           # NaN and +inf get weight 0
                      [nan, nan, nan, nan, nan],           # no finite cost
                      [inf, inf, 5.0, inf, nan]])          # one finite cost: one-hot
    lam = 0.7
    for dt in (np.float32, np.float64):
        w, alive = mr.weights(costs, lam, dt)
        assert w.dtype == dt and alive.tolist() == [True, True, False, True]
        for b in range(4):
            fin = [i for i in range(5) if np.isfinite(costs[b, i])]
            want = np.zeros(5)
            if fin:
                mn = min(costs[b, i] for i in fin)
                for i in fin:
                    want[i] = np.exp(-(costs[b, i] - mn) / np.float64(np.float32(lam)))
            np.testing.assert_allclose(w[b], want, rtol=1e-6 if dt == np.float32 else 1e-14)
    samples = np.arange(4 * 5 * 2 * 1, dtype=np.float64).reshape(4, 5, 2, 1)
    mean = np.full((4, 2, 1), -1.0)
    new, wn = mr.update(samples, costs, mean, lam, 0.25, np.float64)
    w, _ = mr.weights(costs, lam, np.float64)
    for b in (0, 1, 3):
        brute = sum(w[b, s] * samples[b, s] for s in range(5)) / w[b].sum()
        np.testing.assert_allclose(new[b], 0.25 * mean[b] + 0.75 * brute, rtol=1e-14)
        np.testing.assert_allclose(wn[b].sum(), 1.0, rtol=1e-14)
    np.testing.assert_array_equal(new[2], mean[2])          # kept, bit for bit
    assert (wn[2] == 0).all() and wn[0, 1] == wn[0, 3] and wn[3].tolist() == [0, 0, 1, 0, 0]


def test_temperatures_are_their_definition_and_leave_the_weights_non_degenerate():
    """A condition, not a measurement: over the three iterations of every problem of every case the fp64 reference's
    effective sample size 1 / sum w~^2 is >= 3 for at least 90 % of the (problem, iteration) pairs.  Recorded: 76 of 78
    (base's and ragged's second problem fall below in their first iteration)."""
    for name, lam in mc.recompute().items():
        assert abs(lam - mc.TEMPERATURE[name]) <= 1e-9 * lam, name
    ok = total = 0
    for name in mc.CASES:
        _, _, _, t64 = mc.traces(name)
        for it in t64:
            e = mr.ess(it["weights"])
            ok += int((e >= 3).sum())
            total += e.size
    print(f"effective sample size >= 3 on {ok} of {total} (problem, iteration) pairs")
    assert total == 78 and ok >= 0.9 * total


@pytest.mark.parametrize("name", list(mc.CASES))
def test_the_solve_lowers_the_objective_of_the_clipped_start(name):
    _, _, r64, _ = mc.traces(name)
    p = orc.cast_problem(mc.problem(name), np.float64)
    start = orc.objective(p["dyn"], p["cmlp"], p["mpc_w"], p["goal"], np.clip(p["U"], mc.LO, mc.HI), p["x0"])
    ratio = r64["obj"] / start
    print(f"{name}: objective ratios {np.round(ratio, 3).tolist()}")
    assert (ratio < 1).all()


@pytest.mark.parametrize("gname", list(mc.GRAD_CASES))
def test_no_sample_of_a_gradient_case_lies_on_a_bound(gname):
    _, _, _, pre = mc.grad_refs(gname)
    gap = min(float(np.minimum(np.abs(u - mc.LO), np.abs(u - mc.HI)).min()) for u in pre)
    assert gap > 1e-5, gap          # (otherwise: another seed in mppi_cases.py)


def test_numpy_and_torch_forward_agree():
    name, K, more = mc.GRAD_CASES["base_gamma"]
    _, _, fwd, _ = mc.grad_refs("base_gamma")
    r = mr.mppi(mc.problem(name), np.float64, mc.LO, mc.HI, mc.kwargs(name, K, **more), init_std=mc.INIT_STD)
    for a, k in zip(fwd, ("X", "U", "obj")):
        np.testing.assert_allclose(a, r[k], rtol=1e-10, atol=1e-12)


# ---- the arbiter against central differences -------------------------------------------------------------------------
H = 1e-6


def _perturbed(pb, d, h):
    q = dict(pb)
    q["cmlp"] = [(W + h * dW, b + h * db) for (W, b), (dW, db) in zip(pb["cmlp"], d["cmlp"])]
    for k in ("mpc_w", "x0", "goal", "U"):
        q[k] = pb[k] + h * d[k]
    return q


@pytest.mark.parametrize("name", ["base", "m1"])
def test_autograd_against_central_differences(name):
    """d/dh of L_b = <gX, X_b> + <gU, U_b> + gobj_b obj_b along one random direction in (theta, x0, goal, U_init) at
    K = 2: float64 autograd of the torch transcription against central differences of the NumPy fp64 solve.  Steps
    h = H and 2 H with H = 1e-6: the quotient's truncation error is h^2 |d3L| / 6 ~ 1e-12 |d3L| and its rounding error
    1e-16 |L| / h ~ 1e-10 |L|, so the two agree to 1e-5 relative with room for a large third derivative (it grows with
    1 / temperature^3) unless a relu or clamp kink lies inside the step; a problem whose quotient changes by more than
    1e-3 relative between the two steps has one and is left out (at most one per case)."""
    K = 2
    pb = orc.cast_problem(mc.problem(name), np.float64)
    kw = mc.kwargs(name, K)
    gX, gU, gobj = mc.cotangents(name)
    rng = np.random.default_rng(23)
    rnd = lambda a: rng.standard_normal(np.shape(a))  # noqa: E731
    d = dict(cmlp=[(rnd(W), rnd(b)) for W, b in pb["cmlp"]], mpc_w=rnd(pb["mpc_w"]), x0=rnd(pb["x0"]),
             goal=rnd(pb["goal"]), U=rnd(pb["U"]))

    def L(h):
        r = mr.mppi(_perturbed(pb, d, h), np.float64, mc.LO, mc.HI, kw, init_std=mc.INIT_STD)
        return (gX * r["X"]).sum((1, 2)) + (gU * r["U"]).sum((1, 2)) + gobj * r["obj"]

    q1 = (L(H) - L(-H)) / (2 * H)
    q2 = (L(2 * H) - L(-2 * H)) / (4 * H)
    lv = mr.leaves(pb)
    X, U, obj = mr.torch_mppi(lv, mc.LO, mc.HI, kw, mc.INIT_STD)
    Lb = (X * torch.as_tensor(gX)).sum((1, 2)) + (U * torch.as_tensor(gU)).sum((1, 2)) + obj * torch.as_tensor(gobj)
    flat = [lv["mpc_w"], lv["x0"], lv["goal"], lv["U"]] + [a for Wb in lv["cmlp"] for a in Wb]
    dirs = [d["mpc_w"], d["x0"], d["goal"], d["U"]] + [a for Wb in d["cmlp"] for a in Wb]
    auto = np.array([sum(float((g * torch.as_tensor(v)).sum()) for g, v in
                         zip(torch.autograd.grad(Lb[b], flat, retain_graph=True), dirs)) for b in range(pb["B"])])
    smooth = np.abs(q1 - q2) <= 1e-3 * np.abs(q1)
    err = np.abs(auto - q1) / np.abs(q1)
    print(f"{name}: quotients {q1.tolist()}, relative errors {err.tolist()}, smooth {smooth.tolist()}")
    assert (~smooth).sum() <= 1
    assert (err[smooth] <= 1e-5).all()


# ---- the plumbing ----------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()


def _params(fn):
    m = re.search(r"\bint " + fn + r"\((.*?)\);", _header(), re.S)
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_ctypes_and_struct_agree():
    solve = _params("gmpc_mppi_solve")
    assert solve == ["gmpc_ctx* ctx", "int B", "const float* x0", "const float* goal", "const float* u_lo",
                     "const float* u_hi", "const gmpc_mppi_opts* opts", "float* mean_io", "const float* std",
                     "float* X", "float* obj", "float* costs", "float* weights", "float* samples",
                     "float* means_trace", "float* costs_trace", "void* stream"]
    vjp = _params("gmpc_mppi_vjp")
    assert [p.split("*")[-1].strip() if "*" in p else p for p in vjp] == [
        "ctx", "int B", "x0", "goal", "u_lo", "u_hi", "opts", "std", "means_trace", "costs_trace", "U", "X", "gU",
        "gX", "gobj", "grad_x0", "grad_Uinit", "grad_goal", "grad_theta_sum", "grad_dyn_sum", "stream"]
    for name, params in (("gmpc_mppi_solve", solve), ("gmpc_mppi_vjp", vjp)):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params)
        for a, p in zip(args, params):
            opts = C.POINTER(_lib.MppiOpts)
            assert a is (C.c_int if p.startswith("int ") else opts if "gmpc_mppi_opts" in p else C.c_void_p), (name, p)
    m = re.search(r"typedef struct gmpc_mppi_opts \{(.*?)\} gmpc_mppi_opts;", _header(), re.S)
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype = re.match(r"(unsigned long long|int|float)\s", decl).group(1)
            fields += [(x.strip(), ctype) for x in decl[len(ctype):].split(",")]
    ctypes_of = {"int": C.c_int, "float": C.c_float, "unsigned long long": C.c_ulonglong}
    assert [(f, ctypes_of[t]) for f, t in fields] == list(_lib.MppiOpts._fields_)
    assert C.sizeof(_lib.MppiOpts) == 32


def test_keywords_and_options():
    assert E_.MPPI_KWARGS == dict(sampling_smoothing=0.0, evolution_smoothing=0.0, temperature=1.0, max_iter=5,
                                  num_samples=400, seed=0)
    assert set(E_.MPPI_KWARGS) == (set(E_.TRAJAX_CEM_KWARGS) - {"elite_portion"}) | {"temperature"}
    assert mr.DEFAULTS == E_.MPPI_KWARGS
    o = E_.make_mppi_opts(dict(num_samples=33, temperature=0.25, seed=(5 << 32) + 7), iter_offset=3)
    assert (o.max_iter, o.num_samples, o.iter_offset, o.seed) == (5, 33, 3, (5 << 32) + 7)
    assert o.temperature == 0.25 and o.evolution_smoothing == 0.0
    for bad in (dict(elite_portion=0.1), dict(warm_start=True)):
        with pytest.raises(GmpcError, match="mppi: unknown"):
            E_.make_mppi_opts(bad)


class _Recorder:
    """Stands in for the library: records the calls Engine.mppi_solve / mppi_vjp make."""

    def __init__(self):
        self.calls = []

    def gmpc_mppi_solve(self, *args):
        self.calls.append(args)
        return 0

    gmpc_mppi_vjp = gmpc_mppi_solve


def _host_engine(n=3, m=2, T=4):
    eng = E_.Engine.__new__(E_.Engine)
    eng.n, eng.m, eng.T, eng.nx = n, m, T, n
    eng.cost_count, eng.dyn_count, eng.solve_count = 11, 13, 0
    eng.device = torch.device("cpu")
    eng.ctx = None
    eng.lib = _Recorder()
    return eng


def test_engine_passes_the_arguments_in_the_header_order(monkeypatch):
    eng = _host_engine()
    B, n, m, T, N, K = 2, 3, 2, 4, 20, 2
    monkeypatch.setattr(E_, "_ptr", lambda t: None if t is None else t)
    monkeypatch.setattr(E_.Engine, "_stream", lambda self: "stream")
    x0, U, goal = torch.zeros(B, n), torch.full((B, T, m), 0.5), torch.zeros(B, T + 1, n)
    kw = dict(num_samples=N, max_iter=K, seed=9, temperature=0.5)
    out = eng.mppi_solve(x0, U, goal, [-1.0, -2.0], 3.0, kw, want=("samples", "weights"), iter_offset=5, trace=True)
    (ctx, b, a_x0, a_goal, lo, hi, opts, mean, std, X, obj, costs, weights, samples, mtr, ctr, stream), = eng.lib.calls
    assert ctx is None and b == B and a_x0 is x0 and a_goal is goal and stream == "stream"
    assert lo.tolist() == [-1.0, -2.0] and hi.tolist() == [3.0, 3.0]
    o = opts._obj
    assert (o.num_samples, o.max_iter, o.iter_offset, o.seed, o.temperature) == (N, K, 5, 9, 0.5)
    assert mean is out["U"] and mean is not U and torch.equal(mean, U)           # the caller's start is not written
    assert std is out["std"] and torch.equal(std[0, 0], torch.tensor([2.0, 2.5]))   # (hi - lo) / 2 per control
    assert X is out["X"] and tuple(X.shape) == (B, T + 1, n) and obj is out["obj"] and tuple(obj.shape) == (B,)
    assert costs is None and weights is out["weights"] and tuple(weights.shape) == (B, N)
    assert samples is out["samples"] and tuple(samples.shape) == (B, N, T, m)
    assert mtr is out["means_trace"] and tuple(mtr.shape) == (K, B, T, m)
    assert ctr is out["costs_trace"] and tuple(ctr.shape) == (K, B, N)
    plain = eng.mppi_solve(x0, U, goal, None, None, kw, init_std=0.25)
    assert "means_trace" not in plain and eng.lib.calls[-1][14] is None and eng.lib.calls[-1][15] is None
    assert torch.equal(eng.lib.calls[-1][8], torch.full((B, T, m), 0.25)) and eng.lib.calls[-1][4] is None
    # the vjp
    gU, gobj = torch.ones(B, T, m), torch.ones(B)
    g = eng.mppi_vjp(x0, goal, [-1.0, -2.0], 3.0, out, gU=gU, gobj=gobj, kwargs=kw, iter_offset=5, want_goal=False)
    (ctx, b, a_x0, a_goal, lo, hi, opts, a_std, a_mtr, a_ctr, a_U, a_X, a_gU, a_gX, a_gobj, gx0, gUi, gg, gth, gdy,
     stream) = eng.lib.calls[-1]
    assert b == B and a_x0 is x0 and a_goal is goal and lo.tolist() == [-1.0, -2.0] and stream == "stream"
    assert opts._obj.iter_offset == 5 and a_std is out["std"] and a_mtr is mtr and a_ctr is ctr
    assert a_U is out["U"] and a_X is out["X"] and a_gU is gU and a_gX is None and a_gobj is gobj
    assert gx0 is g["x0"] and gUi is g["U"] and gg is None and g["goal"] is None
    assert gth is g["theta"] and tuple(gth.shape) == (3 + 11,) and gdy is g["dyn"] and tuple(gdy.shape) == (13,)
    assert eng.solve_count == 1          # the vjp drops a held solution


def test_host_refusals_come_before_any_call():
    eng = _host_engine()
    B, n, m, T = 2, 3, 2, 4
    x0, U, goal = torch.zeros(B, n), torch.zeros(B, T, m), torch.zeros(B, T + 1, n)
    bad = [
        (dict(u_lo=-1.0, u_hi=None), "mppi: .*init_std"),
        (dict(u_lo=-np.inf, u_hi=1.0), "mppi: .*init_std"),
        (dict(u_lo=1.0, u_hi=-1.0), "u_lo must be <= u_hi"),
        (dict(u_lo=[0.0, 0.0, 0.0], u_hi=1.0), "u_lo must be a scalar or 2 values"),
        (dict(kwargs=dict(elite_portion=0.1)), "mppi: unknown keyword"),
        (dict(want=("elites",)), "mppi: want"),
        (dict(x0=torch.zeros(B, n + 1)), "mppi: x0 must be"),
        (dict(U_init=torch.zeros(B, T + 1, m)), "mppi: U_init must be"),
        (dict(goal=torch.zeros(B, T, n)), "mppi: goal must be"),
    ]
    for change, match in bad:
        args = dict(x0=x0, U_init=U, goal=goal, u_lo=-1.0, u_hi=1.0)
        args.update(change)
        with pytest.raises(GmpcError, match=match):
            eng.mppi_solve(**args)
    sol = dict(U=U, X=torch.zeros(B, T + 1, n), std=U, means_trace=torch.zeros(5, B, T, m),
               costs_trace=torch.zeros(5, B, 400))
    for change, match in [(dict(gU=torch.zeros(B, T)), "mppi_vjp: gU must be"),
                          (dict(gobj=torch.zeros(B, 1)), "mppi_vjp: gobj must be"),
                          (dict(kwargs=dict(max_iter=4)), "mppi_vjp: sol\\['means_trace'\\]"),
                          (dict(kwargs=dict(num_samples=40)), "mppi_vjp: sol\\['costs_trace'\\]"),
                          (dict(sol={k: v for k, v in sol.items() if k != "costs_trace"}), "trace=True")]:
        args = dict(x0=x0, goal=goal, u_lo=-1.0, u_hi=1.0, sol=sol, gU=U)
        args.update(change)
        with pytest.raises(GmpcError, match=match):
            eng.mppi_vjp(**args)
    assert eng.lib.calls == []


# ---- the policy ------------------------------------------------------------------------------------------------------
def _policy(cls, **kw):
    return cls(config=None, cost_model=None, dynamics_model=None, expert_model=None, **kw)


def test_policy_takes_the_solver_with_its_bounds_and_keywords():
    from gan_mpc_amd.gan.js_policy import JS_MPC
    from gan_mpc_amd.policy.base import BaseMPC
    from gan_mpc_amd.policy.eval import EvalMPC
    assert "mppi" in EvalMPC.SOLVERS
    p = _policy(EvalMPC, solver="mppi", control_bounds=(-1.0, 1.0), mppi_kwargs=dict(num_samples=64, warm_start=True))
    assert p.solver == "mppi" and p.control_bounds == (-1.0, 1.0) and p.mppi_solves == 0
    assert p.mppi_kwargs == dict(E_.MPPI_KWARGS, num_samples=64, warm_start=True)
    assert _policy(BaseMPC, solver="mppi", control_bounds=(-1.0, 1.0)).mppi_kwargs == dict(E_.MPPI_KWARGS,
                                                                                         warm_start=False)
    assert _policy(JS_MPC, critic_model=None, solver="mppi", control_bounds=(-1.0, 1.0)).solver == "mppi"
    for kw in (dict(solver="mppi"), dict(solver="mppi", control_bounds=(-1, 0, 1)),
               dict(solver="cem", control_bounds=(-1, 1), mppi_kwargs={}), dict(mppi_kwargs=dict(num_samples=8)),
               dict(solver="mppi", control_bounds=(-1, 1), cem_kwargs={}),
               dict(solver="mppi", control_bounds=(-1, 1), mppi_kwargs=dict(elite_portion=0.1))):
        with pytest.raises(ValueError):
            _policy(EvalMPC, **kw)


def test_training_calls_of_a_mppi_policy_raise_and_name_the_layer():
    from gan_mpc_amd.norm.l2_policy import L2MPC
    from gan_mpc_amd.policy import differentiable as diff
    from gan_mpc_amd.policy import optimizers as opt
    p = _policy(L2MPC, solver="mppi", control_bounds=(-1.0, 1.0))
    hist = np.zeros((2, 3, 4), np.float32)
    for call in (lambda: p.loss_and_grad(hist, None, (None,)), lambda: p.batch_loss(None, hist, None),
                 lambda: diff.ilqr_layer(p, None, None, None, None),
                 lambda: opt.bilevel_optimization(p, None, torch.zeros(2, 4), None, None, 0),
                 lambda: opt._solver(p, None, hold=True)):
        with pytest.raises(NotImplementedError, match="mppi_layer"):
            call()
    assert callable(diff.mppi_layer)


def test_warm_start_shifts_the_previous_controls_and_reset_forgets_them():
    from gan_mpc_amd.policy import optimizers as opt
    from gan_mpc_amd.policy.eval import EvalMPC
    U = torch.arange(2 * 4 * 3, dtype=torch.float32).reshape(2, 4, 3)
    S = opt.shift_warm_start(U)
    assert S.is_contiguous() and torch.equal(S[:, :3], U[:, 1:]) and torch.equal(S[:, 3], U[:, 3])

    class Eng:
        def __init__(self):
            self.starts = []

        def _device_bounds(self, lo, hi):
            return None, None, torch.tensor([lo] * 3), torch.tensor([hi] * 3)

        def mppi_solve(self, x0, U, goal, lo, hi, kw):
            assert "warm_start" not in kw
            self.starts.append((U.clone(), kw["seed"]))
            return dict(U=U + 10.0, X=None, obj=None)

    for warm in (False, True):
        p = _policy(EvalMPC, solver="mppi", control_bounds=(-30.0, 30.0), mppi_kwargs=dict(warm_start=warm, seed=4))
        eng = Eng()
        solve = opt._solver(p, eng)
        x0 = torch.zeros(2, 5)
        first = solve(x0, U, None)
        assert torch.equal(first["U"], torch.clamp(U + 10.0, -30.0, 30.0)) and int(first["iterations"][0]) == 5
        solve(x0, U, None)
        solve(x0, U[:1], None)               # another batch shape: the expert's start
        p.reset_warm_start()
        solve(x0, U, None)
        starts = [s for s, _ in eng.starts]
        assert [seed for _, seed in eng.starts] == [4, 5, 6, 7] and p.mppi_solves == 4
        assert torch.equal(starts[0], U) and torch.equal(starts[2], U[:1]) and torch.equal(starts[3], U)
        assert torch.equal(starts[1], opt.shift_warm_start(first["U"]) if warm else U)
