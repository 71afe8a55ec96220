"""The ensemble fit on the GPU (gmpc_dynamics_ensemble_loss_grad): every member's loss and
gradient against the fp64 oracle (F1), member independence (F2), the index gather (F3), the cross-check against
gmpc_dynamics_loss_grad (F4), determinism and the workspace (F5), statelessness (F6), refusals (F7), the trainer (F8)
and the hand-over to a sampling policy (F9).  F2, F3 and F5 are bitwise.

Achieved on MI355X (run with -s: the tests print them; DESIGN.md section 25 lists every case): F1 worst max-norm error
against fp64 over 540 member comparisons 4.9e-7 on the loss and 8.6e-7 on the gradient for HIP, 3.1e-7 and 4.8e-7 for
the NumPy fp32 oracle, every comparison on the 1e-5 branch; F4 at most 1.3e-7 (loss) and 3.6e-7 (gradient) between the two kernels (bound 1e-4); F8
losses 27.18 / 23.75 / 36.68 at the first update and 4.58 / 7.44 / 3.73 at the last, the fp64 reference's figures."""

import functools

import numpy as np
import pytest
import torch

import ensemble_fit_cases as fc
import gpu_util as gu
import sampled_ensemble_cases as ec
from gan_mpc_amd._lib import GmpcError

pytestmark = pytest.mark.gpu

P3 = 3
DATASET = 40       # dataset rows of the indexed form


def _bits(a):
    return a.view(np.uint32)


def _members(eng, name, which=(0, 1, 2)):
    return eng.to_dev(ec.flat([ec.members(name)[p] for p in which]))


def _call(eng, members, data, tf, rows=None):
    d = eng.to_dev
    loss, grad = eng.dynamics_ensemble_loss_grad(members, d(data[0]), d(data[1]), d(data[2]), fc.DISCOUNT, tf, rows=rows)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _gather(data, idx):
    return tuple(np.ascontiguousarray(a[idx]) for a in data)


@functools.lru_cache(maxsize=None)
def _engine(name):
    return fc.new_engine(name)


# ---- F1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("tf", [True, False], ids=["tf", "free"])
@pytest.mark.parametrize("name", fc.NAMES)
def test_f1_every_member_matches_the_fp64_oracle(name, tf, B):
    eng = _engine(name)
    gu.set_config(f"ensemble fit {name} B={B} tf={tf}")
    mem = _members(eng, name)
    worst = [0.0, 0.0]
    for S in fc.STEPS:
        for form in ("identity", "rows"):
            if form == "identity":
                data, rows = fc.data(name, B, S), None
            else:
                data, rows = fc.data(name, DATASET, S), fc.draw_rows(P3, B, DATASET, seed=S)
            loss, grad = _call(eng, mem, data, tf, rows)
            assert loss.shape == (P3,) and grad.shape == (P3, eng.dyn_count)
            for p in range(P3):
                batch = data if rows is None else _gather(data, rows[p])
                l32, g32 = fc.oracle(ec.members(name)[p], *batch, tf, np.float32)
                l64, g64 = fc.oracle(ec.members(name)[p], *batch, tf, np.float64)
                el = gu.assert_parity("ensemble fit loss", loss[p] / B, l32, l64)[0]
                eg = gu.assert_parity("ensemble fit grad", grad[p] / B, g32, g64, tol=1e-5)[0]
                worst = [max(worst[0], el), max(worst[1], eg)]
    print(f"F1 {name} B={B} tf={tf}: loss {worst[0]:.2e}, grad {worst[1]:.2e} against fp64")


# ---- F2, F3 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf", [True, False], ids=["tf", "free"])
@pytest.mark.parametrize("name", fc.NAMES)
def test_f2_f3_a_member_is_its_own_call_and_the_gather_is_exact(name, tf):
    eng = _engine(name)
    B, S = 65, 5
    data, rows = fc.data(name, DATASET, S), fc.draw_rows(P3, B, DATASET, seed=3)
    assert all(len(set(r.tolist())) < B for r in rows)                    # duplicates inside every member
    loss, grad = _call(eng, _members(eng, name), data, tf, rows)
    for p in range(P3):
        one = _members(eng, name, (p,))
        l1, g1 = _call(eng, one, data, tf, rows[p:p + 1])                 # F2: the member alone, its own index row
        np.testing.assert_array_equal(_bits(loss[p:p + 1]), _bits(l1), err_msg=f"F2 loss {p}")
        np.testing.assert_array_equal(_bits(grad[p:p + 1]), _bits(g1), err_msg=f"F2 grad {p}")
        l2, g2 = _call(eng, one, _gather(data, rows[p]), tf)              # F3: the host-gathered batch, no index
        np.testing.assert_array_equal(_bits(loss[p:p + 1]), _bits(l2), err_msg=f"F3 loss {p}")
        np.testing.assert_array_equal(_bits(grad[p:p + 1]), _bits(g2), err_msg=f"F3 grad {p}")
    assert not np.array_equal(grad[0], grad[1])


# ---- F4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf", [True, False], ids=["tf", "free"])
@pytest.mark.parametrize("name", fc.NAMES)
def test_f4_the_vector_kernel_agrees(name, tf):
    pb = ec.problem(name)
    eng = fc.new_engine(name)
    try:
        d = eng.to_dev
        B, S = 33, fc.T
        data, rows = fc.data(name, DATASET, S), fc.draw_rows(P3, B, DATASET, seed=4)
        mem = _members(eng, name)
        loss, grad = _call(eng, mem, data, tf, rows)
        from gan_mpc_amd import params as P
        cost = d(P.pack_mlp(P.layers_to_tree(pb["cmlp"])))
        for p in range(P3):
            eng.set_params(d(pb["mpc_w"]), mem[p].clone(), cost)
            x, u, y = (d(a) for a in _gather(data, rows[p]))
            l0, g0 = eng.dynamics_loss_grad(x, u, y, fc.DISCOUNT, tf)
            el, eg = gu.rel_err(loss[p], l0.cpu().numpy()[0]), gu.rel_err(grad[p], g0.cpu().numpy())
            print(f"F4 {name} tf={tf} member {p}: loss {el:.2e}, grad {eg:.2e} against k_dynfit")
            assert el <= 1e-4 and eg <= 1e-4
    finally:
        eng.close()


# ---- F5 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "cheetah"])
def test_f5_deterministic_and_independent_of_what_the_workspace_held(name):
    S, tf = fc.T, False
    big, small = fc.data(name, DATASET, S), fc.data(name, 7, S)
    rows = fc.draw_rows(P3, 65, DATASET, seed=5)
    eng, fresh = fc.new_engine(name), fc.new_engine(name)
    try:
        a = _call(eng, _members(eng, name), big, tf, rows)
        b = _call(eng, _members(eng, name), big, tf, rows)
        after = _call(eng, _members(eng, name, (1,)), small, tf)          # B 7, P 1 in the grown workspace
        want = _call(fresh, _members(fresh, name, (1,)), small, tf)
    finally:
        eng.close()
        fresh.close()
    for x, y in zip(a + after, b + want):
        np.testing.assert_array_equal(_bits(x), _bits(y))


# ---- F6 ------------------------------------------------------------------------------------------------------------
def test_f6_the_context_keeps_its_state():
    name = "base"
    pb = ec.problem(name)
    assert pb["T"] == fc.T
    B = pb["B"]
    eng = gu.engine_for(pb, max_batch=fc.MAX_BATCH, critic=False)
    try:
        d = eng.to_dev
        x0, U, goal = d(pb["x0"]), d(pb["U"]), d(pb["goal"])
        eng.ilqr_solve(x0, U, goal, {"maxiter": 3})
        eng.set_sampled_ensemble(_members(eng, name))
        kw = ec.engine_kwargs("icem", name, 2)

        def state():
            loss, grad = eng.bilevel_grad(B, 0, desired=d(pb["true_seq"]))
            sol = eng.icem_solve(x0, U, goal, ec.LO, ec.HI, kw, init_std=ec.init_std("icem"), want=("costs",))
            return [loss.cpu().numpy(), grad.cpu().numpy(), sol["U"].cpu().numpy(), sol["costs"].cpu().numpy()]

        before = state()
        mem = eng.to_dev(ec.flat(ec.members(name))[::-1].copy())          # other members than the set ensemble's
        loss, _ = _call(eng, mem, fc.data(name, DATASET, 5), False, fc.draw_rows(P3, 65, DATASET, seed=6))
        assert np.all(np.isfinite(loss))
        after = state()
    finally:
        eng.close()
    for x, y in zip(before, after):
        np.testing.assert_array_equal(_bits(x), _bits(y))


# ---- F7 ------------------------------------------------------------------------------------------------------------
def test_f7_refused_arguments_at_the_c_abi():
    name = "base"
    eng = fc.new_engine(name, max_batch=16)
    try:
        d = eng.to_dev
        B, S = 7, 5
        x, u, y = (d(a) for a in fc.data(name, B, S))
        mem = _members(eng, name)
        rows = d(fc.draw_rows(P3, B, B), dtype=torch.int32)
        loss, grad = eng.new(P3), eng.new(P3, eng.dyn_count)
        lib = eng.lib
        ok = dict(ctx=eng.ctx, P=P3, mem=mem.data_ptr(), D=B, B=B, S=S, x=x.data_ptr(), u=u.data_ptr(), y=y.data_ptr(),
                  rows=rows.data_ptr(), loss=loss.data_ptr(), grad=grad.data_ptr())

        def call(**change):
            a = dict(ok, **change)
            return lib.gmpc_dynamics_ensemble_loss_grad(a["ctx"], a["P"], a["mem"], a["D"], a["B"], a["S"], a["x"],
                                                        a["u"], a["y"], a["rows"], fc.DISCOUNT, 0, a["loss"], a["grad"],
                                                        eng._stream())

        bad = [dict(P=0), dict(P=17), dict(B=0), dict(B=17), dict(S=0), dict(S=fc.T + 1), dict(D=0),
               dict(D=B + 1, rows=None), dict(ctx=None), dict(mem=None), dict(x=None), dict(u=None), dict(y=None),
               dict(loss=None), dict(grad=None)]
        loss.fill_(-1.0)
        for change in bad:
            assert call(**change) == -1, change                           # GMPC_EINVAL
            assert lib.gmpc_last_error().startswith(b"ensemble fit: "), (change, lib.gmpc_last_error())
        torch.cuda.synchronize()
        assert bool((loss == -1.0).all())                                 # nothing was launched
        assert call() == 0 and call(rows=None) == 0                       # (rows is optional)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all())
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["lstm", "n300"])
def test_f7_refused_shapes_carry_the_prefix(case):
    args = dict(lstm=dict(n=3, m=1, dyn_hidden=(16,), dyn_lstm=8), n300=dict(n=300, m=2))[case]
    n, m = args.pop("n"), args.pop("m")
    args.setdefault("dyn_hidden", (32, 32))
    pb = gu.problem(n, m, 3, 2, seed=1, cost_hidden=(16,), cost_fout=4, **args)
    eng = gu.engine_for(pb, critic=False)
    try:
        z = lambda *s: torch.zeros(*s, device=eng.device)
        with pytest.raises(GmpcError, match="error -1: ensemble fit: "):
            eng.dynamics_ensemble_loss_grad(z(2, eng.dyn_count), z(2, 3, eng.n), z(2, 3, m), z(2, 3, eng.n), 0.95, True)
    finally:
        eng.close()


# ---- F8 ------------------------------------------------------------------------------------------------------------
def _train(eng, members0, bootstrap, num_updates=None):
    from gan_mpc_amd import optim
    from gan_mpc_amd.norm import ensemble_trainer as et
    t = fc.TRAIN
    opt = optim.ClipAdam(t["lr"], **fc.ADAM)
    members = eng.to_dev(members0).clone()
    members, state, losses = et.train_params(
        (fc.EnginePolicy(eng), opt), None, members, fc.train_dataset(), t["num_updates"] if num_updates is None
        else num_updates, t["batch_size"], fc.DISCOUNT, t["teacher_forcing_factor"], t["key"], 0, bootstrap=bootstrap)
    return members.cpu().numpy(), state, losses


def _train_engine():
    from gan_mpc_amd.engine import Engine
    t = fc.TRAIN
    return Engine(t["n"], t["m"], fc.T, fc.train_dims(), [t["n"], 6, 4], fc.TRAIN["batch_size"])


def test_f8_the_trainer_lowers_every_members_loss():
    eng = _train_engine()
    try:
        members, state, losses = _train(eng, fc.students(), True)
        print("F8 losses, first and last update:", losses[0], losses[-1])
        assert losses.shape == (fc.TRAIN["num_updates"], fc.TRAIN["P"]) and np.all(np.isfinite(losses))
        assert np.all(losses[-1] < losses[0])
        steps = fc.TRAIN["windows"] // fc.TRAIN["batch_size"]
        assert [s["count"] for s in state] == [fc.TRAIN["num_updates"] * steps] * fc.TRAIN["P"]
        assert not np.array_equal(members[0], members[1])
        same, _, lsame = _train(eng, fc.students(same=True), False)          # one index draw, identical students
        np.testing.assert_array_equal(_bits(same[0]), _bits(same[1]))
        np.testing.assert_array_equal(_bits(same[0]), _bits(same[2]))
        np.testing.assert_array_equal(_bits(lsame[:, 0]), _bits(lsame[:, 2]))
        boot, _, _ = _train(eng, fc.students(same=True), True)               # their own draws: they part
        assert not np.array_equal(boot[0], boot[1]) and not np.array_equal(boot[0], boot[2])
    finally:
        eng.close()


def test_f8_one_member_is_a_loop_of_engine_calls():
    from gan_mpc_amd import trainer_common as tc
    from gan_mpc_amd.norm import ensemble_trainer as et
    t = fc.TRAIN
    eng = _train_engine()
    try:
        got, _, losses = _train(eng, fc.students(1), True, num_updates=3)
        d = eng.to_dev
        X, U, Y = (d(a) for a in fc.train_dataset())
        mem = d(fc.students(1)).clone()
        m, v = torch.zeros_like(mem[0]), torch.zeros_like(mem[0])
        rng, steps, count, want = tc.as_rng(t["key"]), t["windows"] // t["batch_size"], 0, []
        for up in range(1, 4):
            idx = et.draw_indices(rng, t["windows"], steps, 1, t["batch_size"], True)
            tf = up <= 3 * t["teacher_forcing_factor"]
            total = 0.0
            for s in range(steps):
                loss, grad = eng.dynamics_ensemble_loss_grad(mem, X, U, Y, fc.DISCOUNT, tf, rows=idx[s])
                total = total + loss
                count += 1
                eng.adam_clip_step(mem[0], grad[0], m, v, count, t["lr"], 1.0 / t["batch_size"], **fc.ADAM)
            want.append((total * ((1.0 / t["batch_size"]) / steps)).cpu().numpy())
        np.testing.assert_array_equal(_bits(got), _bits(mem.cpu().numpy()))
        np.testing.assert_array_equal(_bits(losses), _bits(np.stack(want).astype(np.float32)))
    finally:
        eng.close()


# ---- F9 ------------------------------------------------------------------------------------------------------------
def test_f9_trained_members_go_to_an_icem_policy():
    import test_gpu_mirror as mirror
    from gan_mpc_amd import optim
    from gan_mpc_amd.norm import ensemble_trainer as et, l2_policy
    bound = 0.3
    N, M = 17, 6
    config, policy, params, data = mirror._build(functools.partial(
        l2_policy.L2MPC, solver="icem", control_bounds=(-bound, bound), icem_kwargs=dict(num_samples=64, max_iter=3, seed=7)),
        N=N, M=M)

    def act():
        """The action of sample 2 under seed + 0, nothing carried over from an earlier solve."""
        policy.reset_warm_start()
        policy.icem_solves = 0
        policy.expert_model.select(np.array([2]))       # (the table expert serves one call per selection)
        return policy.get_optimal_action(params, data["hist"][2]).cpu().numpy()

    a0 = act()
    # three members from their own seeds, a few steps on windows of the nominal model's own predictions
    members = et.init_members(policy, (config.seed, M), 3, seed=50)
    assert tuple(members.shape) == (3, policy._engine.dyn_count)
    rng = np.random.default_rng(9)
    S, D = 3, 32
    X = rng.standard_normal((D, S, N)).astype(np.float32)
    U = np.tanh(rng.standard_normal((D, S, M))).astype(np.float32)
    eng = policy._engine
    step = lambda c, t: eng.predict(eng.to_dev(X[c:c + 8, t]), eng.to_dev(U[c:c + 8, t])).cpu().numpy()
    Y = np.stack([np.concatenate([step(c, t) for c in range(0, D, 8)]) for t in range(S)], axis=1)   # (max_batch 8)
    members, _, losses = et.train_params((policy, optim.ClipAdam(1e-2)), None, members, (X, U, Y), 3, 8, 0.95, 1.0, 1, 0)
    assert losses.shape == (3, 3) and np.all(np.isfinite(losses))
    policy.set_dynamics_ensemble(members)
    a1 = act()
    assert tuple(policy._engine._ensemble.shape) == (3, policy._engine.dyn_count)
    assert a1.shape == (M,) and np.all(np.isfinite(a1)) and np.all(np.abs(a1) <= np.float32(bound))
    assert not np.array_equal(a0, a1)
    trees = et.members_to_trees(members, params["dynamics_params"])
    policy.set_dynamics_ensemble(trees)                                   # the same members as trees: the same action
    np.testing.assert_array_equal(_bits(act()), _bits(a1))
    policy.set_dynamics_ensemble(None)
    np.testing.assert_array_equal(_bits(act()), _bits(a0))
