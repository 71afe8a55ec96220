"""The weight-gradient GEMMs (csrc/gmpc_wgrad.hip) through gmpc_wgrad_ex / gmpc_wgrad_batch_ex: every kernel form and
launcher path -- the VALU kernel, k_wgrad_mfma<1|2|4|8> on (A, B) and on swapped operands, the column sums alone, the
batch kernel with its own reduction -- each against the fp64 product of the same fp32 operands: bit for bit on the
integer fill, within (rows + 8) 2^-24 sum |a||b| per entry on the normal one.  Operands are allocations with NaNs
wherever the contract does not let the kernel read, +-1e30 in the pad rows it may read, index-carrying NaNs wherever it
may not write and guard words around the partial-sum buffer (tests/wgrad_cases.py: tables, buffers, reference and
checker, themselves checked without a GPU by tests/test_wgrad_cases.py)."""

import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as gu
import wgrad_cases as wc
from gan_mpc_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    # the engine of test_gpu_bgemm: the entry points only need a ctx and its stream
    pb = gu.problem(5, 2, 8, 7, seed=11, dyn_hidden=(33, 47), cost_hidden=(24,), cost_fout=6)
    e = gu.engine_for(pb, critic=False)
    yield e
    e.close()


def _bits(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy())           # bits, not values: NaN payloads


def _launch(eng, Bf, times=1, one_by_one=False):
    """The case's buffers on the device; `times` launches, each from the pre-fill -> what check() takes, per launch.
    one_by_one: the problems of a batch through gmpc_wgrad_ex instead, each with a roomy buffer of its own."""
    c = Bf.case
    held, pre = {}, {}

    def ptr(name, array, offset):
        pre[name] = _bits(array)
        held[name] = pre[name].to(eng.device)
        return held[name].data_ptr() + 4 * offset

    n = len(c.probs)
    descs = (_lib.WgradDesc * n)()
    part = wc.fill_descs(descs, Bf, ptr)
    if c.kind == "single":
        assert wc.route_of(eng.lib, descs[0])[0] == c.route
    else:
        assert wc.batch_route_of(eng.lib, descs, n, c.part_floats) == c.rpc
    if one_by_one:
        roomy = [eng.new(32 * (p.M * p.N + p.N)) for p in c.probs]
        for d, p, buf in zip(descs, c.probs, roomy):
            d.part, d.part_floats, d.mfma_ok = buf.data_ptr(), buf.numel(), 1
            if p.M == 0:
                d.form, d.rows = 1, p.cs_rows
    outs = []
    for i in range(times):
        if i:
            for name in held:
                if name[0] in "Cc" or name == "part":
                    held[name].copy_(pre[name])
        taken = C.c_int(1)
        if c.kind == "single" or one_by_one:
            for d in descs:
                _lib.check(eng.lib.gmpc_wgrad_ex(eng.ctx, C.byref(d), eng._stream()))
        else:
            _lib.check(eng.lib.gmpc_wgrad_batch_ex(eng.ctx, descs, n, C.c_void_p(part), c.part_floats, eng._stream(),
                                                   C.byref(taken)))
        back = lambda name: held[name].cpu().numpy().view(np.float32) if name in held else None      # noqa: E731
        outs.append(dict(C=[back(f"C{j}") for j in range(n)], cs=[back(f"cs{j}") for j in range(n)],
                         part=back("part"), taken=bool(taken.value)))
    return outs


def _kernel(case):
    if case.kind == "batch":
        return "k_wgrad_batch rpc %d" % case.rpc
    form, ntw = case.route[:2]
    return {"valu": "k_wgrad", "colsum": "k_colsum"}.get(form) or \
        ("k_wgrad_mfma<%d>" % ntw) + (" swapped" if form == "mfma_swapped" else "")


@pytest.mark.parametrize("case", wc.CASES, ids=[c.id for c in wc.CASES])
def test_wgrad_case(eng, case):
    repeat = case.id in wc.REPEAT_IDS
    exact = None
    for fill in wc.FILLS:
        Bf = wc.build(case, fill)
        ref = wc.reference(Bf)
        outs = _launch(eng, Bf, times=2 if repeat else 1)

        def record(fig):
            ok = fig["max_rel"] <= (0.0 if fill == "exact" else gu.TOL) and fig["entry"] <= (0.0 if fill == "exact" else 1.0)
            print(f"{case.id} {fill}: {_kernel(case)} max-norm {fig['max_rel']:.3e}, per-entry {fig['entry']:.3f} of "
                  "(rows + 8) u S")
            gu._record(dict(stage=f"wgrad {_kernel(case)}, {fill} fill: max-norm | per-entry error / ((rows + 8) 2^-24 S) "
                                  "in el_hip (exact fill: both must be 0)",
                            config=case.id, e_hip=fig["max_rel"], tol=gu.TOL, tol_used=0.0 if fill == "exact" else gu.TOL,
                            branch="tol", el_hip=fig["entry"], el_used=0.0 if fill == "exact" else 1.0,
                            entries=fig["entries"], passed=bool(ok)))

        wc.check(Bf, ref, outs[0], tol=gu.TOL, on_figures=record)
        if repeat:
            # partial sums per chunk, added in chunk order, no atomics: the same launch again gives the same bits
            for what in ("C", "cs"):
                for a, b in zip(outs[0][what], outs[1][what]):
                    assert (a is None and b is None) or np.array_equal(a.view(np.uint32), b.view(np.uint32))
        if fill == "exact":
            exact = (Bf, ref, outs[0])
    if case.kind == "batch" and not case.declines and len(case.probs) <= wc.WG_MAX:
        # the same problems one by one: on the exact fill both paths give the same bits
        Bf, ref, batch = exact
        single = _launch(eng, Bf, one_by_one=True)[0]
        wc.check(Bf, ref, single, tol=gu.TOL)
        for what in ("C", "cs"):
            for a, b in zip(batch[what], single[what]):
                assert (a is None and b is None) or np.array_equal(a.view(np.uint32), b.view(np.uint32))
