"""The batched TN GEMM family (csrc/gmpc_bgemm.hip) through gmpc_bgemm_tn_ex: every kernel instantiation the dispatcher
can launch and every option the large-state pass sets on BgemmArgs, each against the fp64 product of the same fp32
operands.  Operands are allocations with NaNs wherever the contract does not let the kernel read and index-carrying
NaNs wherever it may not write (tests/bgemm_cases.py: table, buffers, reference and checker, themselves checked without
a GPU by tests/test_bgemm_cases.py)."""

import ctypes as C

import numpy as np
import pytest
import torch

import bgemm_cases as bc
import gpu_util as gu
from gan_mpc_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    # the engine of test_gpu_parity's "tiny-ragged": the GEMM entry point only needs a ctx and its stream
    pb = gu.problem(5, 2, 8, 7, seed=11, dyn_hidden=(33, 47), cost_hidden=(24,), cost_fout=6)
    e = gu.engine_for(pb, critic=False)
    yield e
    e.close()


def _launch(eng, B, times=1):
    """The case's buffers on the device, `times` launches from the same pre-fill -> the C allocations read back."""
    held = {}

    def ptr(name, array, offset):
        a = np.ascontiguousarray(array)
        held[name] = torch.from_numpy(a.view(np.int32).copy()).to(eng.device)       # bits, not values: NaN payloads
        return held[name].data_ptr() + 4 * offset

    desc = bc.fill_desc(_lib.BgemmDesc(), B, ptr)
    assert bc.route_of(eng.lib, desc) == B.case.route
    outs = []
    for i in range(times):
        if i:
            held["C"].copy_(torch.from_numpy(B.prefill.view(np.int32).copy()))
        _lib.check(eng.lib.gmpc_bgemm_tn_ex(eng.ctx, C.byref(desc), eng._stream()))
        outs.append(held["C"].cpu().numpy().view(np.float32))
    return outs


@pytest.mark.parametrize("case", bc.CASES, ids=[c.id for c in bc.CASES])
def test_bgemm_case(eng, case):
    B = bc.build(case)
    ref, S = bc.reference(B)
    repeat = case.id in bc.REPEAT_IDS
    outs = _launch(eng, B, times=2 if repeat else 1)
    route = "k_bgemm_tn<%d>" % case.route[1] if case.family == "strips" else \
        ("k_bthin<%d,%d,10,%d>" if case.family == "thin" else "k_bgemm_tn_lds<2,%d,%d,%d>") % case.route[1:]

    def record(fig):
        ok = fig["max_rel"] <= gu.TOL and fig["entry"] <= 1.0
        print(f"{case.id}: {route} max-norm {fig['max_rel']:.3e}, per-entry {fig['entry']:.3f} of (K + 4) u S")
        gu._record(dict(stage=f"bgemm {route}: max-norm | per-entry error / ((K + K2 + K3 + 4) 2^-24 S) in el_hip",
                        config=case.id, e_hip=fig["max_rel"], tol=gu.TOL, tol_used=gu.TOL, branch="tol",
                        el_hip=fig["entry"], el_used=1.0, entries=fig["entries"], passed=bool(ok)))

    bc.check(B, ref, S, outs[0], tol=gu.TOL, on_figures=record)
    if repeat:
        # no atomics in this unit: the same launch again gives the same bits
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
