"""gmpc_ilqr_solve_fused at the C ABI and the policy interface, without a device: the library exports it, the ctypes
table binds it with gmpc_ilqr_solve's argument types, the header declares it, and EvalMPC rejects an unknown
solver name before anything else happens."""

import ctypes as C
import os
import re

import pytest

from gan_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_fused_solve():
    lib = _lib.load()
    assert hasattr(lib, "gmpc_ilqr_solve_fused")


def test_signature_is_that_of_the_round_based_solve():
    res, args = _lib.SIGNATURES["gmpc_ilqr_solve_fused"]
    res0, args0 = _lib.SIGNATURES["gmpc_ilqr_solve"]
    assert res is res0 is C.c_int
    assert args == args0


def test_header_declares_it_with_the_same_parameters():
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()

    def params(name):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared"
        return [re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1)[0] for p in m.group(1).split(",")]

    assert params("gmpc_ilqr_solve_fused") == params("gmpc_ilqr_solve")


def test_eval_policy_rejects_an_unknown_solver():
    from gan_mpc_amd.policy.eval import EvalMPC
    with pytest.raises(ValueError, match="solver"):
        EvalMPC(config=None, cost_model=None, dynamics_model=None, expert_model=None, solver="bogus")
    assert EvalMPC(config=None, cost_model=None, dynamics_model=None, expert_model=None).solver == "rounds"
