"""CPU-side checks of the batched TN GEMM sweep (tests/bgemm_cases.py): the table reaches every kernel instantiation the
dispatcher can launch (gmpc_bgemm_route: host code, no GPU), the route boundaries are where the table assumes them, the
buffers honour the contract's pad rules, and the checker rejects kernels that are wrong in the ways the whole-solve
parity tests would let pass."""

import ctypes as C
import os

import numpy as np
import pytest

import bgemm_cases as bc
from gan_mpc_amd import _lib

IDS = [c.id for c in bc.CASES]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


_BUILT = {}


def built(case):
    """(buffers, ref, S) of a case, computed once for the module and never written to."""
    if case.id not in _BUILT:
        B = bc.build(case)
        _BUILT[case.id] = (B,) + bc.reference(B)
    return _BUILT[case.id]


def _fake_ptr(name, array, offset):
    return 0x10000 + 4 * offset


def _route(lib, M, N, K, batch=1, **kw):
    d = _lib.BgemmDesc()
    d.batch, d.M, d.N, d.K = batch, M, N, K
    d.X = d.Y = d.C = 0x10000
    d.ldx, d.ldy, d.ldc = M, N, N
    d.alpha = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    if d.K2:
        d.X2, d.Y2, d.ldx2, d.ldy2 = 0x10000, 0x10000, M, N
    return bc.route_of(lib, d)


def test_table_reaches_every_instantiation(lib):
    seen = {}
    for c in bc.CASES:
        B = built(c)[0]
        got = bc.route_of(lib, bc.fill_desc(_lib.BgemmDesc(), B, _fake_ptr))
        assert got == c.route, f"{c.id}: the dispatcher takes {got}, the table says {c.route}"
        seen.setdefault(got, []).append(c.id)
    assert len(bc.ALL_ROUTES) == 17 and set(seen) == set(bc.ALL_ROUTES), set(bc.ALL_ROUTES) ^ set(seen)
    # every instantiation by a plain product too, not only through an option
    plain = {c.route for c in bc.CASES if c.group == "plain"}
    assert plain == set(bc.ALL_ROUTES)


def test_table_has_what_the_sweep_promises():
    by = lambda pred: [c for c in bc.CASES if pred(c)]                      # noqa: E731
    for fam in bc.FAMILIES:
        assert by(lambda c: c.family == fam and c.window and not c.share)
        assert by(lambda c: c.family == fam and c.share == "x") and by(lambda c: c.family == fam and c.share == "y")
        a = by(lambda c: c.family == fam and c.active is not None)
        assert a and all(c.active[0] == 0 and c.active[-1] == 0 and 0 in c.active[1:-1] and 1 in c.active for c in a)
        for pair in bc.PAIRS:
            assert by(lambda c: c.family == fam and (c.alpha, c.beta) == pair)
    for c in bc.CASES:
        assert c.batch >= 2
        if c.route[:3] == ("thin", 1, 4) or c.route[:3] == ("thin", 0, 4):
            assert c.share == ("x" if c.route[1] else "y")                  # the wide operand is shared
    for r in bc.ALL_ROUTES:
        Ks = sorted({c.K for c in bc.CASES if c.route == r and c.group == "plain"})
        if r[0] == "lds":
            kc = r[2]
            assert any(k < kc for k in Ks) and {kc, 2 * kc, 2 * kc + 1} <= set(Ks), (r, Ks)
        else:
            assert any(k % 2 for k in Ks) and any(k % 2 == 0 for k in Ks), (r, Ks)
        if r[0] == "thin":
            assert 2 * bc.BT_RD in Ks and any(2 * bc.BT_RD < k < 3 * bc.BT_RD for k in Ks), (r, Ks)
    # the three ragged shifts of the 16-byte streaming form
    assert {c.M % 4 for c in bc.CASES if c.route == ("thin", 1, 4, 1)} >= {1, 2, 3}
    assert {n for n in (70, 128, 130, 196, 257, 260)} == {c.M for c in bc.CASES if c.upper and c.family == "lds"}


def test_route_boundaries(lib):
    r = lambda *a, **k: _route(lib, *a, **k)                                # noqa: E731
    # the streaming kernel needs K >= 2 BT_RD
    assert r(130, 5, 19) == ("strips", 1) and r(130, 5, 20) == ("thin", 1, 2, 1)
    assert r(7, 131, 19) == ("strips", 4) and r(7, 131, 20) == ("thin", 0, 2, 1)
    assert r(127, 5, 33) == ("strips", 1) and r(128, 5, 33) == ("thin", 1, 2, 1)
    assert r(128, 32, 33) == ("thin", 1, 2, 1) and r(128, 33, 33) == ("thin", 1, 2, 2)
    assert r(128, 64, 33) == ("thin", 1, 2, 2) and r(128, 65, 33)[0] == "lds"
    # the LDS-staged kernel: M > 32 and N > 64
    assert r(32, 70, 9) == ("strips", 2) and r(33, 70, 9) == ("lds", 2, 8, 0)
    assert r(40, 64, 9) == ("strips", 2) and r(40, 65, 9) == ("lds", 2, 8, 0)
    # 128 columns per wave from 4096 waves on (and never with two strips)
    assert r(131, 5, 21, batch=2047) == ("thin", 1, 2, 1) and r(131, 5, 21, batch=2048) == ("thin", 1, 4, 1)
    assert r(128, 5, 21, batch=4095) == ("thin", 1, 2, 1) and r(128, 5, 21, batch=4096) == ("thin", 1, 4, 1)
    assert r(5, 130, 23, batch=2047) == ("thin", 0, 2, 1) and r(5, 130, 23, batch=2048) == ("thin", 0, 4, 1)
    assert r(131, 33, 21, batch=4096) == ("thin", 1, 2, 2)
    # block width: the one that pads N least, ties to the widest
    widths = {n: r(129, n, 5)[1] for n in (128, 129, 192, 193, 256, 257)}
    assert widths == {128: 2, 129: 3, 192: 3, 193: 4, 256: 4, 257: 3}
    assert r(132, 128, 5) == ("lds", 2, 8, 1) and r(132, 192, 5) == ("lds", 3, 16, 1) and r(132, 256, 5) == ("lds", 4, 16, 1)
    assert r(132, 130, 5) == ("lds", 3, 8, 0) and r(130, 132, 5) == ("lds", 3, 8, 0)
    # upper-only: by the area of the blocks that are not skipped
    up = {n: r(n, n, 9, upper_only=1, K2=6)[1:] for n in (128, 130, 196)}
    assert up == {128: (2, 8, 1), 130: (3, 8, 0), 196: (2, 8, 1)}
    assert r(196, 196, 9, K2=6)[1] == 4                    # the same shape as a full product
    # an option routes to the LDS-staged kernel whatever the shape; upper_only alone does not
    assert r(5, 3, 4) == ("strips", 1) and r(5, 3, 4, K2=3) == ("lds", 2, 8, 0)
    assert r(5, 3, 4, E=0x10000, lde=3, En=3) == ("lds", 2, 8, 0) and r(5, 3, 4, rowmask=0x10000, srm=1) == ("lds", 2, 8, 0)
    assert r(130, 5, 33, rowmask=0x10000, srm=5) == ("lds", 2, 8, 0)
    assert r(20, 20, 7, upper_only=1) == ("strips", 1)
    assert r(130, 130, 33, upper_only=1)[0] == "lds"


def test_route_query_checks_its_arguments(lib):
    d = _lib.BgemmDesc()
    out = (C.c_int * 4)()
    assert lib.gmpc_bgemm_route(C.byref(d), out) != 0                     # null operands
    d = bc.fill_desc(_lib.BgemmDesc(), built(bc.CASES[0])[0], _fake_ptr)
    assert lib.gmpc_bgemm_route(C.byref(d), out) == 0
    assert lib.gmpc_bgemm_route(C.byref(d), None) != 0
    d.ldy = d.N - 1
    assert lib.gmpc_bgemm_route(C.byref(d), out) != 0
    assert lib.gmpc_bgemm_tn_ex(None, C.byref(d), None) != 0              # no ctx: rejected before any GPU call


@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_buffers_follow_the_contract(case):
    B, ref, S = built(case)
    c = case
    act = np.flatnonzero(B.act)
    # the reference is finite where something is compared, the bound's scale covers it
    assert np.isfinite(ref[act]).all() and np.isfinite(S[act]).all() and (np.abs(ref[act]) <= S[act] * (1 + 1e-12)).all()
    ops = [o for _, X, Y in B.seg for o in (X, Y)] + ([B.E] if B.E is not None else [])
    for o in ops + [B.Cop]:
        nb = 1 if o.stride == 0 else o.batch
        assert o.ld >= o.width and (o.stride == 0 or o.stride >= o.rows * o.ld)
        assert o.off + (nb - 1) * o.stride + (o.rows - 1) * o.ld + o.width <= o.size
        if c.window:
            assert o.ld % 2 == 1 and o.ld > o.width and o.off > 0 and (o.stride == 0 or o.stride > o.rows * o.ld)
    for o in ops:
        # finite exactly inside the logical matrices of the active elements (all of a shared operand)
        inside = np.zeros(o.size, bool)
        for b in ([0] if o.stride == 0 else act):
            inside[o.idx(b).ravel()] = True
        assert np.isfinite(o.a[inside]).all() and np.isnan(o.a[~inside]).all()
    # the K-segments' leading dimensions differ
    assert len({X.ld for _, X, _ in B.seg}) == len(B.seg) == len({Y.ld for _, _, Y in B.seg})
    for K, X, Y in B.seg:
        nb = 1 if Y.stride == 0 else Y.batch
        assert Y.size - (Y.off + (nb - 1) * Y.stride + K * Y.ld) >= bc.y_pad(Y.ld) >= 8 * Y.ld
    if c.family == "strips":
        # what the strips read of the LAST element's Y lies inside the allocation
        K, X, Y = B.seg[0]
        nb = 1 if Y.stride == 0 else Y.batch
        assert Y.off + (nb - 1) * Y.stride + bc.strips_y_extent(K, Y.ld, c.N, c.route[1]) <= Y.size
    # C: finite exactly where beta reads it, a NaN that names its own place everywhere else
    cin = np.zeros(B.Cop.size, bool)
    if c.beta != 0.0:
        cin[B.Cop.idx()[act].ravel()] = True
    assert np.isfinite(B.prefill[cin]).all() and np.isnan(B.prefill[~cin]).all()
    bits = B.prefill.view(np.uint32)[~cin]
    assert bits.size == np.unique(bits).size or B.Cop.size > 0x3FFFFE
    if c.upper:
        # the driver's upper-only products are symmetric
        assert c.M == c.N and np.abs(ref[act] - np.swapaxes(ref[act], 1, 2)).max() <= 1e-5 * np.abs(ref[act]).max()
    if c.mask == "words":
        first = int(act[0])
        assert not bc.mask_rows(B, first)[:32].any() and bc.mask_rows(B, first)[32:64].all()


@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_fp32_numpy_product_passes(case):
    """The contract followed in fp32 NumPy passes the checker: the per-entry bound is no tighter than fp32 itself."""
    B, ref, S = built(case)
    fig = bc.check(B, ref, S, bc.model_kernel(B))
    assert fig["max_rel"] <= 1e-5 and fig["entry"] <= 1.0
    if case.upper:
        bc.check(B, ref, S, bc.model_kernel(B, "lower_hole"))      # a lower entry left at its pre-fill is allowed


@pytest.mark.parametrize("variant", bc.VARIANTS)
def test_checker_rejects(variant):
    """Every broken kernel is rejected on EVERY case where it differs from the contract (hence on at least one per
    family that has the feature)."""
    hit = []
    for case in bc.CASES:
        if not bc.applies(case, variant) or case.batch > 64:
            continue
        B, ref, S = built(case)
        with pytest.raises(AssertionError):
            bc.check(B, ref, S, bc.model_kernel(B, variant))
        hit.append(case)
    assert hit, f"no case exercises {variant}"
    if variant in ("drop_last_col", "extra_col", "y_pad_row", "write_inactive"):
        assert {c.family for c in hit} == set(bc.FAMILIES)
