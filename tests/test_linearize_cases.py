"""The tables of tests/linearize_cases.py against the library's own decisions (gmpc_linearize_route: host code, no GPU):
the cases reach every instantiation k_linearize_mfma<NT, NTF>, every staging combination and every input-GEMM body, the
route boundaries are where the table assumes them, the planned LDS and the pad rows hold at the extremes of what
gmpc_create admits, the checker passes the fp32 model of the kernel and rejects every broken variant of it, and the exact
fill is exact."""

import ctypes as C
import itertools
import os

import numpy as np
import pytest

import linearize_cases as lc
from gan_mpc_amd import _lib
from gan_mpc_amd.engine import linearize_route_of, make_shape


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


def _shape(n, m, hidden, T=3, **kw):
    return make_shape(n, m, T, [n + m] + list(hidden) + [n], [n, 8, 2], **kw)


def _route(lib, n, m, hidden, nsamp=9, strided=None, **kw):
    big = n > 64 or m > 32
    return linearize_route_of(_shape(n, m, hidden, **kw), nsamp, big if strided is None else strided, lib=lib)


def _case_route(lib, c):
    return linearize_route_of(_shape(c.n, c.m, c.hidden, T=c.T), c.nsamp, c.strided, lib=lib)


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_case_takes_the_route_the_table_names(lib, case):
    r = _case_route(lib, case)
    assert r["family"] == "mfma" and r["mfma_ok"]
    assert {k: r[k] for k in case.want} == case.want
    R = case.nsamp * case.n
    assert r["ntiles"] == -(-R // 32) and r["grid"] == min(256, -(-r["ntiles"] // 4))
    assert r["nsmax"] == 32 // case.n + 2 and r["lds"] <= lc.LDS_MAX


def test_table_covers_every_cell(lib):
    rs = [(c, _case_route(lib, c)) for c in lc.CASES]
    inst = {(r["NT"], r["NTF"]) for _, r in rs}
    assert inst == set(itertools.product(range(1, 9), (1, 2, 3, 8)))
    # the small path alone reaches the 24 instantiations with NTF <= 3; NTF = 8 only through large-state engines
    assert {(r["NT"], r["NTF"]) for c, r in rs if not c.big} == set(itertools.product(range(1, 9), (1, 2, 3)))
    assert all(c.big and c.strided and c.samp_add > 0 for c, r in rs if r["NTF"] == 8)
    assert {r["NGF"] for _, r in rs} == {1, 2, 3}
    both = set(itertools.product((0, 1), (0, 1)))
    assert {(r["stage_w1"], r["stage_wl"]) for c, r in rs if c.Lh >= 2} == both
    assert {(r["stage_w1"], r["stage_wl"]) for c, r in rs if c.Lh == 1} == both
    assert {r["stage_w1"] for _, r in rs if r["body"] == "ring"} == {0, 1}
    assert {r["body"] for _, r in rs} == {"single", "ring", "multi"}
    assert {r["body"] for _, r in rs if r["NGF"] > 1} == {"single", "multi"}
    assert {c.Lh for c in lc.CASES} >= {1, 2, 3, 7}
    assert {w for c in lc.CASES for w in c.hidden} >= {1, 31, 32, 33, 255, 256}
    assert any(list(c.hidden) != sorted(c.hidden) and list(c.hidden) != sorted(c.hidden, reverse=True) for c in lc.CASES)
    assert {c.n for c in lc.CASES} >= {1, 2, 17, 31, 32, 33, 64}
    assert {(c.nsamp * c.n) % 32 == 0 for c in lc.CASES} == {True, False}
    # k-loops: gemm_tile / gemm_tile_x4 advance 6 per trip with tails of 1 and 2 k-steps; the ring 12 per trip, its
    # read-ahead reaches furthest behind the operand for Kp % 12 == 2
    tiled = {c.kp(l) % 6 for c, r in rs for l in range(c.Lh) if not (l == 0 and r["body"] == "ring")}
    ring = [c.kp(0) for c, r in rs if r["body"] == "ring"]
    assert tiled == {0, 2, 4} and {k % 6 for k in ring} == {0, 2, 4} and 2 in {k % 12 for k in ring}
    assert any(c.dims[l + 1] % 2 for c in lc.CASES for l in range(c.Lh))
    # the persistent loop wraps: more tiles than 256 workgroups of 4 waves
    assert any(r["ntiles"] > 4 * r["grid"] and r["grid"] == 256 for _, r in rs)
    assert {c.active for c in lc.CASES} == set(lc.ACTIVE_KINDS) and {c.mask for c in lc.CASES} == set(lc.MASK_KINDS)
    assert all(c.nsamp == 3 or c.nsamp == 9 for c in lc.CASES if c.B == 3)


def test_route_boundaries(lib, monkeypatch):
    monkeypatch.delenv("GMPC_LIN", raising=False)
    monkeypatch.delenv("GMPC_BIG_DENSE", raising=False)
    r = lambda *a, **k: _route(lib, *a, **k)                                  # noqa: E731
    # column tiles: hidden widths in steps of 32, n + m in steps of 32 up to three tiles, then groups of eight
    assert [r(5, 3, (w, 7))["NT"] for w in (32, 33, 224, 225, 256)] == [1, 2, 7, 8, 8]
    assert [r(n, 2, (40,))["NTF"] for n in (30, 31, 62, 63)] == [1, 2, 2, 3]
    assert [(x["NTF"], x["NGF"]) for x in (r(64, 32, (40,)), r(65, 32, (40,)), r(250, 6, (128,)), r(251, 6, (128,)),
                                           r(506, 6, (255,)), r(507, 6, (255,)))] == \
        [(3, 1), (8, 1), (8, 1), (8, 2), (8, 2), (8, 3)]
    # bodies
    assert [r(5, 3, h)["body"] for h in ((40,), (40, 40), (40, 40, 40))] == ["single", "ring", "ring"]
    assert [r(40, 3, h)["body"] for h in ((40,), (40, 40))] == ["single", "multi"]
    # staging against the 160 KiB budget: W_1^T first, each when it still fits
    st = lambda *a: (lambda x: (x["stage_w1"], x["stage_wl"]))(r(*a))        # noqa: E731
    assert st(17, 6, (256, 256)) == (0, 1) and st(28, 3, (256, 256)) == (0, 1) and st(29, 3, (256, 256)) == (0, 0)
    assert st(22, 3, (200, 256)) == (1, 0) and st(22, 3, (221, 256)) == (1, 0) and st(22, 3, (222, 256)) == (0, 1)
    assert st(17, 6, (224,)) == (1, 0) and st(16, 6, (224,)) == (1, 1) and st(17, 6, (225,)) == (0, 1)
    assert st(260, 10, (160, 130)) == (0, 0) and st(100, 3, (64, 50)) == (1, 1)  # several groups: W_1^T is never staged
    # the order of the chains
    fam = lambda *a, **k: r(*a, **k)["family"]                               # noqa: E731
    assert fam(17, 6, (200, 200, 200)) == "sparse" and fam(17, 6, (200, 200)) == "sparse"
    assert fam(17, 6, (200, 200), strided=True) in ("sparse", "regs")
    assert fam(17, 6, (128, 128)) == "regs" and fam(17, 6, (64, 64, 64)) == "regs" and fam(17, 6, (64,)) == "mfma"
    assert fam(17, 6, (200, 150)) == "mfma" and fam(33, 1, (200, 200)) == "mfma" and fam(17, 16, (64, 64)) == "mfma"
    assert fam(100, 20, (200, 200)) == "regs" and fam(80, 10, (200, 200)) == "mfma"       # wide form: n + m >= 97
    assert fam(100, 3, (64, 49)) == "lowrank" and fam(100, 3, (64, 50)) == "mfma"
    lstm = make_shape(8 + 2 * 16, 3, 3, [16, 24, 8], [40, 8, 2], dyn_lstm=16, x_size=8)
    assert linearize_route_of(lstm, 9, False, lib=lib)["family"] == "dynl"
    monkeypatch.setenv("GMPC_LIN", "dense")
    assert fam(17, 6, (200, 200, 200)) == "regs" and fam(17, 6, (200, 150)) == "mfma"
    monkeypatch.setenv("GMPC_BIG_DENSE", "1")
    assert fam(100, 3, (64, 49)) == "mfma"


def test_bad_arguments(lib):
    out = (C.c_int * 12)()
    s = _shape(5, 3, (40,))
    assert lib.gmpc_linearize_route(None, 9, 0, out) != 0
    assert lib.gmpc_linearize_route(C.byref(s), 0, 0, out) != 0
    assert lib.gmpc_linearize_route(C.byref(s), 9, 0, None) != 0
    assert lib.gmpc_linearize_route(C.byref(_shape(5, 3, (300,))), 9, 0, out) != 0       # wider than gmpc_create admits
    assert lib.gmpc_linearize_route(C.byref(s), 9, 0, out) == 0
    assert lib.gmpc_linearize_ex(None, 9, None, None, None, 1, 0, None) != 0


def test_lds_and_vector_chain_at_the_extremes(lib):
    """Widths <= 256 and at most 7 hidden layers: the slabs and mask rows of k_linearize_mfma always fit 160 KiB, so the
    matrix-core chain takes every shape gmpc_create admits and the VALU k_linearize is never dispatched."""
    worst = 0
    for n in list(range(1, 65)) + [65, 100, 512, 1024]:
        for hidden in ((256,) * 7, (256,), (1,) * 7, (256, 1, 256)):
            m = 64 if n > 64 else 1
            if n > 2 * hidden[-1]:
                continue                                                   # (the low-rank form)
            x = _route(lib, n, m, hidden)
            assert x["family"] == "mfma" and x["mfma_ok"] and x["lds"] <= lc.LDS_MAX, (n, hidden, x)
            worst = max(worst, x["lds"])
    # (the route's bytes include what was staged into the room left; the slabs and mask rows alone peak at n = 1 with
    # 7 x 256: 1,664 B below the budget)
    assert worst <= lc.LDS_MAX and 4 * ((32 * 257 + 8) * 4 + 7 * 34 * lc.MW * 4) == 162176 <= lc.LDS_MAX
    assert _route(lib, 1, 1, (256,) * 7, nsamp=2 ** 31 - 64, strided=False)["family"] == "valu"      # only past 2^31 rows


def _gemm_tile_reads(Kp):
    """k-steps gemm_tile / gemm_tile_x4 request (each reads operand rows k0 and k0 + 1)."""
    ks, k0 = [0, 2], 0
    while k0 + 6 <= Kp:
        ks += [k0 + 4, k0 + 6, k0 + 8]
        k0 += 6
    return ks


def _ring_reads(Kp):
    ks = [2 * u for u in range(5)]
    for k0 in range(0, Kp, 12):
        ks += [k0 + 2 * (u + 5) for u in range(6)]
    return ks


def test_pad_rows_cover_every_read_ahead():
    """Every padded operand has GMPC_LIN_PADROWS = 24 zero rows behind its K rows, the slab 32 NT + 1 columns per row and
    8 floats (then the tile's mask rows) behind its last row: no GEMM body reads past either for any width 1..256."""
    far_t = far_r = 0
    for K in range(1, 257):
        Kp = (K + 1) & ~1
        t, g = max(_gemm_tile_reads(Kp)) + 1, max(_ring_reads(Kp)) + 1
        assert t <= K + lc.PADROWS - 1 and g <= K + lc.PADROWS - 1
        far_t, far_r = max(far_t, t - K), max(far_r, g - K)
        # the slab as A operand (row 31 of the tile reads furthest): inside the wave's LDS for the narrowest slab that
        # holds K columns and the smallest mask block behind it (two hidden layers, nsmax = 2)
        SK = 32 * ((K + 31) // 32) + 1
        wave_floats = 32 * SK + 8 + 2 * 2 * lc.MW
        assert 31 * SK + g < wave_floats and 31 * SK + t < 32 * SK + 8
    assert (far_t, far_r) == (4, 20)              # rows K + 4 and K + 20 of 24: K odd, and Kp % 12 == 2 for the ring


@pytest.fixture(scope="module")
def built():
    out = {}
    for c in lc.CASES:
        for fill in lc.FILLS:
            Bf = lc.build(c, fill)
            out[c.id, fill] = (Bf, lc.reference(Bf))
    return out


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_checker_passes_the_model_and_exact_fill_is_exact(built, case):
    for fill in lc.FILLS:
        Bf, ref = built[case.id, fill]
        figs = []
        n = lc.check(Bf, ref, lc.model_kernel(Bf), on_figures=figs.append)
        assert n == (0 if case.active == "off" else case.entries if case.active in ("null", "on") else n)
        if case.active != "off":
            assert 0 < n <= case.entries and figs[0]["entries"] == n
            # exact fill: the fp32 model equals fp64 bit for bit (check() compares bits there); normal fill: inside the bound
            assert figs[0]["entry"] == 0.0 if fill == "exact" else figs[0]["entry"] <= 1.0
        # the second parameter set gives other Jacobians: the second gmpc_set_params of the GPU test cannot pass on the first
        ref2 = lc.reference(Bf, which=1)
        lc.check(Bf, ref2, lc.model_kernel(Bf, which=1))
        if case.active != "off" and fill == "normal":      # (what the GPU test asserts of the two launches)
            assert not np.array_equal(lc.model_kernel(Bf).view(np.uint32), lc.model_kernel(Bf, which=1).view(np.uint32))
        if case.id in lc.REPEAT_IDS and fill == "normal":
            with pytest.raises(AssertionError):
                lc.check(Bf, ref2, lc.model_kernel(Bf, which=0))
    # masks differ between neighbouring samples, in bits inside the layers' widths
    Bf = built[case.id, "exact"][0]
    inside = np.concatenate([lc.unpack_bits(Bf.masks[:, l], case.dims[l + 1]) for l in range(case.Lh)], axis=1)
    assert (inside[1:] != inside[:-1]).any(axis=1).all()


@pytest.mark.parametrize("variant", lc.VARIANTS)
def test_checker_rejects_every_broken_kernel(built, variant):
    rejected, missed = [], []
    for c in lc.CASES:
        Bf0 = built[c.id, "exact"][0]
        if not lc.applies(c, variant, Bf0.active):
            # where the variant cannot differ, it does not
            for fill in lc.FILLS:
                Bf, ref = built[c.id, fill]
                assert np.array_equal(lc.model_kernel(Bf, variant).view(np.uint32), lc.model_kernel(Bf).view(np.uint32)), c.id
            continue
        hit = differs = 0
        for fill in lc.FILLS:
            Bf, ref = built[c.id, fill]
            broken = lc.model_kernel(Bf, variant)
            differs += not np.array_equal(broken.view(np.uint32), lc.model_kernel(Bf).view(np.uint32))
            try:
                lc.check(Bf, ref, broken)
            except AssertionError:
                hit += 1
        if hit:
            rejected.append(c.id)
        elif differs:
            missed.append(c.id)
        else:
            # the shape has the feature, but these bits never switch the broken part on: the sparse mask kinds only
            assert c.mask in ("zeros", "unit"), (variant, c.id)
    assert rejected, f"{variant}: no case rejects it"
    # whatever a broken kernel writes differently from the right one, on either fill, the checker refuses
    assert missed == [], f"{variant}: differs on {missed} but the checker lets it pass there"
