"""CPU-side checks of the weight-gradient sweep (tests/wgrad_cases.py): the tables reach every route the launchers can
take (gmpc_wgrad_route / gmpc_wgrad_batch_route: host code, no GPU), the route boundaries are where the tables assume
them, no route plans to write more of `part` than it holds, the buffers honour the pad rules of the contract, and the
checker rejects kernels that are wrong in the ways the trainers' parity tests would let pass."""

import ctypes as C
import os

import numpy as np
import pytest

import wgrad_cases as wc
from gan_mpc_amd import _lib

IDS = [c.id for c in wc.CASES]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


_BUILT = {}


def built(case, fill):
    """(buffers, reference) of a case and fill, computed once for the module and never written to."""
    if (case.id, fill) not in _BUILT:
        Bf = wc.build(case, fill)
        _BUILT[case.id, fill] = (Bf, wc.reference(Bf))
    return _BUILT[case.id, fill]


def _fake_ptr(name, array, offset):
    return 0x10000 + 4 * offset


def _descs(case):
    Bf = built(case, "exact")[0]
    d = (_lib.WgradDesc * len(case.probs))()
    wc.fill_descs(d, Bf, _fake_ptr)
    return d


def _route(lib, rows, M, N, cs_rows=None, part_floats=1 << 24, mfma_ok=True, form=0):
    d = _lib.WgradDesc()
    d.rows, d.M, d.N, d.lda, d.ldb = rows, M, N, max(M, 1), N
    d.A = d.B = d.C = d.part = 0x10000
    if form == 1:
        d.colsum = 0x10000
    if cs_rows is not None:
        d.colsum, d.cs_rows = 0x10000, cs_rows
    d.mfma_ok, d.form, d.part_floats = int(mfma_ok), form, part_floats
    return wc.route_of(lib, d)


def _batch_route(lib, shapes, part_floats=1 << 24, ldb=None, b=0x10000):
    d = (_lib.WgradDesc * len(shapes))()
    for q, (rows, M, N) in zip(d, shapes):
        q.rows, q.M, q.N, q.lda, q.ldb = rows, M, N, max(M, 1), ldb or N
        q.A = q.C = 0x10000
        q.B = b
        if M == 0:
            q.colsum, q.cs_rows, q.C = 0x20000, rows, 0x20000
    return wc.batch_route_of(lib, d, len(shapes), part_floats)


def test_table_reaches_every_route(lib):
    seen = {}
    for c in wc.SINGLE:
        got, _ = wc.route_of(lib, _descs(c)[0])
        assert got == c.route, f"{c.id}: the launcher takes {got}, the table says {c.route}"
        seen.setdefault(got[:2], []).append(c)
    # the routes gmpc_wgrad_route can return: the VALU kernel, k_wgrad_mfma<1|2|4|8> on (A, B) and on swapped operands,
    # the column sums alone
    assert len(wc.ALL_ROUTES) == 10 and set(seen) == set(wc.ALL_ROUTES), set(wc.ALL_ROUTES) ^ set(seen)
    # every route by a case with M, lda, cs_rows and the buffer at their plain values too
    assert {r for r, cs in seen.items() if any(c.plain for c in cs)} == set(wc.ALL_ROUTES)
    for c in wc.BATCH:
        d = _descs(c)
        got = wc.batch_route_of(lib, d, len(c.probs), c.part_floats)
        assert got == c.rpc, f"{c.id}: the batch launcher gives rows per chunk {got}, the table says {c.rpc}"
    assert {c.rpc for c in wc.BATCH} == {0, 64, 96, 128}


def test_table_has_what_the_sweep_promises():
    by = lambda pred: [c for c in wc.SINGLE if pred(c)]                     # noqa: E731
    p0 = lambda c: c.probs[0]                                               # noqa: E731
    mf = by(lambda c: c.family == "mfma")
    assert {p0(c).N for c in mf} >= {32, 96, 160, 64, 192, 128, 384, 256}
    assert {p0(c).rows for c in mf} >= {64, 65, 66, 70, 72, 76, 127, 129, 191}
    assert {p0(c).M for c in mf} >= {1, 31, 32, 33, 64, 70}
    # with 64 rows per chunk: last chunks of 1, 2, 6, 8, 12 and 63 rows, every Kp % 6
    tails = {p0(c).rows - (c.route[3] - 1) * c.route[2] for c in mf if c.route[2] == 64}
    assert tails >= {1, 2, 6, 8, 12, 63} and {((t + 1) & ~1) % 6 for t in tails} == {0, 2, 4}
    assert any(p0(c).odd_b and p0(c).ldb % 2 == 1 and p0(c).b_off % 2 == 1 for c in mf)
    sw = by(lambda c: c.family == "mfma_swapped")
    assert {p0(c).M for c in sw} >= {32, 64, 96, 256} and {p0(c).rows for c in sw} == {64, 65, 129}
    assert all(p0(c).N == 1 for c in sw)
    va = by(lambda c: c.family == "valu")
    assert {p0(c).rows for c in va} >= {1, 15, 16, 17, 63, 513, 1025}
    assert {p0(c).N for c in va} >= {1, 3, 33, 65, 100} and {p0(c).M for c in va} >= {1, 63, 64, 65, 130}
    assert any(not c.mfma_ok and p0(c).N == 64 for c in va) and {c.route[3] for c in va} == {1, 2, 3}
    assert any((p0(c).M, p0(c).N) == (33, 1) and p0(c).rows >= 64 for c in va)
    co = by(lambda c: c.family == "colsum")
    assert {p0(c).rows for c in co} == {1, 63, 64, 65, 200} and {p0(c).N for c in co} == {1, 257}
    assert all(p0(c).ldb == 264 for c in co if p0(c).N == 257)
    for fam in ("valu", "mfma", "mfma_swapped"):
        # colsum == NULL, cs_rows == rows, rows / 2 and 1 on every route
        assert {p0(c).cs for c in wc.SINGLE if c.family == fam} == {None, "full", "half", "one"}, fam
    assert max(p0(c).rows * max(p0(c).M, 1) * p0(c).N for c in wc.SINGLE) == 1025 * 130 * 384
    assert all(p0(c).rows <= 4096 for c in wc.CASES)                         # the exact fill stays below 2^24
    # ---- batches
    took = [c for c in wc.BATCH if not c.declines]
    assert {len(c.probs) for c in took} >= {1, 3, 8} and any(len(c.probs) == wc.WG_MAX + 1 for c in wc.BATCH)
    gp = [p for c in took for p in c.probs if p.M > 0]
    assert {p.N for p in gp} == {128, 256, 384} and {p.M for p in gp} == {1, 32, 33, 70}
    assert any(len({p.rows for p in c.probs}) >= 3 for c in took)
    tails = {p.rows - (-(-p.rows // 64) - 1) * 64 for c in took if c.rpc == 64 for p in c.probs if p.M > 0}
    assert tails >= {1, 3, 4, 6, 10}
    nks = {((min(64, p.rows - k * 64) + 1) & ~1) // 2 for c in took if c.rpc == 64 for p in c.probs if p.M > 0
           for k in range(-(-p.rows // 64))}
    # k-steps of the streaming ring: a clamped odd tail runs its last k-step apart
    ring = {n % 4 for n in nks} | {(((t + 1) & ~1) // 2 - 1) % 4 for t in tails if t % 2}
    assert ring == {0, 1, 2, 3} and 0 in {((t + 1) & ~1) - 2 for t in tails if t % 2}
    for c in took:
        if len(c.probs) == wc.WG_MAX:
            z = [i for i, p in enumerate(c.probs) if p.M == 0]
            assert z[0] == 0 and z[-1] == wc.WG_MAX - 1 and len(z) == 3
            assert all((c.probs[i].rows, c.probs[i].N, c.probs[i].ldb) == (7, 257, 264) for i in z)
    assert any(p.cs and p.cs_rows < p.rows for p in gp) and any(not p.cs for p in gp)
    assert all(p.ldb % 4 == 0 and p.b_off % 4 == 0 for p in gp)
    # each route (and the batch kernel) repeats one launch
    assert len(set(wc.REPEAT_IDS)) == len(wc.ALL_ROUTES) + 1


def test_route_boundaries(lib):
    r = lambda *a, **k: _route(lib, *a, **k)[0]                             # noqa: E731
    # rows 63 / 64, N % 32, mfma_ok
    assert r(63, 32, 64) == ("valu", 0, 64, 1) and r(64, 32, 64) == ("mfma", 2, 64, 1)
    assert r(64, 32, 63)[0] == "valu" and r(64, 32, 65)[0] == "valu" and r(64, 32, 96) == ("mfma", 1, 64, 1)
    assert r(64, 32, 64, mfma_ok=False) == ("valu", 0, 64, 1)
    assert [r(64, 1, n)[1] for n in (32, 64, 96, 128, 160, 192, 224, 256, 384, 512)] == [1, 2, 1, 4, 1, 2, 1, 8, 4, 8]
    # N == 1: swapped with M % 32 == 0 only, from 64 rows on and only with the pad rows
    assert r(64, 32, 1) == ("mfma_swapped", 1, 64, 1) and r(64, 33, 1)[0] == "valu" and r(64, 31, 1)[0] == "valu"
    assert r(63, 32, 1)[0] == "valu" and r(64, 32, 1, mfma_ok=False)[0] == "valu" and r(64, 32, 2)[0] == "valu"
    assert [r(64, m, 1)[1] for m in (32, 64, 96, 128, 256)] == [1, 2, 1, 4, 8]
    # about 1024 wave-tiles: the chunks grow with the tile count, and double until the partial sums fit
    assert r(4096, 32, 64) == ("mfma", 2, 64, 64) and r(4096, 512, 256) == ("mfma", 8, 64, 64)
    assert r(4096, 1024, 256) == ("mfma", 8, 128, 32)
    mn = 32 * 64
    assert r(300, 32, 64, part_floats=5 * mn) == ("mfma", 2, 64, 5) and r(300, 32, 64, part_floats=5 * mn - 1) == ("mfma", 2, 128, 3)
    assert r(300, 32, 64, part_floats=2 * mn) == ("mfma", 2, 256, 2) and r(300, 32, 64, part_floats=2 * mn - 1) == ("mfma", 2, 512, 1)
    assert r(300, 32, 64, part_floats=mn) == ("mfma", 2, 512, 1) and r(300, 32, 64, part_floats=mn - 1) == ("valu", 0, 304, 1)
    assert r(64, 32, 1, part_floats=32) == ("mfma_swapped", 1, 64, 1) and r(64, 32, 1, part_floats=31)[0] == "valu"
    # VALU: 512 rows per split, rounded up to the stage of 16; as many splits as fit, one when none does
    assert r(512, 5, 33) == ("valu", 0, 512, 1) and r(513, 5, 33) == ("valu", 0, 272, 2) and r(1025, 5, 33) == ("valu", 0, 352, 3)
    per = 5 * 33 + 33
    assert r(1025, 5, 33, cs_rows=9, part_floats=3 * per) == ("valu", 0, 352, 3)
    assert r(1025, 5, 33, cs_rows=9, part_floats=3 * per - 1) == ("valu", 0, 528, 2)
    assert r(1025, 5, 33, cs_rows=9, part_floats=per) == r(1025, 5, 33, cs_rows=9, part_floats=per - 1) == ("valu", 0, 1040, 1)
    # the column sums alone: about 64 rows per chunk
    assert r(64, 0, 257, form=1) == ("colsum", 0, 64, 1) and r(65, 0, 257, form=1) == ("colsum", 0, 33, 2)
    assert r(200, 0, 257, form=1, part_floats=4 * 257) == ("colsum", 0, 50, 4)
    assert r(200, 0, 257, form=1, part_floats=4 * 257 - 1) == ("colsum", 0, 67, 3)
    # ---- the batch: N % 128, rows 63 / 64, 16-byte rows of B, 8 / 9 problems, the buffer
    b = lambda *a, **k: _batch_route(lib, *a, **k)                          # noqa: E731
    assert b([(64, 32, 128)]) == 64 and b([(64, 32, 96)]) == 0 and b([(64, 32, 64)]) == 0 and b([(64, 32, 256)]) == 64
    assert b([(63, 32, 128)]) == 0 and b([(64, 32, 128)], ldb=130) == 0 and b([(64, 32, 128)], ldb=132) == 64
    assert b([(64, 32, 128)], b=0x10008) == 0 and b([(64, 32, 128)], b=0x10010) == 64
    assert b([(64, 1, 128)] * 8) == 64 and b([(64, 1, 128)] * 9) == 0
    assert b([(7, 0, 257)]) == 64 and b([(7, 0, 257), (63, 1, 128)]) == 0           # column sums alone: any shape
    mn = 32 * 128
    assert b([(200, 32, 128)], part_floats=4 * mn) == 64 and b([(200, 32, 128)], part_floats=4 * mn - 1) == 96
    assert b([(200, 32, 128)], part_floats=3 * mn - 1) == 128 and b([(200, 32, 128)], part_floats=2 * mn - 1) == 256
    assert b([(200, 32, 128)], part_floats=mn) == 256 and b([(200, 32, 128)], part_floats=mn - 1) == 0


def test_no_route_plans_past_the_buffer(lib):
    """Whatever the buffer holds, the partial sums a route plans to write fit it -- for the table and around the
    thresholds of a sweep of shapes (the column sums of the matrix-core routes reuse the buffer after C)."""
    shapes = [(c.probs[0].rows, c.probs[0].M, c.probs[0].N) for c in wc.SINGLE if c.form == "auto"]
    shapes += [(4096, 32, 64), (3000, 1, 32), (2000, 64, 1), (700, 33, 1), (700, 3, 5)]
    for rows, M, N in shapes:
        for cs_rows in (None, 1, rows):
            per = M * N + (N if cs_rows else 0)
            for pf in sorted({1, N, M * N - 1, M * N, M * N + 1, per - 1, per, 2 * per - 1, 2 * M * N, 5 * per, 1 << 24}):
                if pf < 1:
                    continue
                (form, ntw, rpc, nch), (crpc, cch) = _route(lib, rows, M, N, cs_rows=cs_rows, part_floats=pf)
                what = (rows, M, N, cs_rows, pf, form, rpc, nch, crpc, cch)
                assert nch >= 1 and nch == -(-rows // rpc), what
                if form == "valu":
                    assert cch == 0 and (nch * per <= pf or (nch == 1 and per > pf)), what
                else:
                    assert nch * M * N <= pf and cch * N <= pf, what
                    assert (cch == 0) == (cs_rows is None) and (cs_rows is None or cch == -(-cs_rows // crpc)), what
    # the shape the old launcher overran: 64 column-sum chunks of N floats in a buffer of M * N = 32 N
    assert _route(lib, 4096, 32, 64, cs_rows=4096, part_floats=32 * 64) == (("mfma", 2, 4096, 1), (128, 32))
    # with room the column sums keep their 64 rows per chunk (what every gradient call has)
    assert _route(lib, 4096, 32, 64, cs_rows=4096)[1] == (64, 64) and _route(lib, 4096, 32, 1, cs_rows=4096)[1] == (64, 64)


def test_entries_check_their_arguments(lib):
    out = (C.c_int * 6)()
    d = _lib.WgradDesc()
    assert lib.gmpc_wgrad_route(C.byref(d), out) != 0                       # null operands
    good = wc.SINGLE[0]
    assert good.probs[0].cs == "full"

    def bad(**kw):
        d = _descs(good)
        for k, v in kw.items():
            setattr(d[0], k, v)
        return lib.gmpc_wgrad_route(C.byref(d[0]), out) != 0

    assert not bad() and lib.gmpc_wgrad_route(C.byref(_descs(good)[0]), None) != 0
    p = good.probs[0]
    assert bad(A=None) and bad(B=None) and bad(C=None) and bad(part=None) and bad(part_floats=0)
    assert bad(rows=0) and bad(M=0) and bad(N=0) and bad(lda=p.M - 1) and bad(ldb=p.N - 1) and bad(form=2)
    assert bad(cs_rows=0) and bad(cs_rows=-1) and bad(cs_rows=p.rows + 1) and not bad(cs_rows=1)
    assert not bad(colsum=None, cs_rows=0)                                  # cs_rows is only read with colsum
    assert bad(form=1, colsum=None) and not bad(form=1, A=None, C=None, M=0)
    # no ctx: rejected before any GPU call
    d = _descs(good)
    taken = C.c_int(7)
    assert lib.gmpc_wgrad_ex(None, C.byref(d[0]), None) != 0
    assert lib.gmpc_wgrad_batch_ex(None, d, 1, 0x10000, 1 << 20, None, C.byref(taken)) != 0 and taken.value == 7
    # the batch query: bad problems and counts are errors, not "declined"
    r2 = (C.c_int * 2)()
    d = _descs(wc.BATCH[0])
    assert lib.gmpc_wgrad_batch_route(d, 1, 1 << 20, r2) == 0 and r2[0] == 1
    assert lib.gmpc_wgrad_batch_route(d, 0, 1 << 20, r2) != 0 and lib.gmpc_wgrad_batch_route(None, 1, 1 << 20, r2) != 0
    assert lib.gmpc_wgrad_batch_route(d, 1, 0, r2) != 0 and lib.gmpc_wgrad_batch_route(d, 1, 1 << 20, None) != 0
    d[0].cs_rows = 0
    assert lib.gmpc_wgrad_batch_route(d, 1, 1 << 20, r2) != 0
    d[0].cs_rows, d[0].M, d[0].C = 1, 0, d[0].colsum + 4                    # M == 0 wants C == colsum
    assert lib.gmpc_wgrad_batch_route(d, 1, 1 << 20, r2) != 0
    d[0].C = d[0].colsum
    assert lib.gmpc_wgrad_batch_route(d, 1, 1 << 20, r2) == 0 and r2[0] == 1


@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_buffers_follow_the_contract(case):
    pay = []
    for fill in wc.FILLS:
        Bf, ref = built(case, fill)
        for pb, r in zip(Bf.probs, ref):
            p = pb.p
            assert p.ldb >= p.N and p.b_off > 0 and (p.cs is None or 1 <= p.cs_rows <= p.rows)
            ops = [(pb.B, pb.b_idx, p.N, not case.swapped)]
            if p.M > 0:
                assert p.lda >= p.M and (not p.window or p.lda > p.M)
                ops.append((pb.A, pb.a_idx, p.M, case.swapped))
                assert np.isfinite(r["C"]).all() and (np.abs(r["C"]) <= r["S"] * (1 + 1e-12)).all()
            for arr, idx, width, padded in ops:
                # finite exactly inside the logical matrix and the pad rows, which are large; NaN rows behind
                inside = np.zeros(arr.size, bool)
                inside[idx(0, p.rows + (wc.PAD if padded else 0)).ravel()] = True
                assert np.isfinite(arr[inside]).all() and np.isnan(arr[~inside]).all()
                assert idx(p.rows + wc.PAD + 1, p.rows + wc.PAD + 2).max() < arr.size
                if padded:
                    pad = arr[idx(p.rows, p.rows + wc.PAD)]
                    assert (np.abs(pad) >= 1e30).all() and (np.abs(pad) < 2e30).all()
                    assert (pad[:, 0] > 0).any() and (pad[:, 0] < 0).any()
            vals = pb.b(0, p.rows)
            if fill == "exact":
                assert (vals == np.round(vals)).all() and (np.abs(vals) <= 4).all() and (vals != 0).all()
            for pre, count in ((pb.C0, p.M * p.N), (pb.cs0, p.N)):
                if pre is not None:
                    assert np.isnan(pre).all() and pre.size == wc.GUARD_LO + count + wc.GUARD_HI
                    pay.append(pre.view(np.uint32))
        assert np.isnan(Bf.part0).all() and Bf.part0.size == wc.GUARD_LO + case.part_floats + wc.PART_HI
        if fill == "exact":
            pay.append(Bf.part0.view(np.uint32))
            bits = np.concatenate(pay)
            assert bits.size == np.unique(bits).size or bits.size > 0x3FFFFE
            pay = []
    if case.kind == "batch" and not case.declines:
        assert all(p.ldb % 4 == 0 and p.b_off % 4 == 0 for p in case.probs if p.M > 0)


@pytest.mark.parametrize("case", wc.CASES, ids=IDS)
def test_fp32_numpy_model_passes(case):
    """The contract followed in fp32 NumPy passes the checker: bit for bit on the exact fill, and the per-entry bound is no
    tighter than fp32 itself on the float fill."""
    for fill in wc.FILLS:
        Bf, ref = built(case, fill)
        fig = wc.check(Bf, ref, wc.model_kernel(Bf))
        assert fig["max_rel"] <= 1e-5 and fig["entry"] <= 1.0
        if fill == "exact":
            assert fig["max_rel"] == 0.0 and fig["entry"] == 0.0


@pytest.mark.parametrize("variant", wc.VARIANTS)
def test_checker_rejects(variant):
    """Every broken kernel is rejected on EVERY case where it differs from the contract, with either fill, and applies
    to at least one case of each family that has the feature."""
    hit = []
    for case in wc.CASES:
        if not wc.applies(case, variant):
            continue
        for fill in wc.FILLS:
            Bf, ref = built(case, fill)
            with pytest.raises(AssertionError):
                wc.check(Bf, ref, wc.model_kernel(Bf, variant))
        hit.append(case)
    assert {c.family for c in hit} == set(wc.VARIANT_FAMILIES[variant]), variant


def test_a_declined_batch_must_leave_everything_alone():
    case = next(c for c in wc.BATCH if c.declines)
    Bf, ref = built(case, "exact")
    wc.check(Bf, ref, wc.model_kernel(Bf))
    for spoil in ("taken", "part", "C"):
        got = wc.model_kernel(Bf)
        if spoil == "taken":
            got["taken"] = True
        elif spoil == "part":
            got["part"][wc.GUARD_LO + 5] = 0.0
        else:
            got["C"][0][wc.GUARD_LO] = 0.0
        with pytest.raises(AssertionError):
            wc.check(Bf, ref, got)
