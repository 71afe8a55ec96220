"""The weight-gradient GEMMs (csrc/gmpc_wgrad.hip): case tables, buffers, fp64 reference, checker and an fp32 model of the
contract with ways to break it (TEST INFRASTRUCTURE, no GPU import).

Shared by tests/test_wgrad_cases.py (CPU: the tables reach every route of the launchers, the checker rejects broken
kernels) and tests/test_gpu_wgrad.py (GPU: every case through gmpc_wgrad_ex / gmpc_wgrad_batch_ex).

    C[M][N] = sum_{r < rows} A[r][:M]^T B[r][:N],      colsum[N] = sum_{r < cs_rows} B[r][:N]

Each operand is built as its ALLOCATION, a flat fp32 array:
  A   the logical [rows][M] at float offset 3 with leading dimension lda (M + 5 in a window); NaN before the offset, in
      the columns >= M and in every row >= rows: A is clamped, nothing outside the logical matrix may be used.
  B   the logical [rows][N] at offset 4 (16-byte aligned; 5 and an odd ldb in the `odd_b` case) with NaN in the columns
      >= N; rows rows .. rows + PAD - 1 hold +-1e30 (the contract wants them allocated and finite: a zero A operand
      meets them), NaN behind them.
  On the transposed route (N == 1, M % 32 == 0) the roles swap: A has the pad rows, B the NaN rows.
  C, colsum   8 guard words, the result, 8 guard words, all pre-filled with NaNs whose payload names their own place.
  part        8 guard words, exactly part_floats floats, 64 guard words.
Two fills: "exact" (non-zero integers in [-4, 4]: every partial sum is an integer below 2^24, so the result must equal
the fp64 reference bit for bit whatever the order of summation) and "float" (standard normal, held to
(rows + 8) 2^-24 sum_r |A_ri| |B_rj| per entry -- the first-order bound (rows - 1) u sum |x| of any fma / tree order plus
room for the second-order terms -- and to the max-norm tolerance of the suite)."""

import ctypes as C

import numpy as np

PAD = 8                               # GMPC_WGRAD_PAD
WG_MAX = 8                            # GMPC_WG_MAX: problems of one batch launch
U = 2.0 ** -24                        # unit roundoff of fp32
FILLS = ("exact", "float")
FORMS = ("valu", "mfma", "mfma_swapped", "colsum")          # gmpc_wgrad_route: route6[0]
FAMILIES = FORMS + ("batch",)
ALL_ROUTES = ([("valu", 0)] + [("mfma", w) for w in (1, 2, 4, 8)] + [("mfma_swapped", w) for w in (1, 2, 4, 8)]
              + [("colsum", 0)])
GUARD_LO, GUARD_HI, PART_HI = 8, 8, 64
A_OFF, B_OFF = 3, 4


class Prob:
    """One problem.  cs: None | "full" | "half" | "one" (cs_rows = rows, rows // 2, 1); M = 0: the column sums alone
    (C == colsum, A = B); window: lda = M + 5, ldb = N + 4; odd_b: B at an odd offset with an odd ldb."""

    def __init__(self, rows, M, N, cs=None, window=False, odd_b=False, ldb=None, b_off=None):
        self.rows, self.M, self.N, self.cs, self.window, self.odd_b = rows, M, N, cs, window, odd_b
        self.lda = M + 5 if window else M
        self.ldb = ldb if ldb is not None else (N + 4 if window else N)
        self.b_off = b_off if b_off is not None else B_OFF
        if odd_b:
            self.ldb, self.b_off = N + 3 if N % 2 == 0 else N + 2, 5
        if M == 0:
            assert cs == "full"
        self.cs_rows = {None: 0, "full": rows, "half": rows // 2, "one": 1}[cs]
        assert cs is None or self.cs_rows >= 1

    @property
    def tag(self):
        return "x".join(map(str, (self.rows, self.M, self.N))) + (f"cs{self.cs_rows}" if self.cs else "") + \
            ("w" if self.window else "") + ("o" if self.odd_b else "")


class Case:
    """kind "single": one problem through gmpc_wgrad_ex, route = (form, NTW, rows per chunk, chunks) as gmpc_wgrad_route
    reports it; kind "batch": problems through gmpc_wgrad_batch_ex, rpc = the batch's rows per chunk (0: it declines).
    part_floats = None: a roomy buffer (32 partial sums; a batch: what its shortest chunks need)."""

    def __init__(self, kind, probs, route=None, rpc=None, mfma_ok=True, form="auto", part_floats=None, tag=""):
        self.kind, self.probs, self.route, self.rpc, self.mfma_ok, self.form = kind, probs, route, rpc, mfma_ok, form
        self.roomy = part_floats is None
        if part_floats is None:
            if kind == "single":
                p = probs[0]
                part_floats = 32 * (p.M * p.N + p.N) if form == "auto" else 32 * p.N
            else:
                part_floats = batch_need(probs, 64) + 64
        self.part_floats = part_floats
        self.family = "batch" if kind == "batch" else route[0]
        self.id = "-".join([self.family if kind == "batch" else "%s%d" % route[:2]] + [p.tag for p in probs[:3]]
                           + ([f"np{len(probs)}"] if kind == "batch" else [])
                           + ([] if self.roomy else [f"part{part_floats}"]) + ([] if mfma_ok else ["nomfma"])
                           + ([tag] if tag else []))

    @property
    def declines(self):
        return self.kind == "batch" and self.rpc == 0

    @property
    def swapped(self):
        return self.kind == "single" and self.route[0] == "mfma_swapped"

    @property
    def plain(self):
        p = self.probs[0]
        return (self.kind == "single" and self.roomy and self.mfma_ok and not p.window and not p.odd_b
                and p.cs in (None, "full") and p.ldb == p.N)

    def chunking(self, i):
        """(matrix-core form?, rows per chunk) of problem i's GEMM part."""
        if self.kind == "batch":
            return True, self.rpc
        return self.route[0] in ("mfma", "mfma_swapped"), self.route[2]


def batch_need(probs, rpc):
    """Floats the batch launcher asks of `part` for chunks of rpc rows (its own rule: 1024 N per column sum)."""
    return sum(-(-p.rows // rpc) * p.M * p.N + (1024 * p.N if p.cs else 0) for p in probs)


def _single():
    out = []

    def s(route, rows, M, N, cs=None, **kw):
        pk = {k: kw.pop(k) for k in ("window", "odd_b", "ldb") if k in kw}
        out.append(Case("single", [Prob(rows, M, N, cs, **pk)], route=route, **kw))

    # ---- matrix cores: every width with everything plain ...
    s(("mfma", 1, 64, 1), 64, 32, 32, "full")
    s(("mfma", 2, 64, 1), 64, 32, 64, "full")
    s(("mfma", 4, 64, 1), 64, 32, 128, "full")
    s(("mfma", 8, 64, 1), 64, 32, 256, "full")
    # ... then widths x row tails x M: with 64 rows per chunk the last chunks have 1, 2, 6, 8, 12 and 63 rows, Kp % 6 takes
    # 0, 2 and 4 (the prefetch of gemm_tile advances 6 rows per trip)
    s(("mfma", 1, 64, 2), 65, 1, 96, "full", window=True)
    s(("mfma", 1, 64, 2), 66, 31, 160, "half", window=True)
    s(("mfma", 2, 64, 2), 70, 33, 64, "one")
    s(("mfma", 2, 64, 2), 72, 64, 192, "one", window=True)
    s(("mfma", 4, 64, 2), 76, 70, 128, None, window=True)
    s(("mfma", 4, 64, 2), 127, 32, 384, "full", window=True)
    s(("mfma", 8, 64, 3), 129, 33, 256, "half")
    s(("mfma", 2, 64, 3), 191, 70, 64, "full", odd_b=True)
    # the chunks double until their partial sums fit: 64 -> 256 (two chunks), -> 512 (one); one chunk of 4096 rows whose
    # column sums alone would want 64 chunks of N floats: more than the buffer
    s(("mfma", 2, 256, 2), 300, 32, 64, "full", part_floats=2 * 32 * 64)
    s(("mfma", 2, 512, 1), 300, 32, 64, "full", part_floats=32 * 64 + 64)
    s(("mfma", 2, 4096, 1), 4096, 32, 64, "full", part_floats=32 * 64)
    # less than one partial sum: the matrix cores decline, the VALU form may not use the buffer
    s(("valu", 0, 80, 1), 70, 33, 64, "full", part_floats=33 * 64 - 1)
    # ---- N == 1 with M % 32 == 0: the operands swap
    s(("mfma_swapped", 1, 64, 1), 64, 32, 1, "full")
    s(("mfma_swapped", 2, 64, 2), 65, 64, 1, None)
    s(("mfma_swapped", 1, 64, 3), 129, 96, 1, "half", window=True)
    s(("mfma_swapped", 8, 64, 2), 65, 256, 1, "full")
    s(("mfma_swapped", 4, 64, 1), 64, 128, 1, None)
    s(("mfma_swapped", 1, 64, 1), 64, 32, 1, "one", window=True)
    s(("valu", 0, 80, 1), 65, 33, 1, "full")
    # ---- VALU: fewer than 64 rows, N % 32 != 0, mfma_ok = false; 16 rows per stage, 64 x 64 per workgroup
    s(("valu", 0, 16, 1), 1, 1, 1, "full")
    s(("valu", 0, 16, 1), 15, 63, 3, "half", window=True)
    s(("valu", 0, 16, 1), 16, 64, 33, None)
    s(("valu", 0, 32, 1), 17, 65, 65, "one", window=True)
    s(("valu", 0, 64, 1), 63, 130, 100, "full", window=True)
    s(("valu", 0, 208, 1), 200, 32, 64, "full", mfma_ok=False)
    s(("valu", 0, 272, 2), 513, 5, 33, "half", window=True)                 # 2 splits, 257 rows rounded up to 16
    s(("valu", 0, 352, 3), 1025, 130, 384, "full", mfma_ok=False)           # 3 splits
    s(("valu", 0, 528, 2), 1025, 7, 33, "full", part_floats=2 * (7 * 33 + 33))     # 3 splits do not fit: 2
    # ---- the column sums alone (the critic head's last layer: ldb = 264)
    for rows, N, ldb, route in [(1, 257, 264, (1, 1)), (63, 1, 1, (63, 1)), (64, 257, 264, (64, 1)), (65, 1, 1, (33, 2)),
                                (200, 257, 264, (50, 4))]:
        out.append(Case("single", [Prob(rows, 0, N, "full", ldb=ldb)], route=("colsum", 0) + route, form="colsum_only"))
    out.append(Case("single", [Prob(200, 0, 257, "full", ldb=264)], route=("colsum", 0, 100, 2), form="colsum_only",
                    part_floats=2 * 257))
    return out


def _batch():
    out = []
    cso = lambda: Prob(7, 0, 257, "full", ldb=264)                          # noqa: E731  column sums only
    ok = lambda: Prob(64, 32, 128, "full")                                  # noqa: E731
    out.append(Case("batch", [ok()], rpc=64))
    # three row counts: last chunks of 1 (the clamped tail alone: Kp - 2 == 0), 8 and 3 rows
    out.append(Case("batch", [Prob(65, 33, 128, "half", window=True), Prob(200, 70, 256, None, window=True),
                              Prob(131, 1, 384, "full")], rpc=64))
    # eight problems, column-sum-only ones first, in the middle and last; last chunks of 1, 3, 4, 6 and 10 rows: with
    # the full chunks (32 k-steps) the ring of depth 4 ends on every remainder
    out.append(Case("batch", [cso(), Prob(65, 32, 128, "full"), Prob(131, 33, 256, "one", window=True), cso(),
                              Prob(68, 70, 128, None), Prob(70, 1, 384, "half", window=True),
                              Prob(74, 33, 128, "full"), cso()], rpc=64))
    two = lambda: [Prob(200, 32, 128, None), Prob(200, 33, 256, "half", window=True)]      # noqa: E731
    assert batch_need(two(), 64) == 312320 and batch_need(two(), 96) == 299776 and batch_need(two(), 128) == 287232
    out.append(Case("batch", two(), rpc=96, part_floats=299776))
    out.append(Case("batch", two(), rpc=128, part_floats=299775))
    # ---- batches the launcher declines
    out.append(Case("batch", [Prob(64, 32, 128, None)], rpc=0, part_floats=32 * 128 - 1))
    out.append(Case("batch", [ok(), Prob(64, 32, 96, None)], rpc=0, tag="N96"))
    out.append(Case("batch", [ok(), Prob(63, 32, 128, None)], rpc=0, tag="rows63"))
    out.append(Case("batch", [ok(), Prob(64, 32, 128, None, ldb=130)], rpc=0, tag="ldb130"))
    out.append(Case("batch", [ok(), Prob(64, 32, 128, None, b_off=6)], rpc=0, tag="misaligned"))
    out.append(Case("batch", [Prob(64, 1, 128, None) for _ in range(WG_MAX + 1)], rpc=0))
    return out


SINGLE = _single()
BATCH = _batch()
CASES = SINGLE + BATCH
assert len({c.id for c in CASES}) == len(CASES), sorted(c.id for c in CASES)
# one case per route (and one batch) whose second launch must give the same bits: the first of each in the tables
REPEAT_IDS = tuple(next(c.id for c in SINGLE if c.route[:2] == r) for r in ALL_ROUTES) + (BATCH[0].id,)


# ---- buffers ---------------------------------------------------------------------------------------------------------
def nan_payload(size, base=0):
    """Quiet NaNs whose mantissa carries 1 + (base + index) mod 2^22 - 2: a float moved from elsewhere is told apart."""
    k = (np.arange(size, dtype=np.uint64) + np.uint64(base)) % np.uint64(0x3FFFFE)
    return (np.uint32(0x7FC00000) | (np.uint32(1) + k.astype(np.uint32))).view(np.float32)


class ProbBuffers:
    """The allocations of one problem (see the module docstring)."""

    def a_idx(self, r0, r1, dense=False):
        p = self.p
        return A_OFF + np.arange(r0, r1)[:, None] * (p.M if dense else p.lda) + np.arange(p.M)[None, :]

    def b_idx(self, r0, r1):
        p = self.p
        return p.b_off + np.arange(r0, r1)[:, None] * p.ldb + np.arange(p.N)[None, :]

    def a(self, r0, r1, **kw):
        return self.A[self.a_idx(r0, r1, **kw)]

    def b(self, r0, r1):
        return self.B[self.b_idx(r0, r1)]


class Buffers:
    pass


def _values(rng, fill, shape):
    if fill == "exact":
        return (rng.integers(1, 5, size=shape) * rng.choice((-1, 1), size=shape)).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _pad_rows(n, width):
    """n rows of about 1e30 with alternating signs: finite, and as hostile as the contract allows."""
    r, c = np.arange(n)[:, None], np.arange(width)[None, :]
    return (1e30 * (1.0 + 0.01 * ((r + 3 * c) % 7)) * np.where((r + c) % 2 == 0, 1.0, -1.0)).astype(np.float32)


def build(case, fill):
    """Allocations of one case and fill, by the rules in the module docstring."""
    seed = int.from_bytes((case.id + fill).encode(), "little") % (2 ** 32)
    rng = np.random.default_rng(seed)
    Bf = Buffers()
    Bf.case, Bf.fill, Bf.probs = case, fill, []
    base = 0
    for p in case.probs:
        pb = ProbBuffers()
        pb.p = p
        pb.pad_a = case.swapped
        pb.B = np.full(p.b_off + (p.rows + PAD + 2) * p.ldb + 3, np.nan, np.float32)
        pb.B[pb.b_idx(0, p.rows)] = _values(rng, fill, (p.rows, p.N))
        if not case.swapped:
            pb.B[pb.b_idx(p.rows, p.rows + PAD)] = _pad_rows(PAD, p.N)
        if p.M > 0:
            pb.A = np.full(A_OFF + (p.rows + PAD + 2) * p.lda + 3, np.nan, np.float32)
            pb.A[pb.a_idx(0, p.rows)] = _values(rng, fill, (p.rows, p.M))
            if case.swapped:
                pb.A[pb.a_idx(p.rows, p.rows + PAD)] = _pad_rows(PAD, p.M)
            pb.C0 = nan_payload(GUARD_LO + p.M * p.N + GUARD_HI, base).copy()
            base += pb.C0.size
        else:
            pb.A, pb.C0 = None, None
        pb.cs0 = None
        if p.cs:
            pb.cs0 = nan_payload(GUARD_LO + p.N + GUARD_HI, base).copy()
            base += pb.cs0.size
        Bf.probs.append(pb)
    Bf.part0 = nan_payload(GUARD_LO + case.part_floats + PART_HI, base).copy()
    return Bf


# ---- reference -------------------------------------------------------------------------------------------------------
def reference(Bf):
    """fp64 from the fp32 operands, per problem: dict(C, S, cs, csS) with S = sum_r |A_ri| |B_rj| and csS = sum_r |B_rj|,
    the scales of the per-entry bounds (C, S None for a column-sum-only problem; cs, csS None without colsum)."""
    out = []
    for pb in Bf.probs:
        p = pb.p
        b = pb.b(0, p.rows).astype(np.float64)
        r = dict(C=None, S=None, cs=None, csS=None)
        if p.M > 0:
            a = pb.a(0, p.rows).astype(np.float64)
            r["C"], r["S"] = a.T @ b + 0.0, np.abs(a).T @ np.abs(b)          # + 0.0: no -0 (the kernels start from +0)
        if p.cs:
            r["cs"], r["csS"] = b[:p.cs_rows].sum(axis=0) + 0.0, np.abs(b[:p.cs_rows]).sum(axis=0)
        out.append(r)
    return out


# ---- checker ---------------------------------------------------------------------------------------------------------
def _check_block(name, got_flat, prefill, count, ref, S, n_sum, fill, tol):
    """One result allocation: the guards bit-identical, the `count` floats between them against ref.  -> (max_rel,
    worst error as a fraction of the per-entry bound)."""
    got_flat = np.ascontiguousarray(got_flat, np.float32)
    assert got_flat.shape == prefill.shape, f"{name}: shape"
    gbits, pbits = got_flat.view(np.uint32), prefill.view(np.uint32)
    guard = np.ones(prefill.size, bool)
    guard[GUARD_LO:GUARD_LO + count] = False
    moved = np.flatnonzero(guard & (gbits != pbits))
    assert moved.size == 0, f"{name}: {moved.size} guard words changed, first at {moved[:4] - GUARD_LO} (0 = first result)"
    got32 = got_flat[GUARD_LO:GUARD_LO + count]
    ref, S = ref.ravel(), S.ravel()
    assert np.isfinite(got32).all(), f"{name}: non-finite result at {np.flatnonzero(~np.isfinite(got32))[:4].tolist()}"
    err = np.abs(got32.astype(np.float64) - ref)
    max_rel = float(err.max() / (np.abs(ref).max() + 1e-300))
    bound = (n_sum + 8) * U * S
    ratio = float((err[S > 0] / bound[S > 0]).max()) if (S > 0).any() else 0.0
    if fill == "exact":
        want = ref.astype(np.float32)
        assert (want.astype(np.float64) == ref).all()                        # the reference itself is exact in fp32
        bad = np.flatnonzero(got32.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (f"{name}: {bad.size} of {count} entries differ from the exact result, first at "
                               f"{bad[:4].tolist()}: got {got32[bad[:4]].tolist()}, want {want[bad[:4]].tolist()}")
    else:
        assert max_rel <= tol, f"{name}: max-norm relative error {max_rel:.3e} > {tol:.0e}"
        over = err > bound
        assert not over.any(), (f"{name}: {int(over.sum())} entries outside ({n_sum} + 8) u S, worst {ratio:.3f} x the "
                                f"bound, first at {np.flatnonzero(over)[:4].tolist()}")
    return max_rel, ratio


def check(Bf, ref, got, tol=1e-5, on_figures=None):
    """Asserts the contract on what a launch left behind.  got = dict(C=[flat C allocation per problem or None],
    cs=[flat colsum allocation or None], part=flat part allocation, taken=bool).  on_figures(dict) receives max_rel
    (max-norm relative error), entry (largest |got - ref| over its bound), both over all results, before the
    assertions on values run."""
    c = Bf.case
    assert bool(got["taken"]) == (not c.declines), f"{c.id}: taken = {got['taken']}"
    part = np.ascontiguousarray(got["part"], np.float32)
    assert part.shape == Bf.part0.shape
    same = part.view(np.uint32) == Bf.part0.view(np.uint32)
    if not c.declines:
        same[GUARD_LO:GUARD_LO + c.part_floats] = True                      # the content of part is unspecified
    moved = np.flatnonzero(~same)
    assert moved.size == 0, (f"{c.id}: {moved.size} words around part changed, first at {moved[:4] - GUARD_LO} of "
                             f"{c.part_floats} floats")
    figs, todo = [], []
    for i, (pb, r) in enumerate(zip(Bf.probs, ref)):
        p = pb.p
        for what, g, pre, count, rr, ss, n in (("C", got["C"][i], pb.C0, p.M * p.N, r["C"], r["S"], p.rows),
                                               ("colsum", got["cs"][i], pb.cs0, p.N, r["cs"], r["csS"], p.cs_rows)):
            if pre is None:
                continue
            name = f"{c.id}[{i}] {Bf.fill} {what}"
            if c.declines:
                assert np.array_equal(np.ascontiguousarray(g, np.float32).view(np.uint32), pre.view(np.uint32)), \
                    f"{name}: written by a batch that was declined"
                continue
            todo.append((name, g, pre, count, rr, ss, n))
    if on_figures is not None and todo:
        # the figures first (they are reported even when an assertion below fails)
        mr, en = 0.0, 0.0
        for name, g, pre, count, rr, ss, n in todo:
            g32 = np.ascontiguousarray(g, np.float32)[GUARD_LO:GUARD_LO + count].astype(np.float64)
            err = np.abs(g32 - rr.ravel())
            with np.errstate(invalid="ignore", divide="ignore"):
                mr = max(mr, float(np.nan_to_num(err.max() / (np.abs(rr).max() + 1e-300), nan=np.inf)))
                q = err / ((n + 8) * U * ss.ravel())
            en = max(en, float(np.nan_to_num(q[ss.ravel() > 0], nan=np.inf).max()) if (ss > 0).any() else 0.0)
        on_figures(dict(max_rel=mr, entry=en, entries=int(sum(t[3] for t in todo))))
    for name, g, pre, count, rr, ss, n in todo:
        figs.append(_check_block(name, g, pre, count, rr, ss, n, Bf.fill, tol))
    return dict(max_rel=max([f[0] for f in figs], default=0.0), entry=max([f[1] for f in figs], default=0.0))


# ---- the contract in fp32 NumPy, and ways to break it ----------------------------------------------------------------
VARIANTS = ("drop_last_row", "odd_tail_uses_pad_row", "a_row_past_rows", "a_col_past_M", "colsum_over_rows",
            "batch_col_perm", "batch_wrong_problem_offset", "colsum_only_skipped", "chunk_dropped",
            "swapped_not_transposed", "write_past_C", "write_past_part")
# the families that have the feature a variant breaks
VARIANT_FAMILIES = {
    "drop_last_row": FAMILIES, "odd_tail_uses_pad_row": ("mfma", "mfma_swapped", "batch"),
    "a_row_past_rows": ("valu", "mfma", "mfma_swapped", "batch"), "a_col_past_M": ("valu", "mfma", "mfma_swapped", "batch"),
    "colsum_over_rows": ("valu", "mfma", "mfma_swapped", "batch"), "batch_col_perm": ("batch",),
    "batch_wrong_problem_offset": ("batch",), "colsum_only_skipped": ("colsum", "batch"),
    "chunk_dropped": ("valu", "mfma", "mfma_swapped", "batch"), "swapped_not_transposed": ("mfma_swapped",),
    "write_past_C": ("valu", "mfma", "mfma_swapped", "batch"), "write_past_part": FAMILIES,
}


def _odd_tail(case, i):
    """The last chunk of problem i has an odd number of rows (matrix-core forms: its last k-step is half empty)."""
    p = case.probs[i]
    matrix, rpc = case.chunking(i)
    return p.M > 0 and matrix and (p.rows - (-(-p.rows // rpc) - 1) * rpc) % 2 == 1


def _gemm_model(case, i, pb, variant):
    """C of problem i in fp32: one product per row chunk, the chunks added in order."""
    p = pb.p
    matrix, rpc = case.chunking(i)
    nch = -(-p.rows // rpc)
    f0 = np.float32(0.0)
    if variant == "swapped_not_transposed" and case.swapped:
        # the matrix-core kernel on (A, B) as they are: A's first column against M "columns" of B's rows
        idx = p.b_off + np.arange(p.rows)[:, None] * p.ldb + np.arange(p.M)[None, :]
        bw = np.where(idx < pb.B.size, pb.B[np.minimum(idx, pb.B.size - 1)], np.float32(np.nan))
        return (pb.a(0, p.rows)[:, :1].T @ bw).reshape(p.M, 1)
    acc = np.zeros((p.M, p.N), np.float32)
    for ch in range(nch):
        if variant == "chunk_dropped" and nch >= 2 and ch == 1:
            continue
        r0, r1 = ch * rpc, min(p.rows, (ch + 1) * rpc)
        last = r1 == p.rows
        if variant == "drop_last_row" and last:
            r1 -= 1
        part = np.zeros((p.M, p.N), np.float32)
        if r1 > r0:
            part = pb.a(r0, r1, dense=(variant == "a_col_past_M")).T @ pb.b(r0, r1)
        if last:
            past_a, past_b = pb.a(p.rows, p.rows + 1)[0], pb.b(p.rows, p.rows + 1)[0]      # row `rows` of the allocations
            if variant == "odd_tail_uses_pad_row" and _odd_tail(case, i):
                # the half-empty k-step is not masked: the clamped operand's last row meets the other's pad row
                if case.swapped:
                    part = part + np.outer(past_a, pb.b(p.rows - 1, p.rows)[0])
                else:
                    part = part + np.outer(pb.a(p.rows - 1, p.rows)[0], past_b)
            if variant == "a_row_past_rows" and (_odd_tail(case, i) or (not matrix and p.rows % 16)):
                # the clamped operand is read past its last row and multiplied by a zero mask instead of selected
                with np.errstate(invalid="ignore"):
                    part = part + (np.outer(past_a, past_b * f0) if case.swapped else np.outer(past_a * f0, past_b * f0))
        acc = acc + part
    if variant == "batch_col_perm" and case.kind == "batch":
        # tile j of a lane stored as if it were columns 32 j + l31: it is columns 4 l31 + j of its 128-column block
        j, l = np.meshgrid(np.arange(4), np.arange(32), indexing="ij")
        out = acc.copy()
        for blk in range(p.N // 128):
            out[:, 128 * blk + (32 * j + l).ravel()] = acc[:, 128 * blk + (4 * l + j).ravel()]
        acc = out
    return acc


def model_kernel(Bf, variant=None):
    """What a correct launch leaves behind (variant None), computed in fp32, or one of the broken VARIANTS; in the form
    check() takes."""
    c = Bf.case
    got = dict(C=[None if pb.C0 is None else pb.C0.copy() for pb in Bf.probs],
               cs=[None if pb.cs0 is None else pb.cs0.copy() for pb in Bf.probs], part=Bf.part0.copy(),
               taken=not c.declines)
    if c.declines:
        return got
    got["part"][GUARD_LO:GUARD_LO + c.part_floats] = 0.0
    if variant == "write_past_part":
        got["part"][GUARD_LO + c.part_floats] = 0.0
    first_gemm = None
    for i, pb in enumerate(Bf.probs):
        p = pb.p
        if p.M > 0:
            v = _gemm_model(c, i, pb, variant)
            if variant == "batch_wrong_problem_offset" and c.kind == "batch":
                if first_gemm is None:
                    first_gemm = v
                else:
                    v = np.resize(first_gemm.ravel(), p.M * p.N).reshape(p.M, p.N)      # the first problem's partial sums
            got["C"][i][GUARD_LO:GUARD_LO + p.M * p.N] = v.ravel()
            if variant == "write_past_C":
                got["C"][i][GUARD_LO + p.M * p.N] = v.ravel()[-1]
        if p.cs:
            if variant == "colsum_only_skipped" and p.M == 0:
                continue
            n = p.rows if variant == "colsum_over_rows" else p.cs_rows
            if variant == "drop_last_row" and n == p.rows:
                n -= 1
            cs = np.zeros(p.N, np.float32)
            for r0 in range(0, n, 64):
                cs = cs + pb.b(r0, min(n, r0 + 64)).sum(axis=0, dtype=np.float32)
            got["cs"][i][GUARD_LO:GUARD_LO + p.N] = cs
    return got


def applies(case, variant):
    """The cases on which a broken variant differs from the contract at all."""
    c = case
    if c.declines:
        return False
    gemm = [i for i, p in enumerate(c.probs) if p.M > 0]
    chunks = lambda i: -(-c.probs[i].rows // c.chunking(i)[1])              # noqa: E731
    return {
        "drop_last_row": True,
        "odd_tail_uses_pad_row": any(_odd_tail(c, i) for i in gemm),
        "a_row_past_rows": any(_odd_tail(c, i) or (not c.chunking(i)[0] and c.probs[i].rows % 16) for i in gemm),
        "a_col_past_M": any(c.probs[i].lda > c.probs[i].M and c.probs[i].rows > 1 for i in gemm),
        "colsum_over_rows": any(p.cs and p.cs_rows < p.rows for p in c.probs),
        "batch_col_perm": c.kind == "batch" and bool(gemm),
        "batch_wrong_problem_offset": c.kind == "batch" and len(gemm) >= 2,
        "colsum_only_skipped": any(p.M == 0 for p in c.probs),
        "chunk_dropped": any(chunks(i) >= 2 for i in gemm),
        "swapped_not_transposed": c.swapped,
        "write_past_C": bool(gemm),
        "write_past_part": True,
    }[variant]


# ---- the descriptors -------------------------------------------------------------------------------------------------
def fill_descs(descs, Bf, ptr):
    """Fills gan_mpc_amd._lib.WgradDesc's (one per problem) from the buffers; ptr(name, array, offset) -> address of
    array[offset] (device memory for a launch, any number with the same alignment for the route queries).  -> the address
    of part[0] (behind its leading guard words)."""
    c = Bf.case
    part = ptr("part", Bf.part0, GUARD_LO)
    for i, (d, pb) in enumerate(zip(descs, Bf.probs)):
        p = pb.p
        d.rows, d.M, d.N, d.ldb, d.cs_rows = p.rows, p.M, p.N, p.ldb, p.cs_rows
        d.B = ptr(f"B{i}", pb.B, p.b_off)
        d.colsum = ptr(f"cs{i}", pb.cs0, GUARD_LO) if p.cs else None
        if p.M > 0:
            d.A, d.lda, d.C = ptr(f"A{i}", pb.A, A_OFF), p.lda, ptr(f"C{i}", pb.C0, GUARD_LO)
        else:
            d.A, d.lda, d.C = d.B, p.ldb, d.colsum
        d.mfma_ok = 1 if c.mfma_ok else 0
        d.form = 1 if c.form == "colsum_only" else 0
        d.part, d.part_floats = part, c.part_floats
    return part


def route_of(lib, desc):
    """gmpc_wgrad_route as a tuple in the form of Case.route, and (rows per chunk, chunks) of the column-sum kernel."""
    r = (C.c_int * 6)()
    assert lib.gmpc_wgrad_route(C.byref(desc), r) == 0
    form = FORMS[r[0]]
    if form == "colsum":
        return (form, 0, r[4], r[5]), (r[4], r[5])
    return (form, r[1], r[2], r[3]), (r[4], r[5])


def batch_route_of(lib, descs, np_, part_floats):
    """gmpc_wgrad_batch_route -> the batch's rows per chunk, 0 when the launcher declines it."""
    r = (C.c_int * 2)()
    assert lib.gmpc_wgrad_batch_route(descs, np_, part_floats, r) == 0
    assert (r[0] == 0) == (r[1] == 0)
    return r[1]
