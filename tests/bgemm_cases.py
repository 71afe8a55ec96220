"""The batched TN GEMM family (csrc/gmpc_bgemm.hip): case table, buffers, fp64 reference, checker (TEST INFRASTRUCTURE, no
GPU import).

Shared by tests/test_bgemm_cases.py (CPU: the table reaches every kernel instantiation the dispatcher can launch, the
checker rejects broken kernels) and tests/test_gpu_bgemm.py (GPU: every case through gmpc_bgemm_tn_ex).

Each operand is built as its ALLOCATION: a flat fp32 array in which the logical matrix of batch element b starts at
off + b * stride and has leading dimension ld >= its width.  Everything the contract does not let the kernel use is a
NaN: gap columns, gaps between batch elements, the pad after Y, every input of an inactive batch element.  C is
pre-filled with NaNs that carry their own index as payload, except the logical matrices of active elements when beta
reads them."""

import ctypes as C

import numpy as np

# route families (gmpc_launch.h) -- ("strips", NTW) | ("thin", WIDE_X, NTJ, NS) | ("lds", WNT, KC, VEC)
FAMILIES = ("strips", "thin", "lds")
ALL_ROUTES = ([("strips", w) for w in (1, 2, 4, 6, 8)]
              + [("thin", wx, 2, ns) for wx in (1, 0) for ns in (1, 2)] + [("thin", 1, 4, 1), ("thin", 0, 4, 1)]
              + [("lds", 2, 8, 0), ("lds", 2, 8, 1), ("lds", 3, 8, 0), ("lds", 3, 16, 1), ("lds", 4, 8, 0),
                 ("lds", 4, 16, 1)])
BT_RD = 10                      # k_bthin's k-steps in flight: the streaming form needs K >= 2 BT_RD
U = 2.0 ** -24                  # unit roundoff of fp32
PAIRS = ((1.0, 0.0), (0.5, 0.0), (2.0, 0.0), (-1.0, 1.0), (0.5, -2.0))     # the driver's (alpha, beta) + the old test's
ACTIVE5 = (0, 1, 0, 1, 0)       # a 0 first, last and in the middle


def y_pad(ldy):
    """Readable floats the contract asks for after row K - 1 of the last Y: the strips read up to 4 rows past K and up
    to 32 NTW - 1 <= 255 columns past N."""
    return max(8 * ldy, 4 * ldy + 256)


def strips_y_extent(K, ldy, N, ntw):
    """Floats of Y[b] the one-wave strips touch, counted from Y[b] (mirror of gemm_tile's read schedule in
    gmpc_device.h: k-steps 0 and 1 up front, then three more per round of 6 rows while k0 + 6 <= Kp)."""
    Kp = K & ~1
    last = K - 1
    if Kp > 0:
        last = max(last, 3)
        k0 = 0
        while k0 + 6 <= Kp:
            last = max(last, k0 + 9)
            k0 += 6
    npad = -(-N // (32 * ntw)) * 32 * ntw
    return last * ldy + npad


class Case:
    """One product.  `window`: every operand is a column window of a wider buffer (odd leading dimension, column offset
    2) with a gap between batch elements; `share` = "x" / "y": that operand has batch stride 0; En: columns of the
    addend E (None: no E); mask: None | "rand" | "words" (b = 0 has an all-clear and an all-set word)."""

    def __init__(self, group, M, N, K, batch, route, K2=0, K3=0, alpha=1.0, beta=0.0, window=False, share="",
                 active=None, En=None, mask=None, upper=False, tag=""):
        self.group, self.M, self.N, self.K, self.batch, self.route = group, M, N, K, batch, tuple(route)
        self.K2, self.K3, self.alpha, self.beta = K2, K3, float(alpha), float(beta)
        self.window, self.share, self.active, self.En, self.mask, self.upper = window, share, active, En, mask, upper
        opts = [f"K2={K2}" if K2 else "", f"K3={K3}" if K3 else "", "win" if window else "",
                f"s{share}0" if share else "", "act" if active else "", f"E{En}" if En is not None else "",
                f"mask-{mask}" if mask else "", "upper" if upper else "", tag]
        self.id = "-".join([group, f"{M}x{N}x{K}b{batch}", f"a{alpha:g}b{beta:g}"] + [o for o in opts if o])

    @property
    def family(self):
        return self.route[0]

    @property
    def ksum(self):
        return self.K + self.K2 + self.K3


def _cases():
    out = []
    n_plain = [0]

    def plain(M, N, K, batch, route, **kw):
        a, b = PAIRS[n_plain[0] % len(PAIRS)]
        n_plain[0] += 1
        out.append(Case("plain", M, N, K, batch, route, alpha=a, beta=b, **kw))

    # ---- the plain product, every instantiation: one odd and one even K (strips, thin: K = 2 BT_RD and one just
    # above that is no multiple of BT_RD); K < KC, = KC, = 2 KC, = 2 KC + 1 and one more (LDS)
    for (M, N, batch, ntw), Ks in [((7, 5, 3, 1), (3, 4)), ((100, 17, 2, 1), (17, 12)), ((7, 77, 3, 2), (70, 7)),
                                   ((30, 102, 2, 4), (33, 6)), ((5, 131, 2, 4), (19, 8)), ((9, 190, 2, 6), (19, 14)),
                                   ((31, 250, 2, 8), (7, 18))]:
        for K in Ks:
            plain(M, N, K, batch, ("strips", ntw))
    for (M, N, batch, wx, ntj, ns), Ks in [((130, 5, 3, 1, 2, 1), (33, 20, 23)), ((7, 131, 3, 0, 2, 1), (35, 20, 21)),
                                           ((129, 33, 2, 1, 2, 2), (21, 20)), ((64, 130, 2, 0, 2, 2), (20, 23))]:
        for K in Ks:
            plain(M, N, K, batch, ("thin", wx, ntj, ns))
    # 16-byte streaming form: batch * ceil(W / 128) * strips >= 4096 waves; the wide operand is shared (stride 0);
    # widths 129, 130, 131 are its three ragged shifts
    for M, N, K in [(131, 5, 21), (130, 5, 21), (129, 5, 21), (131, 5, 20)]:
        plain(M, N, K, 2048, ("thin", 1, 4, 1), share="x")
    for M, N, K in [(5, 130, 23), (5, 131, 20)]:
        plain(M, N, K, 2048, ("thin", 0, 4, 1), share="y")
    for (M, N, batch, wnt, kc, vec), Ks in [((40, 70, 3, 2, 8, 0), (33, 5, 8, 16, 17)),
                                            ((36, 68, 3, 2, 8, 1), (8, 5, 16, 17)),
                                            ((33, 131, 2, 3, 8, 0), (17, 5, 8, 16)),
                                            ((129, 257, 2, 3, 8, 0), (5, 33)),
                                            ((132, 132, 2, 3, 16, 1), (16, 7, 32, 33)),
                                            ((35, 201, 2, 4, 8, 0), (9, 5, 8, 16, 17)),
                                            ((68, 196, 2, 4, 16, 1), (35, 7, 16, 32, 33))]:
        for K in Ks:
            plain(M, N, K, batch, ("lds", wnt, kc, vec))

    # ---- one case per family (both operand orders of the streaming kernel) for layout, `active` and (alpha, beta)
    reps = [(7, 77, 7, ("strips", 2)), (130, 5, 33, ("thin", 1, 2, 1)), (7, 131, 35, ("thin", 0, 2, 1)),
            (40, 70, 33, ("lds", 2, 8, 0))]
    for M, N, K, route in reps:
        out.append(Case("layout", M, N, K, 3, route, alpha=0.5, beta=-2.0, window=True))
        out.append(Case("layout", M, N, K, 3, route, alpha=0.5, beta=-2.0, share="x"))
        out.append(Case("layout", M, N, K, 3, route, alpha=0.5, beta=-2.0, share="y"))
        out.append(Case("active", M, N, K, 5, route, alpha=-1.0, beta=1.0, active=ACTIVE5))
        out.append(Case("active", M, N, K, 5, route, alpha=1.0, beta=0.0, active=ACTIVE5, window=True))
        for a, b in PAIRS:
            out.append(Case("scale", M, N, K, 2, route, alpha=a, beta=b))
    # the 16-byte forms with windows of odd leading dimension (rows that do not start on 16 bytes) and `active`
    out.append(Case("layout", 131, 5, 21, 2048, ("thin", 1, 4, 1), alpha=0.5, beta=-2.0, share="x", window=True))
    out.append(Case("layout", 5, 130, 23, 2048, ("thin", 0, 4, 1), alpha=0.5, beta=-2.0, share="y", window=True))
    out.append(Case("active", 132, 132, 33, 5, ("lds", 3, 16, 1), active=ACTIVE5, window=True))

    # ---- options of the LDS-staged kernel
    tiny = ("lds", 2, 8, 0)
    out.append(Case("opt", 5, 3, 4, 2, tiny, En=3))
    out.append(Case("opt", 5, 3, 4, 2, tiny, mask="rand"))
    out.append(Case("opt", 5, 3, 4, 2, tiny, K2=3))
    # rows masked, X shared (the S_{l-1} product): a mask word boundary inside (40, 70) and at the edge (64)
    out.append(Case("opt", 40, 33, 9, 3, tiny, share="x", mask="rand"))
    out.append(Case("opt", 64, 33, 9, 3, ("lds", 2, 8, 0), share="x", mask="rand"))
    out.append(Case("opt", 70, 33, 9, 3, tiny, share="x", mask="words"))
    out.append(Case("opt", 70, 33, 9, 5, tiny, share="x", mask="words", active=ACTIVE5, window=True))
    out.append(Case("opt", 40, 70, 9, 2, tiny, En=70))
    out.append(Case("opt", 40, 70, 9, 2, tiny, En=37))
    out.append(Case("opt", 40, 70, 9, 2, tiny, En=37, alpha=0.5))
    out.append(Case("opt", 40, 70, 9, 3, tiny, En=37, alpha=0.5, mask="rand", window=True))
    # three K-segments, each with its own tail and leading dimension
    out.append(Case("opt", 40, 70, 10, 2, tiny, K2=6, K3=10))
    out.append(Case("opt", 40, 70, 16, 2, tiny, K2=8))
    out.append(Case("opt", 40, 70, 16, 2, tiny, K2=11))
    out.append(Case("opt", 132, 132, 10, 2, ("lds", 3, 16, 1), K2=6, K3=10))
    out.append(Case("opt", 132, 132, 16, 2, ("lds", 3, 16, 1), K2=8))
    out.append(Case("opt", 35, 201, 10, 2, ("lds", 4, 8, 0), K2=6, K3=10, window=True))
    out.append(Case("opt", 68, 196, 17, 3, ("lds", 4, 16, 1), K2=33, K3=5, alpha=0.5, En=100, window=True))
    # upper-only symmetric results: T1 = A^T (PA) + [K; V]^T [V; K] and the low-rank T1 (three segments + E)
    for n, route in [(70, ("lds", 2, 8, 0)), (128, ("lds", 2, 8, 1)), (130, ("lds", 3, 8, 0)), (196, ("lds", 2, 8, 1)),
                     (257, ("lds", 2, 8, 0)), (260, ("lds", 2, 8, 1))]:
        out.append(Case("upper", n, n, 9, 2, route, K2=6, upper=True))
        out.append(Case("upper", n, n, 11, 2, route, K2=6, K3=10, En=n, upper=True, window=(n in (130, 260))))
    # upper_only alone does not route: the strips return the full product
    out.append(Case("upper", 20, 20, 7, 2, ("strips", 1), upper=True))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _cases()
# one case per family whose second launch must give the same bits: the first of each in the table
REPEAT_IDS = tuple(next(c.id for c in CASES if c.family == f) for f in FAMILIES)


# ---- buffers ---------------------------------------------------------------------------------------------------------
class Operand:
    """A flat fp32 allocation holding `nb` logical rows x width matrices (nb = 1: shared by the batch)."""

    def __init__(self, rows, width, batch, shared, window, tail, extra_ld=0):
        # tail: floats after the last matrix, or a function of the leading dimension that gives them
        self.rows, self.width, self.batch = rows, width, batch
        if window:
            self.ld = width + 2 * extra_ld + (3 if width % 2 == 0 else 4)       # odd
            self.off = 2
        else:
            self.ld, self.off = width + extra_ld, 0
        self.stride = 0 if shared else rows * self.ld + (7 if window else 0)
        nb = 1 if shared else batch
        self.size = self.off + (nb - 1) * self.stride + rows * self.ld + (tail(self.ld) if callable(tail) else tail)
        self.a = np.full(self.size, np.nan, np.float32)

    def idx(self, b=None, rows=None, width=None):
        """Flat indices of the logical matrix of element b (all elements: b = None) -> [batch,] rows, width."""
        r = np.arange(self.rows if rows is None else rows)[:, None] * self.ld
        c = np.arange(self.width if width is None else width)[None, :]
        if b is not None:
            return self.off + b * self.stride + r + c
        return self.off + np.arange(self.batch)[:, None, None] * self.stride + r[None] + c[None]

    def put(self, b, values):
        self.a[self.idx(b)] = values

    def logical(self):
        return self.a[self.idx()]


def nan_payload(size):
    """Quiet NaNs whose mantissa carries 1 + index mod 2^22 - 1: a float moved from elsewhere in C is told apart."""
    bits = np.uint32(0x7FC00000) | (np.uint32(1) + (np.arange(size, dtype=np.uint64) % 0x3FFFFE).astype(np.uint32))
    return bits.view(np.float32)


class Buffers:
    pass


def build(case):
    """Allocations of one case, filled by the rules in the module docstring."""
    c = case
    seed = int.from_bytes(c.id.encode(), "little") % (2 ** 32)
    rng = np.random.default_rng(seed)
    B = Buffers()
    B.case = c
    B.act = np.ones(c.batch, bool) if c.active is None else np.asarray(c.active, bool)
    assert B.act.size == c.batch and B.act.any()
    segs = [(k, i) for i, k in enumerate((c.K, c.K2, c.K3)) if k > 0]
    B.seg = []
    for K, i in segs:
        # the segments' leading dimensions differ (extra_ld); only the first segment's operands are ever shared
        sx = c.share == "x" and i == 0
        sy = c.share == "y" and i == 0
        X = Operand(K, c.M, c.batch, sx, c.window, 3, extra_ld=i)
        Y = Operand(K, c.N, c.batch, sy, c.window, y_pad, extra_ld=2 * i)
        B.seg.append((K, X, Y))
    # values: symmetric products where the result is upper-only, as the driver's are
    for si, (K, X, Y) in enumerate(B.seg):
        for b in range(1 if X.stride == 0 else c.batch):
            if X.stride == 0 or B.act[b]:
                X.put(b, rng.standard_normal((K, c.M)))
        for b in range(1 if Y.stride == 0 else c.batch):
            if not (Y.stride == 0 or B.act[b]):
                continue
            if c.upper and si == 0 and X.stride != 0:
                S = rng.standard_normal((K, K)) / np.sqrt(K)
                Y.put(b, (S + S.T) @ X.a[X.idx(b)].astype(np.float64))                 # X^T (S X) is symmetric
            elif c.upper and K % 2 == 0 and X.stride != 0:
                xb = X.a[X.idx(b)]
                Y.put(b, np.concatenate([xb[K // 2:], xb[:K // 2]]))                   # [K; V]^T [V; K]
            else:
                Y.put(b, rng.standard_normal((K, c.N)))
    B.E = None
    if c.En is not None:
        # lde > N: a kernel that adds E past En reads a NaN, inside the allocation
        B.E = Operand(c.M, c.En, c.batch, False, c.window, 3, extra_ld=c.N - c.En + 1)
        for b in np.flatnonzero(B.act):
            e = rng.standard_normal((c.M, c.En))
            if c.upper:
                e = e + e.T
            B.E.put(b, e)
    B.mask, B.srm = None, 0
    if c.mask:
        nw = (c.M + 31) // 32
        B.srm = nw + 1                                   # one stray word between the elements' masks
        B.mask = rng.integers(0, 2 ** 32, size=c.batch * B.srm, dtype=np.uint64).astype(np.uint32)
        if c.mask == "words":
            first = int(np.flatnonzero(B.act)[0])
            B.mask[first * B.srm] = 0
            B.mask[first * B.srm + 1] = 0xFFFFFFFF
    B.Cop = Operand(c.M, c.N, c.batch, False, c.window, 5)
    B.Cop.a = nan_payload(B.Cop.size).copy()
    B.C0 = None                                          # the logical pre-fill beta reads
    if c.beta != 0.0:
        B.C0 = rng.standard_normal((c.batch, c.M, c.N)).astype(np.float32)
        for b in np.flatnonzero(B.act):
            B.Cop.put(b, B.C0[b])
    B.prefill = B.Cop.a.copy()
    return B


def mask_rows(B, b, shift=0, stride=None):
    """bool [M]: the rows of element b that rowmask keeps (bit r & 31 of word r >> 5)."""
    r = np.arange(B.case.M) + shift
    srm = B.srm if stride is None else stride
    words = B.mask[b * srm + (r >> 5)]
    return ((words >> (r & 31).astype(np.uint32)) & 1).astype(bool)


# ---- reference -------------------------------------------------------------------------------------------------------
def reference(B):
    """fp64 from the fp32 inputs: ref = alpha (X^T Y + X2^T Y2 + X3^T Y3) + beta C0 + E[:, :En], masked rows exactly 0;
    S = |alpha| sum |x||y| + |beta||C0| + |E|, the scale of the per-entry bound.  [batch, M, N]; inactive elements are
    left at NaN (nothing is compared there)."""
    c = B.case
    ref = np.full((c.batch, c.M, c.N), np.nan)
    S = np.full((c.batch, c.M, c.N), np.nan)
    for b in np.flatnonzero(B.act):
        p = np.zeros((c.M, c.N))
        s = np.zeros((c.M, c.N))
        for K, X, Y in B.seg:
            x = X.a[X.idx(0 if X.stride == 0 else b)].astype(np.float64)
            y = Y.a[Y.idx(0 if Y.stride == 0 else b)].astype(np.float64)
            p += x.T @ y
            s += np.abs(x).T @ np.abs(y)
        p *= c.alpha
        s *= abs(c.alpha)
        if c.beta != 0.0:
            p += c.beta * B.C0[b].astype(np.float64)
            s += abs(c.beta) * np.abs(B.C0[b].astype(np.float64))
        if B.E is not None:
            e = B.E.a[B.E.idx(b)].astype(np.float64)
            p[:, :c.En] += e
            s[:, :c.En] += np.abs(e)
        if B.mask is not None:
            keep = mask_rows(B, b)
            p[~keep] = 0.0
            s[~keep] = 0.0
        ref[b], S[b] = p, s
    return ref, S


# ---- checker ---------------------------------------------------------------------------------------------------------
def check(B, ref, S, got_flat, tol=1e-5, on_figures=None):
    """Asserts the contract on the C allocation `got_flat` the kernel left behind; returns the achieved figures:
    max_rel (max-norm relative error), entry (largest |got - ref| as a fraction of the per-entry bound).
    on_figures(dict) is called with them before they are asserted."""
    c = B.case
    got_flat = np.ascontiguousarray(got_flat, np.float32)
    assert got_flat.shape == B.prefill.shape
    gbits, pbits = got_flat.view(np.uint32), B.prefill.view(np.uint32)
    act = np.flatnonzero(B.act)
    idx = B.Cop.idx()[act]                                         # [active, M, N]
    # outside the written region: bit-identical to the pre-fill
    outside = np.ones(got_flat.size, bool)
    outside[idx.ravel()] = False
    moved = np.flatnonzero(outside & (gbits != pbits))
    assert moved.size == 0, f"{c.id}: {moved.size} floats outside the written region changed, first at {moved[:4]}"
    got = got_flat[idx].astype(np.float64)
    r, s = ref[act], S[act]
    need = np.ones(got.shape, bool)
    if c.upper:
        # below the diagonal the kernel may write the product or leave the pre-fill
        skipped = (gbits[idx] == pbits[idx]) & np.tril(np.ones((c.M, c.N), bool), -1)[None]
        need = ~skipped
    assert np.isfinite(got[need]).all(), \
        f"{c.id}: non-finite result at (b, row, col) = {np.argwhere(need & ~np.isfinite(got))[:4].tolist()}"
    err = np.where(need, np.abs(np.where(need, got, 0.0) - r), 0.0)
    max_rel = float(err.max() / (np.abs(r).max() + 1e-300))
    bound = (c.ksum + 4) * U * s
    over = err > bound
    ratio = float((err[s > 0] / bound[s > 0]).max()) if (s > 0).any() else 0.0
    if on_figures is not None:
        on_figures(dict(max_rel=max_rel, entry=ratio, entries=int(need.sum())))
    assert max_rel <= tol, f"{c.id}: max-norm relative error {max_rel:.3e} > {tol:.0e}"
    assert not over.any(), (f"{c.id}: {int(over.sum())} entries outside (K + 4) u S, worst {ratio:.3f} x the bound, first "
                            f"at (b, row, col) = {np.argwhere(over)[:4].tolist()}")
    if B.mask is not None:
        for j, b in enumerate(act):
            rows = ~mask_rows(B, b)
            z = gbits[idx[j][rows]]
            if c.upper:
                z = z[need[j][rows]]
            assert (z == 0).all(), f"{c.id}: masked rows of element {b} are not +0.0"
    return dict(max_rel=max_rel, entry=ratio)


# ---- the contract in fp32 NumPy, and ways to break it ----------------------------------------------------------------
VARIANTS = ("drop_last_col", "extra_col", "y_pad_row", "mask_shift", "mask_stride", "k2_tail", "e_past_en", "e_scaled",
            "write_inactive", "upper_hole")


def model_kernel(B, variant=None):
    """What a correct kernel leaves in the C allocation, computed in fp32 (None, "lower_hole": still correct), or one of
    the broken VARIANTS."""
    c = B.case
    out = B.prefill.copy()
    one = np.float32(1.0)
    alpha, beta = np.float32(c.alpha), np.float32(c.beta)
    for b in range(c.batch):
        if not B.act[b]:
            if variant == "write_inactive":
                out[B.Cop.idx(b)] = 0.0
            continue
        acc = np.zeros((c.M, c.N), np.float32)
        for si, (K, X, Y) in enumerate(B.seg):
            bx, by = (0 if X.stride == 0 else b), (0 if Y.stride == 0 else b)
            kk = K
            if variant == "k2_tail" and si == 1:
                kk = K - K % c.route[2]
            x, y = X.a[X.idx(bx, rows=kk)], Y.a[Y.idx(by, rows=kk)]
            if variant == "y_pad_row" and si == 0:
                x = np.concatenate([x, x[-1:]])
                y = Y.a[Y.idx(by, rows=K + 1)]
            if kk > 0:
                acc = acc + x.T @ y
        v = alpha * acc
        if c.beta != 0.0:
            v = beta * B.C0[b] + v
        if B.E is not None:
            en = c.N if variant == "e_past_en" else c.En
            e = B.E.a[B.E.idx(b, width=en)]
            v[:, :en] = v[:, :en] + (alpha if variant == "e_scaled" else one) * e
        if B.mask is not None:
            keep = mask_rows(B, b, shift=1 if variant == "mask_shift" else 0,
                             stride=0 if variant == "mask_stride" else None)
            v[~keep] = 0.0
        idx = B.Cop.idx(b)
        sel = np.ones((c.M, c.N), bool)
        if c.upper:
            sel = np.triu(sel)                                  # the lower triangle stays at its pre-fill
            if variant == "lower_hole":
                sel[:] = True
                sel[c.M - 1, 0] = False
            if variant == "upper_hole":
                sel[c.M // 3, c.N - 1 - c.N // 5] = False
        if variant == "drop_last_col":
            sel[:, c.N - 1] = False
        out[idx[sel]] = v[sel]
        if variant == "extra_col":
            out[B.Cop.idx(b, width=c.N + 1)[:, c.N]] = v[:, c.N - 1]
    return out


def applies(case, variant):
    """The cases on which a broken variant differs from the contract at all."""
    c = case
    return {"drop_last_col": True, "extra_col": c.window, "y_pad_row": True,
            "mask_shift": c.mask is not None, "mask_stride": c.mask is not None and c.batch > 1,
            "k2_tail": c.K2 > 0 and c.family == "lds" and c.K2 % c.route[2] != 0,
            "e_past_en": c.En is not None and c.En < c.N, "e_scaled": c.En is not None and c.alpha != 1.0,
            "write_inactive": c.active is not None, "upper_hole": c.upper, "lower_hole": c.upper}[variant]


# ---- the descriptor --------------------------------------------------------------------------------------------------
def fill_desc(desc, B, ptr):
    """Fills a gan_mpc_amd._lib.BgemmDesc from the buffers; ptr(name, array, offset) -> address of array[offset] (device
    memory for the launch, any non-zero number for the route query)."""
    c = B.case
    desc.batch, desc.M, desc.N, desc.K = c.batch, c.M, c.N, c.K
    desc.alpha, desc.beta = c.alpha, c.beta
    names = (("X", "sx", "ldx", "Y", "sy", "ldy", "K"), ("X2", "sx2", "ldx2", "Y2", "sy2", "ldy2", "K2"),
             ("X3", "sx3", "ldx3", "Y3", "sy3", "ldy3", "K3"))
    si = 0
    for i, K in enumerate((c.K, c.K2, c.K3)):
        xn, sxn, ldxn, yn, syn, ldyn, kn = names[i]
        if K == 0:
            setattr(desc, kn, 0)
            continue
        _, X, Y = B.seg[si]
        si += 1
        setattr(desc, kn, K)
        setattr(desc, xn, ptr(xn, X.a, X.off)); setattr(desc, sxn, X.stride); setattr(desc, ldxn, X.ld)
        setattr(desc, yn, ptr(yn, Y.a, Y.off)); setattr(desc, syn, Y.stride); setattr(desc, ldyn, Y.ld)
    desc.C, desc.sc, desc.ldc = ptr("C", B.prefill, B.Cop.off), B.Cop.stride, B.Cop.ld
    desc.active = ptr("active", B.act.astype(np.int32), 0) if c.active is not None else None
    if B.E is not None:
        desc.E, desc.se, desc.lde, desc.En = ptr("E", B.E.a, B.E.off), B.E.stride, B.E.ld, c.En
    if B.mask is not None:
        desc.rowmask, desc.srm = ptr("rowmask", B.mask, 0), B.srm
    desc.upper_only = 1 if c.upper else 0
    return desc


def route_of(lib, desc):
    """gmpc_bgemm_route as a tuple in the form of Case.route."""
    r = (C.c_int * 4)()
    assert lib.gmpc_bgemm_route(C.byref(desc), r) == 0
    fam = FAMILIES[r[0]]
    return (fam, r[1]) if fam == "strips" else (fam, r[1], r[2], r[3])
