"""The dense Jacobian chain k_linearize_mfma<NT, NTF> (csrc/gmpc_linearize_mfma.hip): case table, buffers, fp64 reference,
checker and an fp32 model of the kernel's structure with ways to break it (TEST INFRASTRUCTURE, no GPU import).

Shared by tests/test_linearize_cases.py (CPU: the table reaches every instantiation, staging combination and input-GEMM
body according to gmpc_linearize_route; the checker passes the model and rejects every mutation) and
tests/test_gpu_linearize_dense.py (GPU: every case through gmpc_linearize_ex).

    J[s] = W_L^T D_{L-1}(s) W_{L-1}^T ... D_1(s) W_1^T + [I | 0]          [n][n + m] per sample s

with D_l(s) taken from the GIVEN relu bits: no forward pass, so no kinks, and every entry of every case is compared.

Buffers of one (case, fill):
  weights  the flat dynamics parameter vector W_0 | b_0 | W_1 | b_1 | ... (W_l is (in, out) row-major); two sets, for
           the second gmpc_set_params.  "exact": integers chosen so that every partial sum of the chain is an integer
           below 2^22, W_L scaled by a power of two so that entries are O(1) -- the result is the fp64 one bit for bit in
           any order of summation; "normal": seeded Gaussians over sqrt(fan-in).
  masks    [Smask][Lh][8] words for ALL Smask = B T samples of the engine; a strided launch (large state: samp_mul = T,
           samp_add = t) reads B of them, the others hold the bits of the other time steps.  Bits at or past a
           layer's width are set at random (the contract allows them) in every kind but "zeros".
  AB       8 guard words, nsamp n (n + m) floats, 8 guard words, all NaNs whose payload names their place.
  active   None, or one int per trajectory."""

import numpy as np

U = 2.0 ** -24                        # unit roundoff of fp32
MW = 8                                # GMPC_MW: mask words per (sample, hidden layer)
PADROWS = 24                          # GMPC_LIN_PADROWS
LDS_MAX = 160 * 1024
FILLS = ("exact", "normal")
MASK_KINDS = ("random", "ones", "zeros", "unit", "edge")
ACTIVE_KINDS = ("null", "on", "off", "mixed")
GUARD = 8


class Case:
    """n, m, hidden widths; B trajectories of T steps.  big: a large-state engine (n > 64 or m > 32), launched as one
    time step t of every trajectory (nsamp = B, samp_mul = T, samp_add = t); otherwise the whole batch (nsamp = B T).
    want: what gmpc_linearize_route must report for the launch (NT, NTF, NGF, stage_w1, stage_wl, body)."""

    def __init__(self, n, m, hidden, want, mask="random", active="null", B=3, T=3, t=None):
        self.n, self.m, self.hidden, self.want = n, m, tuple(hidden), want
        self.mask, self.active, self.B, self.T = mask, active, B, T
        self.big = n > 64 or m > 32
        assert self.big == (t is not None) and mask in MASK_KINDS and active in ACTIVE_KINDS
        self.samp_mul, self.samp_add = (T, t) if self.big else (1, 0)
        self.nsamp = B if self.big else B * T
        self.smask = B * T
        self.dims = (n + m,) + self.hidden + (n,)
        self.Lh = len(hidden)
        self.nm = n + m
        self.id = "n%dm%d-%s-%s-%s%s" % (n, m, "x".join(map(str, hidden)), mask, active,
                                          "" if (B, T) == (3, 3) else "-B%dT%d" % (B, T))

    @property
    def strided(self):
        return (self.samp_mul, self.samp_add) != (1, 0)

    @property
    def entries(self):
        return self.nsamp * self.n * self.nm

    def kp(self, l):
        """Padded contraction length of the GEMM that consumes hidden layer l (0-based)."""
        return (self.dims[l + 1] + 1) & ~1


def _cases():
    out = []

    def c(n, m, hidden, NT, NTF, NGF, w1, wl, body, **kw):
        out.append(Case(n, m, hidden, dict(NT=NT, NTF=NTF, NGF=NGF, stage_w1=w1, stage_wl=wl, body=body), **kw))

    # ---- n + m <= 32: one input tile; two or more hidden layers take the six-deep ring
    c(1, 1, (1,), 1, 1, 1, 1, 1, "single")
    c(2, 1, (13, 31), 1, 1, 1, 1, 1, "ring", mask="edge")                  # Kp = 14: the ring's furthest read-ahead
    c(17, 6, (32, 32), 1, 1, 1, 1, 1, "ring", mask="ones")                 # ring runs to k = 36 past the slab's 33 columns
    c(17, 6, (33, 40), 2, 1, 1, 1, 1, "ring", active="mixed")
    c(31, 1, (96, 7), 3, 1, 1, 1, 1, "ring", mask="unit")
    c(5, 3, (100, 100), 4, 1, 1, 1, 1, "ring", active="on")
    c(17, 6, (150, 160, 40), 5, 1, 1, 1, 1, "ring", mask="edge", active="mixed")
    c(3, 2, (192, 170), 6, 1, 1, 1, 1, "ring", mask="zeros")
    c(17, 6, (200, 150), 7, 1, 1, 1, 1, "ring", active="off")
    c(17, 6, (224,), 7, 1, 1, 1, 0, "single", mask="edge")                 # one hidden layer, W_1^T staged alone
    c(17, 6, (256, 256), 8, 1, 1, 0, 1, "ring", mask="edge")               # the reference's n, m at 2 x 256: W_L alone
    c(29, 3, (256, 256), 8, 1, 1, 0, 0, "ring")                            # neither operand staged
    c(22, 3, (200, 256), 8, 1, 1, 1, 0, "ring", mask="ones", active="mixed")      # W_1^T alone
    c(29, 3, (256,), 8, 1, 1, 0, 0, "single", mask="unit")
    c(17, 6, (256,), 8, 1, 1, 0, 1, "single", active="mixed")
    c(2, 2, (40, 256, 7), 8, 1, 1, 1, 1, "ring", mask="edge")              # non-monotone widths
    c(4, 2, (9, 33, 31, 12, 255, 6, 18), 8, 1, 1, 1, 1, "ring", active="mixed")   # seven hidden layers
    c(31, 1, (255, 1, 256), 8, 1, 1, 0, 0, "ring", mask="ones")
    c(1, 1, (5, 3), 1, 1, 1, 1, 1, "ring", active="mixed", B=10925, T=3)   # 1025 tiles: the persistent loop wraps
    # ---- 33 <= n + m <= 64: two input tiles (gemm_tile)
    c(32, 1, (31,), 1, 2, 1, 1, 1, "single", mask="edge")
    c(33, 2, (64, 33), 2, 2, 1, 1, 1, "multi", active="mixed")
    c(32, 32, (65, 96), 3, 2, 1, 1, 1, "multi", mask="ones")
    c(33, 31, (128, 100, 128), 4, 2, 1, 1, 1, "multi", mask="unit")
    c(40, 5, (129,), 5, 2, 1, 1, 1, "single", active="off")
    c(50, 14, (192, 12), 6, 2, 1, 1, 1, "multi", mask="zeros")
    c(33, 1, (200, 200), 7, 2, 1, 0, 1, "multi", mask="edge")              # too wide an input for the register chain
    c(40, 8, (256, 255), 8, 2, 1, 0, 0, "multi", active="mixed")
    # ---- 65 <= n + m <= 96: three input tiles
    c(64, 1, (32,), 1, 3, 1, 1, 1, "single", active="mixed")
    c(64, 32, (33, 64), 2, 3, 1, 1, 1, "multi", mask="edge")
    c(40, 30, (96, 96, 96), 3, 3, 1, 1, 1, "multi")
    c(64, 2, (128,), 4, 3, 1, 1, 1, "single", mask="ones")
    c(35, 32, (130, 160), 5, 3, 1, 1, 0, "multi", mask="unit", active="mixed")
    c(64, 5, (161,), 6, 3, 1, 0, 1, "single", mask="zeros")
    c(64, 3, (7, 224), 7, 3, 1, 1, 0, "multi", mask="edge")
    c(64, 32, (256, 256, 256), 8, 3, 1, 0, 0, "multi", active="on")
    # ---- large state: one time step of every trajectory, input GEMM in groups of eight tiles
    c(60, 40, (20, 32), 1, 8, 1, 1, 1, "multi", t=1)
    c(100, 3, (64, 50), 2, 8, 1, 1, 1, "multi", mask="edge", active="mixed", t=2)
    c(65, 40, (96,), 3, 8, 1, 0, 1, "single", mask="ones", t=1)
    c(129, 1, (128, 65), 4, 8, 1, 0, 1, "multi", mask="unit", t=2)
    c(260, 10, (160, 130), 5, 8, 2, 0, 0, "multi", active="mixed", t=1)    # two column groups
    c(97, 33, (33, 192), 6, 8, 1, 1, 0, "multi", mask="zeros", t=2)
    c(128, 64, (200, 210), 7, 8, 1, 0, 0, "multi", mask="edge", t=1)
    c(500, 20, (256, 256), 8, 8, 3, 0, 0, "multi", active="mixed", t=2)    # three column groups
    c(300, 5, (256,), 8, 8, 2, 0, 0, "single", mask="ones", active="off", t=1)
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES), sorted(c.id for c in CASES)
# (the GPU test repeats the launch and swaps the weights in EVERY case.)  The cases on which the CPU test shows that the
# second parameter set cannot pass on the first set's Jacobians: dense bits and every sample compared
REPEAT_IDS = tuple(c.id for c in CASES if c.active == "null" and c.mask in ("random", "edge"))


# ---- buffers ---------------------------------------------------------------------------------------------------------
def nan_payload(size, base=0):
    """Quiet NaNs whose mantissa carries 1 + (base + index) mod 2^22 - 2: a float moved from elsewhere is told apart."""
    k = (np.arange(size, dtype=np.uint64) + np.uint64(base)) % np.uint64(0x3FFFFE)
    return (np.uint32(0x7FC00000) | (np.uint32(1) + k.astype(np.uint32))).view(np.float32)


class Buffers:
    pass


def _exact_weights(case, rng):
    """Integer weights whose chain has only integer partial sums below 2^22 under ANY masks, the last k rows of every
    contraction non-zero (a dropped tail shows); W_L scaled by a power of two so that |J - [I | 0]| <= 1."""
    dims, Lh = case.dims, case.Lh
    g = min(8.0, (2.0 ** 21) ** (1.0 / (Lh + 1)))                    # growth of |partial sum| allowed per contraction
    Ws = []
    for l in range(Lh):
        K = dims[l + 1]                                              # contracted with the rows of the operand above
        forced = int(min(4, K, max(1, g // 2)))
        p = min(1.0, max(0.0, (g - forced) / 1.5) / K)
        W = ((rng.random((dims[l], K)) < p) * rng.choice((-1.0, 1.0), size=(dims[l], K)))
        W[:, K - forced:] = rng.choice((-1.0, 1.0), size=(dims[l], forced))
        Ws.append(W)
    Ws.append(rng.integers(1, 3, size=(dims[Lh], dims[Lh + 1])) * rng.choice((-1.0, 1.0), size=(dims[Lh], dims[Lh + 1])))
    S = np.abs(Ws[Lh]).T
    for l in range(Lh - 1, -1, -1):
        S = S @ np.abs(Ws[l]).T
    assert S.max() < 2.0 ** 22, (case.id, S.max())
    Ws[Lh] = Ws[Lh] * 2.0 ** -int(np.ceil(np.log2(S.max())))
    return [W.astype(np.float32) for W in Ws]


def _normal_weights(case, rng):
    return [(rng.standard_normal((case.dims[l], case.dims[l + 1])) / np.sqrt(case.dims[l])).astype(np.float32)
            for l in range(case.Lh + 1)]


def pack_dyn(case, Ws, rng):
    """The flat parameter vector W_0 | b_0 | W_1 | b_1 | ...  The biases do not enter the Jacobian and lie between the
    weight blocks the padded operands are built from: +-1e30 (the hostile part of every fill -- a builder or a kernel that
    strays into one cannot go unnoticed)."""
    def bias(k):
        return (1e30 * (1.0 + 0.01 * (np.arange(k) % 7)) * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    return np.concatenate([np.concatenate([W.ravel(), bias(W.shape[1])]) for W in Ws])


def _set_units(words, units):
    for u in units:
        words[u >> 5] |= np.uint32(1 << (u & 31))


def _masks(case, rng):
    """[Smask][Lh][MW] words; neighbouring samples differ in every kind."""
    S, Lh = case.smask, case.Lh
    mk = np.zeros((S, Lh, MW), np.uint32)
    past = rng.integers(0, 2 ** 32, size=(S, Lh, MW), dtype=np.uint64).astype(np.uint32)
    rnd = rng.integers(0, 2 ** 32, size=(S, Lh, MW), dtype=np.uint64).astype(np.uint32)
    for l in range(Lh):
        w = case.dims[l + 1]
        inside = np.zeros(MW, np.uint32)
        _set_units(inside, range(w))
        for s in range(S if S <= 64 else 64):
            words = np.zeros(MW, np.uint32)
            if case.mask == "random":
                words = rnd[s, l] & inside
                words[0] = (words[0] & ~np.uint32(1)) | np.uint32(s % 2)     # unit 0 alternates: neighbours differ
            elif case.mask == "ones":
                words = inside.copy()
                if s % 2:      # one unit off, another one in every layer
                    u = (s + 5 * l) % w
                    words[u >> 5] &= ~np.uint32(1 << (u & 31))
            elif case.mask == "zeros":
                if s % 2:
                    _set_units(words, [s % w])
            elif case.mask == "unit":
                _set_units(words, [((3 if w % 3 else 1) * s + l) % w])
            else:   # edge: the units around the word boundary, the layer's last unit, one that moves with the sample
                units = [w - 1, (s + l) % max(1, w - 1)]
                units += ([31] if s % 2 == 0 else []) + ([32] if s % 3 else []) + ([33] if s % 2 else [])
                _set_units(words, [u for u in units if u < w])
            mk[s, l] = words
        if S > 64:      # the wrap case: the first 64 patterns, rotated
            reps = -(-S // 64)
            mk[:, l] = np.tile(mk[:64, l], (reps, 1))[:S]
            mk[:, l] = np.where((np.arange(S) // 64 % 2 == 1)[:, None], mk[:, l] ^ (rnd[:, l] & inside), mk[:, l])
            mk[:, l, 0] = (mk[:, l, 0] & ~np.uint32(1)) | (np.arange(S) % 2).astype(np.uint32)
        if case.mask != "zeros":
            mk[:, l] |= past[:, l] & ~inside
            mk[:, l, MW - 1] |= np.uint32(1 << 31) & ~inside[MW - 1]     # the last bit of the last word
    return mk


def _active(case):
    if case.active == "null":
        return None
    b = np.arange(case.B)
    return {"on": np.ones(case.B, np.int32), "off": np.zeros(case.B, np.int32),
            "mixed": ((b % 2 == 1) | (b % 5 == 3)).astype(np.int32)}[case.active]


def build(case, fill):
    seed = int.from_bytes((case.id + fill).encode(), "little") % (2 ** 32)
    rng = np.random.default_rng(seed)
    Bf = Buffers()
    Bf.case, Bf.fill = case, fill
    mk = _exact_weights if fill == "exact" else _normal_weights
    Bf.W = [mk(case, rng), mk(case, rng)]                             # two parameter sets
    Bf.dyn = [pack_dyn(case, W, rng) for W in Bf.W]
    Bf.masks = _masks(case, rng)
    Bf.active = _active(case)
    Bf.AB0 = nan_payload(GUARD + case.entries + GUARD, 17).copy()
    return Bf


def sample_ids(case, strided_at_s=False):
    s = np.arange(case.nsamp)
    return s if strided_at_s else s * case.samp_mul + case.samp_add


def unpack_bits(words, width=32 * MW):
    """[..., MW] words -> [..., width] 0 / 1."""
    sh = np.arange(32, dtype=np.uint32)
    bits = (words[..., :, None] >> sh) & np.uint32(1)
    return bits.reshape(words.shape[:-1] + (32 * MW,))[..., :width]


# ---- reference -------------------------------------------------------------------------------------------------------
def reference(Bf, which=0):
    """fp64 from the fp32 weights and the given bits: J [nsamp][n][n + m], and the per-entry bound
    gamma_N (|W_L|^T D ... |W_1|^T) + 2^-24 |J|,  gamma_N = N u / (1 - N u),  N = sum over the contracted widths (+ 2)."""
    c = Bf.case
    W = [w.astype(np.float64) for w in Bf.W[which]]
    sid = sample_ids(c)
    M = np.broadcast_to(W[c.Lh].T, (c.nsamp, c.n, c.dims[c.Lh])).copy()
    S = np.abs(M)
    for l in range(c.Lh - 1, -1, -1):
        d = unpack_bits(Bf.masks[sid, l], c.dims[l + 1]).astype(np.float64)[:, None, :]
        M = (M * d) @ W[l].T
        S = (S * d) @ np.abs(W[l]).T
    J = M.copy()
    J[:, np.arange(c.n), np.arange(c.n)] += 1.0
    N = sum(c.dims[l + 1] + 2 for l in range(c.Lh))
    bound = (N * U / (1.0 - N * U)) * S + U * np.abs(J)
    return J, bound


# ---- checker ---------------------------------------------------------------------------------------------------------
def check(Bf, ref, got, on_figures=None):
    """Asserts the contract on the AB allocation a launch left behind; -> entries compared against the reference."""
    c = Bf.case
    J, bound = ref
    got = np.ascontiguousarray(got, np.float32)
    assert got.shape == Bf.AB0.shape
    gb, pb = got.view(np.uint32), Bf.AB0.view(np.uint32)
    guard = np.ones(got.size, bool)
    guard[GUARD:GUARD + c.entries] = False
    moved = np.flatnonzero(guard & (gb != pb))
    assert moved.size == 0, f"{c.id}: {moved.size} guard words changed, first at {(moved[:4] - GUARD).tolist()}"
    body = got[GUARD:GUARD + c.entries].reshape(c.nsamp, c.n, c.nm)
    untouched = (gb == pb)[GUARD:GUARD + c.entries].reshape(c.nsamp, c.n, c.nm)
    on = np.ones(c.nsamp, bool) if Bf.active is None else Bf.active[sample_ids(c) // c.T] != 0
    if Bf.active is not None and not Bf.active.any():
        assert untouched.all(), f"{c.id}: {int((~untouched).sum())} entries written with every trajectory inactive"
        return 0
    with np.errstate(invalid="ignore"):
        err = np.abs(body.astype(np.float64) - J)
        err = np.where(np.isfinite(body), err, np.inf)
    if Bf.fill == "exact":
        want = J.astype(np.float32)
        assert (want.astype(np.float64) == J).all()                  # the reference itself is exact in fp32
        good = body.view(np.uint32) == want.view(np.uint32)
    else:
        good = err <= bound
    if on_figures is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))[on]
        on_figures(dict(entry=float(q.max()), max_err=float(err[on].max()), entries=int(on.sum()) * c.n * c.nm))
    bad = np.argwhere(~good & on[:, None, None])
    assert bad.size == 0, (f"{c.id} {Bf.fill}: {len(bad)} of {int(on.sum()) * c.n * c.nm} entries of active samples wrong, "
                           f"first (sample, row, column) {bad[:4].tolist()}: got {[float(body[tuple(b)]) for b in bad[:4]]}, "
                           f"want {[float(J[tuple(b)]) for b in bad[:4]]}")
    # inactive samples: every row either untouched or right
    rows_ok = untouched.all(axis=2) | good.all(axis=2)
    badr = np.argwhere(~rows_ok & ~on[:, None])
    assert badr.size == 0, f"{c.id}: rows of inactive samples neither untouched nor right, first {badr[:4].tolist()}"
    compared = int(on.sum()) * c.n * c.nm
    if Bf.active is None or Bf.active.all():
        assert compared == c.entries
    return compared


# ---- the kernel's structure in fp32 NumPy, and ways to break it ------------------------------------------------------
VARIANTS = ("wrong_layer_bits", "tile_first_sample_bits", "odd_k_last_dropped", "tail1_dropped", "tail2_dropped",
            "ring_past_kp_not_zeroed", "hidden_tiles_lost", "identity_without_mod", "rows_past_end", "cols_past_end",
            "group_skipped", "group_repeated", "strided_masks_at_s", "skip_on_first_sample")


def _tile_first_sample(c):
    r = np.arange(c.nsamp * c.n)
    return (r // 32 * 32) // c.n


def _tiles_on(c, active):
    """Per row: its tile runs (some sample the tile touches is active)."""
    R = c.nsamp * c.n
    r = np.arange(R)
    if active is None:
        return np.ones(R, bool)
    on_s = active[sample_ids(c) // c.T] != 0
    tile = r // 32
    any_on = np.zeros(tile.max() + 1, bool)
    np.logical_or.at(any_on, tile, on_s[r // c.n])
    return any_on[tile]


def model_kernel(Bf, variant=None, which=0):
    """What a correct launch leaves in the AB allocation (variant None), computed in fp32 along the kernel's structure --
    rows stacked over samples in 32-row tiles, masks per row, padded k-loops, column tiles and groups, identity by the
    tile's first output coordinate --, or one of the broken VARIANTS."""
    c = Bf.case
    W = Bf.W[which]
    n, nm, Lh = c.n, c.nm, c.Lh
    NT, NTF = c.want["NT"], c.want["NTF"]
    out = Bf.AB0.copy()
    R = c.nsamp * n
    r = np.arange(R)
    row_s, row_o, in_tile = r // n, r % n, r % 32
    ms = _tile_first_sample(c) if variant == "tile_first_sample_bits" else row_s
    sid = ms if variant == "strided_masks_at_s" else ms * c.samp_mul + c.samp_add
    bits = []
    for l in range(Lh):
        src = (l + 1) % Lh if variant == "wrong_layer_bits" else l
        bits.append(unpack_bits(Bf.masks[sid, src], c.dims[l + 1]).astype(np.float32))
    M = W[Lh].T[row_o]                                               # the seed rows [R][dims[Lh]]
    for l in range(Lh - 1, -1, -1):
        K = c.dims[l + 1]
        Kp = (K + 1) & ~1
        ring = l == 0 and c.want["body"] == "ring"
        keep = K
        if variant == "odd_k_last_dropped" and K % 2:
            keep = K - 1
        if variant == "tail1_dropped" and not ring and Kp % 6 == 2:
            keep = Kp - 2
        if variant == "tail2_dropped" and not ring and Kp % 6 == 4:
            keep = Kp - 2
        raw = M                                                      # the slab: the unmasked accumulator
        A = (M * bits[l])[:, :keep]
        nxt = A @ W[l].T[:keep]
        if variant == "ring_past_kp_not_zeroed" and ring:
            # k-steps Kp .. 12 ceil(Kp / 12) - 1 of the slab G[32][32 NT + 1] against pad rows of ones: columns below
            # 32 NT are zero, the ones behind it are the next slab row's
            SK = 32 * NT + 1
            slab = np.zeros((R + 32, SK), np.float32)
            slab[:R, :K] = raw
            flat = slab.reshape(-1)
            extra = np.zeros(R, np.float32)
            for k in range(Kp, -(-Kp // 12) * 12):
                extra += flat[np.minimum(r * SK + k, flat.size - 1)]
            nxt = nxt + extra[:, None]
        if variant == "hidden_tiles_lost" and l >= 1:
            nxt[:, 32:] = 0.0
        M = nxt.astype(np.float32)
    # the identity: column (rem0 + o) % n of accumulator row o, rem0 the output coordinate of the tile's first row
    rem0 = (r // 32 * 32) % n
    icol = rem0 + in_tile if variant == "identity_without_mod" else (rem0 + in_tile) % n
    res = M.copy()
    hit = icol < nm
    res[r[hit], icol[hit]] += np.float32(1.0)
    body = out[GUARD:GUARD + c.entries].reshape(R, nm)
    if variant == "skip_on_first_sample" and Bf.active is not None:
        run = Bf.active[(_tile_first_sample(c) * c.samp_mul + c.samp_add) // c.T] != 0
    else:
        run = _tiles_on(c, Bf.active)
    cols = np.ones(nm, bool)
    if variant == "group_skipped":
        cols[32 * NTF:] = False
    if variant == "group_repeated" and nm > 32 * NTF:
        res[:, 32 * NTF:] = res[:, np.arange(32 * NTF, nm) % (32 * NTF)]
    body[np.ix_(run, cols)] = res[np.ix_(run, cols)]
    if run.any():
        if variant == "rows_past_end" and R % 32:
            out[GUARD + c.entries] = res[-1, 0]
        if variant == "cols_past_end" and nm % 32:
            out[GUARD + c.entries] = res[-1, -1]
    return out


def applies(case, variant, active):
    """The cases on which a broken variant can differ from the contract at all."""
    c = case
    R = c.nsamp * c.n
    some_on = active is None or active.any()
    kps = [c.kp(l) for l in range(c.Lh)]
    tiled = [kps[l] for l in range(c.Lh) if not (l == 0 and c.want["body"] == "ring")]
    straddle = bool((_tile_first_sample(c) != np.arange(R) // c.n).any())
    if not some_on:
        return False
    return {
        "wrong_layer_bits": c.Lh >= 2,
        "tile_first_sample_bits": straddle,
        "odd_k_last_dropped": any(c.dims[l + 1] % 2 for l in range(c.Lh)),
        "tail1_dropped": any(k % 6 == 2 for k in tiled),
        "tail2_dropped": any(k % 6 == 4 for k in tiled),
        "ring_past_kp_not_zeroed": c.want["body"] == "ring" and -(-kps[0] // 12) * 12 > 32 * c.want["NT"] + 1,
        "hidden_tiles_lost": c.Lh >= 2 and max(c.dims[1:c.Lh]) > 32,
        "identity_without_mod": straddle,
        "rows_past_end": R % 32 != 0,
        "cols_past_end": c.nm % 32 != 0,
        "group_skipped": c.want["NGF"] > 1,
        "group_repeated": c.want["NGF"] > 1,
        "strided_masks_at_s": c.strided,
        "skip_on_first_sample": active is not None and bool(
            (_tiles_on(c, active) & (active[(_tile_first_sample(c) * c.samp_mul + c.samp_add) // c.T] == 0)).any()),
    }[variant]
