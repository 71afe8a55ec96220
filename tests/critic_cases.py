"""The critic step's dispatch map and the sweep that covers it (TEST INFRASTRUCTURE, no GPU import).

Shared by tests/test_critic_cases.py (CPU: the table covers every cell the map has, its inputs stay inside the fp32
comparison's valid range) and tests/test_gpu_critic_sweep.py (GPU: every case against the fp64 oracle)."""

import numpy as np

import gan_mpc_oracle as orc
import gpu_util as gu

THREADS = 256     # GMPC_THREADS: one workgroup = 4 F gate columns at F = 64
HEAD_ROWS = 8     # k_head2 rows per workgroup (R = 4 G, G = 2 by default)
MAX_LAYERS = 8    # GMPC_MAX_LAYERS: head layers the API accepts
NXS = (4, 8, 17, 32)


def lstm2_nx(n, F):
    """gmpc_critic_lstm.hip, lstm2_nx(): the register-weight kernels' x width, 0 if they do not apply."""
    if F != 64 or n < 1 or n > 32:
        return 0
    return 4 if n <= 4 else 8 if n <= 8 else 17 if n <= 17 else 32


def critic_route(n, F):
    """Mirror of critic_forward_backward (gmpc_api_critic.hip).  gmpc_create allocates the wide-input buffers (xT, xproj)
    when n + F > GMPC_THREADS, and `widein = c->xT != nullptr`; `gen2 = !widein && c->lwp != nullptr &&
    gmpc_lstm2_supported(cd)`, where lwp exists exactly when lstm2_nx() != 0; otherwise gmpc_launch_lstm_fwd /
    gmpc_launch_lstm_bwd (gmpc_critic.hip) run k_lstm_fwd / k_lstm_bwd (run-time n, one form for every n) at F = 64
    and the strided k_lstm_fwd_g / k_lstm_bwd_g at every other F."""
    if n + F > THREADS:
        return ("wide",)
    nx = lstm2_nx(n, F)
    if nx:
        return ("gen2", nx)
    return ("gen1",) if F == 64 else ("generic",)


def bwd2_groups(Bc):
    """gmpc_critic_lstm.hip, bwd2_groups() at the production default: groups of 4 sequences per workgroup."""
    return 2 if Bc > 4 else 1


# head shapes (hidden widths; the output layer of width 1 follows).  Widths 65, 129, 193 leave the last wave of a layer
# with one neuron; DEEP uses every layer slot the API has (7 hidden + the output = GMPC_MAX_LAYERS).
H1 = (1,)
H17 = (17,)
HODD = (65, 129, 193)
H100 = (100, 255)
DEEP = (129, 100, 65, 255, 17, 193, 33)

# (n, F, T, Bc, head_hidden, seed): T1 = T + 1 steps, Bc sequences
CASES = [
    # register-weight kernels, NX = 4 (n = 1, 3 padded; 4 exact)
    (1, 64, 1, 3, HODD, 1),
    (4, 64, 2, 5, H1, 102),
    (3, 64, 3, 17, DEEP, 3),
    (4, 64, 40, 9, H100, 4),
    # NX = 8 (n = 6 padded, 8 exact)
    (6, 64, 1, 8, DEEP, 5),
    (8, 64, 2, 1, H17, 6),
    (8, 64, 3, 7, HODD, 7),
    (6, 64, 9, 16, H1, 8),
    # NX = 17 (n = 9, 16 padded, 17 exact)
    (9, 64, 1, 4, H100, 9),
    (16, 64, 2, 9, HODD, 10),
    (17, 64, 3, 16, H1, 111),
    (12, 64, 6, 5, DEEP, 12),
    # NX = 32 (n = 18, 31 padded, 32 exact)
    (18, 64, 1, 17, H17, 13),
    (31, 64, 2, 3, DEEP, 14),
    (32, 64, 3, 8, H100, 15),
    (32, 64, 12, 1, HODD, 16),
    (20, 64, 2, 4, H1, 17),
    # first generation, F = 64, 32 < n, n + F <= 256 (n = 192: n + F = 256 exactly)
    (33, 64, 5, 6, HODD, 18),
    (192, 64, 4, 9, DEEP, 19),
    (40, 64, 1, 3, H1, 20),
    (100, 64, 2, 8, H100, 21),
    (57, 64, 3, 1, H17, 22),
    # generic F (4 F not 256): strided gate columns, the "single" weight-gradient route
    (3, 1, 4, 5, HODD, 23),
    (5, 7, 2, 9, H1, 424),
    (2, 63, 3, 4, DEEP, 25),
    (6, 65, 1, 8, H100, 126),
    (4, 100, 5, 3, H17, 27),
    (9, 127, 2, 7, HODD, 28),
    (156, 100, 3, 6, DEEP, 29),            # n + F = 256: still the plain form
    (1, 65, 35, 2, H1, 130),
    # wide input, n + F > 256: x Wx and dx as GEMMs around the LSTM kernels
    (193, 64, 3, 5, DEEP, 31),             # n + F = 257 at F = 64
    (157, 100, 2, 8, HODD, 32),            # n + F = 257 at F = 100
    (250, 7, 1, 3, H1, 133),
    (200, 127, 4, 9, H100, 34),
    (300, 64, 2, 1, H17, 35),
]


def case_id(c):
    n, F, T, Bc, head, seed = c
    return f"{critic_route(n, F)[0]}-n{n}-F{F}-T1_{T + 1}-Bc{Bc}-h{'x'.join(map(str, head))}"


def head_widths(head):
    return set(head)


# ------------------------------------------------------------------------------------------------------------------
# coverage: the cells the table must reach (tests/test_critic_cases.py fails if one is missing)
# ------------------------------------------------------------------------------------------------------------------
GEN2_N = (1, 3, 4, 6, 8, 9, 16, 17, 18, 31, 32)
GEN2_BC = (1, 3, 4, 5, HEAD_ROWS - 1, HEAD_ROWS, HEAD_ROWS + 1, 2 * HEAD_ROWS, 2 * HEAD_ROWS + 1)
GENERIC_F = (1, 7, 63, 65, 100, 127)
HEAD_W = (1, 17, 65, 100, 129, 193, 255)
ROUTES = ("gen2", "gen1", "generic", "wide")


def required_cells():
    cells = [("gen2 n", n) for n in GEN2_N]
    cells += [("gen1 n", 33), ("gen1 n", 192), ("wide F=64 n", 193), ("wide n+F=257 F!=64",),
              ("generic n+F=256",)]
    cells += [("generic small n F", F) for F in GENERIC_F]
    cells += [("gen2 T1", nx, t1) for nx in NXS for t1 in (2, 3, 4)] + [("gen2 T1>=33",)]
    cells += [("gen2 Bc", b) for b in GEN2_BC]
    cells += [("gen2 NG", nx, g) for nx in NXS for g in (1, 2)]
    cells += [("gen2 NG=2 second group", kind) for kind in ("ragged", "empty", "full")]
    cells += [("head width", r, w) for r in ROUTES for w in HEAD_W]
    cells += [("head depth 8", r) for r in ROUTES]
    return cells


def cells_of(case):
    """The required cells one case reaches."""
    n, F, T, Bc, head, _ = case
    T1 = T + 1
    route = critic_route(n, F)
    r = route[0]
    out = set()
    if r == "gen2":
        nx = route[1]
        out.add(("gen2 n", n))
        out.add(("gen2 T1", nx, T1))
        if T1 >= 33:
            out.add(("gen2 T1>=33",))
        out.add(("gen2 Bc", Bc))
        out.add(("gen2 NG", nx, bwd2_groups(Bc)))
        if bwd2_groups(Bc) == 2:
            left = Bc % 8     # sequences in the last workgroup (8 per workgroup), 0 = full
            out.add(("gen2 NG=2 second group", "full" if left == 0 else "empty" if left <= 4 else "ragged"))
    elif r == "gen1":
        out.add(("gen1 n", n))
    elif r == "wide":
        if F == 64:
            out.add(("wide F=64 n", n))
        elif n + F == THREADS + 1:
            out.add(("wide n+F=257 F!=64",))
    else:
        if n + F == THREADS:
            out.add(("generic n+F=256",))
        if n <= 32:
            out.add(("generic small n F", F))
    for w in head_widths(head):
        out.add(("head width", r, w))
    if len(head) + 1 == MAX_LAYERS:
        out.add(("head depth 8", r))
    return out


def missing_cells(cases):
    have = set()
    for c in cases:
        have |= cells_of(c)
    return [c for c in required_cells() if c not in have]


# ------------------------------------------------------------------------------------------------------------------
# inputs of one case
# ------------------------------------------------------------------------------------------------------------------
def make_case(case):
    """(pb, xseq, label, xs): a problem with the case's critic (tiny dynamics / cost MLPs, m = 1), Bc sequences with
    mixed labels for critic_loss_grad and another Bc sequences for critic_score_vjp.  Inputs are standard normal: with
    lecun-normal weights the score stays O(1), far from where sigmoid saturates in fp32."""
    n, F, T, Bc, head, seed = case
    pb = orc.make_problem(n, 1, T, (Bc + 1) // 2, seed=seed, dtype=np.float32, dyn_hidden=(8,), cost_hidden=(8,),
                          cost_fout=2, lstm_features=F, head_hidden=head, bias_scale=0.1)
    rng = np.random.default_rng(1000 + seed)
    xseq = rng.standard_normal((Bc, T + 1, n)).astype(np.float32)
    label = np.where(rng.permutation(Bc) % 2 == 0, 1.0, -1.0).astype(np.float32)
    xs = rng.standard_normal((Bc, T + 1, n)).astype(np.float32)
    return pb, xseq, label, xs


SCORE_MAX = 8.0      # |score| bound: sigmoid(8) = 1 - 3e-4, far from fp32 saturation
KINK = 3e-6          # gpu_util.near_kink's default threshold


def head_live_fraction(cr64, x64):
    """The smallest fraction, over the head's hidden layers, of rows with at least one open relu: where it is 0 no
    gradient reaches the LSTM and its blocks would be compared as zeros."""
    _, (_, hT, _) = orc.critic_forward(cr64, x64, keep=True)
    _, zs = orc.mlp_forward(cr64["head"], hT)
    return min(float((z > 0).any(axis=1).mean()) for z in zs)


def head_kinks(cr64, x64, thresh=KINK):
    """(Bc,) bool: gpu_util.near_kink on the head of the fp64 forward, at the final LSTM state."""
    _, (_, hT, _) = orc.critic_forward(cr64, x64, keep=True)
    return gu.near_kink(cr64["head"], hT, thresh)


def _outputs(cr, x, label, xs, n, F, head):
    _, g = orc.critic_loss_and_grad(cr, x, label)
    blocks = gu.split_critic_flat(gu.pack_grads_critic(g), n, F, (F,) + tuple(head) + (1,))
    dx = orc.generator_loss_grad_x(cr, xs)
    return blocks + [("dx", dx), ("dx t=0", dx[:, 0]), ("dx t=T1-1", dx[:, -1])]


def sensitivity(case, trials=8, rel=2.0 ** -23):
    """{block: elementwise change of the fp64 result when every parameter and input is perturbed by one fp32 ulp
    (relative Gaussian, largest over `trials` draws)}.  A correct fp32 computation is the exact one at inputs
    perturbed about this much, so an entry that moves by s here may differ by a few s in any fp32 implementation:
    small entries of the weight gradients are sums over sequences (mixed labels) and products of activations near, but
    not at, a relu kink, and move by 1e-3 .. 1e-2 of themselves.  Blocks: the gradient blocks of split_critic_flat,
    then dx, dx at t = 0 and at t = T1 - 1."""
    n, F, T, Bc, head, seed = case
    pb, x, label, xs = make_case(case)
    cr = orc.cast_problem(pb, np.float64)["critic"]
    x, xs, label = x.astype(np.float64), xs.astype(np.float64), label.astype(np.float64)
    ref = _outputs(cr, x, label, xs, n, F, head)
    rng = np.random.default_rng(seed)

    def pert(a):
        return a * (1 + rel * rng.standard_normal(a.shape))
    worst = {name: 0.0 for name, _ in ref}
    for _ in range(trials):
        cp = dict(Wx=pert(cr["Wx"]), Wh=pert(cr["Wh"]), b=pert(cr["b"]),
                  head=[(pert(W), pert(b)) for W, b in cr["head"]])
        for (name, a), (_, r) in zip(_outputs(cp, pert(x), label, pert(xs), n, F, head), ref):
            worst[name] = max(worst[name], gu.el_err(a, r)[0])
    return worst
