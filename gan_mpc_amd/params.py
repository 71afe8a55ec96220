"""Flax-style parameter pytrees <-> the flat fp32 vectors of the C ABI.

The reference keeps parameters as ``{"params": {"Dense_k": {"kernel": (in,out), "bias": (out,)}}}``
trees (flax ``Dense`` auto-naming, reference cost/nn.py:23-29, dynamics/nn.py:27-34) and the critic's
scanned ``OptimizedLSTMCell`` with kernels ``ii,if,ig,io`` (no bias) and ``hi,hf,hg,ho`` (+bias)
(reference critic/nn.py:28-42; names as in flax 0.7.2).  The C ABI wants one flat
vector per model: kernel (in,out) row-major then bias, layer after layer; the critic as
Wx[n][4F] | Wh[F][4F] | b[4F] with gate order i,f,g,o, then the head's Dense layers.
"""

import numpy as np

GATES = ("i", "f", "g", "o")
LSTM_SCOPE = "ScanOptimizedLSTMCell_0"


def mlp_dims(tree):
    p = tree["params"]
    dims = []
    for k in range(len(p)):
        kern = np.asarray(p[f"Dense_{k}"]["kernel"])
        if k == 0:
            dims.append(kern.shape[0])
        dims.append(kern.shape[1])
    return dims


def pack_mlp(tree):
    p = tree["params"]
    out = []
    for k in range(len(p)):
        d = p[f"Dense_{k}"]
        out.append(np.asarray(d["kernel"], np.float32).reshape(-1))
        out.append(np.asarray(d["bias"], np.float32).reshape(-1))
    return np.concatenate(out)


def unpack_mlp(flat, dims):
    flat = np.asarray(flat, np.float32)
    p, off = {}, 0
    for k, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        kern = flat[off:off + a * b].reshape(a, b).copy()
        off += a * b
        bias = flat[off:off + b].copy()
        off += b
        p[f"Dense_{k}"] = {"kernel": kern, "bias": bias}
    assert off == flat.size, (off, flat.size)
    return {"params": p}


# ---- dynamics: MLP variant (Dense stack) or LSTM variant (dynamics/nn.py:37-57: an OptimizedLSTMCell on
# [x, u] in front of the Dense stack).  Flat layout of the LSTM variant (include/gan_mpc_amd.h):
# Wx[(nx+m)][4F] | Wh[F][4F] | b[4F] (gates i,f,g,o) | the tail's Dense layers.
DYN_LSTM_SCOPE = "OptimizedLSTMCell_0"


def dynamics_is_lstm(tree):
    return any("LSTM" in k for k in tree["params"])


def dynamics_meta(tree):
    """(dyn_dims, lstm_features): the MLP's dims [n+m, ..., n] and 0, or the tail's dims [F, ..., nx] and F."""
    if not dynamics_is_lstm(tree):
        return mlp_dims(tree), 0
    p = tree["params"]
    tail = {"params": {k: v for k, v in p.items() if k.startswith("Dense_")}}
    return mlp_dims(tail), int(np.asarray(p[_lstm_scope(p)]["hi"]["kernel"]).shape[0])


def pack_dynamics(tree):
    if not dynamics_is_lstm(tree):
        return pack_mlp(tree)
    p = tree["params"]
    cell = p[_lstm_scope(p)]
    Wx = np.concatenate([np.asarray(cell["i" + g]["kernel"], np.float32) for g in GATES], axis=1)
    Wh = np.concatenate([np.asarray(cell["h" + g]["kernel"], np.float32) for g in GATES], axis=1)
    b = np.concatenate([np.asarray(cell["h" + g]["bias"], np.float32) for g in GATES])
    tail = {"params": {k: v for k, v in p.items() if k.startswith("Dense_")}}
    return np.concatenate([Wx.reshape(-1), Wh.reshape(-1), b, pack_mlp(tail)])


def unpack_dynamics(flat, dims, F, m=None, scope=DYN_LSTM_SCOPE):
    """Inverse of pack_dynamics: dims / F as returned by dynamics_meta; m (controls) is needed for the LSTM
    variant (the cell's input is [x, u])."""
    if not F:
        return unpack_mlp(flat, dims)
    flat = np.asarray(flat, np.float32)
    nx = dims[-1]
    kin = nx + int(m)
    o1 = kin * 4 * F
    o2 = o1 + F * 4 * F
    Wx, Wh, b = flat[:o1].reshape(kin, 4 * F), flat[o1:o2].reshape(F, 4 * F), flat[o2:o2 + 4 * F]
    cell = {}
    for gi, g in enumerate(GATES):
        cell["i" + g] = {"kernel": Wx[:, gi * F:(gi + 1) * F].copy()}
        cell["h" + g] = {"kernel": Wh[:, gi * F:(gi + 1) * F].copy(), "bias": b[gi * F:(gi + 1) * F].copy()}
    p = {scope: cell}
    p.update(unpack_mlp(flat[o2 + 4 * F:], dims)["params"])
    return {"params": p}


def lstm_dynamics_dict_to_tree(dl, scope=DYN_LSTM_SCOPE):
    """dict(Wx, Wh, b, tail) (the oracle's form) -> flax tree."""
    F = dl["Wh"].shape[0]
    cell = {}
    for gi, g in enumerate(GATES):
        cell["i" + g] = {"kernel": np.asarray(dl["Wx"][:, gi * F:(gi + 1) * F])}
        cell["h" + g] = {"kernel": np.asarray(dl["Wh"][:, gi * F:(gi + 1) * F]),
                         "bias": np.asarray(dl["b"][gi * F:(gi + 1) * F])}
    p = {scope: cell}
    p.update(layers_to_tree(dl["tail"])["params"])
    return {"params": p}


def lstm_dynamics_tree_to_dict(tree):
    p = tree["params"]
    cell = p[_lstm_scope(p)]
    tail = {"params": {k: v for k, v in p.items() if k.startswith("Dense_")}}
    return dict(Wx=np.concatenate([np.asarray(cell["i" + g]["kernel"]) for g in GATES], axis=1),
                Wh=np.concatenate([np.asarray(cell["h" + g]["kernel"]) for g in GATES], axis=1),
                b=np.concatenate([np.asarray(cell["h" + g]["bias"]) for g in GATES]),
                tail=tree_to_layers(tail))


def layers_to_tree(layers):
    """[(W, b), ...] -> flax tree."""
    return {"params": {f"Dense_{k}": {"kernel": np.asarray(W), "bias": np.asarray(b)}
                       for k, (W, b) in enumerate(layers)}}


def tree_to_layers(tree):
    p = tree["params"]
    return [(np.asarray(p[f"Dense_{k}"]["kernel"]), np.asarray(p[f"Dense_{k}"]["bias"]))
            for k in range(len(p))]


def _lstm_scope(p):
    for k in p:
        if "LSTM" in k:
            return k
    raise KeyError("no LSTM cell scope in critic params")


def pack_critic(tree):
    p = tree["params"]
    cell = p[_lstm_scope(p)]
    Wx = np.concatenate([np.asarray(cell["i" + g]["kernel"], np.float32) for g in GATES], axis=1)
    Wh = np.concatenate([np.asarray(cell["h" + g]["kernel"], np.float32) for g in GATES], axis=1)
    b = np.concatenate([np.asarray(cell["h" + g]["bias"], np.float32) for g in GATES])
    out = [Wx.reshape(-1), Wh.reshape(-1), b]
    k = 0
    while f"Dense_{k}" in p:
        out.append(np.asarray(p[f"Dense_{k}"]["kernel"], np.float32).reshape(-1))
        out.append(np.asarray(p[f"Dense_{k}"]["bias"], np.float32).reshape(-1))
        k += 1
    return np.concatenate(out)


def critic_dims(tree):
    p = tree["params"]
    cell = p[_lstm_scope(p)]
    n, F = np.asarray(cell["ii"]["kernel"]).shape
    head = [F]
    k = 0
    while f"Dense_{k}" in p:
        head.append(np.asarray(p[f"Dense_{k}"]["kernel"]).shape[1])
        k += 1
    return n, F, head


def unpack_critic(flat, n, F, head_dims, scope=LSTM_SCOPE):
    flat = np.asarray(flat, np.float32)
    off = 0
    Wx = flat[off:off + n * 4 * F].reshape(n, 4 * F)
    off += n * 4 * F
    Wh = flat[off:off + F * 4 * F].reshape(F, 4 * F)
    off += F * 4 * F
    b = flat[off:off + 4 * F]
    off += 4 * F
    cell = {}
    for gi, g in enumerate(GATES):
        cell["i" + g] = {"kernel": Wx[:, gi * F:(gi + 1) * F].copy()}
        cell["h" + g] = {"kernel": Wh[:, gi * F:(gi + 1) * F].copy(),
                         "bias": b[gi * F:(gi + 1) * F].copy()}
    p = {scope: cell}
    for k, (a, c) in enumerate(zip(head_dims[:-1], head_dims[1:])):
        kern = flat[off:off + a * c].reshape(a, c).copy()
        off += a * c
        bias = flat[off:off + c].copy()
        off += c
        p[f"Dense_{k}"] = {"kernel": kern, "bias": bias}
    assert off == flat.size, (off, flat.size)
    return {"params": p}


def critic_dict_to_tree(cr, scope=LSTM_SCOPE):
    """dict(Wx, Wh, b, head) (plain arrays: Wx, Wh, b, head) -> flax tree."""
    F = cr["Wh"].shape[0]
    cell = {}
    for gi, g in enumerate(GATES):
        cell["i" + g] = {"kernel": np.asarray(cr["Wx"][:, gi * F:(gi + 1) * F])}
        cell["h" + g] = {"kernel": np.asarray(cr["Wh"][:, gi * F:(gi + 1) * F]),
                         "bias": np.asarray(cr["b"][gi * F:(gi + 1) * F])}
    p = {scope: cell}
    for k, (W, b) in enumerate(cr["head"]):
        p[f"Dense_{k}"] = {"kernel": np.asarray(W), "bias": np.asarray(b)}
    return {"params": p}


def critic_tree_to_dict(tree):
    p = tree["params"]
    cell = p[_lstm_scope(p)]
    Wx = np.concatenate([np.asarray(cell["i" + g]["kernel"]) for g in GATES], axis=1)
    Wh = np.concatenate([np.asarray(cell["h" + g]["kernel"]) for g in GATES], axis=1)
    b = np.concatenate([np.asarray(cell["h" + g]["bias"]) for g in GATES])
    head = []
    k = 0
    while f"Dense_{k}" in p:
        head.append((np.asarray(p[f"Dense_{k}"]["kernel"]), np.asarray(p[f"Dense_{k}"]["bias"])))
        k += 1
    return dict(Wx=Wx, Wh=Wh, b=b, head=head)


# ---- expert sequence model (reference expert/nn.py) ----------------------------------------------
# Tree layout written by this package (and read back tolerantly from a flax checkpoint):
#   {"params": {"model": {<cell scope>: {"OptimizedLSTMCell_0": {ii..ho}        (LSTM variant)
#                                        | "Dense_0": {kernel, bias}            (MLP variant)
#                                        "MLPCell_0": {"Dense_k": ...}          state head
#                                        "MLPCell_1": {"Dense_k": ...}}}}}      action head
# The flax auto-names of nn.scan'd cells are recalled, not verified offline, so the
# reader looks the pieces up by structure: the sub-dict holding ii/if/ig/io, and the two MLPCell
# scopes in name order.
EXPERT_CELL_SCOPE = "ScanLSTMCell_0"


def _dense_stack(p):
    out, k = [], 0
    while f"Dense_{k}" in p:
        out.append((np.asarray(p[f"Dense_{k}"]["kernel"], np.float32),
                    np.asarray(p[f"Dense_{k}"]["bias"], np.float32)))
        k += 1
    return out


def _find_scope(tree, pred):
    if isinstance(tree, dict):
        if pred(tree):
            return tree
        for v in tree.values():
            r = _find_scope(v, pred)
            if r is not None:
                return r
    return None


def expert_tree_to_dict(tree):
    cell = _find_scope(tree, lambda d: any(k.startswith("MLPCell") for k in d))
    if cell is None:
        raise KeyError("no MLPCell scopes in expert params")
    heads = sorted(k for k in cell if k.startswith("MLPCell"))
    ex = {"head_x": _dense_stack(cell[heads[0]]), "head_u": _dense_stack(cell[heads[1]])}
    lstm = _find_scope(cell, lambda d: "ii" in d and "hi" in d)
    if lstm is not None:
        ex["lstm"] = dict(
            Wx=np.concatenate([np.asarray(lstm["i" + g]["kernel"], np.float32) for g in GATES], axis=1),
            Wh=np.concatenate([np.asarray(lstm["h" + g]["kernel"], np.float32) for g in GATES], axis=1),
            b=np.concatenate([np.asarray(lstm["h" + g]["bias"], np.float32) for g in GATES]))
    else:
        ex["first"] = _dense_stack(cell)[0]
    return ex


def expert_dict_to_tree(ex, scope=EXPERT_CELL_SCOPE):
    cell = {}
    if "lstm" in ex:
        F = ex["lstm"]["Wh"].shape[0]
        lc = {}
        for gi, g in enumerate(GATES):
            lc["i" + g] = {"kernel": np.asarray(ex["lstm"]["Wx"][:, gi * F:(gi + 1) * F])}
            lc["h" + g] = {"kernel": np.asarray(ex["lstm"]["Wh"][:, gi * F:(gi + 1) * F]),
                           "bias": np.asarray(ex["lstm"]["b"][gi * F:(gi + 1) * F])}
        cell["OptimizedLSTMCell_0"] = lc
    else:
        cell["Dense_0"] = {"kernel": np.asarray(ex["first"][0]), "bias": np.asarray(ex["first"][1])}
    for name, key in (("MLPCell_0", "head_x"), ("MLPCell_1", "head_u")):
        cell[name] = {f"Dense_{k}": {"kernel": np.asarray(W), "bias": np.asarray(b)}
                      for k, (W, b) in enumerate(ex[key])}
    return {"params": {"model": {scope: cell}}}


def pack_expert(ex):
    """plain dict of arrays (or a tree) -> (flat fp32 vector, lstm_features, head_dims_x, head_dims_u) in
    the layout of gmpc_expert_rollout."""
    if "params" in ex:
        ex = expert_tree_to_dict(ex)
    parts = []
    if "lstm" in ex:
        F = ex["lstm"]["Wh"].shape[0]
        parts += [ex["lstm"]["Wx"], ex["lstm"]["Wh"], ex["lstm"]["b"]]
    else:
        F = 0
        parts += [ex["first"][0], ex["first"][1]]
    for key in ("head_x", "head_u"):
        for W, b in ex[key]:
            parts += [W, b]
    flat = np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts])
    dims = lambda layers: [layers[0][0].shape[0]] + [W.shape[1] for W, _ in layers]
    return flat, F, dims(ex["head_x"]), dims(ex["head_u"])


def unpack_expert(flat, lstm_features, head_dims_x, head_dims_u):
    """Inverse of pack_expert: flat vector -> plain dict (lstm | first, head_x, head_u) of fp32 arrays."""
    flat = np.asarray(flat, np.float32).reshape(-1)
    off = [0]

    def take(*shape):
        size = int(np.prod(shape))
        out = flat[off[0]:off[0] + size].reshape(shape).copy()
        off[0] += size
        return out

    n, F, Y = head_dims_x[-1], int(lstm_features), head_dims_x[0]
    ex = {}
    if F > 0:
        ex["lstm"] = dict(Wx=take(n, 4 * F), Wh=take(F, 4 * F), b=take(4 * F))
    else:
        ex["first"] = (take(n, Y), take(Y))
    for key, dims in (("head_x", head_dims_x), ("head_u", head_dims_u)):
        ex[key] = [(take(a, b), take(b)) for a, b in zip(dims[:-1], dims[1:])]
    if off[0] != flat.size:
        raise ValueError(f"expert vector of {flat.size} floats, layout needs {off[0]}")
    return ex
