"""CPU-side checks: the C-ABI library loads and exports every symbol include/gan_mpc_amd.h declares,
fails loudly without a GPU, and the flax-tree <-> flat packing round-trips."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gan_mpc_oracle as orc
from gan_mpc_amd import _lib, params as P
from gan_mpc_amd.engine import make_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgan_mpc_amd.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_header_symbols_are_exported_and_bound():
    lib = _lib_or_skip()
    hdr = open(os.path.join(ROOT, "include", "gan_mpc_amd.h")).read()
    declared = set(re.findall(r"\b(gmpc_[a-z_]+)\s*\(", hdr))
    assert len(declared) >= 14
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert set(_lib.SIGNATURES) == declared


def test_param_counts_match_survey():
    lib = _lib_or_skip()
    s = make_shape(17, 6, 50, [23, 200, 200, 200, 17], [17, 128, 128, 10], 64, [64, 1])
    # 88,617 dynamics / 20,106 cost / 21,057 critic parameters at C2
    assert [lib.gmpc_param_count(C.byref(s), i) for i in range(3)] == [88617, 20106, 21057]
    s = make_shape(17, 6, 50, [23, 200, 200, 200, 17], [17, 128, 128, 10], 64, [64, 256, 256, 256, 1])
    assert lib.gmpc_param_count(C.byref(s), 2) == 169473


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_gpu_fails_loudly():
    lib = _lib_or_skip()
    s = make_shape(3, 1, 5, [4, 8, 3], [3, 8, 2])
    ctx = C.c_void_p()
    rc = lib.gmpc_create(C.byref(s), 4, 0, C.byref(ctx))
    assert rc == -2 and b"no CPU fallback" in lib.gmpc_last_error()
    from gan_mpc_amd.engine import Engine
    with pytest.raises(_lib.GmpcError):
        Engine(3, 1, 5, [4, 8, 3], [3, 8, 2], max_batch=4)


def test_bad_shape_rejected_without_gpu_work():
    lib = _lib_or_skip()
    s = make_shape(1100, 17, 50, [1117, 200, 1100], [1100, 128, 10])
    ctx = C.c_void_p()
    assert lib.gmpc_create(C.byref(s), 4, 0, C.byref(ctx)) == -1
    assert b"unsupported shape" in lib.gmpc_last_error()


def test_mlp_pack_roundtrip():
    pb = orc.make_problem(5, 2, 4, 3, seed=1, dyn_hidden=(7, 9), cost_hidden=(6,), cost_fout=4,
                          bias_scale=0.5)
    tree = P.layers_to_tree(pb["dyn"])
    flat = P.pack_mlp(tree)
    assert flat.size == sum(W.size + b.size for W, b in pb["dyn"])
    assert P.mlp_dims(tree) == [7, 7, 9, 5]
    back = P.tree_to_layers(P.unpack_mlp(flat, P.mlp_dims(tree)))
    for (W, b), (W2, b2) in zip(pb["dyn"], back):
        np.testing.assert_array_equal(W, W2)
        np.testing.assert_array_equal(b, b2)
    # kernel (in,out) row-major then bias
    np.testing.assert_array_equal(flat[:49].reshape(7, 7), pb["dyn"][0][0])
    np.testing.assert_array_equal(flat[49:56], pb["dyn"][0][1])


def test_critic_pack_roundtrip_and_gate_order():
    pb = orc.make_problem(5, 2, 4, 3, seed=2, lstm_features=8, head_hidden=(6,), bias_scale=0.5)
    tree = P.critic_dict_to_tree(pb["critic"])
    cell = tree["params"][P.LSTM_SCOPE]
    assert set(cell) == {"ii", "if", "ig", "io", "hi", "hf", "hg", "ho"}
    assert "bias" not in cell["ii"] and "bias" in cell["hi"]
    flat = P.pack_critic(tree)
    n, F, head = P.critic_dims(tree)
    assert (n, F, head) == (5, 8, [8, 6, 1])
    back = P.critic_tree_to_dict(P.unpack_critic(flat, n, F, head))
    for k in ("Wx", "Wh", "b"):
        np.testing.assert_array_equal(back[k], pb["critic"][k])
    # forget-gate block sits second: columns F..2F of Wx
    np.testing.assert_array_equal(flat[: n * 4 * F].reshape(n, 4 * F)[:, F:2 * F],
                                  cell["if"]["kernel"])


def test_pack_layout_lets_a_caller_pack_a_flax_tree_without_the_python_packers():
    """gmpc_pack_layout (no device needed): scatter every flax leaf to flat[offset + r * ld + c] and get
    exactly the vectors gan_mpc_amd/params.py builds -- dynamics, cost, critic and the training vector."""
    _lib_or_skip()
    from gan_mpc_amd import utils
    from gan_mpc_amd.engine import pack_layout
    pb = orc.make_problem(5, 2, 4, 3, seed=4, lstm_features=64, dyn_hidden=(7, 9), cost_hidden=(6,),
                          cost_fout=4, head_hidden=(11,), bias_scale=0.5)
    trees = {"dynamics_params": P.layers_to_tree(pb["dyn"]), "cost_params": P.layers_to_tree(pb["cmlp"]),
             "critic_params": P.critic_dict_to_tree(pb["critic"]), "mpc_weights": pb["mpc_w"]}
    shape = make_shape(5, 2, 4, [7, 7, 9, 5], [5, 6, 4], 64, [64, 11, 1])

    def scatter(which, tree, size):
        leaves = utils.flatten_tree(tree)
        flat = np.full(size, np.nan, np.float32)
        layout = pack_layout(shape, which)
        assert {name for name, *_ in layout} == set(leaves)
        for name, off, rows, cols, ld in layout:
            leaf = np.asarray(leaves[name], np.float32).reshape(rows, cols)
            for r in range(rows):
                flat[off + r * ld: off + r * ld + cols] = leaf[r]
        assert not np.isnan(flat).any()      # the leaves tile the vector: no hole, nothing twice
        return flat

    want = {0: P.pack_mlp(trees["dynamics_params"]), 1: P.pack_mlp(trees["cost_params"]),
            2: P.pack_critic(trees["critic_params"])}
    for which, key in ((0, "dynamics_params"), (1, "cost_params"), (2, "critic_params")):
        np.testing.assert_array_equal(scatter(which, trees[key], want[which].size), want[which])
    full = np.concatenate([pb["mpc_w"], want[1], want[0], want[2]])
    np.testing.assert_array_equal(scatter(3, trees, full.size), full)
    lib = _lib.load()
    bad = make_shape(5, 2, 4, [7, 7, 9, 5], [5, 6, 4])
    assert lib.gmpc_pack_layout(C.byref(bad), 2, None, 0) == -1 and b"no critic" in lib.gmpc_last_error()


def test_single_evaluations_refuse_rows_they_would_read_past():
    """Engine.get_cost / Engine.predict check every argument is (B, width) before the kernel reads B rows of that
    width from it: a narrower goal row (an x_size-wide goal handed to a full-state engine), a wrong u width or fewer
    rows than x are errors, not reads past the end of the tensor.  The check runs before the library is called, so
    it is exercised here without a context."""
    from gan_mpc_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.n, eng.m, eng.nx = 20, 2, 4         # an LSTM-dynamics engine: xc = [x (4), c, h (8 + 8)]
    x, u, g = torch.zeros(5, 20), torch.zeros(5, 2), torch.zeros(5, 4)
    bad = [("get_cost", (torch.zeros(5, 4), u, g, False)),        # x of the goal's width
           ("get_cost", (x, u, torch.zeros(5, 20), False)),       # goal of the state's width
           ("get_cost", (x, torch.zeros(5, 3), g, False)),
           ("get_cost", (x, u, torch.zeros(4, 4), False)),        # fewer goal rows than x
           ("get_cost", (x, torch.zeros(4, 2), None, True)),
           ("get_cost", (x.reshape(-1), u, g, False)),
           ("predict", (x, torch.zeros(3, 2))),
           ("predict", (torch.zeros(5, 4), u))]
    for call, args in bad:
        with pytest.raises(_lib.GmpcError, match=f"{call}: .* must be"):
            getattr(eng, call)(*args)
