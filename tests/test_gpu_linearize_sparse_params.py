"""k_linearize_sparse reads packed copies of the hidden weights (LinPad::WSP) that gmpc_set_params rebuilds on every
call.  After a second set_params with other dynamics weights the sparse route must still return the dense chain's bits:
a packed copy left from the first weights would not."""
import numpy as np
import pytest

import gpu_util as gu
from gan_mpc_amd import params as P
from test_gpu_linearize_sparse import _check_backward


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 12])
def test_second_set_params(n, monkeypatch):
    pb = gu.problem(n, 6, 4, 6, seed=5)
    eng = gu.engine_for(pb, critic=False)
    AB1 = _check_backward(eng, pb, monkeypatch)
    # same inputs, other dynamics weights
    pb2 = dict(pb, dyn=gu.problem(n, 6, 4, 6, seed=6)["dyn"])
    eng.set_params(eng.to_dev(pb2["mpc_w"]), eng.to_dev(P.pack_dynamics(gu.dyn_tree(pb2["dyn"]))),
                   eng.to_dev(P.pack_mlp(P.layers_to_tree(pb2["cmlp"]))))
    AB2 = _check_backward(eng, pb2, monkeypatch)
    assert not np.array_equal(AB1, AB2)
