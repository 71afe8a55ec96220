"""k_linearize_sparse against GMPC_LIN=dense (bitwise) at shapes and batch sizes the sweep of
test_gpu_linearize_sparse.py does not reach.

Shapes inside the form's limits (200-wide hidden layers, n + m <= 32): n < 16 (no rows for the dense row window), n = 16
exactly, n + m = 32, n = 20 (four rows in the window), two and four hidden layers.  Batch sizes: fewer samples than
one workgroup has waves (most of the persistent grid idle), and more samples than the grid has waves (several samples
per wave, so every wave reuses its LDS lists and S tile)."""
import pytest

import gpu_util as gu
from test_gpu_linearize_sparse import _check_backward

# name: (n, m, T, B, dyn_hidden)
LAYOUT_SHAPES = {
    "n5-m3": (5, 3, 4, 6, (200, 200, 200)),
    "n16-m6": (16, 6, 4, 6, (200, 200, 200)),
    "n16-m16": (16, 16, 3, 5, (200, 200, 200)),
    "n20-m12": (20, 12, 3, 5, (200, 200, 200)),
    "n20-m6": (20, 6, 4, 6, (200, 200, 200)),
    "n17-m6-two-hidden": (17, 6, 4, 6, (200, 200)),
    "n9-m4-four-hidden": (9, 4, 4, 6, (200, 200, 200, 200)),
    # batch: 3 samples (one partly filled workgroup of a 512-workgroup grid) ...
    "n17-m6-three-samples": (17, 6, 1, 3, (200, 200, 200)),
    # ... and 4107 and 4150 samples: two or three per wave of the full persistent grid (2048 waves)
    "n17-m6-many-samples": (17, 6, 37, 111, (200, 200, 200)),
    "n12-m6-many-samples": (12, 6, 50, 83, (200, 200, 200)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYOUT_SHAPES))
def test_layout_shapes(name, monkeypatch):
    n, m, T, B, hidden = LAYOUT_SHAPES[name]
    pb = gu.problem(n, m, T, B, seed=23, dyn_hidden=hidden)
    eng = gu.engine_for(pb, critic=False)
    _check_backward(eng, pb, monkeypatch)
