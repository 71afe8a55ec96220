"""Records tests/golden/rollout_handover/*.npz for tests/test_gpu_rollout_handover.py: the outputs of the
register-weight rollout and of the backward pass after it, on a GPU, from the library that GMPC_LIB names (the build
of the commit BEFORE the change under test; with GMPC_LIB unset, the tree's own).

    GMPC_LIB=/path/to/parent/libgan_mpc_amd.so python tests/golden/make_rollout_handover.py [OUT_DIR]
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_gpu_rollout_handover as th  # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else th.GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    jobs = [(name, name, False) for name in th.CASES] + [(th.NAN_CASE + "-nan", th.NAN_CASE, True)]
    for tag, name, nan in jobs:
        got = th.run_case(name, nan)
        np.savez_compressed(os.path.join(out_dir, tag + ".npz"), seed=np.int64(th.SEED), **got)
        print(tag, {k: v.shape for k, v in got.items()}, flush=True)


if __name__ == "__main__":
    main()
