"""The cases of the one-step disagreement's tests (tests/test_disagreement_host.py, tests/test_gpu_disagreement.py;
gmpc_set_sampled_disagreement; TEST INFRASTRUCTURE): sampled_ensemble_cases' shapes, problems,
members (three around the nominal network) and solver keywords, and per case a penalty, a power of two so that penalty
* D is exact.

The penalties were sized as std_s(J) / std_s(mean_p D) of the fp64 reference at iteration 0, rounded to a power of two
(w256's is not sized: it is used in the bitwise and parity groups only).  test_h3 of the host suite prints and pins what
they give: penalty * mean_p D / J, the range of D, and the number of problems of DECIDED whose iteration-0 elite set
the penalty changes."""

import sampled_ensemble_cases as ec

CASES = ec.CASES
NAMES = ec.NAMES
DECIDED = ec.DECIDED
LO, HI = ec.LO, ec.HI
MEMBERS = ec.MEMBERS
SOLVERS = ec.SOLVERS
PRECISIONS = ec.PRECISIONS
BITWISE = ec.BITWISE
NUM_KEEP = ec.NUM_KEEP
problem = ec.problem
members = ec.members
flat = ec.flat
nominal_flat = ec.nominal_flat
engine_kwargs = ec.engine_kwargs
init_std = ec.init_std

PENALTY = dict(base=128.0, m1=256.0, cheetah=64.0, wide_m=256.0, wide_n=64.0, ragged=32.0, w256=64.0)
# the decided protocol (H4, D6): problems of DECIDED that must stay decided through the third iteration
DECIDED_MIN = dict(mean=20, max=23)
