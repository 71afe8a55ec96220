"""The cases of the ensemble modes' tests (tests/test_ensemble_modes_host.py, tests/test_gpu_ensemble_modes.py;
gmpc_set_sampled_ensemble_mode; TEST INFRASTRUCTURE): sampled_ensemble_cases' cases, its three
members per case and its engine_kwargs, under the mode settings below (dicts of Engine.set_sampled_ensemble_mode's
keywords).  Measured on the CPU with ensemble_modes_ref (test_h3 of the host test prints it): at iteration 0 the fp64
costs of these settings differ from the mean-mode cost by medians of 1.9e-3 (TS1 Q 4) to 6.9e-3 (MAX) relative and
change the elite set of 10 to 14 of the 24 problems, so a wrong rule or schedule cannot pass a 1e-6-level comparison."""

from sampled_ensemble_cases import *       # noqa: F401,F403  (CASES, NAMES, DECIDED, BITWISE, members, flat, ...)
from sampled_ensemble_cases import engine_kwargs, flat, init_std, members, nominal_flat, problem     # noqa: F401

MODES = {
    "std+1":    dict(aggregate="mean_std", risk=1.0),
    "std-0.5":  dict(aggregate="mean_std", risk=-0.5),
    "max":      dict(aggregate="max"),
    "ts1q4":    dict(propagation="ts1", particles=4),
    "ts1q1":    dict(propagation="ts1", particles=1),
    "ts1q4max": dict(aggregate="max", propagation="ts1", particles=4),
}
MODE_NAMES = list(MODES)
# the decided protocol's settings and what the CPU run of the host test measured, minus one (the mean-mode test's rule)
DECIDED_MODES = {"std+1": 20, "max": 20, "ts1q4": 23}
