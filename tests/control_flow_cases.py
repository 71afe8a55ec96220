"""The problems and option rows of the iLQR control-flow tests OFF the small-state MLP path, shared by
tests/test_gpu_control_flow_paths.py (gmpc_ilqr_solve on them against the fp64 oracle) and tests/test_ilqr_control_flow.py
(the oracle itself against the scalar torch restatement on two of them).  TEST INFRASTRUCTURE.

Every row was chosen on the CPU with the NumPy oracle: its members backtrack 7-12 halvings (the second and third
line-search rounds), stop at different iterations, and every trajectory's control flow is decided in the sense of
tests/test_gpu_control_flow.py (share 1.0).  The iteration counts are NOT recorded here: the tests compare with the
oracle they run and assert only the point of each row (a spread, a stop below maxiter, a member that never starts)."""

import gpu_util as gu

# name -> (n, m, T, B, network widths, the path gmpc_ilqr_solve has to take: step-major pipeline?, LSTM dynamics?)
PROBLEMS = {
    # n > 64, last hidden width >= n / 2: dense Jacobians, produced one step ahead on the side stream
    "dense": (70, 7, 6, 5, dict(dyn_hidden=(128, 96), cost_hidden=(64,), cost_fout=12), True, False),
    # n <= 64 with more than 32 controls: the step-major pipeline as well
    "m40": (24, 40, 5, 4, dict(dyn_hidden=(64, 48), cost_hidden=(32,), cost_fout=6), True, False),
    # last hidden width h < n / 2: the low-rank form A = I + W_L^T Vx^T
    "lowrank": (90, 4, 5, 4, dict(dyn_hidden=(30,), cost_hidden=(48,), cost_fout=6), True, False),
    # LSTM dynamics, state 4 + 2 x 6 = 16: the small-state kernels around k_dynl_traj / k_dynl_jac
    "dynl-small": (4, 2, 7, 6, dict(dyn_lstm=6, dyn_hidden=(12,), cost_hidden=(16,), cost_fout=4), False, True),
    # LSTM dynamics, state 17 + 2 x 32 = 81: the step-major pipeline around them
    "dynl-big": (17, 6, 8, 5, dict(dyn_lstm=32, dyn_hidden=(64, 64), cost_hidden=(64,), cost_fout=8), True, True),
}

# (problem, seed, options, NaN start, maxiter)
ROWS = [
    ("dense", 3, {"obj_step_threshold": 0.001}, False, 12),
    ("dense", 3, {"alpha_min": 0.01}, False, 12),
    ("dense", 7, {"inputs_step_threshold": 0.1}, False, 12),
    ("dense", 3, {}, True, 4),
    ("m40", 3, {"obj_step_threshold": 0.003}, False, 12),
    ("m40", 3, {"relative_grad_norm_threshold": 0.03}, False, 12),
    ("m40", 3, {"alpha_min": 0.01}, False, 12),
    ("lowrank", 3, {"obj_step_threshold": 0.001}, False, 12),
    ("lowrank", 3, {}, True, 4),
    ("dynl-small", 7, {"obj_step_threshold": 0.003}, False, 12),
    ("dynl-small", 7, {"relative_grad_norm_threshold": 0.03}, False, 12),
    ("dynl-small", 7, {}, True, 3),
    ("dynl-big", 3, {"obj_step_threshold": 0.0003}, False, 12),
    ("dynl-big", 7, {"alpha_min": 0.01}, False, 12),
    ("dynl-big", 3, {}, True, 4),
]


def row_id(row):
    name, seed, opts, nan, maxiter = row
    return f"{name}-s{seed}-" + ("nan-start" if nan else "/".join(f"{k}={v}" for k, v in opts.items()))


def problem(name, seed):
    """fp32 problem of a row (the fp64 side is orc.cast_problem of it: the same weights)"""
    n, m, T, B, kw, _, _ = PROBLEMS[name]
    return gu.problem(n, m, T, B, seed=seed, out_scale=0.6, **kw)


def start(pb, nan):
    """the controls a row starts from: pb["U"], for the NaN rows with one entry of trajectory 1 made NaN"""
    U = pb["U"].copy()
    if nan:
        U[1, 2, 0] = float("nan")
    return U
