"""ctypes binding of libgan_mpc_amd.so (include/gan_mpc_amd.h).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C gan_mpc_amd/csrc``).  There is
no CPU fallback: if the shared object is missing, or no HIP device is visible when a context is
created, the caller gets an exception.
"""

import ctypes as C
import os

GMPC_MAX_LAYERS = 8
_HERE = os.path.dirname(os.path.abspath(__file__))
# GMPC_LIB: an alternative build of the same library (A/B timing of kernel variants); default: the in-tree one
LIB_PATH = os.environ.get("GMPC_LIB") or os.path.join(_HERE, "libgan_mpc_amd.so")


class GmpcError(RuntimeError):
    pass


class Shape(C.Structure):
    _fields_ = [
        ("n", C.c_int), ("m", C.c_int), ("T", C.c_int),
        ("dyn_layers", C.c_int), ("dyn_dims", C.c_int * (GMPC_MAX_LAYERS + 1)),
        ("cost_layers", C.c_int), ("cost_dims", C.c_int * (GMPC_MAX_LAYERS + 1)),
        ("lstm_features", C.c_int),
        ("head_layers", C.c_int), ("head_dims", C.c_int * (GMPC_MAX_LAYERS + 1)),
        ("dyn_lstm_features", C.c_int), ("x_size", C.c_int),
    ]


class IlqrOpts(C.Structure):
    _fields_ = [
        ("maxiter", C.c_int),
        ("grad_norm_threshold", C.c_float),
        ("relative_grad_norm_threshold", C.c_float),
        ("obj_step_threshold", C.c_float),
        ("inputs_step_threshold", C.c_float),
        ("make_psd", C.c_int),
        ("psd_delta", C.c_float),
        ("alpha_0", C.c_float),
        ("alpha_min", C.c_float),
    ]


class ExpertShape(C.Structure):
    _fields_ = [
        ("lstm_features", C.c_int), ("head_layers", C.c_int),
        ("head_dims_x", C.c_int * (GMPC_MAX_LAYERS + 1)),
        ("head_dims_u", C.c_int * (GMPC_MAX_LAYERS + 1)),
    ]


class Leaf(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("offset", C.c_long), ("rows", C.c_int), ("cols", C.c_int),
                ("ld", C.c_int)]


class CemOpts(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int), ("num_samples", C.c_int), ("num_elites", C.c_int), ("iter_offset", C.c_int),
        ("sampling_smoothing", C.c_float), ("evolution_smoothing", C.c_float),
        ("seed", C.c_ulonglong),
    ]


class MppiOpts(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int), ("num_samples", C.c_int), ("iter_offset", C.c_int),
        ("sampling_smoothing", C.c_float), ("evolution_smoothing", C.c_float), ("temperature", C.c_float),
        ("seed", C.c_ulonglong),
    ]


class IcemOpts(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int), ("num_samples", C.c_int), ("num_elites", C.c_int), ("num_keep", C.c_int),
        ("carry_in", C.c_int), ("iter_offset", C.c_int), ("add_mean", C.c_int), ("return_best", C.c_int),
        ("noise_beta", C.c_float), ("evolution_smoothing", C.c_float), ("decay", C.c_float),
        ("seed", C.c_ulonglong),
    ]


class EnsembleMode(C.Structure):
    """gmpc_ensemble_mode: how a set dynamics ensemble is propagated and aggregated."""
    _fields_ = [("aggregate", C.c_int), ("risk", C.c_float), ("propagation", C.c_int), ("particles", C.c_int)]


_P = C.c_void_p


class BgemmDesc(C.Structure):
    """gmpc_bgemm_desc: every argument of the batched TN GEMM family (gmpc_bgemm_tn_ex / gmpc_bgemm_route)."""
    _fields_ = [
        ("batch", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("X", _P), ("sx", C.c_long), ("ldx", C.c_int),
        ("Y", _P), ("sy", C.c_long), ("ldy", C.c_int),
        ("C", _P), ("sc", C.c_long), ("ldc", C.c_int),
        ("alpha", C.c_float), ("beta", C.c_float),
        ("active", _P),
        ("X2", _P), ("sx2", C.c_long), ("ldx2", C.c_int),
        ("Y2", _P), ("sy2", C.c_long), ("ldy2", C.c_int),
        ("K2", C.c_int),
        ("X3", _P), ("sx3", C.c_long), ("ldx3", C.c_int),
        ("Y3", _P), ("sy3", C.c_long), ("ldy3", C.c_int),
        ("K3", C.c_int),
        ("upper_only", C.c_int),
        ("E", _P), ("se", C.c_long), ("lde", C.c_int), ("En", C.c_int),
        ("rowmask", _P), ("srm", C.c_long),
    ]


class WgradDesc(C.Structure):
    """gmpc_wgrad_desc: one weight-gradient problem and its partial-sum buffer (gmpc_wgrad_ex / gmpc_wgrad_route)."""
    _fields_ = [
        ("rows", C.c_int), ("M", C.c_int), ("N", C.c_int), ("lda", C.c_int), ("ldb", C.c_int), ("cs_rows", C.c_int),
        ("A", _P), ("B", _P), ("C", _P), ("colsum", _P),
        ("mfma_ok", C.c_int), ("form", C.c_int),
        ("part", _P), ("part_floats", C.c_long),
    ]


# name -> (restype, argtypes); exactly the entry points declared in include/gan_mpc_amd.h
SIGNATURES = {
    "gmpc_last_error": (C.c_char_p, []),
    "gmpc_version": (C.c_char_p, []),
    "gmpc_param_count": (C.c_long, [C.POINTER(Shape), C.c_int]),
    "gmpc_pack_layout": (C.c_int, [C.POINTER(Shape), C.c_int, C.POINTER(Leaf), C.c_int]),
    "gmpc_get_cost": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P, _P]),
    "gmpc_predict": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "gmpc_comm_unique_id": (C.c_int, [C.c_char_p]),
    "gmpc_comm_init": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p]),
    "gmpc_comm_world": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gmpc_allreduce_grads": (C.c_int, [_P, _P, C.c_long, _P]),
    "gmpc_create": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_int, C.POINTER(_P)]),
    "gmpc_destroy": (C.c_int, [_P]),
    "gmpc_set_params": (C.c_int, [_P, _P, _P, _P, _P]),
    "gmpc_rollout_cost": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "gmpc_lqr_backward": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_lqr_backward_after_rollout": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_ilqr_solve": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(IlqrOpts), _P, _P, _P, _P, _P,
                                  _P, _P]),
    "gmpc_ilqr_solve_fused": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(IlqrOpts), _P, _P, _P, _P, _P,
                                        _P, _P]),
    "gmpc_ilqr_solve_box": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(IlqrOpts), _P, _P, _P, _P, _P,
                                      _P, _P, _P, _P]),
    "gmpc_ilqr_solve_box_held": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(IlqrOpts), _P, _P, _P, _P, _P,
                                           _P, _P, _P, _P]),
    "gmpc_cem_solve": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(CemOpts), _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_mppi_solve": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(MppiOpts), _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                  _P]),
    "gmpc_mppi_vjp": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(MppiOpts), _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                _P, _P, _P, _P, _P]),
    "gmpc_icem_solve": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(IcemOpts), _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                  _P, _P, _P]),
    "gmpc_icem_plan_host": (C.c_int, [C.POINTER(IcemOpts), C.c_int, _P, _P]),
    "gmpc_set_sampled_precision": (C.c_int, [_P, C.c_int]),
    "gmpc_set_sampled_ensemble": (C.c_int, [_P, C.c_int, _P]),
    "gmpc_set_sampled_ensemble_mode": (C.c_int, [_P, C.POINTER(EnsembleMode)]),
    "gmpc_ensemble_rollout": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_ensemble_rollout_feedback": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_float, _P,
                                                 _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_set_sampled_disagreement": (C.c_int, [_P, C.c_int, C.c_float]),
    "gmpc_ensemble_disagreement": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_ensemble_rollout_vjp": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_ensemble_disagreement_vjp": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_box_qp_host":(C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_bilevel_grad": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_float, _P, _P, _P]),
    "gmpc_bilevel_grad_cotangent": (C.c_int, [_P, C.c_int, _P, _P, C.c_float, _P, _P]),
    "gmpc_bilevel_grad_inputs": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "gmpc_bilevel_grad_dynamics": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "gmpc_rollout_vjp": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_upper_loss": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "gmpc_expert_rollout": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(ExpertShape), _P, _P, _P, _P, _P]),
    "gmpc_expert_param_count": (C.c_long, [C.c_int, C.POINTER(ExpertShape)]),
    "gmpc_expert_loss_grad": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(ExpertShape), _P, _P, _P, _P, C.c_double,
                                        C.c_int, _P, _P, _P]),
    "gmpc_expert_vjp": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(ExpertShape), _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_dynamics_loss_grad": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_double, C.c_int, _P, _P, _P]),
    "gmpc_dynamics_ensemble_loss_grad": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                                                   C.c_double, C.c_int, _P, _P, _P]),
    "gmpc_polyak": (C.c_int, [_P, C.c_long, _P, _P, C.c_double, _P, _P]),
    "gmpc_critic_loss_grad": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "gmpc_critic_score_vjp": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "gmpc_critic_vjp": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_critic_dir_vjp": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gmpc_adam_clip_step": (C.c_int, [_P, C.c_long, _P, _P, _P, _P, C.c_float, C.c_int, C.c_double,
                                      C.c_double, C.c_double, C.c_double, C.c_double, _P]),
    "gmpc_bgemm_tn": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_float, C.c_float,
                                _P]),
    "gmpc_bgemm_tn_ex": (C.c_int, [_P, C.POINTER(BgemmDesc), _P]),
    "gmpc_bgemm_route": (C.c_int, [C.POINTER(BgemmDesc), C.POINTER(C.c_int)]),
    "gmpc_wgrad_ex": (C.c_int, [_P, C.POINTER(WgradDesc), _P]),
    "gmpc_wgrad_batch_ex": (C.c_int, [_P, C.POINTER(WgradDesc), C.c_int, _P, C.c_long, _P, C.POINTER(C.c_int)]),
    "gmpc_wgrad_route": (C.c_int, [C.POINTER(WgradDesc), C.POINTER(C.c_int)]),
    "gmpc_wgrad_batch_route": (C.c_int, [C.POINTER(WgradDesc), C.c_int, C.c_long, C.POINTER(C.c_int)]),
    "gmpc_linearize_ex": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P]),
    "gmpc_linearize_route": (C.c_int, [C.POINTER(Shape), C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "gmpc_linesearch_candidates": (C.c_long, [_P]),
    "gmpc_linesearch_stats": (C.c_int, [_P, C.POINTER(C.c_long), C.c_int]),
    "gmpc_profile_enable": (C.c_int, [_P, C.c_int]),
    "gmpc_set_linearize_event": (C.c_int, [_P, _P]),
    "gmpc_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "gmpc_profile_kernel_name": (C.c_char_p, [_P, C.c_int]),
    "gmpc_debug_buffer": (_P, [_P, C.c_int]),
    "gmpc_debug_buffer_count": (C.c_long, [_P, C.c_int]),
}

_lib = None


def load():
    """Load the shared object and bind every declared symbol (raises if one is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GmpcError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (make -C gan_mpc_amd/csrc).  gan_mpc_amd has no CPU fallback.")
    # The process must hold ONE HIP runtime: torch ships its own libamdhip64 and owns the device
    # buffers this library is handed, so it is loaded first and our shared object binds to that copy.
    # (Loaded the other way round, /opt/rocm's runtime comes in as a second instance that sees no
    # device and could not use torch's pointers anyway.)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise GmpcError(f"libgan_mpc_amd error {rc}: {load().gmpc_last_error().decode()}")
