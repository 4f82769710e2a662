"""ctypes binding of libmfm_hip (include/mfm.h) -- the reference-side stub a maintainer adds.

Every device buffer is a ``torch.Tensor`` on the GPU; only its ``data_ptr()`` crosses the boundary.  The library
fails loudly: a missing ``.so`` raises at load, a missing GPU raises at ``Context`` creation, and every non-zero
status code becomes ``MfmError`` carrying ``mfm_last_error()``.
"""
import ctypes as C
import os

import numpy as np

from .build import LIB

PHI4, GMM, LGCP = 0, 1, 2
FLOW_RWMH, FLOW_IMH = 0, 1
FAMILY_AUTO, FAMILY_TILE, FAMILY_WIDE = 0, 1, 2
EVAL_ROWS_MASK, EVAL_RELU, EVAL_CHAIN, EVAL_BCRT = 0xff, 0x100, 0x200, 0x400      # mfm_fm_eval_instance
ACTIVATIONS = {"relu": 0, "tanh": 1, "elu": 2, "gelu": 3, "swish": 4}          # exe_flow_matching.py:39-45


class MfmError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("dim", C.c_int32), ("fourier_dim", C.c_int32),
        ("hidden_t", C.c_int32 * 2), ("hidden_x", C.c_int32 * 2), ("hidden_xt", C.c_int32 * 2),
        ("n_chain_local", C.c_int32), ("n_chain_total", C.c_int32), ("chain_offset", C.c_int32),
        ("grad_clip", C.c_float), ("sigma", C.c_float), ("cond_flow", C.c_int32), ("hutch", C.c_int32),
        ("rtol", C.c_double), ("atol", C.c_double), ("mxstep", C.c_int32), ("n_ts", C.c_int32),
        ("learning_rate", C.c_double), ("adam_b1", C.c_double), ("adam_b2", C.c_double), ("adam_eps", C.c_double),
        ("weight_decay", C.c_double), ("update_clip", C.c_double),
        ("learning_iter", C.c_int32), ("warmup_steps", C.c_int32), ("max_eval_samples", C.c_int32),
        ("kernel_family", C.c_int32), ("activation", C.c_int32), ("ref_std", C.c_double), ("n_chain_valid", C.c_int32),
        ("depth_t", C.c_int32), ("depth_x", C.c_int32), ("depth_xt", C.c_int32),
        ("hidden_t3", C.c_int32), ("hidden_x3", C.c_int32), ("hidden_xt3", C.c_int32),
        ("ode_method", C.c_int32), ("ode_steps", C.c_int32),
    ]


MAX_DEPTH = 3          # include/mfm.h: MFM_MAX_DEPTH
AUTOCORR_LAG_BLOCK, AUTOCORR_TIME_BLOCK = 32, 256      # include/mfm.h: MFM_AUTOCORR_LAG_BLOCK / _TIME_BLOCK (lags per pass, float32 time block)
ODE_METHODS = {"dopri5": 0, "rk4": 1, "euler": 2}      # include/mfm.h: MFM_ODE_*
SVGD_OPTIMIZERS = {"sgd": 0, "adagrad": 1, "adam": 2, "cocob": 3}      # include/mfm.h: MFM_SVGD_*
SVGD_N_STATE = {"sgd": 0, "adagrad": 1, "adam": 2, "cocob": 5}         # state arrays [n, d] of each kind


_P = C.c_void_p
_U32 = C.c_uint32
_SIGS = {
    "mfm_last_error": (C.c_char_p, []),
    "mfm_version": (C.c_int, []),
    "mfm_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "mfm_destroy": (C.c_int, [_P]),
    "mfm_set_stream": (C.c_int, [_P, _P]),
    "mfm_sync": (C.c_int, [_P]),
    "mfm_num_params": (C.c_int, [_P]),
    "mfm_set_target": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.c_size_t]),
    "mfm_set_fourier": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "mfm_set_params": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "mfm_get_params": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "mfm_reset_optimizer": (C.c_int, [_P]),
    "mfm_mala_init": (C.c_int, [_P, _P, C.c_double, _P, _P]),
    "mfm_mala_step": (C.c_int, [_P, _U32, _U32, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_mala_step_keys": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_mala_run": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_hmc_step": (C.c_int, [_P, _U32, _U32, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P, _P]),
    "mfm_hmc_step_keys": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_int32, _P, _P, _P, _P, _P]),
    "mfm_hmc_run": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_hmc_run_lengths": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_mclmc_init": (C.c_int, [_P, _U32, _U32, _P]),
    "mfm_mclmc_step": (C.c_int, [_P, _U32, _U32, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P, _P, _P]),
    "mfm_mclmc_step_keys": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P, _P, _P]),
    "mfm_mclmc_run": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P,
                                _P, _P, _P, _P]),
    "mfm_ghmc_init": (C.c_int, [_P, _U32, _U32, _P, _P, _P]),
    "mfm_ghmc_step": (C.c_int, [_P, _U32, _U32, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_ghmc_step_keys": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_ghmc_run": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_double, C.c_double, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                               _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_meads_warmup": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                   _P, _P, _P, _P, _P, C.POINTER(C.c_double), _P, _P, _P]),
    "mfm_meads_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "mfm_chees_warmup": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                   C.c_int32, C.c_double, C.c_double, _P, _P, _P, C.POINTER(C.c_double), _P, _P, _P, _P]),
    "mfm_pt_exchange": (C.c_int, [_P, _U32, _U32, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mfm_pt_run": (C.c_int, [_P, C.c_int, _U32, _U32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, C.c_int,
                             C.c_int32, C.c_int32, C.c_int, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_set_lgcp_chol": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "mfm_eslice_init": (C.c_int, [_P, _P, _P]),
    "mfm_eslice_step": (C.c_int, [_P, _U32, _U32, C.c_double, _P, _P, _P, _P, _P]),
    "mfm_eslice_step_keys": (C.c_int, [_P, _P, C.c_double, _P, _P, _P, _P, _P]),
    "mfm_eslice_run": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_eslice_launch_plan": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mfm_cox_hmc_step": (C.c_int, [_P, _U32, _U32, C.c_double, C.c_double, C.c_int, _P, _P, _P, _P, _P]),
    "mfm_cox_hmc_step_keys": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_int32, _P, _P, _P, _P, _P]),
    "mfm_cox_hmc_run": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_cox_hmc_warmup": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_cox_hmc_launch_plan": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mfm_nuts_step": (C.c_int, [_P, _U32, _U32, C.c_double, C.c_double, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_nuts_step_keys": (C.c_int, [_P, _P, C.c_double, C.c_double, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_nuts_run": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32, _P, _P, _P,
                               _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_hmc_warmup": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_mala_warmup": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_hmc_set_inverse_mass": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int32]),
    "mfm_hmc_get_inverse_mass": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "mfm_hmc_warmup_window": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_nuts_warmup": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_double, _P, _P, _P,
                                  _P, _P, _P, _P, _P, _P, _P]),
    "mfm_nuts_warmup_window": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_double, _P, _P, _P,
                                         _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_loglik": (C.c_int, [_P, _P, _P]),
    "mfm_smc_delta": (C.c_int, [_P, _P, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "mfm_smc_weights": (C.c_int, [_P, _P, C.c_int, C.c_double, _P, C.POINTER(C.c_double)]),
    "mfm_smc_resample": (C.c_int, [_P, _U32, _U32, _P, C.c_int, _P, _P]),
    "mfm_smc_resample_scheme": (C.c_int, [_P, C.c_int, _U32, _U32, _P, C.c_int, _P, _P]),
    "mfm_gather_rows": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "mfm_acc_stats": (C.c_int, [_P, _P, C.c_int, _P]),
    "mfm_choice_logw": (C.c_int, [_P, _U32, _U32, _P, C.c_int, C.c_int, _P, _P]),
    "mfm_fm_loss_grad": (C.c_int, [_P, _U32, _U32, _P, _P, _P]),
    "mfm_fm_loss": (C.c_int, [_P, _U32, _U32, _P, C.c_int, C.c_int, C.c_int, _P]),
    "mfm_adamw_step": (C.c_int, [_P, _P]),
    "mfm_comm_unique_id": (C.c_int, [_P]),
    "mfm_comm_init": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "mfm_comm_destroy": (C.c_int, [_P]),
    "mfm_comm_count": (C.c_int, [_P, _P]),
    "mfm_grad_allreduce_begin": (C.c_int, [_P, _P]),
    "mfm_opt_state": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "mfm_vf_apply": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P]),
    "mfm_ode_transform": (C.c_int, [_P, C.c_int, C.c_int, _P, _U32, _U32, _P, C.c_int, _P, _P, _P]),
    "mfm_flow_step": (C.c_int, [_P, C.c_int, _U32, _U32, C.c_double, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_train_iter": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _U32, _U32, _U32, _U32, C.c_double, C.c_double,
                                 _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "mfm_beta_update": (C.c_int, [_P, C.c_double, _P, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    "mfm_normal_rows": (C.c_int, [_P, _P, C.c_int, _P]),
    "mfm_cis_select": (C.c_int, [_P, _U32, _U32, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_stein_disc": (C.c_int, [_P, _P, _P, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    "mfm_max_mean_disc": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_double)]),
    "mfm_autocorr": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P]),
    "mfm_chain_sums": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "mfm_chain_diag": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "mfm_svgd_sqdist": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "mfm_svgd_median": (C.c_int, [_P, _P, C.c_int32, _P]),
    "mfm_svgd_gradient": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "mfm_svgd_apply": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_svgd_step": (C.c_int, [_P, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_int32, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mfm_noise_prefetch": (C.c_int, [_P, C.c_int, C.POINTER(_U32), C.POINTER(_U32)]),
    "mfm_noise_drop": (C.c_int, [_P]),
    "mfm_get_counters": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "mfm_reset_counters": (C.c_int, [_P]),
    "mfm_debug_replay": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "mfm_profile": (C.c_int, [_P, C.c_int]),
    "mfm_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "mfm_pack_index": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "mfm_pack_index_T": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "mfm_fm_eval_instance": (C.c_int, [_P, C.c_int]),
    "mfm_threefry2x32": (C.c_int, [_U32, _U32, _U32, _U32, C.POINTER(_U32)]),
    "mfm_wsk_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mfm_nuts_launch_plan": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mfm_wgrad_info": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "mfm_wide_gemm_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_int32)]),
    "mfm_wide_gemm_tally": (C.c_int, [_P, C.POINTER(C.c_int64), C.c_int]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def load():
    """Load libmfm_hip.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise MfmError(f"{LIB} not found: build it with `python -m mfm_amd.build` (hipcc, gfx950)")
        # torch first: libmfm_hip.so depends on libamdhip64 by SONAME, and PyTorch-ROCm bundles its own copy.  Loaded after
        # torch the dependency resolves to the runtime torch already initialised (one HIP runtime per process: device
        # pointers and streams are shared with torch); loaded BEFORE torch it would bind /opt/rocm's copy, and the second
        # runtime in the process finds no device ("no HIP device available" from mfm_create).
        import torch  # noqa: F401
        lib = C.CDLL(os.environ.get("MFM_LIB", LIB))      # MFM_LIB: development override (A/B of kernel variants)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _chk(rc):
    if rc != 0:
        raise MfmError(f"libmfm_hip error {rc}: {load().mfm_last_error().decode()}")


def _ptr(t, dtype=None):
    """Device pointer of a contiguous CUDA tensor (dtype-checked: a wrong dtype would be silent garbage)."""
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous()):
        raise MfmError("expected a contiguous CUDA tensor")
    if dtype is not None and str(t.dtype).split(".")[-1] != dtype:
        raise MfmError(f"expected a {dtype} tensor, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


F32, F64, U8, I32, I64 = "float32", "float64", "uint8", "int32", "int64"


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def wsk_plan(n_jobs, nbb, cap, g_override=0, ranges=True):
    """``mfm_wsk_plan`` (host only): the stream-K weight-gradient plan as ``dict(G, q, r, n_slices)``, with ``ranges`` also ``wg``,
    an int32 array ``[G, 4]`` of ``(j0, bb0, cnt, n0)`` per workgroup."""
    lib = load()
    out = (C.c_int32 * 4)()
    _chk(lib.mfm_wsk_plan(int(n_jobs), int(nbb), int(cap), int(g_override), out, None))
    plan = dict(G=out[0], q=out[1], r=out[2], n_slices=out[3])
    if ranges:
        wg = np.empty((plan["G"], 4), dtype=np.int32)
        _chk(lib.mfm_wsk_plan(int(n_jobs), int(nbb), int(cap), int(g_override), out, wg.ctypes.data_as(C.POINTER(C.c_int32))))
        plan["wg"] = wg
    return plan


def nuts_launch_plan(dim, max_tree_depth):
    """``mfm_nuts_launch_plan`` (host only): ``(chains per workgroup, LDS bytes per workgroup, workgroups per CU)`` of the NUTS kernels."""
    w, sm, per_cu = C.c_int32(), C.c_int32(), C.c_int32()
    _chk(load().mfm_nuts_launch_plan(int(dim), int(max_tree_depth), C.byref(w), C.byref(sm), C.byref(per_cu)))
    return w.value, sm.value, per_cu.value


ESLICE_MAX_SUBITER = 64      # include/mfm.h: MFM_ESLICE_MAX_SUBITER


def eslice_launch_plan(dim):
    """``mfm_eslice_launch_plan`` (host only): ``(column tiles per wave of the kernel instance, LDS bytes per workgroup)`` of the
    elliptical slice kernel at ``dim``."""
    tpw, sm = C.c_int32(), C.c_int32()
    _chk(load().mfm_eslice_launch_plan(int(dim), C.byref(tpw), C.byref(sm)))
    return tpw.value, sm.value


def cox_hmc_launch_plan(dim):
    """``mfm_cox_hmc_launch_plan`` (host only): ``(column tiles per wave of the kernel instance, LDS bytes per workgroup)`` of the
    Cox process's HMC kernel at ``dim``."""
    tpw, sm = C.c_int32(), C.c_int32()
    _chk(load().mfm_cox_hmc_launch_plan(int(dim), C.byref(tpw), C.byref(sm)))
    return tpw.value, sm.value


def meads_plan(n_valid, n_folds, dim):
    """``mfm_meads_plan`` (host only): ``(m, m_pad, d_pad, Gram workgroups per iteration)`` of a MEADS warmup -- the fold size, its rows
    padded to the 64-row tile, ``dim`` padded to the 32-column chunk, and ``2 K T (T + 1) / 2`` with ``T = m_pad / 64``."""
    out = (C.c_int32 * 4)()
    _chk(load().mfm_meads_plan(int(n_valid), int(n_folds), int(dim), out))
    return tuple(out)


WGRAD_SLABS, WGRAD_STREAM_K, WGRAD_WIDE = 0, 1, 2     # mfm_wgrad_info: kind

# include/mfm.h: MFM_WGEMM_* (the instances of the wide family's GEMM, in enum order) and MFM_WGEMM_SW_* (its latched switches)
WGEMM = ("11", "11_dual", "12", "12_dual", "22", "22_dual", "22_ring8", "22_ring8_dual", "big", "lds", "lds_dual", "lds_wm1", "lds_wm1_dual")
WGEMM_SW = {"MFM_WIDE_NOLDS": 1, "MFM_WIDE_NO_SMALL_TILES": 2, "MFM_WIDE_WM1": 4, "MFM_WIDE_RING8": 8}


def wide_gemm_plan(rows, KB, NT, dual=False, KBT=0, switches=0):
    """``mfm_wide_gemm_plan`` (host only): ``(instance name from WGEMM, gridDim.x, gridDim.y, blockDim.x)`` of the wide family's GEMM
    for this shape under the switch mask ``switches`` (OR of ``WGEMM_SW`` values)."""
    out = (C.c_int32 * 4)()
    _chk(load().mfm_wide_gemm_plan(int(rows), int(KB), int(NT), int(bool(dual)), int(KBT), int(switches), out))
    return WGEMM[out[0]], out[1], out[2], out[3]


class Context:
    """Owner of one ``mfm_ctx`` (one GPU, one process)."""

    def __init__(self, **kw):
        import torch
        self.lib = load()
        if not torch.cuda.is_available():
            raise MfmError("no GPU visible: the MFM hot path has no CPU fallback")
        cfg = Config()
        defaults = dict(fourier_dim=128, hidden_t=(128, 128), hidden_x=(128, 128), hidden_xt=(128, 128),
                        chain_offset=0, grad_clip=0.0, sigma=1e-4, cond_flow=1, hutch=0, rtol=1e-5, atol=1e-5,
                        mxstep=1000, n_ts=2, learning_rate=1e-3, adam_b1=0.9, adam_b2=0.999, adam_eps=1e-8,
                        weight_decay=1e-4, update_clip=1.0, learning_iter=400, warmup_steps=0, max_eval_samples=0,
                        kernel_family=int(os.environ.get("MFM_KERNEL_FAMILY", FAMILY_AUTO)), activation=0)
        defaults.update(kw)
        defaults.setdefault("n_chain_total", defaults["n_chain_local"])
        for k, v in defaults.items():
            if k in ("hidden_t", "hidden_x", "hidden_xt"):      # lists of 1 .. MAX_DEPTH widths (exe_flow_matching.py:74-85)
                hs = [int(h) for h in v]
                if not 1 <= len(hs) <= MAX_DEPTH:
                    raise MfmError(f"{k}: {len(hs)} hidden layers; the kernels take 1 to {MAX_DEPTH} per branch")
                setattr(cfg, k, (C.c_int32 * 2)(*(hs + hs)[:2]))
                setattr(cfg, "depth_" + k[7:], len(hs))
                setattr(cfg, k + "3", hs[2] if len(hs) > 2 else 0)
            else:
                setattr(cfg, k, v)
        self.cfg = cfg
        self.dim, self.n_local = int(cfg.dim), int(cfg.n_chain_local)
        h = _P()
        _chk(self.lib.mfm_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.n_params = self.lib.mfm_num_params(h)
        self.use_current_stream()

    before_params = None      # set by the engine: called before any call that reads or writes the network parameters
    # (a deferred optimizer step whose gradient all-reduce is still in flight is applied there)

    def _p(self):
        if self.before_params is not None:
            self.before_params()

    def close(self):
        if getattr(self, "h", None):
            self.lib.mfm_destroy(self.h)
            self.h = None

    __del__ = close

    def use_current_stream(self):
        import torch
        _chk(self.lib.mfm_set_stream(self.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def sync(self):
        _chk(self.lib.mfm_sync(self.h))

    # ---- target / parameters ------------------------------------------------------------------------------
    def set_target(self, kind, params):
        p = np.ascontiguousarray(params, dtype=np.float64)
        _chk(self.lib.mfm_set_target(self.h, kind, p.ctypes.data_as(C.POINTER(C.c_double)), p.size))

    def set_fourier(self, f):
        f = _f32(f)
        assert f.size == self.cfg.fourier_dim
        _chk(self.lib.mfm_set_fourier(self.h, f.ctypes.data_as(C.POINTER(C.c_float))))

    def set_params(self, flat):
        self._p()
        flat = _f32(flat)
        assert flat.size == self.n_params, (flat.size, self.n_params)
        _chk(self.lib.mfm_set_params(self.h, flat.ctypes.data_as(C.POINTER(C.c_float))))

    def get_params(self):
        self._p()
        out = np.empty(self.n_params, dtype=np.float32)
        _chk(self.lib.mfm_get_params(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def reset_optimizer(self):
        self._p()
        _chk(self.lib.mfm_reset_optimizer(self.h))

    # ---- kernels ----------------------------------------------------------------------------------------------
    def mala_init(self, pos, beta, logp, grad):
        _chk(self.lib.mfm_mala_init(self.h, _ptr(pos, F32), float(beta), _ptr(logp, F64), _ptr(grad, F32)))

    def mala_step(self, key, beta, step_size, pos, logp, grad, acc=None, is_acc=None, proposed=None, weight=None,
                  textbook=False):
        _chk(self.lib.mfm_mala_step(self.h, int(key[0]), int(key[1]), float(beta), float(step_size), int(textbook),
                                    _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(acc, F32), _ptr(is_acc, U8),
                                    _ptr(proposed, F32), _ptr(weight, F32)))

    def mala_step_keys(self, keys, beta, step_size, pos, logp, grad, acc=None, is_acc=None, proposed=None, weight=None,
                       textbook=False):
        """``keys``: int32/uint32 device tensor [n_chain_local, 2], one key per chain (the caller vmaps over its own keys)."""
        _chk(self.lib.mfm_mala_step_keys(self.h, _ptr(keys, I32), float(beta), float(step_size), int(textbook),
                                         _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(acc, F32), _ptr(is_acc, U8),
                                         _ptr(proposed, F32), _ptr(weight, F32)))

    def mala_run(self, key, beta, step_size, n_steps, pos, logp, grad, thin=0, n_acc=None, acc_sum=None, acc=None, is_acc=None,
                 proposed=None, weight=None, traj_pos=None, traj_logp=None, textbook=False, key_mode=None):
        """``mfm_mala_run``: ``n_steps`` MALA steps in one call, state updated in place.  ``key``: one key ``(2,)`` (step-major: step j
        uses ``split(key, n_steps)[j]`` as ``mala_step`` uses its key) or an int32/uint32 device tensor ``[n_chain_local, 2]``
        (chain-major: step j of chain b uses ``split(key[b], n_steps)[j]`` as ``mala_step_keys`` uses a chain's key).  ``key_mode``
        overrides the choice made from the key's shape."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        _chk(self.lib.mfm_mala_run(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step_size),
                                   int(textbook), int(n_steps), int(thin), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                   _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(acc, F32), _ptr(is_acc, U8), _ptr(proposed, F32),
                                   _ptr(weight, F32), _ptr(traj_pos, F32), _ptr(traj_logp, F64)))

    # ---- elliptical slice sampling for the Cox process (include/mfm.h: mfm_eslice_*) ----
    def set_lgcp_chol(self, chol):
        """``mfm_set_lgcp_chol``: install the lower Cholesky factor ``chol [dim, dim]`` (float64, host) of the Cox process prior."""
        L = np.ascontiguousarray(chol, dtype=np.float64)
        if L.shape != (self.dim, self.dim):
            raise MfmError(f"chol must be [{self.dim}, {self.dim}], got {L.shape}")
        _chk(self.lib.mfm_set_lgcp_chol(self.h, L.ctypes.data_as(C.POINTER(C.c_double))))

    def eslice_init(self, pos, loglik):
        _chk(self.lib.mfm_eslice_init(self.h, _ptr(pos, F32), _ptr(loglik, F64)))

    def eslice_step(self, key, beta, pos, loglik, subiter=None, theta=None, momentum=None):
        """``mfm_eslice_step``: one elliptical slice transition of every local chain, state ``(pos, loglik)`` updated in place."""
        _chk(self.lib.mfm_eslice_step(self.h, int(key[0]), int(key[1]), float(beta), _ptr(pos, F32), _ptr(loglik, F64),
                                      _ptr(subiter, I32), _ptr(theta, F64), _ptr(momentum, F32)))

    def eslice_step_keys(self, keys, beta, pos, loglik, subiter=None, theta=None, momentum=None):
        """The same transition on the caller's own keys, an int32/uint32 device tensor ``[n_chain_local, 2]``."""
        _chk(self.lib.mfm_eslice_step_keys(self.h, _ptr(keys, I32), float(beta), _ptr(pos, F32), _ptr(loglik, F64),
                                           _ptr(subiter, I32), _ptr(theta, F64), _ptr(momentum, F32)))

    def eslice_run(self, key, beta, n_steps, pos, loglik, thin=0, subiter_sum=None, n_capped=None, traj_pos=None, traj_loglik=None,
                   subiter=None, theta=None, momentum=None, subiter_max=None, key_mode=None):
        """``mfm_eslice_run``: ``n_steps`` transitions in one launch, state updated in place; ``key`` and ``key_mode`` as ``mala_run``'s;
        ``subiter`` / ``theta`` / ``momentum`` take the last transition's info, ``subiter_max`` the most evaluations of any one transition."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        _chk(self.lib.mfm_eslice_run(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), int(n_steps), int(thin),
                                     _ptr(pos, F32), _ptr(loglik, F64), _ptr(subiter_sum, I32), _ptr(n_capped, I32),
                                     _ptr(traj_pos, F32), _ptr(traj_loglik, F64), _ptr(subiter, I32), _ptr(theta, F64), _ptr(momentum, F32), _ptr(subiter_max, I32)))

    def hmc_step(self, key, beta, step_size, num_steps, pos, logp, grad, acc=None, is_acc=None):
        """Build-side mode (``mfm_hmc_step``): one HMC step of every local chain, state updated in place."""
        _chk(self.lib.mfm_hmc_step(self.h, int(key[0]), int(key[1]), float(beta), float(step_size), int(num_steps),
                                   _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(acc, F32), _ptr(is_acc, U8)))

    def hmc_step_keys(self, keys, beta, step_size, num_steps, pos, logp, grad, acc=None, is_acc=None):
        """``mfm_hmc_step_keys``: ``keys`` is an int32/uint32 device tensor [n_chain_local, 2], one key per chain."""
        _chk(self.lib.mfm_hmc_step_keys(self.h, _ptr(keys, I32), float(beta), float(step_size), int(num_steps),
                                        _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(acc, F32), _ptr(is_acc, U8)))

    def hmc_run(self, key, beta, step_size, num_steps, n_steps, pos, logp, grad, thin=0, n_acc=None, acc_sum=None, acc=None,
                is_acc=None, traj_pos=None, traj_logp=None, key_mode=None):
        """``mfm_hmc_run``: ``n_steps`` HMC steps of ``num_steps`` leapfrog steps each in one launch, state updated in place.  ``key``
        as ``mala_run``'s: one key ``(2,)`` (step-major: step j uses ``split(key, n_steps)[j]`` as ``hmc_step`` uses its key) or an
        int32/uint32 device tensor ``[n_chain_local, 2]`` (chain-major: step j of chain b uses ``split(key[b], n_steps)[j]`` as
        ``hmc_step_keys`` uses a chain's key).  ``key_mode`` overrides the choice made from the key's shape."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        _chk(self.lib.mfm_hmc_run(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step_size),
                                  int(num_steps), int(n_steps), int(thin), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                  _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(acc, F32), _ptr(is_acc, U8),
                                  _ptr(traj_pos, F32), _ptr(traj_logp, F64)))

    def hmc_run_lengths(self, key, beta, step_size, num_steps, pos, logp, grad, thin=0, n_acc=None, acc_sum=None, acc=None, is_acc=None,
                        traj_pos=None, traj_logp=None, total_leapfrog=None, key_mode=None):
        """``mfm_hmc_run_lengths``: ``hmc_run`` with ``num_steps`` an int32 device tensor ``[n_steps]``, the leapfrog steps of each HMC
        step (every entry in [1, 100000]); ``total_leapfrog`` (int64 device tensor of one element, optional) takes their sum."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        n_steps = 0 if num_steps is None else int(num_steps.numel())
        _chk(self.lib.mfm_hmc_run_lengths(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step_size),
                                          _ptr(num_steps, I32), n_steps, int(thin), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                          _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(acc, F32), _ptr(is_acc, U8),
                                          _ptr(traj_pos, F32), _ptr(traj_logp, F64), _ptr(total_leapfrog, I64)))

    # ---- microcanonical Langevin Monte Carlo (include/mfm.h: mfm_mclmc_*) ----
    def mclmc_init(self, key, momentum):
        """``mfm_mclmc_init``: the unit momenta ``momentum [n_chain_local, dim]`` (float64), chain b from ``split(key, n_chain_total)[chain_offset + b]``."""
        _chk(self.lib.mfm_mclmc_init(self.h, int(key[0]), int(key[1]), _ptr(momentum, F64)))

    def mclmc_step(self, key, beta, step_size, L, integrator, pos, logp, grad, momentum, energy_change=None, kinetic_change=None):
        """``mfm_mclmc_step``: one MCLMC step of every local chain (``integrator`` 0: leapfrog, 1: McLachlan; ``L``: the momentum
        decoherence length, ``inf`` for none), state ``(pos, logp, grad, momentum)`` updated in place; the two infos are float64 ``[n_chain_local]``."""
        _chk(self.lib.mfm_mclmc_step(self.h, int(key[0]), int(key[1]), float(beta), float(step_size), float(L), int(integrator),
                                     _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(momentum, F64), _ptr(energy_change, F64), _ptr(kinetic_change, F64)))

    def mclmc_step_keys(self, keys, beta, step_size, L, integrator, pos, logp, grad, momentum, energy_change=None, kinetic_change=None):
        """``mfm_mclmc_step_keys``: ``keys`` is an int32/uint32 device tensor [n_chain_local, 2], one key per chain."""
        _chk(self.lib.mfm_mclmc_step_keys(self.h, _ptr(keys, I32), float(beta), float(step_size), float(L), int(integrator),
                                          _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(momentum, F64), _ptr(energy_change, F64), _ptr(kinetic_change, F64)))

    def mclmc_run(self, key, beta, step_size, L, integrator, n_steps, pos, logp, grad, momentum, thin=0, de_sum=None, de_sumsq=None,
                  n_nonfinite=None, energy_trace=None, traj_pos=None, traj_logp=None, key_mode=None):
        """``mfm_mclmc_run``: ``n_steps`` MCLMC steps in one launch, state updated in place; ``key`` / ``key_mode`` and the trajectory as
        ``hmc_run``'s.  Per chain (optional): ``de_sum`` / ``de_sumsq`` float64, the sums of the steps' energy changes and of their
        squares, ``n_nonfinite`` int32, the steps whose energy change is not finite; ``energy_trace`` float64 ``[n_steps, n_chain_local]``."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        _chk(self.lib.mfm_mclmc_run(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step_size), float(L),
                                    int(integrator), int(n_steps), int(thin), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(momentum, F64),
                                    _ptr(de_sum, F64), _ptr(de_sumsq, F64), _ptr(n_nonfinite, I32), _ptr(energy_trace, F64),
                                    _ptr(traj_pos, F32), _ptr(traj_logp, F64)))

    # ---- generalized HMC with persistent momentum (include/mfm.h: mfm_ghmc_*) ----
    def ghmc_init(self, key, momentum, slice_, inverse_mass=None):
        """``mfm_ghmc_init``: the momenta ``momentum [n_chain_local, dim]`` (float64, ``n / sqrt(inverse_mass)``) and the slice variables
        ``slice_ [n_chain_local]`` (float64, in (-1, 1)), chain b from ``split(key, n_chain_total)[chain_offset + b]``.  ``inverse_mass``:
        a float64 device tensor ``[dim]`` or ``None`` (unit metric)."""
        _chk(self.lib.mfm_ghmc_init(self.h, int(key[0]), int(key[1]), _ptr(inverse_mass, F64), _ptr(momentum, F64), _ptr(slice_, F64)))

    def ghmc_step(self, key, beta, step_size, alpha, delta, pos, logp, grad, momentum, slice_, inverse_mass=None, acc=None, is_acc=None,
                  energy_change=None):
        """``mfm_ghmc_step``: one GHMC transition (one leapfrog step, persistent momentum, slice accept) of every local chain, state
        ``(pos, logp, grad, momentum, slice_)`` updated in place; infos: ``acc`` float32, ``is_acc`` uint8, ``energy_change`` float64."""
        _chk(self.lib.mfm_ghmc_step(self.h, int(key[0]), int(key[1]), float(beta), float(step_size), float(alpha), float(delta), _ptr(inverse_mass, F64),
                                    _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(momentum, F64), _ptr(slice_, F64),
                                    _ptr(acc, F32), _ptr(is_acc, U8), _ptr(energy_change, F64)))

    def ghmc_step_keys(self, keys, beta, step_size, alpha, delta, pos, logp, grad, momentum, slice_, inverse_mass=None, acc=None, is_acc=None,
                       energy_change=None):
        """``mfm_ghmc_step_keys``: ``keys`` is an int32/uint32 device tensor [n_chain_local, 2], one key per chain."""
        _chk(self.lib.mfm_ghmc_step_keys(self.h, _ptr(keys, I32), float(beta), float(step_size), float(alpha), float(delta), _ptr(inverse_mass, F64),
                                         _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(momentum, F64), _ptr(slice_, F64),
                                         _ptr(acc, F32), _ptr(is_acc, U8), _ptr(energy_change, F64)))

    def ghmc_run(self, key, beta, step_size, alpha, delta, n_steps, pos, logp, grad, momentum, slice_, inverse_mass=None, thin=0, n_acc=None,
                 acc_sum=None, energy_sum=None, acc=None, is_acc=None, energy_change=None, traj_pos=None, traj_logp=None, key_mode=None):
        """``mfm_ghmc_run``: ``n_steps`` GHMC transitions in one launch, state updated in place; ``key`` / ``key_mode`` and the trajectory
        as ``hmc_run``'s.  Per chain (optional): ``n_acc`` int32, ``acc_sum`` float64 (sum of the acceptance rates), ``energy_sum``
        float64 (sum of dH over the accepted steps); ``acc`` / ``is_acc`` / ``energy_change``: the last step's infos."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        _chk(self.lib.mfm_ghmc_run(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step_size), float(alpha),
                                   float(delta), _ptr(inverse_mass, F64), int(n_steps), int(thin), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                   _ptr(momentum, F64), _ptr(slice_, F64), _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(energy_sum, F64),
                                   _ptr(acc, F32), _ptr(is_acc, U8), _ptr(energy_change, F64), _ptr(traj_pos, F32), _ptr(traj_logp, F64)))

    def meads_warmup(self, key, beta, step0, alpha0, n_iter, pos, logp, grad, momentum, slice_, n_folds=4, n_valid=None, shuffle_every=0, perms=None,
                     inverse_mass_out=None, trace=None, mass_trace=None, key_mode=None, read_result=True):
        """``mfm_meads_warmup``: ``n_iter`` GHMC transitions of all chains with the step size, the diagonal inverse mass, alpha and delta
        set per fold from cross-chain statistics; state updated in place.  ``perms``: int32 device tensor ``[(n_iter - 1) //
        shuffle_every, n_valid]`` (needed when a shuffle falls inside ``n_iter``).  Returns ``(eps, alpha, delta)`` of the closing pass
        over all chains (``None`` with ``read_result=False``: no host synchronisation); ``inverse_mass_out`` float64 ``[dim]`` takes its
        ``sd^2``, ``trace`` float64 ``[n_iter, n_folds, 6]``, ``mass_trace`` float64 ``[n_iter, n_folds, dim]``."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        res = (C.c_double * 3)() if read_result else None
        _chk(self.lib.mfm_meads_warmup(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step0), float(alpha0), int(n_iter),
                                       int(pos.shape[0] if n_valid is None else n_valid), int(n_folds), int(shuffle_every), _ptr(perms, I32),
                                       _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(momentum, F64), _ptr(slice_, F64), res,
                                       _ptr(inverse_mass_out, F64), _ptr(trace, F64), _ptr(mass_trace, F64)))
        return tuple(res) if read_result else None

    def chees_warmup(self, key, beta, step0, n_iter, pos, logp, grad, traj0=None, n_valid=None, target_accept=0.651, learning_rate=0.025,
                     max_leapfrog=1000, decay=0.5, divergence_threshold=1000.0, trace=None, prop=None, vel=None, alpha=None, key_mode=None,
                     read_result=True):
        """``mfm_chees_warmup``: ``n_iter`` ChEES-HMC iterations, the step size and the trajectory length adapted across the chains
        (the algorithm: ``include/mfm.h``, ``tests/chees_ref.py``); state updated in place.  ``key`` / ``key_mode`` as ``hmc_run``'s.
        ``traj0`` defaults to ``step0`` (one leapfrog step), ``n_valid`` to every chain.  Optional device tensors: ``trace`` float64
        ``[n_iter, 7]``; ``prop`` float32 ``[n, dim]``, ``vel`` float64 ``[n, dim]``, ``alpha`` float64 ``[n]``, the last iteration's
        records.  Returns ``(step_size, trajectory_length, last_step_size, last_trajectory_length)``, which waits for the stream, or
        ``None`` with ``read_result=False`` (no host synchronisation at all)."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        n = self.n_local
        for name, t_, need in (("trace", trace, max(int(n_iter), 0) * 7), ("prop", prop, n * self.dim), ("vel", vel, n * self.dim), ("alpha", alpha, n)):
            if t_ is not None and t_.numel() < need:
                raise MfmError(f"{name} must hold {need} elements (got {t_.numel()})")
        res = (C.c_double * 4)() if read_result else None
        _chk(self.lib.mfm_chees_warmup(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step0),
                                       float(step0 if traj0 is None else traj0), int(n_iter), int(n if n_valid is None else n_valid),
                                       float(target_accept), float(learning_rate), int(max_leapfrog), float(decay), float(divergence_threshold),
                                       _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), res, _ptr(trace, F64), _ptr(prop, F32),
                                       _ptr(vel, F64), _ptr(alpha, F64)))
        return tuple(res) if read_result else None

    @staticmethod
    def _host_f64(a, n=None):
        """A host vector for a ``const double* h_`` argument (kept alive by the caller for the duration of the call)."""
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
        if n is not None and a.size != n:
            raise MfmError(f"expected {n} values, got {a.size}")
        return a, a.ctypes.data_as(C.POINTER(C.c_double))

    def pt_exchange(self, key, betas, n_ladders, parity, pos, logp, grad, replica=None, swap_accepted=None, swap_prob=None):
        """``mfm_pt_exchange``: one exchange sweep of parallel tempering on ``key``: in every one of the ``n_ladders`` ladders of
        ``len(betas)`` slots the pairs ``(k, k + 1)`` with ``k % 2 == parity`` (chain ``r * K + k`` is slot ``k`` of ladder ``r``); the
        pair whose lower slot is chain ``i`` draws from ``split(key, n_chain_total)[i]``.  State swapped in place.  Optional device
        tensors: ``replica`` int32 ``[K * R]``, permuted with the rows; ``swap_accepted`` int32 / ``swap_prob`` float64 ``[R, K - 1]``,
        ADDED to."""
        hb, pb = self._host_f64(betas)
        K, R = hb.size, int(n_ladders)
        for name, t_, need in (("replica", replica, K * R), ("swap_accepted", swap_accepted, R * (K - 1)), ("swap_prob", swap_prob, R * (K - 1))):
            if t_ is not None and t_.numel() < need:
                raise MfmError(f"{name} must hold {need} elements (got {t_.numel()})")
        _chk(self.lib.mfm_pt_exchange(self.h, int(key[0]), int(key[1]), pb, K, R, int(parity), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                      _ptr(replica, I32), _ptr(swap_accepted, I32), _ptr(swap_prob, F64)))

    def pt_run(self, key, betas, step_sizes, n_ladders, n_local, n_rounds, pos, logp, grad, kernel="hmc", num_steps=10, textbook=False,
               exchange=True, thin=0, n_acc=None, acc_sum=None, replica=None, swap_accepted=None, swap_prob=None, traj_pos=None,
               traj_logp=None):
        """``mfm_pt_run``: ``n_rounds`` rounds of parallel tempering in one call (it only enqueues), state updated in place.  A round is
        ``n_local`` local steps of every chain at its slot's ``(betas[k], step_sizes[k])`` -- ``kernel`` ``"hmc"`` with ``num_steps``
        leapfrog steps, or ``"mala"`` under ``textbook`` -- then, with ``exchange``, one even-odd sweep.  The key schedule:
        ``include/mfm.h``.  Optional device tensors: ``n_acc`` int32 / ``acc_sum`` float64 ``[K * R]`` (per slot, over all rounds);
        ``replica`` int32 ``[K * R]`` (in and out); ``swap_accepted`` int32 / ``swap_prob`` float64 ``[R, K - 1]``; with ``thin`` slot 0 of
        every ladder after each kept round: ``traj_pos`` float32 ``[n_rounds / thin, R, dim]``, ``traj_logp`` float64 ``[n_rounds / thin, R]``."""
        hb, pb = self._host_f64(betas)
        K, R = hb.size, int(n_ladders)
        hs, ps = self._host_f64(step_sizes, K)
        kern = {"mala": 0, "hmc": 1}.get(kernel, kernel)
        n_keep = max(int(n_rounds), 0) // int(thin) if int(thin) > 0 else 0
        for name, t_, need in (("n_acc", n_acc, K * R), ("acc_sum", acc_sum, K * R), ("replica", replica, K * R),
                               ("swap_accepted", swap_accepted, R * (K - 1)), ("swap_prob", swap_prob, R * (K - 1)),
                               ("traj_pos", traj_pos, n_keep * R * self.dim), ("traj_logp", traj_logp, n_keep * R)):
            if t_ is not None and t_.numel() < need:
                raise MfmError(f"{name} must hold {need} elements (got {t_.numel()})")
        _chk(self.lib.mfm_pt_run(self.h, int(kern), int(key[0]), int(key[1]), pb, ps, K, R, int(num_steps), int(bool(textbook)), int(n_local),
                                 int(n_rounds), int(bool(exchange)) if not isinstance(exchange, int) else int(exchange), int(thin),
                                 _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(replica, I32),
                                 _ptr(swap_accepted, I32), _ptr(swap_prob, F64), _ptr(traj_pos, F32), _ptr(traj_logp, F64)))

    def _nuts_info(self, depth, num_leapfrog, is_turning, is_divergent, acceptance_rate, energy):
        return (_ptr(depth, I32), _ptr(num_leapfrog, I32), _ptr(is_turning, U8), _ptr(is_divergent, U8), _ptr(acceptance_rate, F64), _ptr(energy, F64))

    def nuts_step(self, key, beta, step_size, max_tree_depth, pos, logp, grad, divergence_threshold=1000.0, depth=None, num_leapfrog=None,
                  is_turning=None, is_divergent=None, acceptance_rate=None, energy=None):
        """Build-side mode (``mfm_nuts_step``): one No-U-turn transition of every local chain, state updated in place.  The info
        tensors ``[n_chain_local]`` are optional: ``depth`` / ``num_leapfrog`` int32, the two flags uint8, ``acceptance_rate`` /
        ``energy`` float64."""
        _chk(self.lib.mfm_nuts_step(self.h, int(key[0]), int(key[1]), float(beta), float(step_size), int(max_tree_depth), float(divergence_threshold),
                                    _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                    *self._nuts_info(depth, num_leapfrog, is_turning, is_divergent, acceptance_rate, energy)))

    def nuts_step_keys(self, keys, beta, step_size, max_tree_depth, pos, logp, grad, divergence_threshold=1000.0, depth=None, num_leapfrog=None,
                       is_turning=None, is_divergent=None, acceptance_rate=None, energy=None):
        """``mfm_nuts_step_keys``: ``keys`` is an int32/uint32 device tensor [n_chain_local, 2], one key per chain."""
        _chk(self.lib.mfm_nuts_step_keys(self.h, _ptr(keys, I32), float(beta), float(step_size), int(max_tree_depth), float(divergence_threshold),
                                         _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                         *self._nuts_info(depth, num_leapfrog, is_turning, is_divergent, acceptance_rate, energy)))

    def nuts_run(self, key, beta, step_size, max_tree_depth, n_steps, pos, logp, grad, divergence_threshold=1000.0, thin=0, leapfrog_sum=None,
                 acc_sum=None, n_divergent=None, depth_sum=None, depth=None, num_leapfrog=None, is_turning=None, is_divergent=None,
                 acceptance_rate=None, energy=None, traj_pos=None, traj_logp=None, key_mode=None):
        """``mfm_nuts_run``: ``n_steps`` No-U-turn transitions in one launch, state updated in place; ``key`` / ``key_mode`` / ``thin`` /
        the trajectory as ``hmc_run``'s.  Per-chain totals (optional): ``leapfrog_sum`` int64, ``acc_sum`` float64 (the sum of the
        transitions' acceptance rates), ``n_divergent`` / ``depth_sum`` int32; the info tensors take the LAST transition's."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        _chk(self.lib.mfm_nuts_run(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step_size),
                                   int(max_tree_depth), float(divergence_threshold), int(n_steps), int(thin),
                                   _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                   _ptr(leapfrog_sum, I64), _ptr(acc_sum, F64), _ptr(n_divergent, I32), _ptr(depth_sum, I32),
                                   *self._nuts_info(depth, num_leapfrog, is_turning, is_divergent, acceptance_rate, energy),
                                   _ptr(traj_pos, F32), _ptr(traj_logp, F64)))

    def _warmup_sizes(self, n_steps, step_avg, step_last, n_acc, acc_sum, step_traj):
        """The library cannot see a tensor's length: an output shorter than the kernel writes is refused here."""
        for name, t_ in (("step_avg", step_avg), ("step_last", step_last), ("n_acc", n_acc), ("acc_sum", acc_sum)):
            if t_ is not None and t_.numel() < self.n_local:
                raise MfmError(f"{name} must hold n_chain_local = {self.n_local} elements (got {t_.numel()})")
        if step_traj is not None and step_traj.numel() < max(int(n_steps), 0) * self.n_local:
            raise MfmError(f"step_traj must hold n_steps * n_chain_local = {int(n_steps) * self.n_local} elements (got {step_traj.numel()})")

    def hmc_warmup(self, key, beta, step0, num_steps, n_steps, target_accept, pos, logp, grad, step_avg, step_last=None, n_acc=None,
                   acc_sum=None, step_traj=None, key_mode=None):
        """``mfm_hmc_warmup``: ``n_steps`` HMC steps of ``num_steps`` leapfrog steps each in one launch, every chain adapting its own
        step size from ``step0`` by dual averaging towards the acceptance probability ``target_accept`` (the recursion:
        ``include/mfm.h``); state updated in place.  ``key`` / ``key_mode`` as ``hmc_run``'s.  ``step_avg`` (float64 ``[n_chain_local]``,
        required) takes the averaged step size, the result; ``step_last`` the last iterate; ``step_traj`` (float64
        ``[n_steps, n_chain_local]``) the step size used at every step."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        self._warmup_sizes(n_steps, step_avg, step_last, n_acc, acc_sum, step_traj)
        _chk(self.lib.mfm_hmc_warmup(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step0),
                                     int(num_steps), int(n_steps), float(target_accept), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                     _ptr(step_avg, F64), _ptr(step_last, F64), _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(step_traj, F64)))

    # HMC for the Cox process on the 16-chain GEMM tile (lgcp_hmc.hip): the keyword names of the hmc_* siblings; the state is the MALA
    # state (mala_init)
    def cox_hmc_step(self, key, beta, step_size, num_steps, pos, logp, grad, acc=None, is_acc=None):
        """``mfm_cox_hmc_step``: one HMC step of every local chain of a Cox process context, state updated in place."""
        _chk(self.lib.mfm_cox_hmc_step(self.h, int(key[0]), int(key[1]), float(beta), float(step_size), int(num_steps),
                                       _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(acc, F32), _ptr(is_acc, U8)))

    def cox_hmc_step_keys(self, keys, beta, step_size, num_steps, pos, logp, grad, acc=None, is_acc=None):
        """``mfm_cox_hmc_step_keys``: ``keys`` is an int32/uint32 device tensor [n_chain_local, 2], one key per chain."""
        _chk(self.lib.mfm_cox_hmc_step_keys(self.h, _ptr(keys, I32), float(beta), float(step_size), int(num_steps),
                                            _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32), _ptr(acc, F32), _ptr(is_acc, U8)))

    def cox_hmc_run(self, key, beta, step_size, num_steps, n_steps, pos, logp, grad, thin=0, n_acc=None, acc_sum=None, acc=None,
                    is_acc=None, traj_pos=None, traj_logp=None, key_mode=None):
        """``mfm_cox_hmc_run``: ``n_steps`` HMC steps of ``num_steps`` leapfrog steps each in one launch; arguments as ``hmc_run``'s."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        _chk(self.lib.mfm_cox_hmc_run(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step_size),
                                      int(num_steps), int(n_steps), int(thin), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                      _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(acc, F32), _ptr(is_acc, U8),
                                      _ptr(traj_pos, F32), _ptr(traj_logp, F64)))

    def cox_hmc_warmup(self, key, beta, step0, num_steps, n_steps, target_accept, pos, logp, grad, step_avg, step_last=None, n_acc=None,
                       acc_sum=None, step_traj=None, key_mode=None):
        """``mfm_cox_hmc_warmup``: the run with every chain adapting its own step size by dual averaging; arguments and outputs as
        ``hmc_warmup``'s."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        self._warmup_sizes(n_steps, step_avg, step_last, n_acc, acc_sum, step_traj)
        _chk(self.lib.mfm_cox_hmc_warmup(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step0),
                                         int(num_steps), int(n_steps), float(target_accept), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                         _ptr(step_avg, F64), _ptr(step_last, F64), _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(step_traj, F64)))

    _inv_mass = None      # host copy of the installed vector (None: unit mass), what set_inverse_mass compares with

    def set_inverse_mass(self, inv_mass=None):
        """``mfm_hmc_set_inverse_mass``: install the diagonal ``inv_mass`` (``[dim]`` float64, finite and positive) of the inverse mass
        matrix for every later ``hmc_step`` / ``hmc_step_keys`` / ``hmc_run`` / ``hmc_warmup`` call; ``None`` returns to unit mass.  The
        context keeps a host copy and makes no call when nothing changes."""
        if inv_mass is None:
            if self._inv_mass is not None:
                _chk(self.lib.mfm_hmc_set_inverse_mass(self.h, None, 0))
                self._inv_mass = None
            return
        v = np.ascontiguousarray(inv_mass, dtype=np.float64).reshape(-1)
        if self._inv_mass is not None and v.shape == self._inv_mass.shape and np.array_equal(v, self._inv_mass):
            return
        _chk(self.lib.mfm_hmc_set_inverse_mass(self.h, v.ctypes.data_as(C.POINTER(C.c_double)), v.size))
        self._inv_mass = v.copy()

    def get_inverse_mass(self):
        """``mfm_hmc_get_inverse_mass``: ``(vector [dim] as the library holds it -- ones when none is installed --, whether one is)``."""
        out, is_set = np.empty(self.dim, dtype=np.float64), C.c_int32(0)
        _chk(self.lib.mfm_hmc_get_inverse_mass(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(is_set)))
        return out, bool(is_set.value)

    def hmc_warmup_window(self, key, beta, step0, num_steps, n_steps, target_accept, pos, logp, grad, step_avg, pos_sum, pos_sumsq,
                          step_last=None, n_acc=None, acc_sum=None, step_traj=None, key_mode=None):
        """``mfm_hmc_warmup_window``: ``hmc_warmup`` on the mass instances (the installed vector, or ones), which also leaves in
        ``pos_sum`` / ``pos_sumsq`` (float64 ``[n_chain_local, dim]``, both required) the sums over the steps of every chain's position
        after accept / reject and of its square: what a window of a mass-matrix adaptation needs in place of a trajectory."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        self._warmup_sizes(n_steps, step_avg, step_last, n_acc, acc_sum, step_traj)
        for name, t_ in (("pos_sum", pos_sum), ("pos_sumsq", pos_sumsq)):
            if t_ is not None and t_.numel() < self.n_local * self.dim:
                raise MfmError(f"{name} must hold n_chain_local * dim = {self.n_local * self.dim} elements (got {t_.numel()})")
        _chk(self.lib.mfm_hmc_warmup_window(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step0),
                                            int(num_steps), int(n_steps), float(target_accept), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                            _ptr(step_avg, F64), _ptr(step_last, F64), _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(step_traj, F64),
                                            _ptr(pos_sum, F64), _ptr(pos_sumsq, F64)))

    def mala_warmup(self, key, beta, step0, n_steps, target_accept, pos, logp, grad, step_avg, step_last=None, n_acc=None,
                    acc_sum=None, step_traj=None, textbook=True, key_mode=None):
        """``mfm_mala_warmup``: the same for the MALA step under the TEXTBOOK acceptance rule (``textbook=False`` is refused by the
        library: the as-written rule's acceptance does not fall as the step grows)."""
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        self._warmup_sizes(n_steps, step_avg, step_last, n_acc, acc_sum, step_traj)
        _chk(self.lib.mfm_mala_warmup(self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step0),
                                      int(textbook), int(n_steps), float(target_accept), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                      _ptr(step_avg, F64), _ptr(step_last, F64), _ptr(n_acc, I32), _ptr(acc_sum, F64), _ptr(step_traj, F64)))

    def _nuts_warmup_args(self, key, beta, step0, max_tree_depth, n_steps, target_accept, pos, logp, grad, step_avg, divergence_threshold,
                          step_last, acc_sum, step_traj, leapfrog_sum, n_divergent, depth_sum, key_mode):
        per_chain = getattr(key, "ndim", 1) == 2
        mode = int(per_chain) if key_mode is None else int(key_mode)
        k0, k1 = (0, 0) if per_chain or key is None else (int(key[0]), int(key[1]))
        self._warmup_sizes(n_steps, step_avg, step_last, None, acc_sum, step_traj)
        for name, t_ in (("leapfrog_sum", leapfrog_sum), ("n_divergent", n_divergent), ("depth_sum", depth_sum)):
            if t_ is not None and t_.numel() < self.n_local:
                raise MfmError(f"{name} must hold n_chain_local = {self.n_local} elements (got {t_.numel()})")
        return (self.h, mode, k0, k1, _ptr(key, I32) if per_chain else None, float(beta), float(step0), int(max_tree_depth),
                float(divergence_threshold), int(n_steps), float(target_accept), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                _ptr(step_avg, F64), _ptr(step_last, F64), _ptr(acc_sum, F64), _ptr(step_traj, F64),
                _ptr(leapfrog_sum, I64), _ptr(n_divergent, I32), _ptr(depth_sum, I32))

    def nuts_warmup(self, key, beta, step0, max_tree_depth, n_steps, target_accept, pos, logp, grad, step_avg, divergence_threshold=1000.0,
                    step_last=None, acc_sum=None, step_traj=None, leapfrog_sum=None, n_divergent=None, depth_sum=None, key_mode=None):
        """``mfm_nuts_warmup``: ``n_steps`` No-U-turn transitions in one launch, every chain adapting its own step size from ``step0`` by
        the dual averaging of ``hmc_warmup`` on its tree's acceptance statistic (the mean over the leaves of ``min(1, exp(H0 - H))``);
        state updated in place.  ``key`` / ``key_mode`` as ``nuts_run``'s.  ``step_avg`` (float64 ``[n_chain_local]``, required) takes the
        averaged step size, the result; ``step_last`` the last iterate; ``step_traj`` (float64 ``[n_steps, n_chain_local]``) the step
        size used at every transition; ``acc_sum`` float64 the sum of the statistics; ``leapfrog_sum`` int64, ``n_divergent`` /
        ``depth_sum`` int32 as ``nuts_run``'s."""
        _chk(self.lib.mfm_nuts_warmup(*self._nuts_warmup_args(key, beta, step0, max_tree_depth, n_steps, target_accept, pos, logp, grad, step_avg,
                                                              divergence_threshold, step_last, acc_sum, step_traj, leapfrog_sum, n_divergent,
                                                              depth_sum, key_mode)))

    def nuts_warmup_window(self, key, beta, step0, max_tree_depth, n_steps, target_accept, pos, logp, grad, step_avg, pos_sum, pos_sumsq,
                           divergence_threshold=1000.0, step_last=None, acc_sum=None, step_traj=None, leapfrog_sum=None, n_divergent=None,
                           depth_sum=None, key_mode=None):
        """``mfm_nuts_warmup_window``: ``nuts_warmup`` on the mass instances (the installed vector, or ones), which also leaves in
        ``pos_sum`` / ``pos_sumsq`` (float64 ``[n_chain_local, dim]``, both required) the sums over the transitions of every chain's
        position and of its square, as ``hmc_warmup_window`` does."""
        args = self._nuts_warmup_args(key, beta, step0, max_tree_depth, n_steps, target_accept, pos, logp, grad, step_avg, divergence_threshold,
                                      step_last, acc_sum, step_traj, leapfrog_sum, n_divergent, depth_sum, key_mode)
        for name, t_ in (("pos_sum", pos_sum), ("pos_sumsq", pos_sumsq)):
            if t_ is not None and t_.numel() < self.n_local * self.dim:
                raise MfmError(f"{name} must hold n_chain_local * dim = {self.n_local * self.dim} elements (got {t_.numel()})")
        _chk(self.lib.mfm_nuts_warmup_window(*args, _ptr(pos_sum, F64), _ptr(pos_sumsq, F64)))

    def loglik(self, pos, out):
        _chk(self.lib.mfm_loglik(self.h, _ptr(pos, F32), _ptr(out, F64)))

    # ---- adaptive tempered SMC pieces (bblackjax/smc) -----------------------------------------------------------
    def smc_delta(self, logliks, target_ess, max_delta):
        out = C.c_double()
        _chk(self.lib.mfm_smc_delta(self.h, _ptr(logliks, F64), logliks.shape[0], float(target_ess), float(max_delta), C.byref(out)))
        return out.value

    def smc_weights(self, logliks, delta, weights):
        out = C.c_double()
        _chk(self.lib.mfm_smc_weights(self.h, _ptr(logliks, F64), logliks.shape[0], float(delta), _ptr(weights, F64), C.byref(out)))
        return out.value

    def smc_resample(self, key, weights, scratch, idx):
        _chk(self.lib.mfm_smc_resample(self.h, int(key[0]), int(key[1]), _ptr(weights, F64), weights.shape[0], _ptr(scratch, F64), _ptr(idx, I32)))

    def choice_logw(self, key, logw, m, scratch, idx):
        """idx[j] = jax.random.choice(key, n, (m,), p=exp(logw - max logw))[j] (``exe_flow_matching.py:458-459``)."""
        _chk(self.lib.mfm_choice_logw(self.h, int(key[0]), int(key[1]), _ptr(logw, F64), logw.shape[0], int(m), _ptr(scratch, F64), _ptr(idx, I32)))

    def acc_stats(self, x, out):
        """out[0:2] (float64) = sum, sum of squares of the float32 vector x."""
        _chk(self.lib.mfm_acc_stats(self.h, _ptr(x, F32), x.shape[0], _ptr(out, F64)))

    def smc_resample_scheme(self, scheme, key, weights, scratch, idx):
        """scheme: 0 systematic, 1 stratified, 2 multinomial (resampling.py); scratch: 2 n + 2 float64."""
        _chk(self.lib.mfm_smc_resample_scheme(self.h, int(scheme), int(key[0]), int(key[1]), _ptr(weights, F64), weights.shape[0],
                                              _ptr(scratch, F64), _ptr(idx, I32)))

    def gather_rows(self, src, idx, dst):
        """dst[r] = src[idx[r]] for the ``idx.shape[0]`` rows of ``dst`` (``src`` may hold more rows: the all-gathered particles of a sharded SMC step)."""
        _chk(self.lib.mfm_gather_rows(self.h, _ptr(src, F32), _ptr(idx, I32), idx.shape[0], src.shape[1], _ptr(dst, F32)))

    def fm_loss_grad(self, key, pos, loss, grads):
        self._p()
        _chk(self.lib.mfm_fm_loss_grad(self.h, int(key[0]), int(key[1]), _ptr(pos, F32), _ptr(loss, F64), _ptr(grads, F32)))

    def fm_loss(self, key, samples, loss, n_total=None, offset=0):
        self._p()
        n = samples.shape[0]
        _chk(self.lib.mfm_fm_loss(self.h, int(key[0]), int(key[1]), _ptr(samples, F32), n, n if n_total is None else n_total,
                                  offset, _ptr(loss, F64)))

    def fm_eval_instance(self, n):
        """The kernel instance an ``fm_loss`` call of ``n`` samples runs (``mfm_fm_eval_instance``; no launch): 0 for the 16-row tile,
        else rows per workgroup (32 / 64) | ``EVAL_RELU`` | ``EVAL_CHAIN`` | ``EVAL_BCRT``."""
        rc = self.lib.mfm_fm_eval_instance(self.h, int(n))
        if rc < 0:
            _chk(rc)
        return rc

    def wgrad_info(self):
        """The weight-gradient kernel this context launches (``mfm_wgrad_info``; no launch): ``dict(kind, n_jobs, nbb, G, q, r)``,
        ``kind`` one of ``WGRAD_SLABS`` / ``WGRAD_STREAM_K`` / ``WGRAD_WIDE``."""
        out = (C.c_int32 * 6)()
        _chk(self.lib.mfm_wgrad_info(self.h, out))
        return dict(zip(("kind", "n_jobs", "nbb", "G", "q", "r"), [int(v) for v in out]))

    def wide_gemm_tally(self, reset=False):
        """Launches of each wide-family GEMM instance by this context since its creation or last reset (``mfm_wide_gemm_tally``;
        counted on the host): ``{name from WGEMM: launches}``."""
        out = (C.c_int64 * len(WGEMM))()
        _chk(self.lib.mfm_wide_gemm_tally(self.h, out, int(bool(reset))))
        return dict(zip(WGEMM, [int(v) for v in out]))

    def adamw_step(self, grads):
        self._p()
        _chk(self.lib.mfm_adamw_step(self.h, _ptr(grads, F32)))

    # ---- context-owned RCCL communicator (include/mfm.h: mfm_comm_*) ---------------------------------------------
    def comm_unique_id(self):
        """128 bytes from ncclGetUniqueId (rank 0; ship them to the other ranks out of band)."""
        buf = (C.c_uint8 * 128)()
        _chk(self.lib.mfm_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, unique_id):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _chk(self.lib.mfm_comm_init(self.h, int(nranks), int(rank), buf))
        self.has_comm = True

    def comm_destroy(self):
        _chk(self.lib.mfm_comm_destroy(self.h))
        self.has_comm = False

    def comm_count(self):
        """Ranks of the context's communicator as RCCL reports them (ncclCommCount); 0 without one."""
        n = C.c_int32(0)
        _chk(self.lib.mfm_comm_count(self.h, C.byref(n)))
        return int(n.value)

    def grad_allreduce_begin(self, grads):
        """Asynchronous SUM all-reduce of the gradient on the context's communication stream; the next adamw_step(grads) waits."""
        _chk(self.lib.mfm_grad_allreduce_begin(self.h, _ptr(grads, F32)))

    def opt_state(self):
        self._p()
        out = (C.c_int32 * 4)()
        lr = C.c_float()
        _chk(self.lib.mfm_opt_state(self.h, out, C.byref(lr)))
        return dict(step=out[0], count=out[1], notfinite_count=out[2], last_applied=out[3], last_lr=lr.value)

    def vf_apply(self, x, t, v, tangent=None, jvp=None):
        self._p()
        _chk(self.lib.mfm_vf_apply(self.h, _ptr(x, F32), _ptr(t, F32), _ptr(tangent, F32), x.shape[0], _ptr(v, F32), _ptr(jvp, F32)))

    def ode_transform(self, direction, x, out, ldj, keys=None, key=(0, 0), nsteps=None):
        self._p()
        _chk(self.lib.mfm_ode_transform(self.h, direction, 0 if keys is None else 1, _ptr(keys, I32), int(key[0]), int(key[1]),
                                        _ptr(x, F32), x.shape[0], _ptr(out, F32), _ptr(ldj, F32), _ptr(nsteps, I32)))

    def flow_step(self, mode, key, beta, pos, logp, grad, acc=None, is_acc=None, proposed=None, nsteps=None):
        self._p()
        _chk(self.lib.mfm_flow_step(self.h, mode, int(key[0]), int(key[1]), float(beta), _ptr(pos, F32), _ptr(logp, F64), _ptr(grad, F32),
                                    _ptr(acc, F32), _ptr(is_acc, U8), _ptr(proposed, F32), _ptr(nsteps, I32)))

    def train_iter(self, count, mcmc_per_flow_steps, flow_mode, key_gen, key_train, beta, step_size, pos, logp, grad, loss, grads,
                   acc=None, nsteps=None, apply_update=True):
        """One loop iteration (exe_flow_matching.py:432-439): generator (flow-MH step when ``count % (K+1) == 0``, MALA step
        otherwise) + train_step on the new positions, in one library call."""
        self._p()
        _chk(self.lib.mfm_train_iter(self.h, int(count), int(mcmc_per_flow_steps), int(flow_mode), int(key_gen[0]), int(key_gen[1]),
                                     int(key_train[0]), int(key_train[1]), float(beta), float(step_size), _ptr(pos, F32), _ptr(logp, F64),
                                     _ptr(grad, F32), _ptr(acc, F32), _ptr(nsteps, I32), _ptr(loss, F64), _ptr(grads, F32),
                                     1 if apply_update else 0))

    def noise_prefetch(self, keys_gn, keys_step):
        """Produce the draws of the iterations keyed ``keys_gn[j]`` (MALA step) / ``keys_step[j]`` (training batch) on the side
        stream; returns False where the configuration is not served (the kernels then draw in line as always)."""
        kg = np.ascontiguousarray(keys_gn, dtype=np.uint32).reshape(-1, 2)
        ks = np.ascontiguousarray(keys_step, dtype=np.uint32).reshape(-1, 2)
        assert kg.shape == ks.shape
        if kg.shape[0] == 0:
            return False
        rc = self.lib.mfm_noise_prefetch(self.h, kg.shape[0], kg.ctypes.data_as(C.POINTER(_U32)), ks.ctypes.data_as(C.POINTER(_U32)))
        if rc == -2:            # MFM_EUNSUPPORTED
            return False
        _chk(rc)
        return True

    def noise_drop(self):
        _chk(self.lib.mfm_noise_drop(self.h))

    COUNTERS = ("mala_chain_steps", "fm_train_samples", "fm_eval_samples", "ode_solves", "dopri_attempts", "field_evals",
                "optimizer_steps", "mala_hbm_bytes")

    def counters(self):
        """Algorithmic work done through this context since creation / ``reset_counters`` (``mfm_get_counters``)."""
        out = (C.c_int64 * 8)()
        _chk(self.lib.mfm_get_counters(self.h, out))
        return dict(zip(self.COUNTERS, [int(v) for v in out]))

    def reset_counters(self):
        _chk(self.lib.mfm_reset_counters(self.h))

    def debug_replay(self, dt, acc, ratio, dt_own, diag=None):
        """Arm the next ``ode_transform`` / ``flow_step`` with a prescribed step sequence (parity instrumentation,
        ``mfm_debug_replay``): float32 ``dt``, uint8 ``acc``, float32 outputs ``ratio`` / ``dt_own``, all CUDA tensors of shape
        [n, cap] (transform) or [2, n, cap] (flow step)."""
        cap = dt.shape[-1]
        for t_ in (acc, ratio, dt_own):
            assert t_.shape == dt.shape
        self._replay_keep = (dt, acc, ratio, dt_own, diag)      # the library holds raw pointers until the armed call has run
        _chk(self.lib.mfm_debug_replay(self.h, cap, _ptr(dt, F32), _ptr(acc, U8), _ptr(ratio, F32), _ptr(dt_own, F32), _ptr(diag, F64)))

    PROF_CLASSES = ("mala_step", "fm_fwd_bwd", "wgrad", "adamw", "flow_step", "fm_eval", "reduce", "_")

    def profile(self, enable=True, classes=None):
        """HIP-event timing of the kernel classes named in ``classes`` (default: all) on the context's stream."""
        mask = 0 if not enable else (-1 if classes is None else sum(1 << self.PROF_CLASSES.index(c) for c in classes))
        _chk(self.lib.mfm_profile(self.h, mask))

    def profile_read(self):
        ms, cnt = (C.c_double * 8)(), (C.c_int64 * 8)()
        _chk(self.lib.mfm_profile_read(self.h, ms, cnt))
        return {n: dict(ms=ms[i], launches=cnt[i]) for i, n in enumerate(self.PROF_CLASSES) if cnt[i]}

    def normal_rows(self, keys, out):
        """out[i] = normal(keys[i], (dim,)); keys: int32 CUDA tensor [n, 2] holding uint32 bit patterns."""
        _chk(self.lib.mfm_normal_rows(self.h, _ptr(keys, I32), out.shape[0], _ptr(out, F32)))

    def cis_select(self, key, n_is, u0, vol0, refs, xs, vols, lps, pos, logp, acc=None, is_acc=None, proposed=None, weight=None):
        _chk(self.lib.mfm_cis_select(self.h, int(key[0]), int(key[1]), int(n_is), _ptr(u0, F32), _ptr(vol0, F32), _ptr(refs, F32),
                                     _ptr(xs, F32), _ptr(vols, F32), _ptr(lps, F64), _ptr(pos, F32), _ptr(logp, F64), _ptr(acc, F32),
                                     _ptr(is_acc, U8), _ptr(proposed, F32), _ptr(weight, F32)))

    def stein_disc(self, x, grad, beta=-0.5):
        """(U, V) statistics of ``mcmc_utils.py:28-85`` for CUDA samples x [n, d] and grad log p at x."""
        out = (C.c_double * 2)()
        _chk(self.lib.mfm_stein_disc(self.h, _ptr(x, F32), _ptr(grad, F32), x.shape[0], float(beta), out))
        return out[0], out[1]

    def max_mean_disc(self, x, y):
        """``mcmc_utils.py:88-111`` for CUDA sample sets x, y [m, d]."""
        if x.shape != y.shape:
            raise ValueError("max_mean_disc: both sample sets must have the same shape (the reference uses m = X.shape[0] for both)")
        out = C.c_double()
        _chk(self.lib.mfm_max_mean_disc(self.h, _ptr(x, F32), _ptr(y, F32), x.shape[0], C.byref(out)))
        return out.value

    def autocorr(self, x, n_lags=None, rho=None, tau=None, ess=None, mean=None, var=None):
        """``mfm_autocorr`` on the float32 CUDA trajectory ``x [n, ...]`` (time-major: every trailing index is one series).  Outputs
        (any subset, CUDA tensors): ``rho`` float32 ``[n_lags, n_series]`` (``rho[0] = 1``), ``tau`` / ``ess`` float32 ``[n_series]``
        (Geyer's initial positive sequence over the first ``n_lags`` lags), ``mean`` / ``var`` float64 ``[n_series]``.  Asynchronous on
        the context's stream."""
        n = int(x.shape[0]) if x.ndim else 0
        n_series = int(x.numel() // n) if n else 0
        _chk(self.lib.mfm_autocorr(self.h, _ptr(x, F32), n, n_series, int(n if n_lags is None else n_lags), _ptr(rho, F32), _ptr(tau, F32),
                                   _ptr(ess, F32), _ptr(mean, F64), _ptr(var, F64)))

    def chain_sums(self, x, sums, n_chain=None, split=True, chain_offset=0):
        """``mfm_chain_sums`` on the float32 CUDA trajectory ``x [n, n_chain_ld, dim]`` (time-major, contiguous): the sums over the
        sub-chains of chains ``chain_offset .. chain_offset + n_chain - 1`` (default: all from the offset on) into ``sums``, a float64
        CUDA tensor ``[n_lags + 2, dim]`` whose first extent sets ``n_lags``.  Rows: sum of the sub-chain means, of their squares, of the
        lag sums ``A_0 .. A_{n_lags-1}``; additive over disjoint sets of chains.  ``split``: both halves of every chain are sub-chains.
        Returns ``(n_sub, n_subchains)``.  Asynchronous on the context's stream."""
        if x.ndim != 3:
            raise MfmError(f"chain_sums: expected a trajectory [n, n_chain, dim], got {tuple(x.shape)}")
        if sums.ndim != 2 or sums.shape[0] < 3 or sums.shape[1] != x.shape[2]:
            raise MfmError(f"chain_sums: sums must be [n_lags + 2, dim = {x.shape[2]}] with n_lags >= 1, got {tuple(sums.shape)}")
        n, ld, dim = (int(v) for v in x.shape)
        off = int(chain_offset)
        if not 0 <= off < max(ld, 1):
            raise MfmError(f"chain_sums: chain_offset must be in [0, {ld}) (got {off})")
        n_chain = ld - off if n_chain is None else int(n_chain)
        if off + n_chain > ld:                                       # (n_chain < 1 is the library's to refuse)
            raise MfmError(f"chain_sums: chain_offset + n_chain = {off + n_chain} exceeds the {ld} chains of a row")
        px = C.c_void_p((_ptr(x, F32).value or 0) + 4 * off * dim)         # (the row stride stays n_chain_ld * dim)
        _chk(self.lib.mfm_chain_sums(self.h, px, n, n_chain, ld, dim, int(bool(split)), int(sums.shape[0]) - 2, _ptr(sums, F64)))
        return (n // 2, 2 * n_chain) if split else (n, n_chain)

    def chain_diag(self, sums, n_sub, n_subchains, rhat=None, ess=None, tau=None, rho=None):
        """``mfm_chain_diag``: split-R-hat, multi-chain effective sample size and integrated autocorrelation time (float32 CUDA tensors
        ``[dim]``) and optionally ``rho [n_lags, dim]`` from ``sums [n_lags + 2, dim]`` (float64, summed over the chains of every rank),
        the sub-chain length ``n_sub`` and the TOTAL number of sub-chains.  Any subset of outputs, not none."""
        if sums.ndim != 2 or sums.shape[0] < 3:
            raise MfmError(f"chain_diag: sums must be [n_lags + 2, dim] with n_lags >= 1, got {tuple(sums.shape)}")
        n_lags, dim = int(sums.shape[0]) - 2, int(sums.shape[1])
        for name, t_, want in (("rhat", rhat, (dim,)), ("ess", ess, (dim,)), ("tau", tau, (dim,)), ("rho", rho, (n_lags, dim))):
            if t_ is not None and tuple(t_.shape) != want:
                raise MfmError(f"chain_diag: {name} must have shape {want}, got {tuple(t_.shape)}")
        _chk(self.lib.mfm_chain_diag(self.h, _ptr(sums, F64), int(n_sub), int(n_subchains), dim, n_lags, _ptr(rhat, F32), _ptr(ess, F32),
                                     _ptr(tau, F32), _ptr(rho, F32)))

    # ---- Stein variational gradient descent (include/mfm.h: mfm_svgd_*) -------------------------------------------------------------
    def svgd_sqdist(self, x, D):
        """``D [n, n]`` float32 = squared distances of the float32 CUDA particles ``x [n, d]`` (any n >= 2, d >= 1)."""
        _chk(self.lib.mfm_svgd_sqdist(self.h, _ptr(x, F32), int(x.shape[0]), int(x.shape[1]), _ptr(D, F32)))

    def svgd_median(self, D, length_scale):
        """``length_scale`` (float64 CUDA tensor of one element) = median heuristic of the strict lower triangle of ``D [n, n]``."""
        _chk(self.lib.mfm_svgd_median(self.h, _ptr(D, F32), int(D.shape[0]), _ptr(length_scale, F64)))

    def svgd_gradient(self, x, g, D, length_scale, fg, i0=0, n_rows=None):
        """``fg [n_rows, d]`` = rows ``[i0, i0 + n_rows)`` (default: all) of the functional gradient of ``x, g [n, d]`` under ``D`` and the
        device scalar ``length_scale``."""
        n = int(x.shape[0])
        _chk(self.lib.mfm_svgd_gradient(self.h, _ptr(x, F32), _ptr(g, F32), _ptr(D, F32), _ptr(length_scale, F64), n, int(x.shape[1]),
                                        int(i0), int(n - int(i0) if n_rows is None else n_rows), _ptr(fg, F32)))

    @staticmethod
    def _svgd_opt(kind, hyper, state):
        if kind not in SVGD_OPTIMIZERS:
            raise MfmError(f"svgd: unknown optimizer kind {kind!r} (one of {', '.join(SVGD_OPTIMIZERS)})")
        hp = (C.c_double * 4)(*([float(v) for v in hyper] + [0.0] * 4)[:4])
        st = [_ptr(t, F32) for t in state] + [None] * 5
        return SVGD_OPTIMIZERS[kind], hp, st[:5]

    def svgd_apply(self, kind, hyper, count, x, fg, state=()):
        """One optimizer update of ``x [n, d]`` in place from ``fg``; ``state``: the kind's float32 arrays ``[n, d]``, updated in place;
        ``count``: updates already applied."""
        k, hp, st = self._svgd_opt(kind, hyper, state)
        _chk(self.lib.mfm_svgd_apply(self.h, k, hp, int(count), int(x.shape[0]), int(x.shape[1]), _ptr(x, F32), _ptr(fg, F32), *st))

    def svgd_step(self, beta, kind, hyper, count, n_iter, x, state, length_scale, update_median=True, ls_used=None):
        """``n_iter`` SVGD iterations in place on the ``n_chain_valid`` particles of ``x [n_chain_local, dim]``; ``length_scale``: float64
        CUDA tensor of one element (in / out); ``ls_used``: optional float64 ``[n_iter]``, the scale every iteration used."""
        k, hp, st = self._svgd_opt(kind, hyper, state)
        _chk(self.lib.mfm_svgd_step(self.h, float(beta), k, hp, int(count), int(n_iter), int(bool(update_median)), _ptr(x, F32), *st,
                                    _ptr(length_scale, F64), _ptr(ls_used, F64)))

    def beta_update(self, prev_beta, logliks, alpha):
        out = C.c_double()
        _chk(self.lib.mfm_beta_update(self.h, float(prev_beta), _ptr(logliks, F64), logliks.numel(), float(alpha), C.byref(out)))
        return out.value
