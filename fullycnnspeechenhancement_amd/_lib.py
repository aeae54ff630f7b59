"""ctypes binding of librced_hip.so (C ABI: include/rced.h).

The library is the product; there is NO CPU fallback.  If the .so is missing this module raises
at load() time -- build it with `python __graft_entry__.py` (or `make -C fullycnnspeechenhancement_amd/csrc`).
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RCED_LIB: A/B experiments only (an alternative build of the same ABI); the product is librced_hip.so
SO_PATH = os.environ.get("RCED_LIB") or os.path.join(_HERE, "librced_hip.so")

RCED_OK, RCED_ERR_ARG, RCED_ERR_HIP, RCED_ERR_ALLOC, RCED_ERR_STATE = 0, 1, 2, 3, 4
PATH_AUTO, PATH_LAYERWISE, PATH_FUSED = 0, 1, 2
K_GENERIC, K_FUSED, K_FINAL = 0, 1, 2
PCM_S16, PCM_F32 = 0, 1
STOI_CLASSIC, STOI_EXTENDED = 1, 2

# every symbol include/rced.h declares: (restype, argtypes)
_c_float_p = ctypes.POINTER(ctypes.c_float)
_c_int_p = ctypes.POINTER(ctypes.c_int)
_vp = ctypes.c_void_p
SYMBOLS = {
    "rced_num_layers": (ctypes.c_int, [ctypes.c_int]),
    "rced_num_weights": (ctypes.c_size_t, [ctypes.c_int]),
    "rced_num_trainable": (ctypes.c_size_t, [ctypes.c_int]),
    "rced_layer_desc": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _c_int_p]),
    "rced_layer_scope": (ctypes.c_char_p, [ctypes.c_int, ctypes.c_int]),
    "rced_create": (ctypes.c_int, [ctypes.c_int, _c_float_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_vp)]),
    "rced_destroy": (None, [_vp]),
    "rced_forward": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "rced_check": (ctypes.c_int, [_vp]),
    "rced_forward_host": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int]),
    "rced_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "rced_set_option": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int]),
    "rced_get_option": (ctypes.c_int, [_vp, ctypes.c_char_p, _c_int_p]),
    "rced_conv_bn_relu": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp] + [ctypes.c_int] * 9 + [_vp]),
    "rced_conv_bn_relu_train": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp] + [ctypes.c_int] * 8 + [_vp, ctypes.c_int, _vp]),
    "rced_stft_num_frames": (ctypes.c_int, [ctypes.c_int]),
    "rced_stft": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp]),
    "rced_istft": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp]),
    "rced_stft_ex": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int]),
    "rced_istft_ex": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int]),
    "rced_istft_ola": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp]),
    "rced_wave_loss": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_int, ctypes.c_double, _vp, _vp, ctypes.c_int, _vp]),
    "rced_wave_loss_fr": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _vp] + [ctypes.c_int] * 5 + [ctypes.c_double, ctypes.c_double,
                                         ctypes.c_int, ctypes.c_double, _vp, _vp, ctypes.c_int, _vp]),
    "rced_mr_stft_check": (ctypes.c_int, [_vp]),
    "rced_mr_stft": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_double, _vp, _vp, ctypes.c_int, _vp]),
    "rced_wave_loss_mr": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _vp] + [ctypes.c_int] * 5 + [ctypes.c_double, ctypes.c_double,
                                         ctypes.c_int, ctypes.c_double, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "rced_framing_check": (ctypes.c_int, [ctypes.c_int] * 3),
    "rced_stft_num_frames_fr": (ctypes.c_int, [ctypes.c_int] * 3),
    "rced_stft_fr": (ctypes.c_int, [_vp, _vp] + [ctypes.c_int] * 6 + [_vp, _vp, ctypes.c_int, _vp]),
    "rced_istft_fr": (ctypes.c_int, [_vp, _vp] + [ctypes.c_int] * 5 + [_vp, ctypes.c_int, _vp]),
    "rced_istft_fr_check": (ctypes.c_int, [ctypes.c_int] * 3),
    "rced_istft_ola_fr": (ctypes.c_int, [_vp, _vp, _vp] + [ctypes.c_int] * 5 + [_vp, ctypes.c_int, _vp]),
    "rced_sdr": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp]),
    "rced_stoi": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp]),
    "rced_stoi_ex": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
                                    ctypes.c_int, _vp]),
    "rced_si_sdr": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp]),
    "rced_seg_snr": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp]),
    "rced_llr": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, _vp,
                                ctypes.c_int, _vp, ctypes.c_int, _vp]),
    "rced_wss": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp,
                                ctypes.c_int, _vp]),
    "rced_fwseg": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp,
                                  ctypes.c_int, _vp]),
    "rced_cepd": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp,
                                 ctypes.c_int, _vp, ctypes.c_int, _vp]),
    "rced_bss_sdr": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "rced_mix_snr": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int,
                                    ctypes.c_double, _vp, ctypes.c_int, _vp]),
    "rced_gather_pcm": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_longlong, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                       ctypes.c_int, _vp]),
    "rced_convolve": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                     ctypes.c_int, _vp]),
    "rced_resample_length": (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]),
    "rced_resample_taps": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _c_int_p, _c_int_p, _c_int_p, _c_int_p,
                                          ctypes.POINTER(ctypes.c_double), ctypes.c_size_t]),
    "rced_resample": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, _vp, _vp, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    "rced_stream_delay":(ctypes.c_int, []),
    "rced_stream_create": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "rced_stream_create_ex": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "rced_stream_fr_check": (ctypes.c_int, [ctypes.c_int] * 4),
    "rced_stream_delay_fr": (ctypes.c_int, [ctypes.c_int] * 2),
    "rced_stream_finish_max_fr": (ctypes.c_int, [ctypes.c_int] * 2),
    "rced_stream_create_fr": (ctypes.c_int, [_vp] + [ctypes.c_int] * 7 + [ctypes.POINTER(_vp)]),
    "rced_stream_destroy": (None, [_vp]),
    "rced_stream_push": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp]),
    "rced_stream_finish": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rced_stream_reset": (ctypes.c_int, [_vp, ctypes.c_int]),
    "rced_rstream_create": (ctypes.c_int, [ctypes.c_int] * 10 + [ctypes.POINTER(_vp)]),
    "rced_rstream_create_ex": (ctypes.c_int, [ctypes.c_int] * 11 + [ctypes.POINTER(_vp)]),
    "rced_rstream_destroy": (None, [_vp]),
    "rced_rstream_started": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "rced_rstream_delay": (ctypes.c_int, [_vp]),
    "rced_rstream_push": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp]),
    "rced_rstream_finish": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rced_rstream_reset": (ctypes.c_int, [_vp, ctypes.c_int]),
    "rced_rfree_available": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]),
    "rced_rfree_plan": (ctypes.c_int, [ctypes.c_int] * 7 + [_c_int_p] * 4),
    "rced_rfree_create": (ctypes.c_int, [ctypes.c_int] * 10 + [ctypes.POINTER(_vp)]),
    "rced_rfree_destroy": (None, [_vp]),
    "rced_rfree_push": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp]),
    "rced_rfree_finish": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "rced_rfree_reset": (ctypes.c_int, [_vp, ctypes.c_int]),
    "rced_train_create": (ctypes.c_int, [ctypes.c_int, _c_float_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(_vp)]),
    "rced_train_destroy": (None, [_vp]),
    "rced_train_step": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                       ctypes.POINTER(ctypes.c_double), _vp]),
    "rced_train_forward": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "rced_train_exchange_size": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    "rced_train_grad": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_double), _vp]),
    "rced_train_step_wave": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, _vp,
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _vp]),
    "rced_train_grad_wave": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp,
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _vp]),
    "rced_train_step_wave_fr": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, _vp] + [ctypes.c_int] * 3 +
                                [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _vp]),
    "rced_train_grad_wave_fr": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp] + [ctypes.c_int] * 3 +
                                [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _vp]),
    "rced_train_step_wave_mr": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, _vp] + [ctypes.c_int] * 3 +
                                [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _vp]),
    "rced_train_grad_wave_mr": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp] + [ctypes.c_int] * 3 +
                                [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _vp]),
    "rced_train_apply": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_float, _vp]),
    "rced_train_sync_points": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]),
    "rced_train_sync_begin": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, _vp]),
    "rced_train_sync_next": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "rced_train_sync_end": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    "rced_train_sync_abort": (ctypes.c_int, [_vp]),
    "rced_train_sync_reduce": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_size_t, _vp, _vp]),
    "rced_train_copy_variables": (ctypes.c_int, [_vp, _vp, _vp]),
    "rced_train_global_step": (ctypes.c_longlong, [_vp]),
    "rced_train_grid_stats": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "rced_train_get_variables": (ctypes.c_int, [_vp, _c_float_p, ctypes.c_size_t]),
    "rced_train_get_gradients": (ctypes.c_int, [_vp, _c_float_p, ctypes.c_size_t]),
    "rced_train_get_state": (ctypes.c_int, [_vp, _c_float_p, _c_float_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_longlong)]),
    "rced_train_set_state": (ctypes.c_int, [_vp, _c_float_p, _c_float_p, ctypes.c_size_t, ctypes.c_longlong]),
    "rced_last_kernel_ms": (ctypes.c_float, [_vp]),
    "rced_profile_query": (ctypes.c_int, [_vp, ctypes.c_int, _c_float_p, _c_int_p]),
    "rced_last_error": (ctypes.c_char_p, []),
    "rced_version": (ctypes.c_char_p, []),
}

_lib = None


class WaveArgs(ctypes.Structure):
    """rced.h: rced_wave_args."""
    _fields_ = [("w_spectral", ctypes.c_double), ("w_sse", ctypes.c_double), ("w_si_sdr", ctypes.c_double), ("skip_edges", ctypes.c_int),
                ("phase_dev", _vp), ("clean_dev", _vp), ("clean_stride", ctypes.c_int), ("lengths_dev", _vp), ("frames_dev", _vp)]


class MrArgs(ctypes.Structure):
    """rced.h: rced_mr_args."""
    _fields_ = [("w_mr", ctypes.c_double), ("n_res", ctypes.c_int), ("window", ctypes.c_int * 4), ("stride", ctypes.c_int * 4),
                ("window_name", ctypes.c_int * 4)]


class RcedError(RuntimeError):
    """Raised for every non-zero status from the C ABI (mirrors TF raising from sess.run)."""

    def __init__(self, code, msg):
        super().__init__("rced error %d: %s" % (code, msg))
        self.code = code


def load():
    """Load librced_hip.so.  Import torch first when both live in one process, so that the
    one HIP runtime torch ships (same soname, libamdhip64.so.7) is the one we bind to."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            "%s not found: the HIP extension is not built (run `python __graft_entry__.py`). "
            "There is no CPU fallback for the R-CED forward pass." % SO_PATH)
    try:
        import torch  # noqa: F401  (binds torch's bundled libamdhip64 first)
    except Exception:  # pragma: no cover - torch-less use of the C ABI is fine
        pass
    lib = ctypes.CDLL(SO_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != RCED_OK:
        raise RcedError(rc, load().rced_last_error().decode())


def version():
    return load().rced_version().decode()
