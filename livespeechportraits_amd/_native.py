"""ctypes binding of liblspf2f.so (include/lspf2f.h, include/lspa2h.h, include/lsplle.h, include/lsprnn.h, include/lspraster.h, include/lspmel.h, include/lspunet.h, include/lspjpeg.h, include/lspjpegdec.h, include/lsppng.h, include/lsppngenc.h, include/lsplmk.h, include/lspavi.h, include/lsprs.h, include/lspresize.h).

There is deliberately no fallback: if the shared library is missing or does not
load, importing the hot path raises -- a GPU box must never silently run
something else (see DESIGN.md "No CPU path").
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t,
                    c_uint32, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblspf2f.so")
ABI_VERSION = 1

OK = 0
ERR_NAMES = {
    -1: "INVALID_ARGUMENT", -2: "UNSUPPORTED", -3: "MISSING_TENSOR", -4: "SHAPE",
    -5: "STATE", -6: "HIP", -7: "NO_DEVICE",
}
VARIANT_IDS = {"normal": 0, "large": 1}
DTYPE_IDS = {"f32": 0, "bf16": 1, "f16": 2}
FORM_IDS = {"rows": 0, "fullk": 1, "fullk2": 2, "wino": 3, "wino4": 4, "winoup": 5, "rowup": 6, "band": 7, "row": 8, "gemm_last": 9, "rowlast": 10}
FLAG_KEEP_INTERMEDIATES = 1
FLAG_NO_GRAPH = 2
FLAG_INSTANCE_NORM = 4
FLAG_WINO4 = 8
NORM_IDS = {"batch": 0, "instance": 1}


class NativeLibraryError(RuntimeError):
    pass


# ---- switches of tools, tests and A-B runs.  The LIBRARY never reads the process environment: the switches travel as the `tune` string of
# lspf2f_create_tuned ("key=value,..."; include/lspf2f.h lists the keys).  For shell-driven A-B scripts (tools/*.sh) the Python host maps
# LSP_HIP_<KEY>=<int> environment variables onto those keys HERE, once per Engine; an explicit `tune=` argument wins.
_PRESENCE_ENV = {   # legacy names whose mere presence is the switch
    "LSP_HIP_LASTCONV_DIRECT": ("lastconv_direct", 1), "LSP_HIP_LASTCONV_STRIP": ("lastconv", 1), "LSP_HIP_LASTCONV_ROWS": ("lastconv", 2),
    "LSP_HIP_LASTCONV_GENERIC": ("lastconv", 3), "LSP_HIP_LASTCONV_MFMA": ("lastconv", 4), "LSP_HIP_LASTCONV_VALU": ("lastconv", 5),
    "LSP_HIP_FIRSTCONV_DIRECT": ("firstconv", 1), "LSP_HIP_FIRSTCONV_REGSTAGE": ("firstconv", 2),
}
_RENAMED_ENV = {"LSP_HIP_XCD": "igemm_xcd", "LSP_HIP_FULLK_SPLIT_TILES": "fullk_split_tiles"}
# the keys lspf2f_create_tuned knows (include/lspf2f.h); an LSP_HIP_* variable that maps to none of them is a switch of the Python host
# (LSP_HIP_CAND_CACHE, networks.py) or a typo: it is not handed to the library (a typo gets a warning)
TUNE_KEYS = frozenset((
    "graph", "wino", "wino4", "wino_pre", "wino_ureg", "wino_prio", "in_wino_stats", "wino_xcd", "wino_il", "wino_rot", "winoup", "winoup_nb", "winoup_target", "igemm_xcd",
    "bandconv", "bandconv_min_blocks", "bandconv_min_frames", "patch16", "patchup16", "patch16_deep", "patch16_min_blocks", "rowup", "rowlast", "rowlast_fused", "rowconv", "fullk_split", "fullk_split_tiles", "fullk_s2",
    "all_forms", "blob_pad_kb", "fused_splitk", "fused_splitk16", "fullk16", "fullk16_min_frames", "out_wt", "prefetch", "smallm_dma", "smallm_kb", "smallm_static", "in_small_regs", "in_smallm_fused", "in_small_max_hw", "lastconv_direct", "lastconv", "firstconv"))
_HOST_ENV = frozenset(("LSP_HIP_CAND_CACHE", "LSP_HIP_TUNE"))


def tune_string(tune=None) -> bytes:
    """`tune` (None, a dict or a "k=v,k=v" string) merged over the LSP_HIP_* environment variables, as the library wants it."""
    kv = {}
    for name, val in os.environ.items():
        if not name.startswith("LSP_HIP_"):
            continue
        if name in _PRESENCE_ENV:
            k, v = _PRESENCE_ENV[name]
            kv.setdefault(k, v)
            continue
        if name in _HOST_ENV:
            continue
        key = _RENAMED_ENV.get(name, name[len("LSP_HIP_"):].lower())
        if key not in TUNE_KEYS:
            import warnings
            warnings.warn("%s is not a switch of liblspf2f (known keys: include/lspf2f.h): ignored" % name)
            continue
        try:
            kv[key] = int(val)
        except ValueError:
            raise ValueError("%s=%r: the switches of liblspf2f take integers" % (name, val))
    if "LSP_HIP_TUNE" in os.environ:
        tune_env = os.environ["LSP_HIP_TUNE"]
        for tok in filter(None, (t.strip() for t in tune_env.split(","))):
            k, v = tok.split("=")
            kv[k.strip()] = int(v)
    if isinstance(tune, str):
        for tok in filter(None, (t.strip() for t in tune.split(","))):
            k, v = tok.split("=")
            kv[k.strip()] = int(v)
    elif tune:
        kv.update({k: int(v) for k, v in tune.items()})
    return ",".join("%s=%d" % (k, v) for k, v in sorted(kv.items())).encode()


class Lspf2fError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lspf2f error %d (%s): %s" % (code, ERR_NAMES.get(code, "?"), msg))
        self.code = code


class Config(Structure):
    _fields_ = [("abi_version", c_int32), ("variant", c_int32), ("input_nc", c_int32),
                ("feat_nc", c_int32), ("output_nc", c_int32), ("ngf", c_int32),
                ("num_downs", c_int32), ("height", c_int32), ("width", c_int32),
                ("max_batch", c_int32), ("dtype", c_int32), ("flags", c_uint32)]


class LayerInfo(Structure):
    _fields_ = [("name", c_char_p), ("kernel", c_char_p),
                ("cin", c_int32), ("cout", c_int32), ("h_in", c_int32), ("h_out", c_int32),
                ("stride", c_int32), ("upsample", c_int32), ("concat", c_int32),
                ("residual", c_int32), ("relu", c_int32), ("tanh_out", c_int32),
                ("tile_m", c_int32), ("tile_n", c_int32), ("split_k", c_int32), ("k_group", c_int32),
                ("flops_per_frame", c_int64), ("exec_flops_per_frame", c_int64), ("act_bytes_per_frame", c_int64),
                ("weight_bytes", c_int64), ("w_offset", c_int64), ("scale_offset", c_int64),
                ("shift_offset", c_int64), ("out_offset", c_int64)]


# every symbol include/lspf2f.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "lspf2f_create": (c_int, [POINTER(Config), POINTER(c_void_p)]),
    "lspf2f_create_tuned": (c_int, [POINTER(Config), c_char_p, POINTER(c_void_p)]),
    "lspf2f_destroy": (c_int, [c_void_p]),
    "lspf2f_last_error": (c_char_p, []),
    "lspf2f_abi_version": (c_int, []),
    "lspf2f_num_tensors": (c_int, [c_void_p]),
    "lspf2f_tensor_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int64 * 4), POINTER(c_int)]),
    "lspf2f_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, c_size_t]),
    "lspf2f_packed_bytes": (c_size_t, [c_void_p]),
    "lspf2f_pack_weights": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspf2f_bind_weights": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspf2f_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "lspf2f_bind_workspace": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspf2f_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "lspf2f_set_candidates": (c_int, [c_void_p, c_void_p, c_void_p]),
    "lspf2f_forward_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "lspf2f_num_layers": (c_int, [c_void_p]),
    "lspf2f_plan_batch": (c_int, [c_void_p, c_int]),
    "lspf2f_layer_info_get": (c_int, [c_void_p, c_int, POINTER(LayerInfo)]),
    "lspf2f_forward_timed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                     POINTER(c_float)]),
    "lspf2f_subset_timed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, POINTER(c_int), c_int,
                                    POINTER(c_float), POINTER(c_int)]),
    "lspf2f_conv3x3_scratch_bytes": (c_size_t, [c_int] * 13),
    "lspf2f_conv3x3": (c_int, [c_void_p] * 7 + [c_int] * 14 + [c_void_p, c_size_t, c_void_p]),
    "lspf2f_instance_norm_scratch_bytes": (c_size_t, [c_int] * 4),
    "lspf2f_instance_norm": (c_int, [c_void_p] * 2 + [c_int] + [c_void_p] * 2 + [c_int] * 6 + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "lspf2f_conv3x3_instnorm_scratch_bytes": (c_size_t, [c_int] * 13),
    "lspf2f_conv3x3_instnorm": (c_int, [c_void_p] * 6 + [c_int] * 14 + [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "lspf2f_unet_prepare": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p]),
    "lspf2f_pixel_shuffle": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "lspf2f_clock_probe": (c_int, [c_void_p, c_uint32, c_void_p]),
    "lspf2f_memcpy": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "lspf2f_layer_form_offset": (c_int64, [c_void_p, c_int, c_int]),
    "lspf2f_debug_poison": (c_int, [c_void_p, ctypes.c_ubyte, c_void_p, POINTER(c_uint32)]),
}



A2H_MAX_STREAMS = 16
RNN_MAX_SEQUENCES = 16
MEL_MAX_SEGMENTS = 16


class A2HStreamCall(Structure):
    """lspa2h_stream_call (include/lspa2h.h)"""
    _fields_ = [("slot", c_int32), ("row0", c_int32), ("n_new", c_int32), ("step0", c_int32), ("step1", c_int32),
                ("pre_dev", c_void_p), ("noise_dev", c_void_p), ("expq_dev", c_void_p), ("state_in", c_void_p), ("state_out", c_void_p),
                ("out_dev", c_void_p)]


class A2HConfig(Structure):
    """lspa2h_config (include/lspa2h.h)"""
    _fields_ = [(n, c_int32) for n in ("abi_version", "residual_layers", "residual_blocks", "residual_channels",
                                       "dilation_channels", "skip_channels", "kernel_size", "input_channels",
                                       "cond_channels", "hidden_size", "ncenter", "ndim", "loss",
                                       "max_audio_frames")] + [("flags", c_uint32)]


A2H_ABI_VERSION = 1
A2H_LOSS_IDS = {"GMM": 0, "L2": 1}
A2H_FLAG_SINGLE_WORKGROUP = 1
A2H_FLAG_CONSECUTIVE_BLOCKS = 2
_GEN_ARGS = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_int, c_void_p]
# every symbol include/lspa2h.h declares
A2H_SIGNATURES = {
    "lspa2h_create": (c_int, [POINTER(A2HConfig), POINTER(c_void_p)]),
    "lspa2h_destroy": (c_int, [c_void_p]),
    "lspa2h_last_error": (c_char_p, []),
    "lspa2h_abi_version": (c_int, []),
    "lspa2h_receptive_field": (c_int, [c_void_p]),
    "lspa2h_num_tensors": (c_int, [c_void_p]),
    "lspa2h_tensor_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_size_t)]),
    "lspa2h_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, c_size_t]),
    "lspa2h_packed_bytes": (c_size_t, [c_void_p]),
    "lspa2h_pack_weights": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspa2h_bind_weights": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspa2h_workspace_bytes": (c_size_t, [c_void_p]),
    "lspa2h_bind_workspace": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspa2h_generate": (c_int, _GEN_ARGS),
    "lspa2h_generate_timed": (c_int, _GEN_ARGS + [POINTER(c_float), POINTER(c_float)]),
    "lspa2h_debug_cond": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int)]),
    "lspa2h_status": (c_int, [c_void_p, c_void_p, POINTER(c_uint32)]),
    "lspa2h_state_bytes": (c_size_t, [c_void_p]),
    "lspa2h_generate_resume": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "lspa2h_workspace_bytes_multi": (c_size_t, [c_void_p, c_int]),
    "lspa2h_bind_workspace_multi": (c_int, [c_void_p, c_void_p, c_size_t, c_int]),
    "lspa2h_generate_resume_multi": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "lspa2h_status_multi": (c_int, [c_void_p, c_void_p, POINTER(c_uint32)]),
    "lspa2h_sample_gmm": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
}

# every symbol include/lsplle.h declares
LLE_SIGNATURES = {
    "lsplle_last_error": (c_char_p, []),
    "lsplle_knn_workspace_bytes": (c_size_t, [c_int, c_int]),
    "lsplle_knn": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lsplle_solve": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                             c_float, c_void_p]),
}



class RNNConfig(Structure):
    """lsprnn_config (include/lsprnn.h)"""
    _fields_ = [(n, c_int32) for n in ("abi_version", "cell", "num_layers", "input_size", "hidden_size", "max_steps")] + [("flags", c_uint32)]


RNN_ABI_VERSION = 1
RNN_FLAG_PER_LAYER = 1
RNN_CELL_IDS = {"GRU": 0, "LSTM": 1}
# every symbol include/lsprnn.h declares
RNN_SIGNATURES = {
    "lsprnn_create": (c_int, [POINTER(RNNConfig), POINTER(c_void_p)]),
    "lsprnn_destroy": (c_int, [c_void_p]),
    "lsprnn_last_error": (c_char_p, []),
    "lsprnn_abi_version": (c_int, []),
    "lsprnn_num_tensors": (c_int, [c_void_p]),
    "lsprnn_tensor_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_size_t)]),
    "lsprnn_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, c_size_t]),
    "lsprnn_packed_bytes": (c_size_t, [c_void_p]),
    "lsprnn_pack_weights": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsprnn_bind_weights": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsprnn_workspace_bytes": (c_size_t, [c_void_p]),
    "lsprnn_bind_workspace": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsprnn_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "lsprnn_state_floats": (c_size_t, [c_void_p]),
    "lsprnn_forward_state": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsprnn_forward_multi": (c_int, [c_void_p, c_int, c_void_p, POINTER(c_int), c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    "lsprnn_status": (c_int, [c_void_p, c_void_p, POINTER(c_uint32)]),
    "lsprnn_linear": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
}

# every symbol include/lspraster.h declares
RASTER_SIGNATURES = {
    "lspraster_last_error": (c_char_p, []),
    "lspraster_edge_maps": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
}
RASTER_POINT_DTYPES = {"int32": 0, "float32": 1, "float64": 2}

# every symbol include/lspmel.h declares
MEL_SIGNATURES = {
    "lspmel_last_error": (c_char_p, []),
    "lspmel_num_windows": (c_int, [c_int64]),
    "lspmel_basis_floats": (c_size_t, []),
    "lspmel_make_basis": (c_int, [c_void_p, c_size_t]),
    "lspmel_workspace_bytes": (c_size_t, [c_int]),
    "lspmel_compute": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lspmel_window_start": (c_int64, [c_int64]),
    "lspmel_compute_ranges": (c_int, [c_int, POINTER(c_void_p), POINTER(c_int64), POINTER(c_int64), POINTER(c_int), POINTER(c_int64), POINTER(c_int),
                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lspmel_compute_range": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}



class UnetConfig(Structure):
    """lspunet_config (include/lspunet.h)"""
    _fields_ = [(n, c_int32) for n in ("abi_version", "input_nc", "feat_nc", "output_nc", "ngf", "num_downs", "size", "max_batch", "dtype")] + [("flags", c_uint32)]


UNET_ABI_VERSION = 1
UNET_FLAG_NO_GRAPH = 1
_UNET_FWD = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]
# every symbol include/lspunet.h declares
UNET_SIGNATURES = {
    "lspunet_create": (c_int, [POINTER(UnetConfig), c_char_p, POINTER(c_void_p)]),
    "lspunet_destroy": (c_int, [c_void_p]),
    "lspunet_last_error": (c_char_p, []),
    "lspunet_abi_version": (c_int, []),
    "lspunet_num_tensors": (c_int, [c_void_p]),
    "lspunet_tensor_info": (c_int, [c_void_p, c_int, POINTER(c_char_p), POINTER(c_int64 * 4), POINTER(c_int)]),
    "lspunet_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, c_size_t]),
    "lspunet_packed_bytes": (c_size_t, [c_void_p]),
    "lspunet_pack_weights": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspunet_bind_weights": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspunet_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "lspunet_bind_workspace": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lspunet_forward": (c_int, _UNET_FWD),
    "lspunet_forward_timed": (c_int, _UNET_FWD + [POINTER(c_float)]),
    "lspunet_num_launches": (c_int, [c_void_p, c_int]),
    "lspunet_launch_info": (c_int, [c_void_p, c_int, c_int, POINTER(c_char_p), POINTER(c_char_p), POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
}

class JpegEncOptions(ctypes.Structure):
    """lspjpeg_options"""
    _fields_ = [(n, ctypes.c_int32) for n in ("abi_version", "width", "height", "components", "quality", "optimize", "restart_interval")]


JPEG_ABI_VERSION = 1


class JpegEncFormat(ctypes.Structure):
    """lspjpeg_format"""
    _fields_ = [(n, ctypes.c_int32) for n in ("abi_version", "width", "height", "components", "quality", "optimize", "restart_interval", "h_samp", "v_samp")]


JPEG_FORMAT_ABI_VERSION = 1

# every symbol include/lspjpeg.h declares
JPEG_SIGNATURES = {
    "lspjpeg_create": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "lspjpeg_create_opts": (c_int, [POINTER(JpegEncOptions), POINTER(c_void_p)]),
    "lspjpeg_create_format": (c_int, [POINTER(JpegEncFormat), POINTER(c_void_p)]),
    "lspjpeg_host_optimal_table": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "lspjpeg_host_block_map": (c_int64, [POINTER(JpegEncFormat), c_void_p, c_size_t]),
    "lspjpeg_destroy": (c_int, [c_void_p]),
    "lspjpeg_last_error": (c_char_p, []),
    "lspjpeg_header": (c_int64, [c_void_p, c_void_p, c_size_t]),
    "lspjpeg_capacity_bytes": (c_size_t, [c_void_p]),
    "lspjpeg_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "lspjpeg_encode": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}


class JpegDecInfo(ctypes.Structure):
    """lspjpeg_dec_info"""
    _fields_ = [("status", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("components", ctypes.c_int32),
                ("hsamp", ctypes.c_int32), ("vsamp", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("mcus", ctypes.c_int32),
                ("segments", ctypes.c_int32), ("default_tables", ctypes.c_int32), ("scan_offset", ctypes.c_uint64), ("scan_bytes", ctypes.c_uint64)]


class JpegDecOutput(ctypes.Structure):
    """lspjpeg_dec_output"""
    _fields_ = [("ptr", c_void_p), ("table", c_void_p), ("plane_stride", c_int64), ("form", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class JpegDecSummary(ctypes.Structure):
    """lspjpeg_dec_summary"""
    _fields_ = [("files", ctypes.c_uint32), ("segments", ctypes.c_uint32), ("max_blocks", ctypes.c_uint32), ("max_pixels", ctypes.c_uint32),
                ("total_blocks", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("workspace_bytes", ctypes.c_uint64), ("status_offset", ctypes.c_uint64)]


class JpegDecScan(ctypes.Structure):
    """lspjpeg_dec_scan"""
    _fields_ = [("components", ctypes.c_int32), ("component", ctypes.c_uint8 * 4), ("dc_table", ctypes.c_uint8 * 4), ("ac_table", ctypes.c_uint8 * 4),
                ("ss", ctypes.c_int32), ("se", ctypes.c_int32), ("ah", ctypes.c_int32), ("al", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("units", ctypes.c_int32), ("segments", ctypes.c_int32), ("reserved", ctypes.c_int32), ("begin", ctypes.c_uint64), ("end", ctypes.c_uint64)]


# every symbol include/lspjpegdec.h declares
JPEGDEC_SIGNATURES = {
    "lspjpeg_dec_last_error": (c_char_p, []),
    "lspjpeg_dec_probe": (c_int, [c_void_p, c_size_t, POINTER(JpegDecInfo)]),
    "lspjpeg_dec_plan": (c_int64, [POINTER(c_void_p), POINTER(c_size_t), POINTER(JpegDecOutput), c_int, c_int, c_void_p, c_size_t]),
    "lspjpeg_dec_probe_flags": (c_int, [c_void_p, c_size_t, ctypes.c_uint, POINTER(JpegDecInfo)]),
    "lspjpeg_dec_plan_flags": (c_int64, [POINTER(c_void_p), POINTER(c_size_t), POINTER(JpegDecOutput), c_int, c_int, ctypes.c_uint, c_void_p, c_size_t]),
    "lspjpeg_dec_plan_scans": (c_int, [c_void_p, c_int]),
    "lspjpeg_dec_plan_scan": (c_int, [c_void_p, c_int, c_int, POINTER(JpegDecScan)]),
    "lspjpeg_dec_summary_of": (c_int, [c_void_p, POINTER(JpegDecSummary)]),
    "lspjpeg_dec_plan_parallel": (c_int, [c_void_p, c_int, POINTER(ctypes.c_uint32), POINTER(ctypes.c_uint32)]),
    "lspjpeg_dec_host_parallel_stats": (c_int, [POINTER(ctypes.c_uint32), POINTER(ctypes.c_uint32)]),
    "lspjpeg_dec_plan_file": (c_int, [c_void_p, c_int, POINTER(JpegDecInfo)]),
    "lspjpeg_dec_plan_qtable": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "lspjpeg_dec_plan_segment": (c_int, [c_void_p, c_int, POINTER(ctypes.c_uint32), POINTER(ctypes.c_uint32), POINTER(ctypes.c_uint32),
                                         POINTER(ctypes.c_uint64), POINTER(ctypes.c_uint64)]),
    "lspjpeg_dec_host_coefficients": (c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    "lspjpeg_dec_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}


class PngDecInfo(ctypes.Structure):
    """lsppng_dec_info"""
    _fields_ = [("status", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("color_type", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("components", ctypes.c_int32), ("idat_bytes", ctypes.c_uint64), ("raw_bytes", ctypes.c_uint64)]


class PngDecSummary(ctypes.Structure):
    """lsppng_dec_summary"""
    _fields_ = [("files", ctypes.c_uint32), ("max_pixels", ctypes.c_uint32), ("bytes", ctypes.c_uint64), ("workspace_bytes", ctypes.c_uint64),
                ("status_offset", ctypes.c_uint64)]


# every symbol include/lsppng.h declares (lsppng_dec_output has the layout of lspjpeg_dec_output, which csrc/pngdec.hip asserts: JpegDecOutput)
PNGDEC_SIGNATURES = {
    "lsppng_dec_last_error": (c_char_p, []),
    "lsppng_dec_probe": (c_int, [c_void_p, c_size_t, POINTER(PngDecInfo)]),
    "lsppng_dec_plan": (c_int64, [POINTER(c_void_p), POINTER(c_size_t), POINTER(JpegDecOutput), c_int, c_int, c_void_p, c_size_t]),
    "lsppng_dec_summary_of": (c_int, [c_void_p, POINTER(PngDecSummary)]),
    "lsppng_dec_plan_file": (c_int, [c_void_p, c_int, POINTER(PngDecInfo)]),
    "lsppng_dec_host_scanlines": (c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    "lsppng_dec_host_pixels": (c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    "lsppng_dec_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}


class PngEncOptions(ctypes.Structure):
    """lsppng_enc_options"""
    _fields_ = [(n, c_int32) for n in ("abi_version", "level", "filter")]


PNGENC_ABI_VERSION = 1
PNGENC_CHUNK = 16384
PNGENC_HEADER_BYTES = 33
# every symbol include/lsppngenc.h declares
PNGENC_SIGNATURES = {
    "lsppng_enc_create": (c_int, [c_int, c_int, c_int, POINTER(PngEncOptions), POINTER(c_void_p)]),
    "lsppng_enc_destroy": (c_int, [c_void_p]),
    "lsppng_enc_last_error": (c_char_p, []),
    "lsppng_enc_header": (c_int64, [c_void_p, c_void_p, c_size_t]),
    "lsppng_enc_capacity_bytes": (c_size_t, [c_void_p]),
    "lsppng_enc_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "lsppng_enc_encode": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lsppng_enc_host_file": (c_int64, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "lsppng_enc_host_code_lengths": (c_int, [c_void_p, c_int, c_int, c_void_p]),
}


class LmkConfig(Structure):
    """lsplmk_config (include/lsplmk.h)"""
    _fields_ = [(n, c_int32) for n in ("abi_version", "amp_method", "proj_f64", "n_candidates", "max_sessions", "ring_rows", "radius_mouth",
                                       "radius_rot", "radius_trans", "future_mouth", "future_rot", "future_trans")] + \
               [(n, ctypes.c_double) for n in ("sigma_mouth", "sigma_rot", "sigma_trans")] + [("amp", ctypes.c_double * 6), ("scale", ctypes.c_double)] + \
               [(n, c_float) for n in ("rot_amp", "trans_amp", "shoulder_amp", "pad_dx", "pad_dy")] + \
               [(n, c_void_p) for n in ("taps_mouth", "taps_rot", "taps_trans", "mean_mouth", "base_pts", "brow", "brow_indices", "mean_translation",
                                        "camera_intrinsic", "view_rotation", "view_translation", "shoulder3d", "ref_trans")]


class LmkSessionCall(Structure):
    """lsplmk_session_call (include/lsplmk.h)"""
    _fields_ = [(n, c_int32) for n in ("slot", "mouth_have", "mouth_fresh", "pose_have", "pose_fresh", "pose_stride", "emit0", "n_emit", "nframe",
                                       "reserved")] + [("mouth_dev", c_void_p), ("poses_dev", c_void_p), ("out_dev", c_void_p)]


LMK_ABI_VERSION = 1
LMK_MAX_SESSIONS = 16
LMK_MAX_RADIUS = 128
LMK_AMP_IDS = {"XY": 0, "XYZ": 1, "LowerMore": 2, "delta": 3, "CloseSmall": 4}
# every symbol include/lsplmk.h declares
LMK_SIGNATURES = {
    "lsplmk_create": (c_int, [POINTER(LmkConfig), POINTER(c_void_p)]),
    "lsplmk_destroy": (c_int, [c_void_p]),
    "lsplmk_last_error": (c_char_p, []),
    "lsplmk_abi_version": (c_int, []),
    "lsplmk_params_bytes": (c_size_t, [c_void_p]),
    "lsplmk_pack_params": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsplmk_bind_params": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsplmk_state_bytes": (c_size_t, [c_void_p]),
    "lsplmk_bind_state": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsplmk_clip_workspace_bytes": (c_size_t, [c_int]),
    "lsplmk_clip": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lsplmk_tick": (c_int, [c_void_p, c_int, POINTER(LmkSessionCall), c_void_p]),
    "lsplmk_check_tick": (c_int, [c_void_p, c_int, POINTER(LmkSessionCall)]),
}

class AviRun(Structure):
    """lspavi_run (include/lspavi.h)"""
    _fields_ = [(n, c_int32) for n in ("first", "count", "audio_format", "reserved")] + [("frame0", ctypes.c_int64), ("ring_dev", c_void_p)] + \
               [(n, ctypes.c_int64) for n in ("ring_samples", "sample0", "avail_begin", "avail_end")]


# every symbol include/lspavi.h declares
AVI_MAX_BATCH = 64
AVI_MAX_STREAMS = 16
AVI_STATUS_WORDS = 8
AVI_AUDIO_FORMATS = {None: 0, "s16": 1, "f32": 3}               # the WAVEFORMATEX wFormatTag
AVI_SIGNATURES = {
    "lspavi_last_error": (c_char_p, []),
    "lspavi_capacity_bytes": (c_size_t, [c_int, c_size_t, c_int, c_int, c_int, c_int]),
    "lspavi_workspace_bytes": (c_size_t, [c_int]),
    "lspavi_pack": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, ctypes.c_int64, ctypes.c_int64, c_int, c_int, c_int,
                            c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lspavi_capacity_bytes_multi": (c_size_t, [c_int, c_size_t, c_int, c_int, c_int, c_int]),
    "lspavi_workspace_bytes_multi": (c_size_t, [c_int]),
    "lspavi_pack_multi": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_int, POINTER(AviRun), c_int, c_int, c_int, c_void_p, c_size_t,
                                  c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
}



class RsConfig(Structure):
    """lsprs_config (include/lsprs.h)"""
    _fields_ = [("abi_version", c_int32), ("n_rates", c_int32), ("rates", c_int32 * 4), ("max_sessions", c_int32), ("max_push", c_int32)]


class RsSessionCall(Structure):
    """lsprs_session_call (include/lsprs.h)"""
    _fields_ = [(n, c_int32) for n in ("slot", "rate_index", "format", "channels")] + [("n_have", c_int64), ("out0", c_int64)] + \
               [(n, c_int32) for n in ("n_fresh", "n_out", "finished", "reserved")] + [("fresh_dev", c_void_p), ("out_dev", c_void_p)]


RS_ABI_VERSION = 1
RS_MAX_SESSIONS = 16
RS_MAX_RATES = 4
RS_FORMATS = {"f32": 0, "s16": 1}
# every symbol include/lsprs.h declares
RS_SIGNATURES = {
    "lsprs_create": (c_int, [POINTER(RsConfig), POINTER(c_void_p)]),
    "lsprs_destroy": (c_int, [c_void_p]),
    "lsprs_last_error": (c_char_p, []),
    "lsprs_abi_version": (c_int, []),
    "lsprs_rate_info": (c_int, [c_void_p, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_size_t)]),
    "lsprs_history": (c_int, [c_void_p]),
    "lsprs_params_bytes": (c_size_t, [c_void_p]),
    "lsprs_pack_params": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsprs_bind_params": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsprs_state_bytes": (c_size_t, [c_void_p]),
    "lsprs_bind_state": (c_int, [c_void_p, c_void_p, c_size_t]),
    "lsprs_out_count": (c_int64, [c_void_p, c_int, c_int64, c_int]),
    "lsprs_clip": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "lsprs_tick": (c_int, [c_void_p, c_int, POINTER(RsSessionCall), c_void_p]),
    "lsprs_check_tick": (c_int, [c_void_p, c_int, POINTER(RsSessionCall)]),
    "lsprs_launch_count": (c_int64, [c_void_p]),
}



class RszInfo(Structure):
    """lsprsz_info (include/lspresize.h)"""
    _fields_ = [(n, c_int32) for n in ("in_w", "in_h", "out_w", "out_h", "filter", "need_h", "need_v", "ksize_h", "ksize_v", "row0", "rows", "path_h",
                                       "path_v", "launches")] + [("lds_h", c_uint32), ("lds_v", c_uint32), ("bytes", ctypes.c_uint64)]


class RszOutput(Structure):
    """lsprsz_output (include/lspresize.h)"""
    _fields_ = [("ptr", c_void_p), ("table", c_void_p), ("image_stride", c_int64), ("plane_stride", c_int64), ("form", c_int32), ("reserved", c_int32)]


RSZ_MAX_SIDE = 8192
RSZ_FILTERS = {"box": 0, "bilinear": 1, "hamming": 2, "bicubic": 3, "lanczos": 4}
RSZ_PATHS = {0: None, 1: "tile", 2: "general"}
RSZ_FORM_U8, RSZ_FORM_PLANAR_F32 = 0, 1
# every symbol include/lspresize.h declares
RSZ_SIGNATURES = {
    "lsprsz_last_error": (c_char_p, []),
    "lsprsz_plan": (c_int64, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    "lsprsz_plan_info": (c_int, [c_void_p, POINTER(RszInfo)]),
    "lsprsz_plan_axis": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_size_t]),
    "lsprsz_workspace_bytes": (c_int64, [c_void_p, c_int, c_int]),
    "lsprsz_resize": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, POINTER(RszOutput), c_void_p, c_size_t, c_void_p]),
}

_lib = None


def load() -> ctypes.CDLL:
    """Load liblspf2f.so and bind every declared symbol; raises NativeLibraryError loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C livespeechportraits_amd/csrc`). There is no CPU/PyTorch fallback."
            % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise NativeLibraryError("failed to load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in list(SIGNATURES.items()) + list(A2H_SIGNATURES.items()) + list(LLE_SIGNATURES.items()) + list(RNN_SIGNATURES.items()) + list(RASTER_SIGNATURES.items()) + list(MEL_SIGNATURES.items()) + list(UNET_SIGNATURES.items()) + list(JPEG_SIGNATURES.items()) + list(JPEGDEC_SIGNATURES.items()) + list(PNGDEC_SIGNATURES.items()) + list(PNGENC_SIGNATURES.items()) + list(LMK_SIGNATURES.items()) + list(AVI_SIGNATURES.items()) + list(RS_SIGNATURES.items()) + list(RSZ_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError("%s does not export %s" % (LIB_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    if lib.lspf2f_abi_version() != ABI_VERSION:
        raise NativeLibraryError("ABI version mismatch: library %d, binding %d"
                                 % (lib.lspf2f_abi_version(), ABI_VERSION))
    if lib.lspa2h_abi_version() != A2H_ABI_VERSION:
        raise NativeLibraryError("lspa2h ABI version mismatch: library %d, binding %d"
                                 % (lib.lspa2h_abi_version(), A2H_ABI_VERSION))
    if lib.lspunet_abi_version() != UNET_ABI_VERSION:
        raise NativeLibraryError("lspunet ABI version mismatch: library %d, binding %d" % (lib.lspunet_abi_version(), UNET_ABI_VERSION))
    if lib.lsplmk_abi_version() != LMK_ABI_VERSION:
        raise NativeLibraryError("lsplmk ABI version mismatch: library %d, binding %d" % (lib.lsplmk_abi_version(), LMK_ABI_VERSION))
    if lib.lsprs_abi_version() != RS_ABI_VERSION:
        raise NativeLibraryError("lsprs ABI version mismatch: library %d, binding %d" % (lib.lsprs_abi_version(), RS_ABI_VERSION))
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != OK:
        msg = load().lspf2f_last_error()
        raise Lspf2fError(rc, msg.decode() if msg else "")


class Lspa2hError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lspa2h error %d: %s" % (code, msg))
        self.code = code


def check_a2h(rc: int) -> None:
    if rc != OK:
        msg = load().lspa2h_last_error()
        raise Lspa2hError(rc, msg.decode() if msg else "")


class LsplleError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lsplle error %d: %s" % (code, msg))
        self.code = code


def check_lle(rc: int) -> None:
    if rc != OK:
        msg = load().lsplle_last_error()
        raise LsplleError(rc, msg.decode() if msg else "")


class LsprnnError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lsprnn error %d: %s" % (code, msg))
        self.code = code


def check_rnn(rc: int) -> None:
    if rc != OK:
        msg = load().lsprnn_last_error()
        raise LsprnnError(rc, msg.decode() if msg else "")


class LsprasterError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lspraster error %d: %s" % (code, msg))
        self.code = code


def check_raster(rc: int) -> None:
    if rc != OK:
        msg = load().lspraster_last_error()
        raise LsprasterError(rc, msg.decode() if msg else "")


class LspmelError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lspmel error %d: %s" % (code, msg))
        self.code = code


def check_mel(rc: int) -> None:
    if rc != OK:
        msg = load().lspmel_last_error()
        raise LspmelError(rc, msg.decode() if msg else "")


class LspunetError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lspunet error %d (%s): %s" % (code, ERR_NAMES.get(code, "?"), msg))
        self.code = code


def check_unet(rc: int) -> None:
    if rc != OK:
        msg = load().lspunet_last_error()
        raise LspunetError(rc, msg.decode() if msg else "")


class LspjpegError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lspjpeg error %d: %s" % (code, msg))
        self.code = code


def check_jpeg(rc: int) -> None:
    if rc != OK:
        msg = load().lspjpeg_last_error()
        raise LspjpegError(rc, msg.decode() if msg else "")


def check_jpeg_dec(rc: int) -> int:
    """negative codes of include/lspjpegdec.h raise; anything else (0, a size, a status word) is handed back"""
    if rc < 0:
        msg = load().lspjpeg_dec_last_error()
        raise LspjpegError(rc, msg.decode() if msg else "")
    return rc


class LsppngError(RuntimeError):
    """negative return code of include/lsppng.h"""


def check_png_dec(rc: int) -> int:
    """negative codes of include/lsppng.h raise; anything else (0, a size, a status word) is handed back"""
    if rc < 0:
        msg = load().lsppng_dec_last_error()
        raise LsppngError("lsppng_dec error %d: %s" % (rc, msg.decode() if msg else "?"))
    return rc


def check_png_enc(rc: int) -> int:
    """negative codes of include/lsppngenc.h raise; anything else (0, a size) is handed back"""
    if rc < 0:
        msg = load().lsppng_enc_last_error()
        raise LsppngError("lsppng_enc error %d: %s" % (rc, msg.decode() if msg else "?"))
    return rc


class LspaviError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lspavi error %d: %s" % (code, msg))
        self.code = code


def check_avi(rc: int) -> None:
    if rc != OK:
        msg = load().lspavi_last_error()
        raise LspaviError(rc, msg.decode() if msg else "")


class LsplmkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lsplmk error %d: %s" % (code, msg))
        self.code = code


def check_lmk(rc: int) -> None:
    if rc != OK:
        msg = load().lsplmk_last_error()
        raise LsplmkError(rc, msg.decode() if msg else "")


class LsprsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lsprs error %d: %s" % (code, msg))
        self.code = code


def check_rs(rc: int) -> None:
    if rc != OK:
        msg = load().lsprs_last_error()
        raise LsprsError(rc, msg.decode() if msg else "")


class LsprszError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("lsprsz error %d: %s" % (code, msg))
        self.code = code


def check_rsz(rc: int) -> int:
    """negative codes of include/lspresize.h raise; anything else (0, a size, a count) is handed back"""
    if rc < 0:
        msg = load().lsprsz_last_error()
        raise LsprszError(rc, msg.decode() if msg else "")
    return rc
