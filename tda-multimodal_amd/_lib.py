"""ctypes binding of the C ABI in include/tda_rips.h, tda_umap.h and tda_dgm.h (libtda_rips.so, gfx950).

The product path has exactly one implementation: the HIP library.  If it is
missing or no gfx950 device is visible, calls raise -- there is no CPU
fallback (the CPU restatement under oracle/ is test infrastructure only).
The host side of a call's inputs and results (the NaN check, the per-layer
result objects) is the small CPython extension _hostviews.so, required too.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
BUILD_DIR = os.path.join(_HERE, "_build")
LIB_PATH = os.environ.get("TDA_RIPS_LIB") or os.path.join(BUILD_DIR, "libtda_rips.so")
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

TDA_F32, TDA_F64 = 0, 1
ERRORS = {-1: ValueError, -2: NotImplementedError, -3: RuntimeError, -4: RuntimeError, -5: RuntimeError}


class RipsArgs(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("is_dist", ctypes.c_int32),
        ("maxdim", ctypes.c_int32),
        ("thresh", ctypes.c_float),
        ("modulus", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("stream", ctypes.c_void_p),
        ("want_dist", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("labels", ctypes.c_void_p),
        ("n_label_sets", ctypes.c_int32),
        ("want_twonn", ctypes.c_int32),
        ("twonn_eps", ctypes.c_float),
        ("twonn_discard", ctypes.c_double),
        ("slot", ctypes.c_int32),
        ("x_parts", ctypes.c_void_p),  # ABI 6: const void* const* (dynamic batching)
        ("n_parts", ctypes.c_int32),
    ]


_i64p = ctypes.POINTER(ctypes.c_int64)
_f32p = ctypes.POINTER(ctypes.c_float)


class RipsResult(ctypes.Structure):
    _fields_ = [
        ("L", ctypes.c_int64),
        ("maxdim", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("count", _i64p),
        ("offset", _i64p),
        ("birth", _f32p),
        ("death", _f32p),
        ("birth_idx", _i64p),
        ("death_idx", _i64p),
        ("thresh", _f32p),
        ("num_edges", _i64p),
        ("checksum", ctypes.POINTER(ctypes.c_uint64)),
        ("n_all_pairs", _i64p),
        ("n_columns", _i64p),
        ("n_residual", _i64p),
        ("n_adds", _i64p),
        ("dist", _f32p),
        ("device_ms", ctypes.c_double),
        ("n_stages", ctypes.c_int32),
        ("stage_name", ctypes.POINTER(ctypes.c_char_p)),
        ("stage_ms", _f32p),
        ("silhouette", ctypes.POINTER(ctypes.c_double)),
        ("twonn", _f32p),
        ("blob", ctypes.c_void_p),
        ("blob_bytes", ctypes.c_int64),
        ("n_pairs", ctypes.c_int64),
        ("dist64", ctypes.POINTER(ctypes.c_double)),
        ("n_cap_reruns", ctypes.c_int64),  # ABI 8
    ]


TDA_FLAG_STAGE_TIMES = 1
TDA_FLAG_STAGE_SERIAL = 2
TDA_FLAG_DIST64 = 4
TDA_FLAG_NO_PERSISTENCE = 8
TDA_FLAG_ONE_STREAM = 16
TDA_FLAG_INPUT_READY = 32
TDA_MAX_SLOTS = 8
TDA_MAX_PARTS = 16
TDA_PIPE_POLL, TDA_PIPE_BLOCK, TDA_PIPE_DISPATCH = 0, 1, 2  # tda_pipe_wait modes
TDA_PIPE_BUSY = 1  # tda_pipe_wait: the ticket's call has not run yet


class UmapArgs(ctypes.Structure):  # include/tda_umap.h
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("metric", ctypes.c_int32),
        ("n_neighbors", ctypes.c_int32),
        ("n_components", ctypes.c_int32),
        ("n_epochs", ctypes.c_int32),
        ("init", ctypes.c_int32),
        ("negative_sample_rate", ctypes.c_int32),
        ("a", ctypes.c_float),
        ("b", ctypes.c_float),
        ("learning_rate", ctypes.c_float),
        ("repulsion_strength", ctypes.c_float),
        ("seed", ctypes.c_uint64),
        ("device", ctypes.c_int32),
        ("out", ctypes.c_void_p),
        ("graph_out", ctypes.c_void_p),
        ("stream", ctypes.c_void_p),
    ]


class EdArgs(ctypes.Structure):  # include/tda_rips.h tda_ed_args
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("B", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("device", ctypes.c_int32),
        ("stream", ctypes.c_void_p),
    ]


class SpectralArgs(ctypes.Structure):  # include/tda_rips.h tda_spectral_args
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("B", ctypes.c_int64),
        ("S", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("n_windows", ctypes.c_int64),
        ("n_alpha", ctypes.c_int32),
        ("alphas", ctypes.POINTER(ctypes.c_double)),
        ("eps", ctypes.c_double),
        ("device", ctypes.c_int32),
        ("stream", ctypes.c_void_p),
    ]


TDA_MAX_ALPHAS = 16  # orders per tda_matrix_entropy call


class GreedyArgs(ctypes.Structure):  # include/tda_rips.h tda_greedy_args
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("is_dist", ctypes.c_int32),
        ("n_perm", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("stream", ctypes.c_void_p),
        ("want_dperm2all", ctypes.c_int32),
    ]


class GreedyResult(ctypes.Structure):  # include/tda_rips.h tda_greedy_result
    _fields_ = [
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("n_perm", ctypes.c_int64),
        ("idx_perm", _i64p),
        ("lambdas", _f32p),
        ("dperm2all", _f32p),
        ("sub_dev", ctypes.c_void_p),  # device pointer: (L, n_perm, n_perm) f32, valid until tda_greedy_free
        ("device", ctypes.c_int32),
        ("device_ms", ctypes.c_double),
        ("select_ms", ctypes.c_double),
    ]


class ResampleArgs(ctypes.Structure):  # include/tda_rips.h tda_resample_args
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("is_dist", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("stream", ctypes.c_void_p),
        ("B", ctypes.c_int64),
        ("m", ctypes.c_int32),
        ("idx_per_layer", ctypes.c_int32),
        ("idx", ctypes.c_void_p),  # host int32 (B, m), or (L, B, m) with idx_per_layer
    ]


class ResampleResult(ctypes.Structure):  # include/tda_rips.h tda_resample_result
    _fields_ = [
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("B", ctypes.c_int64),
        ("m", ctypes.c_int64),
        ("hausdorff", _f32p),
        ("device", ctypes.c_int32),
        ("device_ms", ctypes.c_double),
    ]


class SubsampleH0Args(ctypes.Structure):  # include/tda_rips.h tda_subsample_h0_args
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("is_dist", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("stream", ctypes.c_void_p),
        ("B", ctypes.c_int64),
        ("m", ctypes.c_int32),
        ("idx_per_layer", ctypes.c_int32),
        ("idx", ctypes.c_void_p),  # host int32 (B, m), or (L, B, m) with idx_per_layer
        ("sizes", ctypes.c_void_p),  # host int32 (B,)
        ("alpha", ctypes.c_double),
        ("want_deaths", ctypes.c_int32),
    ]


class SubsampleH0Result(ctypes.Structure):  # include/tda_rips.h tda_subsample_h0_result
    _fields_ = [
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("B", ctypes.c_int64),
        ("m", ctypes.c_int64),
        ("E", ctypes.POINTER(ctypes.c_double)),
        ("deaths", _f32p),
        ("device", ctypes.c_int32),
        ("device_ms", ctypes.c_double),
    ]


class GeodesicArgs(ctypes.Structure):  # include/tda_rips.h tda_geodesic_args
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("is_dist", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("stream", ctypes.c_void_p),
        ("n_neighbors", ctypes.c_int32),  # k >= 1, or 0: not given
        ("graph_only", ctypes.c_int32),
        ("radius", ctypes.c_double),  # >= 0, or < 0: not given
    ]


class GeodesicResult(ctypes.Structure):  # include/tda_rips.h tda_geodesic_result
    _fields_ = [
        ("L", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("dist", _f32p),
        ("n_components", ctypes.POINTER(ctypes.c_int32)),
        ("n_edges", _i64p),
        ("device", ctypes.c_int32),
        ("device_ms", ctypes.c_double),
    ]


class PermArgs(ctypes.Structure):  # include/tda_rips.h tda_perm_args
    _fields_ = [
        ("w", ctypes.c_void_p),  # host float64 (S, S)
        ("obs", ctypes.c_void_p),  # host uint8 (S,)
        ("lab", ctypes.c_void_p),  # host uint8 (B, S)
        ("S", ctypes.c_int64),
        ("B", ctypes.c_int64),
        ("G", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PermResult(ctypes.Structure):  # include/tda_rips.h tda_perm_result
    _fields_ = [
        ("S", ctypes.c_int64),
        ("B", ctypes.c_int64),
        ("t_obs", ctypes.c_double),
        ("null", ctypes.POINTER(ctypes.c_double)),
        ("count", ctypes.c_int64),
        ("pvalue", ctypes.c_double),
        ("device", ctypes.c_int32),
        ("device_ms", ctypes.c_double),
    ]


TDA_PERM_MAX_S = 2048  # diagrams of a tda_permutation_test call
TDA_PERM_MAX_GROUPS = 64
TDA_PERM_MAX_TABLE = 1 << 27  # entries (B * S) of one call's label table
TDA_PERM_LDS_S = 128  # csrc/perm_kernels.h kPermLdsS: the largest S whose matrix k_perm_resident stages in LDS
TDA_PERM_ROWS = 8  # csrc/perm_kernels.h kPermR: labellings of one k_perm_tiled workgroup
TDA_RS_LDS_N = 128  # csrc/resample_kernels.h kRsLdsN: the largest N whose matrix k_resample_hausdorff stages in LDS
TDA_RS_MAX_POINTS = 8192  # N and m of a tda_resample call
TDA_RESAMPLE_MAX_OUT = 1 << 27  # resamples (L * B) of one call
TDA_SH0_MAX_OUT = 1 << 27  # subsamples (L * B), and deaths (L * B * (m - 1)), of one tda_subsample_h0 call
TDA_SH0_LDS_N = 128  # csrc/sh0_kernels.h kSh0LdsN: the largest N whose matrix k_subsample_h0 stages in LDS
TDA_SH0_LDS_M = 128  # csrc/sh0_kernels.h kSh0LdsM: the largest row length of that path
TDA_GEO_MAX_N = 8192  # N of a tda_geodesic call
TDA_GEO_MAX_OUT = 1 << 28  # values (L * N * N) of one tda_geodesic call
TDA_GEO_LDS_N = 128  # csrc/geo_kernels.h kGeoLdsN: the largest N whose matrix k_geo_resident closes in LDS
TDA_GEO_TILE = 64  # csrc/geo_kernels.h kGeoTile: the side of a tile of the blocked closure


class SwArgs(ctypes.Structure):  # include/tda_dgm.h tda_sw_args
    _fields_ = [
        ("points", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("S", ctypes.c_int64),
        ("pairs", ctypes.c_void_p),
        ("P", ctypes.c_int64),
        ("M", ctypes.c_int32),
        ("device", ctypes.c_int32),
    ]


class SwResult(ctypes.Structure):  # include/tda_dgm.h tda_sw_result
    _fields_ = [
        ("P", ctypes.c_int64),
        ("dist", ctypes.POINTER(ctypes.c_double)),
        ("device_ms", ctypes.c_double),
    ]


TDA_SW_MAX_POINTS = 4096  # finite points of a pair of diagrams together
TDA_SW_MAX_DIRECTIONS = 1024
TDA_SW_MAX_WORK = 1 << 27  # pairs x directions per call


class BnArgs(ctypes.Structure):  # include/tda_dgm.h tda_bn_args
    _fields_ = [
        ("points", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("S", ctypes.c_int64),
        ("pairs", ctypes.c_void_p),
        ("P", ctypes.c_int64),
        ("device", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class BnResult(ctypes.Structure):  # include/tda_dgm.h tda_bn_result
    _fields_ = [
        ("P", ctypes.c_int64),
        ("dist", ctypes.POINTER(ctypes.c_double)),
        ("device_ms", ctypes.c_double),
    ]


TDA_BN_MAX_POINTS = 512  # finite points of one diagram


class WsArgs(ctypes.Structure):  # include/tda_dgm.h tda_ws_args
    _fields_ = [
        ("points", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("S", ctypes.c_int64),
        ("pairs", ctypes.c_void_p),
        ("P", ctypes.c_int64),
        ("device", ctypes.c_int32),
        ("flags", ctypes.c_int32),
    ]


class WsResult(ctypes.Structure):  # include/tda_dgm.h tda_ws_result
    _fields_ = [
        ("P", ctypes.c_int64),
        ("dist", ctypes.POINTER(ctypes.c_double)),
        ("device_ms", ctypes.c_double),
        ("match_off", _i64p),
        ("match", ctypes.POINTER(ctypes.c_int32)),
    ]


TDA_WS_MAX_POINTS = 512  # finite points of one diagram
TDA_WS_WANT_MATCHING = 1


class PlArgs(ctypes.Structure):  # include/tda_dgm.h tda_pl_args
    _fields_ = [
        ("points", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("S", ctypes.c_int64),
        ("grid", ctypes.c_void_p),
        ("G", ctypes.c_int32),
        ("K", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PlResult(ctypes.Structure):  # include/tda_dgm.h tda_pl_result
    _fields_ = [
        ("S", ctypes.c_int64),
        ("F", ctypes.c_int64),
        ("values", ctypes.POINTER(ctypes.c_double)),
        ("device_ms", ctypes.c_double),
    ]


class PiArgs(ctypes.Structure):  # include/tda_dgm.h tda_pi_args
    _fields_ = [
        ("points", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("S", ctypes.c_int64),
        ("x_edges", ctypes.c_void_p),
        ("y_edges", ctypes.c_void_p),
        ("W", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("sigma", ctypes.c_double),
        ("weight_power", ctypes.c_double),
        ("device", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PiResult(ctypes.Structure):  # include/tda_dgm.h tda_pi_result
    _fields_ = [
        ("S", ctypes.c_int64),
        ("F", ctypes.c_int64),
        ("values", ctypes.POINTER(ctypes.c_double)),
        ("device_ms", ctypes.c_double),
    ]


TDA_VEC_MAX_POINTS = 4096  # finite points of one diagram
TDA_VEC_MAX_OUT = 1 << 24  # doubles of one call's result
TDA_PL_MAX_DEPTH = 64
TDA_PL_MAX_STEPS = 4096
TDA_PI_MAX_PIXELS = 256  # per axis
TDA_PI_ERF_ULP = 16  # E of the image's accuracy bound C(n) = 2 E + 9 + n


class PcArgs(ctypes.Structure):  # include/tda_dgm.h tda_pc_args
    _fields_ = [
        ("points", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("S", ctypes.c_int64),
        ("coef", ctypes.c_void_p),
        ("grid", ctypes.c_void_p),
        ("G", ctypes.c_int32),
        ("kernel", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PcResult(ctypes.Structure):  # include/tda_dgm.h tda_pc_result
    _fields_ = [
        ("S", ctypes.c_int64),
        ("F", ctypes.c_int64),
        ("values", ctypes.POINTER(ctypes.c_double)),
        ("device_ms", ctypes.c_double),
    ]


TDA_PC_INDICATOR = 0  # kernel: 1 on [b, d)
TDA_PC_TENT = 1  # kernel: max(0, min(t - b, d - t))
TDA_PC_NORMALIZE = 1  # flags
TDA_PC_KEEP_ESSENTIAL = 2  # flags: indicator only


class HkArgs(ctypes.Structure):  # include/tda_dgm.h tda_hk_args
    _fields_ = [
        ("points", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("S", ctypes.c_int64),
        ("pairs", ctypes.c_void_p),
        ("P", ctypes.c_int64),
        ("sigma", ctypes.c_double),
        ("device", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class HkResult(ctypes.Structure):  # include/tda_dgm.h tda_hk_result
    _fields_ = [
        ("P", ctypes.c_int64),
        ("kern", ctypes.POINTER(ctypes.c_double)),
        ("self", ctypes.POINTER(ctypes.c_double)),
        ("dist", ctypes.POINTER(ctypes.c_double)),
        ("device_ms", ctypes.c_double),
    ]


TDA_HK_MAX_POINTS = 4096  # finite points of one diagram
TDA_HK_EXP_ULP = 3  # E of the heat kernel's accuracy bound C(n1, n2)


class PfArgs(ctypes.Structure):  # include/tda_dgm.h tda_pf_args
    _fields_ = [
        ("points", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("S", ctypes.c_int64),
        ("pairs", ctypes.c_void_p),
        ("P", ctypes.c_int64),
        ("sigma", ctypes.c_double),
        ("device", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PfResult(ctypes.Structure):  # include/tda_dgm.h tda_pf_result
    _fields_ = [
        ("P", ctypes.c_int64),
        ("a", ctypes.POINTER(ctypes.c_double)),
        ("b", ctypes.POINTER(ctypes.c_double)),
        ("h", ctypes.POINTER(ctypes.c_double)),
        ("dist", ctypes.POINTER(ctypes.c_double)),
        ("device_ms", ctypes.c_double),
    ]


TDA_PF_MAX_POINTS = 1024  # finite points of a diagram that a pair names
TDA_PF_EXP_ULP = 3  # E of the persistence Fisher accuracy bound B(n1, n2)
TDA_PF_CUT = 708  # a term whose argument is below -708 is +0.0
TDA_PF_LANES = 64  # evaluation points of a part
TDA_PF_CHUNK = 128  # sources staged at a time


class UmapTransformArgs(ctypes.Structure):  # include/tda_umap.h
    _fields_ = [
        ("x_train", ctypes.c_void_p),
        ("emb_train", ctypes.c_void_p),
        ("y", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("x_on_device", ctypes.c_int32),
        ("L", ctypes.c_int64),
        ("M", ctypes.c_int64),
        ("N", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("metric", ctypes.c_int32),
        ("n_neighbors", ctypes.c_int32),
        ("n_components", ctypes.c_int32),
        ("n_epochs", ctypes.c_int32),
        ("negative_sample_rate", ctypes.c_int32),
        ("a", ctypes.c_float),
        ("b", ctypes.c_float),
        ("learning_rate", ctypes.c_float),
        ("repulsion_strength", ctypes.c_float),
        ("disconnection", ctypes.c_float),
        ("seed", ctypes.c_uint64),
        ("device", ctypes.c_int32),
        ("out", ctypes.c_void_p),
        ("stream", ctypes.c_void_p),
    ]


# every symbol declared in include/tda_rips.h and include/tda_umap.h
EXPORTS = ("tda_rips_batch", "tda_rips_dm", "tda_rips_free", "tda_last_error", "tda_version", "tda_device_ok",
           "tda_effective_dim", "tda_effective_dim_windows", "tda_matrix_entropy", "tda_greedy_perm", "tda_greedy_free",
           "tda_resample", "tda_resample_free", "tda_geodesic", "tda_geodesic_free", "tda_permutation_test", "tda_perm_free", "tda_umap_batch", "tda_umap_transform", "tda_debug_dist_plan", "tda_debug_attempts",
           "tda_pipe_create", "tda_pipe_submit", "tda_pipe_flush", "tda_pipe_wait", "tda_pipe_release", "tda_pipe_destroy")
# the entries of include/tda_dgm.h, all of one shape, int entry(const args*, result**) and void free(result*):
# name -> (entry symbol, free symbol, args struct, result struct)
DGM_ENTRIES = {
    "sw": ("tda_sliced_wasserstein", "tda_sw_free", SwArgs, SwResult),
    "bn": ("tda_bottleneck", "tda_bn_free", BnArgs, BnResult),
    "ws": ("tda_wasserstein", "tda_ws_free", WsArgs, WsResult),
    "pl": ("tda_landscape", "tda_pl_free", PlArgs, PlResult),
    "pi": ("tda_persistence_image", "tda_pi_free", PiArgs, PiResult),
    "hk": ("tda_heat_kernel", "tda_hk_free", HkArgs, HkResult),
    "pc": ("tda_persistence_curve", "tda_pc_free", PcArgs, PcResult),
    "pf": ("tda_persistence_fisher", "tda_persistence_fisher_free", PfArgs, PfResult),
}
# their symbols, one tuple per addition to the header
DGM_EXPORTS = DGM_ENTRIES["sw"][:2]
BOTTLENECK_EXPORTS = DGM_ENTRIES["bn"][:2]
WASSERSTEIN_EXPORTS = DGM_ENTRIES["ws"][:2]
VECTOR_EXPORTS = DGM_ENTRIES["pl"][:2] + DGM_ENTRIES["pi"][:2]
HEAT_EXPORTS = DGM_ENTRIES["hk"][:2]
CURVE_EXPORTS = DGM_ENTRIES["pc"][:2]
FISHER_EXPORTS = DGM_ENTRIES["pf"][:2]
# include/tda_rips.h again: the subsample H0 entry (its names hold a digit, so they have a tuple of their own)
SUBSAMPLE_H0_EXPORTS = ("tda_subsample_h0", "tda_subsample_h0_free")

# include/tda_rips.h again: the side entries of the same shape, int entry(const args*, result**) and void free(result*)
SIDE_ENTRIES = {
    "greedy": ("tda_greedy_perm", "tda_greedy_free", GreedyArgs, GreedyResult),
    "resample": ("tda_resample", "tda_resample_free", ResampleArgs, ResampleResult),
    "sh0": SUBSAMPLE_H0_EXPORTS + (SubsampleH0Args, SubsampleH0Result),
    "geo": ("tda_geodesic", "tda_geodesic_free", GeodesicArgs, GeodesicResult),
    "perm": ("tda_permutation_test", "tda_perm_free", PermArgs, PermResult),
}
_ENTRIES = {**DGM_ENTRIES, **SIDE_ENTRIES}

_lib = None


def build(verbose: bool = False, out: str | None = None, extra_flags: tuple = ()) -> str:
    """Compile csrc/rips.hip for gfx950 into _build/libtda_rips.so (in-tree).

    ``out``/``extra_flags`` build variants (e.g. ``-DTDA_PROFILE`` into another
    path, selected at load time with TDA_RIPS_LIB)."""
    import shutil
    import tempfile

    out = out or LIB_PATH
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # compile from a snapshot of the sources: hipcc reads them once for the device pass and again,
    # minutes later, for the host pass, so an edit in between would give a library whose host
    # and device sides disagree on the kernel argument structs
    snap = tempfile.mkdtemp(prefix="tda_build_")
    try:
        shutil.copytree(CSRC, os.path.join(snap, "pkg", "csrc"))  # csrc/../../include stays the include dir
        shutil.copytree(INCLUDE, os.path.join(snap, "include"))
        src = os.path.join(snap, "pkg", "csrc", "rips.hip")
        cmd = [
            os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"),
            "--offload-arch=gfx950",
            "-O3",
            "-std=c++17",
            "-shared",
            "-fPIC",
            "-I" + os.path.join(snap, "include"),
            *extra_flags,
            "-o",
            out + ".tmp",
            src,
        ]
        r = subprocess.run(cmd, capture_output=True, text=True)
    finally:
        shutil.rmtree(snap, ignore_errors=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])
    if verbose and r.stderr:
        print(r.stderr, file=sys.stderr)
    os.replace(out + ".tmp", out)
    if out == LIB_PATH:
        build_hostviews()
    return out


HOSTVIEWS_PATH = os.path.join(BUILD_DIR, "_hostviews.so")
_hostviews = None


def build_hostviews(out: str | None = None) -> str:
    """Compile csrc/hostviews.c (CPython + numpy C API, host code: a batch's
    per-layer result objects in one call) into _build/_hostviews.so."""
    import sysconfig

    import numpy as np

    out = out or HOSTVIEWS_PATH
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [os.environ.get("CC", "gcc"), "-O3", "-shared", "-fPIC", "-Wall", "-Werror", "-I" + sysconfig.get_paths()["include"],
           "-I" + np.get_include(), "-o", out + ".tmp", os.path.join(CSRC, "hostviews.c")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hostviews build failed:\n" + r.stderr[-4000:])
    os.replace(out + ".tmp", out)
    return out


def hostviews():
    """The _hostviews extension (segments / layer_tuples); raise loudly if it is absent."""
    global _hostviews
    if _hostviews is None:
        import importlib.machinery
        import importlib.util

        if not os.path.exists(HOSTVIEWS_PATH):
            raise RuntimeError(f"host extension not built: {HOSTVIEWS_PATH} is missing (run __graft_entry__.build())")
        loader = importlib.machinery.ExtensionFileLoader("_hostviews", HOSTVIEWS_PATH)
        spec = importlib.util.spec_from_file_location("_hostviews", HOSTVIEWS_PATH, loader=loader)
        mod = importlib.util.module_from_spec(spec)
        loader.exec_module(mod)
        _hostviews = mod
    return _hostviews


def lib():
    """Load libtda_rips.so; raise loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"HIP extension not built: {LIB_PATH} is missing (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    L.tda_rips_batch.argtypes = [ctypes.POINTER(RipsArgs), ctypes.POINTER(ctypes.POINTER(RipsResult))]
    L.tda_rips_batch.restype = ctypes.c_int
    L.tda_rips_dm.argtypes = [_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int32,
                              ctypes.POINTER(ctypes.POINTER(RipsResult))]
    L.tda_rips_dm.restype = ctypes.c_int
    L.tda_rips_free.argtypes = [ctypes.POINTER(RipsResult)]
    L.tda_rips_free.restype = None
    L.tda_last_error.argtypes = []
    L.tda_last_error.restype = ctypes.c_char_p
    L.tda_version.restype = ctypes.c_int
    L.tda_device_ok.argtypes = [ctypes.c_int32]
    L.tda_device_ok.restype = ctypes.c_int
    _i32p = ctypes.POINTER(ctypes.c_int32)
    L.tda_debug_dist_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, _i32p, _i32p, _i32p]
    L.tda_debug_dist_plan.restype = ctypes.c_int
    L.tda_debug_attempts.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    L.tda_debug_attempts.restype = ctypes.c_int
    L.tda_umap_batch.argtypes = [ctypes.POINTER(UmapArgs)]
    L.tda_umap_batch.restype = ctypes.c_int
    L.tda_effective_dim.argtypes = [ctypes.POINTER(EdArgs), _f32p]
    L.tda_effective_dim.restype = ctypes.c_int
    L.tda_effective_dim_windows.argtypes = [ctypes.POINTER(SpectralArgs), _f32p]
    L.tda_effective_dim_windows.restype = ctypes.c_int
    L.tda_matrix_entropy.argtypes = [ctypes.POINTER(SpectralArgs), _f32p]
    L.tda_matrix_entropy.restype = ctypes.c_int
    L.tda_umap_transform.argtypes = [ctypes.POINTER(UmapTransformArgs)]
    L.tda_umap_transform.restype = ctypes.c_int
    # the native sweep pipeline (tda_pipe_*): the pipe is an opaque handle, tickets and call ids are uint64
    _u64p = ctypes.POINTER(ctypes.c_uint64)
    L.tda_pipe_create.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    L.tda_pipe_create.restype = ctypes.c_int
    L.tda_pipe_submit.argtypes = [ctypes.c_void_p, ctypes.POINTER(RipsArgs), ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                  ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _u64p]
    L.tda_pipe_submit.restype = ctypes.c_int
    L.tda_pipe_flush.argtypes = [ctypes.c_void_p]
    L.tda_pipe_flush.restype = ctypes.c_int
    L.tda_pipe_wait.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(RipsResult)), _i64p, _i64p, _i32p,
                                _u64p, ctypes.c_int32]
    L.tda_pipe_wait.restype = ctypes.c_int
    L.tda_pipe_release.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    L.tda_pipe_release.restype = ctypes.c_int
    L.tda_pipe_destroy.argtypes = [ctypes.c_void_p]
    L.tda_pipe_destroy.restype = None
    for entry, free, Args, Result in _ENTRIES.values():
        getattr(L, entry).argtypes = [ctypes.POINTER(Args), ctypes.POINTER(ctypes.POINTER(Result))]
        getattr(L, entry).restype = ctypes.c_int
        getattr(L, free).argtypes = [ctypes.POINTER(Result)]
        getattr(L, free).restype = None
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().tda_last_error().decode(errors="replace")
        raise ERRORS.get(rc, RuntimeError)(msg)


@contextlib.contextmanager
def result(entry: str, args):
    """One call of a result-returning entry (a key of DGM_ENTRIES or SIDE_ENTRIES): the return code
    checked, the library-owned result struct yielded and freed on exit.  What outlives the block
    must be copied inside it."""
    symbol, free, _, Result = _ENTRIES[entry]
    L = lib()
    res = ctypes.POINTER(Result)()
    check(getattr(L, symbol)(ctypes.byref(args), ctypes.byref(res)))
    try:
        yield res.contents
    finally:
        getattr(L, free)(res)
