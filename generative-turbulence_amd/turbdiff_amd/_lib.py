"""ctypes binding of libtdx_hip.so -- the C ABI declared in include/tdx.h.

The library is built in-tree by ``__graft_entry__.build()`` (``make -C csrc``) and lives next
to this file.  There is no CPU implementation behind this module: if the shared object is
missing, or a kernel launch fails, a RuntimeError is raised.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path

import torch

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("TDX_LIB", _HERE / "libtdx_hip.so"))  # TDX_LIB: kernel-development builds

F32, BF16 = 0, 1
F16 = 3  # TDX_F16: IEEE half tensors (fp16 MFMA operands, fp32 accumulation)
CONV_AUTO, CONV_DIRECT, CONV_MFMA, CONV_SPLIT = 0, 1, 2, 3
F32_SPLIT = 2  # TDX_F32_SPLIT: pack code of fp32 weights for CONV_SPLIT
WS_CLEAN = 0x100  # TDX_WS_CLEAN (include/tdx.h)
ACT_NONE, ACT_SILU, ACT_GELU, ACT_RELU, ACT_SOFTPLUS, ACT_TANH = range(6)  # TDX_ACT_*

_vp, _i, _i64, _u64, _f, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_size_t

# name -> (restype, argtypes); must list every symbol of include/tdx.h
SIGNATURES = {
    "tdx_version": (_i, []),
    "tdx_arch": (C.c_char_p, []),
    "tdx_switch_count": (_i, []),
    "tdx_switch_name": (C.c_char_p, [_i]),
    "tdx_switch_default": (_i, [_i]),
    "tdx_switch_value": (_i, [_i]),
    "tdx_set_scratch": (_i, [_vp, _sz]),
    "tdx_ncv_to_nvc": (_i, [_vp, _vp, _i, _i, _i64, _i, _i, _vp]),
    "tdx_nvc_to_ncv": (_i, [_vp, _vp, _i, _i, _i64, _i, _i, _vp]),
    "tdx_cast": (_i, [_vp, _vp, _i64, _i, _i, _vp]),
    "tdx_conv3_pack_weight": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "tdx_conv3_pack_weights": (_i, [_vp, _i, _i, _vp]),
    "tdx_transpose_many": (_i, [_vp, _i, _vp]),
    "tdx_conv3_fwd": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tdx_conv3_uses_ring": (_i, [_i] * 7),
    "tdx_conv3_ring_brick_depth": (_i, [_i] * 7),
    "tdx_conv3_fwd_kernel": (_i, [_i] * 9),
    "tdx_conv3_fwd_gn": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tdx_conv3_fwd_partial": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tdx_conv3_bwd_data_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "tdx_conv3_bwd_data": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "tdx_conv3_bwd_data_add": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "tdx_conv3_bwd_data_skip_supported": (_i, [_i] * 9),
    "tdx_conv3_bwd_data_skip": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "tdx_conv3_bwd_weight_workspace_bytes": (_sz, [_i, _i, _i]),
    "tdx_conv3_bwd_weight": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "tdx_conv3_bwd_weight_plan": (_i, [_i] * 9 + [_vp]),
    "tdx_conv1_fwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _i64, _i, _i, _vp]),
    "tdx_conv1_fwd_gn": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i64, _i, _i, _vp]),
    "tdx_conv1_bwd_weight": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i64, _i, _vp]),
    "tdx_conv1_bwd_weight_oc": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i64, _i, _vp]),
    "tdx_conv1_fwd_plan": (_i, [_i] * 8 + [_vp]),
    "tdx_conv1_bwd_weight_plan": (_i, [_i, _i, _i64, _i, _i, _vp]),
    "tdx_encode_fwd": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i64, _i, _i, _vp]),
    "tdx_encode_bwd": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp]),
    "tdx_decode_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _vp]),
    "tdx_decode_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _vp]),
    "tdx_gn_workspace_bytes": (_sz, [_i, _i]),
    "tdx_gn_stats": (_i, [_vp, _vp, _i, _i64, _i, _i, _f, _i, _vp, _vp]),
    "tdx_gn_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _vp]),
    "tdx_gn_apply_decode": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _vp]),
    "tdx_gn_apply_encoded": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _vp]),
    "tdx_gn_apply_decode_act": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _vp]),
    "tdx_gn_apply_encoded_act": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _vp]),
    "tdx_gn_bwd": (_i, [_vp] * 12 + [_i, _i64, _i, _i, _i, _i, _vp, _vp]),
    "tdx_bn_workspace_bytes": (_sz, [_i64, _i]),
    "tdx_bn_stats": (_i, [_vp, _vp, _vp, _i64, _i, _f, _i, _vp, _vp]),
    "tdx_bn_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i, _f, _i, _vp]),
    "tdx_bn_bwd": (_i, [_vp] * 8 + [_i64, _i, _f, _i, _i, _vp, _vp]),
    "tdx_flow_decompose_workspace_bytes": (_sz, [_i] * 7),
    "tdx_flow_decompose_fwd": (_i, [_vp] * 6 + [_i] * 8 + [_vp]),
    "tdx_flow_decompose_bwd": (_i, [_vp] * 9 + [_i] * 8 + [_vp, _vp]),
    "tdx_resize_fwd": (_i, [_vp, _vp] + [_i] * 9 + [_vp]),
    "tdx_resize_bwd": (_i, [_vp, _vp, _vp] + [_i] * 9 + [_vp]),
    "tdx_resize_plan": (_i, [_i] * 9 + [_vp]),
    "tdx_attn_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tdx_attn_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "tdx_attn_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "tdx_attn_plan": (_i, [_i] * 5 + [_vp]),
    "tdx_cell_mask": (_i, [_vp, _i64, _vp, _i64, _vp]),
    "tdx_q_sample": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _i64, _vp]),
    "tdx_p_sample_step": (_i, [_vp] * 7 + [_i, _vp, _i, _i, _vp, _i, _i, _i64, _vp]),
    "tdx_p_sample_step_rng": (_i, [_vp] * 5 + [_i, _vp, _i, _i, _vp, _i, _i, _i64, _u64, _vp, _vp, _vp]),
    "tdx_p_sample_step_lv": (_i, [_vp] * 8 + [_i, _vp, _i, _i, _vp, _i, _i, _i64, _vp]),
    "tdx_p_sample_step_lv_rng": (_i, [_vp] * 6 + [_i, _vp, _i, _i, _vp, _i, _i, _i64, _u64, _vp, _vp, _vp]),
    "tdx_ddim_step": (_i, [_vp] * 7 + [_i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i64, _vp]),
    "tdx_ddim_step_rng": (_i, [_vp] * 5 + [_i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i64, _u64, _vp, _vp, _vp]),
    "tdx_p_sample_step_lv_respaced": (_i, [_vp] * 7 + [_i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i64, _vp]),
    "tdx_p_sample_step_lv_respaced_rng": (_i, [_vp] * 5 + [_i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i64, _u64, _vp, _vp, _vp]),
    "tdx_ddim_step_lv": (_i, [_vp] * 7 + [_i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i64, _vp]),
    "tdx_ddim_step_lv_rng": (_i, [_vp] * 5 + [_i, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i64, _u64, _vp, _vp, _vp]),
    "tdx_masked_loss": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _i, _i, _i64, _vp, _vp]),
    "tdx_masked_loss_dyn": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i64, _vp, _vp]),
    "tdx_masked_loss_workspace_bytes": (_sz, []),
    "tdx_elbo_loss": (_i, [_vp] * 5 + [_i64, _vp, _vp, _vp, _i, _i, _i, _i, C.c_double, _vp, _vp, _i, _i, _i64, _vp, _vp]),
    "tdx_elbo_loss_dyn": (_i, [_vp] * 5 + [_vp, _vp, _vp, _vp, _i, _i, _i, _i, C.c_double, _vp, _vp, _i, _i, _i64, _vp, _vp]),
    "tdx_elbo_loss_workspace_bytes": (_sz, []),
    "tdx_grid_embed": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _vp]),
    "tdx_grid_select": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i64, _i64, _vp]),
    "tdx_cell_embed_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i64, _vp]),
    "tdx_cell_embed_bwd_workspace_bytes": (_sz, [_i, _i]),
    "tdx_cell_embed_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i64, _vp, _vp]),
    "tdx_tke_energy": (_i, [_vp, _vp, _i, _i64, _vp]),
    "tdx_tke_sphere": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "tdx_fd": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _i, _vp]),
    "tdx_ot_features": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _f, _f, _f, _vp]),
    "tdx_ot_workspace_bytes": (_sz, [_i, _i]),
    "tdx_ot_auction": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _i, _i, _i, C.c_double, _i, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    "tdx_moments_update": (_i, [_vp, _i, _i64, _vp, _vp, _i64, _vp]),
    "tdx_field_stats_workspace_bytes": (_sz, [_i64, _i]),
    "tdx_field_stats": (_i, [_vp, _i64, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "tdx_w2n_blocks": (_i, [_i64]),
    "tdx_w2n_assign": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "tdx_w2n_reduce": (_i, [_vp, _i, _i, _vp, _vp]),
    "tdx_lagprod_workspace_bytes": (_sz, [_i, _i64, _i]),
    "tdx_lagprod_update": (_i, [_vp, _i, _i64, _vp, _vp, _i64, _i, _vp, _vp, _i64, _vp, _vp]),
    "tdx_smooth_residual_workspace_bytes": (_sz, [_i64, _i]),
    "tdx_smooth_residual_update": (_i, [_vp, _i, _i64, _vp, _i, _i, _vp, _vp, _i64, _vp, _vp]),
    "tdx_sqdev_workspace_bytes": (_sz, [_i64, _i]),
    "tdx_sqdev_sum": (_i, [_vp, _vp, _i, _i64, _i, _i, _vp, _vp, _vp]),
    "tdx_fma64_probe": (_i, [_vp, _i, _i, _vp]),
    "tdx_randn": (_i, [_vp, _i64, _u64, _u64, _vp, _vp]),
    "tdx_randn_batched": (_i, [_vp, _i, _i64, _u64, _vp, _vp, _vp]),
    "tdx_convg_apply": (_i, [_vp, _vp, _vp, _vp] + [_i] * 16 + [_vp]),
    "tdx_convg_fold_clamp": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tdx_convg_bwd_weight": (_i, [_vp, _vp, _vp, _vp] + [_i] * 15 + [_vp]),
    "tdx_convg_apply_fused": (_i, [_vp, _vp, _vp, _vp] + [_i] * 13 + [_vp, _i, _vp]),
    "tdx_convg_fold_fused": (_i, [_vp] * 6 + [_i] * 7 + [_vp]),
    "tdx_film_supported": (_i, [_i, _i]),
    "tdx_film_fwd": (_i, [_vp, _i, _i, _vp, _i, _vp]),
    "tdx_film_bwd_workspace_bytes": (_sz, [_i, _i, _vp, _i]),
    "tdx_film_bwd": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "tdx_opt_chunk_elems": (_i64, []),
    "tdx_grad_norm": (_i, [_vp, _vp, _vp, _i, _f, _vp, _vp, _vp]),
    "tdx_radam_step": (_i, [_vp, _vp, _vp, _i, _vp, _i64, _f, _f, _f, _f, _i, _vp]),
    "tdx_signal_host": (_i, [_vp, _vp, C.c_uint32, _vp]),
    "tdx_stage_scaled": (_i, [_vp, _i, _f, _vp]),
    "tdx_grad_norm_scaled": (_i, [_vp, _vp, _vp, _i, _f, _f, _vp, _vp, _vp]),
    "tdx_radam_step_scaled": (_i, [_vp, _vp, _vp, _i, _vp, _i64, _f, _f, _f, _f, _i, _vp]),
    "tdx_adam_step": (_i, [_vp, _vp, _vp, _i, _vp, _i64] + [C.c_double] * 5 + [_i, _i, _vp]),
    "tdx_adam_step_scaled": (_i, [_vp, _vp, _vp, _i, _vp, _i64] + [C.c_double] * 5 + [_i, _i, _vp]),
}

FILM_MAX_LAYERS = 32  # TDX_FILM_MAX_LAYERS


class FilmLayer(C.Structure):  # TdxFilmLayer
    _fields_ = [("weight", _vp), ("bias", _vp), ("out", _vp), ("channels", _i)]


class PackJob(C.Structure):  # TdxPackJob
    _fields_ = [("w", _vp), ("wf", _vp), ("wb", _vp), ("Cin", _i), ("Cout", _i)]


class TransposeJob(C.Structure):  # TdxTransposeJob
    _fields_ = [("src", _vp), ("dst", _vp), ("rows", _i), ("cols", _i)]


class StageItem(C.Structure):  # TdxStageItem
    _fields_ = [("src", _vp), ("dst", _vp), ("n", _i64)]


class FilmGrad(C.Structure):  # TdxFilmGrad
    _fields_ = [("weight", _vp), ("grad_out", _vp), ("grad_weight", _vp), ("grad_bias", _vp), ("channels", _i)]


class ConvgEpilogue(C.Structure):  # TdxConvgEpilogue
    _fields_ = [("relu", _i), ("add0", _vp), ("add1", _vp), ("add_bcast", _i), ("h", _vp), ("out_f32", _i), ("x", _vp),
                ("x_next", _vp), ("inside", _vp), ("dx_mean", _vp), ("dx_std", _vp), ("F", _i)]


_lib = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP kernels have not been built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C generative-turbulence_amd/csrc`)."
            )
        lib = C.CDLL(str(LIB_PATH))
        lax = "TDX_LIB" in os.environ and os.environ.get("TDX_LIB_LAX") == "1"  # A/B runs against older builds
        for name, (res, args) in SIGNATURES.items():
            if lax and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


_SCRATCH: "OrderedDict" = None  # (device index, stream handle) -> arena tensor, least recently bound first
_ACTIVE = None  # key of the arena the library currently points at
SCRATCH_BYTES = int(os.environ.get("TDX_SCRATCH_MB", "96")) << 20
SCRATCH_SMALL_BYTES = 4096  # streams that only need the zero block at the arena's head (the weight-gradient side stream)
SCRATCH_MAX_ARENAS = int(os.environ.get("TDX_SCRATCH_MAX_ARENAS", "6"))
# entry points that may use the arena (K-split slabs of the small-grid kernels, the zero block of the DMA kernels)
ARENA_USERS = {"tdx_conv3_fwd", "tdx_conv3_fwd_gn", "tdx_conv3_fwd_partial", "tdx_conv3_bwd_data", "tdx_conv3_bwd_data_add",
               "tdx_conv3_bwd_data_skip", "tdx_conv3_bwd_weight", "tdx_attn_fwd"}  # tdx_attn_fwd: partial (O, m, l) of the stream-K schedule
# TDX_DETERMINISTIC=1: these merge their parameter gradients through per-split slabs in the launching stream's arena as well
DET_ARENA_USERS = {"tdx_conv1_bwd_weight", "tdx_conv1_bwd_weight_oc", "tdx_encode_bwd", "tdx_decode_bwd", "tdx_gn_stats"}


_SWITCH_INDEX = None  # name -> row of the library's switch table (the table is static; values are never kept)


def _switch_index() -> dict:
    global _SWITCH_INDEX
    if _SWITCH_INDEX is None:
        lib = load()
        _SWITCH_INDEX = {lib.tdx_switch_name(i).decode(): i for i in range(lib.tdx_switch_count())}
    return _SWITCH_INDEX


def switch_names() -> tuple:
    """The library's environment switches (its own table), in the table's order."""
    return tuple(_switch_index())


def switch(name: str) -> int:
    """What a launch issued now reads for the library switch `name`: parsed by the library, from the environment as it is now."""
    i = _switch_index()[name]
    return _lib.tdx_switch_value(i)


def switch_default(name: str) -> int:
    i = _switch_index()[name]
    return _lib.tdx_switch_default(i)


def deterministic() -> bool:
    """TDX_DETERMINISTIC=1 in the environment, as the library reads it (per call): run-to-run reproducible gradients."""
    return switch("TDX_DETERMINISTIC") != 0


# bind + launch of an arena user is one critical section: the library keeps ONE arena pointer per process and ctypes
# releases the GIL during a foreign call, so a second launching thread could otherwise re-bind between the two
_LAUNCH_LOCK = threading.RLock()
_SMALL_STREAMS = set()  # (device index, stream handle) of streams declared zero-block-only


def declare_zero_block_only(stream) -> None:
    """The given torch stream will only launch arena users that read the 16-byte zero block (tdx_conv3_bwd_weight):
    it gets a 4-KiB arena instead of TDX_SCRATCH_MB.  (torch draws stream handles from a pool of 32 per device and priority: a
    stream a caller creates much later can be the same handle -- its convs then run without the small-grid kernels, correct but
    on the brick kernels.  A high-priority side stream would avoid the collision but slows every kernel beside a live RCCL
    communicator -- ops._WgradSide, TDX_WGRAD_STREAM_PRIORITY.)"""
    _SMALL_STREAMS.add((stream.device.index, stream.cuda_stream))


def ensure_scratch(device=None) -> None:
    """Hand the library its scratch arena for (`device`, the CURRENT stream) -- tdx_set_scratch: K-split slabs of the
    small-grid conv kernels on the deep U-Net levels, zero block of the LDS-DMA kernels.  The library keeps ONE arena
    pointer per process and its kernels get it as a launch argument, so the binding is per launch: every stream that
    launches convs owns its own arena (a hipGraph captured on a side stream keeps replaying on that stream's arena while
    eager work on another stream uses another), and `call` re-binds whenever the launching stream changes.  At most
    TDX_SCRATCH_MAX_ARENAS arenas are kept (least recently bound dropped first; whoever captured a graph on an arena
    holds its tensor -- `scratch_arena()` -- so a dropped arena stays allocated while its graph lives; torch's pooled
    stream handles wrap around after 32 streams, which is why long-lived users keep ONE stream instead of making new ones).
    TDX_SCRATCH_MB=0: no arena (those layers then run on the brick kernels)."""
    global _SCRATCH, _ACTIVE
    if _SCRATCH is None:
        from collections import OrderedDict

        _SCRATCH = OrderedDict()
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    key = (idx, stream(idx))
    if _ACTIVE == key:
        return
    if SCRATCH_BYTES <= 0:
        load().tdx_set_scratch(None, 0)
        _ACTIVE = key
        return
    buf = _SCRATCH.get(key)
    if buf is None:
        nbytes = SCRATCH_SMALL_BYTES if key in _SMALL_STREAMS else SCRATCH_BYTES
        with torch.cuda.device(idx):
            buf = _SCRATCH[key] = torch.zeros(nbytes, dtype=torch.uint8, device=torch.device("cuda", idx))
        while len(_SCRATCH) > SCRATCH_MAX_ARENAS:
            _SCRATCH.popitem(last=False)
    else:
        _SCRATCH.move_to_end(key)
    rc = load().tdx_set_scratch(buf.data_ptr(), buf.numel())
    if rc != 0:
        raise RuntimeError(f"tdx_set_scratch failed: {rc}")
    _ACTIVE = key


def scratch_arena(device=None):
    """The arena tensor bound to (`device`, current stream), or None.  A graph captured on this stream must hold it."""
    ensure_scratch(device)
    return _SCRATCH.get(_ACTIVE) if _SCRATCH is not None else None


H16_DTYPES = (torch.bfloat16, torch.float16)  # 16-bit storage formats that share the matrix-core kernels


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16
    raise TypeError(f"tdx kernels support float32, bfloat16 and float16 activations, got {dt}")


_CONV_IMPLS = {"auto": CONV_AUTO, "direct": CONV_DIRECT, "mfma": CONV_MFMA, "split": CONV_SPLIT}
_conv_impl_override: str | None = None


def set_conv_impl(name: str | None) -> None:
    """Process-wide default of the 3x3x3 conv implementation ("auto", "direct", "mfma", "split"; None: "auto") for code
    that runs outside any model's conv_impl_scope and without TDX_CONV_IMPL.  "split" = split-precision MFMA convs on
    fp32 tensors."""
    global _conv_impl_override
    if name is not None and name not in _CONV_IMPLS:
        raise ValueError(f"unknown conv implementation {name!r}")
    _conv_impl_override = name


_conv_impl_scopes: list = []  # innermost model whose forward is running (DenoisingModel.conv_impl)


class conv_impl_scope:
    """`with conv_impl_scope(name):` -- the conv implementation of ONE model while its forward runs (name None: no-op).
    The autograd nodes created inside remember it for their backward, so two models with different arithmetic (an
    f32s trainer next to an f32 one) no longer share a process-wide switch."""

    def __init__(self, name: str | None):
        if name is not None and name not in _CONV_IMPLS:
            raise ValueError(f"unknown conv implementation {name!r}")
        self.name = name

    def __enter__(self):
        if self.name is not None:
            _conv_impl_scopes.append(self.name)

    def __exit__(self, *exc):
        if self.name is not None:
            _conv_impl_scopes.pop()


def conv_impl() -> int:
    """TDX_CONV_IMPL (the explicit test / benchmark knob) > the running model's own choice > set_conv_impl > "auto"."""
    env = os.environ.get("TDX_CONV_IMPL")
    if env:
        return _CONV_IMPLS[env]
    if _conv_impl_scopes:
        return _CONV_IMPLS[_conv_impl_scopes[-1]]
    return _CONV_IMPLS[_conv_impl_override or "auto"]


def pack_code(dt: torch.dtype) -> int:
    """dtype code for tdx_conv3_pack_weight: fp32 weights are packed as bf16 hi + lo images under
    TDX_CONV_IMPL=split (split-precision MFMA convs for fp32 tensors)."""
    if dt == torch.float32 and conv_impl() == CONV_SPLIT:
        return F32_SPLIT
    return dtype_code(dt)


def ptr(t: torch.Tensor | None):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("tdx kernels need device tensors (no CPU path exists in the product)")
    if not t.is_contiguous():
        raise RuntimeError("tdx kernels need contiguous tensors")
    return t.data_ptr()


# the launching stream's handle, ~700 times per training step: torch.cuda.current_stream() builds a Python Stream object
# per call (2.65 us measured), the raw query returns the same handle in a tenth of that
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream(device_index=None):
    if _raw_stream is None:
        return torch.cuda.current_stream(device_index).cuda_stream
    return _raw_stream(torch.cuda.current_device() if device_index is None else device_index)


_ERR = {-1: "TDX_EINVAL (bad argument)", -2: "TDX_ESHAPE (unsupported shape)", -3: "TDX_EDTYPE (unsupported dtype)"}


class KernelTimer:
    """HIP-event timing of selected entry points on the stream they are launched on
    (bench.py's roofline leg).  `work` is an optional per-call amount (flops or bytes)."""

    def __init__(self, names):
        self.names = set(names)
        self.records = []  # (name, start_event, end_event, work, meta)
        self.pending_work = 0.0

    def summary(self, where=None):
        """{name: launches / ms / work / bytes}; `where(meta)` selects records (meta = what the caller attached:
        e.g. the kernel family and the algorithmic bytes of a conv call)."""
        torch.cuda.synchronize()
        out = {}
        for name, s, e, work, meta in self.records:
            if where is not None and not where(meta or {}):
                continue
            d = out.setdefault(name, {"launches": 0, "ms": 0.0, "work": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["work"] += work
            d["bytes"] += (meta or {}).get("bytes", 0.0)
        return out


TIMER: KernelTimer | None = None


def call(name: str, *args, work: float = 0.0, meta=None):
    """meta: None, a dict, or a zero-argument callable returning one (evaluated only while a timer is attached)."""
    if name in ARENA_USERS or (name in DET_ARENA_USERS and deterministic()):
        with _LAUNCH_LOCK:
            ensure_scratch()  # the arena of the launching stream
            rc = _launch(name, args, work, meta)
    else:
        rc = _launch(name, args, work, meta)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {_ERR.get(rc, f'hipError {rc}')}")


def _launch(name, args, work, meta):
    t = TIMER
    if t is not None and name in t.names:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rc = getattr(load(), name)(*args)
        e.record()
        t.records.append((name, s, e, work, meta() if callable(meta) else meta))
        return rc
    return getattr(load(), name)(*args)


def query(name: str, *args) -> int:
    return int(getattr(load(), name)(*args))


def kernel_sources_fingerprint(pattern: str = "tdx_conv*") -> str | None:
    """sha256 (16 hex digits) over the conv kernels' sources next to the library (csrc/tdx_conv*.hip|h, in name order):
    what a committed profile describes.  tools/summarize_profiles.py stores it in profiles/*_traffic.json and bench.py
    quotes `roofline.traffic` only from a file whose fingerprint equals the tree's."""
    import hashlib

    src = _HERE.parent / "csrc"
    files = sorted(f for f in src.glob(pattern) if f.suffix in (".hip", ".h"))
    if not files:
        return None
    h = hashlib.sha256()
    for f in files:
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


KERNEL_DIRECT, KERNEL_BRICK, KERNEL_SMALL, KERNEL_RING = 0, 1, 2, 3  # TDX_KERNEL_* (tdx_conv3_fwd_kernel)


# TDX_WGRAD_* (tdx_conv3_bwd_weight_plan)
WGRAD_DIRECT, WGRAD_BRICK16, WGRAD_SMALL, WGRAD_RING, WGRAD_BRICK_F32, WGRAD_SPLIT, WGRAD_SPLIT_RING = range(7)
WGRAD_KERNELS = ("direct", "brick16", "small", "ring", "brick_f32", "split", "split_ring")
WGRAD_PLAN_INTS = 16  # TDX_WGRAD_PLAN_INTS
# TDX_WGRAD_PLAN_*: index of each field in the plan array
WGRAD_PLAN_FIELDS = ("kernel", "tile", "depth", "nsplit", "nslab", "sum_unpack", "nbg", "xs", "gx", "ngroups", "max_slabs", "nbricks", "order")


def conv3_bwd_weight_plan(C1, C2, Cout, B, X, Y, Z, dtype: int, impl: int) -> dict:
    """What tdx_conv3_bwd_weight would launch for this call, as the library's own host code plans it: {"status": the code
    that call would return, "kernel": a name of WGRAD_KERNELS, and the other WGRAD_PLAN_FIELDS}.  Launches nothing; reads the
    library switches from the environment as it is now and whether an arena is bound (`call` binds the launching stream's
    before the launch: bind it first -- ensure_scratch -- to ask about a call on this stream)."""
    buf = (C.c_int * WGRAD_PLAN_INTS)()
    status = int(load().tdx_conv3_bwd_weight_plan(C1, C2, Cout, B, X, Y, Z, dtype, impl, buf))
    plan = {k: int(buf[i]) for i, k in enumerate(WGRAD_PLAN_FIELDS)}
    plan["kernel"] = WGRAD_KERNELS[plan["kernel"]]
    plan["status"] = status
    return plan


CONV1_KERNELS = ("vector", "h16", "f32")  # TDX_CONV1_*
CONV1_PLAN_INTS = 8  # TDX_CONV1_PLAN_INTS
CONV1_PLAN_FIELDS = ("kernel", "nt", "tile_rows", "mt", "nsplit", "nslab", "step_rows", "rows_per_split")  # TDX_CONV1_PLAN_*


def _conv1_plan(entry, fields, *args) -> dict:
    buf = (C.c_int * CONV1_PLAN_INTS)()
    status = int(getattr(load(), entry)(*args, buf))
    plan = {k: int(buf[CONV1_PLAN_FIELDS.index(k)]) for k in fields}
    plan["kernel"] = CONV1_KERNELS[plan["kernel"]]
    plan["status"] = status
    return plan


def conv1_fwd_plan(C1, C2, Cout, ldw, w_mod16, has_add, gn_tail, dtype: int) -> dict:
    """What tdx_conv1_fwd (gn_tail: tdx_conv1_fwd_gn) would launch for this call, as the library's own route decides it:
    {"status": the code that call would return, "kernel": a name of CONV1_KERNELS, "nt", "tile_rows"}.  w_mod16: the address
    of w modulo 16.  Launches nothing; reads the library switches from the environment as it is now."""
    return _conv1_plan("tdx_conv1_fwd_plan", CONV1_PLAN_FIELDS[:3], C1, C2, Cout, ldw, w_mod16, int(has_add), int(gn_tail), dtype)


def conv1_bwd_weight_plan(Cin, Cout, rows, transposed, dtype: int) -> dict:
    """What tdx_conv1_bwd_weight (transposed: tdx_conv1_bwd_weight_oc) would launch, as the library's own host code plans it:
    {"status", "kernel", and the other CONV1_PLAN_FIELDS but "tile_rows"}.  Launches nothing; reads the library switches as of
    now and the bound arena's size (under TDX_DETERMINISTIC `call` binds the launching stream's before the launch: bind it
    first -- ensure_scratch -- to ask about a call on this stream)."""
    fields = CONV1_PLAN_FIELDS[:2] + CONV1_PLAN_FIELDS[3:]
    return _conv1_plan("tdx_conv1_bwd_weight_plan", fields, Cin, Cout, rows, int(transposed), dtype)


RESIZE_FWD_KERNELS = ("gather", "pairs")  # TDX_RESIZE_GATHER, TDX_RESIZE_PAIRS
RESIZE_BWD_KERNELS = ("tiled", "generic")  # TDX_RESIZE_TILED, TDX_RESIZE_GENERIC
RESIZE_PLAN_INTS = 18  # TDX_RESIZE_PLAN_INTS
RESIZE_PLAN_FIELDS = ("fwd_kernel", "fwd_tx", "fwd_ty", "fwd_tz", "fwd_nx", "fwd_ny", "fwd_nz", "bwd_kernel", "bwd_k", "bwd_tx",
                      "bwd_ty", "bwd_tz", "bwd_nx", "bwd_ny", "bwd_nz", "span_x", "span_y", "span_z")  # TDX_RESIZE_PLAN_*


def resize_plan(B, C, src, dst, dtype: int) -> dict:
    """What tdx_resize_fwd and tdx_resize_bwd would launch for x (B, *src, C) -> y (B, *dst, C), as the library's own host
    function plans both: {"status": the code those calls would return, "fwd_kernel": a name of RESIZE_FWD_KERNELS,
    "bwd_kernel": a name of RESIZE_BWD_KERNELS, and the other RESIZE_PLAN_FIELDS}.  Launches nothing."""
    buf = (_i * RESIZE_PLAN_INTS)()  # `C` is the channel count here, not ctypes
    status = int(load().tdx_resize_plan(B, *src, *dst, C, dtype, buf))
    plan = {k: int(buf[i]) for i, k in enumerate(RESIZE_PLAN_FIELDS)}
    plan["fwd_kernel"] = RESIZE_FWD_KERNELS[plan["fwd_kernel"]]
    plan["bwd_kernel"] = RESIZE_BWD_KERNELS[plan["bwd_kernel"]]
    plan["status"] = status
    return plan


ATTN_KERNELS = ("vector", "mfma")  # TDX_ATTN_VECTOR, TDX_ATTN_MFMA
ATTN_PLAN_INTS = 13  # TDX_ATTN_PLAN_INTS
ATTN_PLAN_FIELDS = ("fwd", "bwd", "nqb", "ntile", "nwg", "chunk", "streamk", "bound", "tw_dq", "tw_dkv", "bwd_gx", "bwd_gy",
                    "workspace")  # TDX_ATTN_PLAN_*


def attn_plan(B, N, H, D, dtype: int) -> dict:
    """What tdx_attn_fwd and tdx_attn_bwd would launch for qkv (B, N, 3 H D), as the library's own host function plans both:
    {"status": the code those calls would return, "fwd" and "bwd": names of ATTN_KERNELS, and the other ATTN_PLAN_FIELDS
    (0 where they do not apply; all 0, family "vector", unless the status is 0)}.  Launches nothing; reads the library switches
    as of now and the bound arena's size (`call` binds the launching stream's before tdx_attn_fwd: bind it first --
    ensure_scratch -- to ask about a call on this stream)."""
    buf = (_i * ATTN_PLAN_INTS)()
    status = int(load().tdx_attn_plan(B, N, H, D, dtype, buf))
    plan = {k: int(buf[i]) for i, k in enumerate(ATTN_PLAN_FIELDS)}
    plan["fwd"], plan["bwd"] = ATTN_KERNELS[plan["fwd"]], ATTN_KERNELS[plan["bwd"]]
    plan["status"] = status
    return plan


def conv3_fwd_meta(C1, C2, Cout, B, X, Y, Z, dt, real=None):
    """Bookkeeping of one forward conv call for the timers: the kernel family that serves it and its algorithmic HBM
    bytes (input + output + weights once; `real` = input channels that carry data)."""
    es = 2 if dt in H16_DTYPES else 4
    cin = real or (C1 + C2)
    return {"kind": query("tdx_conv3_fwd_kernel", C1, C2, Cout, B, X, Y, Z, dtype_code(dt), conv_impl()),
            "bytes": float((cin + Cout) * B * X * Y * Z * es + 27 * cin * Cout * es)}
