"""ctypes binding of the C ABI in include/dpc_hip.h.

The product path loads ``dpc_amd/libdpc_hip.so`` (gfx950 code objects, built by
``make`` / ``__graft_entry__.build()``) and raises if it is missing -- there is no
CPU or eager-PyTorch fallback.  ``load_emulator()`` exists for the CPU test tier
only (``tests/``): it loads the same kernel sources compiled against the host-side
SIMT simulator in ``tests/simt_emu`` and is never used by the engine on its own.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(_HERE, "libdpc_hip.so")
EMU_LIB_PATH = os.path.join(os.path.dirname(_HERE), "tests", "simt_emu", "libdpc_emu.so")

F32, BF16 = 0, 1
ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = -1, -2, -3   # DPC_ERR_* (include/dpc_hip.h)
ABI_VERSION = 2


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {dt}")


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dtype_in", "dtype_out", "mode", "N", "RT", "RH", "RW", "ST", "SH", "SW", "Ci", "src_ld",
        "Co", "ldw", "ldo", "KT", "KH", "KW", "st", "sh", "sw", "pt", "ph", "pw")]


class GruChainDesc(C.Structure):
    """struct dpc_gru_chain_desc (include/dpc_hip.h)"""
    _fields_ = ([(n, C.c_int32) for n in ("dtype", "M", "D", "SQ", "P", "n_agg", "n_steps", "reserved")] +
                [("p_drop", C.c_float), ("reserved2", C.c_uint32), ("seed", C.c_uint64)] +
                [(n, C.c_void_p) for n in ("step_dev", "drop_masks", "packed", "bias_u", "bias_r", "bias_o", "bias_1", "bias_2",
                                           "X_all", "H_all", "HR_all", "U_all", "R_all", "O_all", "P1_all", "pred",
                                           "d_pred", "G_all", "dP1", "dP2", "d_x", "ws", "d_hlast")])


class LcHeadDesc(C.Structure):
    """struct dpc_lc_head_desc (include/dpc_hip.h)"""
    _fields_ = ([(n, C.c_int32) for n in ("dtype", "B", "SQ", "D", "num_class", "train")] +
                [("p_drop", C.c_float), ("momentum", C.c_float), ("eps", C.c_float), ("reserved", C.c_uint32), ("seed", C.c_uint64)] +
                [(n, C.c_void_p) for n in ("step_dev", "drop_mask", "h_last", "bn_weight", "bn_bias", "bn_running_mean", "bn_running_var",
                                           "bn_num_batches", "fc_weight", "fc_bias", "target", "ctx", "xhat", "bn_out", "y", "stat",
                                           "logits", "dlogits", "row_ws", "result", "g_fc_weight", "g_fc_bias", "g_bn_weight",
                                           "g_bn_bias", "dctx", "d_hlast", "d_bn_out")])


class AdamSegment(C.Structure):
    """struct dpc_adam_segment (include/dpc_hip.h)"""
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("lr", C.c_float), ("weight_decay", C.c_float), ("active", C.c_int32),
                ("reserved", C.c_int32)]


ADAM_MAX_SEGMENTS = 512   # DPC_ADAM_MAX_SEGMENTS


class GradState(C.Structure):
    """struct dpc_grad_state (include/dpc_hip.h): the gradient guard's verdict, in device memory"""
    _fields_ = [("sumsq", C.c_double), ("norm", C.c_float), ("coef", C.c_float), ("skip", C.c_int32), ("n_skipped", C.c_int32),
                ("n_clipped", C.c_int32), ("reserved", C.c_int32)]


GRAD_PARTIALS = 1024   # DPC_GRAD_PARTIALS
ACCUM_ADD, ACCUM_FINISH = 0, 1   # DPC_ACCUM_* (include/dpc_hip.h): modes of dpc_grad_accumulate


class LambSegment(C.Structure):
    """struct dpc_lamb_segment (include/dpc_hip.h): one per parameter slot; chunk0 / n_chunks are filled by dpc_lamb_build_chunks"""
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("lr", C.c_float), ("weight_decay", C.c_float), ("active", C.c_int32),
                ("adapt", C.c_int32), ("chunk0", C.c_int32), ("n_chunks", C.c_int32), ("reserved", C.c_int32 * 2)]


class LambChunk(C.Structure):
    """struct dpc_lamb_chunk (include/dpc_hip.h)"""
    _fields_ = [("begin", C.c_int64), ("len", C.c_int32), ("seg", C.c_int32)]


class LambRecord(C.Structure):
    """struct dpc_lamb_record (include/dpc_hip.h): a segment's norms and trust ratio of the last LAMB step, in device memory"""
    _fields_ = [("sum_p2", C.c_double), ("sum_u2", C.c_double), ("pnorm", C.c_float), ("unorm", C.c_float), ("ratio", C.c_float),
                ("reserved", C.c_int32)]


LAMB_CHUNK = 4096   # DPC_LAMB_CHUNK

LR_CONSTANT, LR_COSINE, LR_LINEAR, LR_MULTISTEP = 0, 1, 2, 3   # DPC_LR_* (include/dpc_hip.h)
LR_MAX_MILESTONES = 8   # DPC_LR_MAX_MILESTONES


class LrSchedule(C.Structure):
    """struct dpc_lr_schedule (include/dpc_hip.h): host memory, passed to the kernel by value"""
    _fields_ = [("kind", C.c_int32), ("warmup_steps", C.c_int32), ("total_steps", C.c_int32), ("n_milestones", C.c_int32),
                ("min_mult", C.c_double), ("gamma", C.c_double), ("milestones", C.c_int32 * LR_MAX_MILESTONES)]


class LrState(C.Structure):
    """struct dpc_lr_state (include/dpc_hip.h): the multiplier of the last step taken, in device memory"""
    _fields_ = [("mult", C.c_float), ("k", C.c_int32), ("reserved", C.c_int32 * 2)]


class NegqState(C.Structure):
    """struct dpc_negq_state (include/dpc_hip.h): the negative queue's record, in device memory"""
    _fields_ = [("pushes", C.c_int32), ("filled", C.c_int32), ("reserved", C.c_int32 * 2)]


NEGQ_MAX_SLOTS = 64   # DPC_NEGQ_MAX_SLOTS


def negq_pitch(R: int) -> int:
    """DPC_NEGQ_PITCH (include/dpc_hip.h): rows of one slot of the ring"""
    return (R + 63) // 64 * 64


class NegClasses(C.Structure):
    """struct dpc_neg_classes (include/dpc_hip.h): geometry and class weights of dpc_ce_topk[_bf16]_cls, passed by value"""
    _fields_ = ([(n, C.c_int32) for n in ("B", "P", "SQ", "flags")] +
                [(n, C.c_float) for n in ("w_spatial", "w_temporal", "w_easy", "reserved")])


NEGCLS_MAX_WEIGHT = 65536.0   # DPC_NEGCLS_MAX_WEIGHT


def neg_class_weights(weights) -> tuple:
    """(w_S, w_T, w_E) as the three float32 values the launcher sees; ValueError for what it would refuse"""
    try:
        w = tuple(float(x) for x in weights)
    except (TypeError, ValueError):
        raise ValueError(f"negative-class weights must be three numbers (spatial, temporal, easy), got {weights!r}") from None
    if len(w) != 3:
        raise ValueError(f"negative-class weights must be three numbers (spatial, temporal, easy), got {weights!r}")
    for x in w:
        if not (x == x and 0.0 <= x <= NEGCLS_MAX_WEIGHT):
            raise ValueError(f"negative-class weights must be finite and within [0, {NEGCLS_MAX_WEIGHT:g}], got {weights!r}")
    return tuple(C.c_float(x).value for x in w)


class ConvEpilogue(C.Structure):
    """struct dpc_conv_epilogue (include/dpc_hip.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("addend", "addend_mask", "bn_raw", "bn_mask", "bn_mean", "bn_invstd", "stats")]


class Resample(C.Structure):
    """struct dpc_resample (include/dpc_hip.h)"""
    _fields_ = [("xb", C.c_void_p), ("xk", C.c_void_p), ("yb", C.c_void_p), ("yk", C.c_void_p), ("ksx", C.c_int32), ("ksy", C.c_int32)]


class RecipeDesc(C.Structure):
    """struct dpc_recipe_desc (include/dpc_hip.h)"""
    _fields_ = ([(n, C.c_double) for n in ("sized_p", "gray_p", "jitter_p", "brightness", "contrast", "saturation", "hue")] +
                [("flip_code", C.c_int32), ("flags", C.c_int32)])


RECIPE_JITTER_CONSISTENT, RECIPE_SCALE_AFTER_SIZED = 1, 2   # DPC_RECIPE_* (include/dpc_hip.h): bits of RecipeDesc.flags


def recipe_slots(n_frames: int) -> int:
    """DPC_RECIPE_SLOTS (include/dpc_hip.h): uniforms one clip of n_frames frames owns"""
    return 58 + 9 * n_frames


class PackEntry(C.Structure):
    """struct dpc_pack_entry (include/dpc_hip.h)"""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("d0", C.c_int32), ("d1", C.c_int32), ("d2", C.c_int32), ("block0", C.c_int32),
                ("s0", C.c_int64), ("s1", C.c_int64), ("s2", C.c_int64)]


class Copy2dEntry(C.Structure):
    """struct dpc_copy2d_entry (include/dpc_hip.h)"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_ld", C.c_int64), ("dst_ld", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32),
                ("block0", C.c_int32), ("pad", C.c_int32)]


class DpcError(RuntimeError):
    pass


_vp, _i32, _i64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
_SIGS = {
    "dpc_abi_version": [],
    "dpc_conv_stats_rows": [C.POINTER(ConvDesc)],
    "dpc_conv_igemm": [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp],
    "dpc_conv_igemm_ex": [C.POINTER(ConvDesc), _vp, _vp, _vp, C.POINTER(ConvEpilogue), _vp],
    "dpc_gemm_nt_splitk": [_i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, C.POINTER(_i32), _vp],
    "dpc_gemm_tn_splitk": [_i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, C.POINTER(_i32), _vp],
    "dpc_conv_wgrad": [C.POINTER(ConvDesc), _vp, _vp, _i32, _vp, C.POINTER(_i32), _vp],
    "dpc_conv_plan": [C.POINTER(ConvDesc), _i32, _i32, _i32, C.c_char_p, _i32],
    "dpc_last_kernel": [C.c_char_p, _i32],
    "dpc_set_reserved_cus": [_i32],
    "dpc_set_f32_matmul": [_i32],
    "dpc_diag_squat": [_i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp],
    "dpc_pack3d": [_vp, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _vp],
    "dpc_pack3d_multi": [_vp, _i32, _i32, _i32, _vp],
    "dpc_reduce_unpack": [_vp, _i32, _vp, _i32, _i32, _i32, _i64, _i64, _i64, _i32, _vp],
    "dpc_transpose2d_bf16x2": [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp],
    "dpc_transpose2d": [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp],
    "dpc_pack_input_s2d": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "dpc_synthetic_input": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, C.c_uint64, _vp, _vp],
    "dpc_synthetic_labels": [_vp, _i32, _i32, C.c_uint64, _vp, _vp],
    "dpc_pack_stem_weight": [_vp, _vp, _i32, _i32, _vp],
    "dpc_unpack_stem_wgrad": [_vp, _i32, _vp, _i32, _vp],
    "dpc_bn_finalize": [_vp, _i32, _i32, _f64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp],
    "dpc_bn_apply": [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "dpc_bn_bwd_reduce": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _i32, _vp, C.POINTER(_i32), _vp],
    "dpc_bn_bwd_finalize": [_vp, _i32, _i32, _f64, _vp, _vp, _vp, _vp],
    "dpc_bn_bwd_apply": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "dpc_bn_relu_maxpool_fwd": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "dpc_maxpool_bwd": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "dpc_tpool_split_fwd": [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "dpc_tpool_split_bwd": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "dpc_colsum": [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp],
    "dpc_pool_bn_bwd_reduce": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, C.POINTER(_i32), _vp],
    "dpc_pooled_bn_bwd_reduce": [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, C.POINTER(_i32), _vp],
    "dpc_pool_bn_bwd_apply": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "dpc_mask_gen": [_vp, _i32, _i32, _i32, _vp],
    "dpc_ce_topk": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp],
    "dpc_ce_topk_bf16": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp],
    "dpc_step_advance": [_vp, _vp, _f64, _f64, _vp],
    "dpc_adam_dev": [_vp, _vp, _vp, _vp, _i64, _f32, _f64, _f64, _f32, _f32, _vp, _f32, _vp],
    "dpc_adam_groups_dev": [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _f64, _f64, _f32, _vp, _f32, _vp],
    "dpc_grad_sumsq": [_vp, _i64, _vp, _i32, _vp, _vp],
    "dpc_grad_verdict": [_vp, _i32, _f64, _i32, _vp, _vp],
    "dpc_step_advance_gated": [_vp, _vp, _f64, _f64, _vp, _vp],
    "dpc_adam_dev_ex": [_vp, _vp, _vp, _vp, _i64, _f32, _f64, _f64, _f32, _f32, _vp, _f32, _vp, _vp],
    "dpc_adam_groups_dev_ex": [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _f64, _f64, _f32, _vp, _f32, _vp, _vp],
    "dpc_grad_scale": [_vp, _i64, _vp, _i32, _vp, _vp],
    "dpc_grad_accumulate": [_vp, _vp, _i64, _i64, _i64, _vp, _i32, _i32, _f32, _vp],
    "dpc_adam_dev_ema": [_vp, _vp, _vp, _vp, _i64, _f32, _f64, _f64, _f32, _f32, _vp, _f32, _vp, _vp, _vp, _f32, _vp],
    "dpc_adam_groups_dev_ema": [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _f64, _f64, _f32, _vp, _f32, _vp, _vp, _vp, _f32, _vp],
    "dpc_arena_swap": [_vp, _vp, _i64, _vp],
    "dpc_step_advance_sched": [_vp, _vp, _f64, _f64, _vp, C.POINTER(LrSchedule), _vp, _vp],
    "dpc_adam_dev_sched": [_vp, _vp, _vp, _vp, _i64, _f32, _f64, _f64, _f32, _f32, _vp, _f32, _vp, _vp, _vp, _f32, _vp, _vp],
    "dpc_adam_groups_dev_sched": [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _f64, _f64, _f32, _vp, _f32, _vp, _vp, _vp, _f32, _vp, _vp],
    "dpc_adamw_dev": [_vp, _vp, _vp, _vp, _i64, _f32, _f64, _f64, _f32, _f32, _vp, _f32, _vp, _vp, _vp, _f32, _vp, _vp],
    "dpc_adamw_groups_dev": [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _f64, _f64, _f32, _vp, _f32, _vp, _vp, _vp, _f32, _vp, _vp],
    "dpc_lamb_build_chunks": [C.POINTER(LambSegment), _i32, _i64, C.POINTER(LambChunk), _i32],
    "dpc_lamb_moments": [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _i32, _f64, _f64, _f32, _vp, _f32, _vp, _vp, _vp],
    "dpc_lamb_ratios": [_vp, _i32, _vp, _i32, _vp, _vp, _vp],
    "dpc_lamb_apply": [_vp, _vp, _vp, _i64, _vp, _i32, _vp, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp],
    "dpc_counter_advance": [_vp, _vp],
    "dpc_copy2d_f32": [_vp, _i64, _vp, _i64, _i32, _i32, _vp],
    "dpc_copy2d_multi": [_vp, _i32, _i32, _vp],
    "dpc_dropout_mask": [_vp, _i64, _f32, C.c_uint64, _vp, _vp],
    "dpc_gru_pack": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "dpc_gru_chain_fwd": [C.POINTER(GruChainDesc), _vp],
    "dpc_gru_chain_bwd": [C.POINTER(GruChainDesc), _vp],
    "dpc_score_ws_floats": [_i32, _i32, C.POINTER(_i64), C.POINTER(_i64)],
    "dpc_score_fwd": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "dpc_score_bwd": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp],
    "dpc_ce_finalize": [_vp, _i32, _vp, _vp],
    "dpc_negq_ws_floats": [_i32, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)],
    "dpc_negq_push": [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    "dpc_negq_clear": [_vp, _vp, _vp],
    "dpc_negq_fwd": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _i32, _vp, _vp, _vp],
    "dpc_negq_bwd": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "dpc_ce_topk_ext": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "dpc_ce_topk_bf16_ext": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "dpc_ce_topk_cls": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, NegClasses, _vp, _vp, _vp],
    "dpc_ce_topk_bf16_cls": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, NegClasses, _vp, _vp, _vp],
    "dpc_ce_sym_ws_floats": [_i32, _i32, C.POINTER(_i64)],
    "dpc_ce_colpass": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "dpc_ce_topk_sym": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _vp, _vp],
    "dpc_ce_topk_bf16_sym": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _vp, _vp],
    "dpc_rownorm_fwd": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _f32, _vp],
    "dpc_rownorm_bwd": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _f32, _vp],
    "dpc_bn_finalize_running": [_vp, _i32, _i32, _f64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp],
    "dpc_bn_eval_coeffs": [_vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _vp, _vp, _vp],
    "dpc_relu_tpool_fwd": [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "dpc_relu_tpool_bwd": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "dpc_lc_head_fwd": [C.POINTER(LcHeadDesc), _vp],
    "dpc_lc_head_bwd": [C.POINTER(LcHeadDesc), _vp],
    "dpc_frames_to_input": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32,
                            C.POINTER(C.c_float), C.POINTER(C.c_float), _vp, _vp, _i32, _vp],
    "dpc_frames_to_input_ex": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(Resample), _vp, _vp, _vp,
                               C.POINTER(C.c_float), C.POINTER(C.c_float), _vp, _vp, _i32, _vp],
    "dpc_video_windows_to_input": [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(Resample),
                                   C.POINTER(C.c_float), C.POINTER(C.c_float), _vp, _vp, _i32, _vp],
    "dpc_store_to_input": [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(Resample), _vp, _vp, _vp,
                           C.POINTER(C.c_float), C.POINTER(C.c_float), _vp, _vp, _i32, _vp, _vp],
    "dpc_draw_recipe": [C.POINTER(RecipeDesc), _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, C.c_uint64, _vp, _vp,
                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "dpc_draw_recipe_ex": [C.POINTER(RecipeDesc), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, C.c_uint64,
                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "dpc_lc_test_accumulate": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "dpc_lc_test_finish": [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "dpc_embed_accumulate": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "dpc_embed_finish": [_vp, _vp, _i32, _f32, _vp, _vp],
    "dpc_knn_ws_bytes": [_i32, _i32, _i32],
    "dpc_knn_topk": [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i64, _vp],
    "dpc_knn_recall": [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp],
    "dpc_stem_wgrad_fused": [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i32), _vp],
    "dpc_adam": [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _vp],
}


class Lib:
    """Loaded kernel library + thin checked wrappers (return codes -> DpcError)."""

    def __init__(self, path: str, kind: str):
        if not os.path.exists(path):
            raise DpcError(
                f"{path} not found: build it with `make` (or __graft_entry__.build()); "
                "dpc_amd has no CPU/eager fallback")
        self.kind = kind
        self.path = path
        self.c = C.CDLL(path)
        self._bound = {}
        if self.call("dpc_abi_version") != ABI_VERSION:
            raise DpcError("ABI version mismatch")

    def _fn(self, name: str):
        fn = self._bound.get(name)
        if fn is None:
            fn = getattr(self.c, name)  # AttributeError => ABI mismatch, loud by design
            fn.argtypes = _SIGS[name]
            fn.restype = C.c_int
            self._bound[name] = fn
        return fn

    def missing_symbols(self):
        return [n for n in _SIGS if not hasattr(self.c, n)]

    # -- stream handle for the device the tensors live on
    def stream(self) -> C.c_void_p:
        if self.kind == "hip":
            return C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return C.c_void_p(0)

    def call(self, name: str, *args) -> int:
        conv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        rc = self._fn(name)(*conv)
        if rc < 0:
            raise DpcError(f"{name} failed with code {rc}")
        return rc


PLAN_IGEMM, PLAN_WGRAD, PLAN_ADDEND, PLAN_STATS, PLAN_ADDEND_MASK, PLAN_BNRED = 0, 1, 1, 2, 4, 8


def conv_plan(lib: "Lib", desc: ConvDesc, op: int = PLAN_IGEMM, addend: bool = False, stats: bool = False, dy_ld: int = 0,
              addend_mask: bool = False, bnred: bool = False) -> str:
    """name of the kernel dpc_conv_igemm(_ex) / dpc_conv_wgrad would launch for `desc` (include/dpc_hip.h: dpc_conv_plan);
    "" when the combination is not supported (dpc_conv_igemm_ex returns DPC_ERR_UNSUPPORTED)"""
    buf = C.create_string_buffer(192)
    flags = ((PLAN_ADDEND if addend else 0) | (PLAN_STATS if stats else 0) | (PLAN_ADDEND_MASK if addend_mask else 0) |
             (PLAN_BNRED if bnred else 0))
    rc = lib._fn("dpc_conv_plan")(C.byref(desc), op, flags, dy_ld or desc.Co, buf, 192)
    if rc == -3:
        return ""
    if rc < 0:
        raise DpcError(f"dpc_conv_plan failed with code {rc}")
    return buf.value.decode()


def last_kernel(lib: "Lib") -> str:
    buf = C.create_string_buffer(192)
    lib.call("dpc_last_kernel", buf, 192)
    return buf.value.decode()


_HIP: Optional[Lib] = None
_EMU: Optional[Lib] = None


def load_hip() -> Lib:
    global _HIP
    if _HIP is None:
        _HIP = Lib(HIP_LIB_PATH, "hip")
    return _HIP


def load_emulator() -> Lib:
    """CPU functional simulator of the kernels -- tests only."""
    global _EMU
    if _EMU is None:
        _EMU = Lib(EMU_LIB_PATH, "emu")
    return _EMU


def lib_for(device: torch.device, emu: Optional[Lib] = None) -> Lib:
    if device.type == "cuda":
        return load_hip()
    if emu is not None and emu.kind == "emu":
        return emu
    raise DpcError("dpc_amd runs on MI355X only: tensors must live on a cuda (HIP) device")
