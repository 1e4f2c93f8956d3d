"""ctypes binding of ``libclipmi.so`` (C ABI declared in ``include/clipmi.h``).

The HIP library is the product: there is no CPU or PyTorch fallback.  If the shared object is missing or a symbol
cannot be resolved this module raises at import time, and every wrapper raises ``ClipmiError`` on a non-zero
return code with the library's own error text.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CLIPMI_LIBRARY selects another BUILD of the same library (the tuning build with phase stamps); never a different backend
LIB_PATH = os.environ.get("CLIPMI_LIBRARY") or os.path.join(_HERE, "csrc", "libclipmi.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "clipmi.h")

ABI_VERSION = 16

OK, ERR_ARG, ERR_SHAPE, ERR_HIP, ERR_WORKSPACE, ERR_STATE = 0, -1, -2, -3, -4, -5
F16, F32 = 0, 1
_DT = {torch.float16: F16, torch.float32: F32}                  # the dtype argument of every entry point that takes fp16 or fp32
COMM_ID_BYTES = 128
EPI_NONE, EPI_BIAS, EPI_BIAS_QUICKGELU, EPI_BIAS_RESIDUAL, EPI_BIAS_RELU, EPI_BIAS_RESIDUAL16_RELU = 0, 1, 2, 3, 4, 5
CALL_DEFAULT, CALL_STREAM_F32, CALL_STREAM_F16 = 0, 1, 2   # per-call flags of the tower calls (include/clipmi.h)
FILTER_BILINEAR, FILTER_BICUBIC = 2, 3                      # clipmi_preprocess filters (Pillow's numbers)
PROMPT_COOP, PROMPT_KGCOOP, PROMPT_PROGRAD = 0, 1, 2        # `mode` of clipmi_prompt_head / clipmi_prompt_train_step (plain integers there)
OPTIM_SGD, OPTIM_ADAM = 0, 1                                # clipmi_taskres_train_step / clipmi_taskres_fit optimisers


class ClipmiError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str):
        super().__init__(f"{what} failed: {detail or '?'} (code {code})")
        self.code = code


class Geometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "embed_dim", "image_resolution", "patch_size", "vision_width", "vision_layers",
        "context_length", "vocab_size", "text_width", "text_layers", "text_heads")]


class BlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "ln1_g", "ln1_b", "w_qkv", "b_qkv", "w_out", "b_out", "ln2_g", "ln2_b", "w_fc", "b_fc", "w_proj", "b_proj",
        "w_qkv_f", "g_qkv", "c_qkv", "w_fc_f", "g_fc", "c_fc")]


class VisionWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "conv_w", "class_embedding", "positional_embedding", "ln_pre_g", "ln_pre_b", "ln_post_g", "ln_post_b",
        "proj_t")] + [("blocks", C.POINTER(BlockWeights))]


class TextWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "token_embedding", "positional_embedding", "ln_final_g", "ln_final_b", "proj_t")] + [
        ("blocks", C.POINTER(BlockWeights))]


class ImageDesc(C.Structure):
    """clipmi_image_desc: byte (y, x, c) of image b is pixels[offset + y*stride_y + x*stride_x + c*stride_c]."""
    _fields_ = [("offset", C.c_int64), ("height", C.c_int32), ("width", C.c_int32),
                ("stride_y", C.c_int64), ("stride_x", C.c_int64), ("stride_c", C.c_int64)]


class ViewDesc(C.Structure):
    """clipmi_view_desc: the box (top, left, height, width) of image ``image``, stretched to one output image; ``flip`` mirrors it."""
    _fields_ = [(n, C.c_int32) for n in ("image", "top", "left", "height", "width", "flip")]


class ProcalModel(C.Structure):
    """clipmi_procal_model: the fitted ProCal point sets as the kernels take them (include/clipmi.h)."""
    _fields_ = [("points_true", C.c_void_p), ("points_false", C.c_void_p), ("n_true", C.c_int32), ("n_false", C.c_int32),
                ("scale", (C.c_double * 2) * 2), ("norm", C.c_double * 2), ("ratio", C.c_double)]


ISOTONIC_MAX_TABLES = 8
ORDER_STATS_MAX_RANKS = 64     # CLIPMI_ORDER_STATS_MAX_RANKS
GROUP_GAP_MAX_GROUPS = 1024    # CLIPMI_GROUP_GAP_MAX_GROUPS


class IsotonicModel(C.Structure):
    """clipmi_isotonic_model: the packed threshold tables and the inner proximity-bin edges (include/clipmi.h)."""
    _fields_ = [("table", C.c_void_p), ("n_tables", C.c_int32), ("offset", C.c_int32 * (ISOTONIC_MAX_TABLES + 1)),
                ("edges", C.c_double * (ISOTONIC_MAX_TABLES - 1))]


class PromptHook(C.Structure):
    _fields_ = [("n_ctx", C.c_int32), ("n_deep", C.c_int32), ("shallow", C.c_void_p), ("deep", C.c_void_p)]


class BlockDgrad(C.Structure):
    """clipmi_block_dgrad: the transposed fp16 weights of one text block (include/clipmi.h)."""
    _fields_ = [("w_qkv_t", C.c_void_p), ("w_out_t", C.c_void_p), ("w_fc_t", C.c_void_p), ("w_proj_t", C.c_void_p)]


class TextDgrad(C.Structure):
    """clipmi_text_dgrad: text_projection as fp16 [Dt, E] and the blocks' transposed weights."""
    _fields_ = [("proj", C.c_void_p), ("blocks", C.POINTER(BlockDgrad))]


class ScalerState(C.Structure):
    """clipmi_scaler_state: the dynamic loss scale's device block, 20 bytes (include/clipmi.h)."""
    _fields_ = [("scale", C.c_float), ("growth_tracker", C.c_int32), ("skipped_steps", C.c_int32), ("applied_steps", C.c_int32),
                ("found_inf", C.c_int32)]


class VisionDgrad(C.Structure):
    """clipmi_vision_dgrad: visual.proj as fp16 [Dv, E] and the image blocks' transposed weights."""
    _fields_ = [("proj", C.c_void_p), ("blocks", C.POINTER(BlockDgrad))]


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: the HIP extension has not been built. Run `python -c 'import __graft_entry__ as g; "
        f"g.build()'` (or `make -C clip_calibration_amd/csrc`). There is no CPU fallback.")

lib = C.CDLL(LIB_PATH)

_vp, _i, _i64, _f, _sz, _u = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t, C.c_uint

_SIGNATURES = {
    "clipmi_abi_version": (C.c_int, []),
    "clipmi_strerror": (C.c_char_p, [_i]),
    "clipmi_last_error": (C.c_char_p, []),
    "clipmi_set_option": (_i, [C.c_char_p, _i]),
    "clipmi_get_option": (_i, [C.c_char_p, C.POINTER(_i)]),
    "clipmi_gemm_f16": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
    "clipmi_gemm_residual_f16": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, C.POINTER(_i), _i, _i, _i, _vp]),
    "clipmi_gemm_residual_fold": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, C.POINTER(_i), _i, _i, _i, _vp]),
    "clipmi_gemm_ln_fold": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i, _i64, _i, _i, _f, _vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
    "clipmi_layernorm": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _f, _vp]),
    "clipmi_attention": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "clipmi_attention_cls": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "clipmi_patchify": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "clipmi_patch_embed_scratch_bytes": (_sz, [_i, _i, _i]),
    "clipmi_patch_embed": (_i, [_vp, _i, _vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "clipmi_embed_ln": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "clipmi_l2_normalize": (_i, [_vp, _i, _vp, _i, _i, _vp]),
    "clipmi_logits": (_i, [_vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "clipmi_fused_tail_workspace_bytes": (_sz, [_i, _i]),
    "clipmi_l2_normalize_to": (_i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    "clipmi_comm_unique_id": (_i, [_vp]),
    "clipmi_comm_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "clipmi_comm_destroy": (_i, [_vp]),
    "clipmi_comm_ranks": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "clipmi_allgather": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "clipmi_fused_tail": (_i, [_vp, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _i, _i, _i, _vp]),
    "clipmi_calibrate_rows": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "clipmi_conv3x3_nhwc": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "clipmi_im2col3x3_nchw": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "clipmi_im2col3x3_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "clipmi_avgpool_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "clipmi_attnpool_tokens": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "clipmi_attnpool": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "clipmi_adapter_blend": (_i, [_vp, _vp, _vp, C.c_float, _vp, _i, _i, _i, _vp]),
    "clipmi_scale_add": (_i, [_vp, _vp, C.c_float, _vp, C.c_longlong, _vp]),
    "clipmi_group_mean": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "clipmi_cocoop_ctx": (_i, [_vp] * 7 + [_i] * 5 + [_vp]),
    "clipmi_cocoop_prompts": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "clipmi_logits_per_image": (_i, [_vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "clipmi_softmax_rows": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "clipmi_knn_dists": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "clipmi_nearest_rows": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "clipmi_nearest_rows_workspace": (_sz, [_i, _i, _i, _i]),
    "clipmi_nearest_rows_splits": (_i, [_i, _i]),
    "clipmi_ece_accumulate": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp]),
    "clipmi_procal_kde": (_i, [C.POINTER(ProcalModel), _vp, _vp, _vp, _i, _vp]),
    "clipmi_procal_rows": (_i, [C.POINTER(ProcalModel), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "clipmi_isotonic_pack": (_i, [_vp, _vp, _vp, _i, _vp]),
    "clipmi_isotonic_rows": (_i, [C.POINTER(IsotonicModel), _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "clipmi_isotonic_keys": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "clipmi_isotonic_gap_stats": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    "clipmi_tempscale_workspace_bytes": (_sz, [_i]),
    "clipmi_tempscale_batch": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_tempscale_fit": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _i, _i, _vp, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_pts_param_count": (_i, [_i, _i, _i]),
    "clipmi_pts_topk": (_i, [_vp, _i64, _i, _i, _i, _vp, _vp]),
    "clipmi_pts_apply": (_i, [_vp, _i64, _i, _i, _vp, _i, _i, _i, _vp, _i64, _vp, _vp]),
    "clipmi_pts_eval": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "clipmi_pts_fit": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _f, _f, _f, _i, C.c_double, C.c_double, C.c_double,
                            _vp, _vp, _vp, _sz, _vp]),
    "clipmi_adapter_train_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "clipmi_adapter_train_step": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp, _i, _f, _f, _f, _i, _vp, _vp, _sz, _vp]),
    "clipmi_adapter_fit": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _i, _f, _f, _f, _i, _vp,
                                _vp, _sz, _vp]),
    "clipmi_taskres_train_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_taskres_train_step": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _i, _i64, _f, _f, _f, _i, C.c_double,
                                       C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "clipmi_taskres_fit": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _i, _i64, _f, _f, _f, _i,
                                C.c_double, C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "clipmi_layernorm_backward": (_i, [_vp, _i64, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _f, _vp]),
    "clipmi_quickgelu_backward": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "clipmi_attention_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "clipmi_attention_backward_full": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "clipmi_attention_backward_long_bytes": (_sz, [_i, _i, _i]),
    "clipmi_attention_backward_long": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "clipmi_coop_head_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_coop_head": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_ctx_step": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _i, _f, _f, _f, _i, _vp]),
    "clipmi_text_train_bytes": (_i, [_vp, _i, _i, C.POINTER(_sz), C.POINTER(_sz)]),
    "clipmi_text_encoder_train": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _i, _i, C.POINTER(PromptHook), _vp, _vp, _sz, _vp, _sz, _u, _vp]),
    "clipmi_text_encoder_backward": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "clipmi_coop_train_step_bytes": (_sz, [_vp, _i, _i, _i]),
    "clipmi_coop_train_step": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i64, _vp, _i, _f, _f, _vp, _i, _f,
                                    _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_vision_train_bytes": (_i, [_vp, _i, _i, C.POINTER(_sz), C.POINTER(_sz)]),
    "clipmi_vision_encoder_train": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _u, _vp]),
    "clipmi_vision_encoder_backward": (_i, [_vp, C.POINTER(VisionDgrad), _vp, _i, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "clipmi_vpt_head_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_vpt_head": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_vpt_step": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _i, _f, _f, _f, _i, _vp]),
    "clipmi_vpt_train_step_bytes": (_sz, [_vp, _i, _i, _i]),
    "clipmi_vpt_train_step": (_i, [_vp, C.POINTER(VisionDgrad), _vp, _i, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _f, _f, _vp, _i, _f, _f, _f, _i, _vp, _vp,
                                   _vp, _sz, _vp, _sz, _vp]),
    "clipmi_text_encoder_train_deep": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _sz, _vp, _sz, _u, _vp]),
    "clipmi_text_encoder_backward_deep": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "clipmi_maple_block_floats": (_sz, [_i, _i, _i, _i]),
    "clipmi_maple_couple": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "clipmi_maple_head_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_maple_head": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_maple_step_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_maple_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _i, _f, _f, _f, _i, _vp, _sz, _vp]),
    "clipmi_maple_train_step_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "clipmi_maple_train_step": (_i, [_vp, C.POINTER(TextDgrad), C.POINTER(VisionDgrad), _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i,
                                     _f, _f, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_promptsrc_head_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_promptsrc_head": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_promptsrc_block_floats": (_sz, [_i, _i, _i, _i, _i, _i]),
    "clipmi_promptsrc_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _i, _f, _f, _f, _i, _vp]),
    "clipmi_gpa_accumulate": (_i, [_vp, _vp, _i64, _f, _i, _vp]),
    "clipmi_promptsrc_train_step_bytes": (_sz, [_vp, _i, _i, _i, _i, _i, _i]),
    "clipmi_promptsrc_train_step": (_i, [_vp, C.POINTER(TextDgrad), C.POINTER(VisionDgrad), _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i,
                                         _i, _i, _f, _f, _f, _f, _f, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_prompt_head_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "clipmi_prompt_head": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _f, _f, _i, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_prograd_step_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "clipmi_prograd_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _i, _f, _f, _f, _i, _vp, _sz, _vp]),
    "clipmi_prompt_train_step_bytes": (_sz, [_vp, _i, _i, _i, _i, _i, _i]),
    "clipmi_prompt_train_step": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i64, _vp, _i, _f, _f, _i, _vp, _f, _f,
                                      _f, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_grad_scale_rows": (_i, [_vp, _i, _i, _vp, _vp]),
    "clipmi_shard_compact": (_i, [_vp, _vp, _i, _i, _i64, _vp]),
    "clipmi_ctx_partial": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "clipmi_ctx_step_gathered": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _i, _i, _f, _vp, _i, _f, _f, _f, _i, _vp]),
    "clipmi_shard_prograd_workspace_bytes": (_sz, [_i64]),
    "clipmi_shard_prograd_dots": (_i, [_vp, _vp, _i, _i64, _i, _i, _i, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "clipmi_shard_prograd_apply": (_i, [_vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i, _f, _f, _f, _i, _vp, _sz, _vp]),
    "clipmi_block_rank_mean": (_i, [_vp, _i, _sz, _sz, _vp, _vp]),
    "clipmi_block_step_gathered": (_i, [_vp, _i, _sz, _sz, _f, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _i, _vp]),
    "clipmi_ctx_step_scaled_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "clipmi_ctx_step_scaled": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _f, _f, _i, _vp, _f, _f, _f, _i, _vp, _sz, _vp]),
    "clipmi_prompt_train_step_scaled_bytes": (_sz, [_vp, _i, _i, _i, _i, _i, _i]),
    "clipmi_prompt_train_step_scaled": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i64, _vp, _i, _f, _vp, _f, _f, _i,
                                             _i, _vp, _f, _vp, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_prompt_place": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "clipmi_prompt_unplace": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "clipmi_prompt_train_step_placed_bytes": (_sz, [_vp, _i, _i, _i, _i, _i, _i]),
    "clipmi_prompt_train_step_placed": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _i64, _vp, _i, _f, _f,
                                             _i, _vp, _f, _f, _f, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_prompt_train_step_scaled_placed_bytes": (_sz, [_vp, _i, _i, _i, _i, _i, _i]),
    "clipmi_prompt_train_step_scaled_placed": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _i64, _vp, _i, _f,
                                                    _vp, _f, _f, _i, _i, _vp, _f, _vp, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_block_step_scaled_workspace_bytes": (_sz, [_i64]),
    "clipmi_block_step_scaled": (_i, [_vp, _vp, _vp, _vp, _i64, _vp, _f, _f, _i, _vp, _f, _f, _f, _i, _vp, _sz, _vp]),
    "clipmi_block_step_adam": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _f, _vp, _i64, _vp, _i64, C.c_double, C.c_double, C.c_double, _f, _i, _vp]),
    "clipmi_block_step_adam_scaled_workspace_bytes": (_sz, [_i64]),
    "clipmi_block_step_adam_scaled": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _f, _f, _i, _vp, _vp, _i64, C.c_double, C.c_double, C.c_double, _f, _i,
                                           _vp, _sz, _vp]),
    "clipmi_cocoop_train_step_scaled_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "clipmi_cocoop_train_step_scaled": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i64, _vp, _i, _f, _vp, _f, _f, _i,
                                             _vp, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_vpt_train_step_scaled_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "clipmi_vpt_train_step_scaled": (_i, [_vp, C.POINTER(VisionDgrad), _vp, _i, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _f, _vp, _f, _f, _i, _vp, _f, _f, _f,
                                          _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_maple_train_step_scaled_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "clipmi_maple_train_step_scaled": (_i, [_vp, C.POINTER(TextDgrad), C.POINTER(VisionDgrad), _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i,
                                            _f, _vp, _f, _f, _i, _vp, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_promptsrc_train_step_scaled_bytes": (_sz, [_vp, _i, _i, _i, _i, _i, _i, _i]),
    "clipmi_promptsrc_train_step_scaled": (_i, [_vp, C.POINTER(TextDgrad), C.POINTER(VisionDgrad), _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                                _i, _i, _i, _i, _f, _vp, _f, _f, _i, _f, _f, _f, _vp, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp,
                                                _sz, _vp]),
    "clipmi_proda_embed": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "clipmi_proda_head_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "clipmi_proda_head": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_proda_ctx_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _i, _f, _f, _f, _i, _vp]),
    "clipmi_proda_train_step_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "clipmi_proda_train_step": (_i, [_vp, C.POINTER(TextDgrad), _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp, _i, _f, _f,
                                     _f, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_proda_ctx_step_scaled_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_proda_ctx_step_scaled": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _f, _i, _vp, _f, _f, _f, _i, _vp, _sz, _vp]),
    "clipmi_proda_train_step_scaled_bytes": (_sz, [_vp, _i, _i, _i, _i, _i, _i]),
    "clipmi_proda_train_step_scaled": (_i, [_vp, C.POINTER(TextDgrad), _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp, _i,
                                            _f, _vp, _f, _f, _i, _f, _vp, _f, _f, _f, _i, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_proda_embed_shard": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "clipmi_proda_shard_compact": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _vp]),
    "clipmi_proda_ctx_partial": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "clipmi_proda_ctx_step_gathered": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _f, _f, _f, _i, _vp]),
    "clipmi_proda_ctx_reduce_gathered_scaled": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _f, _f, _i, _vp, _f, _f, _f, _i, _vp, _sz, _vp]),
    "clipmi_cocoop_block_floats": (_sz, [_i, _i, _i, _i]),
    "clipmi_cocoop_meta": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "clipmi_cocoop_embed": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "clipmi_cocoop_head_workspace_bytes": (_sz, [_i, _i]),
    "clipmi_cocoop_head": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_cocoop_reduce_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "clipmi_cocoop_reduce": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "clipmi_cocoop_step": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _f, _f, _f, _i, _vp]),
    "clipmi_cocoop_embed_classes": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "clipmi_cocoop_shard_compact": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _vp]),
    "clipmi_cocoop_shard_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "clipmi_cocoop_dcs_partial": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "clipmi_cocoop_reduce_gathered": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "clipmi_cocoop_train_step_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "clipmi_cocoop_train_step": (_i, [_vp, C.POINTER(TextDgrad), _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i64, _vp, _i, _f, _f, _vp, _i, _f, _f, _f, _i,
                                      _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_order_stats_workspace_bytes": (_sz, [_i, _i]),
    "clipmi_order_stats": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_group_gap_accumulate": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp]),
    "clipmi_class_counts": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "clipmi_create": (_i, [C.POINTER(Geometry), C.POINTER(_vp)]),
    "clipmi_destroy": (_i, [_vp]),
    "clipmi_set_vision_weights": (_i, [_vp, C.POINTER(VisionWeights)]),
    "clipmi_set_text_weights": (_i, [_vp, C.POINTER(TextWeights)]),
    "clipmi_vision_workspace_bytes": (_sz, [_vp, _i, _i]),
    "clipmi_text_workspace_bytes": (_sz, [_vp, _i, _i]),
    "clipmi_model_set_option": (_i, [_vp, C.c_char_p, _i]),
    "clipmi_model_get_option": (_i, [_vp, C.c_char_p, C.POINTER(_i)]),
    "clipmi_encode_image": (_i, [_vp, _vp, _i, _i, C.POINTER(PromptHook), _vp, _vp, _sz, _u, _vp]),
    "clipmi_text_blocks": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(PromptHook), _vp, _sz, _u, _vp]),
    "clipmi_text_encoder": (_i, [_vp, _vp, _i, _vp, _i, _i, C.POINTER(PromptHook), _vp, _vp, _sz, _u, _vp]),
    "clipmi_encode_text": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _u, _vp]),
    "clipmi_profile_block": (_i, [_vp, _i, _i, _i, _vp, _sz, C.POINTER(_f), _vp]),
    "clipmi_encode_image_timed": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _u, C.POINTER(_f), _i, C.POINTER(_i), _vp]),
    "clipmi_preprocess_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "clipmi_preprocess": (_i, [_vp, _i64, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _sz, _vp]),
    "clipmi_augment_workspace_bytes": (_sz, [_vp, _i, _vp, _i, _i, _i]),
    "clipmi_augment": (_i, [_vp, _i64, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _sz, _vp]),
    "clipmi_probe_mfma_f16": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(_i), _vp]),
    "clipmi_val_score_workspace_bytes": (_sz, [_i, _i]),
    "clipmi_val_score": (_i, [_vp, _i64, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "clipmi_best_select_workspace_bytes": (_sz, [_i64]),
    "clipmi_best_select": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i64, _vp, _sz, _vp]),
    "clipmi_adapter_val_logits": (_i, [_vp, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp]),
    "clipmi_taskres_val_logits": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp]),
    "clipmi_adapter_fit_monitored_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_adapter_fit_monitored": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _i, _f, _f, _f, _i,
                                          _vp, _vp, _sz, _vp, _i64, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "clipmi_taskres_fit_monitored_workspace_bytes": (_sz, [_i, _i, _i]),
    "clipmi_taskres_fit_monitored": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _vp, _i, _i64, _f, _f, _f, _i,
                                          C.c_double, C.c_double, C.c_double, _vp, _vp, _sz, _vp, _i64, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _sz,
                                          _vp]),
    "clipmi_val_score_rows": (_i, [_vp, _i64, _vp, _i, _i, _i, _vp, _vp]),
    "clipmi_val_score_finish_workspace_bytes": (_sz, [_i, _i]),
    "clipmi_val_score_finish": (_i, [_vp, _i, _i, _vp, _vp, _sz, _vp]),
    "clipmi_vision_val_chunk_bytes": (_sz, [_vp, _i, _i, _i]),
    "clipmi_vision_val_chunk": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _f, _vp, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "clipmi_cocoop_val_rows": (_i, [_vp, _vp, _f, _vp, _i, _i, _i, _i, _vp, _vp]),
    "clipmi_cocoop_val_chunk_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "clipmi_cocoop_val_chunk": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _i, _f, _vp, _i, _vp, _u, _vp, _sz, _vp]),
    "clipmi_proda_val_mean": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "clipmi_proda_val_monitor_bytes": (_sz, [_i, _i, _i]),
    "clipmi_proda_val_logits_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "clipmi_proda_val_logits": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _u, _i, _vp, _i64, _vp, _i, _i, _vp, _i, _vp, _vp,
                                     _vp, _sz, _vp, _sz, _vp]),
    "clipmi_row_scores_acc_bytes": (_sz, [_i, _i]),
    "clipmi_row_scores": (_i, [_vp, _i64, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "clipmi_row_scores_finish_workspace_bytes": (_sz, [_i, _i]),
    "clipmi_row_scores_finish": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _sz, _vp]),
}

for _name, (_res, _args) in _SIGNATURES.items():
    try:
        _fn = getattr(lib, _name)
    except AttributeError as e:  # pragma: no cover
        raise ImportError(f"{LIB_PATH} does not export {_name}; rebuild the extension") from e
    _fn.restype = _res
    _fn.argtypes = _args

if lib.clipmi_abi_version() != ABI_VERSION:
    raise ImportError(f"{LIB_PATH}: ABI version {lib.clipmi_abi_version()} != {ABI_VERSION}; rebuild the extension")


def last_error() -> str:
    return (lib.clipmi_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc != OK:
        raise ClipmiError(rc, what, last_error() or (lib.clipmi_strerror(rc) or b"").decode())


def set_option(name: str, value: int) -> None:
    """Process-wide runtime switch (include/clipmi.h, clipmi_set_option): tests and A/B tools only -- product code selects
    precision per model (CLIP.set_option) or per call (flags), never through this."""
    check(lib.clipmi_set_option(name.encode(), int(value)), "clipmi_set_option")


def get_option(name: str) -> int:
    v = C.c_int(0)
    check(lib.clipmi_get_option(name.encode(), C.byref(v)), "clipmi_get_option")
    return v.value


class option:
    """``with option("ln_fold", 0): ...`` -- set a switch for a block and restore the previous value."""

    def __init__(self, name: str, value: int):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.prev)
        return False


_VARIANT_LETTERS = {"a": 10, "s": 13, "r": 16}


def gemm_variant_id(v) -> int:
    """'0' '1' / 'a' 's' 'r' (the CLIPMI_GEMM_VARIANT spellings) or an int -> option value; None -> -1."""
    if v is None:
        return -1
    if isinstance(v, int):
        return v
    return _VARIANT_LETTERS.get(v, None) if v in _VARIANT_LETTERS else int(v)


def exported_symbols():
    return sorted(_SIGNATURES)
