"""ctypes binding of the C ABI in include/pevit_hip.h.

The HIP library is the product: there is no CPU or PyTorch fallback behind these calls.  If
``libpevit_hip.so`` is missing or fails to load, importing the engine raises -- build it with
``python -c 'import __graft_entry__ as g; g.build()'`` (or ``make -C pevit_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpevit_hip.so")

c_void_p, c_int, c_float, c_size_t, c_char_p = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_char_p


class PevitDims(C.Structure):
    _fields_ = [("width", C.c_int32), ("layers", C.c_int32), ("patch", C.c_int32), ("resolution", C.c_int32),
                ("out_dim", C.c_int32), ("method", C.c_int32), ("lora_rank", C.c_int32),
                ("num_classes", C.c_int32), ("weight_format", C.c_int32)]


GEMM_KNOBS = ("config", "stagger", "big", "ksplit", "ksplit_small", "ksplit_stagger", "ksplit_mink", "kphase_nl", "kz2", "skinny",
              "skinny_slices", "streamk", "persistent")           # enum pevit_gemm_knob


class PevitTextDims(C.Structure):
    """pevit_text_dims of include/pevit_hip.h"""
    _fields_ = [(n, C.c_int32) for n in ("width", "layers", "context_length", "vocab_size", "out_dim", "weight_format")]


class PevitGemmExArgs(C.Structure):
    """pevit_gemm_ex_args of include/pevit_hip.h (the test-only pevit_op_gemm_ex); zero-initialised = nothing set"""
    _fields_ = ([(n, c_void_p) for n in ("A", "B", "B2", "bias", "resid", "bscale", "oscale", "out_f32", "out_f32_2", "out_bf16",
                                         "out2_bf16", "aux_bf16", "sk_slab", "sk_flag")] +
                [("head_stride", c_size_t)] +
                [(n, C.c_int32) for n in ("epilogue", "M", "N", "K", "lda", "ldb", "b_rows", "ldb2", "b2_rows", "n_fp8", "b_fp8", "a_fp8",
                                          "ldr", "ldo", "ldo2", "ldob", "ldob2", "ldaux", "E", "H", "tokens", "sk_slots")] +
                [("tune_set", C.c_uint32), ("tune", C.c_int32 * len(GEMM_KNOBS))])

    def set_tune(self, **knobs):
        for k, v in knobs.items():
            i = GEMM_KNOBS.index(k)
            self.tune[i] = v
            self.tune_set |= 1 << i


class PevitGemmPlanInfo(C.Structure):
    """pevit_gemm_plan_info of include/pevit_hip.h (pevit_debug_gemm_plan)"""
    _fields_ = ([(n, C.c_int32) for n in ("path", "ops", "cfg", "wm", "nl", "stag", "tiles", "grid", "band", "sk_share", "sk_band",
                                          "tiles_n", "nslices", "ksl")] + [("err", C.c_char * 160)])


class PevitAdapterFwdArgs(C.Structure):
    """pevit_adapter_fwd_args of include/pevit_hip.h (the test-only pevit_op_adapter_fwd_ex); zero-initialised = nothing set"""
    _fields_ = ([(n, c_void_p) for n in ("hraw", "bpr", "x_mid", "gamma", "beta", "wd", "b_down", "wu", "b_up", "z", "mean_a",
                                         "rstd_a", "act", "apre", "x_out")] +
                [(n, C.c_int32) for n in ("act_kind", "T", "E")])


class PevitAdapterBwdArgs(C.Structure):
    """pevit_adapter_bwd_args of include/pevit_hip.h (the test-only pevit_op_adapter_bwd_ex); zero-initialised = nothing set"""
    _fields_ = ([(n, c_void_p) for n in ("dyb", "dres", "wuT", "saved", "wdT", "hraw", "bpr", "mean_a", "rstd_a", "gamma", "dpre",
                                         "dh_bf16", "partial", "tn_x1", "tn_y1", "tn_partial1", "tn_x2", "tn_y2", "tn_partial2",
                                         "tn_csy2")] +
                [(n, C.c_int32) for n in ("act_kind", "T", "E", "tn_blocks")])


class PevitAdapterSeg(C.Structure):
    """pevit_adapter_seg of include/pevit_hip.h: one segment (rows [first, end) and its operands) of pevit_op_adapter_fwd_seg"""
    _fields_ = ([(n, C.c_int32) for n in ("first", "end")] +
                [(n, c_void_p) for n in ("gamma", "beta", "wd", "b_down", "wu", "b_up")])


class PevitAdapterFwdSegArgs(C.Structure):
    """pevit_adapter_fwd_seg_args of include/pevit_hip.h (the test-only pevit_op_adapter_fwd_seg); zero-initialised = nothing set"""
    _fields_ = ([(n, c_void_p) for n in ("hraw", "bpr", "x_mid", "x_out")] + [("segs", C.POINTER(PevitAdapterSeg))] +
                [(n, C.c_int32) for n in ("act_kind", "E", "nseg")])


class PevitSegment(C.Structure):
    """pevit_segment of include/pevit_segments.h: one segment of pevit_predict_segments"""
    _fields_ = [(n, C.c_int32) for n in ("first", "count", "slot")] + [(n, c_void_p) for n in ("running_mean", "running_var", "logits", "features")]


class PevitOpSegment(C.Structure):
    """pevit_op_segment of include/pevit_hip.h (the test-only pevit_op_delta_add_seg / pevit_op_attn_fwd_delta_seg)"""
    _fields_ = [(n, C.c_int32) for n in ("first", "count", "tcol")] + [(n, c_void_p) for n in ("q16", "bias")]


LOWRANK_FORMS = {"u": 0, "grad": 1, "combo": 2, "u_f32": 3, "grad_f32": 4}       # enum pevit_lowrank_form


class PevitLowrankArgs(C.Structure):
    """pevit_lowrank_args of include/pevit_hip.h (the test-only pevit_op_lowrank_ex); zero-initialised = nothing set"""
    _fields_ = ([(n, c_void_p) for n in ("dqkv", "qT", "q32", "u32", "u_bf16_cols", "xn", "t", "partial", "dbias_partial", "xn_prev",
                                         "u32_prev", "partial_prev")] +
                [(n, C.c_int32) for n in ("form", "ld", "ldx", "chunks", "B", "H", "N", "E", "xcd_order", "this_layer", "prev")])


class PevitPrepLowrankArgs(C.Structure):
    """pevit_prep_lowrank_args of include/pevit_hip.h (the test-only pevit_op_prep_lowrank); zero-initialised = nothing set"""
    _fields_ = ([(n, c_void_p) for n in ("rule1_l", "rule1_r", "rule2_l", "rule2_r", "q_left", "q_right", "a1q", "a2q", "a1v", "a2v",
                                         "w_aug_rows", "wT_aug_cols", "q32", "qT", "q16")] +
                [(n, c_size_t) for n in ("arena_bytes", "param_floats")] +
                [(n, C.c_int32) for n in ("method", "layers", "E", "r", "f32", "ldw", "ldwT")] + [("ascale", c_float)])


class PevitChainLowrankArgs(C.Structure):
    """pevit_chain_lowrank_args of include/pevit_hip.h (the test-only pevit_op_chain_lowrank); zero-initialised = nothing set"""
    _fields_ = ([(n, c_void_p) for n in ("partial", "dbias_partial", "G", "rule_scratch", "params", "grads")] +
                [(n, c_size_t) for n in ("partial_layer", "dbias_layer", "p_layer0", "p_layer_stride")] +
                [(n, C.c_int32) for n in ("method", "chunks", "layers", "E", "r")] + [("ascale", c_float)])


class PevitHeadArgs(C.Structure):
    """pevit_head_args of include/pevit_hip.h (the test-only pevit_op_head_ex); zero-initialised = nothing set"""
    _fields_ = ([(n, c_void_p) for n in ("feat", "labels", "targets", "W", "bias", "gW", "gb", "running_mean", "running_var", "ybn",
                                         "rstd", "logits", "dlogits", "dybn", "loss", "dfeat", "dfeat_bf16")] +
                [(n, C.c_int32) for n in ("training", "B", "D", "Cc")])


class PevitOptimGroup(C.Structure):
    """pevit_optim_group of include/pevit_hip.h: one parameter group of pevit_optim_step (doubles: Python's scalars unrounded)"""
    _fields_ = [(n, C.c_double) for n in ("lr", "weight_decay", "momentum", "beta1", "beta2", "eps")] + [("nesterov", C.c_int)]


class PevitProbeArgs(C.Structure):
    """pevit_probe_args of include/pevit_hip.h (pevit_probe_step); zero-initialised = nothing set"""
    _fields_ = ([("feat", c_void_p), ("rows", C.c_int64), ("index", c_void_p), ("labels", c_void_p), ("targets", c_void_p),
                 ("running_mean", c_void_p), ("running_var", c_void_p), ("logits", c_void_p), ("loss", c_void_p)] +
                [(n, C.c_int) for n in ("batch", "bn_training", "update", "flags")] +
                [(n, C.c_float) for n in ("scale", "lr", "momentum", "weight_decay")])


class PevitProbePredictArgs(C.Structure):
    """pevit_probe_predict_args of include/pevit_hip.h (pevit_probe_predict)"""
    _fields_ = [("feat", c_void_p), ("rows", C.c_int64), ("index_or_null", c_void_p), ("first_row", C.c_int64), ("count", C.c_int),
                ("running_mean", c_void_p), ("running_var", c_void_p), ("scale", C.c_float), ("logits", c_void_p)]


class PevitResizeRaggedDesc(C.Structure):
    """pevit_resize_ragged_desc of include/pevit_hip.h: one image of a ragged set (40 bytes; preprocess.RAGGED_DESC is its numpy twin)"""
    _fields_ = [("offset", C.c_int64)] + [(n, C.c_int32) for n in ("h", "w", "kh_off", "bh_off", "ksize_h", "kv_off", "bv_off", "ksize_v")]


class PevitResizeRaggedArgs(C.Structure):
    """pevit_resize_ragged_args of include/pevit_hip.h (pevit_resize_ragged_u8); zero-initialised = nothing set"""
    _fields_ = [("pool", c_void_p), ("pool_bytes", C.c_int64), ("desc", c_void_p), ("k_pool", c_void_p), ("k_len", C.c_int64),
                ("b_pool", c_void_p), ("b_len", C.c_int64), ("index", c_void_p), ("dst", c_void_p)] + \
               [(n, C.c_int32) for n in ("n_images", "batch", "out", "max_ksize_v")]


OPTIM_KINDS = {"sgd": 0, "adam": 1, "adamw": 2}           # enum pevit_optim_kind
OPTIM_MAX_GROUPS = 8                                       # PEVIT_OPTIM_MAX_GROUPS
OPTIM_NO_GRAD = 255                                        # group_of value of an element whose parameter has .grad None

WEIGHT_FORMATS = {"bf16": 0, "fp8": 1, "f32-verify": 2, "fp8-act": 3}


METHOD_IDS = {"kadaptation": 0, "lora": 1, "adapter": 2, "compacter": 3, "none": 4}

P = c_void_p
# name -> (restype, argtypes); mirrors include/pevit_hip.h one to one
SIGNATURES = {
    "pevit_last_error": (c_char_p, []),
    "pevit_version": (c_int, []),
    "pevit_ctx_create": (c_int, [C.POINTER(PevitDims), C.POINTER(c_void_p)]),
    "pevit_ctx_destroy": (None, [P]),
    "pevit_arena_bytes": (c_size_t, [P]),
    "pevit_workspace_bytes": (c_size_t, [P, c_int]),
    "pevit_workspace_state_bytes": (c_size_t, [P]),
    "pevit_num_tower_params": (c_size_t, [P]),
    "pevit_num_params": (c_size_t, [P]),
    "pevit_param_grad_mask": (c_int, [P, P, c_size_t]),
    "pevit_bind": (c_int, [P, P, c_size_t, P, c_size_t, c_int]),
    "pevit_set_params": (c_int, [P, P, P, P, P]),
    "pevit_load_block": (c_int, [P, P, c_int] + [P] * 12),
    "pevit_load_stem": (c_int, [P, P] + [P] * 8),
    "pevit_load_phm_rule": (c_int, [P, P, P]),
    "pevit_transformer_forward": (c_int, [P, P, P, P, c_int, c_int]),
    "pevit_transformer_backward": (c_int, [P, P, P, P, c_int]),
    "pevit_blocks_forward": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_blocks_backward": (c_int, [P, P, P, P, c_int, c_int, c_int]),
    "pevit_attention_forward": (c_int, [P, P, c_int, P, P, c_int, c_int, P, c_int]),
    "pevit_attention_backward": (c_int, [P, P, c_int, P, P, c_int]),
    "pevit_visual_forward": (c_int, [P, P, P, P, c_int, c_int]),
    "pevit_visual_backward": (c_int, [P, P, P, c_int]),
    "pevit_visual_backward_part": (c_int, [P, P, P, c_int, c_int, c_int]),
    "pevit_param_layer_offset": (c_size_t, [P, c_int]),
    "pevit_head_forward_backward": (c_int, [P, P, P, P, P, P, c_int, P, P, P, c_int]),
    "pevit_predict": (c_int, [P, P, P, P, P, P, P, c_int]),
    "pevit_predict_u8": (c_int, [P, P, P, P, P, P, P, c_int]),
    "pevit_encode_image": (c_int, [P, P, P, P, c_int]),
    "pevit_encode_image_u8": (c_int, [P, P, P, P, c_int]),
    "pevit_zeroshot": (c_int, [P, P, P, P, c_int, c_float, P, P, P, c_int]),
    "pevit_zeroshot_u8": (c_int, [P, P, P, P, c_int, c_float, P, P, P, c_int]),
    "pevit_infer_create": (c_int, [C.POINTER(PevitDims), C.POINTER(c_void_p)]),
    "pevit_set_infer_params": (c_int, [P, P, c_int]),
    "pevit_op_zeroshot_head": (c_int, [P, P, P, c_float, P, P, c_int, c_int, c_int]),
    "pevit_probe_step": (c_int, [P, P, C.POINTER(PevitProbeArgs)]),
    "pevit_probe_predict": (c_int, [P, P, C.POINTER(PevitProbePredictArgs)]),
    "pevit_text_create": (c_int, [C.POINTER(PevitTextDims), C.POINTER(c_void_p)]),
    "pevit_load_text_stem": (c_int, [P, P] + [P] * 5),
    "pevit_encode_text": (c_int, [P, P, P, P, c_int]),
    "pevit_zero_grads": (c_int, [P, P]),
    "pevit_sgd_step": (c_int, [P, P, c_float, c_float, c_float, c_float, c_int]),
    "pevit_set_optim_state": (c_int, [P, P, P]),
    "pevit_optim_step": (c_int, [P, P, c_int, C.POINTER(PevitOptimGroup), c_int, c_int, c_float, c_int]),
    "pevit_train_forward_backward": (c_int, [P, P, P, P, P, P, c_int, P, P, c_int]),
    "pevit_set_input_norm": (c_int, [P, P, P]),
    "pevit_visual_forward_u8": (c_int, [P, P, P, P, c_int, c_int]),
    "pevit_train_forward_backward_u8": (c_int, [P, P, P, P, P, P, c_int, P, P, c_int]),
    "pevit_resize_geometry": (c_int, [c_int, c_int, c_int] + [C.POINTER(c_int)] * 4),
    "pevit_resize_axis": (c_int, [c_int, c_int, c_int, c_int, P, P]),
    "pevit_resize_u8": (c_int, [P, P, c_int, c_int, c_int, P, c_int, c_int, P, P, c_int, P, P, c_int]),
    "pevit_resize_ragged_check": (c_int, [P, c_int, C.c_int64, C.c_int64, C.c_int64, c_int]),
    "pevit_resize_ragged_u8": (c_int, [P, C.POINTER(PevitResizeRaggedArgs)]),
    "pevit_head_forward_backward_bce": (c_int, [P, P, P, P, P, P, c_int, P, P, P, c_int]),
    "pevit_train_forward_backward_bce": (c_int, [P, P, P, P, P, P, c_int, P, P, c_int]),
    "pevit_train_forward_backward_bce_u8": (c_int, [P, P, P, P, P, P, c_int, P, P, c_int]),
    "pevit_profile_begin": (c_int, [P, c_int]),
    "pevit_profile_end": (c_int, [P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(c_int)]),
    "pevit_profile_launch": (c_int, [P, c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(c_int)]),
    "pevit_profile_launch_bytes": (c_int, [P, c_int, C.POINTER(C.c_double)]),
    "pevit_op_gemm": (c_int, [P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, c_int,
                              P, c_int, P, c_int, P, c_int, c_size_t, c_int, c_int, c_int]),
    "pevit_op_gemm_fp8": (c_int, [P, c_int, P, c_int, P, c_int, c_int, P, P, c_int, c_int, c_int, P, P, c_int, P, c_int,
                                  P, c_int, P, c_int, P, c_int, c_size_t, c_int, c_int, c_int]),
    "pevit_op_gemm_f8a": (c_int, [P, c_int, P, c_int, P, c_int, c_int, P, c_int, c_int, c_int, P, P, c_int, P, c_int, P, c_int,
                                  P, c_int, c_int, c_size_t, c_int, c_int, c_int]),
    "pevit_op_cast_fp8": (c_int, [P, P, P, c_int, c_int]),
    "pevit_debug_last_gemm_path": (c_int, []),
    "pevit_op_quant_fp8": (c_int, [P, P, c_int, c_int, P, P, P]),
    "pevit_op_dequant_fp8": (c_int, [P, P, P, c_int, c_int, P]),
    "pevit_op_ln_fwd": (c_int, [P, P, P, P, c_int, c_int, P, P, P, P]),
    "pevit_op_ln_bwd": (c_int, [P, P, P, P, P, P, P, P, P, c_int, c_int]),
    "pevit_op_ln_bwd_scaled": (c_int, [P, P, P, P, P, P, P, P, P, c_int, c_int, P]),
    "pevit_op_attn_fwd": (c_int, [P, P, P, P, P, c_int, P, c_int, c_int, c_int]),
    "pevit_op_attn_bwd": (c_int, [P, P, P, P, P, c_int, P, c_int, P, P, c_int, c_int, c_int, c_int]),
    "pevit_op_attn_fwd_causal": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_op_cast_bf16": (c_int, [P, P, P, c_size_t, c_float]),
    "pevit_op_delta_add": (c_int, [P, P, P, P, P, P, c_float, c_int, c_int, c_int]),
    "pevit_op_attn_fwd_delta": (c_int, [P, P, P, P, P, P, P, c_float, P, c_int, P, c_int, c_int, c_int]),
    "pevit_op_attn_delta_hpw": (c_int, [c_int, c_int, c_int]),
    "pevit_op_delta_add_seg": (c_int, [P, P, P, P, c_int, c_float, c_int, c_int, c_int, c_int, C.POINTER(PevitOpSegment)]),
    "pevit_op_attn_fwd_delta_seg": (c_int, [P, P, P, P, P, c_int, c_float, P, c_int, c_int, c_int, c_int, c_int, C.POINTER(PevitOpSegment)]),
    "pevit_op_attn_probs": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int]),
    # test-only forms (csrc/verify.hip; the GEMM ones csrc/ops.hip): the step-only members of the launchers' parameter structs
    "pevit_op_ln_fwd_ex": (c_int, [P, P, P, P, c_int, c_int, c_size_t, P, P, P, P, P]),
    "pevit_op_ln_bwd_ex": (c_int, [P, P, c_int, P, P, P, P, P, c_int, c_int, P, P, c_int, c_int, c_size_t, P, P]),
    "pevit_op_attn_fwd_ex": (c_int, [P, P, P, P, P, c_int, P, c_int, c_int, c_int, P]),
    "pevit_op_attn_bwd_ex": (c_int, [P, P, P, P, P, c_int, P, c_int, P, P, c_int, c_int, c_int, c_int, c_int]),
    "pevit_op_gemm_ex": (c_int, [P, C.POINTER(PevitGemmExArgs)]),
    "pevit_op_gemm_sk_slots": (c_int, []),
    "pevit_debug_gemm_plan": (c_int, [C.POINTER(PevitGemmExArgs), c_int, C.POINTER(PevitGemmPlanInfo)]),
    "pevit_debug_gemm_epi_traits": (c_int, [c_int]),
    "pevit_op_adapter_fwd_ex": (c_int, [P, C.POINTER(PevitAdapterFwdArgs)]),
    "pevit_op_adapter_bwd_ex": (c_int, [P, C.POINTER(PevitAdapterBwdArgs)]),
    "pevit_op_adapter_blocks": (c_int, [c_int]),
    "pevit_op_adapter_fused_ok": (c_int, [c_int]),
    "pevit_op_adapter_fwd_seg": (c_int, [P, C.POINTER(PevitAdapterFwdSegArgs)]),
    "pevit_op_lowrank_ex": (c_int, [P, C.POINTER(PevitLowrankArgs)]),
    "pevit_op_prep_lowrank": (c_int, [P, C.POINTER(PevitPrepLowrankArgs)]),
    "pevit_op_chain_lowrank": (c_int, [P, C.POINTER(PevitChainLowrankArgs)]),
    "pevit_op_rule_sum": (c_int, [P, P, P, c_int, c_int]),
    "pevit_op_lowrank_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, C.POINTER(C.c_int32)]),
    "pevit_op_head_ex": (c_int, [P, C.POINTER(PevitHeadArgs)]),
    "pevit_op_conv_weight": (c_int, [P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_op_cls_row": (c_int, [P, P, P, P, c_int, c_int, c_int]),
    "pevit_op_im2col_ex": (c_int, [P, P, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int]),
    "pevit_op_cast_ex": (c_int, [P, P, P, c_size_t, c_float, c_int]),
    "pevit_op_transpose": (c_int, [P, P, c_int, c_int, P, c_int, c_int, c_float, c_int]),
    "pevit_op_permute_rows": (c_int, [P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_op_zero": (c_int, [P, P, c_size_t]),
    "pevit_op_scale_f32": (c_int, [P, P, c_size_t, c_float]),
    "pevit_op_text_embed": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_op_text_eot_gather": (c_int, [P, P, P, P, c_int, c_int, c_int]),
    "pevit_debug_timeline": (c_int, [P]),
    "pevit_debug_occupy": (c_int, [P, c_int, c_int, C.c_double]),
    "pevit_op_lowrank_u": (c_int, [P, P, c_int, P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_op_lowrank_grad": (c_int, [P, P, c_int, P, P, c_int, P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_op_lowrank_chunks": (c_int, [c_int]),
    "pevit_op_tn_chunks": (c_int, [c_int]),
    "pevit_op_tn_gemm64": (c_int, [P, P, c_int, P, c_int, P, P, P, c_int, c_int]),
    "pevit_op_lna_blocks": (c_int, [c_int]),
    "pevit_op_ln_bwd_affine": (c_int, [P, P, P, P, P, P, P, P, P, P, c_int, c_int]),
    "pevit_op_colsum_reduce": (c_int, [P, P, c_int, c_int, P, P, P]),
    "pevit_op_prep_bottleneck": (c_int, [P, c_int, P, P, P, P, P, P, P, P, P, c_int]),
    "pevit_op_chain_bottleneck": (c_int, [P, c_int, P, P, P, P, P, c_int, c_size_t, c_size_t, c_size_t, c_size_t]),
    "pevit_op_im2col": (c_int, [P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_op_im2col_u8": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int]),
    "pevit_tune": (c_int, [P, c_char_p, c_int]),
    "pevit_ar_create": (c_int, [C.POINTER(c_void_p), c_int, c_int, c_size_t]),
    "pevit_ar_destroy": (None, [P]),
    "pevit_ar_handle_bytes": (c_int, []),
    "pevit_ar_export": (c_int, [P, P]),
    "pevit_ar_import": (c_int, [P, c_int, P]),
    "pevit_allreduce_flat": (c_int, [P, P, P, c_size_t]),
    "pevit_ar_error": (c_int, [P, P]),
    "pevit_ar_error_word": (c_void_p, [P]),
    "pevit_ar_fine_grained": (c_int, [P]),
    "pevit_ar_reset": (c_int, [P, P]),
    "pevit_set_external_poison": (c_int, [P, P]),
    "pevit_set_step_gate": (c_int, [P, P]),               # round 5: the fused step waits for this event behind its stem (pipelined DP)
    "pevit_streamk_error": (c_int, [P, P]),
    "pevit_streamk_status": (c_int, [P, P, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
}

# include/pevit_segments.h (which pevit_hip.h includes): the entry points of a multi-slot inference context, a table of their own
SEGMENT_SIGNATURES = {
    "pevit_infer_create_slots": (c_int, [C.POINTER(PevitDims), c_int, C.POINTER(c_void_p)]),
    "pevit_load_adapter_slot": (c_int, [P, P, c_int, P, c_int]),
    "pevit_predict_segments": (c_int, [P, P, P, c_int, c_int, C.POINTER(PevitSegment)]),
    "pevit_predict_segments_u8": (c_int, [P, P, P, c_int, c_int, C.POINTER(PevitSegment)]),
}
MAX_SLOTS, MAX_SEGMENTS = 8, 16          # PEVIT_MAX_SLOTS, PEVIT_MAX_SEGMENTS_PER_CALL

# include/pevit_segments_all.h (which pevit_hip.h includes): slot contexts for all four methods, a table of their own
SEGMENT_ALL_SIGNATURES = {
    "pevit_infer_create_slots_all": (c_int, [C.POINTER(PevitDims), c_int, C.POINTER(c_void_p)]),
    "pevit_load_adapter_slot_rule": (c_int, [P, P, c_int, P, c_int, P]),
}

# include/pevit_clip.h (which pevit_hip.h includes): gradient-norm clipping over the flat gradient buffer, a table of their own
CLIP_SIGNATURES = {
    "pevit_clip_scratch_floats": (c_size_t, [c_size_t]),
    "pevit_clip_grad_norm": (c_int, [P, P, c_float, c_float, P]),
    "pevit_op_clip_grad_norm": (c_int, [P, P, P, c_size_t, c_float, c_float, P]),
}

_lib = None


class PevitError(RuntimeError):
    pass


def load():
    """Load the shared library (once) and attach the signatures.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PevitError(
            f"{LIB_PATH} not found: the gfx950 HIP library has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback.")
    # torch first: its wheel carries its own libamdhip64; loaded AFTER this library (which would then pull the system runtime in)
    # the process holds two HIP runtimes, and the second one finds "no ROCm-capable device" (seen with `python __graft_entry__.py
    # smoke`, where build() loads the library before smoke() imports torch)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(SEGMENT_SIGNATURES.items()) + list(SEGMENT_ALL_SIGNATURES.items()) + \
            list(CLIP_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().pevit_last_error()
        raise PevitError(f"{what} failed: {msg.decode() if msg else 'unknown error'}")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
