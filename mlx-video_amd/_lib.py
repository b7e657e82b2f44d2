"""ctypes binding of libltxk.so (include/ltxk.h).  Fails loudly when the HIP extension is
missing: there is no CPU fallback on the product path."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LTXK_LIB", os.path.join(_HERE, "libltxk.so"))


class LtxkError(RuntimeError):
    pass


class GemmArgs(Structure):
    _fields_ = [
        ("A", c_void_p), ("W", c_void_p), ("bias", c_void_p), ("out", c_void_p),
        ("resid", c_void_p), ("gate", c_void_p), ("gate_row", c_void_p),
        ("M", c_int32), ("N", c_int32), ("K", c_int32),
        ("lda", c_int32), ("ldo", c_int32), ("ldr", c_int32), ("gate_stride", c_int32),
        ("epilogue", c_int32), ("out_tokens_per_batch", c_int32), ("alpha", c_float),
        ("out2", c_void_p), ("n_split", c_int32), ("ldo2", c_int32), ("sumsq", c_void_p), ("sumsq_ld", c_int32),
        ("workspace", c_void_p), ("workspace_bytes", c_int64),
    ]


class GemmPlan(Structure):
    _fields_ = [
        ("form", c_int32), ("tile_rows", c_int32), ("tile_cols", c_int32),
        ("row_tiles", c_int32), ("col_tiles", c_int32), ("slices", c_int32), ("ksteps", c_int32),
    ]


class GemmGroupedArgs(Structure):
    _fields_ = [
        ("A", c_void_p), ("W", c_void_p), ("bias", c_void_p), ("out", c_void_p), ("out2", c_void_p), ("sumsq", c_void_p),
        ("out_gstride", c_int64), ("out2_gstride", c_int64), ("sumsq_gstride", c_int64),
        ("G", c_int32), ("M", c_int32), ("N", c_int32), ("K", c_int32),
        ("lda", c_int32), ("ldo", c_int32), ("ldo2", c_int32), ("sumsq_ld", c_int32),
        ("n_split", c_int32), ("out_tokens_per_batch", c_int32),
    ]


class GemmGroupedPlan(Structure):
    _fields_ = [
        ("tile_rows", c_int32), ("rem_rows", c_int32), ("row_tiles", c_int32), ("col_tiles", c_int32), ("tiles", c_int32),
    ]


class AttnArgs(Structure):
    _fields_ = [
        ("q", c_void_p), ("k", c_void_p), ("vt", c_void_p), ("out", c_void_p),
        ("ldq", c_int32), ("ldk", c_int32), ("ldvt", c_int32), ("ldo", c_int32),
        ("B", c_int32), ("H", c_int32), ("Tq", c_int32), ("Tk", c_int32), ("scale", c_float),
        ("q_sumsq", c_void_p), ("q_sumsq_ld", c_int32), ("q_sumsq_n", c_int32),
        ("q_norm_weight", c_void_p), ("cos", c_void_p), ("sin", c_void_p), ("eps", c_float), ("flags", c_int32),
    ]


class AttnPlan(Structure):
    _fields_ = [
        ("kernel", c_int32), ("mfma_k", c_int32), ("tiles_192", c_int32), ("tiles_128", c_int32),
        ("whole_workgroups", c_int32), ("split_tiles", c_int32), ("workgroups", c_int32), ("xcd_order", c_int32),
    ]


class Conv3dArgs(Structure):
    _fields_ = [
        ("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("out", c_void_p),
        ("resid", c_void_p), ("zero_page", c_void_p),
        ("B", c_int32), ("D", c_int32), ("H", c_int32), ("W", c_int32),
        ("Cin", c_int32), ("Cout", c_int32),
        ("causal", c_int32), ("pad_mode", c_int32),
        ("workspace", c_void_p), ("workspace_bytes", c_int64), ("taps_d", c_int32),
        ("act_out", c_void_p), ("act_scale", c_void_p), ("act_shift", c_void_p), ("act_eps", c_float), ("act_silu", c_int32),
    ]


class ConvTapsArgs(Structure):
    _fields_ = [
        ("struct_bytes", c_int32),
        ("B", c_int32), ("D", c_int32), ("H", c_int32), ("W", c_int32), ("Cin", c_int32), ("Cout", c_int32),
        ("kh", c_int32), ("kw", c_int32), ("dil_h", c_int32),
        ("pad_top", c_int32), ("pad_bottom", c_int32), ("pad_left", c_int32), ("pad_right", c_int32),
        ("n_mean", c_int32), ("slope", c_float),
        ("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("zero_page", c_void_p),
        ("resid", c_void_p), ("mean_a1", c_void_p), ("mean_a2", c_void_p),
        ("out", c_void_p), ("act_out", c_void_p), ("out_f32", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_int64),
    ]


class Conv3dPlan(Structure):
    _fields_ = [
        ("kernel", c_int32), ("tile_rows", c_int32), ("tile_cols", c_int32), ("row_tiles", c_int32), ("col_tiles", c_int32),
        ("slices", c_int32), ("ksteps", c_int32),
        ("tail_tile_rows", c_int32), ("tail_m_base", c_int32), ("tail_row_tiles", c_int32), ("fused_act", c_int32),
    ]


class StepArgs(Structure):
    _fields_ = [
        ("v_pos", c_void_p), ("v_neg", c_void_p), ("v_pert", c_void_p), ("latent", c_void_p), ("out", c_void_p),
        ("clean", c_void_p), ("mask", c_void_p), ("sigmas_dev", c_void_p),
        ("B", c_int32), ("C", c_int32), ("S", c_int32),
        ("cfg_scale", c_float), ("stg_scale", c_float), ("sigma", c_float), ("sigma_next", c_float), ("flags", c_int32),
    ]


class GuiderArgs(Structure):
    _fields_ = [
        ("v_pos", c_void_p), ("v_neg", c_void_p), ("v_pert", c_void_p), ("latent", c_void_p), ("out", c_void_p),
        ("clean", c_void_p), ("mask", c_void_p), ("sigmas_dev", c_void_p), ("record", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_int64),
        ("B", c_int32), ("C", c_int32), ("S", c_int32), ("guider", c_int32),
        ("cfg_scale", c_float), ("stg_scale", c_float), ("sigma", c_float), ("sigma_next", c_float),
        ("eta", c_float), ("norm_threshold", c_float), ("flags", c_int32),
    ]


class CausalAttnArgs(Structure):
    _fields_ = [
        ("q", c_void_p), ("k", c_void_p), ("vt", c_void_p), ("out", c_void_p), ("row_start", c_void_p),
        ("ldq", c_int32), ("ldk", c_int32), ("ldvt", c_int32), ("ldo", c_int32),
        ("B", c_int32), ("Hq", c_int32), ("Hkv", c_int32), ("T", c_int32), ("window", c_int32), ("scale", c_float),
    ]


class SampleArgs(Structure):
    _fields_ = [
        ("struct_bytes", c_int32),
        ("B", c_int32), ("V", c_int32), ("ld", c_int32), ("n_max", c_int32), ("hist_cap", c_int32), ("rep_ctx", c_int32),
        ("n_eos", c_int32), ("flags", c_int32),
        ("temperature", c_float), ("penalty", c_float),
        ("logits", c_void_p), ("ctl", c_void_p), ("done", c_void_p), ("next_ids", c_void_p), ("history", c_void_p),
        ("hist_len", c_void_p), ("tokens_out", c_void_p), ("eos", c_void_p), ("uniforms", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", c_int64),
    ]


# name -> (restype, argtypes); mirrors include/ltxk.h one to one.
SIGNATURES = {
    "ltxk_version": (c_int32, []),
    "ltxk_last_error": (c_char_p, []),
    "ltxk_abi_sizeof": (c_int32, [c_int32]),
    "ltxk_gemm_bf16": (c_int32, [POINTER(GemmArgs), c_void_p]),
    "ltxk_gemm_plan": (c_int32, [POINTER(GemmArgs), POINTER(GemmPlan)]),
    "ltxk_gemm_w8": (c_int32, [POINTER(GemmArgs), c_void_p, c_void_p]),
    "ltxk_gemv_w8": (c_int32, [POINTER(GemmArgs), c_void_p, c_void_p]),
    "ltxk_gemv_w4": (c_int32, [POINTER(GemmArgs), c_void_p, c_void_p]),
    "ltxk_gemm_w8_plan": (c_int32, [POINTER(GemmArgs), POINTER(GemmPlan)]),
    "ltxk_gemm_w8a8": (c_int32, [POINTER(GemmArgs), c_void_p, c_void_p, c_void_p]),
    "ltxk_gemm_w8a8_plan": (c_int32, [POINTER(GemmArgs), POINTER(GemmPlan)]),
    "ltxk_quant_rows_fp8": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p]),
    "ltxk_gemm_mxfp4": (c_int32, [POINTER(GemmArgs), c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "ltxk_gemm_mxfp4_plan": (c_int32, [POINTER(GemmArgs), POINTER(GemmPlan)]),
    "ltxk_quant_rows_mxfp4": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "ltxk_gemm_bf16_grouped": (c_int32, [POINTER(GemmGroupedArgs), c_void_p]),
    "ltxk_gemm_grouped_args_sizeof": (c_int32, []),
    "ltxk_gemm_grouped_plan": (c_int32, [POINTER(GemmGroupedArgs), POINTER(GemmGroupedPlan)]),
    "ltxk_qknorm_grouped_ss": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_float,
                                         c_void_p, c_int64, c_int32, c_void_p]),
    "ltxk_flash_attn": (c_int32, [POINTER(AttnArgs), c_void_p]),
    "ltxk_flash_attn_dh64": (c_int32, [POINTER(AttnArgs), c_void_p]),
    "ltxk_flash_attn_plan": (c_int32, [POINTER(AttnArgs), c_int32, POINTER(AttnPlan)]),
    "ltxk_flash_attn_plan_sizeof": (c_int32, []),
    "ltxk_flash_attn_bf16": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                       c_int32, c_int32, c_int32, c_int32, c_float, c_void_p]),
    "ltxk_rmsnorm_modulate": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p, c_int32,
                                        c_void_p, c_void_p]),
    "ltxk_layernorm_modulate": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p, c_int32,
                                          c_void_p, c_void_p]),
    "ltxk_qknorm_rope": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                   c_int32, c_int32, c_float, c_void_p]),
    "ltxk_timestep_embed": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p]),
    "ltxk_rope_table": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                  POINTER(c_float), c_void_p]),
    "ltxk_ada_combine": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_uint32, c_void_p]),
    "ltxk_rmsnorm_modulate_ss": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_int32, c_int32, c_void_p,
                                           c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "ltxk_rmsnorm_modulate2": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_int32, c_int32,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "ltxk_qknorm_rope_ss": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                      c_int32, c_int32, c_float, c_void_p, c_int32, c_void_p]),
    "ltxk_qknorm_rope_dh64": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                        c_int32, c_int32, c_float, c_void_p, c_int32, c_void_p]),
    "ltxk_silu": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "ltxk_latent_to_tokens": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "ltxk_conv3d_k3_bf16": (c_int32, [POINTER(Conv3dArgs), c_void_p]),
    "ltxk_conv3d_plan": (c_int32, [POINTER(Conv3dArgs), POINTER(Conv3dPlan)]),
    "ltxk_conv3d_plan_sizeof": (c_int32, []),
    # audio VAE decoder / vocoder (csrc/conv_taps.hip); the struct carries its own size (struct_bytes), checked by the library
    "ltxk_conv_taps_bf16": (c_int32, [POINTER(ConvTapsArgs), c_void_p]),
    "ltxk_conv_taps_plan": (c_int32, [POINTER(ConvTapsArgs), POINTER(Conv3dPlan)]),
    "ltxk_pixelnorm_act": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_float, c_void_p, c_void_p, c_int64,
                                     c_int32, c_void_p]),
    "ltxk_d2s_add": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                               c_void_p]),
    "ltxk_s2d_skip": (c_int32, [c_void_p, c_void_p, c_void_p] + [c_int32] * 10 + [c_void_p]),
    "ltxk_latent_denorm_cl": (c_int32, [c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64,
                                        c_void_p]),
    "ltxk_latent_norm_cf": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64,
                                      c_void_p]),
    "ltxk_unpatchify_cf": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                     c_void_p]),
    "ltxk_patchify_cl": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                   c_void_p]),
    "ltxk_to_uint8": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "ltxk_resize_area": (c_int32, [c_void_p, c_int32, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "ltxk_groupnorm_act": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_int32, c_int32,
                                     c_float, c_int32, c_void_p]),
    "ltxk_tile_blend_accum": (c_int32, [c_void_p] + [c_int32] * 6 + [c_void_p] * 5 + [c_int32] * 8 + [c_void_p]),
    "ltxk_tile_blend_finalize": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p]),
    "ltxk_step_scalars": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    "ltxk_euler_step": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p]),
    "ltxk_cfg_euler_step_dev": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                          c_int32, c_float, c_void_p, c_int32, c_void_p]),
    "ltxk_guided_euler_step": (c_int32, [POINTER(StepArgs), c_void_p]),
    "ltxk_guider_args_sizeof": (c_int32, []),
    "ltxk_guidance_sums_workspace_bytes": (c_int64, [c_int32, c_int32, c_int32]),
    "ltxk_guidance_sums": (c_int32, [POINTER(GuiderArgs), c_void_p]),
    "ltxk_guider_euler_step": (c_int32, [POINTER(GuiderArgs), c_void_p]),
    "ltxk_attn_value_passthrough": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_uint64,
                                              c_void_p]),
    "ltxk_cfg_euler_step": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                      c_int32, c_float, c_float, c_float, c_int32, c_void_p]),
    # text stage (csrc/text_ops.hip; ltxk_qknorm_rope_1d: csrc/elementwise.hip)
    "ltxk_masked_layer_stats": (c_int32, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                          c_int32, c_void_p, c_void_p, c_void_p]),
    "ltxk_layer_norm_compact": (c_int32, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "ltxk_rmsnorm_rows": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_float, c_void_p]),
    "ltxk_qknorm_rope_1d": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                      c_float, c_void_p]),
    "ltxk_gelu_erf": (c_int32, [c_void_p, c_int64, c_void_p]),
    "ltxk_connector_assemble": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                          c_int32, c_int32, c_void_p]),
    # Gemma-3 text encoder (csrc/text_ops.hip, csrc/causal_attn.hip)
    "ltxk_embed_rows": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p]),
    "ltxk_embed_rows_fp8": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p]),
    "ltxk_rmsnorm_weight_rows": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32,
                                           c_float, c_void_p]),
    "ltxk_headnorm_rope": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int32, c_float, c_void_p]),
    "ltxk_geglu_tanh": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "ltxk_causal_attn": (c_int32, [POINTER(CausalAttnArgs), c_void_p]),
    "ltxk_causal_attn_args_sizeof": (c_int32, []),
    # Gemma-3 decoding (csrc/causal_attn_step.hip)
    "ltxk_causal_attn_step": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                        c_void_p, c_int32, c_void_p] + [c_int32] * 6 + [c_float, c_void_p, c_int64, c_void_p]),
    # the decode step as one replayed graph: positions in device memory, sampling on the device (csrc/sample.hip)
    "ltxk_causal_attn_dev_step": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                            c_void_p, c_int32, c_void_p] + [c_int32] * 4 + [c_void_p, c_int32, c_int32, c_float, c_void_p,
                                                                                            c_int64, c_void_p]),
    "ltxk_headnorm_rope_at": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_int32, c_void_p, c_float, c_void_p]),
    "ltxk_sample_rows": (c_int32, [POINTER(SampleArgs), c_void_p]),
    # step cache of the denoise loop (csrc/step_cache.hip)
    "ltxk_step_cache_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "ltxk_step_cache_depth": (c_int32, [c_int64, c_int32]),
    "ltxk_step_cache_probe": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    "ltxk_residual_store": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "ltxk_residual_apply": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
}

# ltxk_abi_sizeof(i) is the size of ABI_STRUCTS[i]
ABI_STRUCTS = (GemmArgs, Conv3dArgs, AttnArgs, GemmPlan, StepArgs)

_lib = None
AB_LIB_PATH = os.path.join(_HERE, "libltxk_ab.so")
ATTN_NO_TAIL_SPLIT = 1        # ltxk.h: LTXK_ATTN_NO_TAIL_SPLIT
GEMM_FORM_SINGLE, GEMM_FORM_BIG, GEMM_FORM_SPLITK = 0, 1, 2     # ltxk.h: LTXK_GEMM_FORM_*
CONV_KERNEL_PER_TAP, CONV_KERNEL_KW, CONV_KERNEL_TAPS = 0, 1, 2  # ltxk.h: LTXK_CONV_KERNEL_*
ATTN_KERNEL_128, ATTN_KERNEL_MIX = 0, 1                         # ltxk.h: LTXK_ATTN_KERNEL_*
GUIDER_CFG_STAR, GUIDER_APG = 1, 2                              # ltxk.h: LTXK_GUIDER_*
GUIDER_RECORD_FLOATS = 8                                        # ltxk.h: LTXK_GUIDER_RECORD_FLOATS
SAMPLE_DRAW, SAMPLE_ADVANCE = 1, 2                              # ltxk.h: LTXK_SAMPLE_*
PROBE_INIT = 1                                                  # ltxk.h: LTXK_PROBE_INIT


def _open(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise LtxkError(
            f"{path} is missing: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C mlx-video_amd/csrc`). "
            "There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    for which, st in enumerate(ABI_STRUCTS):
        if lib.ltxk_abi_sizeof(which) != ctypes.sizeof(st):
            raise LtxkError(f"{path} is stale: sizeof({st.__name__}) is {lib.ltxk_abi_sizeof(which)} in the library, "
                            f"{ctypes.sizeof(st)} in this binding; rebuild it (make -C mlx-video_amd/csrc)")
    # (structs added after the ltxk_abi_sizeof index list was closed report their size through an entry of their own)
    for fn, st in ((lib.ltxk_gemm_grouped_args_sizeof, GemmGroupedArgs), (lib.ltxk_conv3d_plan_sizeof, Conv3dPlan),
                   (lib.ltxk_flash_attn_plan_sizeof, AttnPlan), (lib.ltxk_guider_args_sizeof, GuiderArgs),
                   (lib.ltxk_causal_attn_args_sizeof, CausalAttnArgs)):
        if fn() != ctypes.sizeof(st):
            raise LtxkError(f"{path} is stale: sizeof({st.__name__}) is {fn()} in the library, "
                            f"{ctypes.sizeof(st)} in this binding; rebuild it (make -C mlx-video_amd/csrc)")
    return lib


def load() -> ctypes.CDLL:
    """Load libltxk.so; raise LtxkError with the build recipe if it is not there."""
    global _lib
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


class use_library:
    """``with use_library(AB_LIB_PATH):`` routes every ops call inside the block to another build of the same ABI - the
    -DLTXK_AB measurement build, whose launch-form switches are environment variables (csrc/common.h).  For scripts/ and
    for the tests that compare two launch forms of one kernel bit for bit; the product path never enters it."""

    def __init__(self, path: str = AB_LIB_PATH):
        self.lib = _open(path)

    def __enter__(self):
        global _lib
        self.prev, _lib = _lib, self.lib
        return self.lib

    def __exit__(self, *a):
        global _lib
        _lib = self.prev


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().ltxk_last_error()
        raise LtxkError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
