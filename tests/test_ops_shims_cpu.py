"""The call shims of ``ops`` without a GPU: every refusal of ``ops._operands`` on CPU tensors (wrong dtype, wrong shape,
wrong layout, wrong alignment - each naming the operand - and, last, the device) for every shim that hands a tensor to the
library, the integers a shim compares with its tensors, the views the models pass, the rule that only ``_lib.py`` and
``ops.py`` speak to the library.  The VAE / upsampler rows of the table run in tests/test_vae_shims_cpu.py."""
import ast
import glob
import inspect
import io
import os
import re
import tokenize

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mlx-video_amd")
BF, F32 = torch.bfloat16, torch.float32
# entries of _lib.SIGNATURES that ops.py does not call: introspection, struct sizes, and the positional legacy entries
NOT_IN_OPS = {"ltxk_version", "ltxk_last_error", "ltxk_abi_sizeof", "ltxk_gemm_grouped_args_sizeof", "ltxk_conv3d_plan_sizeof",
              "ltxk_flash_attn_plan_sizeof", "ltxk_guider_args_sizeof", "ltxk_causal_attn_args_sizeof",
              "ltxk_flash_attn_bf16", "ltxk_cfg_euler_step", "ltxk_cfg_euler_step_dev"}


def z(*shape, dtype=BF):
    return torch.zeros(shape, dtype=dtype)


def nc(t):
    """The same shape and values, not contiguous."""
    return torch.stack([t, t], dim=-1)[..., 0]


# shim -> (positional arguments of a call that only the device refuses, keyword arguments, operand names by position)
B, D, H, W = 1, 2, 4, 4
GOOD = {
    "conv3d": ((z(B, D, H, W, 64), z(128, 3, 3, 3, 64), z(128), True, 0),
               dict(resid=z(B, D, H, W, 128), act=dict(eps=1e-8, scale=z(B, 128), shift=z(B, 128))), ("x", "w", "bias")),
    "pixelnorm_act": ((z(B, D, H, W, 64), 1e-8, True, z(B, 64), z(B, 64)), {}, ("x", None, None, "scale", "shift")),
    "d2s_add": ((z(B, D, H, W, 256), z(B, D, H, W, 64)), {}, ("conv", "xin")),
    "groupnorm_act": ((z(B, D, H, W, 64), z(64), z(64), z(B, D, H, W, 64)), {}, ("x", "gamma", "beta", "resid")),
    "latent_denorm_cl": ((z(B, 128, D, H, W), z(128), z(128), z(B, 128, D, H, W), 0.05), dict(out=z(B, D, H, W, 128)),
                         ("latent", "mean", "std", "noise")),
    "latent_norm_cf": ((z(B, D, H, W, 192)[..., :128], z(128), z(128)), dict(out=z(B, 128, D, H, W)), ("x", "mean", "std")),
    "patchify_cl": ((z(B, 3, D, 8, 12), 4, 64), dict(out=z(B, D, 2, 3, 64)), ("video",)),
    "unpatchify_cf": ((z(B, D, 2, 3, 48), 3, 4), dict(out=z(B, 3, D, 8, 12)), ("x",)),
    "s2d_skip": ((z(B, D, H, W, 64), z(B, D, H, W, 128), (2, 2, 2)), dict(out=z(B, 1, 2, 2, 512)), ("conv", "xpad")),
    "to_uint8": ((z(B, 3, D, H, W),), dict(out=z(B, D, H, W, 3, dtype=torch.uint8)), ("video",)),
    "tile_blend_accum": ((z(B, 3, 2, 4, 4), z(2, dtype=F32), z(3, dtype=F32), z(4, dtype=F32), z(B, 3, 5, 8, 8, dtype=F32),
                          z(B, 1, 5, 8, 8, dtype=F32), 1, 2, 3), {}, ("tile", "mt", "mh", "mw", "acc", "wsum")),
    "tile_blend_finalize": ((z(B, 3, 5, 8, 8, dtype=F32), z(B, 1, 5, 8, 8, dtype=F32)), dict(out=z(B, 3, 5, 8, 8)), ("acc", "wsum")),
}
# the DiT, step-tail, text-stage and Gemma shims at D = 512, H = 4, M = 8 rows (B = 2 batch rows of N = 4 tokens); a key
# "shim#form" is a second well-formed call of the same shim
M, DM, HH, N, P = 8, 512, 4, 4, 512 // 64
F8, I32 = torch.float8_e4m3fn, torch.int32
f32 = lambda *shape: z(*shape, dtype=F32)                   # noqa: E731
i32 = lambda *shape: z(*shape, dtype=I32)                   # noqa: E731
f8 = lambda *shape: z(*shape, dtype=torch.uint8).view(F8)   # noqa: E731
_tail = (z(2, N, 128), z(2, N, 128), z(2, N, 128), z(2, 128, 1, 2, 2))
VAE_SHIMS = tuple(GOOD)     # their rows of the table run in tests/test_vae_shims_cpu.py, under the test ids they have always had
GOOD.update({
    "gemm": ((z(M, DM), z(2 * DM, DM), z(2 * DM)),
             dict(out=z(M, DM), out2=z(2, DM, 64), n_split=DM, out_tokens_per_batch=N, sumsq=f32(M, P)), ("a", "w", "bias")),
    "gemm#gate": ((z(M, DM), z(DM, DM), z(DM)), dict(epilogue=3, out=z(M, DM), resid=z(M, DM), gate=z(2, 6, DM)[:, 2], gate_row=i32(M),
                                                      gate_stride=6 * DM, sumsq=f32(M, P)), ("a", "w", "bias")),
    "gemm#transposed": ((z(M, DM), z(DM, DM), z(DM)), dict(out=z(2, DM, 64), out_tokens_per_batch=N), ("a", "w", "bias")),
    "gemm#w8a8": ((f8(M, DM), f8(DM, DM), z(DM)), dict(a_scale=f32(M), w_scale=f32(DM)), ("a", "w", "bias")),
    "quant_rows_fp8": ((z(M, DM),), dict(out=(f8(M, DM), f32(M))), ("a",)),
    "gemm_grouped": ((z(M, DM), z(3, dtype=torch.int64), z(3, dtype=torch.int64), 2 * DM),
                     dict(out=z(3, M, DM), out2=z(3, 2, DM, 64), n_split=DM, out_tokens_per_batch=N, sumsq=f32(3, M, P)),
                     ("a", "w_table", "bias_table")),
    "flash_attn": ((z(M, DM), z(M, DM), z(2, DM, 64), z(M, DM), 2, HH, N, N, 0.088), {}, ("q", "k", "vt", "out")),
    "flash_attn#fused": ((z(M, DM), z(M, DM), z(2, DM, 64), z(M, DM), 2, HH, N, N, 0.088),
                         dict(q_sumsq=f32(M, P), q_norm_weight=z(DM), cos=f32(HH, N, 64), sin=f32(HH, N, 64)), ("q", "k", "vt", "out")),
    "attn_value_passthrough": ((z(2, DM, 64), z(M, DM), 2, N, 1), {}, ("vt", "out")),
    "causal_attn": ((z(M, 512), z(M, 256), z(2, 256, 8), z(M, 512), i32(2), 2, 2, 1, N, 0.0625), {}, ("q", "k", "vt", "out", "row_start")),
    "rmsnorm_modulate": ((z(M, DM), 1e-6, z(2, 6, DM)[:, 1], z(2, 6, DM)[:, 0], 6 * DM, i32(M)), dict(out=z(M, DM)),
                         ("x", None, "scale", "shift", None, "mod_row")),
    "rmsnorm_modulate#ss": ((z(M, DM), 1e-6, z(2, 6, DM)[:, 1], z(2, 6, DM)[:, 0], 6 * DM, i32(M)),
                            dict(out=z(M, DM), sumsq=f32(M, P), scale_is_one_plus=True), ("x", None, "scale", "shift", None, "mod_row")),
    "layernorm_modulate": ((z(M, DM), 1e-6, z(1, 2, DM)[:, 1], z(1, 2, DM)[:, 0], 2 * DM, i32(M)), dict(out=z(M, DM)),
                           ("x", None, "scale", "shift", None, "mod_row")),
    "qknorm_rope": ((z(M, 2 * DM), 2, DM, z(2, DM), f32(HH, N, 64), f32(HH, N, 64), N, HH, 1e-6), {},
                    ("buf", None, None, "weight", "cos", "sin")),
    "qknorm_rope#ss": ((z(M, 2 * DM), 2, DM, z(2 * DM), f32(HH, N, 64), f32(HH, N, 64), N, HH, 1e-6), dict(sumsq=f32(M, 2 * P)),
                       ("buf", None, None, "weight", "cos", "sin")),
    "qknorm_grouped": ((z(3, M, DM), z(3, DM), HH, 1e-6, f32(3, M, P)), {}, ("buf", "weight", None, None, "sumsq")),
    "qknorm_rope_1d": ((z(M, 2 * DM + 8), DM, z(2, DM), f32(HH, N, 64), f32(HH, N, 64), N, HH), {}, ("buf", None, "weight", "cos", "sin")),
    "rmsnorm_rows": ((z(M, DM),), dict(out=z(M, DM)), ("x",)),
    "rmsnorm_weight_rows": ((z(M, DM), z(DM)), dict(resid=z(M, DM), out=z(M, DM)), ("x", "weight")),
    "headnorm_rope": ((z(M, 1024), 2, 1, z(256), z(256), f32(N, 128), f32(N, 128), N), {},
                      ("buf", None, None, "q_weight", "k_weight", "cos", "sin")),
    "timestep_embed": ((z(3),), {}, ("t",)),
    "rope_table": ((f32(3, N, 2), f32(16), HH, DM, (20, 64, 64)), {}, ("positions", "freq")),
    "ada_combine": ((z(2, 6, DM), z(3, 6 * DM), 2, 3, 6, DM), {}, ("table", "ada")),
    "silu": ((z(3, DM),), {}, ("x",)),
    "latent_to_tokens": ((z(2, 128, 1, 2, 2),), {}, ("latent",)),
    "euler_only": ((z(2, 128, 4), z(2, 128, 4), 0.5, 0.25), {}, ("latent", "denoised")),
    "resize_area": ((f32(3, 8, 8), 4, 4), {}, ("x",)),
    "step_scalars": ((z(5, 3), f32(5, 2), i32(1), z(3), f32(2)), {}, ("ts_all", "sig_all", "step", "ts", "sig")),
    "gelu_erf_": ((z(M, DM),), {}, ("x",)),
    "geglu_tanh_": ((z(M, 64),), {}, ("gu",)),
    "embed_rows": ((z(16, DM), i32(M), 22.0), dict(out=z(M, DM), ids_host=i32(M)), ("table", "ids")),
    "connector_assemble": ((z(5, DM), z(2, DM), i32(2), i32(2), 2, N), {}, ("feat", "registers", "row0", "row_count")),
    "masked_layer_stats": ((z(3, 2, N, DM), i32(2), i32(2)), {}, ("x", "row_start", "row_count")),
    "layer_norm_compact": ((z(3, 2, N, DM), i32(2), i32(2), i32(2), f32(2, 3, 3), z(5, 3 * DM), 5), {},
                           ("x", "row_start", "row_count", "row0", "stats", "out")),
    "step_tail": (_tail, dict(cfg_scale=4.0, stg_scale=1.0, sigma=0.5, sigma_next=0.25, clean=z(2, 128, 1, 2, 2), mask_tok=f32(2, N),
                              out=z(2, 128, 1, 2, 2), sigmas_dev=f32(2)), ("v_pos", "v_neg", "v_pert", "latent")),
    "step_tail#apg": (_tail, dict(cfg_scale=4.0, sigma=0.5, sigma_next=0.25, guider="apg", record=f32(2, 8)),
                      ("v_pos", "v_neg", "v_pert", "latent")),
    "guidance_sums": ((_tail[0], _tail[1], _tail[3], "apg", 0.5), dict(record=f32(2, 8), workspace=f32(4096), sigmas_dev=f32(2)),
                      ("v_pos", "v_neg", "latent")),
})
# public functions of ops with a tensor parameter that are no shim of their own, and why (pointer_table takes a list of tensors
# whose addresses it stores and hands none of them to the library)
NO_SHIM = {"cfg_euler_step": "a spelling of step_tail", "guided_euler_step": "a spelling of step_tail",
           "guider_euler_step": "a spelling of step_tail"}
# "wrong extent" where a longer last dimension is a legal operand: the mutation that is wrong instead (None: every extent is legal)
extra_dim = lambda t: t[None]                                # noqa: E731
OTHER_EXTENT = {
    ("d2s_add", "conv"): extra_dim, ("d2s_add", "xin"): extra_dim,                      # more channels
    **{("tile_blend_accum", n): extra_dim for n in ("tile", "mt", "mh", "mw", "wsum")},      # a larger tile or box
    **{(s, "sumsq"): extra_dim for s in ("gemm", "gemm#gate", "gemm_grouped", "rmsnorm_modulate#ss", "qknorm_rope#ss", "qknorm_grouped")},
    ("gemm", "out2"): extra_dim, ("gemm#transposed", "out"): extra_dim, ("gemm_grouped", "out2"): extra_dim,        # V^T: ld >= tokens
    ("flash_attn", "vt"): extra_dim, ("flash_attn#fused", "vt"): extra_dim, ("flash_attn#fused", "q_sumsq"): extra_dim,
    ("attn_value_passthrough", "vt"): extra_dim, ("attn_value_passthrough", "out"): extra_dim,
    **{("causal_attn", n): extra_dim for n in ("q", "k", "vt", "out")}, ("layer_norm_compact", "out"): extra_dim,
    ("guidance_sums", "workspace"): extra_dim,
    ("gemm_grouped", "a"): extra_dim, ("masked_layer_stats", "x"): extra_dim,           # K / T x D: whatever the operand has
    # in place on the leading columns of a wider buffer: the operand is buf[:, :cols]
    ("qknorm_rope", "buf"): extra_dim, ("qknorm_rope#ss", "buf"): extra_dim, ("qknorm_rope_1d", "buf"): extra_dim,
    ("headnorm_rope", "buf"): extra_dim,
    ("latent_to_tokens", "latent"): lambda t: t[0, 0, 0], ("resize_area", "x"): lambda t: t[0, 0],      # (B,C,...) / (...,H,W): any extent
    ("step_tail", "latent"): lambda t: t[0, 0, 0, 0], ("step_tail#apg", "latent"): lambda t: t[0, 0, 0, 0],
    ("guidance_sums", "latent"): lambda t: t[0, 0, 0, 0],
    ("geglu_tanh_", "gu"): lambda t: z(M, 72),                                           # F a multiple of 8
    **{k: None for k in (("timestep_embed", "t"), ("silu", "x"), ("gelu_erf_", "x"), ("euler_only", "latent"),
                         ("rope_table", "freq"), ("connector_assemble", "feat"))},
}
# operands a shim derives sizes from: their wrong extent is reported under the partner it no longer fits
NAMED_AS = {("gemm_grouped", "w_table"): "bias_table", ("embed_rows", "ids"): "out", ("embed_rows", "table"): "out",
            ("connector_assemble", "registers"): "feat", ("step_scalars", "ts_all"): "ts",
            ("masked_layer_stats", "x"): "", ("layer_norm_compact", "x"): "out"}
# shims that copy an operand that is not contiguous instead of refusing it
NORMALISED = {("latent_to_tokens", "latent"), ("euler_only", "latent"), ("euler_only", "denoised"), ("resize_area", "x")}
# rows may carry a leading dimension: the strided mutation gives them a non-unit inner stride, which is refused all the same


def _cases():
    """(id, shim, args, kwargs, exception, operand): every tensor operand of every shim with the wrong dtype, one dimension
    too long, and non-contiguous; the keyword tensors (resid, out, act's vectors) the same way."""
    wrong = lambda t: F32 if t.dtype != F32 else BF                                     # noqa: E731
    either_float = ("resize_area", "x")                        # float32 and bfloat16 are both operands: an integer type is wrong
    longer = lambda t: torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 8,), dtype=t.dtype)   # noqa: E731
    # (the same view of a buffer of another dtype: strides and offset stay, so only the dtype is wrong)
    retype = lambda t, d: torch.zeros(t.untyped_storage().nbytes() // t.element_size(), dtype=d).as_strided(t.shape, t.stride(), t.storage_offset())   # noqa: E731
    muts = (("dtype", lambda t: retype(t, wrong(t)), TypeError), ("shape", longer, ValueError), ("strided", nc, ValueError))
    for key, (args, kw, names) in GOOD.items():
        shim = key.split("#")[0]
        for i, name in enumerate(names):
            if name is None or args[i] is None:
                continue
            for tag, mut, exc in muts:
                if (key, name, tag) in (("latent_norm_cf", "x", "strided"), ("tile_blend_accum", "acc", "shape")):
                    continue       # rows may carry a leading dimension (its own case below); acc defines the volume
                if tag == "strided" and ((shim, name) in NORMALISED or args[i].numel() == 1):
                    continue       # copied, not refused; a single element has no stride to get wrong
                if tag == "dtype" and (shim, name) == either_float:
                    mut = lambda t: retype(t, torch.int32)                            # noqa: E731
                if tag == "shape":
                    mut = OTHER_EXTENT.get((key, name), mut)
                    if mut is None:
                        continue
                bad = list(args)
                bad[i] = mut(args[i])
                # a longer first operand is the one the sizes derive from: the mismatch is then reported under its partner's name
                derived = tag == "shape" and bad[i].dim() == args[i].dim() and (i == 0 or (shim, name) in NAMED_AS)
                yield f"{key}.{name}.{tag}", shim, tuple(bad), kw, exc, NAMED_AS.get((shim, name), "") if derived else name
        for k, val in kw.items():
            if not isinstance(val, (torch.Tensor, dict)):
                continue
            for tag, mut, exc in muts:
                if k == "act":
                    for v in ("scale", "shift"):
                        yield f"{key}.act.{v}.{tag}", shim, args, dict(kw, act=dict(val, **{v: mut(val[v])})), exc, v
                elif k == "ids_host" or (tag == "strided" and (shim, k) in NORMALISED):
                    continue
                else:
                    if tag == "shape":
                        mut = OTHER_EXTENT.get((key, k), mut)
                    yield f"{key}.{k}.{tag}", shim, args, dict(kw, **{k: mut(val)}), exc, k
    # the derived sizes and the pairs that go together
    g = {k: v[0] for k, v in GOOD.items()}
    yield "latent_norm_cf.x.inner_stride", "latent_norm_cf", (z(B, D, H, W, 256)[..., ::2],) + g["latent_norm_cf"][1:], {}, ValueError, "x"
    yield "conv3d.w.Cin", "conv3d", (g["conv3d"][0], z(128, 3, 3, 3, 32)) + g["conv3d"][2:], {}, ValueError, "weight"
    yield "conv3d.act.scale_alone", "conv3d", g["conv3d"], dict(act=dict(eps=1e-8, scale=z(B, 128))), ValueError, "scale"
    yield "pixelnorm_act.scale_alone", "pixelnorm_act", g["pixelnorm_act"][:4], {}, ValueError, "scale"
    yield "d2s_add.conv.channels", "d2s_add", (z(B, D, H, W, 100), None), {}, ValueError, "conv"
    yield "groupnorm_act.groups", "groupnorm_act", g["groupnorm_act"], dict(groups=24), ValueError, "groups"
    yield "patchify_cl.Cpad", "patchify_cl", (g["patchify_cl"][0], 4, 40), {}, ValueError, "Cpad"
    yield "patchify_cl.H", "patchify_cl", (z(B, 3, D, 9, 12), 4, 64), {}, ValueError, "P"
    yield "unpatchify_cf.C", "unpatchify_cf", (g["unpatchify_cf"][0], 4, 4), {}, ValueError, "x"
    yield "s2d_skip.stride", "s2d_skip", g["s2d_skip"][:2] + ((1, 3, 2),), {}, ValueError, "stride"
    yield "s2d_skip.xpad.channels", "s2d_skip", (g["s2d_skip"][0], z(B, D, H, W, 96), (2, 2, 2)), {}, ValueError, "xpad"
    yield "tile_blend_accum.tile.channels", "tile_blend_accum", (z(B, 4, 2, 4, 4),) + g["tile_blend_accum"][1:], {}, ValueError, "tile"
    yield "tile_blend_accum.tile.rank", "tile_blend_accum", (z(B, 3, 4, 4),) + g["tile_blend_accum"][1:], {}, ValueError, "tile"


CASES = list(_cases())


@pytest.mark.parametrize("key", sorted(set(GOOD) - set(VAE_SHIMS)))
def test_well_formed_cpu_operands_are_refused_for_the_device_only(key):
    from mlx_video_amd import _lib, ops
    shim = key.split("#")[0]
    args, kw, _ = GOOD[key]
    with pytest.raises(_lib.LtxkError, match=f"{shim}: .* device tensor.*no CPU fallback"):
        getattr(ops, shim)(*args, **kw)
    required = [p for p in inspect.signature(getattr(ops, shim)).parameters.values() if p.kind is p.KEYWORD_ONLY and p.default is p.empty]
    if "#" not in key and not required:          # (a second form needs its keywords)
        with pytest.raises(_lib.LtxkError, match=f"{shim}: .* device tensor"):
            getattr(ops, shim)(*args)


OTHERS = [c for c in CASES if c[1] not in VAE_SHIMS]


@pytest.mark.parametrize("shim,args,kw,exc,operand", [c[1:] for c in OTHERS], ids=[c[0] for c in OTHERS])
def test_shims_refuse_bad_operands_before_any_launch(shim, args, kw, exc, operand):
    """Follows test_guiders_cpu.py::test_ops_refuse_bad_arguments_before_any_launch: CPU tensors throughout, so a refusal
    other than the device's proves that it comes before the device check - and before any pointer reaches the library."""
    from mlx_video_amd import ops
    with pytest.raises(exc, match=f"{shim}: .*{operand}"):
        getattr(ops, shim)(*args, **kw)


def _with(key, pos=None, **kw):
    """GOOD[key] with positional arguments (index -> value) and keywords replaced: (shim, args, kwargs)."""
    args, base, _ = GOOD[key]
    args = list(args)
    for i, v in (pos or {}).items():
        args[i] = v
    return key.split("#")[0], tuple(args), dict(base, **kw)


def off_by_one(*shape, dtype=BF):
    """A contiguous tensor that starts one element past a 16-byte boundary."""
    n = 1
    for d in shape:
        n *= d
    return torch.zeros(n + 1, dtype=dtype)[1:].view(shape)


def _explicit():
    """(id, (shim, args, kwargs), exception or None for "the device only", operand)."""
    V = ValueError
    # a misaligned operand per family
    for key, pos, shape in (("gemm", 0, (M, DM)), ("quant_rows_fp8", 0, (M, DM)), ("gemm_grouped", 0, (M, DM)), ("flash_attn", 0, (M, DM)),
                            ("attn_value_passthrough", 0, (2, DM, 64)), ("causal_attn", 0, (M, 512)), ("rmsnorm_modulate", 0, (M, DM)),
                            ("layernorm_modulate", 0, (M, DM)), ("qknorm_rope", 0, (M, 2 * DM)), ("qknorm_grouped", 0, (3, M, DM)),
                            ("qknorm_rope_1d", 0, (M, 2 * DM + 8)), ("rmsnorm_rows", 0, (M, DM)), ("rmsnorm_weight_rows", 1, (DM,)),
                            ("headnorm_rope", 0, (M, 1024)), ("ada_combine", 0, (2, 6, DM)), ("silu", 0, (3, DM)), ("euler_only", 1, (2, 128, 4)),
                            ("gelu_erf_", 0, (M, DM)), ("geglu_tanh_", 0, (M, 64)), ("embed_rows", 0, (16, DM)),
                            ("connector_assemble", 1, (2, DM)), ("masked_layer_stats", 0, (3, 2, N, DM)),
                            ("layer_norm_compact", 5, (5, 3 * DM)), ("step_tail", 0, (2, N, 128)), ("guidance_sums", 1, (2, N, 128))):
        yield f"{key}.misaligned", _with(key, {pos: off_by_one(*shape)}), V, f"{GOOD[key][2][pos]} must be 16-byte aligned"
    yield "gemm.bias.misaligned", _with("gemm", {2: off_by_one(2 * DM)}), V, "bias must be 8-byte aligned"
    # each minimum extent, one short of it and exactly at it
    for tag, cols, exc in (("short", -1, V), ("exact", 0, None)):
        e = lambda name: name if exc else ""                # noqa: E731
        yield f"gemm.sumsq.{tag}", _with("gemm", sumsq=f32(M, P + cols)), exc, e("sumsq")
        yield f"gemm.out2.ld.{tag}", _with("gemm", out2=z(2, DM, N + cols)), exc, e("out2")
        yield f"gemm.transposed.out.ld.{tag}", _with("gemm#transposed", out=z(2, DM, N + cols)), exc, e("out")
        yield f"gemm_grouped.sumsq.{tag}", _with("gemm_grouped", sumsq=f32(3, M, P + cols)), exc, e("sumsq")
        yield f"gemm_grouped.out2.ld.{tag}", _with("gemm_grouped", out2=z(3, 2, DM, N + cols)), exc, e("out2")
        yield f"flash_attn.vt.ld.{tag}", _with("flash_attn", {2: z(2, DM, N + cols)}), exc, e("vt")
        yield f"flash_attn.q_sumsq.{tag}", _with("flash_attn#fused", q_sumsq=f32(M, P + 4 * cols)), exc, e("q_sumsq")      # (16-byte rows)
        yield f"attn_value_passthrough.vt.ld.{tag}", _with("attn_value_passthrough", {0: z(2, DM, N + cols)}), exc, e("vt")
        yield f"attn_value_passthrough.vt.batch.{tag}", _with("attn_value_passthrough", {0: z(2 + cols, DM, 64)}), exc, e("vt")
        yield f"attn_value_passthrough.out.rows.{tag}", _with("attn_value_passthrough", {1: z(M + cols, DM)}), exc, e("out")
        yield f"attn_value_passthrough.out.cols.{tag}", _with("attn_value_passthrough", {1: z(M, DM + 8 * cols)}), exc, e("out")
        yield f"causal_attn.vt.ld.{tag}", _with("causal_attn", {2: z(2, 256, N + cols)}), exc, e("vt")
        yield f"causal_attn.q.cols.{tag}", _with("causal_attn", {0: z(M, 512 + 8 * cols)}), exc, e("q")
        yield f"causal_attn.k.cols.{tag}", _with("causal_attn", {1: z(M, 256 + 8 * cols)}), exc, e("k")
        yield f"causal_attn.out.cols.{tag}", _with("causal_attn", {3: z(M, 512 + 8 * cols)}), exc, e("out")
        yield f"rmsnorm_modulate.sumsq.{tag}", _with("rmsnorm_modulate#ss", sumsq=f32(M, P + cols)), exc, e("sumsq")
        yield f"qknorm_rope.sumsq.{tag}", _with("qknorm_rope#ss", sumsq=f32(M, 2 * P + cols)), exc, e("sumsq")
        yield f"qknorm_rope.buf.cols.{tag}", _with("qknorm_rope", {0: z(M, 2 * DM + 8 * cols)}), exc, e("buf")
        yield f"qknorm_grouped.sumsq.{tag}", _with("qknorm_grouped", {4: f32(3, M, P + cols)}), exc, e("sumsq")
        yield f"qknorm_rope_1d.buf.cols.{tag}", _with("qknorm_rope_1d", {0: z(M, 2 * DM + 8 * cols)}), exc, e("buf")
        yield f"headnorm_rope.buf.cols.{tag}", _with("headnorm_rope", {0: z(M, 768 + 8 * cols)}), exc, e("buf")
        yield f"layer_norm_compact.out.rows.{tag}", _with("layer_norm_compact", {5: z(5 + cols, 3 * DM)}), exc, e("out")
        yield f"layer_norm_compact.out.cols.{tag}", _with("layer_norm_compact", {5: z(5, 3 * DM + 8 * cols)}), exc, e("out")
    from mlx_video_amd import ops
    need = ops.guidance_sums_workspace_bytes(2, 128, N) // 4
    yield "guidance_sums.workspace.short", _with("guidance_sums", workspace=f32(need - 1)), V, "workspace"
    yield "guidance_sums.workspace.exact", _with("guidance_sums", workspace=f32(need)), None, ""
    yield "quant_rows_fp8.out[0].dtype", _with("quant_rows_fp8", out=(z(M, DM), f32(M))), TypeError, r"out\[0\]"
    yield "quant_rows_fp8.out[0].strided", _with("quant_rows_fp8", out=(f8(M, 2 * DM)[:, ::2], f32(M))), V, r"out\[0\]"
    yield "quant_rows_fp8.out[0].rows_of_a_wider_buffer", _with("quant_rows_fp8", out=(f8(M, 2 * DM)[:, :DM], f32(M))), None, ""
    yield "quant_rows_fp8.out[1].shape", _with("quant_rows_fp8", out=(f8(M, DM), f32(M + 1))), V, r"out\[1\]"
    # the integers a shim takes although its tensors determine them
    for i, (name, operand) in enumerate((("L", "table"), ("U", "ada"), ("K", "table"), ("D", "table")), start=2):
        for d in (1, -1):
            yield f"ada_combine.{name}{d:+d}", _with("ada_combine", {i: GOOD["ada_combine"][0][i] + d}), V, operand
    for i, (name, operand) in enumerate((("B", "q"), ("H", "q"), ("Tq", "q"), ("Tk", "k")), start=4):
        yield f"flash_attn.{name}", _with("flash_attn#fused", {i: GOOD["flash_attn"][0][i] + 1}), V, operand
    yield "flash_attn.Tq.tables", _with("flash_attn#fused", {0: z(2 * 5, DM), 3: z(2 * 5, DM), 6: 5}, q_sumsq=f32(2 * 5, P)), V, "cos"
    yield "flash_attn.H.weight", _with("flash_attn#fused", {0: z(M, 640), 1: z(M, 640), 2: z(2, 640, 64), 3: z(M, 640), 5: 5},
                                       q_sumsq=f32(M, 12), cos=f32(5, N, 64), sin=f32(5, N, 64)), V, "q_norm_weight"
    yield "flash_attn.q_norm_weight.one_row", _with("flash_attn#fused", q_norm_weight=z(1, DM)), None, ""
    yield "flash_attn.out.float32", _with("flash_attn", {3: f32(M, DM)}), TypeError, "out"
    yield "flash_attn.q.inner_stride", _with("flash_attn", {0: z(M, 2 * DM)[:, ::2]}), V, "q"
    yield "flash_attn.vt.batch_stride", _with("flash_attn", {2: z(2, 2 * DM, 64)[:, :DM]}), V, "vt"
    yield "flash_attn.q_sumsq.alone", _with("flash_attn", q_sumsq=f32(M, P)), V, "q_norm_weight"
    yield "qknorm_rope.nseg", _with("qknorm_rope", {1: 3}), V, "buf"
    yield "qknorm_rope.D", _with("qknorm_rope", {2: 256}), V, "D"
    yield "qknorm_rope.T", _with("qknorm_rope", {6: N + 1}), V, "cos"
    yield "qknorm_rope.H", _with("qknorm_rope", {7: 8}), V, "H"
    yield "qknorm_rope.sin_alone", _with("qknorm_rope", {4: None}), V, "cos and sin"
    yield "step_scalars.ts", _with("step_scalars", {3: z(4)}), V, "ts"
    yield "step_scalars.sig", _with("step_scalars", {4: f32(3)}), V, "sig"
    # dense (M,D) rows that the C entry takes without a stride
    yield "rmsnorm_modulate.x.rows_of_a_wider_buffer", _with("rmsnorm_modulate", {0: z(M, 2 * DM)[:, :DM]}, out=None), V, "x must be contiguous"
    yield "layernorm_modulate.x.rows_of_a_wider_buffer", _with("layernorm_modulate", {0: z(M, 2 * DM)[:, :DM]}, out=None), V, "x must be contiguous"
    yield "silu.x.rows_of_a_wider_buffer", _with("silu", {0: z(3, 2 * DM)[:, :DM]}), V, "x must be contiguous"
    yield "rmsnorm_modulate.mod_stride", _with("rmsnorm_modulate", {4: 3 * DM}), V, "scale"
    yield "rmsnorm_modulate.shift_alone", _with("rmsnorm_modulate", {2: None}), V, "scale and shift"
    yield "gemm.gate_stride", _with("gemm#gate", gate_stride=3 * DM), V, "gate"
    yield "gemm.out2.missing", _with("gemm", out2=None), V, "out2"
    # the views the models pass (ltx_model.forward_tokens, text_connector, gemma): legal, so only the device refuses them
    qk, qkss, vt, att, mod = z(2 * M, 2 * DM), f32(2 * M, 2 * P), z(4, DM, 64), z(2 * M, DM), z(3, 6, DM)
    w, cs = z(DM), f32(HH, N, 64)
    yield "view.flash_attn.row_slice", ("flash_attn", (qk[M:, :DM], qk[M:, DM:], vt[2:], att[M:], 2, HH, N, N, 0.088),
                                        dict(q_sumsq=qkss[M:], q_norm_weight=w, cos=cs, sin=cs)), None, ""
    yield "view.flash_attn.stacked_kv", ("flash_attn", (att[:M], z(3, M, DM)[1], z(3, 2, DM, 64)[1], att[M:], 2, HH, N, N, 0.088), {}), None, ""
    yield "view.qknorm_rope.k_half", ("qknorm_rope", (qk[:, DM:], 1, DM, w, cs, cs, N, HH, 1e-6), dict(sumsq=qkss[:, P:])), None, ""
    yield "view.rmsnorm_modulate.mod_rows", ("rmsnorm_modulate", (att, 1e-6, mod[:, 4], mod[:, 3], 6 * DM, i32(2 * M)),
                                             dict(out=z(2 * M + 2, DM)[:2 * M], sumsq=qkss[:, :P], scale_is_one_plus=True)), None, ""
    yield "view.gemm.split_into_views", ("gemm", (att, z(3 * DM, DM), z(3 * DM)), dict(out=qk, out2=vt, n_split=2 * DM, out_tokens_per_batch=N,
                                                                                        sumsq=qkss)), None, ""
    yield "view.gemm.gate_rows", ("gemm", (att, z(DM, DM), z(DM)), dict(epilogue=3, out=att, resid=att, gate=mod[:, 2], gate_row=i32(2 * M),
                                                                        gate_stride=6 * DM, sumsq=qkss[:, :P])), None, ""
    yield "view.gemm.rows_of_geglu", ("gemm", (z(M, 2 * DM)[:, :DM], z(DM, DM), None), {}), None, ""
    yield "view.attn_value_passthrough", ("attn_value_passthrough", (vt, att, 4, N, 0b0101), {}), None, ""
    yield "view.causal_attn.qk_halves", ("causal_attn", (z(M, 768)[:, :512], z(M, 768)[:, 512:], z(2, 256, 64), z(M, 512), i32(2), 2, 2, 1, N,
                                                         0.0625), {}), None, ""
    yield "view.masked_layer_stats.strided_stack", ("masked_layer_stats", (z(4, 2, N + 4, DM + 8)[1:, :, 4:, :DM], i32(2), i32(2)), {}), None, ""


EXPLICIT = list(_explicit())


@pytest.mark.parametrize("call,exc,operand", [c[1:] for c in EXPLICIT], ids=[c[0] for c in EXPLICIT])
def test_sizes_alignment_minimum_extents_and_model_views(call, exc, operand):
    """The refusals no mutation of one operand reaches, and the accept side: ``exc`` None is a call that only the device
    refuses - every other check has passed on it."""
    from mlx_video_amd import _lib, ops
    shim, args, kw = call
    if exc is None:
        with pytest.raises(_lib.LtxkError, match=f"{shim}: .* device tensor"):
            getattr(ops, shim)(*args, **kw)
    else:
        with pytest.raises(exc, match=f"{shim}: .*{operand}"):
            getattr(ops, shim)(*args, **kw)


def _shims():
    """Every public function of ops whose signature annotates a tensor parameter, minus NO_SHIM."""
    from mlx_video_amd import ops
    for name, fn in vars(ops).items():
        if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not name.startswith("_") and \
                any("Tensor" in str(p.annotation) for p in inspect.signature(fn).parameters.values()):
            yield name


def test_refusal_table_covers_every_shim_three_ways():
    shims = set(_shims())
    assert set(NO_SHIM) <= shims and len(shims) > 40 and "pointer_table" not in shims
    assert {k.split("#")[0] for k in GOOD} == shims - set(NO_SHIM)
    for shim in shims - set(NO_SHIM):
        tags = {c[0].rsplit(".", 1)[1] for c in CASES if c[1] == shim}
        want = {"dtype", "shape", "strided"}
        if all((shim, n) in NORMALISED for k, v in GOOD.items() if k.split("#")[0] == shim for n in v[2] if n):
            want.discard("strided")         # every operand of it is copied when it is not contiguous
        if shim in ("timestep_embed", "silu", "gelu_erf_"):
            want.discard("shape")           # one operand of any extent
        assert want <= tags, (shim, tags)
    # every positional tensor of a GOOD call is a named operand
    for key, (args, kw, names) in GOOD.items():
        for i, a in enumerate(args):
            assert not isinstance(a, torch.Tensor) or (i < len(names) and names[i]), (key, i)


PLANS_AND_SIZES = ("gemm_plan", "gemm_grouped_plan", "flash_attn_plan", "conv3d_plan", "guidance_sums_workspace_bytes")


def test_every_function_that_launches_checks_its_operands():
    """ops.py by its syntax tree: a function that calls an entry of the library checks its operands through ``_operands`` -
    itself, or through the step tail's validator - unless it is a plan / size function, which hands over no tensor."""
    tree = ast.parse(open(os.path.join(PKG, "ops.py"), encoding="utf-8").read())
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    assert "_req" not in funcs and "_req_layers" not in funcs and "_operands" in funcs

    def calls(fn):
        return {c.func.id for c in ast.walk(fn) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}

    def launches(fn):
        return any(isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr.startswith("ltxk_") and
                   isinstance(c.func.value, ast.Call) and ast.unparse(c.func.value) == "_lib.load()" for c in ast.walk(fn))

    assert "_operands" in calls(funcs["_step_tail_args"])
    speakers = [name for name, fn in funcs.items() if launches(fn)]
    assert len(speakers) > 45 and set(PLANS_AND_SIZES) <= set(speakers)
    for name in speakers:
        if name not in PLANS_AND_SIZES:
            assert calls(funcs[name]) & {"_operands", "_step_tail_args"}, f"{name} launches without checking its operands"


def test_one_scratch_cache_keeps_sizes_and_dtypes():
    from mlx_video_amd import ops
    assert ops.GEMM_WORKSPACE_BYTES == 64 << 20 and ops.SPLITK_WORKSPACE_BYTES == 96 << 20
    assert ops._SCRATCH_KINDS == {"gemm_splitk": (ops.GEMM_WORKSPACE_BYTES // 4, F32, torch.empty),
                                  "conv_splitk": (ops.SPLITK_WORKSPACE_BYTES // 4, F32, torch.empty),
                                  "zero_page": (256, torch.uint8, torch.zeros)}
    cpu = torch.device("cpu")
    zp = ops._scratch("zero_page", cpu)
    try:
        assert zp is ops._scratch("zero_page", cpu) and zp.dtype == torch.uint8 and zp.numel() == 256 and not bool(zp.any())
    finally:
        ops._SCRATCH.pop(("zero_page", 0), None)


# ------------------------------------------------------------------------------------------------- who speaks to the library
def _code_tokens(src):
    """The source's tokens without comments and docstrings."""
    doc = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and ast.get_docstring(node, clean=False) is not None:
            doc.update(range(node.body[0].lineno, node.body[0].end_lineno + 1))
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type != tokenize.COMMENT and not (tok.type == tokenize.STRING and tok.start[0] in doc):
            yield tok


def test_only_lib_and_ops_speak_to_the_library():
    """ops.py: "One function per entry point of include/ltxk.h" - and nobody else calls one."""
    from mlx_video_amd import _lib
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) > 10
    for path in files:
        name = os.path.basename(path)
        if name in ("_lib.py", "ops.py"):
            continue
        src = open(path, encoding="utf-8").read()
        hits = [(t.start[0], t.string) for t in _code_tokens(src) if "ltxk_" in t.string]
        assert not hits, f"{name} names a library entry in code: {hits[:5]}"
        for node in ast.walk(ast.parse(src)):
            mods = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            assert not any(m.split(".")[0] == "ctypes" for m in mods), f"{name} imports ctypes (line {node.lineno})"
    ops_src = "".join(t.string + " " for t in _code_tokens(open(os.path.join(PKG, "ops.py"), encoding="utf-8").read()))
    called = set(re.findall(r"\. (ltxk_\w+) \(", ops_src))
    assert set(_lib.SIGNATURES) - called == NOT_IN_OPS
    assert called <= set(_lib.SIGNATURES)
