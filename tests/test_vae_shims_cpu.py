"""The VAE / upsampler call shims of ``ops`` without a GPU: every refusal of ``ops._operands`` on CPU tensors (wrong dtype,
wrong shape, wrong layout - each naming the operand - and, last, the device), the rule that only ``_lib.py`` and ``ops.py``
speak to the library, and the model constructors' bf16 normalisation of their weights."""
import ast
import glob
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


def _cases():
    """(id, shim, args, kwargs, exception, operand): every tensor operand of every shim with the wrong dtype, one dimension
    too long, and non-contiguous; the keyword tensors (resid, out, act's vectors) the same way."""
    wrong = lambda t: F32 if t.dtype != F32 else BF                                     # noqa: E731
    longer = lambda t: torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 8,), dtype=t.dtype)   # noqa: E731
    muts = (("dtype", lambda t: t.to(wrong(t)), TypeError), ("shape", longer, ValueError), ("strided", nc, ValueError))
    for shim, (args, kw, names) in GOOD.items():
        for i, name in enumerate(names):
            if name is None:
                continue
            for tag, mut, exc in muts:
                if (shim, name, tag) in (("latent_norm_cf", "x", "strided"), ("tile_blend_accum", "acc", "shape")):
                    continue       # rows may carry a leading dimension (its own case below); acc defines the volume
                bad = list(args)
                # where a longer last dimension is a legal operand (more channels, a larger tile or box): one dimension too many
                bad[i] = args[i][None] if tag == "shape" and shim in ("d2s_add", "tile_blend_accum") else mut(args[i])
                # a longer first operand is the one the sizes derive from: the mismatch is then reported under its partner's name
                yield f"{shim}.{name}.{tag}", shim, tuple(bad), kw, exc, "" if (i == 0 and tag == "shape" and bad[i].dim() == args[i].dim()) else name
        for key, val in kw.items():
            for tag, mut, exc in muts:
                if key == "act":
                    for v in ("scale", "shift"):
                        yield f"{shim}.act.{v}.{tag}", shim, args, dict(kw, act=dict(val, **{v: mut(val[v])})), exc, v
                else:
                    yield f"{shim}.{key}.{tag}", shim, args, dict(kw, **{key: mut(val)}), exc, key
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


@pytest.mark.parametrize("shim", sorted(GOOD))
def test_well_formed_cpu_operands_are_refused_for_the_device_only(shim):
    from mlx_video_amd import _lib, ops
    args, kw, _ = GOOD[shim]
    with pytest.raises(_lib.LtxkError, match=f"{shim}: .* device tensor"):
        getattr(ops, shim)(*args, **kw)
    with pytest.raises(_lib.LtxkError, match=f"{shim}: .* device tensor"):
        getattr(ops, shim)(*args)


@pytest.mark.parametrize("shim,args,kw,exc,operand", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_shims_refuse_bad_operands_before_any_launch(shim, args, kw, exc, operand):
    """Follows test_guiders_cpu.py::test_ops_refuse_bad_arguments_before_any_launch: CPU tensors throughout, so a refusal
    other than the device's proves that it comes before the device check - and before any pointer reaches the library."""
    from mlx_video_amd import ops
    with pytest.raises(exc, match=f"{shim}: .*{operand}"):
        getattr(ops, shim)(*args, **kw)


def test_refusal_table_covers_every_shim_three_ways():
    for shim in GOOD:
        tags = {c[0].rsplit(".", 1)[1] for c in CASES if c[1] == shim}
        assert {"dtype", "shape", "strided"} <= tags, (shim, tags)


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


# ------------------------------------------------------------------------------------------------- constructors
def _decoder_weights(dtype):
    return {"conv_in.conv.weight": z(8, 3, 3, 3, 8, dtype=dtype), "conv_out.conv.weight": z(8, 3, 3, 3, 8, dtype=dtype),
            "up_blocks.1.conv.weight": z(8, 3, 3, 3, 8, dtype=dtype), "latents_mean": z(128, dtype=dtype), "latents_std": z(128, dtype=dtype)}


def _encoder_weights(dtype):
    return {"conv_in.weight": z(8, 3, 3, 3, 64, dtype=dtype), "conv_out.weight": z(129, 3, 3, 3, 8, dtype=dtype),
            "conv_out.bias": z(129, dtype=dtype), "per_channel_statistics.mean": z(128, dtype=dtype),
            "per_channel_statistics.std": z(128, dtype=dtype)}


def _upsampler_weights(dtype):
    return {"initial_conv.weight": z(8, 3, 3, 3, 8, dtype=dtype), "upsampler.conv.weight": z(32, 3, 3, 8, dtype=dtype),
            "initial_norm.weight": z(8, dtype=dtype)}


@pytest.mark.parametrize("which", ["decoder", "encoder", "upsampler"])
def test_constructors_keep_bf16_weights_and_convert_the_rest(which):
    from mlx_video_amd.upsampler import LatentUpsampler
    from mlx_video_amd.video_vae import LTX2VideoDecoder, VideoEncoder
    cls, make = {"decoder": (LTX2VideoDecoder, _decoder_weights), "encoder": (VideoEncoder, _encoder_weights),
                 "upsampler": (LatentUpsampler, _upsampler_weights)}[which]
    w32 = make(F32)
    m = cls(w32)
    assert all(m.W[k].dtype == BF and m.W[k].is_contiguous() for k in w32)
    wbf = make(BF)
    m = cls(wbf)
    assert all(m.W[k] is wbf[k] for k in wbf)                                  # no copy, no launch
    strided = {k: nc(v) for k, v in make(BF).items()}
    m = cls(strided)
    assert all(m.W[k].is_contiguous() and m.W[k].dtype == BF for k in strided)
