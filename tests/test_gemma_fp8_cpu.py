"""FP8 Gemma-3 panels, the parts that need no GPU: the two new C entries and their host-side refusals, the refusals of
``ops.gemm(gemv=True)`` and ``ops.embed_rows(row_scale=)`` on CPU tensors (each names its operand and arrives before the device
refusal), per-row scales under concatenation, the streaming loader, ``GemmaEncoder(fp8=)``'s panels, and the CLI flag."""
import ctypes
import inspect

import pytest
import torch

from test_fp8_cpu import _write_safetensors

BF, F8, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.float32


def z(*shape, dtype=BF):
    return torch.zeros(shape, dtype=dtype)


def f8(*shape):
    return torch.zeros(shape, dtype=torch.uint8).view(F8)


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_exported_and_bound():
    from mlx_video_amd import _lib
    lib = _lib.load()
    for name in ("ltxk_gemv_w8", "ltxk_embed_rows_fp8"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None and hasattr(lib, name)
    assert lib.ltxk_abi_sizeof(0) == ctypes.sizeof(_lib.GemmArgs)          # ltxk_gemm_args is unchanged
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "ltxk.h")).read()
    assert "int ltxk_gemv_w8(" in hdr and "int ltxk_embed_rows_fp8(" in hdr


def _args(M, N, K, /, **over):
    from mlx_video_amd._lib import GemmArgs
    a = GemmArgs()
    a.A = a.W = a.out = 1 << 12
    a.M, a.N, a.K, a.lda, a.ldo = M, N, K, K, N
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_gemv_entry_refuses_on_the_host():
    """Every argument outside the entry's contract is LTXK_EINVAL with a message, before anything is launched (no device here)."""
    from mlx_video_amd import _lib
    lib = _lib.load()
    bad = [dict(M=0), dict(M=9), dict(N=0), dict(K=24), dict(K=0), dict(epilogue=1), dict(epilogue=4, resid=1 << 12, ldr=64),
           dict(resid=1 << 12), dict(gate=1 << 12), dict(gate_row=1 << 12), dict(out2=1 << 12), dict(n_split=8),
           dict(out_tokens_per_batch=1), dict(sumsq=1 << 12), dict(workspace=1 << 12, workspace_bytes=1 << 20), dict(lda=16),
           dict(lda=36), dict(ldo=4), dict(A=0), dict(W=0), dict(out=0), dict(A=(1 << 12) + 8), dict(W=(1 << 12) + 8)]
    for over in bad:
        assert lib.ltxk_gemv_w8(ctypes.byref(_args(2, 8, 32, **over)), None, None) == -1, over
        assert lib.ltxk_last_error().startswith(b"ltxk_gemv_w8"), over
    assert lib.ltxk_gemv_w8(None, None, None) == -1
    assert lib.ltxk_gemv_w8(ctypes.byref(_args(2, 8, 32)), ctypes.c_void_p((1 << 12) + 2), None) == -1 and b"w_scale" in lib.ltxk_last_error()


def test_embed_rows_fp8_entry_refuses_on_the_host():
    from mlx_video_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 12)
    good = dict(table=p, rs=None, V=8, D=32, ids=p, out=p, ldo=32, M=2)
    for over in (dict(D=24), dict(D=8), dict(ldo=16), dict(ldo=36), dict(V=0), dict(M=0), dict(table=None), dict(out=ctypes.c_void_p((1 << 12) + 8)),
                 dict(rs=ctypes.c_void_p((1 << 12) + 2))):
        a = dict(good, **over)
        rc = lib.ltxk_embed_rows_fp8(a["table"], a["rs"], a["V"], a["D"], a["ids"], a["out"], a["ldo"], a["M"], 1.0, None)
        assert rc == -1 and lib.ltxk_last_error().startswith(b"ltxk_embed_rows_fp8"), over


# -------------------------------------------------------------------------------------------------------------- the shims
def test_gemv_shim_refusals_name_the_operand_before_the_device():
    from mlx_video_amd import _lib, ops
    assert ops.GEMV_MAX_M == 8 and inspect.signature(ops.gemm).parameters["gemv"].default is False
    a, w, b, sc = z(2, 32), f8(8, 32), z(8), z(8, dtype=F32)
    with pytest.raises(_lib.LtxkError, match="device tensor"):              # the call these are mutations of: only the device refuses
        ops.gemm(a, w, b, w_scale=sc, out=z(2, 8), gemv=True)
    with pytest.raises(TypeError, match="`w`"):
        ops.gemm(a, z(8, 32), b, gemv=True)
    with pytest.raises(ValueError, match="`a` of 1 to 8 rows"):
        ops.gemm(z(9, 32), w, b, gemv=True)
    with pytest.raises(ValueError, match="K % 16"):
        ops.gemm(z(2, 24), f8(8, 24), b, gemv=True)
    with pytest.raises(ValueError, match="`epilogue`"):
        ops.gemm(a, w, b, epilogue=ops.EPI_BIAS_GELU, gemv=True)
    for name, kw in (("out2", dict(out2=z(1, 4, 8), n_split=4, out_tokens_per_batch=2, out=z(2, 4))), ("n_split", dict(n_split=4, out2=None)),
                     ("out_tokens_per_batch", dict(out_tokens_per_batch=2, out=z(1, 8, 8))), ("sumsq", dict(sumsq=z(2, 1, dtype=F32))),
                     ("resid", dict(resid=z(2, 8))), ("gate", dict(gate=z(1, 8))), ("gate_row", dict(gate_row=z(2, dtype=torch.int32)))):
        with pytest.raises(ValueError, match=f"`{name}`"):
            ops.gemm(a, w, b, gemv=True, **kw)
    with pytest.raises((TypeError, ValueError), match="a_scale"):
        ops.gemm(f8(2, 32), w, b, a_scale=z(2, dtype=F32), gemv=True)
    # the operand checks of _operands: dtype, shape, layout, alignment - each before the device
    with pytest.raises(TypeError, match="a must be"):
        ops.gemm(z(2, 32, dtype=F32), w, b, gemv=True)
    with pytest.raises(TypeError, match="bias must be"):
        ops.gemm(a, w, z(8, dtype=F32), gemv=True)
    with pytest.raises(ValueError, match="bias must be"):
        ops.gemm(a, w, z(7), gemv=True)
    with pytest.raises(ValueError, match="out must be"):
        ops.gemm(a, w, b, out=z(2, 9), gemv=True)
    with pytest.raises(TypeError, match="w_scale must be"):
        ops.gemm(a, w, b, w_scale=z(8), gemv=True)
    with pytest.raises(ValueError, match="w_scale must be"):
        ops.gemm(a, w, b, w_scale=z(9, dtype=F32), gemv=True)
    with pytest.raises(ValueError, match="w must be"):
        ops.gemm(a, f8(8, 64)[:, :32], b, gemv=True)
    with pytest.raises(ValueError, match="a must be 16-byte aligned"):
        ops.gemm(z(2, 40)[:, 4:36], w, b, gemv=True)
    with pytest.raises(ValueError, match="rows of `a`"):
        ops.gemm(z(2, 36)[:, :32], w, b, gemv=True)
    with pytest.raises(_lib.LtxkError, match="device tensor"):              # a row stride of K + 8 is fine
        ops.gemm(z(2, 40)[:, :32], w, None, gemv=True)
    # gemv=False is the call it was
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        ops.gemm(a, w, b, w_scale=sc)


def test_embed_rows_shim_refusals():
    from mlx_video_amd import _lib, ops
    ids = z(3, dtype=torch.int32)
    with pytest.raises(TypeError, match="row_scale goes with"):
        ops.embed_rows(z(16, 32), ids, 2.0, row_scale=z(16, dtype=F32))
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.embed_rows(f8(16, 24), ids, 2.0)
    with pytest.raises(TypeError, match="row_scale must be"):
        ops.embed_rows(f8(16, 32), ids, 2.0, row_scale=z(16))
    with pytest.raises(ValueError, match="row_scale must be"):
        ops.embed_rows(f8(16, 32), ids, 2.0, row_scale=z(15, dtype=F32))
    with pytest.raises(ValueError, match="out must be"):
        ops.embed_rows(f8(16, 32), ids, 2.0, out=z(3, 16))
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        ops.embed_rows(f8(16, 32), ids, 2.0, row_scale=z(16, dtype=F32), ids_host=ids)
    with pytest.raises(_lib.LtxkError, match="device tensor"):              # a bf16 table is the call it was
        ops.embed_rows(z(16, 32), ids, 2.0, ids_host=ids)


# -------------------------------------------------------------------------------------------------- weights and the encoder
def _tiny():
    from mlx_video_amd.gemma import GemmaConfig, random_gemma_weights
    cfg = GemmaConfig(hidden_size=32, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=256,
                      intermediate_size=48, vocab_size=40, sliding_window=8, sliding_window_pattern=2)
    W = random_gemma_weights("cpu", cfg, seed=11)
    # rows of very different sizes, so that a per-row scale that strayed to another row would show
    for k in W:
        if W[k].ndim == 2:
            W[k] = (W[k].float() * torch.logspace(-2, 1, W[k].shape[0])[:, None]).to(BF)
    return cfg, W


def test_concatenated_scales_are_the_scale_of_the_concatenated_panel():
    from mlx_video_amd.gemma import GemmaEncoder
    from mlx_video_amd.weights import quantize_fp8
    cfg, W = _tiny()
    p = "layers.1.self_attn."
    parts = [quantize_fp8(W[p + f"{n}_proj.weight"], "channel") for n in "qkv"]
    whole8, whole_s = quantize_fp8(torch.cat([W[p + f"{n}_proj.weight"] for n in "qkv"], 0), "channel")
    assert torch.equal(torch.cat([s for _, s in parts]), whole_s)
    assert torch.equal(torch.cat([w.view(torch.uint8) for w, _ in parts]), whole8.view(torch.uint8))
    enc = GemmaEncoder(dict(W), cfg, fp8="channel")
    ly = enc.layers[1]
    assert torch.equal(ly["qkv"].view(torch.uint8), whole8.view(torch.uint8)) and torch.equal(ly["qkv_s"], whole_s)
    g8, gs = quantize_fp8(torch.cat([W["layers.1.mlp.gate_proj.weight"], W["layers.1.mlp.up_proj.weight"]], 0), "channel")
    assert torch.equal(ly["gu"].view(torch.uint8), g8.view(torch.uint8)) and torch.equal(ly["gu_s"], gs)


def test_encoder_panels_dtypes_bytes_and_release():
    from mlx_video_amd.gemma import GemmaEncoder
    from mlx_video_amd.weights import SCALE_SUFFIX, dequantize_fp8, quantize_fp8
    cfg, W = _tiny()
    ref = GemmaEncoder(dict(W), cfg)
    assert ref.weight_dtype == BF and ref.embed_row_scale is None and ref.layers[0]["qkv_s"] is None
    assert torch.equal(ref.embed, W["embed_tokens.weight"])
    assert ref.weight_bytes() == sum(v.numel() * 2 for v in W.values())
    src = dict(W)
    enc = GemmaEncoder(src, cfg, fp8="channel")
    assert enc.weight_dtype == F8
    assert not any(v.ndim == 2 for v in src.values()), "a consumed bf16 matrix is still held by the dict"       # released as consumed
    assert set(src) == {k for k, v in W.items() if v.ndim == 1}
    for name in ("qkv", "o", "gu", "down"):
        assert enc.layers[0][name].dtype == F8 and enc.layers[0][name + "_s"].dtype == F32
        assert enc.layers[0][name + "_s"].shape == (enc.layers[0][name].shape[0],)
    assert enc.embed.dtype == F8 and enc.embed_row_scale.shape == (cfg.vocab_size,) and enc.norm.dtype == BF and enc.layers[0]["qn"].dtype == BF
    mats = sum(v.numel() for v in W.values() if v.ndim == 2)
    rows = sum(v.shape[0] for v in W.values() if v.ndim == 2)
    assert enc.weight_bytes() == mats + 4 * rows + sum(v.numel() * 2 for v in W.values() if v.ndim == 1)
    # a dequantised row lies within amax * 2^-4 of the original
    w = W["layers.0.mlp.down_proj.weight"]
    err = (dequantize_fp8(enc.layers[0]["down"], enc.layers[0]["down_s"], torch.float64) - w.double()).abs()
    assert bool((err <= w.double().abs().amax(1, keepdim=True) * 2.0 ** -4).all())
    # "none": the plain cast, no scales
    plain = GemmaEncoder(dict(W), cfg, fp8="none")
    assert plain.embed_row_scale is None and plain.layers[1]["o_s"] is None
    assert torch.equal(plain.layers[1]["o"].view(torch.uint8), W["layers.1.self_attn.o_proj.weight"].to(F8).view(torch.uint8))
    # a dict that already holds e4m3 matrices is taken as it is, with or without fp8=
    Q = {}
    for k, v in W.items():
        if v.ndim == 2:
            Q[k], Q[k + SCALE_SUFFIX] = quantize_fp8(v, "channel")
        else:
            Q[k] = v
    for kw in ({}, {"fp8": "none"}):
        taken = GemmaEncoder(dict(Q), cfg, **kw)
        assert taken.weight_dtype == F8 and torch.equal(taken.layers[0]["qkv"].view(torch.uint8), enc.layers[0]["qkv"].view(torch.uint8))
        assert torch.equal(taken.layers[0]["qkv_s"], enc.layers[0]["qkv_s"]) and torch.equal(taken.embed_row_scale, enc.embed_row_scale)
    unscaled = {k: v for k, v in Q.items() if not k.endswith(SCALE_SUFFIX)}
    assert GemmaEncoder(unscaled, cfg).layers[0]["qkv_s"] is None
    mixed = dict(Q)
    mixed["layers.0.self_attn.o_proj.weight"] = W["layers.0.self_attn.o_proj.weight"]
    with pytest.raises(ValueError, match="o_proj.weight"):
        GemmaEncoder(mixed, cfg)
    with pytest.raises(ValueError, match="fp8="):
        GemmaEncoder(dict(W), cfg, fp8="group")


def test_gemma_weights_streams_to_fp8(tmp_path):
    from mlx_video_amd.weights import SCALE_SUFFIX, gemma_weights, quantize_fp8
    cfg, W = _tiny()
    kept = W["layers.0.self_attn.o_proj.weight"].to(F8)                    # an F8_E4M3 tensor of the checkpoint
    ck = {"language_model.model." + k: v for k, v in W.items()}
    ck["language_model.model.layers.0.self_attn.o_proj.weight"] = kept
    _write_safetensors(tmp_path / "model.safetensors", ck)
    on = gemma_weights(tmp_path, "cpu", fp8="channel")
    for k, v in W.items():
        if v.ndim == 1:
            assert on[k].dtype == BF and torch.equal(on[k], v) and k + SCALE_SUFFIX not in on
        elif k == "layers.0.self_attn.o_proj.weight":
            assert torch.equal(on[k].view(torch.uint8), kept.view(torch.uint8)) and k + SCALE_SUFFIX not in on      # as it is, unscaled
        else:
            w8, sc = quantize_fp8(v, "channel")
            assert on[k].dtype == F8 and torch.equal(on[k].view(torch.uint8), w8.view(torch.uint8)) and torch.equal(on[k + SCALE_SUFFIX], sc)
    plain = gemma_weights(tmp_path, "cpu", fp8="none")
    assert not any(k.endswith(SCALE_SUFFIX) for k in plain) and plain["embed_tokens.weight"].dtype == F8
    assert gemma_weights(tmp_path, "cpu", fp8=True, fp8_scaling="none").keys() == plain.keys()
    off = gemma_weights(tmp_path, "cpu")
    assert all(v.dtype == BF for v in off.values()) and set(off) == set(W)
    with pytest.raises(ValueError, match="fp8 scaling"):
        gemma_weights(tmp_path, "cpu", fp8="group")


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_flag_and_refusals(monkeypatch):
    from mlx_video_amd import generate as GV
    from mlx_video_amd.gemma import GemmaEncoder
    assert inspect.signature(GV.generate_video).parameters["fp8_text_encoder"].default is False
    ap = GV.build_parser()
    assert ap.parse_args([]).fp8_text_encoder is False and ap.parse_args(["--fp8-text-encoder"]).fp8_text_encoder is True
    seen = {}
    monkeypatch.setattr(GV, "generate_video", lambda **kw: seen.update(kw))
    GV.main(["--prompt", "x", "--model-repo", "/nonexistent", "--gemma-repo", "/nonexistent-gemma", "--fp8-text-encoder", "--fp8-scaling", "none"])
    assert seen["fp8_text_encoder"] is True and seen["fp8_scaling"] == "none" and seen["enable_fp8"] is False
    seen.clear()
    GV.main(["--prompt", "x", "--model-repo", "/nonexistent", "--enable-fp8"])          # --enable-fp8 alone: the transformer only
    assert "fp8_text_encoder" not in seen and seen["enable_fp8"] is True
    with pytest.raises(ValueError, match="--gemma-repo"):
        GV.main(["--prompt", "x", "--model-repo", "/nonexistent", "--fp8-text-encoder"])
    monkeypatch.undo()
    cfg, W = _tiny()
    base = dict(prompt="x", transformer=object(), vae_decoder=object(), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="drop fp8_text_encoder.*or drop gemma="):
        GV.generate_video(gemma=GemmaEncoder(dict(W), cfg), fp8_text_encoder=True, **base)
    with pytest.raises(ValueError, match="gemma_repo="):
        GV.generate_video(fp8_text_encoder=True, **base)
