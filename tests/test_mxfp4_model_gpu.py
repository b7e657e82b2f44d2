"""The MXFP4 DiT (ltxk_gemm_mxfp4 in-block GEMMs) through the model and the pipeline, on the 2-block small config of
test_fp8_act_model_gpu (D = 512: every K is a multiple of 256).

Bitwise: eager == graph replay; with batch_invariant a B = 1 forward gives the matching rows of the B = 2 forward (every in-block
launch is the one single-pass kernel and quantisation is per row).  Launches are counted: seven ltxk_gemm_mxfp4 per block, one
context quantisation per forward, none on a forward that is handed a prepared ContextKV.

Accuracy is a condition on the kernel route, not a preset tolerance on the format.  *emu* is the same model with ops.gemm_mxfp4
replaced, in the test only, by: dequantise both operands to bf16 on the device (exact: e2m1 x 2^e is a bf16 value) and call the
existing bf16 ops.gemm.  It feeds identical quantised operands to tested code and differs from the new route in the fp32 summation
order alone.  With e = rel-L2(new, emu) and d = rel-L2(emu, bf16 forward on the original weights) the test asserts e <= 0.1 d: a
wrong fragment, nibble or scale mapping leaves e of the order of d or above.  e, d and d's ratio to the W8A8 figure of this config
(3.76e-2) go to the parity ledger."""
import numpy as np
import pytest
import torch

import parity
from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U8 = torch.uint8
D_W8A8 = 3.76e-2          # rel-L2 of the W8A8 forward to the bf16 forward on this config (tests/test_fp8_act_model_gpu.py)


def _cfgs():
    from mlx_video_amd.ltx_model import LTXModelConfig
    cfg = O.DiTConfig(num_layers=2, heads=4, caption_channels=256)
    return cfg, LTXModelConfig(num_attention_heads=4, num_layers=2, caption_channels=256, cross_attention_dim=cfg.dim)


@pytest.fixture(scope="module")
def small(dev):
    """Weights (bf16 on the device and their MXFP4 dict), one input and its step tables - built once, never modified."""
    from mlx_video_amd.ltx_model import LTXModel, Modality, TimestepPlan, precompute_freqs_cis
    from mlx_video_amd.weights import quantize_transformer_weights_mxfp4
    cfg, mc = _cfgs()
    W = O.make_weights(cfg, seed=11)
    B, F, Hh, Ww, S = 2, 3, 5, 6, 100
    N = F * Hh * Ww
    g = torch.Generator().manual_seed(42)
    lat = torch.randn(B, N, 128, generator=g).to(BF)
    ctx = torch.randn(B, S, cfg.caption_channels, generator=g).to(BF)
    ts = torch.full((B, N), 0.909375).to(BF)
    ts[:, : Hh * Ww] = 0.0
    pos = torch.from_numpy(O.create_position_grid(B, F, Hh, Ww))
    mod = Modality(latent=lat.to(dev), timesteps=ts.to(dev), positions=pos.to(dev), context=ctx.to(dev))
    Wdev = {k: v.to(dev) for k, v in W.items()}
    w4 = quantize_transformer_weights_mxfp4(Wdev)
    m = LTXModel(mc, w4)
    pe = precompute_freqs_cis(mod.positions, m.inner_dim, m.positional_embedding_theta, m.positional_embedding_max_pos, m.num_attention_heads)
    return dict(cfg=cfg, mc=mc, Wdev=Wdev, w4=w4, mod=mod, pe=pe, B=B, N=N, S=S, plan=TimestepPlan.from_timesteps(mod.timesteps))


def _model(small):
    from mlx_video_amd.ltx_model import LTXModel
    return LTXModel(small["mc"], small["w4"])


def _fwd(m, small, **kw):
    mod = small["mod"]
    v = m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"], **kw).clone()
    torch.cuda.synchronize()
    return v


def test_model_recognises_the_dict(dev, small):
    from mlx_video_amd.ltx_model import LTXModel, MXFP4
    m, mb = _model(small), LTXModel(small["mc"], small["Wdev"])
    assert m.weight_dtype == MXFP4 and m.weight_dtype not in (BF, torch.float8_e4m3fn) and mb.weight_dtype == BF
    blk = m.blocks[0]
    D = m.inner_dim
    assert blk.qkv.w.dtype == U8 and tuple(blk.qkv.w.shape) == (3 * D, D // 2) and tuple(blk.qkv.mx.shape) == (3 * D, D // 32)
    assert tuple(blk.kv2.w.shape) == (2 * D, D // 2) and blk.ff1.K == D and blk.ff2.K == 4 * D
    assert m.patchify.w.dtype == BF and m.patchify.mx is None and m.out.w.dtype == BF and m.ada.w.dtype == BF
    # q|k|v packs row-wise: the rows of to_k are rows D..2D of the panel, codes and scales alike
    k = "transformer_blocks.0.attn1.to_k.weight"
    assert torch.equal(blk.qkv.w[D:2 * D], small["w4"][k]) and torch.equal(blk.qkv.mx[D:2 * D], small["w4"][k + "_mxscale"])
    # weight_bytes counts codes and scales: the in-block matrices at 4.25 bits per weight, everything else bf16
    mats = sum(v.numel() for k, v in small["Wdev"].items() if k + "_mxscale" in small["w4"])
    rest = sum(v.numel() * 2 for k, v in small["Wdev"].items() if k + "_mxscale" not in small["w4"])
    assert m.weight_bytes() == mats * 17 // 32 + rest and mb.weight_bytes() == mats * 2 + rest
    with pytest.raises(TypeError, match="MXFP4.*fresh-copy"):
        m.weight_views()
    # the joint model takes bf16 sub-models only
    from mlx_video_amd.av_model import LTXAVModel
    from mlx_video_amd.ltx_model import LTXModelConfig
    audio = LTXModel.random_init(LTXModelConfig.audio(num_attention_heads=4, num_layers=2, cross_attention_dim=256, caption_channels=256), dev)
    with pytest.raises(ValueError, match="bf16 sub-models"):
        LTXAVModel(m, audio, {})


def test_eager_equals_graph_replay(dev, small):
    m, mod = _model(small), small["mod"]
    v = _fwd(m, small)                                                # (also the warm-up a capture needs)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        vg = m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"])
    gr.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v.float()).all())
    assert torch.equal(v.view(torch.int16), vg.view(torch.int16))


def test_batch_invariant_rows(dev, small):
    from mlx_video_amd.ltx_model import TimestepPlan
    m, mod = _model(small), small["mod"]
    m.batch_invariant = True
    both = _fwd(m, small)
    for b in range(small["B"]):
        one = m.forward_tokens(mod.latent[b:b + 1].contiguous(), TimestepPlan.from_timesteps(mod.timesteps[b:b + 1]),
                               mod.context[b:b + 1].contiguous(), small["pe"])
        torch.cuda.synchronize()
        assert torch.equal(one[0].view(torch.int16), both[b].view(torch.int16)), f"row {b} depends on the batch"


def test_launch_accounting(dev, small, monkeypatch):
    from mlx_video_amd import ops
    m, mod = _model(small), small["mod"]
    rows, gemms = [], []
    real_q, real_g = ops.quant_rows_mxfp4, ops.gemm_mxfp4
    monkeypatch.setattr(ops, "quant_rows_mxfp4", lambda a, out=None: (rows.append(a.shape[0]), real_q(a, out=out))[1])
    monkeypatch.setattr(ops, "gemm_mxfp4", lambda *a, **kw: (gemms.append((a[0].shape[0], a[2].shape[0])), real_g(*a, **kw))[1])
    ops.TIMER = ops.KernelTimer()
    try:
        _fwd(m, small)
        fams = [r[0] for r in ops.TIMER.records]
    finally:
        ops.TIMER = None
    L, M, MS, D = 2, small["B"] * small["N"], small["B"] * small["S"], m.inner_dim
    assert M != MS
    assert rows.count(MS) == 1, f"the text context was quantised {rows.count(MS)} times in one forward"
    assert rows.count(M) == 6 * L            # nx (q|k|v), att, nx (q2), att, nx (FF1), hff per block
    # q|k|v, to_out, q2, text k|V^T, to_out2, FF1, FF2 per block - and nothing else runs on the new GEMM
    assert sorted(gemms) == sorted(L * [(M, 3 * D), (M, D), (M, D), (MS, 2 * D), (M, D), (M, 4 * D), (M, D)])
    assert fams.count("gemm_mxfp4") == 7 * L and fams.count("quant_rows_mxfp4") == 6 * L + 1
    assert "gemm_bf16" in fams and "gemm_w8" not in fams and "gemm_w8a8" not in fams      # patchify, AdaLN, caption projection, head: bf16
    # hoisted context: prepare_context quantises it once, and the forward then not at all
    rows.clear()
    kv = m.prepare_context(mod.context)
    assert rows.count(MS) == 1
    rows.clear()
    gemms.clear()
    _fwd(m, small, ctx_kv=kv)
    assert rows.count(MS) == 0 and rows.count(M) == 6 * L and len(gemms) == 6 * L


def test_kernel_route_adds_nothing_visible(dev, small, monkeypatch):
    from mlx_video_amd import ops
    from mlx_video_amd.ltx_model import LTXModel
    from mlx_video_amd.weights import dequantize_mxfp4
    new = _fwd(_model(small), small)

    def emu(a, a_scales, w, w_scales, bias=None, **kw):
        # (exact: every e2m1 x 2^e here is a bf16 value - scale bytes far inside 1..254)
        return ops.gemm(dequantize_mxfp4(a, a_scales, BF), dequantize_mxfp4(w, w_scales, BF), bias, split_k=False, **kw)

    monkeypatch.setattr(ops, "gemm_mxfp4", emu)
    emu_out = _fwd(_model(small), small)
    monkeypatch.undo()
    ref = _fwd(LTXModel(small["mc"], small["Wdev"]), small)
    e, d = parity.rel_l2(new, emu_out), parity.rel_l2(emu_out, ref)
    print(f"small forward: e = rel-L2(new, emu) = {e:.3e}, d = rel-L2(emu, bf16) = {d:.3e}, e / d = {e / d:.3e}, d / W8A8 = {d / D_W8A8:.2f}")
    name = "test_mxfp4_model_gpu::test_kernel_route_adds_nothing_visible"
    parity.LEDGER[name + "#d"] = {"measured": d, "note": "rel-L2 of the emulated MXFP4 forward to the bf16 forward (small config)"}
    parity.LEDGER[name + "#d_over_w8a8"] = {"measured": d / D_W8A8, "note": "d / 3.76e-2, the W8A8 figure of the same config"}
    parity.check(name + "#e", e, 0.1 * d, note="rel-L2 of the ltxk_gemm_mxfp4 forward to the emulated one; bound 0.1 x d of the same run")


def _pipeline_parts(dev):
    from oracle import vae as OV
    from mlx_video_amd.upsampler import LatentUpsampler
    from mlx_video_amd.video_vae import LTX2VideoDecoder
    cfg, mc = _cfgs()
    W = {k: v.to(dev) for k, v in O.make_weights(cfg, seed=31).items()}
    dec = LTX2VideoDecoder({k: v.to(dev) for k, v in OV.make_decoder_weights(seed=32, layers_per_block=1).items()}, num_layers_per_block=1)
    ups = LatentUpsampler({k: v.to(dev) for k, v in OV.make_upsampler_weights(mid=128, nb=1).items()}, num_blocks_per_stage=1)
    emb = torch.randn(2, 64, 256, generator=torch.Generator().manual_seed(51)).to(BF)
    return cfg, mc, W, dec, ups, emb


def test_pipelines_with_enable_mxfp4(dev, tmp_path):
    """Distilled (two stages) and dev (guided) at the smallest geometry, frames and latents: generate_video(enable_mxfp4=True) on
    the bf16 dict equals the same call on MXFP4 models built by hand; with a stage-2 LoRA, on merge-then-quantise done by hand."""
    from safetensors.torch import save_file

    from mlx_video_amd import lora, ops
    from mlx_video_amd.generate import PipelineType, generate_video
    from mlx_video_amd.ltx_model import LTXModel
    from mlx_video_amd.weights import quantize_transformer_weights_mxfp4
    cfg, mc, W, dec, ups, emb = _pipeline_parts(dev)
    hand = LTXModel(mc, quantize_transformer_weights_mxfp4(W))
    dist = dict(prompt="x", pipeline=PipelineType.DISTILLED, height=128, width=128, num_frames=9, stage1_steps=2, stage2_steps=1,
                vae_decoder=dec, upsampler=ups, prompt_embeds=emb[:1], device=dev, seed=3)
    ops.TIMER = ops.KernelTimer()
    try:
        frames = generate_video(transformer_weights=W, transformer_config=mc, enable_mxfp4=True, **dist)
        fams = {r[0] for r in ops.TIMER.records}
    finally:
        ops.TIMER = None
    assert frames.shape == (9, 128, 128, 3) and frames.dtype == np.uint8 and 5 < frames.mean() < 250
    assert "gemm_mxfp4" in fams and "quant_rows_mxfp4" in fams
    assert all(v.dtype == BF for v in W.values())                     # the caller's dict is untouched
    lat = generate_video(transformer_weights=W, transformer_config=mc, enable_mxfp4=True, return_latents=True, **dist)
    lat_hand = generate_video(transformer=hand, return_latents=True, **dist)
    assert bool(torch.isfinite(lat.float()).all()) and torch.equal(lat, lat_hand)
    # a LoRA merged into the stage-2 transformer: bf16 merge, then quantised
    g = torch.Generator().manual_seed(71)
    sd, Dm = {}, cfg.dim
    for i in range(cfg.num_layers):
        for raw in ("attn1.to_q", "attn2.to_out.0", "ff.net.0.proj"):
            o = 4 * Dm if raw.startswith("ff") else Dm
            sd[f"diffusion_model.transformer_blocks.{i}.{raw}.lora_A.weight"] = (torch.randn(8, Dm, generator=g) * 0.1).to(BF)
            sd[f"diffusion_model.transformer_blocks.{i}.{raw}.lora_B.weight"] = (torch.randn(o, 8, generator=g) * 0.1).to(BF)
    path = tmp_path / "lora.safetensors"
    save_file(sd, str(path))
    lat_l = generate_video(transformer_weights=W, transformer_config=mc, enable_mxfp4=True, return_latents=True,
                           distilled_loras=[(str(path), 0.8)], **dist)
    merged = lora.apply_lora_to_weights(W, [lora.LoraSpec(path, 0.8)])
    stage2 = LTXModel(mc, quantize_transformer_weights_mxfp4(merged))
    lat_l_hand = generate_video(transformer=hand, stage2_transformer=stage2, return_latents=True, **dist)
    assert torch.equal(lat_l, lat_l_hand) and not torch.equal(lat_l, lat)
    # dev pipeline (CFG pair as one B = 2 forward, captured step)
    devkw = dict(prompt="x", pipeline=PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
                 vae_decoder=dec, prompt_embeds=emb[:1], negative_prompt_embeds=emb[1:], compile_step=True, cfg_batch=True,
                 device=dev, seed=5, return_latents=True)
    lat_d = generate_video(transformer_weights=W, transformer_config=mc, enable_mxfp4=True, **devkw)
    lat_d_hand = generate_video(transformer=hand, **devkw)
    assert bool(torch.isfinite(lat_d.float()).all()) and torch.equal(lat_d, lat_d_hand)
    with pytest.raises(ValueError, match="enable_mxfp4.*enable_fp8"):
        generate_video(transformer_weights=W, transformer_config=mc, enable_mxfp4=True, enable_fp8=True, **dist)
