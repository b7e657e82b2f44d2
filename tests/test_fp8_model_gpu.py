"""FP8 (e4m3) weight storage through the model and the pipeline, on the small config of test_dit_gpu's forward test.

"none" scaling is exactly checkable: every e4m3 value is a bf16 value and the W8 GEMMs give the bf16 GEMMs' bits on the
converted panel (tests/test_gemm_w8_gpu.py), so an fp8 model equals the bf16 model built from the converted weights bit for bit -
eager, replayed from a captured graph, and in batch-invariant mode.  "channel" scaling changes the numbers; it is held to the
tolerance test_forward_small states against the fp32 oracle (3e-2 relative L2), the oracle running the dequantised weights."""
import numpy as np
import pytest
import torch

from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def _cfgs():
    from mlx_video_amd.ltx_model import LTXModelConfig
    cfg = O.DiTConfig(num_layers=2, heads=4, caption_channels=256)
    return cfg, LTXModelConfig(num_attention_heads=4, num_layers=2, caption_channels=256, cross_attention_dim=cfg.dim)


@pytest.fixture(scope="module")
def small(dev):
    """The oracle's weights on the device, their fp8 dicts, and one input - built once, never modified."""
    from mlx_video_amd.ltx_model import Modality
    from mlx_video_amd.weights import transformer_weights
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
    return dict(cfg=cfg, mc=mc, W=W, Wdev={k: v.to(dev) for k, v in W.items()}, lat=lat, ctx=ctx, ts=ts, pos=pos, mod=mod,
                none=transformer_weights(W, dev, fp8=True, fp8_scaling="none"),
                channel=transformer_weights(W, dev, fp8=True, fp8_scaling="channel"))


def _upcast(w8dict):
    return {k: (v.to(BF) if v.dtype == F8 else v) for k, v in w8dict.items() if not k.endswith("_scale")}


@pytest.mark.parametrize("mode", ["eager", "graph", "batch_invariant"])
def test_fp8_model_plain_cast_equals_bf16_model_of_upcast_weights(dev, small, mode):
    from mlx_video_amd.ltx_model import LTXModel
    assert not any(k.endswith("_scale") for k in small["none"]) and small["none"]["proj_out.weight"].dtype == F8
    m8, mb = LTXModel(small["mc"], small["none"]), LTXModel(small["mc"], _upcast(small["none"]))
    assert m8.weight_dtype == F8 and mb.weight_dtype == BF
    m8.batch_invariant = mb.batch_invariant = mode == "batch_invariant"
    from mlx_video_amd.ltx_model import TimestepPlan, precompute_freqs_cis
    mod = small["mod"]
    # the step's own inputs built outside the capture (host tables), as the denoise loops do
    pe = precompute_freqs_cis(mod.positions, m8.inner_dim, m8.positional_embedding_theta, m8.positional_embedding_max_pos, m8.num_attention_heads)
    plan = TimestepPlan.from_timesteps(mod.timesteps)
    outs = []
    for m in (m8, mb):
        v = m.forward_tokens(mod.latent, plan, mod.context, pe)          # (also the warm-up a capture needs)
        if mode == "graph":
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                v = m.forward_tokens(mod.latent, plan, mod.context, pe)
            gr.replay()
        torch.cuda.synchronize()
        outs.append(v.clone())
    assert bool(torch.isfinite(outs[0].float()).all())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_fp8_model_channel_scaling_within_the_small_forward_tolerance(dev, small):
    from mlx_video_amd.ltx_model import LTXModel
    from mlx_video_amd.weights import dequantize_fp8
    w = small["channel"]
    assert w["proj_out.weight"].dtype == F8 and w["proj_out.weight_scale"].dtype == torch.float32
    assert w["proj_out.bias"].dtype == BF and w["transformer_blocks.0.scale_shift_table"].dtype == BF
    m8 = LTXModel(small["mc"], w)
    v, _ = m8(video=small["mod"])
    torch.cuda.synchronize()
    Wd = {k: (dequantize_fp8(t, w.get(k + "_scale")).cpu() if t.dtype == F8 else t.cpu()) for k, t in w.items() if not k.endswith("_scale")}
    cfg = small["cfg"]
    pe = O.precompute_freqs_cis(small["pos"][:1], cfg.dim, heads=cfg.heads)
    ref_f = O.ltx_forward(small["lat"].float(), small["ts"].float(), small["ctx"].float(), pe, Wd, cfg, O.F32)
    err = float((v.double().cpu() - ref_f.double()).norm() / ref_f.double().norm())
    print(f"fp8 channel-scaled forward vs fp32 oracle on the dequantised weights: rel-L2 {err:.3e}")
    assert err < 3e-2                                   # test_dit_gpu.test_forward_small's bound against the fp32 oracle


def test_fp8_model_weight_bytes_and_views(dev, small):
    from mlx_video_amd import lora
    from mlx_video_amd.ltx_model import LTXModel
    mb = LTXModel(small["mc"], small["Wdev"])
    m8 = LTXModel(small["mc"], small["channel"])
    assert mb.weight_bytes() == sum(v.numel() * v.element_size() for v in small["Wdev"].values())
    # half the matrix bytes, plus the biases, norm weights and tables (bf16) and the scale vectors
    assert m8.weight_bytes() < 0.52 * mb.weight_bytes()
    assert isinstance(mb.weight_views(), dict)
    with pytest.raises(TypeError, match="fresh-copy"):
        m8.weight_views()
    with pytest.raises(TypeError, match="in_place=False"):      # a LoRA delta never goes into an e4m3 panel
        k = "transformer_blocks.0.attn1.to_q.weight"
        D = small["cfg"].dim
        sd = {"transformer_blocks.0.attn1.to_q.lora_A.weight": torch.zeros(8, D, dtype=BF, device=dev),
              "transformer_blocks.0.attn1.to_q.lora_B.weight": torch.zeros(D, 8, dtype=BF, device=dev)}
        p = __import__("pathlib").Path("unused")
        lora.apply_lora_to_weights({k: small["channel"][k]}, [lora.LoraSpec(p, 1.0)], lora_states={p: sd})


def test_distilled_pipeline_with_fp8(dev):
    """One end-to-end two-stage run at the smallest geometry of test_pipeline_gpu (128x128x9) with enable_fp8: generate_video
    quantises the weight dict it is given and both stages run on the fp8 transformer."""
    from oracle import vae as OV
    from mlx_video_amd import ops
    from mlx_video_amd.generate import PipelineType, generate_video
    from mlx_video_amd.upsampler import LatentUpsampler
    from mlx_video_amd.video_vae import LTX2VideoDecoder
    cfg, mc = _cfgs()
    W = {k: v.to(dev) for k, v in O.make_weights(cfg, seed=31).items()}
    dec = LTX2VideoDecoder({k: v.to(dev) for k, v in OV.make_decoder_weights(seed=32, layers_per_block=1).items()}, num_layers_per_block=1)
    ups = LatentUpsampler({k: v.to(dev) for k, v in OV.make_upsampler_weights(mid=128, nb=1).items()}, num_blocks_per_stage=1)
    emb = torch.randn(1, 64, 256, generator=torch.Generator().manual_seed(51)).to(BF)
    ops.TIMER = ops.KernelTimer()
    try:
        frames = generate_video(prompt="x", pipeline=PipelineType.DISTILLED, height=128, width=128, num_frames=9, stage1_steps=2,
                                stage2_steps=1, transformer_weights=W, transformer_config=mc, vae_decoder=dec, upsampler=ups,
                                prompt_embeds=emb, device=dev, seed=3, enable_fp8=True)
        fams = {r[0] for r in ops.TIMER.records}
    finally:
        ops.TIMER = None
    assert frames.shape == (9, 128, 128, 3) and frames.dtype == np.uint8
    assert 5 < frames.mean() < 250
    assert "gemm_w8" in fams                                 # the transformer really ran on fp8 panels
    assert all(v.dtype == BF for v in W.values())            # the caller's dict is untouched
