"""FP8 activations (W8A8 in-block GEMMs) through the model and the pipeline, on the 2-block small config of test_fp8_model_gpu.

Bitwise properties: eager == graph replay; with batch_invariant a B = 1 forward gives the matching rows of the B = 2 forward
(quantisation is per row).  The text context is quantised once per forward.  Accuracy is measured, not preset: with d8 the
relative L2 between the W8A16 forward and the bf16 forward on the original weights (both existing code) and dA the same for the
W8A8 forward, per-row e4m3 rounding of an activation has the relative step of per-channel e4m3 rounding of a weight, so
independent equal errors predict dA ~ sqrt(2) d8; the test asserts dA <= 2 d8 (the extra sqrt(2): correlation, softmax).

Measured on MI355X: d8 = 3.759e-2, dA = 3.762e-2, dA / d8 = 1.001 on this config; 6.106e-2, 6.571e-2, 1.076 on one L = 48,
D = 4096 forward (scripts/ab_fp8_act.py).  The test writes its three figures to the parity ledger."""
import numpy as np
import pytest
import torch

import parity
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
    """Weights (bf16 on the device and their channel-scaled fp8 dict), one input and its step tables - built once, never modified."""
    from mlx_video_amd.ltx_model import LTXModel, Modality, TimestepPlan, precompute_freqs_cis
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
    w8 = transformer_weights(W, dev, fp8=True, fp8_scaling="channel")
    mA = LTXModel(mc, w8, fp8_activations=True)
    pe = precompute_freqs_cis(mod.positions, mA.inner_dim, mA.positional_embedding_theta, mA.positional_embedding_max_pos, mA.num_attention_heads)
    return dict(cfg=cfg, mc=mc, Wdev={k: v.to(dev) for k, v in W.items()}, w8=w8, mod=mod, pe=pe, B=B, N=N, S=S,
                plan=TimestepPlan.from_timesteps(mod.timesteps))


def _model(small, **kw):
    from mlx_video_amd.ltx_model import LTXModel
    return LTXModel(small["mc"], small["w8"], **kw)


def test_fp8_activations_need_fp8_weights(dev, small):
    from mlx_video_amd.ltx_model import LTXModel
    with pytest.raises(ValueError, match="fp8_activations"):
        LTXModel(small["mc"], small["Wdev"], fp8_activations=True)
    assert _model(small).fp8_activations is False and _model(small, fp8_activations=True).fp8_activations is True


def test_eager_equals_graph_replay(dev, small):
    m, mod = _model(small, fp8_activations=True), small["mod"]
    v = m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"]).clone()       # (also the warm-up a capture needs)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        vg = m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"])
    gr.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v.float()).all())
    assert torch.equal(v.view(torch.int16), vg.view(torch.int16))


def test_w8a8_launches_and_context_quantised_once(dev, small, monkeypatch):
    from mlx_video_amd import ops
    m, mod = _model(small, fp8_activations=True), small["mod"]
    rows = []
    real = ops.quant_rows_fp8
    monkeypatch.setattr(ops, "quant_rows_fp8", lambda a, out=None: (rows.append(a.shape[0]), real(a, out=out))[1])
    ops.TIMER = ops.KernelTimer()
    try:
        m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"])
        torch.cuda.synchronize()
        fams = [r[0] for r in ops.TIMER.records]
    finally:
        ops.TIMER = None
    L, M, MS = 2, small["B"] * small["N"], small["B"] * small["S"]
    assert M != MS
    assert rows.count(MS) == 1, f"the text context was quantised {rows.count(MS)} times in one forward"
    assert rows.count(M) == 6 * L            # nx (q|k|v), att, nx (q2), att, nx (FF1), hff per block
    assert fams.count("gemm_w8a8") == 7 * L and fams.count("quant_rows_fp8") == 6 * L + 1
    assert "gemm_w8" in fams                 # patchify, the timestep / AdaLN GEMMs, the caption projection and the head stay W8A16
    # hoisted context: prepare_context quantises it once too, and the forward then not at all
    rows.clear()
    kv = m.prepare_context(mod.context)
    assert rows.count(MS) == 1
    rows.clear()
    m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"], ctx_kv=kv)
    torch.cuda.synchronize()
    assert rows.count(MS) == 0 and rows.count(M) == 6 * L


def test_batch_invariant_rows(dev, small):
    from mlx_video_amd.ltx_model import TimestepPlan
    m, mod = _model(small, fp8_activations=True), small["mod"]
    m.batch_invariant = True
    both = m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"]).clone()
    for b in range(small["B"]):
        one = m.forward_tokens(mod.latent[b:b + 1].contiguous(), TimestepPlan.from_timesteps(mod.timesteps[b:b + 1]),
                               mod.context[b:b + 1].contiguous(), small["pe"])
        torch.cuda.synchronize()
        assert torch.equal(one[0].view(torch.int16), both[b].view(torch.int16)), f"row {b} depends on the batch"


def test_stg_forward_runs(dev, small):
    from mlx_video_amd.guidance import BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType
    m, mod = _model(small, fp8_activations=True), small["mod"]
    p = PerturbationConfig([Perturbation(PerturbationType.SKIP_VIDEO_SELF_ATTN, [1])])
    pert = BatchedPerturbationConfig([PerturbationConfig.empty(), p])
    plain = m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"]).clone()
    v = m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"], perturbations=pert)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v.float()).all())
    assert torch.equal(v[0].view(torch.int16), plain[0].view(torch.int16)) and not torch.equal(v[1], plain[1])


def test_accuracy_against_w8a16(dev, small):
    from mlx_video_amd.ltx_model import LTXModel
    mod = small["mod"]

    def fwd(m):
        v = m.forward_tokens(mod.latent, small["plan"], mod.context, small["pe"]).clone()
        torch.cuda.synchronize()
        return v

    ref = fwd(LTXModel(small["mc"], small["Wdev"]))
    d8 = parity.rel_l2(fwd(_model(small)), ref)
    dA = parity.rel_l2(fwd(_model(small, fp8_activations=True)), ref)
    print(f"small forward vs bf16: W8A16 d8 = {d8:.3e}, W8A8 dA = {dA:.3e}, dA / d8 = {dA / d8:.3f}")
    name = "test_fp8_act_model_gpu::test_accuracy_against_w8a16"
    parity.LEDGER[name + "#d8"] = {"measured": d8, "note": "rel-L2 W8A16 forward vs bf16 forward (small config)"}
    parity.LEDGER[name + "#ratio"] = {"measured": dA / d8, "note": "dA / d8; predicted sqrt(2), asserted <= 2"}
    parity.check(name + "#dA", dA, 2.0 * d8, note="rel-L2 W8A8 forward vs bf16 forward; bound 2 x d8 measured in the same run")


def test_distilled_pipeline_with_fp8_activations(dev):
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
                                prompt_embeds=emb, device=dev, seed=3, enable_fp8=True, fp8_activations=True)
        fams = {r[0] for r in ops.TIMER.records}
    finally:
        ops.TIMER = None
    assert frames.shape == (9, 128, 128, 3) and frames.dtype == np.uint8
    assert 5 < frames.mean() < 250
    assert "gemm_w8a8" in fams and "quant_rows_fp8" in fams
