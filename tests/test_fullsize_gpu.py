"""Parity at BASELINE.json's full sizes (512x512x33: N=1280 tokens, B=2 CFG pair, D=4096, FF=16384; VAE
latent 5x16x16 -> 33x512x512) through size-independent properties, plus one full-width block against
the oracle.  Properties: sub-problem consistency (a tile-aligned slice of the full problem reproduces
the full result bit for bit), permutation equivariance, softmax normalisation, causality of the causal
VAE, tiling == no tiling where one tile covers the volume, round trips of the index maps."""
import math

import parity
import pytest
import torch

from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_gemm_fullsize_properties(dev):
    from mlx_video_amd import ops
    g = torch.Generator(device=dev).manual_seed(0)
    M, N, K = 2560, 16384, 4096
    a = torch.randn((M, K), generator=g, device=dev).to(BF)
    w = (torch.randn((N, K), generator=g, device=dev) * 0.02).to(BF)
    b = (torch.randn((N,), generator=g, device=dev) * 0.01).to(BF)
    full = ops.gemm(a, w, b, epilogue=ops.EPI_BIAS_GELU)
    # (i) row-slice consistency: rows 320..479 (one 160-row tile) computed alone are bit-identical
    part = ops.gemm(a[320:480].contiguous(), w, b, epilogue=ops.EPI_BIAS_GELU)
    assert torch.equal(part, full[320:480])
    # (ii) row permutation equivariance, bit exact
    perm = torch.randperm(M, generator=g, device=dev)
    assert torch.equal(ops.gemm(a[perm].contiguous(), w, b, epilogue=ops.EPI_BIAS_GELU), full[perm])
    # (iii) identity weights: x @ I^T + 0 == x exactly (K=N=4096)
    eye = torch.eye(K, device=dev, dtype=BF)
    assert torch.equal(ops.gemm(a, eye, None), a)
    # (iv) against an independent fp32 product on a random sample of outputs
    cols = torch.randint(0, N, (64,), generator=g, device=dev)
    y = a.float() @ w[cols].float().t() + b[cols].float()
    ref = O.gelu_tanh(y.to(BF).float().cpu(), O.BF16)
    parity.auto(rel_l2(full[:, cols].float().cpu(), ref), 3e-3)


def test_attention_fullsize_properties(dev):
    from mlx_video_amd import ops
    B, H, N, D = 2, 32, 1280, 4096
    g = torch.Generator(device=dev).manual_seed(1)
    q = torch.randn((B * N, D), generator=g, device=dev).to(BF)
    k = torch.randn((B * N, D), generator=g, device=dev).to(BF)
    v = torch.randn((B, N, D), generator=g, device=dev).to(BF)
    vt = v.transpose(1, 2).contiguous()
    out = torch.empty((B * N, D), dtype=BF, device=dev)
    sc = 1.0 / math.sqrt(128)
    ops.flash_attn(q, k, vt, out, B, H, N, N, sc)
    # (i) softmax rows sum to one: V = 1 -> output 1 (within bf16 rounding of P)
    ones = torch.ones_like(vt)
    o1 = torch.empty_like(out)
    ops.flash_attn(q, k, ones, o1, B, H, N, N, sc)
    assert float((o1.float() - 1.0).abs().max()) < 8e-3
    # (ii) permuting the keys (K rows and V columns together) leaves the result unchanged up to fp order
    perm = torch.randperm(N, generator=g, device=dev)
    kp = k.reshape(B, N, D)[:, perm].reshape(B * N, D).contiguous()
    vtp = vt[:, :, perm].contiguous()
    o2 = torch.empty_like(out)
    ops.flash_attn(q, kp, vtp, o2, B, H, N, N, sc)
    parity.auto(rel_l2(o2.float(), out.float()), 6e-3)
    # (iii) independent fp32 attention for 2 heads
    for h in (0, 17):
        qh = q.reshape(B, N, H, 128)[:, :, h].float()
        kh = k.reshape(B, N, H, 128)[:, :, h].float()
        vh = v.reshape(B, N, H, 128)[:, :, h].float()
        ref = torch.softmax(qh @ kh.transpose(1, 2) * sc, -1) @ vh
        parity.auto(rel_l2(out.reshape(B, N, H, 128)[:, :, h].float(), ref), 1e-2)


def test_block_fullwidth_vs_oracle(dev):
    """One full-width DiT block (D=4096, 32 heads, FF 16384) on the bench shape B=2, N=1280, S=1024."""
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig, Modality
    cfg = O.DiTConfig(num_layers=1)
    W = O.make_weights(cfg, seed=12)
    model = LTXModel(LTXModelConfig(num_layers=1), {k: v.to(dev) for k, v in W.items()})
    B, F, Hh, Ww, S = 2, 5, 16, 16, 1024
    N = F * Hh * Ww
    g = torch.Generator().manual_seed(44)
    lat = torch.randn(1, N, 128, generator=g).to(BF).expand(B, N, 128).contiguous()
    ctx = torch.randn(B, S, 3840, generator=g).to(BF)
    ts = torch.full((B, N), 0.909375).to(BF)
    pos = torch.from_numpy(O.create_position_grid(1, F, Hh, Ww))
    pe = O.precompute_freqs_cis(pos, cfg.dim)
    ref = O.ltx_forward(lat.float(), ts.float(), ctx.float(), pe, W, cfg, O.BF16)
    v, _ = model(video=Modality(latent=lat.to(dev), timesteps=ts.to(dev), positions=pos.to(dev), context=ctx.to(dev)))
    torch.cuda.synchronize()
    assert v.shape == (B, N, 128)
    parity.auto(rel_l2(v.float().cpu(), ref), 1e-2)
    reff = O.ltx_forward(lat.float(), ts.float(), ctx.float(), pe, W, cfg, O.BF16_FLASH)
    parity.auto(rel_l2(v.float().cpu(), reff), 5e-3, tag="vs_flash_policy")
    assert not torch.equal(v[0], v[1])           # the two CFG branches see different contexts


def test_vae_fullsize_properties(dev):
    from mlx_video_amd import ops
    from mlx_video_amd.video_vae import LTX2VideoDecoder, TilingConfig, random_decoder_weights, to_uint8_frames
    dec = LTX2VideoDecoder(random_decoder_weights(dev, layers=1), num_layers_per_block=1)
    g = torch.Generator(device=dev).manual_seed(3)
    lat = torch.randn((1, 128, 5, 16, 16), generator=g, device=dev).to(BF)
    full = dec(lat, causal=True)
    assert full.shape == (1, 3, 33, 512, 512) and bool(torch.isfinite(full.float()).all())
    # (i) causality: with causal convolutions the first 1+8(k-1) frames depend on the first k latent frames only
    # (the small-volume stages use split-K whose slice count depends on the voxel count, so the two runs sum
    # their fp32 partials in different groupings: equal to accumulation order, not bit for bit)
    pre = dec(lat[:, :, :3].contiguous(), causal=True)
    parity.auto(rel_l2(pre.float(), full[:, :, :17].float()), 1.5e-2)
    # a change in a LATER latent frame must not move the earlier frames at all
    lat_b = lat.clone()
    lat_b[:, :, 4] += 1.0
    assert torch.equal(dec(lat_b, causal=True)[:, :, :25], full[:, :, :25])
    # (ii) one tile covering everything == plain decode; a real spatial tiling stays close away from seams
    nc = dec(lat)
    assert torch.equal(dec.decode_tiled(lat, TilingConfig.spatial_only(512, 64)), nc)
    tiled = dec.decode_tiled(lat, TilingConfig.spatial_only(256, 64))
    assert tiled.shape == nc.shape and bool(torch.isfinite(tiled.float()).all())
    # (iii) batch consistency: decoding two latents together == separately, equal up to split-K grouping (the small-volume
    # stages' slice count depends on B x voxels), each row checked on its own
    lat2 = torch.cat([lat, lat.flip(2)], 0)
    both = dec(lat2)
    parity.auto(rel_l2(both[1].float(), dec(lat.flip(2))[0].float()), 1.5e-2)
    parity.auto(rel_l2(both[0].float(), nc[0].float()), 1.5e-2, tag="batch_row0")
    assert torch.equal(dec(lat2), both)                      # same geometry twice: deterministic (slab split-K, no atomics)
    # (iv) uint8 conversion: monotone, range, layout
    u8 = to_uint8_frames(nc)
    assert u8.shape == (1, 33, 512, 512, 3) and u8.dtype == torch.uint8
    x = nc[0, 1, 7].float()
    assert torch.equal(u8[0, 7, :, :, 1], ((x + 1) / 2).clamp(0, 1).to(BF).float().mul(255).to(BF).to(torch.uint8))
    # (v) patchify/unpatchify round trip at 33x512x512, bit exact
    pt = ops.patchify_cl(nc, 4, 64)
    assert pt.shape == (1, 33, 128, 128, 64)
    back = ops.unpatchify_cf(pt[..., :48].contiguous(), 3, 4)
    torch.cuda.synchronize()
    assert torch.equal(back, nc)


def test_denoise_fullsize_smoke(dev):
    """Two full-shape CFG steps with a 2-block full-width model: finite, deterministic, cfg_batch == two passes."""
    from mlx_video_amd.denoise import denoise_dev
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    from mlx_video_amd.schedulers import create_position_grid, ltx2_scheduler
    model = LTXModel.random_init(LTXModelConfig(num_layers=2), dev, seed=5)
    g = torch.Generator(device=dev).manual_seed(6)
    lat = torch.randn((1, 128, 5, 16, 16), generator=g, device=dev).to(BF)
    cp = torch.randn((1, 1024, 3840), generator=g, device=dev).to(BF)
    cn = torch.randn((1, 1024, 3840), generator=g, device=dev).to(BF)
    sig = ltx2_scheduler(40, 1280)[:3]
    pos = create_position_grid(1, 5, 16, 16).to(dev)
    a = denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=True)
    b = denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=False)
    c = denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a.float()).all())
    assert torch.equal(a, c)                      # deterministic
    # B=2 puts 128 of the 640 attention tiles in a short round whose workgroups split the keys (attention.hip):
    # those rows sum in a different order than in the B=1 launches, so the pair is close, not identical ...
    parity.auto(rel_l2(a, b), 2e-3)
    # ... and with the split off (LTXK_ATTN_NO_TAIL_SPLIT), batching the CFG pair does not change a single bit
    model.attn_tail_split = False
    a0 = denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=True)
    b0 = denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=False)
    torch.cuda.synchronize()
    assert torch.equal(a0, b0)


@pytest.mark.parametrize("tc", [False, True])
def test_vae_decode_with_fused_pixelnorm(dev, tc):
    """``fuse_act`` (PixelNorm + modulation + SiLU carried by the conv epilogues of the 256 / 128-channel stages,
    off by default because it measured slower) decodes the same 33x512x512 video up to the association order of the
    row statistic; also with timestep conditioning (per-batch modulation inside the fused epilogue)."""
    from mlx_video_amd.video_vae import LTX2VideoDecoder, random_decoder_weights
    if tc:
        from oracle import vae as OV
        W = {k: v.to(dev) for k, v in OV.make_decoder_weights(seed=8, timestep_conditioning=True, layers_per_block=2).items()}
    else:
        W = random_decoder_weights(dev, layers=2)
    dec = LTX2VideoDecoder(W, num_layers_per_block=2, timestep_conditioning=tc)
    g = torch.Generator(device=dev).manual_seed(4)
    lat = torch.randn((1, 128, 5, 16, 16), generator=g, device=dev).to(BF)
    noise = torch.randn((1, 128, 5, 16, 16), generator=g, device=dev).to(BF) if tc else None
    a = dec(lat, noise=noise)
    dec.fuse_act = True
    b = dec(lat, noise=noise)
    torch.cuda.synchronize()
    assert a.shape == b.shape == (1, 3, 33, 512, 512)
    parity.auto(rel_l2(b.float(), a.float()), 5e-3)
