"""Video-VAE parity: HIP kernels through the C ABI vs the CPU oracle (oracle/vae.py, bf16-storage
policy) on seeded inputs.  Index maps (patchify/unpatchify/d2s/s2d, uint8 layout) are bit-exact;
convolutions differ only by fp32 accumulation order (<= 1 bf16 ulp on a small fraction); full
decode/encode: stated tolerance rel-L2 <= 2e-2 (40+ bf16 layers)."""
import parity
import math

import pytest
import torch

from oracle import dit as O
from oracle import vae as OV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def cl(x):   # (B,C,D,H,W) -> channels-last (B,D,H,W,C)
    return x.permute(0, 2, 3, 4, 1).contiguous()


def cf(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


@pytest.mark.parametrize("cin,cout,causal,reflect,shape", [
    (128, 128, False, True, (1, 3, 5, 6)), (128, 128, True, False, (2, 2, 4, 4)), (64, 256, True, False, (1, 4, 6, 5)),
    (256, 48, False, True, (1, 2, 8, 8)), (1024, 1024, False, True, (1, 2, 4, 4)), (128, 1024, False, True, (1, 1, 2, 2)),
    (512, 128, True, True, (1, 5, 3, 7))])
def test_conv3d(dev, cin, cout, causal, reflect, shape):
    from mlx_video_amd import ops
    b, d, h, w = shape
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(b, cin, d, h, w, generator=g).to(BF)
    wt = (torch.randn(cout, 3, 3, 3, cin, generator=g) / (27 * cin) ** 0.5).to(BF)
    bias = (torch.randn(cout, generator=g) * 0.1).to(BF)
    res = torch.randn(b, cout, d, h, w, generator=g).to(BF)
    ref = OV.causal_conv3d(x.float(), wt, bias, O.BF16, causal, reflect)
    out = ops.conv3d(cl(x).to(dev), wt.to(dev), bias.to(dev), causal, ops.PAD_REFLECT if reflect else ops.PAD_ZEROS)
    out_r = ops.conv3d(cl(x).to(dev), wt.to(dev), bias.to(dev), causal, ops.PAD_REFLECT if reflect else ops.PAD_ZEROS,
                     resid=cl(res).to(dev))
    torch.cuda.synchronize()
    parity.auto(rel_l2(cf(out), ref), 3e-3)
    parity.auto(rel_l2(cf(out_r), O.BF16.r(ref + res.float())), 3e-3)


@pytest.mark.parametrize("C", [64, 128, 256, 512, 1024, 2048])      # 64: eight lanes per row, two rows per DPP row (common.h group_sum)
@pytest.mark.parametrize("mod", [False, True])
def test_pixelnorm_act(dev, C, mod):
    from mlx_video_amd import ops
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(2, C, 2, 3, 5, generator=g) * 2).to(BF)
    p = O.BF16
    ref = OV.pixel_norm(x.float(), p, 1e-8)
    sc = sh = None
    if mod:
        sc = torch.randn(2, C, generator=g).to(BF)
        sh = torch.randn(2, C, generator=g).to(BF)
        ref = OV._mod(ref, sc.float().reshape(2, C, 1, 1, 1), sh.float().reshape(2, C, 1, 1, 1), p)
    ref = O.silu(ref, p)
    out = ops.pixelnorm_act(cl(x).to(dev), 1e-8, True, sc.to(dev) if mod else None, sh.to(dev) if mod else None)
    torch.cuda.synchronize()
    parity.auto(rel_l2(cf(out), ref), 3e-3)


@pytest.mark.parametrize("C,res,mod,keep", [(128, False, False, False), (128, True, True, True), (256, True, False, True), (256, False, True, False)])
def test_conv3d_fused_pixelnorm_act(dev, C, res, mod, keep):
    """The PixelNorm (+ modulation) + SiLU carried by the conv epilogue (decoder.py:136-180) equals the conv followed by
    ltxk_pixelnorm_act (same rounding points; only the association of the 128/256-term mean of squares differs, so a rare
    element moves by one bf16 step), and equals the oracle's conv -> pixel_norm -> silu chain.  Ragged volume (rows past M
    in the last tile), two batch rows with different modulation."""
    from mlx_video_amd import ops
    from mlx_video_amd import video_vae as V
    g = torch.Generator().manual_seed(C + res)
    # more than 128 tiles, so that the un-fused reference launch is not split along K either (split-K sums in another order)
    B, D, H, W = (2, 5, 64, 55) if C == 128 else (2, 3, 63, 56)
    assert V.conv_act_fusable(C, B * D * H * W, force=True)
    x = torch.randn(B, C, D, H, W, generator=g).to(BF)
    w = (torch.randn(C, 3, 3, 3, C, generator=g) / math.sqrt(27 * C)).to(BF)
    b = (torch.randn(C, generator=g) * 0.1).to(BF)
    r = torch.randn(B, C, D, H, W, generator=g).to(BF) if res else None
    sc = torch.randn(B, C, generator=g).to(BF) if mod else None
    sh = torch.randn(B, C, generator=g).to(BF) if mod else None
    dv = lambda t: None if t is None else t.to(dev)
    act = dict(eps=1e-8, silu=True, scale=dv(sc), shift=dv(sh))
    y_sep = ops.conv3d(cl(x).to(dev), w.to(dev), b.to(dev), False, ops.PAD_REFLECT, resid=dv(cl(r)) if res else None)
    a_sep = ops.pixelnorm_act(y_sep, 1e-8, True, dv(sc), dv(sh))
    y_f, a_f = ops.conv3d(cl(x).to(dev), w.to(dev), b.to(dev), False, ops.PAD_REFLECT, resid=dv(cl(r)) if res else None, act=act, keep_out=keep)
    torch.cuda.synchronize()
    assert (y_f is None) == (not keep)
    if keep:
        assert torch.equal(y_f, y_sep)
    mism = float((a_f != a_sep).float().mean())
    assert mism < 2e-3, f"fused and separate PixelNorm outputs differ in {mism:.2%} of elements"
    assert float((a_f.float() - a_sep.float()).abs().max()) <= 0.0625
    p = O.BF16
    ref = OV.causal_conv3d(x.float(), w.float(), b.float(), p, False, True)
    if res:
        ref = p.r(ref + r.float())
    ref = OV.pixel_norm(ref, p, 1e-8)
    if mod:
        ref = OV._mod(ref, sc.float().reshape(B, C, 1, 1, 1), sh.float().reshape(B, C, 1, 1, 1), p)
    ref = O.silu(ref, p)
    parity.auto(rel_l2(cf(a_f), ref), 6e-3)


def test_d2s_add_exact(dev):
    from mlx_video_amd import ops
    g = torch.Generator().manual_seed(1)
    B, Ci, D, H, W = 1, 64, 3, 2, 3
    Co = Ci // 2
    x = torch.randn(B, Ci, D, H, W, generator=g).to(BF)
    cv = torch.randn(B, Co * 8, D, H, W, generator=g).to(BF)
    ref = O.BF16.r(OV.depth_to_space(cv.float(), 2, 2, 2)[:, :, 1:] +
                   OV.depth_to_space(x.float(), 2, 2, 2).repeat(1, 4, 1, 1, 1)[:, :, 1:])
    out = ops.d2s_add(cl(cv).to(dev), cl(x).to(dev))
    torch.cuda.synchronize()
    assert out.shape == (B, 2 * D - 1, 2 * H, 2 * W, Co)
    assert torch.equal(cf(out).float().cpu(), ref)


def test_patchify_unpatchify_uint8_exact(dev):
    from mlx_video_amd import ops
    from mlx_video_amd import video_vae as V
    g = torch.Generator().manual_seed(2)
    vid = (torch.rand(1, 3, 2, 8, 12, generator=g) * 2.4 - 1.2).to(BF)
    ref_p = OV.patchify(vid.float(), 4)                                  # (1,48,2,2,3)
    out = ops.patchify_cl(vid.to(dev), 4, 64)
    assert out.shape == (1, 2, 2, 3, 64)
    back = ops.unpatchify_cf(out[..., :48].contiguous(), 3, 4)
    assert back.shape == (1, 3, 2, 8, 12)
    u8 = V.to_uint8_frames(vid.to(dev))
    assert torch.equal(u8, ops.to_uint8(vid.to(dev)))
    torch.cuda.synchronize()
    assert torch.equal(cf(out[..., :48]).float().cpu(), ref_p) and float(out[..., 48:].abs().max()) == 0.0
    assert torch.equal(back.cpu(), vid)                                   # unpatchify(patchify(x)) == x
    assert torch.equal(OV.unpatchify(ref_p, 4), vid.float())
    assert torch.equal(u8[0].cpu(), OV.to_uint8(vid[0].float(), O.BF16))


@pytest.mark.parametrize("stride,cx,cc", [((1, 2, 2), 128, 64), ((2, 1, 1), 64, 64), ((2, 2, 2), 64, 16)])
def test_s2d_skip(dev, stride, cx, cc):
    from mlx_video_amd import ops
    st_, sh, sw = stride
    g = torch.Generator().manual_seed(3)
    B, Dp, Hp, Wp = 1, 4, 4, 6
    x = torch.randn(B, cx, Dp, Hp, Wp, generator=g).to(BF)
    cv = torch.randn(B, cc, Dp, Hp, Wp, generator=g).to(BF)
    mult = st_ * sh * sw
    co = cc * mult
    xin = OV.space_to_depth(x.float(), st_, sh, sw)
    gsz = xin.shape[1] // co
    xin = O.BF16.r(xin.reshape(B, co, gsz, *xin.shape[2:]).mean(dim=2))
    ref = O.BF16.r(OV.space_to_depth(cv.float(), st_, sh, sw) + xin)
    out = ops.s2d_skip(cl(cv).to(dev), cl(x).to(dev), stride)
    torch.cuda.synchronize()
    assert out.shape == (B, Dp // st_, Hp // sh, Wp // sw, co)
    parity.auto(rel_l2(cf(out), ref), 2e-3)


@pytest.mark.parametrize("causal", [False, True])
def test_decode_small(dev, causal):
    from mlx_video_amd.video_vae import LTX2VideoDecoder
    W = OV.make_decoder_weights(seed=21, layers_per_block=2)
    dec = LTX2VideoDecoder({k: v.to(dev) for k, v in W.items()}, num_layers_per_block=2)
    g = torch.Generator().manual_seed(4)
    lat = torch.randn(1, 128, 2, 3, 4, generator=g).to(BF)
    ref = OV.vae_decode(lat.float(), W, O.BF16, causal=causal, layers_per_block=2)
    out = dec(lat.to(dev), causal=causal)
    torch.cuda.synchronize()
    assert out.shape == (1, 3, 9, 96, 128) and ref.shape == out.shape
    parity.auto(rel_l2(out, ref), 2e-2)
    parity.auto(rel_l2(out, OV.vae_decode(lat.float(), W, O.F32, causal=causal, layers_per_block=2)), 5e-2)
    # test_vae_streaming.py:18-54: chunked_conv (an MLX memory workaround) must give the regular result; here it is
    # accepted and is the same launch sequence, so the outputs are bit-identical (7 latent frames: d > 4 is where
    # the reference's chunking would activate)
    lat7 = torch.randn(1, 128, 7, 2, 2, generator=g).to(BF).to(dev)
    assert torch.equal(dec(lat7, causal=causal, chunked_conv=True), dec(lat7, causal=causal, chunked_conv=False))


def test_decode_timestep_conditioned(dev):
    from mlx_video_amd.video_vae import LTX2VideoDecoder
    W = OV.make_decoder_weights(seed=22, layers_per_block=1, timestep_conditioning=True)
    dec = LTX2VideoDecoder({k: v.to(dev) for k, v in W.items()}, timestep_conditioning=True, num_layers_per_block=1)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(1, 128, 1, 2, 2, generator=g).to(BF)
    noise = torch.randn(1, 128, 1, 2, 2, generator=g).to(BF)
    ref = OV.vae_decode(lat.float(), W, O.BF16, timestep=0.05, noise=noise.float(), layers_per_block=1)
    out = dec(lat.to(dev), noise=noise.to(dev))
    torch.cuda.synchronize()
    parity.auto(rel_l2(out, ref), 2e-2)
    with pytest.raises(ValueError, match="noise"):
        dec(lat.to(dev))


def test_decode_tiled_matches_oracle_tiling(dev):
    from mlx_video_amd.video_vae import LTX2VideoDecoder, TilingConfig
    W = OV.make_decoder_weights(seed=23, layers_per_block=1)
    dec = LTX2VideoDecoder({k: v.to(dev) for k, v in W.items()}, num_layers_per_block=1)
    g = torch.Generator().manual_seed(6)
    lat = torch.randn(1, 128, 4, 3, 4, generator=g).to(BF)
    emitted = []
    out = dec.decode_tiled(lat.to(dev), TilingConfig(spatial_config=TilingConfig.spatial_only(64, 32).spatial_config,
                                                     temporal_config=TilingConfig.temporal_only(16, 8).temporal_config),
                           on_frames_ready=lambda fr, i: emitted.append((i, fr.shape[2])))
    torch.cuda.synchronize()
    ref = OV.decode_with_tiling(lambda z: OV.vae_decode(z.float(), W, O.BF16, layers_per_block=1), lat, 64, 32, 16, 8, O.BF16)
    assert out.shape == (1, 3, 25, 96, 128)
    parity.auto(rel_l2(out, ref), 2e-2)
    cov = set()
    for i, n in emitted:
        cov |= set(range(i, i + n))
    assert cov == set(range(25))                      # every frame emitted exactly once overall


def test_encode_small(dev):
    from mlx_video_amd.video_vae import VideoEncoder
    blocks = [("res_x", 1), ("compress_space_res", (1, 2, 2)), ("res_x", 1), ("compress_time_res", (2, 1, 1)),
              ("res_x", 1), ("compress_all_res", (2, 2, 2)), ("res_x", 1), ("compress_all_res", (2, 2, 2)), ("res_x", 1)]
    W = OV.make_encoder_weights(seed=24, blocks=blocks)
    enc = VideoEncoder({k: v.to(dev) for k, v in W.items()}, encoder_blocks=blocks)
    g = torch.Generator().manual_seed(7)
    vid = (torch.rand(1, 3, 9, 64, 96, generator=g) * 2 - 1).to(BF)
    ref = OV.vae_encode(vid.float(), W, O.BF16, blocks)
    out = enc(vid.to(dev))
    torch.cuda.synchronize()
    assert out.shape == (1, 128, 2, 2, 3) and ref.shape == out.shape
    parity.auto(rel_l2(out, ref), 2e-2)
    with pytest.raises(ValueError, match="1 \\+ 8"):
        enc(vid[:, :, :8].to(dev))


def test_latent_upsampler(dev):
    from mlx_video_amd.upsampler import LatentUpsampler, upsample_latents
    W = OV.make_upsampler_weights(mid=128, nb=2)
    up = LatentUpsampler({k: v.to(dev) for k, v in W.items()}, num_blocks_per_stage=2)
    g = torch.Generator().manual_seed(8)
    lat = torch.randn(1, 128, 3, 4, 5, generator=g).to(BF)
    mean = (torch.randn(128, generator=g) * 0.1).to(BF)
    std = (1 + 0.1 * torch.randn(128, generator=g)).abs().to(BF)
    ref = OV.upsample_latents(lat.float(), W, mean, std, O.BF16, nb=2)
    out = upsample_latents(lat.to(dev), up, mean.to(dev), std.to(dev))
    torch.cuda.synchronize()
    assert out.shape == (1, 128, 3, 8, 10) and ref.shape == out.shape
    parity.auto(rel_l2(out, ref), 2e-2)


def test_upsample_latents_takes_float32_statistics(dev):
    """latent_mean / latent_std as float32 vectors whose values are bf16 values (the round trip bf16 -> float32 is exact)
    give the bits of the bf16 vectors: upsample_latents converts them instead of handing float32 memory to a bf16 kernel."""
    from mlx_video_amd.upsampler import LatentUpsampler, upsample_latents
    W = OV.make_upsampler_weights(mid=128, nb=2)
    up = LatentUpsampler({k: v.to(dev) for k, v in W.items()}, num_blocks_per_stage=2)
    g = torch.Generator().manual_seed(8)
    lat = torch.randn(1, 128, 3, 4, 5, generator=g).to(BF).to(dev)
    mean = (torch.randn(128, generator=g) * 0.1).to(BF).to(dev)
    std = (1 + 0.1 * torch.randn(128, generator=g)).abs().to(BF).to(dev)
    out = upsample_latents(lat, up, mean, std)
    out32 = upsample_latents(lat.float(), up, mean.float(), std.float())
    torch.cuda.synchronize()
    assert out.shape == (1, 128, 3, 8, 10) and out32.dtype == BF
    assert torch.equal(out, out32)


@pytest.mark.parametrize("s_ov,t_ov", [(0, 0), (32, 8)], ids=["overlap0", "overlap32_8"])
def test_decode_with_tiling_normalises_a_foreign_tile(dev, s_ov, t_ov):
    """decode_with_tiling takes any callable.  A stub decoder (a deterministic torch function of the tile latent) returns
    its tile once as contiguous bf16 and once with the same values as float32 through a permuted view: the blended
    outputs are equal bit for bit.  Latents (1,128,3,3,5) under the smallest tiles the validators accept, 64 px and 16
    frames = 2 latent cells, with no overlap and with the smallest non-zero one: 2 tiles along t and h, 3 or 4 along w,
    the odd extents leaving a ragged last tile on every axis."""
    from mlx_video_amd.video_vae import SpatialTilingConfig, TemporalTilingConfig, TilingConfig, decode_with_tiling
    lat = torch.randn((1, 128, 3, 3, 5), generator=torch.Generator().manual_seed(11)).to(BF).to(dev)
    shapes = []

    def stub(foreign):
        def decoder_fn(x, causal=False, timestep=None, debug=False, chunked_conv=False):
            f = x.shape[2]
            v = x[:, :3].float().repeat_interleave(8, dim=2)[:, :, 7:]             # 1 + 8(f-1) frames
            v = v.repeat_interleave(32, dim=3).repeat_interleave(32, dim=4)
            v = (v + torch.linspace(-1, 1, v.shape[4], device=x.device)).to(BF)    # position-dependent inside the tile
            assert v.shape[2] == 1 + 8 * (f - 1)
            shapes.append(tuple(x.shape[2:]))
            if not foreign:
                return v.contiguous()
            t = v.float().permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)
            assert t.dtype == torch.float32 and not t.is_contiguous() and torch.equal(t.to(BF), v)
            return t
        return decoder_fn

    tc = TilingConfig(SpatialTilingConfig(64, s_ov), TemporalTilingConfig(16, t_ov))
    own = decode_with_tiling(stub(False), lat, tc)
    n_tiles = len(shapes)
    foreign = decode_with_tiling(stub(True), lat, tc)
    torch.cuda.synchronize()
    assert n_tiles >= 2 * 2 * 3 and len(set(shapes)) > 1                         # several tiles on every axis, ragged ones among them
    assert own.shape == (1, 3, 17, 96, 160) and own.dtype == BF and bool(torch.isfinite(own.float()).all())
    assert torch.equal(own, foreign)


def test_lora_merge(dev):
    from mlx_video_amd.lora import LoraSpec, apply_lora_to_weights, merge_lora_pair
    # reference known answer (tests/test_lora.py:8-29): I + 0.5*(1_{4x2}.1_{2x4}) = I + 1 -- at GEMM-legal sizes
    n = 64
    w = torch.eye(n).to(BF)
    A, B = torch.ones(2, n).to(BF), torch.ones(n, 2).to(BF)
    out = merge_lora_pair(w.to(dev), A.to(dev), B.to(dev), 0.5)
    torch.cuda.synchronize()
    assert torch.equal(out.float().cpu(), torch.eye(n) + 1.0)
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(256, 128, generator=g) * 0.02).to(BF)
    A = (torch.randn(16, 128, generator=g) * 0.1).to(BF)
    B = (torch.randn(256, 16, generator=g) * 0.1).to(BF)
    sd = {"diffusion_model.transformer_blocks.0.attn1.to_out.0.lora_A.weight": A,
          "diffusion_model.transformer_blocks.0.attn1.to_out.0.lora_B.weight": B}
    Wd = {"transformer_blocks.0.attn1.to_out.weight": w.to(dev)}
    spec = LoraSpec(path="mem", strength=0.7)
    merged = apply_lora_to_weights(Wd, [spec], lora_states={"mem": sd})["transformer_blocks.0.attn1.to_out.weight"]
    torch.cuda.synchronize()
    ref = O.BF16.r(w.float() + O.BF16.r(0.7 * (B.float() @ A.float())))
    assert float((merged.float().cpu() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max())
    # a LoRA stored as F32 / F16 (lora.py:114 multiplies B @ A in fp32 from the STORED dtype): this implementation feeds the matrix
    # cores bf16 operands - the stated deviation of lora._pack_group, pinned here: the merge equals the reference formula
    # evaluated on the bf16-rounded factors, and stays within 3 bf16 ulps of the delta of the formula on the fp32 factors
    A32, B32 = torch.randn(16, 128, generator=g) * 0.1, torch.randn(256, 16, generator=g) * 0.1
    sd32 = {k: v for k, v in zip(sd, (A32, B32))}
    m32 = apply_lora_to_weights(Wd, [spec], lora_states={"mem": sd32})["transformer_blocks.0.attn1.to_out.weight"].float().cpu()
    torch.cuda.synchronize()
    ref_bf = O.BF16.r(w.float() + O.BF16.r(0.7 * (B32.to(BF).float() @ A32.to(BF).float())))
    assert float((m32 - ref_bf).abs().max()) <= 2.0 ** -8 * float(ref_bf.abs().max())
    delta32 = 0.7 * (B32 @ A32)
    assert float((m32 - (w.float() + delta32)).abs().max()) <= 3 * 2.0 ** -8 * float(delta32.abs().max()) + 2.0 ** -8 * float(w.float().abs().max())


def test_on_frames_ready_covers_89_frames(dev):
    """test_vae_streaming.py:159-197 as written there: a mock decoder, temporal_only(32, 8), 12 latent frames ->
    89 output frames, every frame index handed to the callback."""
    from mlx_video_amd.video_vae import TilingConfig, decode_with_tiling
    seen = set()
    calls = []

    def on_frames_ready(frames, start_idx):
        calls.append((start_idx, frames.shape[2]))
        for i in range(frames.shape[2]):
            seen.add(start_idx + i)

    g = torch.Generator(device=dev).manual_seed(3)

    def mock_decoder(x, causal=False, timestep=None, debug=False, chunked_conv=False):
        b, c, f, h, w = x.shape
        return torch.randn((b, 3, 1 + (f - 1) * 8, h * 32, w * 32), generator=g, device=dev).to(BF)

    lat = torch.zeros((1, 128, 12, 4, 4), dtype=BF, device=dev)
    out = decode_with_tiling(mock_decoder, lat, TilingConfig.temporal_only(tile_size=32, overlap=8), 32, 8,
                             on_frames_ready=on_frames_ready)
    torch.cuda.synchronize()
    assert out.shape == (1, 3, 89, 128, 128)
    assert seen == set(range(89)) and len(calls) >= 2          # streamed in more than one piece, nothing twice
    assert sum(n for _, n in calls) == 89


@pytest.mark.parametrize("cout,shape", [(128, (3, 160, 160)), (256, (3, 128, 128)), (512, (2, 112, 112))])
@pytest.mark.parametrize("res", [False, True])
def test_conv3d_short_last_round_as_half_tiles(dev, res, cout, shape, monkeypatch, ab_lib):
    """Convs whose tile count ends in a short round of 256 CUs - 128 channels on 3x160x160 voxels = 300 tiles of 256 rows,
    256 channels on 3x128x128 = 308 tiles of 160 rows, 512 channels on 2x112x112 = 157 x 2 tiles: the rows past the last
    whole round run as a second launch of lower tiles (conv3d.hip; LTXK_CONV_TAIL=0 in the A/B build switches it off).  Every output row is still one K-ordered
    sum: same bits as the single launch, with and without the residual."""
    from mlx_video_amd import ops
    g = torch.Generator(device=dev).manual_seed(3 + cout)
    x = torch.randn((1,) + shape + (128,), generator=g, device=dev).to(torch.bfloat16)
    w = (torch.randn((cout, 3, 3, 3, 128), generator=g, device=dev) * 0.02).to(torch.bfloat16)
    b = (torch.randn(cout, generator=g, device=dev) * 0.1).to(torch.bfloat16)
    r = torch.randn((1,) + shape + (cout,), generator=g, device=dev).to(torch.bfloat16) if res else None
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("LTXK_CONV_TAIL", mode)
        outs[mode] = ops.conv3d(x, w, b, True, 0, resid=r)
        torch.cuda.synchronize()
    assert torch.equal(outs["0"], outs["1"])
    assert float(outs["1"].float().abs().mean()) > 0.05


@pytest.mark.parametrize("shape,out", [((3, 5, 64, 96), (32, 48)), ((2, 2, 96, 144), (64, 96)), ((1, 3, 50, 70), (20, 33)),
                                       ((1, 1, 33, 40), (33, 40)), ((1, 2, 768, 768), (384, 384))])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_resize_area_vs_oracle(dev, shape, out, dt):
    """ltxk_resize_area (cv2.INTER_AREA on float frames, prepare_video_for_encoding utils.py:699-705) against the numpy
    restatement of OpenCV's area table (oracle/media.py): integer factors (closed form: the block mean), fractional factors
    (1.5x, 2.5x / 2.12x: parity unpinned beyond the restatement - cv2 is not installed), identity."""
    import numpy as np
    from oracle import media as OM
    from mlx_video_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(*shape, generator=g) * 2 - 1
    if dt == "bf16":
        x = x.to(torch.bfloat16)
    got = ops.resize_area(x.to(dev), *out)
    torch.cuda.synchronize()
    ref = torch.from_numpy(OM.resize_area(x.float().numpy(), *out)).to(torch.bfloat16)
    assert got.shape == ref.shape and got.dtype == torch.bfloat16
    d = (got.float().cpu() - ref.float()).abs()
    assert float((d > 0).float().mean()) < 2e-3 and float(d.max()) <= 2 ** -7          # fp32 order: rare single-ulp bf16 flips
    H, W = shape[-2:]
    if H % out[0] == 0 and W % out[1] == 0:           # known answer: the plain block mean
        fy, fx = H // out[0], W // out[1]
        mean = x.float().reshape(*shape[:-2], out[0], fy, out[1], fx).mean((-3, -1)).to(torch.bfloat16)
        dm = (got.float().cpu() - mean.float()).abs()
        assert float((dm > 0).float().mean()) < 2e-3 and float(dm.max()) <= 2 ** -7
    with pytest.raises(Exception, match="not a downscale"):
        ops.resize_area(x.to(dev), shape[-2] + 1, shape[-1])


KW_CASES = [  # (B, D, H, W, Cin, Cout, causal, pad_mode, residual); every case has > 128 tiles of 256 x 128, so the kw form runs
    (1, 3, 128, 128, 128, 128, 0, 1, True),      # the 128-channel stage: tiles = 2 image rows exactly
    (1, 4, 90, 100, 128, 128, 1, 1, False),      # W not a multiple of 16: runs start inside MFMA row blocks; ragged last tile
    (1, 5, 64, 64, 256, 256, 0, 1, True),        # the 256-channel stage: W = 64 (5 image rows per tile), two column tiles
    (2, 4, 66, 72, 64, 48, 1, 0, False),         # zero padding (encoder side), two batch items, Cout 48 (conv_out), Cin 64
    (1, 2, 96, 192, 128, 512, 2, 0, False),      # zero temporal halo (upsampler mode), 4 column tiles
    (1, 2, 260, 65, 128, 128, 0, 1, True),       # W = 65: odd width, two frames
    (1, 3, 100, 131, 192, 128, 2, 1, True),      # Cin = 192 (six 32-channel blocks), W = 131, zero temporal halo + reflect
    (1, 2, 60, 300, 128, 128, 0, 1, False),      # W = 300 > the 256-row tile: tiles start mid-row (left neighbour is a real voxel, not a halo)
    (1, 2, 70, 257, 64, 128, 1, 0, True),        # W = 257, zero padding: every tile boundary drifts by one voxel per image row
]


@pytest.mark.parametrize("case", KW_CASES)
def test_conv3d_kw_reuse_kernel_vs_per_tap_kernel(dev, case, monkeypatch):
    """conv3d_k3_kw_kernel (one A panel per (kd,kh) shared by the three kw taps) against the per-tap kernel (LTXK_CONV_KW=0
    in the A/B build): the same products and rounding points summed in another K order -> fp32-order differences only
    (rare single-ulp flips), on every halo mode, widths that do / do not align runs with MFMA blocks, ragged tiles, several
    column tiles, with and without the residual; the tail launch of half tiles gives the same bits as one launch."""
    from mlx_video_amd import _lib, ops
    B, D, H, W, Cin, Cout, causal, pad, res = case
    g = torch.Generator(device=dev).manual_seed(B * 7 + H + W + Cin + Cout)
    x = torch.randn((B, D, H, W, Cin), generator=g, device=dev).to(torch.bfloat16)
    w = (torch.randn((Cout, 3, 3, 3, Cin), generator=g, device=dev) * 0.02).to(torch.bfloat16)
    b = (torch.randn(Cout, generator=g, device=dev) * 0.1).to(torch.bfloat16)
    r = torch.randn((B, D, H, W, Cout), generator=g, device=dev).to(torch.bfloat16) if res else None
    with _lib.use_library(_lib.AB_LIB_PATH):
        outs = {}
        for name, env in (("per_tap", {"LTXK_CONV_KW": "0"}), ("kw", {"LTXK_CONV_KW": "2"}), ("kw_no_tail", {"LTXK_CONV_KW": "2", "LTXK_CONV_TAIL": "0"})):
            for k in ("LTXK_CONV_KW", "LTXK_CONV_TAIL"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            outs[name] = ops.conv3d(x, w, b, causal, pad, resid=r)
            torch.cuda.synchronize()
    assert torch.equal(outs["kw"], outs["kw_no_tail"])
    assert not torch.equal(outs["kw"], outs["per_tap"]) or Cin <= 64, "the kw form did not run (same bits as the per-tap kernel)"
    a, ref = outs["kw"].float(), outs["per_tap"].float()
    assert bool(torch.isfinite(a).all())
    parity.auto(rel_l2(a, ref), 3e-4)
    d = (a - ref).abs()
    assert float((d > 2.0 ** -7 * torch.maximum(a.abs(), ref.abs()).clamp_min(1e-3)).float().mean()) < 1e-3      # > 1 ulp apart: almost never
    # the product library takes the kw form where one column tile spans Cout, the per-tap form otherwise
    assert torch.equal(ops.conv3d(x, w, b, causal, pad, resid=r), outs["kw" if Cout <= 128 else "per_tap"])
