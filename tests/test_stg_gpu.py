"""Spatio-temporal guidance (STG) on the GPU: the value-passthrough kernel and the guided step tail bit for bit against
their restatements, the perturbed forward and a 3-step STG loop against the CPU oracle (ref_stg.py), batch invariance
of the B=3 [pos, neg, pos+] forward, and the denoise loop / pipeline plumbing."""
import numpy as np
import pytest
import torch

import parity
import ref_stg
from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN16 = torch.tensor(float("nan"), dtype=BF).view(torch.int16).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ passthrough kernel
@pytest.mark.parametrize("D", [128, 512, 4096])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 1280, 1296])
def test_value_passthrough_is_a_bit_exact_transpose(dev, T, D):
    from mlx_video_amd import ops
    B = 3
    ldvt = (T + 63) // 64 * 64 + 8            # padded beyond the 64-rounded length the model uses
    ldo = D + 8
    g = torch.Generator(device=dev).manual_seed(T * 7 + D)
    vt = torch.full((B, D, ldvt), float("nan"), dtype=BF, device=dev)
    vt[:, :, :T] = torch.randn((B, D, T), generator=g, device=dev).to(BF)
    vt_before = vt.clone()
    for mask in (0b100, 0b101, 0b010, 0b111):
        out = torch.full((B * T, ldo), float("nan"), dtype=BF, device=dev)
        ops.attn_value_passthrough(vt, out, B, T, mask)
        torch.cuda.synchronize()
        o = _bits(out).reshape(B, T, ldo)
        for b in range(B):
            if mask >> b & 1:
                assert torch.equal(o[b, :, :D], _bits(vt[b, :, :T].transpose(0, 1))), f"T={T} D={D} mask={mask:#b} row {b}"
                assert bool((o[b, :, D:] == NAN16).all()), "the ldo padding was written"
            else:
                assert bool((o[b] == NAN16).all()), f"T={T} D={D} mask={mask:#b}: unselected row {b} was written"
    assert torch.equal(_bits(vt), _bits(vt_before))


def test_value_passthrough_refuses_bad_arguments(dev):
    from mlx_video_amd import _lib, ops
    vt = torch.zeros((2, 128, 64), dtype=BF, device=dev)
    out = torch.zeros((128, 128), dtype=BF, device=dev)
    with pytest.raises(ValueError):
        ops.attn_value_passthrough(vt, out, 2, 65, 1)            # T > ldvt
    with pytest.raises(_lib.LtxkError):
        ops.attn_value_passthrough(torch.zeros((2, 96, 64), dtype=BF, device=dev), out, 2, 64, 1)    # D not a multiple of 128


# ----------------------------------------------------------------------------------------------------- guided tail
def _tail_ref(vp, vn, vq, x, clean, mask, cfg, stg, s, sn, bf16_euler):
    """float32 restatement of ltxk_guided_euler_step (tokens (B,S,C), latent (B,C,S))."""
    def r(t):
        return t.to(BF).float()
    p = vp.float().transpose(1, 2)
    v = p
    if vn is not None:
        v = r(v + r((cfg - 1.0) * r(v - vn.float().transpose(1, 2))))
    if vq is not None:
        v = r(v + r(stg * r(p - vq.float().transpose(1, 2))))
    xf = x.float()
    x0 = r(xf - s * v)
    if mask is not None:
        m = mask[:, None, :]
        x0 = r(r(x0 * m) + r(clean.float() * r(1.0 - m)))
    if bf16_euler:
        o = x0 + r(r(sn * r(xf - x0)) / s)
    elif sn > 0:
        o = x0 + (sn * (xf - x0)) / s
    else:
        o = x0
    return o.to(BF)


@pytest.mark.parametrize("s,sn", [(0.75, 0.5), (0.5, 0.0)])
@pytest.mark.parametrize("dev_sig", [False, True])
@pytest.mark.parametrize("bf16_euler", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("with_neg", [False, True])
def test_guided_tail_bits(dev, with_neg, masked, bf16_euler, dev_sig, s, sn):
    from mlx_video_amd import ops
    B, C, S = 2, 128, 200
    g = torch.Generator().manual_seed(3)
    vp, vn, vq = (torch.randn(B, S, C, generator=g).to(BF) for _ in range(3))
    x = torch.randn(B, C, S, generator=g).to(BF)
    clean = torch.randn(B, C, S, generator=g).to(BF) if masked else None
    mask = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (B, S), generator=g)] if masked else None
    cfg, stg = 4.0, 1.5
    d = dict(clean=clean.to(dev) if masked else None, mask_tok=mask.to(dev) if masked else None, bf16_euler=bf16_euler)
    sig = torch.tensor([s, sn], dtype=torch.float32, device=dev) if dev_sig else None
    vn_d = vn.to(dev) if with_neg else None
    out = ops.guided_euler_step(vp.to(dev), vn_d, vq.to(dev), x.to(dev), cfg, stg, s, sn, sigmas_dev=sig, **d)
    # v_pert = None is the CFG step tail, launch for launch
    plain = ops.guided_euler_step(vp.to(dev), vn_d, None, x.to(dev), cfg, stg, s, sn, sigmas_dev=sig, **d)
    today = ops.cfg_euler_step(vp.to(dev), vn_d, x.to(dev), cfg, s, sn, sigmas_dev=sig, **d)
    torch.cuda.synchronize()
    ref = _tail_ref(vp, vn if with_neg else None, vq, x, clean, mask, cfg, stg, s, sn, bf16_euler)
    assert torch.equal(_bits(out.cpu()), _bits(ref))
    assert torch.equal(_bits(plain), _bits(today))
    assert torch.equal(_bits(today.cpu()), _bits(_tail_ref(vp, vn if with_neg else None, None, x, clean, mask, cfg, stg, s, sn,
                                                          bf16_euler)))
    assert not torch.equal(out, today)


# --------------------------------------------------------------------------------------------- forward vs the oracle
def _small_model(cfg, W, dev):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    mc = LTXModelConfig(num_attention_heads=cfg.heads, num_layers=cfg.num_layers, caption_channels=cfg.caption_channels,
                        cross_attention_dim=cfg.dim)
    return LTXModel(mc, {k: v.to(dev) for k, v in W.items()})


def _stg_batch(n_rows, pert_rows, blocks):
    from mlx_video_amd.guidance import BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType
    p = PerturbationConfig([Perturbation(PerturbationType.SKIP_VIDEO_SELF_ATTN, blocks)])
    return BatchedPerturbationConfig([p if r in pert_rows else PerturbationConfig.empty() for r in range(n_rows)])


def test_perturbed_forward_matches_oracle(dev):
    from mlx_video_amd.ltx_model import Modality
    cfg = O.DiTConfig(num_layers=3, heads=4, caption_channels=256)
    L = cfg.num_layers
    W = O.make_weights(cfg, seed=61)
    model = _small_model(cfg, dict(W), dev)
    F, Hh, Ww, S = 2, 4, 4, 64
    N = F * Hh * Ww
    g = torch.Generator().manual_seed(62)
    lat1 = torch.randn(1, N, 128, generator=g).to(BF)
    cp, cn = (torch.randn(1, S, cfg.caption_channels, generator=g).to(BF) for _ in range(2))
    lat = lat1.repeat(3, 1, 1)
    ctx = torch.cat([cp, cn, cp], 0)
    ts = torch.full((3, N), 0.909375).to(BF)
    ts[:, : Hh * Ww] = 0.0
    pos = torch.from_numpy(O.create_position_grid(3, F, Hh, Ww))
    pe = O.precompute_freqs_cis(pos[:1], cfg.dim, heads=cfg.heads)
    blocks = [0, L - 1]
    ref_b = ref_stg.ltx_forward_stg(lat.float(), ts.float(), ctx.float(), pe, W, cfg, O.BF16, rows=[2], blocks=blocks)
    ref_f = ref_stg.ltx_forward_stg(lat.float(), ts.float(), ctx.float(), pe, W, cfg, O.F32, rows=[2], blocks=blocks)
    v, _ = model(video=Modality(latent=lat.to(dev), timesteps=ts.to(dev), positions=pos.to(dev), context=ctx.to(dev)),
                 perturbations=_stg_batch(3, [2], blocks))
    torch.cuda.synchronize()
    err = 0.0
    for r in range(3):
        err = max(err, parity.auto(parity.rel_l2(v[r], ref_b[r]), 1e-2, tag=f"bf16_row{r}"))
        parity.auto(parity.rel_l2(v[r], ref_f[r]), 3e-2, tag=f"f32_row{r}")
    # the skip took effect: the perturbed row is far from the unperturbed positive row
    assert parity.rel_l2(v[2], v[0]) >= 10 * err


# -------------------------------------------------------------------------------------------------- batch invariance
GEOM = {32: (2, 4, 4), 320: (5, 8, 8)}
S_CTX = 64


@pytest.fixture(scope="module")
def wide_model(dev):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    return LTXModel.random_init(LTXModelConfig(num_layers=2), dev, seed=23)


@pytest.mark.parametrize("blocks", [None, [1]])
@pytest.mark.parametrize("T", [32, 320])
def test_stg_rows_do_not_depend_on_the_batch(dev, wide_model, T, blocks):
    from mlx_video_amd.ltx_model import TimestepPlan, precompute_freqs_cis
    from mlx_video_amd.schedulers import create_position_grid
    model = wide_model
    g = torch.Generator(device=dev).manual_seed(200 + T)
    tok1 = torch.randn((1, T, 128), generator=g, device=dev).to(BF)
    cp, cn = (torch.randn((1, S_CTX, 3840), generator=g, device=dev).to(BF) for _ in range(2))
    pe = precompute_freqs_cis(create_position_grid(1, *GEOM[T]).to(dev), 4096)
    ts = torch.tensor([0.625], dtype=BF, device=dev)

    def plan(B):
        return TimestepPlan(ts, torch.zeros(B * T, dtype=torch.int32, device=dev))
    try:
        model.batch_invariant = True
        three = model.forward_tokens(tok1.repeat(3, 1, 1), plan(3), torch.cat([cp, cn, cp], 0), pe,
                                     perturbations=_stg_batch(3, [2], blocks))
        two = model.forward_tokens(tok1.repeat(2, 1, 1), plan(2), torch.cat([cp, cn], 0), pe)
        one = model.forward_tokens(tok1, plan(1), cp, pe, perturbations=_stg_batch(1, [0], blocks))
        plain = model.forward_tokens(tok1, plan(1), cp, pe)
        torch.cuda.synchronize()
    finally:
        model.batch_invariant = False
    assert bool(torch.isfinite(three.float()).all())
    assert torch.equal(three[:2], two), f"T={T} blocks={blocks}: the CFG rows of the B=3 forward differ from the B=2 forward"
    assert torch.equal(three[2], one[0]), f"T={T} blocks={blocks}: the perturbed row differs from the B=1 perturbed forward"
    assert not torch.equal(one, plain)


# ------------------------------------------------------------------------------------------------------ denoise loop
def _loop_inputs(dev, T=32, seed=9):
    from mlx_video_amd.schedulers import create_position_grid, ltx2_scheduler
    F, H, W = GEOM[T]
    g = torch.Generator(device=dev).manual_seed(seed)
    lat = torch.randn((1, 128, F, H, W), generator=g, device=dev).to(BF)
    cp = torch.randn((1, S_CTX, 3840), generator=g, device=dev).to(BF)
    cn = torch.randn((1, S_CTX, 3840), generator=g, device=dev).to(BF)
    return lat, create_position_grid(1, F, H, W).to(dev), cp, cn, ltx2_scheduler(30, T)[:4]


def test_stg_off_is_todays_loop(dev, wide_model):
    from mlx_video_amd.denoise import denoise_dev
    lat, pos, cp, cn, sig = _loop_inputs(dev)
    for kw in (dict(compile_step=True, cfg_batch=True, use_graph=True), dict(compile_step=False, cfg_batch=False)):
        a = denoise_dev(lat, pos, cp, cn, wide_model, sig, cfg_scale=4.0, **kw)
        b = denoise_dev(lat, pos, cp, cn, wide_model, sig, cfg_scale=4.0, stg_scale=0.0, stg_blocks=[1], stg_mode="stg_av", **kw)
        torch.cuda.synchronize()
        assert torch.equal(a, b)


@pytest.mark.parametrize("cfg_scale", [4.0, 1.0])
def test_stg_loop_forms_agree(dev, wide_model, cfg_scale):
    """STG on, batch-invariant mode: cfg_batch (one B=3 / B=2 forward) == separate forwards, and graph replay == eager."""
    from mlx_video_amd.denoise import denoise_dev
    lat, pos, cp, cn, sig = _loop_inputs(dev, seed=11)
    kw = dict(cfg_scale=cfg_scale, stg_scale=1.0, stg_blocks=[1], compile_step=True)
    try:
        wide_model.batch_invariant = True
        batched = denoise_dev(lat, pos, cp, cn, wide_model, sig, cfg_batch=True, **kw)
        separate = denoise_dev(lat, pos, cp, cn, wide_model, sig, cfg_batch=False, **kw)
        cache = {}
        graph = denoise_dev(lat, pos, cp, cn, wide_model, sig, cfg_batch=True, use_graph=True, graph_cache=cache, **kw)
        graph2 = denoise_dev(lat, pos, cp, cn, wide_model, sig, cfg_batch=True, use_graph=True, graph_cache=cache, **kw)
        off = denoise_dev(lat, pos, cp, cn, wide_model, sig, cfg_batch=True, use_graph=True, graph_cache=cache,
                          **dict(kw, stg_scale=0.0))
        torch.cuda.synchronize()
    finally:
        wide_model.batch_invariant = False
    assert bool(torch.isfinite(batched.float()).all())
    assert torch.equal(batched, separate), "cfg_batch changes the bits of an STG loop in batch-invariant mode"
    assert torch.equal(graph, batched) and torch.equal(graph2, batched), "graph replay differs from the eager STG loop"
    assert len(cache) == 2 and not torch.equal(off, batched)


@pytest.mark.parametrize("conditioned", [False, True])
def test_stg_loop_matches_oracle(dev, conditioned):
    from mlx_video_amd.conditioning import LatentState
    from mlx_video_amd.denoise import denoise_dev
    from mlx_video_amd.schedulers import create_position_grid, ltx2_scheduler
    cfg = O.DiTConfig(num_layers=2, heads=4, caption_channels=256)
    W = O.make_weights(cfg, seed=13)
    model = _small_model(cfg, dict(W), dev)
    B, F, Hh, Ww, S = 1, 2, 4, 4, 64
    N = F * Hh * Ww
    g = torch.Generator().manual_seed(44)
    lat = torch.randn(B, 128, F, Hh, Ww, generator=g).to(BF)
    cp = torch.randn(B, S, cfg.caption_channels, generator=g).to(BF)
    cn = torch.randn(B, S, cfg.caption_channels, generator=g).to(BF)
    sig = ltx2_scheduler(3, N)
    pos = create_position_grid(1, F, Hh, Ww)
    clean = mask = state = None
    if conditioned:
        clean = torch.randn(B, 128, F, Hh, Ww, generator=g).to(BF)
        mask = torch.ones(B, 1, F, 1, 1)
        mask[:, :, 0] = 0.0
        state = LatentState(lat.to(dev), clean.to(dev), mask.to(BF).to(dev))
    ref = ref_stg.denoise_dev_stg(lat.float(), pos.numpy(), cp.float(), cn.float(), W, cfg, sig.tolist(), O.BF16, 4.0, 1.0, [1],
                                  clean.float() if conditioned else None, mask)
    out = denoise_dev(lat.to(dev), pos.to(dev), cp.to(dev), cn.to(dev), model, sig, cfg_scale=4.0, state=state,
                      compile_step=True, cfg_batch=True, stg_scale=1.0, stg_blocks=[1])
    torch.cuda.synchronize()
    assert out.shape == lat.shape
    parity.auto(parity.rel_l2(out, ref), 2e-2)
    if conditioned:
        assert torch.equal(out[:, :, 0].cpu(), clean[:, :, 0])


# -------------------------------------------------------------------------------------------------------- pipeline
def _pipeline_mods(dev):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    from mlx_video_amd.upsampler import LatentUpsampler
    from mlx_video_amd.video_vae import LTX2VideoDecoder
    from oracle import vae as OV
    cfg = O.DiTConfig(num_layers=2, heads=4, caption_channels=256)
    W = O.make_weights(cfg, seed=31)
    mc = LTXModelConfig(num_attention_heads=4, num_layers=2, caption_channels=256, cross_attention_dim=cfg.dim)
    Wd = OV.make_decoder_weights(seed=32, layers_per_block=1)
    Wu = OV.make_upsampler_weights(mid=128, nb=1)
    return dict(transformer=LTXModel(mc, {k: v.to(dev) for k, v in W.items()}),
                vae_decoder=LTX2VideoDecoder({k: v.to(dev) for k, v in Wd.items()}, num_layers_per_block=1),
                upsampler=LatentUpsampler({k: v.to(dev) for k, v in Wu.items()}, num_blocks_per_stage=1))


def test_pipelines_run_with_stg(dev):
    from mlx_video_amd.generate import PipelineType, generate_video
    m = _pipeline_mods(dev)
    g = torch.Generator().manual_seed(52)
    pe_pos = torch.randn(1, 64, 256, generator=g).to(BF)
    pe_neg = torch.randn(1, 64, 256, generator=g).to(BF)
    kw = dict(prompt="x", height=128, width=128, num_frames=9, cfg_scale=4.0, prompt_embeds=pe_pos,
              negative_prompt_embeds=pe_neg, device=dev, seed=5, compile_step=True, cfg_batch=True, **m)
    off = generate_video(pipeline=PipelineType.DEV, num_inference_steps=2, **kw)
    on = generate_video(pipeline=PipelineType.DEV, num_inference_steps=2, stg_scale=1.0, stg_blocks=[1], **kw)
    assert on.shape == (9, 128, 128, 3) and on.dtype == np.uint8
    assert not np.array_equal(on, off)
    lat_off = generate_video(pipeline=PipelineType.DEV, num_inference_steps=2, return_latents=True, **kw)
    lat_on = generate_video(pipeline=PipelineType.DEV, num_inference_steps=2, return_latents=True, stg_scale=1.0, **kw)
    assert bool(torch.isfinite(lat_on.float()).all()) and not torch.equal(lat_on, lat_off)
    # the distilled pipeline's guided stage 2 (stage2_dev) runs STG too
    s2 = generate_video(pipeline=PipelineType.DISTILLED, stage1_steps=2, stage2_steps=1, stage2_dev=True, stg_scale=1.0,
                        stg_mode="stg_av", **kw)
    s2_off = generate_video(pipeline=PipelineType.DISTILLED, stage1_steps=2, stage2_steps=1, stage2_dev=True, **kw)
    assert s2.shape == (9, 128, 128, 3) and 0 < s2.mean() < 255
    assert not np.array_equal(s2, s2_off)
