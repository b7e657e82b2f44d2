"""Spatio-temporal guidance (STG) without a GPU: the CLI surface, argument errors, the perturbation configs against the
known answers of ltx_core/guidance/perturbations.py, the C-ABI binding of the new entry points, the velocity-space
guidance against the x0-space guiders in fp64, and the test-side restatement of the perturbed forward (ref_stg.py)."""
import ctypes
import types

import pytest
import torch

import ref_stg
from oracle import dit as O


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_parser_takes_the_stg_flags():
    from mlx_video_amd.generate import build_parser
    a = build_parser().parse_args([])
    assert a.stg_scale is None and a.stg_blocks is None and a.stg_mode is None      # the reference's defaults
    a = build_parser().parse_args(["--stg-scale", "1.5", "--stg-blocks", "3", "29", "--stg-mode", "stg_av"])
    assert a.stg_scale == 1.5 and a.stg_blocks == [3, 29] and a.stg_mode == "stg_av"
    assert build_parser().parse_args(["--stg-blocks"]).stg_blocks == []
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--stg-mode", "stg_a"])


def test_main_passes_the_stg_flags_through(monkeypatch):
    from mlx_video_amd import generate as G
    seen = {}
    monkeypatch.setattr(G, "generate_video", lambda **kw: seen.update(kw))
    G.main(["--pipeline", "dev", "--stg-scale", "1.0", "--stg-blocks", "29", "--stg-mode", "stg_v"])
    assert seen["stg_scale"] == 1.0 and seen["stg_blocks"] == [29] and seen["stg_mode"] == "stg_v"
    seen.clear()
    G.main(["--pipeline", "dev"])
    assert seen["stg_scale"] is None and seen["stg_blocks"] is None and seen["stg_mode"] is None


# ---------------------------------------------------------------------------------------------------------- errors
def _dummy_model(layers=4):
    return types.SimpleNamespace(config=types.SimpleNamespace(num_layers=layers))


@pytest.mark.parametrize("blocks,mode", [([], "stg_v"), ([4], "stg_v"), ([-1], "stg_v"), ([0, 7], "stg_av"), (None, "stg_x")])
def test_denoise_dev_refuses_bad_stg_arguments(blocks, mode):
    from mlx_video_amd.denoise import denoise_dev
    lat = torch.zeros(1, 128, 1, 2, 2, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        denoise_dev(lat, None, None, None, _dummy_model(4), [1.0, 0.5, 0.0], cfg_scale=4.0, stg_scale=1.0, stg_blocks=blocks,
                    stg_mode=mode)


@pytest.mark.parametrize("pipe,extra", [("distilled", {}), ("keyframe", {}), ("ic_lora", {"video_conditionings": [("v.mp4", 0, 1.0)]})])
def test_generate_video_refuses_stg_without_a_guided_stage(pipe, extra):
    from mlx_video_amd.generate import PipelineType, generate_video
    with pytest.raises(ValueError, match="STG"):
        generate_video(pipeline=PipelineType(pipe), stg_scale=1.0, **extra)


def test_generate_video_refuses_an_unknown_stg_mode():
    from mlx_video_amd.generate import PipelineType, generate_video
    with pytest.raises(ValueError, match="stg_mode"):
        generate_video(pipeline=PipelineType.DEV, stg_scale=1.0, stg_mode="stg_a")


# ------------------------------------------------------------------------------------------------------- guidance.py
def test_perturbation_configs_known_answers():
    from mlx_video_amd.guidance import (BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType,
                                        stg_perturbation)
    V, A = PerturbationType.SKIP_VIDEO_SELF_ATTN, PerturbationType.SKIP_AUDIO_SELF_ATTN
    every = Perturbation(V, None)
    some = Perturbation(V, [1, 3])
    assert every.is_perturbed(V, 0) and every.is_perturbed(V, 47) and not every.is_perturbed(A, 0)
    assert some.is_perturbed(V, 3) and not some.is_perturbed(V, 2)
    assert not PerturbationConfig(None).is_perturbed(V, 0) and not PerturbationConfig.empty().is_perturbed(V, 0)
    cfg = BatchedPerturbationConfig([PerturbationConfig.empty(), PerturbationConfig([some]), PerturbationConfig([every])])
    assert torch.equal(cfg.mask(V, 1), torch.tensor([1.0, 0.0, 0.0]))
    assert torch.equal(cfg.mask(V, 2), torch.tensor([1.0, 1.0, 0.0]))
    assert torch.equal(cfg.mask(A, 1), torch.ones(3))
    ml = cfg.mask_like(V, 3, torch.zeros(3, 5, 7, dtype=torch.bfloat16))
    assert ml.shape == (3, 1, 1) and ml.dtype == torch.bfloat16 and ml.flatten().tolist() == [1.0, 0.0, 0.0]
    assert cfg.any_in_batch(V, 2) and not cfg.all_in_batch(V, 2) and not cfg.any_in_batch(A, 0)
    assert BatchedPerturbationConfig([PerturbationConfig([every])] * 2).all_in_batch(V, 5)
    assert cfg.rows(V, 1) == [1, 2] and cfg.rows(V, 0) == [2]
    e = BatchedPerturbationConfig.empty(4)
    assert len(e.perturbations) == 4 and torch.equal(e.mask(V, 0), torch.ones(4))
    # the STG row of --stg-blocks / --stg-mode: None = every block; stg_av adds the (inert) audio type
    assert stg_perturbation(None, "stg_v", 48) == PerturbationConfig([every])
    assert stg_perturbation([29], "stg_av", 48).is_perturbed(V, 29) and not stg_perturbation([29], "stg_v", 48).is_perturbed(V, 28)
    assert stg_perturbation([29], "stg_av", 48).is_perturbed(A, 29)


# ------------------------------------------------------------------------------------------------------------- C ABI
def test_binding_declares_the_stg_entry_points():
    from mlx_video_amd import _lib
    assert "ltxk_guided_euler_step" in _lib.SIGNATURES and "ltxk_attn_value_passthrough" in _lib.SIGNATURES
    assert _lib.SIGNATURES["ltxk_attn_value_passthrough"][1][7] is ctypes.c_uint64
    lib = _lib.load()
    assert lib.ltxk_abi_sizeof(4) == ctypes.sizeof(_lib.StepArgs) and _lib.ABI_STRUCTS[4] is _lib.StepArgs
    assert lib.ltxk_abi_sizeof(5) == -1
    assert lib.ltxk_version() >= 402


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from mlx_video_amd import _lib, ops
    x = torch.zeros(1, 128, 4, dtype=torch.bfloat16)
    v = torch.zeros(1, 4, 128, dtype=torch.bfloat16)
    with pytest.raises(_lib.LtxkError):
        ops.guided_euler_step(v, None, v, x, 4.0, 1.0, 0.5, 0.25)
    with pytest.raises(_lib.LtxkError):
        ops.attn_value_passthrough(torch.zeros(1, 128, 64, dtype=torch.bfloat16), torch.zeros(64, 128, dtype=torch.bfloat16), 1, 64, 1)


# ----------------------------------------------------------------------------------------------- guidance algebra
def test_velocity_space_guidance_equals_x0_space_guiders_fp64():
    """x0 = x - sigma*v is affine in v with coefficients summing to one, so guiding velocities then taking x0 equals
    cond + CFGGuider.delta + STGGuider.delta on the three x0 predictions (guiders.py) in exact arithmetic."""
    from mlx_video_amd import components as C
    g = torch.Generator().manual_seed(5)
    x, vp, vn, vq = (torch.randn(2, 128, 3, 4, 4, generator=g, dtype=torch.float64) for _ in range(4))
    for cfg, stg, sigma in ((4.0, 1.0, 0.9), (1.0, 2.5, 0.3), (3.0, -0.5, 1.0)):
        gv = vp + (cfg - 1.0) * (vp - vn)
        v = gv + stg * (vp - vq)
        x0 = O.to_denoised(x, v, sigma, O.F64)
        xp, xn, xq = (O.to_denoised(x, t, sigma, O.F64) for t in (vp, vn, vq))
        ref = xp + C.CFGGuider(cfg).delta(xp, xn) + C.STGGuider(stg).delta(xp, xq)
        assert float((x0 - ref).norm() / ref.norm()) < 1e-12


# ------------------------------------------------------------------------------------------- ref_stg restatement
def _tiny():
    cfg = O.DiTConfig(num_layers=2, heads=2, caption_channels=64)
    W = O.make_weights(cfg, seed=3)
    g = torch.Generator().manual_seed(9)
    B, F, H, Wd = 2, 1, 2, 4
    N = F * H * Wd
    lat = torch.randn(B, N, 128, generator=g)
    ctx = torch.randn(B, 8, 64, generator=g)
    ts = torch.full((B, N), 0.5)
    pe = O.precompute_freqs_cis(torch.from_numpy(O.create_position_grid(1, F, H, Wd)), cfg.dim, heads=cfg.heads)
    return cfg, W, lat, ctx, ts, pe


def test_ref_stg_without_blocks_is_the_oracle_forward():
    cfg, W, lat, ctx, ts, pe = _tiny()
    ref = O.ltx_forward(lat, ts, ctx, pe, W, cfg, O.BF16)
    assert torch.equal(ref_stg.ltx_forward_stg(lat, ts, ctx, pe, W, cfg, O.BF16, rows=[0, 1], blocks=[]), ref)
    assert torch.equal(ref_stg.ltx_forward_stg(lat, ts, ctx, pe, W, cfg, O.BF16, rows=[], blocks=None), ref)
    assert O.attention.__name__ == "attention" and O.sdpa.__name__ == "sdpa"          # the oracle is restored
    pert = ref_stg.ltx_forward_stg(lat, ts, ctx, pe, W, cfg, O.BF16, rows=[1], blocks=[1])
    assert torch.equal(pert[0], ref[0]) and not torch.equal(pert[1], ref[1])


def test_ref_stg_perturbed_attention_returns_v():
    cfg, W, lat, ctx, ts, pe = _tiny()
    p = O.BF16
    x = O.linear(p.r(lat), W["patchify_proj.weight"], W["patchify_proj.bias"], p)
    t = p.r(p.r(ts) * cfg.timestep_scale_multiplier)
    ss, _ = O.adaln_single(t.reshape(-1), W, "adaln_single", p)
    c = O.linear(ctx, W["caption_projection.linear1.weight"], W["caption_projection.linear1.bias"], p)
    c = O.linear(O.gelu_tanh(c, p), W["caption_projection.linear2.weight"], W["caption_projection.linear2.bias"], p)
    cos, sin = pe
    pe2 = (cos.expand(2, *cos.shape[1:]), sin.expand(2, *sin.shape[1:]))
    for blk, hit in ((0, True), (1, False)):
        taps = {}
        with ref_stg.skip_self_attention(rows=[1], blocks=[0]):
            O.transformer_block(x, ss.reshape(2, x.shape[1], -1), c, pe2, W, blk, cfg, p, taps=taps)
        assert torch.equal(taps["a1.att"][1], taps["a1.v"][1]) == hit
        assert not torch.equal(taps["a1.att"][0], taps["a1.v"][0])
        assert not torch.equal(taps["a2.att"][1], taps["a2.v"][1])          # cross-attention (S = N here) is untouched
