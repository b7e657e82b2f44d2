"""Separate audio generation, the parts that need no device: the audio key map, the config preset, the audio position grid, the
one-axis rotation table, the latent <-> volume view, the parser and refusals of the surface, the head_dim = 64 refusals of the ops
shims, and the float64 attention bound at head dim 64 (ref_attn64) - what it accepts and what it rejects."""
import math

import numpy as np
import pytest
import torch

import ref64 as R
import ref_attn64 as R64
from oracle import dit as O

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ weights, config
def test_audio_key_map_keeps_the_audio_transformer_and_nothing_cross_modal():
    from mlx_video_amd.weights import _transformer_key, audio_transformer_weights
    p = "model.diffusion_model."
    raw_keys = [
        # the audio transformer
        "audio_patchify_proj.weight", "audio_patchify_proj.bias", "audio_adaln_single.emb.timestep_embedder.linear_1.weight",
        "audio_adaln_single.linear.bias", "audio_caption_projection.linear_2.weight", "audio_scale_shift_table", "audio_proj_out.weight",
        "transformer_blocks.3.audio_attn1.to_q.weight", "transformer_blocks.3.audio_attn1.to_out.0.bias",
        "transformer_blocks.3.audio_attn1.q_norm.weight", "transformer_blocks.3.audio_attn2.to_k.weight",
        "transformer_blocks.3.audio_ff.net.0.proj.weight", "transformer_blocks.3.audio_ff.net.2.bias",
        "transformer_blocks.3.audio_scale_shift_table",
        # cross-modal and connector tensors: none of them belongs to it (audio_to_video_attn also starts with audio_)
        "transformer_blocks.3.audio_to_video_attn.to_q.weight", "transformer_blocks.3.video_to_audio_attn.to_out.0.weight",
        "transformer_blocks.3.scale_shift_table_a2v_ca_audio", "transformer_blocks.3.scale_shift_table_a2v_ca_video",
        "av_ca_video_scale_shift_adaln_single.linear.weight", "av_ca_a2v_gate_adaln_single.linear.weight",
        "audio_embeddings_connector.learnable_registers", "audio_embeddings_connector.transformer_1d_blocks.0.attn1.to_q.weight",
        # the video transformer
        "patchify_proj.weight", "scale_shift_table", "transformer_blocks.3.attn1.to_q.weight", "transformer_blocks.3.ff.net.2.bias",
        "transformer_blocks.3.scale_shift_table", "video_embeddings_connector.learnable_registers",
    ]
    raw = {p + k: torch.zeros(2, 2) for k in raw_keys}
    raw["vae.decoder.conv_in.weight"] = torch.zeros(2, 2)
    got = audio_transformer_weights(raw, "cpu")
    assert set(got) == {
        "patchify_proj.weight", "patchify_proj.bias", "adaln_single.emb.timestep_embedder.linear1.weight", "adaln_single.linear.bias",
        "caption_projection.linear2.weight", "scale_shift_table", "proj_out.weight", "transformer_blocks.3.attn1.to_q.weight",
        "transformer_blocks.3.attn1.to_out.bias", "transformer_blocks.3.attn1.q_norm.weight", "transformer_blocks.3.attn2.to_k.weight",
        "transformer_blocks.3.ff.proj_in.weight", "transformer_blocks.3.ff.proj_out.bias", "transformer_blocks.3.scale_shift_table"}
    assert all(v.dtype == BF for v in got.values())
    # the video map is unchanged: it still takes none of the audio tensors
    video = {_transformer_key(k) for k in raw} - {None}
    assert video == {"patchify_proj.weight", "scale_shift_table", "transformer_blocks.3.attn1.to_q.weight",
                     "transformer_blocks.3.ff.proj_out.bias", "transformer_blocks.3.scale_shift_table"}


def test_audio_config_preset_and_inference_from_shapes():
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    from mlx_video_amd.weights import infer_audio_transformer_config
    c = LTXModelConfig.audio()
    assert (c.num_attention_heads, c.attention_head_dim, c.inner_dim, c.cross_attention_dim) == (32, 64, 2048, 2048)
    assert tuple(c.positional_embedding_max_pos) == (20,) and (c.in_channels, c.out_channels, c.num_layers) == (128, 128, 48)
    assert LTXModelConfig().attention_head_dim == 128 and tuple(LTXModelConfig().positional_embedding_max_pos) == (20, 2048, 2048)
    tiny = LTXModelConfig.audio(num_attention_heads=8, num_layers=2, cross_attention_dim=512, caption_channels=256)
    shapes = {"patchify_proj.weight": (512, 128), "proj_out.weight": (128, 512), "caption_projection.linear1.weight": (512, 256),
              "transformer_blocks.0.attn1.to_q.weight": (512, 512), "transformer_blocks.1.attn1.to_q.weight": (512, 512)}
    assert infer_audio_transformer_config(shapes) == tiny
    assert set(LTXModel.expected_keys(tiny)) == set(O.make_weights(O.DiTConfig(num_layers=2, heads=8, d_head=64, caption_channels=256,
                                                                              max_pos=(20,)), seed=7))


# ------------------------------------------------------------------------------------------------ positions, table, latent view
def test_audio_position_grid_known_answers():
    from mlx_video_amd.schedulers import compute_audio_frames, create_audio_position_grid
    g = create_audio_position_grid(2, 3)
    assert g.dtype == torch.float32 and tuple(g.shape) == (2, 1, 3, 2)
    f = np.float32
    # latent frame i starts at mel frame max(4i - 3, 0); one mel frame is 160 / 16000 s
    starts = np.array([0, 1, 5], dtype=f) * 160 / 16000
    ends = np.array([1, 5, 9], dtype=f) * 160 / 16000
    assert np.array_equal(g[0, 0, :, 0].numpy(), starts) and np.array_equal(g[1, 0, :, 1].numpy(), ends)
    assert np.allclose(starts, [0, 0.01, 0.05]) and np.allclose(ends, [0.01, 0.05, 0.09])
    assert compute_audio_frames(33, 24) == 34 and compute_audio_frames(121, 24) == 126


@pytest.mark.parametrize("H,dim", [(8, 512), (32, 2048)])
def test_one_axis_rope_table_against_the_oracle(H, dim):
    """The host table of ltx_model.precompute_freqs_cis for (B,1,N,2) positions against oracle.dit.precompute_freqs_cis.  Both form
    the angle ((start+end)/2 / max_pos * 2 - 1) * theta^linspace * pi/2 in fp32 with the same operations, so the angles are
    equal bit for bit and the only difference allowed is the cos / sin evaluation of equal fp32 arguments: each evaluation is
    within 1 ulp of the exact value (the accuracy the vectorised and the scalar libm routines both document), hence two of
    them within 2 fp32 ulps of each other - asserted per element on the larger magnitude's ulp."""
    from mlx_video_amd.ltx_model import precompute_freqs_cis
    from mlx_video_amd.schedulers import create_audio_position_grid
    pos = create_audio_position_grid(2, 126)
    got = precompute_freqs_cis(pos, dim, 10000.0, (20,), H)
    ref = O.precompute_freqs_cis(pos, dim, 10000.0, (20,), H)
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape) == (2, H, 126, dim // H // 2)
        ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -126))) - 23)
        worst = float(((a - b).abs() / ulp).max())
        print(f"one-axis table H={H} dim={dim}: worst {worst:.2f} ulp")
        assert worst <= 2.0
    with pytest.raises(ValueError, match="axes"):
        precompute_freqs_cis(pos, dim, 10000.0, (20, 2048, 2048), H)


def test_audio_latent_volume_round_trip_is_the_reference_transpose():
    from mlx_video_amd.denoise import audio_latent_to_volume, audio_volume_to_latent
    lat = torch.randn(2, 8, 21, 16, generator=torch.Generator().manual_seed(3)).to(BF)
    vol = audio_latent_to_volume(lat)
    assert tuple(vol.shape) == (2, 128, 21, 1, 1) and vol.is_contiguous()
    tokens = O.latent_to_tokens(vol)                                             # what ops.latent_to_tokens computes of the volume
    assert torch.equal(tokens, lat.permute(0, 2, 1, 3).reshape(2, 21, 128))      # generate.py:936-937
    assert torch.equal(audio_volume_to_latent(vol), lat)
    vel = torch.randn(2, 21, 128, generator=torch.Generator().manual_seed(4)).to(BF)
    assert torch.equal(audio_volume_to_latent(O.tokens_to_latent(vel, vol.shape)), vel.reshape(2, 21, 8, 16).permute(0, 2, 1, 3))   # 950-951


# ------------------------------------------------------------------------------------------------ surface
def test_audio_parser_flags_and_refusals():
    import inspect
    from mlx_video_amd import generate as G
    sig = inspect.signature(G.generate_video).parameters
    assert [sig[n].default for n in ("audio_mode", "audio_model_repo", "audio_steps", "audio_transformer", "audio_prompt_embeds")] == \
        ["auto", None, 8, None, None]
    a = G.build_parser().parse_args([])
    assert (a.audio, a.audio_mode, a.audio_model_repo, a.audio_steps) == (False, "auto", None, 8)
    a = G.build_parser().parse_args(["--audio", "--audio-mode", "separate", "--audio-model-repo", "dir", "--audio-steps", "4"])
    assert (a.audio, a.audio_mode, a.audio_model_repo, a.audio_steps) == (True, "separate", "dir", 4)
    with pytest.raises(SystemExit):
        G.build_parser().parse_args(["--audio-mode", "both"])
    with pytest.raises(ValueError, match="(?s)audio.*not supported"):
        G.generate_video(audio=True)                                             # nothing to load an audio transformer from
    with pytest.raises(ValueError, match="(?s)joint.*not supported"):
        G.generate_video(audio=True, audio_mode="joint", audio_transformer=object())
    with pytest.raises(ValueError, match="audio_mode"):
        G.generate_video(audio=True, audio_mode="both")
    with pytest.raises(ValueError, match="audio-steps"):
        G.generate_video(audio=True, audio_transformer=object(), audio_steps=9)
    # "auto" resolves to separate: with a transformer given it gets past the audio refusals, to the first thing that is missing
    with pytest.raises(FileNotFoundError, match="no transformer"):
        G.generate_video(audio=True, audio_mode="auto", audio_transformer=object())


def test_denoise_audio_only_refuses_wrong_shapes():
    from types import SimpleNamespace
    from mlx_video_amd.denoise import denoise_audio_only
    tr = SimpleNamespace(config=SimpleNamespace(in_channels=128), positional_embedding_max_pos=[20])
    lat, pos, ctx = torch.zeros(1, 8, 5, 16), torch.zeros(1, 1, 5, 2), torch.zeros(1, 4, 256)
    with pytest.raises(ValueError, match="audio_latents"):
        denoise_audio_only(lat[0], pos, ctx, tr, [1.0, 0.0])
    with pytest.raises(ValueError, match="128"):
        denoise_audio_only(torch.zeros(1, 8, 5, 8), pos, ctx, tr, [1.0, 0.0])
    with pytest.raises(ValueError, match="audio_positions"):
        denoise_audio_only(lat, torch.zeros(1, 3, 5, 2), ctx, tr, [1.0, 0.0])
    tr.positional_embedding_max_pos = [20, 2048, 2048]
    with pytest.raises(ValueError, match="audio-only"):
        denoise_audio_only(lat, pos, ctx, tr, [1.0, 0.0])


# ------------------------------------------------------------------------------------------------ ops shims at head_dim = 64
def test_head_dim_64_shim_refusals():
    from mlx_video_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, dtype=BF)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    B, T, H = 2, 6, 8
    M, D = B * T, 64 * H
    qk = (z(M, 2 * D), 2, D, z(2, D))
    tail = (T, H, 1e-6)
    with pytest.raises(ValueError, match="cos"):                                   # the dh = 128 table shape
        ops.qknorm_rope(*qk, f32(H, T, 64), f32(H, T, 64), *tail, head_dim=64)
    with pytest.raises(ValueError, match="D = "):                                  # D != 64 * H
        ops.qknorm_rope(z(M, 2 * D), 2, D, z(2, D), f32(H, T, 32), f32(H, T, 32), T, H // 2, 1e-6, head_dim=64)
    with pytest.raises(ValueError, match="D = 256 must be 128"):                   # the default keeps today's message
        ops.qknorm_rope(z(M, 512), 2, 256, z(2, 256), None, None, T, 4, 1e-6)
    with pytest.raises(ValueError, match="head_dim"):
        ops.qknorm_rope(*qk, None, None, *tail, head_dim=32)
    with pytest.raises(ValueError, match="sumsq"):                                 # D/64 = H partials per segment
        ops.qknorm_rope(*qk, None, None, *tail, sumsq=f32(M, 2 * H - 1), head_dim=64)
    off = torch.zeros(M * 2 * D + 8, dtype=BF)[4:4 + M * 2 * D].view(M, 2 * D)      # 8 bytes past a 16-byte boundary
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.qknorm_rope(off, 2, D, z(2, D), None, None, *tail, head_dim=64)
    with pytest.raises(_lib.LtxkError, match="device tensor"):                     # well formed: refused for the device only
        ops.qknorm_rope(*qk, f32(H, T, 32), f32(H, T, 32), *tail, sumsq=f32(M, 2 * H), head_dim=64)

    att = (z(M, D), z(B * 70, D), z(B, D, 128), z(M, D), B, H, T, 70, 0.125)
    with pytest.raises(ValueError, match="q_sumsq"):
        ops.flash_attn(*att, q_sumsq=f32(M, 2 * H), q_norm_weight=z(D), head_dim=64)
    with pytest.raises(ValueError, match="head_dim"):
        ops.flash_attn(*att, head_dim=256)
    with pytest.raises(ValueError, match="q must be"):                             # operands at H * 128 columns are not dh = 64 ones
        ops.flash_attn(z(M, 2 * D), *att[1:], head_dim=64)
    with pytest.raises(ValueError, match="vt must be"):                            # V^T shorter than Tk
        ops.flash_attn(att[0], att[1], z(B, D, 64), *att[3:], head_dim=64)
    offq = torch.zeros(M * D + 8, dtype=BF)[4:4 + M * D].view(M, D)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.flash_attn(offq, *att[1:], head_dim=64)
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        ops.flash_attn(*att, head_dim=64)
    with pytest.raises(ValueError, match="q must be"):                             # and the default still reads them at 128
        ops.flash_attn(*att)


# ------------------------------------------------------------------------------------------------ the attention bound at dh = 64
SHAPES = [(1, 2, 77, 70), (2, 3, 129, 65), (1, 2, 100, 129)]
SCALE = 1.0 / math.sqrt(64)


def _ratio(out, ref, Tk):
    d, bound = R64.attention_bound(out, *ref, Tk)
    return d / bound


def test_ref_attn64_is_ref64_at_head_dim_128():
    q, k, v, planted = R.attention_inputs(1, 2, 20, 70, "spiked", 0)
    q2, k2, v2, planted2 = R64.attention_inputs(1, 2, 20, 70, "spiked", 0, 128)
    assert torch.equal(q, q2) and torch.equal(k, k2) and torch.equal(v, v2) and planted == planted2
    s = 1.0 / math.sqrt(128)
    assert all(torch.equal(a, b) for a, b in zip(R.attention(q, k, v, 2, s), R64.attention(q, k, v, 2, s, 128)))
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(6, 512, generator=g).to(BF), (1 + 0.3 * torch.randn(2, 256, generator=g)).to(BF)
    ang = torch.rand(2, 3, 64, generator=g)
    for cs in ((None, None), (torch.cos(ang), torch.sin(ang))):
        a, b = R.qknorm_rope(x, w, *cs, 3, 2, 1e-6), R64.qknorm_rope(x, w, *cs, 3, 2, 1e-6, 128)
        assert torch.equal(a[0], b[0]) and (a[1] is None and b[1] is None or torch.equal(a[1], b[1]))


@pytest.mark.parametrize("family", R64.ATTN_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_bound_dh64_accepts_every_correct_computation(shape, family):
    """The bound passes, on every element, oracle.dit.sdpa under the flash policy and under the fp32-P policy (sdpa takes the head
    dim from its inputs) and an fp32 emulation of a loop over 64-key tiles with the header's rounding points."""
    B, H, Tq, Tk = shape
    q, k, v, _ = R64.attention_inputs(B, H, Tq, Tk, family, 0, 64)
    ref = R64.attention(q, k, v, H, SCALE, 64)
    outs = {"flash": O.sdpa(q.float(), k.float(), v.float(), H, O.BF16_FLASH), "fp32_p": O.sdpa(q.float(), k.float(), v.float(), H, O.BF16),
            "tile_loop": R64.flash_loop_fp32(q, k, v, H, SCALE, 64)}
    for name, out in outs.items():
        worst = float(_ratio(out.to(BF), ref, Tk).max())
        print(f"{shape} {family} {name}: worst d/bound {worst:.3f}")
        assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("family", R64.ATTN_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_bound_dh64_rejects_planted_faults(shape, family):
    """Each fault a kernel of this structure could have puts at least one element beyond the bound: the last key dropped, an
    unmasked pad slot of the ragged tile (V^T pad 1024), every row stored one place off, the second key tile skipped."""
    B, H, Tq, Tk = shape
    q, k, v, _ = R64.attention_inputs(B, H, Tq, Tk, family, 0, 64)
    ref = R64.attention(q, k, v, H, SCALE, 64)
    for fault in ("drop_key", "pad_slot", "row_off", "skip_tile"):
        out = R64.flash_loop_fp32(q, k, v, H, SCALE, 64, fault=fault)
        worst = float(_ratio(out, ref, Tk).max())
        print(f"{shape} {family} {fault}: worst d/bound {worst:.3g}")
        assert worst > 1.0, fault


# ------------------------------------------------------------------------------------------------ the audio embeddings connector
@pytest.mark.parametrize("family", [0, 1, 2])
def test_audio_connector_key_families_load(tmp_path, family):
    """text_connector_weights(which="audio") reads the audio connector's tensors of the three key families under the module
    keys, with the shared aggregate_embed; the default still reads the video connector's and ignores these."""
    from safetensors.torch import save_file
    from mlx_video_amd.weights import text_connector_weights
    from test_text_stage_cpu import _connector_sd
    D, L = 128, 3
    sd, agg = _connector_sd(D, L)
    agg_key, video, audio = [
        ("text_embedding_projection.aggregate_embed.weight", "model.diffusion_model.video_embeddings_connector.", "model.diffusion_model.audio_embeddings_connector."),
        ("text_embedding_projection.aggregate_embed.weight", "connector.video_embeddings_connector.", "connector.audio_embeddings_connector."),
        ("text_proj_in.weight", "video_connector.", "audio_connector.")][family]
    raw = {video + k: v for k, v in sd.items()}
    raw.update({audio + k: (v.float() + 1).to(BF) for k, v in sd.items()})
    raw[agg_key] = agg
    path = tmp_path / "ltx-2-synthetic.safetensors"
    save_file({k: v.contiguous() for k, v in raw.items()}, str(path))
    name = lambda k: k.replace(".to_out.0.", ".to_out.").replace(".ff.net.0.proj.", ".ff.proj_in.").replace(".ff.net.2.", ".ff.proj_out.")
    Wv, Wa = text_connector_weights([path], "cpu"), text_connector_weights([path], "cpu", which="audio")
    assert set(Wv) == set(Wa) == {name(k) for k in sd} | {"aggregate_embed.weight_layer_major"}
    for k, v in sd.items():
        assert torch.equal(Wv[name(k)], v) and torch.equal(Wa[name(k)], (v.float() + 1).to(BF)), k
    assert torch.equal(Wv["aggregate_embed.weight_layer_major"], Wa["aggregate_embed.weight_layer_major"])
    with pytest.raises(ValueError, match="which"):
        text_connector_weights([path], "cpu", which="both")
    only_video = tmp_path / "video_only.safetensors"
    save_file({k: v.contiguous() for k, v in raw.items() if not k.startswith(audio)}, str(only_video))
    with pytest.raises(ValueError, match="audio_"):
        text_connector_weights([only_video], "cpu", which="audio")


def test_text_connector_without_audio_set_refuses_both():
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    W = random_connector_weights("cpu", D=128, L=2, layers=1, R=8)
    tc = TextConnector(W)
    assert tc.audio_blocks is None
    with pytest.raises(ValueError, match="audio"):
        tc.both(torch.zeros(2, 1, 8, 128), torch.ones(1, 8, dtype=torch.int64))
    bad = dict(random_connector_weights("cpu", D=128, L=2, layers=1, R=8, seed=2), learnable_registers=torch.zeros(4, 128, dtype=BF))
    with pytest.raises(ValueError, match="learnable_registers"):
        TextConnector(W, bad)
