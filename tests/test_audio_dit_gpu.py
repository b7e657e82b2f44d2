"""The audio-only transformer (head dim 64, one position axis) on the device: forward, denoise_audio_only, generate_video(audio=True).

The yardstick is computed here, not pinned (the rule of tests/test_gemma_model_gpu.py / test_audio_model_gpu.py): oracle.dit
restates this model unchanged (DiTConfig.heads / d_head / max_pos, sdpa derives the head dim), so e_ref = rel-L2 of oracle.dit
under BF16_FLASH against F64 and the device must satisfy err <= 1.25 * e_ref.  The 1.25 is the project's stated margin between
two bf16 evaluations with different summation orders; a wrong head split or rotation partner moves a state by >= 1e-1 against
e_ref ~ 5e-3.  Both columns are printed and ledgered.
  (a) tiny model L = 2, H = 8, D = 512, caption 256, B = 2, S = 70; T = 21 (below one key tile, inside a 16-row block) and
      T = 70 (ragged in the second key tile): every hidden state and the velocity;
  (b) one full-width block: L = 1, H = 32, D = 2048, T = 126, S = 128;
  (c) denoise_audio_only over two steps against the same loop written with the oracle's ltx_forward / to_denoised / euler_step;
      eager against use_graph, with and without cache_context, and two runs: bit-identical;
  (d) generate_video(audio=True, audio_transformer=..., audio_prompt_embeds=...) writes a .wav of the expected frame count and
      reports the audio_generate phase."""
import json
import wave

import parity
import pytest
import torch

from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SIGMA = 0.725


def _rel(a, b) -> float:
    return parity.rel_l2(a, b)


def _model(cfg: O.DiTConfig, W, dev):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    mc = LTXModelConfig.audio(num_attention_heads=cfg.heads, num_layers=cfg.num_layers, cross_attention_dim=cfg.dim,
                              caption_channels=cfg.caption_channels)
    assert mc.attention_head_dim == cfg.d_head == 64 and tuple(mc.positional_embedding_max_pos) == tuple(cfg.max_pos) == (20,)
    return LTXModel(mc, {k: v.to(dev) for k, v in W.items()})


def _rule(what, rows):
    for name, e_ref, e_dev in rows:
        print(f"{what} {name}: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    for name, e_ref, e_dev in rows:
        parity.auto(e_ref, 1.0, tag=f"{what}_{name}_e_ref")
        parity.auto(e_dev, 1.25 * e_ref, tag=f"{what}_{name}_device")


def _forward_case(dev, cfg, W, model, B, T, S, seed):
    from mlx_video_amd.ltx_model import TimestepPlan, precompute_freqs_cis
    from mlx_video_amd.schedulers import create_audio_position_grid
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, T, cfg.in_channels, generator=g).to(BF)
    ctx = torch.randn(B, S, cfg.caption_channels, generator=g).to(BF)
    pos = create_audio_position_grid(B, T)
    ts = torch.full((B, T), O.bf16_round_scalar(SIGMA))
    pe = O.precompute_freqs_cis(pos, cfg.dim, cfg.theta, cfg.max_pos, cfg.heads)
    v64, h64 = O.ltx_forward(lat, ts, ctx, pe, W, cfg, O.F64, return_hidden=True)
    vpol, hpol = O.ltx_forward(lat, ts, ctx, pe, W, cfg, O.BF16_FLASH, return_hidden=True)
    hidden = []
    pe_dev = precompute_freqs_cis(pos[:1].to(dev), cfg.dim, cfg.theta, cfg.max_pos, cfg.heads)
    v = model.forward_tokens(lat.to(dev), TimestepPlan.from_timesteps(ts.to(BF).to(dev)), ctx.to(dev), pe_dev, hidden=hidden)
    torch.cuda.synchronize()
    assert len(hidden) == cfg.num_layers
    rows = [(f"hidden{i}", _rel(hpol[i], h64[i]), _rel(hidden[i], h64[i])) for i in range(cfg.num_layers)]
    rows.append(("velocity", _rel(vpol, v64), _rel(v, v64)))
    return rows


TINY = O.DiTConfig(num_layers=2, heads=8, d_head=64, caption_channels=256, max_pos=(20,))


@pytest.fixture(scope="module")
def tiny(dev):
    W = O.make_weights(TINY, seed=7)
    return W, _model(TINY, W, dev)


@pytest.mark.parametrize("T", [21, 70])
def test_tiny_audio_model_against_float64(dev, tiny, T):
    W, model = tiny
    _rule(f"tiny_T{T}", _forward_case(dev, TINY, W, model, 2, T, 70, 11 + T))


def test_full_width_audio_block_against_float64(dev):
    cfg = O.DiTConfig(num_layers=1, heads=32, d_head=64, max_pos=(20,))
    W = O.make_weights(cfg, seed=8)
    _rule("full_width", _forward_case(dev, cfg, W, _model(cfg, W, dev), 1, 126, 128, 5))


def _oracle_loop(lat, pos, ctx, W, cfg, sig, p):
    """generate.py:994-1027 with the oracle's pieces: tokens by transpose(0,2,1,3).reshape, timesteps and x0 with the bf16 sigma
    (the loop holds sigma in the model dtype), Euler in the policy's arithmetic with the Python floats."""
    b, c, t, f = lat.shape
    pe = O.precompute_freqs_cis(pos, cfg.dim, cfg.theta, cfg.max_pos, cfg.heads)
    x = p.r(lat)
    for i in range(len(sig) - 1):
        s_bf = O.bf16_round_scalar(sig[i])
        tok = x.permute(0, 2, 1, 3).reshape(b, t, c * f)
        v = O.ltx_forward(tok, torch.full((b, t), s_bf), ctx, pe, W, cfg, p)
        vel = v.reshape(b, t, c, f).permute(0, 2, 1, 3)
        x = O.euler_step(x, O.to_denoised(x, vel, s_bf, p), sig[i], sig[i + 1], p)
    return x


def test_denoise_audio_only_loop(dev, tiny):
    from mlx_video_amd.denoise import denoise_audio_only
    from mlx_video_amd.schedulers import STAGE_1_SIGMAS, _subsample_sigmas, create_audio_position_grid
    W, model = tiny
    B, T, S = 2, 21, 70
    sig = _subsample_sigmas(list(STAGE_1_SIGMAS), 2, "farthest")
    assert len(sig) == 3 and sig[-1] == 0.0
    g = torch.Generator().manual_seed(31)
    lat = torch.randn(B, 8, T, 16, generator=g).to(BF)
    ctx = torch.randn(B, S, TINY.caption_channels, generator=g).to(BF)
    pos = create_audio_position_grid(B, T)
    x64 = _oracle_loop(lat, pos, ctx, W, TINY, sig, O.F64)
    xpol = _oracle_loop(lat, pos, ctx, W, TINY, sig, O.BF16_FLASH)
    args = (lat.to(dev), pos.to(dev), ctx.to(dev), model, sig)
    out = denoise_audio_only(*args)
    assert out.shape == lat.shape and out.dtype == BF
    _rule("loop", [("latents", _rel(xpol, x64), _rel(out, x64))])
    assert torch.equal(out, denoise_audio_only(*args)), "two runs differ"
    assert torch.equal(out, denoise_audio_only(*args, cache_context=True)), "cache_context changes the bits"
    eager = denoise_audio_only(*args, compile_step=True)
    assert torch.equal(eager, denoise_audio_only(*args, compile_step=True, use_graph=True)), "the captured step differs from the eager one"
    assert torch.equal(eager, denoise_audio_only(*args, compile_step=True, use_graph=True, cache_context=True)), \
        "the captured step with cache_context differs"


def test_generate_video_audio_surface(dev, tmp_path, tiny):
    import ref_audio as A
    from mlx_video_amd.audio_vae import AudioDecoder, Vocoder
    from mlx_video_amd.generate import generate_video
    from mlx_video_amd.pipelines import PipelineType
    from mlx_video_amd.schedulers import compute_audio_frames
    from test_pipeline_gpu import _Noise, _mods
    _, audio_model = tiny
    on = lambda W: {k: v.to(dev) for k, v in W.items()}
    dec = AudioDecoder(on(A.make_decoder_weights(seed=7, ch=64, num_res_blocks=1)), ch=64, num_res_blocks=1)
    voc = Vocoder(on(A.make_vocoder_weights(seed=3)))
    m = _mods(dev)
    g = torch.Generator().manual_seed(50)
    emb = torch.randn(2, 64, 256, generator=g).to(BF)
    aemb = torch.randn(1, 70, TINY.caption_channels, generator=g).to(BF)
    out, prof = tmp_path / "clip.npy", tmp_path / "clip.profile.json"
    kw = dict(prompt="x", pipeline=PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
              transformer=m["transformer"], vae_decoder=m["vae_decoder"], prompt_embeds=emb[0:1], negative_prompt_embeds=emb[1:2],
              device=dev, audio=True, audio_transformer=audio_model, audio_prompt_embeds=aemb, audio_steps=2, audio_decoder=dec,
              vocoder=voc)
    generate_video(noise_fn=_Noise(7, dev), output_path=str(out), profile_json_path=str(prof), profile=True, **kw)
    T = compute_audio_frames(9, 24.0)
    assert T == 9
    frames = 240 * (4 * T - 3)
    with wave.open(str(tmp_path / "clip.wav"), "rb") as wf:
        assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()) == (2, 2, 24000, frames)
        pcm = wf.readframes(frames)
    rep = json.loads(prof.read_text())
    assert rep["audio"] is True and rep["phases_s"]["audio_generate"] > 0 and rep["phases_s"]["audio_decode"] > 0
    # the audio is seeded from `seed` alone: other video noise, the same waveform
    out2 = tmp_path / "clip2.npy"
    generate_video(noise_fn=_Noise(8, dev), output_path=str(out2), **kw)
    with wave.open(str(tmp_path / "clip2.wav"), "rb") as wf:
        assert wf.readframes(frames) == pcm


def test_text_connector_both_runs_each_set_over_shared_features(dev):
    """TextConnector(video, audio).both(): the video context is the video connector's own call bit for bit, and the audio context
    is what a connector built from the audio set (same aggregate_embed: the feature extractor is shared) gives alone."""
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    D, L = 256, 3
    Wv = random_connector_weights(dev, D=D, L=L, layers=1, R=16, seed=17)
    Wa = dict(random_connector_weights(dev, D=D, L=L, layers=1, R=16, seed=18), **{"aggregate_embed.weight": Wv["aggregate_embed.weight"]})
    g = torch.Generator().manual_seed(19)
    hs = torch.randn(L, 2, 32, D, generator=g).to(BF).to(dev)
    mask = torch.tensor([[0] * 10 + [1] * 22, [1] * 32]).to(dev)
    video, audio = TextConnector(Wv, Wa).both(hs, mask)
    assert torch.equal(video, TextConnector(Wv)(hs, mask))
    assert torch.equal(audio, TextConnector(Wa)(hs, mask))
    assert not torch.equal(video, audio)
