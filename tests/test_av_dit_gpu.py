"""Joint audio-video denoising on the device: the AudioVideo forward (av_model.LTXAVModel), denoise_dev_av and
generate_video(audio_mode="joint").

The yardstick is the rule of tests/test_audio_dit_gpu.py, computed here and not pinned: ref_av_dit restates the model from the
reference's source out of oracle.dit's pieces; e_ref = rel-L2 of that restatement under BF16_FLASH against F64, and the device
must satisfy err <= 1.25 * e_ref, the project's stated margin between two bf16 evaluations with different summation orders.
tests/test_av_dit_cpu.py shows that a v2a reading the post-a2v stream, swapped scale / shift rows and a key side rotated with the
query's table each move a velocity by more than 10 * e_ref at the tiny shape.  Both columns are printed and ledgered.
  (a) tiny model: L = 2, video 8 heads x 128 (Dv = 1024), audio 8 heads x 64 (Da = 512), caption 256, B = 2, S = 70, video grid
      (3,5,5): N = 75 (ragged in the second 64-key tile and in a 16-row block), Ta in {21, 70}; one case with two distinct video
      timestep rows (frame 0 held at timestep 0): every hidden state of both streams and both velocities;
  (b) the degenerate model (cross to_out zeroed): at fuse = 0 both velocities are bit-identical to the sub-models' own
      forward_tokens; at the default fuse the 1.25 rule (the row statistics then come from another GEMM's epilogue);
  (c) one full-width block: Dv = 4096, Da = 2048, 32 heads each, L = 1, B = 1, N = 2*8*8 = 128, Ta = 34, S = 128;
  (d) denoise_dev_av over two steps against the restated loop, cfg_batch on and off; two runs, eager against use_graph, and a
      second call through the same graph_cache with other inputs: bit-identical to their eager runs; STG / apg refused;
  (e) generate_video(audio=True, audio_mode="joint", av_transformer=...) writes the .wav and reports the phases."""
import json
import wave

import parity
import pytest
import torch

import ref_av_dit as RA
from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SIGMA = 0.725
CFG_V = O.DiTConfig(num_layers=2, heads=8, d_head=128, caption_channels=256)
CFG_A = O.DiTConfig(num_layers=2, heads=8, d_head=64, caption_channels=256, max_pos=(20,))
GRID = (3, 5, 5)


def _rel(a, b) -> float:
    return parity.rel_l2(a, b)


def _rule(what, rows):
    for name, e_ref, e_dev in rows:
        print(f"{what} {name}: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    for name, e_ref, e_dev in rows:
        parity.auto(e_ref, 1.0, tag=f"{what}_{name}_e_ref")
        parity.auto(e_dev, 1.25 * e_ref, tag=f"{what}_{name}_device")


def _model(dev, W, cfg_v, cfg_a, fuse=15):
    from mlx_video_amd.av_model import LTXAVModel
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    Wv, Wa, Wc = W
    on = lambda d: {k: v.to(dev) for k, v in d.items()}
    mv = LTXModelConfig(num_attention_heads=cfg_v.heads, num_layers=cfg_v.num_layers, cross_attention_dim=cfg_v.dim,
                        caption_channels=cfg_v.caption_channels)
    ma = LTXModelConfig.audio(num_attention_heads=cfg_a.heads, num_layers=cfg_a.num_layers, cross_attention_dim=cfg_a.dim,
                              caption_channels=cfg_a.caption_channels)
    return LTXAVModel(LTXModel(mv, on(Wv), fuse=fuse), LTXModel(ma, on(Wa), fuse=fuse), on(Wc))


def _inputs(cfg_v, cfg_a, B, grid, Ta, S, seed, hold_frame0=False):
    from mlx_video_amd.schedulers import create_audio_position_grid
    g = torch.Generator().manual_seed(seed)
    N = grid[0] * grid[1] * grid[2]
    s = O.bf16_round_scalar(SIGMA)
    c = dict(vlat=torch.randn(B, N, 128, generator=g).to(BF), alat=torch.randn(B, Ta, 128, generator=g).to(BF),
             vctx=torch.randn(B, S, cfg_v.caption_channels, generator=g).to(BF), actx=torch.randn(B, S, cfg_a.caption_channels, generator=g).to(BF),
             vpos=torch.from_numpy(O.create_position_grid(B, *grid)), apos=create_audio_position_grid(B, Ta),
             vts=torch.full((B, N), s), ats=torch.full((B, Ta), s))
    if hold_frame0:                                    # a conditioning mask holds frame 0: its tokens run at timestep 0
        c["vts"][:, :grid[1] * grid[2]] = 0.0
    c["vpe"] = O.precompute_freqs_cis(c["vpos"], cfg_v.dim, cfg_v.theta, cfg_v.max_pos, cfg_v.heads)
    c["ape"] = O.precompute_freqs_cis(c["apos"], cfg_a.dim, cfg_a.theta, cfg_a.max_pos, cfg_a.heads)
    c["vcpe"] = RA.cross_freqs_cis(c["vpos"], cfg_v, cfg_a, cfg_v.heads)
    c["acpe"] = RA.cross_freqs_cis(c["apos"], cfg_v, cfg_a, cfg_a.heads)
    return c


def _ref(c, W, cfg_v, cfg_a, p):
    return RA.av_forward(c["vlat"], c["vts"], c["vctx"], c["vpe"], c["vcpe"], c["alat"], c["ats"], c["actx"], c["ape"], c["acpe"], *W,
                         cfg_v, cfg_a, p, return_hidden=True)


def _device(dev, model, c, hidden=True):
    from mlx_video_amd.ltx_model import TimestepPlan, precompute_freqs_cis
    V, A = model.video, model.audio
    vpos, apos = c["vpos"][:1].to(dev), c["apos"][:1].to(dev)
    vpe = precompute_freqs_cis(vpos, V.inner_dim, V.positional_embedding_theta, V.positional_embedding_max_pos, V.num_attention_heads)
    ape = precompute_freqs_cis(apos, A.inner_dim, A.positional_embedding_theta, A.positional_embedding_max_pos, A.num_attention_heads)
    hv, ha = ([], []) if hidden else (None, None)
    v, a = model.forward_tokens(c["vlat"].to(dev), TimestepPlan.from_timesteps(c["vts"].to(BF).to(dev)), c["vctx"].to(dev), vpe,
                                model.cross_freqs_cis(vpos, V.num_attention_heads),
                                c["alat"].to(dev), TimestepPlan.from_timesteps(c["ats"].to(BF).to(dev)), c["actx"].to(dev), ape,
                                model.cross_freqs_cis(apos, A.num_attention_heads), video_hidden=hv, audio_hidden=ha)
    torch.cuda.synchronize()
    return v, a, hv, ha


def _rows(ref64, refpol, got, L):
    v64, a64, hv64, ha64 = ref64
    vp, ap, hvp, hap = refpol
    v, a, hv, ha = got
    assert len(hv) == len(ha) == L
    rows = [(f"video_hidden{i}", _rel(hvp[i], hv64[i]), _rel(hv[i], hv64[i])) for i in range(L)]
    rows += [(f"audio_hidden{i}", _rel(hap[i], ha64[i]), _rel(ha[i], ha64[i])) for i in range(L)]
    return rows + [("video_velocity", _rel(vp, v64), _rel(v, v64)), ("audio_velocity", _rel(ap, a64), _rel(a, a64))]


@pytest.fixture(scope="module")
def tiny(dev):
    W = RA.make_av_weights(CFG_V, CFG_A, seed=7)
    return W, _model(dev, W, CFG_V, CFG_A)


@pytest.mark.parametrize("Ta,hold", [(21, False), (70, False), (21, True)], ids=["Ta21", "Ta70", "Ta21_two_timestep_rows"])
def test_tiny_av_model_against_float64(dev, tiny, Ta, hold):
    W, model = tiny
    c = _inputs(CFG_V, CFG_A, 2, GRID, Ta, 70, 11 + Ta + hold, hold_frame0=hold)
    got = _device(dev, model, c)
    if hold:
        assert torch.unique(c["vts"]).numel() == 2
    _rule(f"tiny_Ta{Ta}{'_hold' if hold else ''}", _rows(_ref(c, W, CFG_V, CFG_A, O.F64), _ref(c, W, CFG_V, CFG_A, O.BF16_FLASH), got, 2))
    # the single launch for the two cross modulations and the two single launches give the same bits
    model.modulate2 = False
    try:
        v2, a2, _, _ = _device(dev, model, c, hidden=False)
    finally:
        model.modulate2 = True
    assert torch.equal(v2, got[0]) and torch.equal(a2, got[1])


def test_degenerate_av_model_is_two_independent_forwards(dev, tiny):
    from mlx_video_amd.ltx_model import TimestepPlan, precompute_freqs_cis
    Wv, Wa, Wc = tiny[0]
    W0 = (Wv, Wa, RA.zero_cross_out(Wc))
    c = _inputs(CFG_V, CFG_A, 2, GRID, 21, 70, 41)
    # no carried statistics: bit-identical to each sub-model alone
    m0 = _model(dev, W0, CFG_V, CFG_A, fuse=0)
    v, a, _, _ = _device(dev, m0, c, hidden=False)
    for sub, lat, ts, ctx, pos, got in ((m0.video, "vlat", "vts", "vctx", "vpos", v), (m0.audio, "alat", "ats", "actx", "apos", a)):
        pe = precompute_freqs_cis(c[pos][:1].to(dev), sub.inner_dim, sub.positional_embedding_theta, sub.positional_embedding_max_pos,
                                  sub.num_attention_heads)
        alone = sub.forward_tokens(c[lat].to(dev), TimestepPlan.from_timesteps(c[ts].to(BF).to(dev)), c[ctx].to(dev), pe)
        assert torch.equal(got, alone)
    # the default launch structure: the 1.25 rule against the restatement (which equals oracle.dit there, test_av_dit_cpu.py)
    got = _device(dev, _model(dev, W0, CFG_V, CFG_A), c)
    _rule("degenerate", _rows(_ref(c, W0, CFG_V, CFG_A, O.F64), _ref(c, W0, CFG_V, CFG_A, O.BF16_FLASH), got, 2))


def test_full_width_av_block_against_float64(dev):
    cfg_v = O.DiTConfig(num_layers=1, heads=32, d_head=128)
    cfg_a = O.DiTConfig(num_layers=1, heads=32, d_head=64, max_pos=(20,))
    W = RA.make_av_weights(cfg_v, cfg_a, seed=8)
    c = _inputs(cfg_v, cfg_a, 1, (2, 8, 8), 34, 128, 5)
    got = _device(dev, _model(dev, W, cfg_v, cfg_a), c)
    _rule("full_width", _rows(_ref(c, W, cfg_v, cfg_a, O.F64), _ref(c, W, cfg_v, cfg_a, O.BF16_FLASH), got, 1))


# ------------------------------------------------------------------------------------------------ the loop
def _loop_inputs(seed, Ta=21, S=70):
    from mlx_video_amd.schedulers import create_audio_position_grid
    g = torch.Generator().manual_seed(seed)
    return dict(vlat=torch.randn(1, 128, *GRID, generator=g).to(BF), alat=torch.randn(1, 8, Ta, 16, generator=g).to(BF),
                vpos=torch.from_numpy(O.create_position_grid(1, *GRID)), apos=create_audio_position_grid(1, Ta),
                ctx=[torch.randn(1, S, 256, generator=g).to(BF) for _ in range(4)])          # video pos, neg, audio pos, neg


def _run_loop(dev, model, c, sig, **kw):
    from mlx_video_amd.denoise import denoise_dev_av
    out = denoise_dev_av(c["vlat"].to(dev), c["alat"].to(dev), c["vpos"].to(dev), c["apos"].to(dev), *[t.to(dev) for t in c["ctx"]],
                         model, sig, cfg_scale=4.0, **kw)
    torch.cuda.synchronize()
    return out


def test_denoise_dev_av_loop(dev, tiny):
    from mlx_video_amd.schedulers import ltx2_scheduler
    W, model = tiny
    sig = ltx2_scheduler(2, 75).tolist()
    assert len(sig) == 3 and sig[-1] == 0.0
    c = _loop_inputs(61)
    ref = lambda p: RA.denoise_dev_av(c["vlat"], c["alat"], c["vpos"], c["apos"], *c["ctx"], *W, CFG_V, CFG_A, sig, p, cfg_scale=4.0)
    (v64, a64), (vp, ap) = ref(O.F64), ref(O.BF16_FLASH)
    for batch in (False, True):
        v, a = _run_loop(dev, model, c, sig, cfg_batch=batch)
        assert v.shape == c["vlat"].shape and a.shape == c["alat"].shape and v.dtype == a.dtype == BF
        _rule(f"loop_cfg_batch{int(batch)}", [("video_latents", _rel(vp, v64), _rel(v, v64)), ("audio_latents", _rel(ap, a64), _rel(a, a64))])
        v2, a2 = _run_loop(dev, model, c, sig, cfg_batch=batch)
        assert torch.equal(v, v2) and torch.equal(a, a2), "two runs differ"
    # the captured step against the eager one, and a second call through the same cache with other latents and contexts
    cache = {}
    for inputs in (c, _loop_inputs(62)):
        ev, ea = _run_loop(dev, model, inputs, sig, cfg_batch=True, compile_step=True)
        gv, ga = _run_loop(dev, model, inputs, sig, cfg_batch=True, compile_step=True, use_graph=True, graph_cache=cache)
        assert torch.equal(ev, gv) and torch.equal(ea, ga), "the captured joint step differs from the eager one"
    assert len(cache) == 1
    for kw in (dict(stg_scale=1.0), dict(guider="apg")):
        with pytest.raises(ValueError, match="joint"):
            _run_loop(dev, model, c, sig, **kw)


# ------------------------------------------------------------------------------------------------ the surface
def test_generate_video_joint_surface(dev, tmp_path, tiny):
    import ref_audio as A
    from mlx_video_amd.audio_vae import AudioDecoder, Vocoder
    from mlx_video_amd.generate import generate_video
    from mlx_video_amd.pipelines import PipelineType
    from mlx_video_amd.schedulers import compute_audio_frames
    from test_pipeline_gpu import _Noise, _mods
    _, model = tiny
    on = lambda W: {k: v.to(dev) for k, v in W.items()}
    dec = AudioDecoder(on(A.make_decoder_weights(seed=7, ch=64, num_res_blocks=1)), ch=64, num_res_blocks=1)
    voc = Vocoder(on(A.make_vocoder_weights(seed=3)))
    g = torch.Generator().manual_seed(50)
    emb = torch.randn(4, 64, 256, generator=g).to(BF)
    out, prof = tmp_path / "clip.npy", tmp_path / "clip.profile.json"
    frames = generate_video(prompt="x", pipeline=PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2,
                            cfg_scale=4.0, vae_decoder=_mods(dev)["vae_decoder"], prompt_embeds=emb[0:1], negative_prompt_embeds=emb[1:2],
                            device=dev, audio=True, audio_mode="joint", av_transformer=model, audio_prompt_embeds=emb[2:3],
                            audio_negative_prompt_embeds=emb[3:4], audio_decoder=dec, vocoder=voc, noise_fn=_Noise(7, dev),
                            output_path=str(out), profile_json_path=str(prof), profile=True)
    assert frames.shape == (9, 128, 128, 3)
    T = compute_audio_frames(9, 24.0)
    n = 240 * (4 * T - 3)
    with wave.open(str(tmp_path / "clip.wav"), "rb") as wf:
        assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()) == (2, 2, 24000, n)
    rep = json.loads(prof.read_text())
    assert rep["audio"] is True and rep["audio_mode"] == "joint"
    assert rep["phases_s"]["dev_denoise"] > 0 and rep["phases_s"]["audio_decode"] > 0 and "audio_generate" not in rep["phases_s"]
