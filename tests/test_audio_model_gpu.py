"""The audio decode end to end on the device: AudioDecoder, Vocoder, decode_audio and the generate_video surface.

The yardstick is computed here, not pinned (the rule of tests/test_gemma_model_gpu.py): e_ref[s] = rel-L2 of the bf16-policy
restatement (tests/ref_audio.py: rounding at the device path's rounding points, sums in float64) against the float64 restatement
at stage output s, and the device must satisfy err_device[s] <= 1.25 * e_ref[s] for every stage.  The 1.25 exists because two
bf16 evaluations with different summation orders are samples of one error size, not ordered; it leaves no room for a fault - a
wrong tap, a polyphase panel off by one phase or a mean over the wrong blocks moves a stage by >= 1e-1 against e_ref ~ 1e-2.
Shapes: the decoder at ch = 64 with one res block on latents (2, 8, 5, 8) (channels 256 / 128 / 64, 5 -> 9 -> 17 frames, 8 -> 32
bins); the vocoder's full channel plan (1024 -> 32, all 45 res-block convolutions, five polyphase panels) on 5 mel frames (1200
samples).  Random weights scaled by fan-in^-1/2.  Both columns are printed."""
import wave

import numpy as np
import pytest
import torch

import ref_audio as A

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64


def _on(W, dev):
    return {k: v.to(dev) for k, v in W.items()}


@pytest.fixture(scope="module")
def vocoder_run(dev):
    """One vocoder run shared by the tests below: weights, mel, the device waveform and stage outputs, both restatements."""
    from mlx_video_amd.audio_vae import Vocoder
    W = A.make_vocoder_weights(seed=3)
    g = torch.Generator().manual_seed(4)
    mel = torch.randn(2, 2, 5, 64, generator=g).to(BF)
    voc = Vocoder(_on(W, dev))
    voc.record = True
    wav = voc(mel.to(dev))
    torch.cuda.synchronize()
    Wd, ref, pol = _on(W, dev), {}, {}
    slope, fslope = voc.slope, voc.final_slope
    y64 = A.vocoder(mel.to(dev), Wd, False, slope, fslope, stages=ref)
    ypol = A.vocoder(mel.to(dev), Wd, True, slope, fslope, stages=pol)
    voc.record = False
    return dict(W=W, mel=mel, voc=voc, wav=wav, stages=dict(voc.stages), ref=ref, pol=pol, y64=y64, ypol=ypol)


def _stage_rule(what, rows):
    for name, e_ref, e_dev in rows:
        print(f"{what} {name}: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    for name, e_ref, e_dev in rows:
        assert e_dev <= 1.25 * e_ref, f"{what} {name}: device error {e_dev:.3e} exceeds 1.25 x the policy twin's {e_ref:.3e}"


def test_vocoder_stages_against_float64(vocoder_run):
    r = vocoder_run
    rows = []
    for name in sorted(r["ref"]):
        got = r["stages"][name][:, 0, :, 0]
        rows.append((name, A.rel_err(r["pol"][name], r["ref"][name]), A.rel_err(got, r["ref"][name])))
    assert len(rows) == 10
    rows.append(("waveform", A.rel_err(r["ypol"], r["y64"]), A.rel_err(r["wav"], r["y64"])))
    _stage_rule("vocoder", rows)


def test_vocoder_waveform_shape_and_range(vocoder_run):
    wav = vocoder_run["wav"]
    assert wav.dtype == torch.float32 and tuple(wav.shape) == (2, 2, 5 * 240)
    assert bool(torch.isfinite(wav).all()) and float(wav.abs().max()) <= 1.0


def test_decoder_stages_against_float64(dev):
    from mlx_video_amd.audio_vae import AudioDecoder
    cfg = dict(ch=64, num_res_blocks=1, mel_bins=32)
    W = A.make_decoder_weights(seed=5, ch=64, num_res_blocks=1, latent_bins=8)
    lat = torch.randn(2, 8, 5, 8, generator=torch.Generator().manual_seed(6)).to(BF)
    dec = AudioDecoder(_on(W, dev), **cfg)
    dec.record = True
    mel = dec(lat.to(dev))
    torch.cuda.synchronize()
    assert tuple(mel.shape) == (2, 2, 17, 32) and mel.dtype == BF
    ref, pol = {}, {}
    Wd = _on(W, dev)
    m64 = A.audio_decoder(lat.to(dev), Wd, False, stages=ref, **cfg)
    mpol = A.audio_decoder(lat.to(dev), Wd, True, stages=pol, **cfg)
    rows = [(n, A.rel_err(pol[n], ref[n]), A.rel_err(dec.stages[n][:, 0], ref[n])) for n in ref]
    assert len(rows) == 1 + 2 + 3 * 2 + 2 + 1
    rows.append(("mel", A.rel_err(mpol, m64), A.rel_err(mel, m64)))
    _stage_rule("decoder", rows)


def test_decode_audio_and_generate_surface(dev, tmp_path, vocoder_run):
    """decode_audio gives float32 (2, 240 * (4T - 3)); generate_video(audio_latents=...) writes a .wav whose samples are
    decode_audio's under save_audio's rule, and reports the audio_decode phase."""
    from mlx_video_amd.audio_vae import AudioDecoder, decode_audio
    from mlx_video_amd.generate import generate_video
    from mlx_video_amd.pipelines import PipelineType
    from test_pipeline_gpu import _Noise, _mods
    dec = AudioDecoder(_on(A.make_decoder_weights(seed=7, ch=64, num_res_blocks=1), dev), ch=64, num_res_blocks=1)
    voc = vocoder_run["voc"]
    lat = torch.randn(1, 8, 2, 16, generator=torch.Generator().manual_seed(9)).to(BF).to(dev)
    wav = decode_audio(lat, dec, voc)
    assert wav.dtype == torch.float32 and tuple(wav.shape) == (2, 240 * 5)
    assert bool(torch.isfinite(wav).all()) and float(wav.abs().max()) <= 1.0
    assert torch.equal(wav, decode_audio(lat, dec, voc))                                   # bits depend on the arguments alone
    m = _mods(dev)
    emb = torch.randn(2, 64, 256, generator=torch.Generator().manual_seed(50)).to(BF)
    out = tmp_path / "clip.npy"
    prof = tmp_path / "clip.profile.json"
    generate_video(prompt="x", pipeline=PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
                   transformer=m["transformer"], vae_decoder=m["vae_decoder"], prompt_embeds=emb[0:1], negative_prompt_embeds=emb[1:2],
                   noise_fn=_Noise(7, dev), device=dev, output_path=str(out), audio_latents=lat, audio_decoder=dec, vocoder=voc,
                   profile_json_path=str(prof), profile=True)
    with wave.open(str(tmp_path / "clip.wav"), "rb") as wf:
        assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()) == (2, 2, 24000, 1200)
        pcm = np.frombuffer(wf.readframes(1200), dtype=np.int16).reshape(1200, 2)
    assert np.array_equal(pcm, (np.clip(wav.cpu().numpy().T, -1.0, 1.0) * 32767).astype(np.int16))
    import json
    rep = json.loads(prof.read_text())
    assert rep["audio"] is True and rep["phases_s"]["audio_decode"] > 0
