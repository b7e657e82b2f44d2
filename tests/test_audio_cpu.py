"""Audio decode on the host: the float64 restatement (tests/ref_audio.py) against an independent HiFi-GAN, the layout rules
(stereo packing, the ``(c f)`` statistics index, polyphase panels, causal halos and frame counts), the per-element bound of
tests/test_conv_taps_gpu.py shown to accept a float32 evaluation and reject the faults it exists for, the checkpoint key maps,
the WAV / mux writers, and the plan rules and refusals of the ``kernel=`` form of ``ops.conv3d``."""
import ctypes
import stat
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_audio as A

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
KS_PAIRS = [(16, 6), (15, 5), (8, 2), (4, 2), (4, 2)]


# ------------------------------------------------------------------------------------------------ the restatement
def test_vocoder_restatement_equals_speecht5_hifigan():
    """Mono, float64, the full rate / kernel plan on 32 initial channels: transformers' SpeechT5HifiGan (normalize_before=False)
    is the same network written independently.  1e-9: float64 sums in another order."""
    from transformers import SpeechT5HifiGan, SpeechT5HifiGanConfig
    from mlx_video_amd import weights
    cfg = SpeechT5HifiGanConfig(model_in_dim=64, upsample_initial_channel=32, upsample_rates=[6, 5, 2, 2, 2],
                                upsample_kernel_sizes=[16, 15, 8, 4, 4], normalize_before=False)
    m = SpeechT5HifiGan(cfg).double().eval()
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=F64) * (0.3 if p.dim() == 1 else (p[0].numel()) ** -0.5))
    sd = {k.replace("upsampler.", "upsamplers."): v for k, v in m.state_dict().items() if k not in ("mean", "scale")}
    W = {k: v.to(F64) for k, v in sd.items()}
    # the key map's layout rules, kept in float64 here (vocoder_weights itself casts to bf16)
    Wm = {}
    for k, v in W.items():
        kk = weights._vocoder_key(k, False)
        Wm[kk] = (v.permute(1, 2, 0) if kk.startswith("ups.") else v.permute(0, 2, 1)) if v.dim() == 3 else v
    mel = torch.randn(2, 7, 64, generator=g, dtype=F64)
    with torch.no_grad():
        want = m(mel)
    got = A.vocoder(mel, Wm, False, slope=0.1, final_slope=0.01)[:, 0]
    assert got.shape == want.shape == (2, 7 * 240)
    assert float((got - want).abs().max()) <= 1e-9


def test_stereo_packing_and_statistics_index():
    from mlx_video_amd.audio_vae import AudioDecoder, Vocoder
    voc = Vocoder.__new__(Vocoder)
    mel = torch.arange(2 * 2 * 3 * 64, dtype=F32).reshape(2, 2, 3, 64) / 1024
    x = voc.pack_mel(mel)
    assert x.shape == (2, 1, 3, 1, 128) and x.dtype == BF
    for b, s, t, f in [(0, 0, 0, 0), (1, 1, 2, 63), (0, 1, 1, 5), (1, 0, 2, 40)]:
        assert float(x[b, 0, t, 0, s * 64 + f]) == float(mel[b, s, t, f].to(BF))
    assert voc.pack_mel(mel[:, 0]).shape == (2, 1, 3, 1, 64)
    # statistics entry c * F + f scales latent [b, c, t, f]
    W = A.make_decoder_weights(seed=1, ch=64, num_res_blocks=1)
    W["per_channel_statistics._std_of_means"] = torch.arange(1, 129, dtype=F32).to(BF)
    W["per_channel_statistics._mean_of_means"] = -torch.arange(128, dtype=F32).to(BF)
    dec = AudioDecoder(W, ch=64, num_res_blocks=1)
    lat = torch.ones(1, 8, 2, 16, dtype=BF)
    y = dec.denormalize(lat)
    assert y.shape == (1, 1, 2, 16, 64) and float(y[..., 8:].abs().max()) == 0.0
    for c, f in [(0, 0), (3, 7), (7, 15), (1, 0)]:
        assert float(y[0, 0, 1, f, c]) == float(c * 16 + f + 1) - float(c * 16 + f)
    got = A.denormalize(lat, W, True)
    assert torch.equal(got, y[:, 0, :, :, :8].to(F64))


@pytest.mark.parametrize("k,s", KS_PAIRS[:4])
@pytest.mark.parametrize("T", [1, 2, 9])
def test_polyphase_panel_equals_conv_transpose(k, s, T):
    from mlx_video_amd.audio_vae import pack_conv_transpose
    g = torch.Generator().manual_seed(k * 10 + s)
    Cin, Cout = 6, 5
    w = torch.randn(Cout, k, Cin, generator=g, dtype=F64)
    b = torch.randn(Cout, generator=g, dtype=F64)
    x = torch.randn(2, T, Cin, generator=g, dtype=F64)
    panel, pb, (pt, pbot) = pack_conv_transpose(w, b, s)
    assert panel.shape == (s * Cout, pt + pbot + 1, 1, Cin) and pt + pbot + 1 == {(16, 6): 3, (15, 5): 3, (8, 2): 5, (4, 2): 3}[(k, s)]
    y, _ = A.conv_taps(x[:, None, :, None], panel, pb, 1, (pt, pbot, 0, 0))
    got = y[:, 0, :, 0].reshape(2, T * s, Cout)                       # (T, s*Cout) viewed as (T*s, Cout): no copy
    want = F.conv_transpose1d(x.transpose(1, 2), w.permute(2, 0, 1), b, stride=s, padding=(k - s) // 2).transpose(1, 2)
    assert want.shape == got.shape and float((got - want).abs().max()) <= 1e-12


def test_pack_conv_transpose_refuses_odd_overlap():
    from mlx_video_amd.audio_vae import pack_conv_transpose
    with pytest.raises(ValueError):
        pack_conv_transpose(torch.zeros(2, 5, 2), torch.zeros(2), 2)


@pytest.mark.parametrize("T", [1, 2, 5])
def test_decoder_frame_counts(T):
    """Causal halo (2 above, none below) keeps the length, upsample-and-drop gives 2n - 1 twice, crop / pad lands on 4T - 3."""
    from mlx_video_amd.audio_vae import AudioDecoder
    W = A.make_decoder_weights(seed=2, ch=64, num_res_blocks=1, latent_bins=4)
    lat = torch.randn(1, 8, T, 4, generator=torch.Generator().manual_seed(T)).to(BF)
    st = {}
    mel = A.audio_decoder(lat, W, False, ch=64, num_res_blocks=1, mel_bins=16, stages=st)
    assert st["conv_in"].shape[1] == T and st["up.2.upsample"].shape[1] == 2 * T - 1 and st["up.1.upsample"].shape[1] == 4 * T - 3
    assert mel.shape == (1, 2, 4 * T - 3, 16)
    # causal: frame t of the output depends on latent frames <= ceil(t / 4) only
    lat2 = lat.clone()
    lat2[:, :, -1] += 1.0
    mel2 = A.audio_decoder(lat2, W, False, ch=64, num_res_blocks=1, mel_bins=16)
    if T > 1:
        keep = 4 * (T - 1) - 3
        assert torch.equal(mel[:, :, :keep], mel2[:, :, :keep]) and not torch.equal(mel, mel2)
    dec = AudioDecoder.__new__(AudioDecoder)
    dec.out_ch = 2
    h = torch.arange(1 * 5 * 3 * 4, dtype=F32).reshape(1, 5, 3, 4)
    out = dec._adjust(h, 7, 2)                                           # pads time 5 -> 7, crops bins 3 -> 2, channels 4 -> 2
    assert out.shape == (1, 2, 7, 2) and float(out[:, :, 5:].abs().max()) == 0 and torch.equal(out[0, :, :5], h[0, :, :2, :2].permute(2, 0, 1))
    assert torch.equal(A.adjust_output(h, 7, 2, 2), out)


# ------------------------------------------------------------------------------------------------ the bound
def _bound_case(seed, resid, nmean, slope, dil=3, k=7, B=2, T=40, C=64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, 1, C, generator=g).to(BF)
    w = (torch.randn(C, k, 1, C, generator=g) * (k * C) ** -0.5).to(BF)
    b = (0.1 * torch.randn(C, generator=g)).to(BF)
    ex = [torch.randn(B, 1, T, 1, C, generator=g).to(BF) for _ in range(3)]
    return x, w, b, (ex[0] if resid else None), tuple(ex[1:nmean]) if nmean else (), slope


def _f32_eval(x, w, b, dil, pad, r, mw, slope, xsrc=None):
    """The kernel's arithmetic in float32 on the host: fp32 sum, then the epilogue with bf16 roundings."""
    c = A.conv_taps(x if xsrc is None else xsrc, w, b, dil, pad)[0].to(F32)
    y = c.to(BF).to(F32)
    if r is not None:
        y = (y + r.to(F32)).to(BF).to(F32)
    if mw:
        for a in mw:
            y = y + a.to(F32)
        y = (y / (len(mw) + 1)).to(BF).to(F32)
    act = torch.maximum(y, (y * slope).to(BF).to(F32)) if slope is not None else None
    return y, act


@pytest.mark.parametrize("form", ["plain", "resid", "mean2", "mean3", "leaky", "all"])
def test_bound_accepts_fp32_and_rejects_faults(form):
    kw = {"plain": (False, 0, None), "resid": (True, 0, None), "mean2": (False, 2, None), "mean3": (False, 3, None),
          "leaky": (False, 0, 0.1), "all": (True, 3, 0.1)}[form]
    dil, k = 3, 7
    pad = (9, 9, 0, 0)
    x, w, b, r, mw, slope = _bound_case(11, *kw)
    c, mag = A.conv_taps(x, w, b, dil, pad)
    y, act = A.taps_exact(c, r, mw, slope)
    e, e_act = A.taps_bound(c, mag, k * 64, r, mw, slope)
    out, aout = _f32_eval(x, w, b, dil, pad, r, mw, slope)
    assert float(((out.to(F64) - y).abs() / e).max()) <= 1.0
    if slope is not None:
        assert float(((aout.to(F64) - act).abs() / e_act).max()) <= 1.0
    # the policy twin (exact sums, the kernel's roundings) lies inside it too
    yp, ap = A.taps_policy(c, r, mw, slope)
    assert float(((yp - y).abs() / e).max()) <= 1.0

    def worst(w2=w, dil2=dil, pad2=pad, xsrc=None):
        o, _ = _f32_eval(x, w2, b, dil2, pad2, r, mw, slope, xsrc)
        return float(((o.to(F64) - y).abs() / e).max())

    w_bad = w.clone()
    w_bad[:, 3] = w[:, 4]                                                     # one wrong tap
    assert worst(w2=w_bad) > 50
    assert worst(dil2=4, pad2=(12, 12, 0, 0)) > 50                            # a dilation off by one
    # a tap read across the batch boundary: the two frames convolved as one 2T-long frame
    xs = x.reshape(1, 1, 2 * x.shape[2], 1, 64)
    o = _f32_eval(x, w, b, dil, pad, None, (), None, xsrc=xs)[0].reshape(x.shape[0], 1, x.shape[2], 1, 64)
    y0, _ = A.taps_exact(c)
    e0, _ = A.taps_bound(c, mag, k * 64)
    ratio = (o.to(F64) - y0).abs() / e0
    assert float(ratio[0, 0, -9:].max()) > 50 and float(ratio[0, 0, :-9].max()) <= 1.0


def test_tanh_figure_is_zero_for_an_exact_tanh_and_sees_a_wrong_one():
    x, w, b, *_ = _bound_case(5, False, 0, None, C=64)
    w = w[:2].contiguous()
    b = b[:2].contiguous()
    c, mag = A.conv_taps(x, w, b, 1, (3, 3, 0, 0))
    good = torch.tanh(c).to(F32)
    assert float(A.tanh_excess_ulps(good, c, mag, 7 * 64)) <= 0.5
    assert float(A.tanh_excess_ulps(torch.tanh(c).to(BF).to(F32), c, mag, 7 * 64)) > 1000        # a waveform rounded to bf16


# ------------------------------------------------------------------------------------------------ key maps, loaders
def _torch_layout(W, kind):
    """The product-layout dict as a PyTorch checkpoint would hold it."""
    out = {}
    for k, v in W.items():
        if kind == "vocoder" and v.dim() == 3:
            v = v.permute(2, 0, 1) if k.startswith("ups.") else v.permute(0, 2, 1)
        if kind == "decoder" and v.dim() == 4:
            v = v.permute(0, 3, 1, 2)
        out[k] = v.contiguous()
    return out


def test_key_maps_three_sources(tmp_path):
    from safetensors.torch import save_file
    from mlx_video_amd import weights
    Wd = A.make_decoder_weights(seed=3, ch=64, num_res_blocks=1)
    Wv = A.make_vocoder_weights(seed=4, initial=64)
    stats = {"_mean_of_means": "mean-of-means", "_std_of_means": "std-of-means"}

    def same(got, want):
        assert set(got) == set(want)
        assert all(got[k].dtype == BF and torch.equal(got[k], want[k]) for k in want)

    # 1. unified: `audio_vae.` / `vocoder.` prefixes, MLX layouts and names as they are
    uni = {"audio_vae.decoder." + k: v for k, v in Wd.items() if not k.startswith("per_channel")}
    uni.update({"audio_vae." + k: v for k, v in Wd.items() if k.startswith("per_channel")})
    uni.update({"vocoder." + k: v for k, v in Wv.items()})
    uni["audio_vae.encoder.conv_in.conv.weight"] = torch.zeros(1)
    uni["transformer.x"] = torch.zeros(1)
    pick_a = {k: v for k, v in uni.items() if k.startswith("audio_vae.")}
    same(weights.audio_decoder_weights(pick_a, "cpu", "mlx"), Wd)
    same(weights.vocoder_weights({k: v for k, v in uni.items() if k.startswith("vocoder.")}, "cpu", "mlx"), Wv)
    # 2. the component files: PyTorch layouts, diffusers statistics names, upstream vocoder names
    comp = {"decoder." + k: v for k, v in _torch_layout(Wd, "decoder").items() if not k.startswith("per_channel")}
    comp["latents_mean"], comp["latents_std"] = Wd["per_channel_statistics._mean_of_means"], Wd["per_channel_statistics._std_of_means"]
    comp["encoder.conv_in.conv.weight"] = torch.zeros(4, 2, 3, 3)
    same(weights.audio_decoder_weights(comp, "cpu"), Wd)
    ren = {"ups.": "upsamplers.", "resblocks.": "resnets.", "conv_pre.": "conv_in.", "conv_post.": "conv_out."}
    vcomp = {}
    for k, v in _torch_layout(Wv, "vocoder").items():
        pre = next(p for p in ren if k.startswith(p))
        vcomp[ren[pre] + k[len(pre):]] = v
    same(weights.vocoder_weights(vcomp, "cpu"), Wv)
    # 3. the full checkpoint: `audio_vae.decoder.` / `vocoder.` among everything else, float32 on disk -> bf16
    full = {"audio_vae.decoder." + k: v.float() for k, v in _torch_layout(Wd, "decoder").items() if not k.startswith("per_channel")}
    for mine, theirs in stats.items():
        full["audio_vae.per_channel_statistics." + theirs] = Wd["per_channel_statistics." + mine].float()
    full["audio_vae.per_channel_statistics.channel"] = torch.zeros(128)
    full["vae.per_channel_statistics.mean-of-means"] = torch.zeros(128)
    full["vae.decoder.conv_in.conv.weight"] = torch.zeros(2, 2, 3, 3, 3)
    full.update({"vocoder." + k: v.float() for k, v in _torch_layout(Wv, "vocoder").items()})
    full["model.diffusion_model.audio_proj.weight"] = torch.zeros(2, 2)
    same(weights.audio_decoder_weights(full, "cpu"), Wd)
    same(weights.vocoder_weights(full, "cpu"), Wv)
    # the video VAE's loader keeps ignoring all of them
    vd = weights.vae_decoder_weights(full, "cpu")
    assert not any("audio" in k or "vocoder" in k for k in vd) and float(vd["latents_mean"].abs().max()) == 0.0
    # loaders: component files first, then the full checkpoint, then an error that says what was looked for
    repo = tmp_path / "repo"
    (repo / "audio_vae").mkdir(parents=True)
    save_file({k: v.contiguous() for k, v in comp.items()}, str(repo / "audio_vae" / "diffusion_pytorch_model.safetensors"))
    save_file({k: v.contiguous() for k, v in full.items() if k.startswith("vocoder.")}, str(repo / "ltx-2-19b-dev.safetensors"))
    dec = weights.load_audio_decoder(repo, "cpu")
    assert torch.equal(dec.conv_out[0], Wd["conv_out.conv.weight"]) and dec.conv_in[0].shape[-1] == 64
    voc = weights.load_vocoder(repo, "cpu")
    assert voc.ups[0][0].shape == (6 * 32, 3, 1, 64) and voc.upsample_factor == 240
    assert weights.load_vocoder(None, "cpu", unified_weights=uni).conv_post[0].shape == (2, 7, 1, 2)
    with pytest.raises(FileNotFoundError, match="audio_vae"):
        weights.load_audio_decoder(tmp_path / "empty", "cpu")


# ------------------------------------------------------------------------------------------------ media and surface
def test_save_audio_bytes(tmp_path):
    from mlx_video_amd import media
    a = np.array([[0.0, 0.5, -0.5, 2.0, np.nan, np.inf], [1.0, -1.0, 0.25, -3.0, -np.inf, 1e-5]], np.float32)
    media.save_audio(torch.from_numpy(a), tmp_path / "a.wav")
    with wave.open(str(tmp_path / "a.wav"), "rb") as wf:
        assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()) == (2, 2, 24000, 6)
        pcm = np.frombuffer(wf.readframes(6), np.int16).reshape(6, 2)
    assert pcm.T.tolist() == [[0, 16383, -16383, 32767, 0, 32767], [32767, -32767, 8191, -32767, -32767, 0]]
    media.save_audio(a[0], tmp_path / "m.wav", 16000)
    with wave.open(str(tmp_path / "m.wav"), "rb") as wf:
        assert (wf.getnchannels(), wf.getframerate(), wf.getnframes()) == (1, 16000, 6)


def test_mux_command_and_child(tmp_path, monkeypatch):
    import shutil
    from mlx_video_amd import media
    cmd = media.mux_command("ffmpeg", "v.mp4", "a.wav", "o.mp4")
    assert cmd == ["ffmpeg", "-y", "-i", "v.mp4", "-i", "a.wav", "-map", "0:v:0", "-map", "1:a:0", "-c:v", "copy", "-c:a", "aac",
                   "-b:a", "256k", "-ar", "24000", "-ac", "2", "-movflags", "+faststart", "o.mp4"]
    assert "-shortest" not in cmd
    monkeypatch.setattr(shutil, "which", lambda name: None)
    assert media.mux_video_audio("v.mp4", "a.wav", tmp_path / "o.mp4") is False
    fake = tmp_path / "ffmpeg"                                         # a stand-in that writes its arguments to its last one
    fake.write_text("#!/bin/sh\nfor a; do last=$a; done\necho \"$@\" > \"$last\"\n")
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setattr(shutil, "which", lambda name: str(fake))
    assert media.mux_video_audio("v.mp4", "a.wav", tmp_path / "o.txt") is True
    assert (tmp_path / "o.txt").read_text().split()[:5] == ["-y", "-i", "v.mp4", "-i", "a.wav"]
    bad = tmp_path / "ffmpeg_bad"
    bad.write_text("#!/bin/sh\necho boom >&2\nexit 3\n")
    bad.chmod(bad.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setattr(shutil, "which", lambda name: str(bad))
    with pytest.raises(RuntimeError, match="boom"):
        media.mux_video_audio("v.mp4", "a.wav", tmp_path / "o2.mp4")


def test_surface_names():
    import inspect
    from mlx_video_amd import generate as G
    sig = inspect.signature(G.generate_video).parameters
    assert all(sig[n].default is None for n in ("audio_latents", "audio_decoder", "vocoder", "output_audio"))
    args = G.build_parser().parse_args(["--audio-latents", "l.npy", "--output-audio", "o.wav"])
    assert args.audio_latents == "l.npy" and args.output_audio == "o.wav"
    with pytest.raises(ValueError, match="not supported"):
        G.generate_video(audio=True)                                   # the DiT branch is not here: audio=True keeps raising


# ------------------------------------------------------------------------------------------------ plan rules, refusals
def test_plan_rules():
    from mlx_video_amd import _lib, ops
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__import__("os").path.dirname(__file__)), "include", "ltxk.h")).read()
    assert "#define LTXK_VERSION 412" in hdr and _lib.load().ltxk_version() >= 412
    one = dict(kernel=(7, 1), dilation=3, pad=(9, 9, 0, 0))
    p = ops.conv3d_plan(2, 1, 300, 1, 64, 64, **one)
    assert p.kernel == _lib.CONV_KERNEL_TAPS and (p.tile_rows, p.tile_cols, p.row_tiles, p.col_tiles) == (256, 64, 3, 1)
    assert p.slices == 1 and p.ksteps == 7 and not p.tail and not p.fused_act       # 7 K-steps: nothing to split
    p = ops.conv3d_plan(2, 1, 300, 1, 512, 512, **one)                              # 12 tiles, 56 K-steps: 7 slices of 8
    assert (p.tile_cols, p.row_tiles, p.col_tiles, p.slices, p.ksteps) == (128, 3, 4, 7, 8)
    assert ops.conv3d_plan(2, 1, 300, 1, 512, 512, workspace=(0, 0), **one).slices == 1
    p = ops.conv3d_plan(2, 1, 300, 1, 512, 512, workspace=(1 << 12, 2 * 600 * 512 * 4), **one)      # the scratch holds two slabs
    assert (p.slices, p.ksteps) == (2, 28)
    p = ops.conv3d_plan(1, 1, 60000, 1, 32, 32, kernel=(3, 1), pad=(1, 1, 0, 0))     # Cin 32: 3 taps are one and a half K-steps
    assert (p.ksteps, p.slices, p.row_tiles) == (2, 1, 235)
    p = ops.conv3d_plan(2, 1, 5, 1, 1024, 3072, kernel=(3, 1), pad=(1, 1, 0, 0))     # the first polyphase panel
    assert (p.col_tiles, p.slices, p.ksteps) == (24, 6, 8)
    p = ops.conv3d_plan(1, 1, 501, 64, 128, 2, kernel=(3, 3), pad=(2, 0, 1, 1))      # conv_out: 126 tiles of 64 columns
    assert (p.tile_cols, p.row_tiles, p.slices, p.ksteps) == (64, 126, 2, 9)
    # without kernel= the plan is the 3x3x3 kernel's, as before
    assert ops.conv3d_plan(1, 3, 16, 16, 128, 128).kernel == _lib.CONV_KERNEL_PER_TAP


def test_refusals_on_the_host():
    from mlx_video_amd import _lib, ops
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt)
    x, w, b = z(1, 1, 8, 1, 64), z(64, 3, 1, 64), z(64)
    good = dict(kernel=(3, 1), pad=(1, 1, 0, 0))
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        ops.conv3d(x, w, b, False, 0, **good)                                        # everything else passes: only the device is wrong
    for kw, exc, word in [(dict(kernel=(3, 1), pad=(1, 0, 0, 0)), ValueError, "pad"), (dict(kernel=(3, 1)), ValueError, "pad"),
                          (dict(kernel=(17, 1), pad=(8, 8, 0, 0)), ValueError, "kh"), (dict(kernel=(3, 2), pad=(1, 1, 0, 1)), ValueError, "kw"),
                          (dict(kernel=(3, 1), pad=(9, 9, 0, 0), dilation=9), ValueError, "dilation"),
                          (dict(good, tanh_out=True, leaky=0.1), ValueError, "tanh_out"), (dict(good, keep_out=False), ValueError, "keep_out"),
                          (dict(good, mean_with=(x, x, x)), ValueError, "mean_with"), (dict(good, resid=z(1, 1, 8, 1, 32)), ValueError, "resid"),
                          (dict(good, mean_with=(z(1, 1, 8, 1, 64, dt=F32),)), TypeError, "mean_with"),
                          (dict(good, act=dict(eps=1e-6)), ValueError, "act"), (dict(dilation=2), ValueError, "kernel="),
                          (dict(leaky=0.1), ValueError, "kernel=")]:
        with pytest.raises(exc, match=word):
            ops.conv3d(x, w, b, False, 0, **kw)
    with pytest.raises(ValueError, match="weight"):
        ops.conv3d(x, z(64, 5, 1, 64), b, False, 0, **good)
    with pytest.raises(ValueError, match="Cin"):
        ops.conv3d(z(1, 1, 8, 1, 48), z(64, 3, 1, 48), b, False, 0, **good)
    with pytest.raises(ValueError, match="PAD_ZEROS"):
        ops.conv3d(x, w, b, False, ops.PAD_REFLECT, **good)
    # the library checks the struct's own size and the halo sums itself
    lib = _lib.load()
    a = _lib.ConvTapsArgs()
    pl = _lib.Conv3dPlan()
    assert lib.ltxk_conv_taps_plan(ctypes.byref(a), ctypes.byref(pl)) != 0 and b"struct_bytes" in lib.ltxk_last_error()
    with pytest.raises(_lib.LtxkError, match="Cin"):
        ops.conv3d_plan(1, 1, 8, 1, 48, 64, **good)
    with pytest.raises(ValueError, match="kernel="):
        ops.conv3d_plan(1, 1, 8, 1, 64, 64, dilation=2)
