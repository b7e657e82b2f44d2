"""Audio decode: audio VAE decoder (latents -> mel spectrogram) and HiFi-GAN vocoder (mel -> stereo 24 kHz waveform).

Follows the reference's ``audio_vae/audio_vae.py:221-468`` (AudioDecoder, config of ``generate.py:1711-1723``) and
``audio_vae/vocoder.py`` (Vocoder, ``generate.py:1770-1778``).  Every convolution is one ``ops.conv3d(kernel=...)`` launch
(csrc/conv_taps.hip): the decoder's causal 3x3 as ``pad=(2, 0, 1, 1)`` on (B,1,T,F,C) volumes, the vocoder's dilated
Conv1d with time as H and W = 1 on (B,1,T,1,C), its ConvTranspose1d as one stride-1 launch over a polyphase panel packed
once at load (``pack_conv_transpose``).  The vocoder's leaky ReLUs, residual adds, the mean of the three res blocks and
the final tanh run in the epilogues: no elementwise launch remains there.  Weights come in the layout the key maps of
``weights.py`` give: Conv2d (Cout,kh,kw,Cin), Conv1d (Cout,k,Cin), ConvTranspose1d (Cout,k,Cin)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops

BF16 = torch.bfloat16
LATENT_DOWNSAMPLE_FACTOR = 4
AUDIO_LATENT_CHANNELS = 8
AUDIO_SAMPLE_RATE = 24000
LRELU_SLOPE = 0.1
CAUSAL_3X3 = (2, 0, 1, 1)      # (top, bottom, left, right): causal on height (time), centred on width (mel bins)
PIXELNORM_EPS = 1e-6


def bf16_slope(slope: float) -> float:
    """The slope as the reference's ``x * negative_slope`` sees it: a Python scalar takes the bf16 array's dtype."""
    return float(torch.tensor(slope, dtype=torch.float32).to(BF16))


def pack_conv_transpose(w: torch.Tensor, bias: torch.Tensor, stride: int) -> Tuple[torch.Tensor, torch.Tensor, Tuple[int, int]]:
    """ConvTranspose1d(kernel k, stride s, padding p = (k - s) / 2) as a stride-1 convolution into s * Cout columns.
    ``w`` (Cout, k, Cin) holds Wt[ci, co, j] at w[co, j, ci].  Output sample q*s + r is
        y[q*s + r, co] = sum_m sum_ci x[q + f_r - m, ci] * Wt[ci, co, j_r + m*s],   j_r = (r + p) mod s, f_r = (r + p) div s,
    so over the union of offsets e = f_r - m the panel P[r*Cout + co, e - e_min, ci] = Wt[ci, co, j_r + (f_r - e)*s] (zero
    where that tap does not exist) gives y as the (T, s*Cout) output viewed as (T*s, Cout).  Returns (panel (s*Cout, taps, 1,
    Cin), bias repeated s times, (pad_top, pad_bottom) = (-e_min, e_max))."""
    Cout, k, Cin = w.shape
    s = int(stride)
    if (k - s) % 2 or k < s:
        raise ValueError(f"pack_conv_transpose: kernel {k} and stride {s} need k >= s and k - s even")
    p = (k - s) // 2
    taps = {}
    for r in range(s):
        j_r, f_r = (r + p) % s, (r + p) // s
        m = 0
        while j_r + m * s < k:
            taps[(r, f_r - m)] = j_r + m * s
            m += 1
    e_min, e_max = min(e for _, e in taps), max(e for _, e in taps)
    panel = torch.zeros((s, Cout, e_max - e_min + 1, 1, Cin), dtype=w.dtype, device=w.device)
    for (r, e), j in taps.items():
        panel[r, :, e - e_min, 0] = w[:, j]
    return panel.reshape(s * Cout, e_max - e_min + 1, 1, Cin).contiguous(), bias.repeat(s).contiguous(), (-e_min, e_max)


def _pad_cin(w: torch.Tensor, cin: int) -> torch.Tensor:
    """(Cout,kh,kw,Cin) with the input channels zero-padded to ``cin``."""
    if w.shape[-1] == cin:
        return w.contiguous()
    out = torch.zeros((*w.shape[:-1], cin), dtype=w.dtype, device=w.device)
    out[..., :w.shape[-1]] = w
    return out


class AudioDecoder:
    """Latents (B, 8, T, 16) -> mel spectrogram (B, 2, 4T-3, mel_bins).  PixelNorm, causal on height, no attention."""

    def __init__(self, weights: Dict[str, torch.Tensor], *, ch: int = 128, out_ch: int = 2, ch_mult: Sequence[int] = (1, 2, 4),
                 num_res_blocks: int = 2, z_channels: int = AUDIO_LATENT_CHANNELS, mel_bins: Optional[int] = 64):
        self.ch, self.out_ch, self.ch_mult, self.num_res_blocks = ch, out_ch, tuple(ch_mult), num_res_blocks
        self.z_channels, self.mel_bins = z_channels, mel_bins
        W = {k: v.to(BF16) for k, v in weights.items()}
        self.mean = W["per_channel_statistics._mean_of_means"].contiguous()
        self.std = W["per_channel_statistics._std_of_means"].contiguous()

        def conv(name):
            return W[f"{name}.conv.weight"].contiguous(), W[f"{name}.conv.bias"].contiguous()

        def block(name, cin, cout):
            b = {"conv1": conv(f"{name}.conv1"), "conv2": conv(f"{name}.conv2")}
            if cin != cout:
                w, bias = conv(f"{name}.nin_shortcut")
                b["nin"] = (w.reshape(cout, cin).contiguous(), bias)
            return b

        top = ch * self.ch_mult[-1]
        w, b = conv("conv_in")
        self.conv_in = (_pad_cin(w, 64), b)
        self.mid = [block("mid.block_1", top, top), block("mid.block_2", top, top)]
        self.up = {}
        cin = top
        for level in reversed(range(len(self.ch_mult))):
            cout = ch * self.ch_mult[level]
            blocks = []
            for i in range(num_res_blocks + 1):
                blocks.append(block(f"up.{level}.block.{i}", cin, cout))
                cin = cout
            self.up[level] = {"block": blocks, "upsample": conv(f"up.{level}.upsample.conv") if level != 0 else None}
        self.conv_out = conv("conv_out")
        self.stages = {}          # name -> tensor of the last call when ``record`` is set (tests)
        self.record = False

    @staticmethod
    def _conv(x, wb, resid=None):
        return ops.conv3d(x, wb[0], wb[1], False, ops.PAD_ZEROS, resid=resid, kernel=(3, 3), pad=CAUSAL_3X3)

    def _block(self, x, blk):
        h = ops.pixelnorm_act(x, PIXELNORM_EPS, True)
        h = self._conv(h, blk["conv1"])
        h = ops.pixelnorm_act(h, PIXELNORM_EPS, True)
        if "nin" in blk:
            w, b = blk["nin"]
            x = ops.gemm(x.view(-1, x.shape[-1]), w, b).view(*x.shape[:-1], w.shape[0])
        return self._conv(h, blk["conv2"], resid=x)

    def _note(self, name, t):
        if self.record:
            self.stages[name] = t

    def denormalize(self, latents: torch.Tensor) -> torch.Tensor:
        """(B, C, T, F) -> channels-last (B, 1, T, F, 64) bf16: x * std + mean with the ``(c f)`` statistics index c*F + f,
        each op rounded to bf16 as the reference's, the 8 channels zero-padded to the kernel's 64."""
        B, C, T, F = latents.shape
        x = latents.to(BF16)
        x = x * self.std.view(1, C, 1, F) + self.mean.view(1, C, 1, F)
        out = torch.zeros((B, 1, T, F, 64), dtype=BF16, device=x.device)
        out[..., :C] = x.permute(0, 2, 3, 1).unsqueeze(1)
        return out

    def __call__(self, latents: torch.Tensor) -> torch.Tensor:
        B, C, T, F = latents.shape
        if C != self.z_channels:
            raise ValueError(f"AudioDecoder: latents must be (B, {self.z_channels}, T, F), got {tuple(latents.shape)}")
        x = self.denormalize(latents)
        h = self._conv(x, self.conv_in)
        self._note("conv_in", h)
        for i, blk in enumerate(self.mid):
            h = self._block(h, blk)
            self._note(f"mid.{i}", h)
        for level in reversed(range(len(self.ch_mult))):
            st = self.up[level]
            for i, blk in enumerate(st["block"]):
                h = self._block(h, blk)
                self._note(f"up.{level}.{i}", h)
            if st["upsample"] is not None:
                h = h.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
                h = self._conv(h, st["upsample"])[:, :, 1:].contiguous()      # drop the first row: length 2n - 1 (upsample.py:61-78)
                self._note(f"up.{level}.upsample", h)
        h = ops.pixelnorm_act(h, PIXELNORM_EPS, True)
        h = self._conv(h, self.conv_out)                                       # (B, 1, 4T-3, 4F, out_ch)
        self._note("conv_out", h)
        return self._adjust(h[:, 0], max(T * LATENT_DOWNSAMPLE_FACTOR - (LATENT_DOWNSAMPLE_FACTOR - 1), 1),
                            self.mel_bins if self.mel_bins is not None else F)

    def _adjust(self, h: torch.Tensor, frames: int, bins: int) -> torch.Tensor:
        """Crop, then zero-pad (B, H, W, C) to (frames, bins); returns (B, C, frames, bins) (audio_vae.py:398-444)."""
        h = h[:, :frames, :bins, :self.out_ch]
        pt, pf = frames - h.shape[1], bins - h.shape[2]
        if pt > 0 or pf > 0:
            h = torch.nn.functional.pad(h, (0, 0, 0, max(pf, 0), 0, max(pt, 0)))
        return h.permute(0, 3, 1, 2).contiguous()


class Vocoder:
    """Mel spectrogram (B, 2, T, 64) (or mono (B, T, 64)) -> waveform (B, channels, T * prod(upsample_rates)) float32."""

    def __init__(self, weights: Dict[str, torch.Tensor], *, resblock_kernel_sizes: Sequence[int] = (3, 7, 11),
                 upsample_rates: Sequence[int] = (6, 5, 2, 2, 2), upsample_kernel_sizes: Sequence[int] = (16, 15, 8, 4, 4),
                 resblock_dilation_sizes: Sequence[Sequence[int]] = ((1, 3, 5), (1, 3, 5), (1, 3, 5)),
                 upsample_initial_channel: int = 1024, stereo: bool = True, output_sample_rate: int = AUDIO_SAMPLE_RATE):
        self.kernels, self.rates = tuple(resblock_kernel_sizes), tuple(upsample_rates)
        self.dilations = tuple(tuple(d) for d in resblock_dilation_sizes)
        self.stereo, self.output_sample_rate = stereo, output_sample_rate
        if not 2 <= len(self.kernels) <= 3:
            raise ValueError("Vocoder: the fused mean takes two or three res blocks per stage")
        W = {k: v.to(BF16) for k, v in weights.items()}

        def conv1d(name):          # (Cout, k, Cin) -> (Cout, k, 1, Cin)
            w = W[f"{name}.weight"]
            return w.reshape(w.shape[0], w.shape[1], 1, w.shape[2]).contiguous(), W[f"{name}.bias"].contiguous()

        self.conv_pre = conv1d("conv_pre")
        self.ups = [pack_conv_transpose(W[f"ups.{i}.weight"], W[f"ups.{i}.bias"], s) for i, s in enumerate(self.rates)]
        self.resblocks = []
        for j in range(len(self.rates) * len(self.kernels)):
            nd = len(self.dilations[j % len(self.kernels)])
            self.resblocks.append(([conv1d(f"resblocks.{j}.convs1.{i}") for i in range(nd)],
                                   [conv1d(f"resblocks.{j}.convs2.{i}") for i in range(nd)]))
        self.conv_post = conv1d("conv_post")
        self.slope = bf16_slope(LRELU_SLOPE)
        self.final_slope = bf16_slope(0.01)            # the leaky ReLU in front of conv_post is the default one (vocoder.py:133-135)
        self.stages = {}
        self.record = False

    @property
    def upsample_factor(self) -> int:
        f = 1
        for r in self.rates:
            f *= r
        return f

    @staticmethod
    def _conv(x, wb, dil=1, **kw):
        k = wb[0].shape[1]
        half = (k - 1) * dil // 2
        return ops.conv3d(x, wb[0], wb[1], False, ops.PAD_ZEROS, kernel=(k, 1), dilation=dil, pad=(half, (k - 1) * dil - half, 0, 0), **kw)

    def _resblock(self, x, lx, j, last_kw):
        """ResBlock1 (resnet.py:57-65) on x with leaky(x) = lx at hand; the last conv's epilogue takes ``last_kw``."""
        convs1, convs2 = self.resblocks[j]
        dil = self.dilations[j % len(self.kernels)]
        n = len(convs1)
        for i in range(n):
            _, lt = self._conv(lx, convs1[i], dil[i], leaky=self.slope, keep_out=False)
            if i + 1 < n:
                x, lx = self._conv(lt, convs2[i], resid=x, leaky=self.slope)
            else:
                return self._conv(lt, convs2[i], resid=x, **last_kw)

    def pack_mel(self, mel: torch.Tensor) -> torch.Tensor:
        """(B, 2, T, F) -> (B, 1, T, 1, 2F) bf16 with channel s*F + f (vocoder.py:101-113); mono (B, T, F) -> (B, 1, T, 1, F)."""
        if mel.dim() == 4:
            B, S, T, F = mel.shape
            mel = mel.permute(0, 2, 1, 3).reshape(B, T, S * F)
        B, T, C = mel.shape
        return mel.to(BF16).reshape(B, 1, T, 1, C).contiguous()

    def __call__(self, mel: torch.Tensor) -> torch.Tensor:
        x = self.pack_mel(mel)
        B = x.shape[0]
        nk = len(self.kernels)
        _, lx = self._conv(x, self.conv_pre, leaky=self.slope, keep_out=False)
        self._note("conv_pre.leaky", lx)
        for i, s in enumerate(self.rates):
            panel, bias, (pt, pb) = self.ups[i]
            u, lu = ops.conv3d(lx, panel, bias, False, ops.PAD_ZEROS, kernel=(panel.shape[1], 1), pad=(pt, pb, 0, 0), leaky=self.slope)
            T = u.shape[2] * s
            u, lu = u.view(B, 1, T, 1, -1), lu.view(B, 1, T, 1, -1)
            self._note(f"ups.{i}", u)
            outs = [self._resblock(u, lu, i * nk + k, {}) for k in range(nk - 1)]
            nxt = self.slope if i + 1 < len(self.rates) else self.final_slope
            x, lx = self._resblock(u, lu, i * nk + nk - 1, dict(mean_with=tuple(outs), leaky=nxt, keep_out=self.record))
            self._note(f"stage.{i}", x)
        wav = self._conv(lx, self.conv_post, tanh_out=True)                       # (B, 1, L, 1, channels) float32
        return wav[:, 0, :, 0].permute(0, 2, 1).contiguous()

    def _note(self, name, t):
        if self.record:
            self.stages[name] = t


def decode_audio(latents: torch.Tensor, decoder: AudioDecoder, vocoder: Vocoder) -> torch.Tensor:
    """Audio latents (B, 8, T, 16) (or (8, T, 16)) -> float32 waveform (channels, samples), samples = 240 * (4T - 3); a batch of
    more than one keeps its leading dimension (audio_vae.py:471-486)."""
    if latents.dim() == 3:
        latents = latents.unsqueeze(0)
    wav = vocoder(decoder(latents))
    return (wav[0] if wav.shape[0] == 1 else wav).float()
