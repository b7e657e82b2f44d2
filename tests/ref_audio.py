"""Float64 restatement of the audio decode (audio VAE decoder + HiFi-GAN vocoder) on torch.nn.functional, with a bf16-policy
twin that rounds exactly where ltxk_conv_taps_bf16 (include/ltxk.h) and the row kernels round, and the per-element bound the
tap convolution is held to.  Works on whatever device its inputs live on.

Layouts are the product's: Conv2d weights (Cout,kh,kw,Cin), Conv1d / ConvTranspose1d (Cout,k,Cin) (ConvTranspose1d: Wt[ci,co,j]
at w[co,j,ci]); activations channels-last.  ``policy=False``: nothing is rounded (the exact function of the bf16 weights and
inputs).  ``policy=True``: every rounding point of the device path, sums in float64 - the error a perfect accumulator would
leave, the yardstick of tests/test_audio_model_gpu.py."""
import math

import torch
import torch.nn.functional as F

import ref64 as R

F64 = torch.float64
U24 = R.U24


def _rbf64(x):
    """float64 -> nearest bf16 (ties to even), as float64, on x's device (ref64.rbf works on the host).  The float64 value is
    rounded directly: going through float32 first would round twice."""
    m, e = torch.frexp(x)                         # x = m * 2^e, 0.5 <= |m| < 1
    q = torch.round(m * 256.0) / 256.0            # 8 significant bits; torch.round is half-to-even
    return torch.where(torch.isfinite(x), torch.ldexp(q, e), x)


def _rnd(policy):
    return _rbf64 if policy else (lambda t: t)


# ------------------------------------------------------------------------------------------------ the tap convolution
def conv_taps(x, w, bias, dil=1, pad=(0, 0, 0, 0)):
    """ltxk_conv_taps_bf16's sum in float64: x (B,D,H,W,Cin), w (Cout,kh,kw,Cin), bias (Cout).  Returns (y, mag), both
    (B,D,H,W,Cout): y = sum x*w + bias, mag = sum |x*w|.  One matmul per tap over an explicitly zero-padded frame: no library
    convolution.  Frames (B*D of them) never see each other."""
    B, D, H, W, Cin = x.shape
    Cout, kh, kw, _ = w.shape
    pt, pb, pl, pr = pad
    assert pt + pb == (kh - 1) * dil and pl + pr == kw - 1
    xp = F.pad(x.to(F64).reshape(B * D, H, W, Cin), (0, 0, pl, pr, pt, pb))
    w64 = w.to(F64)
    y = torch.zeros((B * D * H * W, Cout), dtype=F64, device=x.device)
    mag = torch.zeros_like(y)
    for i in range(kh):
        for j in range(kw):
            s = xp[:, i * dil:i * dil + H, j:j + W].reshape(-1, Cin)
            wt = w64[:, i, j].t()
            y += s @ wt
            mag += s.abs() @ wt.abs()
    y = y + bias.to(F64)
    return y.reshape(B, D, H, W, Cout), mag.reshape(B, D, H, W, Cout)


def leaky(y, slope):
    return torch.maximum(y, y * slope)


def taps_exact(c, resid=None, mean_with=(), slope=None):
    """The exact (unrounded) values of the epilogue chain from c = conv + bias: (y, act or None)."""
    y = c if resid is None else c + resid.to(F64)
    if mean_with:
        for a in mean_with:
            y = y + a.to(F64)
        y = y / (len(mean_with) + 1)
    return y, (leaky(y, slope) if slope is not None else None)


def taps_policy(c, resid=None, mean_with=(), slope=None):
    """The same chain with the kernel's rounding points (include/ltxk.h, steps 1-5) on an exact accumulator."""
    y = _rbf64(c)
    if resid is not None:
        y = _rbf64(y + resid.to(F64))
    if mean_with:
        for a in mean_with:
            y = y + a.to(F64)
        y = _rbf64(y / (len(mean_with) + 1))
    return y, (torch.maximum(y, _rbf64(y * slope)) if slope is not None else None)


def _half_ulp(v):
    return 0.5 * R._ulp_dev(v)


def taps_bound(c, mag, K, resid=None, mean_with=(), slope=None):
    """(e_out, e_act): the most a correct kernel's bf16 ``out`` / ``act_out`` can be away from ``taps_exact``.

    The first two stages are ref64.conv3d_bound's terms (tests/test_conv3d_bound_gpu.py), K = kh*kw*Cin:
      acc   = K 2^-24 mag + 2^-24 (|c| + K 2^-24 mag)                  fp32 accumulation in any order + the fp32 bias add
      e1    = acc + 1/2 ulp_bf16(|c| + acc)                             y1 = bf16(acc + bias)
      e2    = e1 + 2^-24 (|c| + |r| + e1) + 1/2 ulp_bf16(|c + r| + ..)  y2 = bf16(y1 + resid)
    and every further rounding adds half a bf16 ulp of that intermediate (taken at its largest possible magnitude), every
    fp32 operation 2^-24 of its result's largest magnitude:
      e3    = (e2 + 2^-24 s1 + 2^-24 s2) / n + 2^-24 |v3| + 1/2 ulp_bf16(|v3| + ..)     v3 = (y2 + a1 [+ a2]) / n, s_i the partial sums
      e_act = max(e_out, slope e_out + 2^-24 slope |v| + 1/2 ulp_bf16(slope (|v| + e_out)))   max(y, bf16(y * slope)) is 1-Lipschitz in each branch
    The last rounding of ``out`` is taken at |v| + e as well (conv3d_bound takes it at the output itself; the same up to a binade edge)."""
    acc = K * U24 * mag
    e = acc + U24 * (c.abs() + acc)
    v = c
    e = e + _half_ulp(v.abs() + e)
    if resid is not None:
        r = resid.to(F64)
        e = e + U24 * (v.abs() + r.abs() + e)
        v = v + r
        e = e + _half_ulp(v.abs() + e)
    if mean_with:
        n = len(mean_with) + 1
        for a in mean_with:
            a = a.to(F64)
            e = e + U24 * (v.abs() + a.abs() + e)
            v = v + a
        v = v / n
        e = e / n
        e = e + U24 * (v.abs() + e)
        e = e + _half_ulp(v.abs() + e)
    e_act = None
    if slope is not None:
        t = slope * (v.abs() + e)
        e_act = torch.maximum(e, slope * e + U24 * t + _half_ulp(t))
    return e, e_act


def ulp_f32(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)


def tanh_excess_ulps(out_f32, c, mag, K):
    """The tanh form's figure: how far, in fp32 ulps of the result, out_f32 lies from tanh(c) beyond what the accumulation
    error alone explains (tanh is 1-Lipschitz: an argument off by ``acc`` moves the result by at most ``acc``).  What is left
    is the device tanhf's own error plus one fp32 rounding - not derivable on the host, so pinned (tests/golden/audio_pins.json)."""
    acc = K * U24 * mag
    acc = acc + U24 * (c.abs() + acc)
    t = torch.tanh(c)
    d = (out_f32.to(F64) - t).abs()
    return ((d - acc).clamp_min(0) / ulp_f32(t)).max()


# ------------------------------------------------------------------------------------------------ ConvTranspose1d
def conv_transpose1d(x, w, bias, stride):
    """F.conv_transpose1d in float64: x (B,T,Cin) channels-last, w (Cout,k,Cin), padding (k - stride) / 2 -> (B, T*stride, Cout)."""
    k = w.shape[1]
    wt = w.to(F64).permute(2, 0, 1)                                   # (Cin, Cout, k)
    y = F.conv_transpose1d(x.to(F64).transpose(1, 2), wt, bias.to(F64), stride=stride, padding=(k - stride) // 2)
    return y.transpose(1, 2)


def conv1d(x, w, bias, dil=1):
    """nn.Conv1d(padding = (k-1)*dil/2) in float64 through conv_taps: x (B,T,Cin), w (Cout,k,Cin) -> (B,T,Cout)."""
    k = w.shape[1]
    half = (k - 1) * dil // 2
    y, _ = conv_taps(x[:, None, :, None], w[:, :, None], bias, dil, (half, (k - 1) * dil - half, 0, 0))
    return y[:, 0, :, 0]


# ------------------------------------------------------------------------------------------------ the vocoder
VOC_KERNELS, VOC_RATES, VOC_UP_KERNELS = (3, 7, 11), (6, 5, 2, 2, 2), (16, 15, 8, 4, 4)
VOC_DILATIONS = ((1, 3, 5),) * 3


def make_vocoder_weights(seed=0, initial=1024, stereo=True, kernels=VOC_KERNELS, rates=VOC_RATES, up_kernels=VOC_UP_KERNELS,
                         dilations=VOC_DILATIONS, mel=64):
    """Random bf16 weights scaled by fan-in^-1/2, in the product's layout and key names."""
    g = torch.Generator().manual_seed(seed)
    W = {}

    def conv(name, cout, k, cin, fan=None):
        W[f"{name}.weight"] = (torch.randn(cout, k, cin, generator=g) * (fan or k * cin) ** -0.5).to(torch.bfloat16)
        W[f"{name}.bias"] = (0.1 * torch.randn(cout, generator=g)).to(torch.bfloat16)

    conv("conv_pre", initial, 7, mel * (2 if stereo else 1))
    j = 0
    for i, (s, k) in enumerate(zip(rates, up_kernels)):
        cin, cout = initial >> i, initial >> (i + 1)
        conv(f"ups.{i}", cout, k, cin, fan=cin * k / s)
        for kk, dd in zip(kernels, dilations):
            for d in range(len(dd)):
                conv(f"resblocks.{j}.convs1.{d}", cout, kk, cout)
                conv(f"resblocks.{j}.convs2.{d}", cout, kk, cout)
            j += 1
    conv("conv_post", 2 if stereo else 1, 7, initial >> len(rates))
    return W


def vocoder(mel, W, policy, slope=0.1, final_slope=0.01, kernels=VOC_KERNELS, rates=VOC_RATES, dilations=VOC_DILATIONS, stages=None):
    """vocoder.py in float64: mel (B,2,T,F) stereo or (B,T,F) mono -> (B, channels, T * prod(rates)).  ``policy``: round where the
    device path rounds (its fused order: the mean sums block 3, then 1, then 2).  ``stages``: a dict that receives the stage outputs."""
    rb = _rnd(policy)
    if mel.dim() == 4:
        B, S, T, Fb = mel.shape
        mel = mel.permute(0, 2, 1, 3).reshape(B, T, S * Fb)
    x = mel.to(F64)
    nk = len(kernels)

    def lk(t, s=slope):
        return torch.maximum(t, rb(t * s))

    def c1(t, name, d=1):
        return rb(conv1d(t, W[f"{name}.weight"], W[f"{name}.bias"], d))

    x = c1(x, "conv_pre")
    for i, s in enumerate(rates):
        u = rb(conv_transpose1d(lk(x), W[f"ups.{i}.weight"], W[f"ups.{i}.bias"], s))
        if stages is not None:
            stages[f"ups.{i}"] = u
        outs = []
        for k in range(nk):
            j = i * nk + k
            y = u
            for d, dil in enumerate(dilations[k]):
                t = c1(lk(y), f"resblocks.{j}.convs1.{d}", dil)
                t = c1(lk(t), f"resblocks.{j}.convs2.{d}")
                y = rb(t + y)
            outs.append(y)
        acc = outs[-1]
        for o in outs[:-1]:
            acc = acc + o
        x = rb(acc / nk)
        if stages is not None:
            stages[f"stage.{i}"] = x
    x = conv1d(lk(x, final_slope), W["conv_post.weight"], W["conv_post.bias"])
    return torch.tanh(x).transpose(1, 2)


# ------------------------------------------------------------------------------------------------ the audio decoder
def make_decoder_weights(seed=0, ch=128, ch_mult=(1, 2, 4), num_res_blocks=2, z=8, out_ch=2, latent_bins=16):
    g = torch.Generator().manual_seed(seed)
    W = {}

    def conv(name, cout, cin, k=3):
        W[f"{name}.conv.weight"] = (torch.randn(cout, k, k, cin, generator=g) * (k * k * cin) ** -0.5).to(torch.bfloat16)
        W[f"{name}.conv.bias"] = (0.1 * torch.randn(cout, generator=g)).to(torch.bfloat16)

    def block(name, cin, cout):
        conv(f"{name}.conv1", cout, cin)
        conv(f"{name}.conv2", cout, cout)
        if cin != cout:
            conv(f"{name}.nin_shortcut", cout, cin, 1)

    top = ch * ch_mult[-1]
    conv("conv_in", top, z)
    block("mid.block_1", top, top)
    block("mid.block_2", top, top)
    cin = top
    for level in reversed(range(len(ch_mult))):
        cout = ch * ch_mult[level]
        for i in range(num_res_blocks + 1):
            block(f"up.{level}.block.{i}", cin, cout)
            cin = cout
        if level != 0:
            conv(f"up.{level}.upsample.conv", cin, cin)
    conv("conv_out", out_ch, cin)
    W["per_channel_statistics._mean_of_means"] = (0.2 * torch.randn(z * latent_bins, generator=g)).to(torch.bfloat16)
    W["per_channel_statistics._std_of_means"] = (1.0 + 0.2 * torch.rand(z * latent_bins, generator=g)).to(torch.bfloat16)
    return W


def causal_conv2d(x, w, b):
    """CausalConv2d (causal_conv_2d.py) on (B,H,W,C): 3x3 pads (2,0,1,1), 1x1 none."""
    k = w.shape[1]
    pad = ((k - 1), 0, (k - 1) // 2, (k - 1) - (k - 1) // 2)
    return conv_taps(x[:, None], w, b, 1, pad)[0][:, 0]


rbf = _rbf64


def pixelnorm_silu(x, policy, eps=1e-6):
    """PixelNorm + SiLU with the rounding points of ltxk_pixelnorm_act (ref64.pixelnorm_act) under the policy, exact otherwise."""
    if policy:
        y, _, _ = R.pixelnorm_act(x.reshape(-1, x.shape[-1]), eps, silu_on=True)
        return y.reshape(x.shape).to(x.device)
    n = x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    return n / (1.0 + torch.exp(-n))


def upsample_frames(T):
    """Frames after one causal 2x upsample: repeat, causal conv (same length), drop the first row."""
    return 2 * T - 1


def adjust_output(h, frames, bins, out_ch):
    """audio_vae.py:398-444 on (B,H,W,C): crop, zero-pad, -> (B,C,frames,bins)."""
    h = h[:, :frames, :bins, :out_ch]
    pt, pf = frames - h.shape[1], bins - h.shape[2]
    if pt > 0 or pf > 0:
        h = F.pad(h, (0, 0, 0, max(pf, 0), 0, max(pt, 0)))
    return h.permute(0, 3, 1, 2)


def denormalize(latents, W, policy):
    """(B,C,T,F) -> (B,T,F,C): x * std + mean, statistics index c*F + f (the reference's "b c t f -> b t (c f)")."""
    rb = _rnd(policy)
    B, C, T, Fb = latents.shape
    std = W["per_channel_statistics._std_of_means"].to(F64).to(latents.device).view(1, C, 1, Fb)
    mean = W["per_channel_statistics._mean_of_means"].to(F64).to(latents.device).view(1, C, 1, Fb)
    return rb(rb(latents.to(F64) * std) + mean).permute(0, 2, 3, 1)


def audio_decoder(latents, W, policy, ch=128, ch_mult=(1, 2, 4), num_res_blocks=2, out_ch=2, mel_bins=64, stages=None):
    """AudioDecoder.__call__ in float64: latents (B,8,T,16) bf16 -> (B,2,4T-3,mel_bins)."""
    rb = _rnd(policy)
    B, C, T, Fb = latents.shape

    def conv(t, name):
        return rb(causal_conv2d(t, W[f"{name}.conv.weight"], W[f"{name}.conv.bias"]))

    def block(t, name):
        h = conv(pixelnorm_silu(t, policy), f"{name}.conv1")
        h = conv(pixelnorm_silu(h, policy), f"{name}.conv2")
        if f"{name}.nin_shortcut.conv.weight" in W:
            t = conv(t, f"{name}.nin_shortcut")
        return rb(t + h)

    def note(name, t):
        if stages is not None:
            stages[name] = t

    h = conv(denormalize(latents, W, policy), "conv_in")
    note("conv_in", h)
    for i in (1, 2):
        h = block(h, f"mid.block_{i}")
        note(f"mid.{i - 1}", h)
    for level in reversed(range(len(ch_mult))):
        for i in range(num_res_blocks + 1):
            h = block(h, f"up.{level}.block.{i}")
            note(f"up.{level}.{i}", h)
        if level != 0:
            h = h.repeat_interleave(2, 1).repeat_interleave(2, 2)
            h = conv(h, f"up.{level}.upsample.conv")[:, 1:]
            note(f"up.{level}.upsample", h)
    h = conv(pixelnorm_silu(h, policy), "conv_out")
    note("conv_out", h)
    return adjust_output(h, max(4 * T - 3, 1), mel_bins if mel_bins is not None else Fb, out_ch)


def rel_err(got, ref):
    return float((got.to(F64) - ref).norm() / ref.norm().clamp_min(1e-300))
