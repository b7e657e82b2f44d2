"""Float64 restatements of the row, elementwise and VAE glue kernels of include/ltxk.h, for the edge-shape tests
(tests/test_rowops_gpu.py, tests/test_vae_glue_gpu.py; checked against the oracle in tests/test_ref64_cpu.py).

Every function computes in float64 and rounds to bf16 only where the kernel and the reference model materialise a bf16
array (the kernel comments and the oracle/ function of the same op name those points).  The rounding is done here in
float64 (``rbf``), never through float32, so a reference value is the correctly rounded bf16 of the exact expression.
Scalars the kernels receive as fp32 are passed in already rounded to fp32 (``f32``).

``assert_bf16_close`` is the comparator: bf16 ulps measured at max(|ref|, mag) with an absolute floor of 2^-126 (a
kernel that flushes a subnormal result to zero is not wrong); no element more than ``max_ulps`` away and at most
``max_frac`` of the elements off at all.  NaN where the reference is finite (an untouched sentinel) counts as infinitely
far.

conv3d / conv3d_bound and attention / attention_bound are of another kind: they round nothing, run on the device their
inputs live on, and come with an element-wise bound derived from the kernel's rounding points (tests/test_conv3d_bound_gpu.py,
tests/test_attn_bound_gpu.py)."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

Tensor = torch.Tensor
F64 = torch.float64
BF = torch.bfloat16
ULP_FLOOR = 2.0 ** -126


def f64(x) -> Tensor:
    if not isinstance(x, torch.Tensor):
        return torch.as_tensor(x, dtype=F64)
    return x.detach().cpu().to(F64)


def f32(v: float) -> float:
    """A host scalar as the kernel receives it (fp32)."""
    return float(np.float32(v))


def ulp_bf16(m: Tensor) -> Tensor:
    """bf16 ulp at magnitude m (the spacing of the binade m lies in), never below ULP_FLOOR."""
    m = f64(m).abs().clamp_min(ULP_FLOOR)
    m = torch.where(torch.isfinite(m), m, torch.full_like(m, 2.0 ** 127))
    e = torch.floor(torch.log2(m))
    e = torch.where(torch.exp2(e) > m, e - 1, e)          # log2 of a value just below a power of two may round up
    return torch.exp2(e - 7).clamp_min(ULP_FLOOR)


def rbf(x) -> Tensor:
    """float64 -> nearest bf16 (ties to even), returned as float64.  Overflow -> +-inf; NaN/inf pass through."""
    x = f64(x)
    a = x.abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -133)))
    e = torch.where(torch.exp2(e) > a.clamp_min(2.0 ** -133), e - 1, e)
    q = torch.exp2(e.clamp_min(-126) - 7)                  # spacing; subnormal bf16 below 2^-126
    r = torch.round(x / q) * q                             # torch.round: half to even; x/q is exact (power-of-two scale)
    r = torch.where(r.abs() > 3.3895313892515355e38, torch.sign(x) * math.inf, r)
    return torch.where(torch.isfinite(x), r, x)


def silu(x: Tensor) -> Tensor:
    """float64 silu of bf16 inputs, one rounding (adaln.py:45, upsampler.py:160-174)."""
    x = f64(x)
    return rbf(x / (1.0 + torch.exp(-x)))


def bf16_stats(got, ref, mag=None) -> Tuple[float, float]:
    """(max ulp error, fraction of elements off at all) of got against ref, ulp at max(|ref|, mag)."""
    g, r = f64(got).flatten(), f64(ref).flatten()
    m = r.abs() if mag is None else torch.maximum(r.abs(), f64(mag).flatten().abs())
    d = (g - r).abs()
    same = (g == r) | (torch.isnan(g) & torch.isnan(r))
    d = torch.where(same, torch.zeros_like(d), d)
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    u = d / ulp_bf16(m)
    return float(u.max()) if u.numel() else 0.0, float((d > 0).double().mean()) if d.numel() else 0.0


def assert_bf16_close(got, ref, *, max_ulps: float = 1, max_frac: float = 0.0, mag=None, what: str = "") -> Tuple[float, float]:
    ulps, frac = bf16_stats(got, ref, mag)
    assert ulps <= max_ulps, f"{what}: an element is {ulps:.3g} bf16 ulps off (allowed {max_ulps})"
    assert frac <= max_frac, f"{what}: {frac:.3e} of the elements differ (allowed {max_frac:.3e})"
    return ulps, frac


# --------------------------------------------------------------------------------------------------- DiT step rows
def norm_modulate(x, eps: float, scale=None, shift=None, *, layernorm: bool = False, one_plus: bool = False):
    """rms_norm (weight 1) or LayerNorm(affine=False) + modulation: n = bf16(norm), one_p = bf16(1+scale) (or scale as
    given when it already holds bf16(1+scale)), out = bf16(bf16(n*one_p) + shift).  Returns (out, mag) with mag the
    magnitude of the terms of the final add (it can cancel)."""
    x = f64(x)
    if layernorm:
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        pre = (x - mu) / torch.sqrt(var + eps)
    else:
        pre = x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    if scale is None:
        return rbf(pre), None
    n = rbf(pre)
    one_p = f64(scale) if one_plus else rbf(1.0 + f64(scale))
    prod = rbf(n * one_p)
    return rbf(prod + f64(shift)), (n * one_p).abs() + f64(shift).abs()


def qknorm_rope(x, weight, cos, sin, T: int, H: int, eps: float):
    """q/k RMSNorm over each D-wide segment (learned weight, one rounding) + SPLIT rope (fp32 math, one rounding).
    x (M, nseg*D); weight (nseg, D); cos/sin (H, T, 64) or None; row m is token m % T.  Returns (out, mag): mag the
    terms of the rotation (it can cancel a rounding of the normalised pair), None without rope."""
    x = f64(x)
    M = x.shape[0]
    nseg, D = weight.shape
    seg = x.reshape(M, nseg, D)
    rstd = 1.0 / torch.sqrt((seg * seg).mean(-1, keepdim=True) + eps)
    y = rbf(seg * rstd * f64(weight)[None])
    if cos is None:
        return y.reshape(M, nseg * D), None
    yh = y.reshape(M, nseg, H, 2, 64)
    t = torch.arange(M) % T
    c = f64(cos)[:, t].permute(1, 0, 2)[:, None]          # (M,1,H,64)
    s = f64(sin)[:, t].permute(1, 0, 2)[:, None]
    x1, x2 = yh[..., 0, :], yh[..., 1, :]
    o = torch.stack([x1 * c - s * x2, x2 * c + s * x1], dim=-2)
    mag = torch.stack([(x1 * c).abs() + (s * x2).abs(), (x2 * c).abs() + (s * x1).abs()], dim=-2)
    return rbf(o).reshape(M, nseg * D), mag.reshape(M, nseg * D)


def rope_table(positions, freq, H: int, dim: int, max_pos: Sequence[float]):
    """SPLIT rope table, middle-of-interval positions: positions (3,T,2), freq (n_freq), max_pos 3 scalars (fp32).
    Returns cos, sin, ang, frac_freq (all (H,T,dim/2/H) float64): ang the exact angle of the fp32 inputs and
    frac_freq = |2*frac*freq|, the size of the term whose fp32 rounding the angle error scales with."""
    pos, fr = f64(positions), f64(freq)
    T, nf = pos.shape[1], fr.numel()
    half = dim // 2
    pad = half - 3 * nf
    mid = (pos[..., 0] + pos[..., 1]) / 2.0                                     # (3,T)
    frac = mid / f64([f32(m) for m in max_pos])[:, None]
    ang = ((frac * 2.0 - 1.0).T[:, None, :] * fr[None, :, None]).reshape(T, 3 * nf)   # idx-major, axis-minor
    big = ((frac * 2.0).abs().T[:, None, :] * fr.abs()[None, :, None]).reshape(T, 3 * nf)
    z = torch.zeros(T, pad, dtype=F64)
    ang = torch.cat([z, ang], 1)
    big = torch.cat([z, big], 1)
    c = torch.cat([torch.ones(T, pad, dtype=F64), torch.cos(ang[:, pad:])], 1)
    s = torch.cat([z, torch.sin(ang[:, pad:])], 1)
    per = half // H
    r = lambda a: a.reshape(T, H, per).permute(1, 0, 2).contiguous()
    return r(c), r(s), r(ang), r(big)


def timestep_embed(t, dim: int, mult: float):
    """[cos | sin](bf16(t*mult) * exp(-ln(1e4) i/half)), one rounding each.  Returns (out (U,dim), ang (U,dim)) with
    ang the exact argument of each output."""
    tt = rbf(f64(t).flatten() * f32(mult))
    half = dim // 2
    fr = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F64) / half)
    ang = tt[:, None] * fr[None]
    return torch.cat([rbf(torch.cos(ang)), rbf(torch.sin(ang))], 1), torch.cat([ang, ang], 1)


def ada_combine(table, ada, one_plus_mask: int = 0):
    """table (L,K,D), ada (U,K*D) -> (L,U,K,D): bf16(table + ada), then bf16(1 + that) for the k in one_plus_mask."""
    tb = f64(table)
    L, K, D = tb.shape
    a = f64(ada).reshape(-1, K, D)
    v = rbf(tb[:, None] + a[None])
    bits = torch.tensor([(one_plus_mask >> k) & 1 for k in range(K)], dtype=torch.bool)[None, None, :, None]
    return torch.where(bits, rbf(1.0 + v), v)


def cfg_euler_step(v_pos, v_neg, latent, sigma: float, sigma_next: float, cfg: float = 1.0, clean=None, mask=None,
                   bf16_euler: bool = False):
    """The step tail: CFG combine (per-op bf16) + token -> latent transpose + x0 = bf16(x - sigma*v) + mask blend +
    Euler (fp32 formula with one rounding, or op by op in bf16).  v_* (B,S,C) tokens, latent (B,C,S), clean (B,C,S),
    mask (B,S).  Returns (out (B,C,S), mag): mag bounds every intermediate the output inherits a rounding from."""
    vp = f64(v_pos).transpose(1, 2)
    x = f64(latent)
    v = vp
    mag = vp.abs()
    if v_neg is not None:
        vn = f64(v_neg).transpose(1, 2)
        d = rbf(vp - vn)
        v = rbf(vp + rbf((cfg - 1.0) * d))
        mag = torch.maximum(vp.abs(), ((cfg - 1.0) * d).abs())
    x0 = rbf(x - sigma * v)
    mag = torch.maximum(torch.maximum(mag, x.abs()), (sigma * v).abs())
    if mask is not None:
        m = f64(mask)[:, None, :]
        x0 = rbf(rbf(x0 * m) + rbf(f64(clean) * rbf(1.0 - m)))
        mag = torch.maximum(mag, f64(clean).abs())
    if bf16_euler:
        out = rbf(x0 + rbf(rbf(sigma_next * rbf(x - x0)) / sigma))
    elif sigma_next > 0:
        out = rbf(x0 + sigma_next * (x - x0) / sigma)
    else:
        out = x0
    return out, mag


def euler_step(latent, denoised, sigma: float, sigma_next: float):
    """bf16(x0 + sigma_next*(x - x0)/sigma), one rounding.  Returns (out, mag of the final add's terms)."""
    x, d = f64(latent), f64(denoised)
    step = sigma_next * (x - d) / sigma
    return rbf(d + step), d.abs() + step.abs()


# ------------------------------------------------------------------------------------------------------- VAE glue
def groupnorm_act(x, gamma, beta, G: int, eps: float, resid=None, apply_silu: bool = False):
    """GroupNorm over (voxels, C/G) per (batch, group), float64 mean and centred variance, then
    bf16((x-mean)/sqrt(var+eps)*gamma+beta) [+ resid -> bf16] [silu -> bf16].  x (B,V,C) channels-last.
    Returns (out, mag): mag = |norm*gamma| + |beta| (the affine add can cancel) plus |gamma*mean/sd|*2^-12 (the fp32
    statistics of a kernel are good to far less than that: an allowance of ~2^-19 |mean| per ulp near zero), plus
    |resid| with a residual."""
    x = f64(x)
    B, V, C = x.shape
    xg = x.reshape(B, V, G, C // G)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    sd = torch.sqrt(var + eps)
    y = ((xg - mean) / sd).reshape(B, V, C)
    gm = f64(gamma)
    mag = (y * gm).abs() + f64(beta).abs() + ((mean / sd).expand_as(xg).reshape(B, V, C) * gm).abs() * 2.0 ** -12
    y = rbf(y * gm + f64(beta))
    if resid is not None:
        mag = torch.maximum(mag, y.abs() + f64(resid).abs())
        y = rbf(y + f64(resid))
    if apply_silu:                                 # silu(y) ~ y/2 near 0: a flip of y is up to two ulps of the output
        y = silu(y)
    return y, mag


def latent_denorm_cl(latent, mean, std, noise=None, noise_scale: float = 0.0):
    """(B,C,S) -> (B,S,C): bf16(x*std + mean) in one rounding; with noise the blend bf16(bf16(noise*s) + bf16((1-s)*x))
    first, 1-s formed in fp32 as the kernel (and the reference's scalar arithmetic) forms it.  Returns (out, mag) with
    mag = |x*std| + |mean| (the add can cancel a rounding of the blend)."""
    x = f64(latent)
    if noise is not None:
        s = f32(noise_scale)
        oms = f32(1.0 - s)
        x = rbf(rbf(f64(noise) * s) + rbf(oms * x))
    xs, mu = x * f64(std)[None, :, None], f64(mean)[None, :, None]
    return rbf(xs + mu).transpose(1, 2).contiguous(), (xs.abs() + mu.abs()).transpose(1, 2).contiguous()


def latent_norm_cf(x, mean, std):
    """(B,S,C) -> (B,C,S): bf16((x - mean)/std), one rounding."""
    y = (f64(x) - f64(mean)) / f64(std)
    return rbf(y).transpose(1, 2).contiguous()


def tile_blend(tiles, F: int, H: int, W: int):
    """Tiled-decode blend in float64: tiles = [(tile (B,C,Tt,Th,Tw), (at,ah,aw), mt, mh, mw, (t0,h0,w0))];
    out = bf16(sum tile*m / max(sum m, 1e-8)) with m = mt[t]*mh[y]*mw[x] over the used box of each tile."""
    B, C = tiles[0][0].shape[:2]
    acc = torch.zeros(B, C, F, H, W, dtype=F64)
    ws = torch.zeros(B, 1, F, H, W, dtype=F64)
    for tile, (at, ah, aw), mt, mh, mw, (t0, h0, w0) in tiles:
        m = f64(mt)[:at, None, None] * f64(mh)[None, :ah, None] * f64(mw)[None, None, :aw]
        acc[:, :, t0:t0 + at, h0:h0 + ah, w0:w0 + aw] += f64(tile)[:, :, :at, :ah, :aw] * m
        ws[:, :, t0:t0 + at, h0:h0 + ah, w0:w0 + aw] += m
    return rbf(acc / ws.clamp_min(1e-8))


def to_uint8(video) -> Tensor:
    """(B,C,F,H,W) bf16 video in [-1,1] -> (B,F,H,W,C) uint8: u = bf16(bf16(x+1)/2) clamped to [0,1],
    trunc(bf16(u*255))."""
    v = f64(video).permute(0, 2, 3, 4, 1)
    u = rbf(rbf(v + 1.0) / 2.0).clamp(0.0, 1.0)
    return torch.trunc(rbf(u * 255.0)).to(torch.uint8)


def patchify(video, P: int, Cpad: Optional[int] = None) -> Tensor:
    """(B,C,D,H,W) -> (B,D,H/P,W/P,Cpad) channels-last, channel c*P*P + p_w*P + p_h holding video[b,c,d,h*P+p_h,
    w*P+p_w] (ops.py:9-44, width before height); channels past C*P*P zero.  A gather over explicit indices."""
    v = torch.as_tensor(video)
    B, C, D, H, W = v.shape
    Cpad = C * P * P if Cpad is None else Cpad
    ch = torch.arange(C * P * P)
    c, pw, ph = ch // (P * P), (ch // P) % P, ch % P
    hh = (torch.arange(H // P)[:, None] * P + ph[None, :])                     # (Hp, CPP)
    ww = (torch.arange(W // P)[:, None] * P + pw[None, :])                     # (Wp, CPP)
    g = v[:, c[None, None, :], :, hh[:, None, :], ww[None, :, :]]             # (Hp,Wp,CPP,B,D)... advanced-index order
    g = g.permute(3, 4, 0, 1, 2)                                               # (B,D,Hp,Wp,CPP)
    out = torch.zeros(B, D, H // P, W // P, Cpad, dtype=v.dtype)
    out[..., :C * P * P] = g
    return out


def unpatchify(x, C: int, P: int) -> Tensor:
    """(B,D,H,W,C*P*P) channels-last -> (B,C,D,H*P,W*P): out[b,c,d,y,x] = x[b,d,y//P,x//P, c*P*P + (x%P)*P + y%P]."""
    x = torch.as_tensor(x)
    B, D, H, W, _ = x.shape
    yo, xo = torch.arange(H * P), torch.arange(W * P)
    c = torch.arange(C)
    ch = c[:, None, None] * P * P + (xo % P)[None, None, :] * P + (yo % P)[None, :, None]   # (C,Ho,Wo)
    g = x[:, :, (yo // P)[None, :, None], (xo // P)[None, None, :], ch]                  # (B,D,C,Ho,Wo)
    return g.permute(0, 2, 1, 3, 4).contiguous()


# ------------------------------------------------------------------------------------- conv3d (implicit GEMM) + PixelNorm
U24 = 2.0 ** -24                                      # fp32 unit roundoff


def _ulp_dev(x: Tensor) -> Tensor:
    """bf16 ulp of |x| (float64, on x's device), floored at the smallest normal - test_gemm_splitk_gpu.py's ``_ulp``."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def conv3d_halo(x: Tensor, causal: int, pad_mode: int, taps_d: int = 3) -> Tensor:
    """The halo of ltxk_conv3d_k3_bf16 (include/ltxk.h; convolution.py:120-157) materialised: x (B,D,H,W,C) ->
    (B,D+2,H+2,W+2,C), or (B,D,H+2,W+2,C) for the per-frame kernel (taps_d = 1: no temporal halo).
    Temporal: causal = 1 the first frame twice in front; 0 the first frame in front and the last behind; 2 zeros.
    Spatial: pad_mode 0 zeros; 1 reflect without the edge sample (row 1 in front, row H-2 behind)."""
    if taps_d == 3:
        first, last = x[:, :1], x[:, -1:]
        if causal == 1:
            x = torch.cat([first, first, x], 1)
        elif causal == 0:
            x = torch.cat([first, x, last], 1)
        else:
            z = torch.zeros_like(first)
            x = torch.cat([z, x, z], 1)
    if pad_mode == 1:
        x = torch.cat([x[:, :, 1:2], x, x[:, :, -2:-1]], 2)
        x = torch.cat([x[:, :, :, 1:2], x, x[:, :, :, -2:-1]], 3)
    else:
        zh = torch.zeros_like(x[:, :, :1])
        x = torch.cat([zh, x, zh], 2)
        zw = torch.zeros_like(x[:, :, :, :1])
        x = torch.cat([zw, x, zw], 3)
    return x


def conv3d(x: Tensor, w: Tensor, bias: Tensor, causal: int, pad_mode: int, taps_d: int = 3, resid: Optional[Tensor] = None):
    """ltxk_conv3d_k3_bf16 in float64, on the device its inputs live on: x (B,D,H,W,Cin) channels-last bf16, w
    (Cout,3,3,3,Cin) - or (Cout,3,3,Cin) with taps_d = 1 -, bias (Cout), resid (B,D,H,W,Cout) or None.
    Returns (y, mag), both (B,D,H,W,Cout) float64: y = sum x*w + bias (+ resid), exact up to float64 roundoff (products
    of bf16 values are exact, the sums carry ~2^-53), mag = sum |x*w| over the same taps.  Nothing is rounded to bf16.
    The halo is built explicitly (conv3d_halo) and every tap is one matmul of a shifted slice: no library convolution."""
    B, D, H, W, Cin = x.shape
    Cout = w.shape[0]
    xp = conv3d_halo(x.to(F64), int(causal), int(pad_mode), taps_d)
    w64 = w.to(F64).reshape(Cout, 3 if taps_d == 3 else 1, 3, 3, Cin)
    y = torch.zeros((B * D * H * W, Cout), dtype=F64, device=x.device)
    mag = torch.zeros_like(y)
    for kd in range(w64.shape[1]):
        for kh in range(3):
            for kw in range(3):
                s = xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, Cin)
                wt = w64[:, kd, kh, kw].t()
                y += s @ wt
                mag += s.abs() @ wt.abs()
    y = (y + bias.to(F64)).reshape(B, D, H, W, Cout)
    if resid is not None:
        y = y + resid.to(F64)
    return y, mag.reshape(B, D, H, W, Cout)


def conv3d_bound(out: Tensor, y: Tensor, mag: Tensor, K: int, resid: Optional[Tensor] = None):
    """(d, bound), element-wise on the inputs' device: the distance of a kernel's bf16 output from ``conv3d``'s y and
    the most a correct implicit GEMM with fp32 accumulation can be away (test_gemm_splitk_gpu.py's rule, K = taps*Cin):
      |out - y| <= 1/2 ulp_bf16(out) + K 2^-24 mag + 2^-24 (|y| + K 2^-24 mag)
    - one bf16 rounding, the fp32 accumulation in ANY order (tap order, the kw kernel's order, K slices and their fp32
    or float64 sum), the fp32 bias add.  With a residual (y includes it) the output is bf16(bf16(conv + bias) + resid),
    two roundings and one fp32 add: that file's epi == 4 form."""
    o = out.to(F64)
    acc = K * U24 * mag
    if resid is None:
        return (o - y).abs(), 0.5 * _ulp_dev(o) + acc + U24 * (y.abs() + acc)
    r = resid.to(F64)
    c = y - r
    ec = acc + U24 * (c.abs() + acc)
    e1 = 0.5 * _ulp_dev(c.abs() + ec) + ec
    return (o - y).abs(), 0.5 * _ulp_dev(o) + U24 * (r.abs() + c.abs() + e1) + e1


def near_bf16_midpoint(v: Tensor, rel: float = 2.0 ** -18) -> Tensor:
    """True where the float64 value v lies within rel*|v| of the midpoint of two neighbouring bf16 values: a rounding
    that a computation carrying a relative error up to rel may take the other way."""
    v = f64(v)
    q = ulp_bf16(v)
    mid = (torch.floor(v / q) + 0.5) * q
    return (v - mid).abs() <= rel * v.abs()


def pixelnorm_act(x, eps: float, scale=None, shift=None, rows_per_batch: int = 0, silu_on: bool = False):
    """ltxk_pixelnorm_act, the rounding chain of vae_ops.hip's header (oracle/vae.py::pixel_norm, _mod, silu):
    q = bf16(x^2), m = bf16(mean_c q), e = bf16(m + eps), s = bf16(sqrt e), y = bf16(x / s); then
    bf16(bf16(y * bf16(1 + scale)) + shift) with row v using scale/shift row v // rows_per_batch; then bf16(silu).
    x (V,C); scale/shift (B,C) or None.  Returns (out, mag, exempt): mag the terms of the modulation's add (None
    without it), exempt (V) bool - the rows whose mean q, m + eps or sqrt(e) lies within relative 2^-18 of a bf16
    rounding midpoint, where an fp32 kernel may round the row statistic the other way and move the whole row."""
    x = f64(x)
    V, C = x.shape
    mq = rbf(x * x).mean(-1, keepdim=True)
    m = rbf(mq)
    me = m + eps
    e = rbf(me)
    rt = torch.sqrt(e)
    s = rbf(rt)
    exempt = (near_bf16_midpoint(mq) | near_bf16_midpoint(me) | near_bf16_midpoint(rt)).reshape(V)
    y = rbf(x / s)
    mag = None
    if scale is not None:
        b = torch.arange(V) // rows_per_batch
        one_p = rbf(1.0 + f64(scale))[b]
        sh = f64(shift)[b]
        mag = (y * one_p).abs() + sh.abs()
        y = rbf(rbf(y * one_p) + sh)
    if silu_on:
        y = silu(y)
    return y, mag, exempt


def pixelnorm_rows(C: int) -> int:
    """V of the ltxk_pixelnorm_act edge case for C channels: 2*R*k + 1 >= 257 rows, R = 4 * (64/LPR) rows per workgroup
    (LPR = min(C/8, 64) lanes per row): whole workgroups plus a lone row in the last one."""
    R = 4 * (64 // min(C // 8, 64))
    k = -(-256 // (2 * R))
    return 2 * R * k + 1


PIXELNORM_RPB = 129           # rows of batch 0: a multiple of no rows-per-wave (8, 4, 2), so one wave holds both batches
PIXELNORM_SEED = 1            # chosen on the reference alone: no row of any C is exempt with it (0 exempts one row at C = 1024, 2048)


def pixelnorm_inputs(C: int):
    """The inputs test_vae_glue_gpu.py feeds ltxk_pixelnorm_act at C channels (test_ref64_cpu.py asserts that at most 1 %
    of their rows are exempt): x (V,C) randn*3 with row 5 all zero (eps alone under the root) and row 7 constant, two
    batches' scale and shift (2,C)."""
    g = torch.Generator().manual_seed(PIXELNORM_SEED * 7919 + C)
    V = pixelnorm_rows(C)
    x = torch.randn(V, C, generator=g) * 3
    x[5] = 0.0
    x[7] = 1.5
    scale = 0.5 * torch.randn(2, C, generator=g)
    shift = torch.randn(2, C, generator=g)
    return x.to(BF), scale.to(BF), shift.to(BF)


def assert_rows_close(got, ref, exempt, *, max_ulps: float, max_frac: float, mag=None, what: str = "") -> Tuple[float, float]:
    """assert_bf16_close for (V,C) rows of which some are ``exempt`` (pixelnorm_act): every row counts towards max_ulps,
    only the others towards max_frac.  Returns (max ulps over all rows, fraction off among the non-exempt rows)."""
    ulps, _ = bf16_stats(got, ref, mag)
    keep = ~exempt
    _, frac = bf16_stats(f64(got)[keep], f64(ref)[keep], None if mag is None else f64(mag)[keep])
    assert ulps <= max_ulps, f"{what}: an element is {ulps:.3g} bf16 ulps off (allowed {max_ulps})"
    assert frac <= max_frac, f"{what}: {frac:.3e} of the elements of non-exempt rows differ (allowed {max_frac:.3e})"
    return ulps, frac


# ------------------------------------------------------------------------------------------ flash attention (dh = 128)
FA_DH = 128
LOG2E_F32 = 1.4426950408889634
ATTN_FAMILIES = ("flat", "peaked", "spiked")


def attn_c(scale: float) -> float:
    """The kernel's exponent constant fp32(fp32(scale) * fp32(log2 e)), as oracle.dit.sdpa builds it."""
    return float(np.float32(np.float32(scale) * np.float32(LOG2E_F32)))


def _heads(t: Tensor, H: int) -> Tensor:
    B, T, _ = t.shape
    return t.to(F64).reshape(B, T, H, FA_DH).transpose(1, 2)               # (B,H,T,128)


def attention_probs(q: Tensor, k: Tensor, H: int, scale: float):
    """(P, x, smag), each (B,H,Tq,Tk) float64 on the inputs' device: the exact softmax weights of ``attention``, the
    exponents x = c * q.k^T in the exp2 domain and smag = |q|.|k|^T."""
    qh, kh = _heads(q, H), _heads(k, H)
    x = attn_c(scale) * (qh @ kh.transpose(-1, -2))                       # products of bf16 values, sums of 128: exact in float64
    smag = qh.abs() @ kh.abs().transpose(-1, -2)
    p = torch.exp2(x - x.amax(-1, keepdim=True))
    return p / p.sum(-1, keepdim=True), x, smag


def attention(q: Tensor, k: Tensor, v: Tensor, H: int, scale: float):
    """ltxk_flash_attn in float64, on the device its inputs live on: q (B,Tq,H*128), k, v (B,Tk,H*128) bf16.  Per head,
    with c = attn_c(scale): s = q.k^T (exact), x = c*s, P = 2^(x - rowmax) / rowsum, y = P v.  Returns (y, A, dx), each
    (B,Tq,H*128) float64: y the exact result (nothing rounded), A = P |v|, and dx (per row and head, broadcast over the
    channels) the most the EXPONENT of one key can be off in a kernel that forms s in fp32 and x - M with one fma:
        dx = max_k(c * 128 * 2^-24 * smag) + 2^-24 * (2 max_k |x| + 8)
    - fp32 accumulation of 128 products in any order; the fma's rounding of a value no larger than |x| + |M| with the
    integer offset M within 7 of the row max (FA_DEFER = 6 and a ceil)."""
    B, Tq, D = q.shape
    c = attn_c(scale)
    p, x, smag = attention_probs(q, k, H, scale)
    vh = _heads(v, H)
    y = p @ vh
    A = p @ vh.abs()
    dx = (c * FA_DH * U24 * smag).amax(-1, keepdim=True) + U24 * (2.0 * x.abs().amax(-1, keepdim=True) + 8.0)
    back = lambda t: t.transpose(1, 2).reshape(B, Tq, D)
    return back(y), back(A), back(dx.expand(B, H, Tq, FA_DH))


def attention_bound(out: Tensor, y: Tensor, A: Tensor, dx: Tensor, Tk: int):
    """(d, bound), element-wise on the inputs' device: the distance of a kernel's bf16 output from ``attention``'s y and
    the most a correct kernel with the rounding points of include/ltxk.h can be away, whatever its tiling, deferral
    history, key split and summation order:
        e1    = 2^-22 + ln2 * dx * 1.001 + Tk * 2^-24
        e     = 2^-8 + e1
        bound = 1/2 ulp_bf16(out) + (e*A + e1*|y|) / (1 - e1) + 2^-22 |y| + 2^-120
    e1 is the relative error of one un-rounded P: v_exp_f32 (1 ulp), the exponent error dx, and the fp32
    sums of up to Tk terms in ANY order (tiles, key halves, merge).  The numerator sum bf16(P) v carries e on every term -
    bf16 keeps 8 significand bits, so half an ulp is up to 2^-8 relative at the bottom of a binade -; l sums the
    un-rounded P and carries e1 only; 2^-22 |y| is o * (1/l) in fp32; 2^-120 covers a flushed subnormal P.  An output
    that is NaN (an unwritten sentinel, 0/0) is infinitely far."""
    o = out.to(F64)
    e1 = 2.0 ** -22 + math.log(2.0) * dx * 1.001 + Tk * U24
    e = 2.0 ** -8 + e1
    bound = 0.5 * _ulp_dev(torch.nan_to_num(o, nan=0.0)) + (e * A + e1 * y.abs()) / (1.0 - e1) + 2.0 ** -22 * y.abs() + 2.0 ** -120
    d = (o - y).abs()
    return torch.where(torch.isnan(d), torch.full_like(d, math.inf), d), bound


def attention_fused_dx(qp: Tensor, k: Tensor, H: int, scale: float) -> Tensor:
    """What the fused query preparation adds to ``attention``'s dx, (B,Tq,H*128): its fp32 sum of the row's squares runs in
    another order than ltxk_qknorm_rope's, a 1-ulp flip of rstd can move at most a couple of elements of the prepared
    query q' by one bf16 ulp, and two such flips move an exponent by at most
        2 * c * ulp_bf16(max_d |q'_d|) * max_d |k_d|       per (row, head), the key maximum over all keys of the head."""
    B, Tq, D = qp.shape
    qm = _heads(qp, H).abs().amax(-1, keepdim=True)                        # (B,H,Tq,1)
    km = _heads(k, H).abs().amax(dim=(-1, -2), keepdim=True)               # (B,H,1,1)
    add = 2.0 * attn_c(scale) * _ulp_dev(qm) * km
    return add.expand(B, H, Tq, FA_DH).transpose(1, 2).reshape(B, Tq, D)


def attention_planted_keys(Tq: int, Tk: int):
    """[(row, key)] of the spiked family: keys 0, 31, 32, 63, 64, Tk-1 and the first key of the last key tile, those that
    exist, each planted on query row (7*key) % Tq.  Keys that land on one row hold equal shares of it, and the family's
    precondition asks 0.25 of the row for each: a row takes three, a fourth moves on to the next row with room (only where
    Tq divides the stride of several edge keys: Tq = 16, Tk = 97 sends keys 0, 32, 64 and 96 to row 0, and 96 goes to row 1)."""
    keys = sorted({j for j in (0, 31, 32, 63, 64, Tk - 1, 64 * ((Tk - 1) // 64)) if 0 <= j < Tk})
    load, pairs = {}, []
    for j in keys:
        row = (7 * j) % Tq
        while load.get(row, 0) >= 3 and min(load.get(r, 0) for r in range(Tq)) < 3:
            row = (row + 1) % Tq
        load[row] = load.get(row, 0) + 1
        pairs.append((row, j))
    return pairs


def attention_plant(q: Tensor, k: Tensor):
    """k with the spiked family's keys planted from q (k[b, key] = 4 * q[b, row], every head; exact in bf16).  Returns
    (k, [(row, key)])."""
    k = k.clone()
    pairs = attention_planted_keys(q.shape[1], k.shape[1])
    for row, j in pairs:
        k[:, j] = (4.0 * q[:, row].float()).to(BF)
    return k, pairs


def attention_inputs(B: int, H: int, Tq: int, Tk: int, family: str, seed: int):
    """The inputs of the attention bound tests (seeded on the CPU, shared by test_ref64_cpu.py and
    test_attn_bound_gpu.py): (q (B,Tq,H*128), k, v (B,Tk,H*128), planted), bf16.
      flat    q, k, v randn;
      peaked  q randn * 4 - logits of std ~4: a row's mass sits on a few keys;
      spiked  flat, plus ``attention_plant``: every edge key is the dominant one of some row, which forces a rescale after
              deferral, in the ragged last tile among others.  planted = its (row, key) pairs, [] otherwise."""
    assert family in ATTN_FAMILIES, family
    g = torch.Generator().manual_seed(seed * 1000003 + ((B * 131 + H) * 4099 + Tq) * 4099 + Tk)
    D = H * FA_DH
    q = torch.randn(B, Tq, D, generator=g)
    k = torch.randn(B, Tk, D, generator=g).to(BF)
    v = torch.randn(B, Tk, D, generator=g).to(BF)
    q = (q * 4 if family == "peaked" else q).to(BF)
    planted = []
    if family == "spiked":
        k, planted = attention_plant(q, k)
    return q, k, v, planted
