"""A set-valued float64 reference of the DiT row kernels and the VAE glue kernels (csrc/rows.h, elementwise.hip,
step_tail.hip, vae_ops.hip, the fused PixelNorm epilogue of conv3d.hip): instead of one correctly rounded value per
element, an interval [lo, hi] of float64 values is carried through the kernel's chain of operations, and the device's
bf16 output ``got`` must satisfy rbf(lo) <= got <= rbf(hi) in EVERY element - no share of the elements is exempt and
no ulp of slack is granted (tests/test_ref_rows_cpu.py shows what the rule accepts and rejects; the GPU call sites are
tests/test_rowops_gpu.py, test_vae_glue_gpu.py, test_attn64_gpu.py and test_conv3d_bound_gpu.py).

The rules.  Nothing in them is measured; u = 2^-24 is the fp32 unit roundoff.

  fp32 operation     (+ - * / sqrtf fmaf as written in the kernel; -ffp-contract=off, IEEE division and square root) the
                     exact result interval is widened by u * max(|lo|, |hi|) on either side; where it then reaches below
                     2^-126 in magnitude it is extended to 0 (a subnormal result flushed to zero is not an error; the
                     allowance is spent only where a flush can happen, and ``within`` counts +-0 and the subnormals as
                     one value).  ``fl``.
                     The widening holds even where the exact result is a single value: bf16(fp32(v)), the kernel's double
                     rounding, and bf16(v), ref64's single rounding, are both admitted.
  exact operation    where BOTH endpoints of the exact result are already fp32 numbers (v == float32(v), zero or normal)
                     nothing is added: rounding is monotone and leaves them where they are.  This covers the product of
                     two bf16 values, 1 + scale and most sums of two bf16 values; without it the exact ties of the bf16
                     rounding that follows would admit both neighbours for a third of the elements.
  bf16 rounding      [lo, hi] -> [rbf(lo), rbf(hi)] with ref64.rbf (round to nearest even from float64).  ``rb``.
  product, quotient  min and max over the endpoint combinations; a square of an interval that holds 0 starts at 0.
  reduction          the fp32 sum of k terms in ANY order whose longest chain of additions is ``depth`` is within
                     depth * u * sum|terms| of the exact sum (for non-negative terms: depth * u relative).  ``depth`` is
                     read from the kernel (table below).  A sum whose terms are all integer multiples of a power of two q
                     with sum|terms| <= 2^24 q is exact in every order (each partial sum is such a multiple and fits 24
                     bits): a constant or all-zero row carries no error, as on the device.
  / (float)D, + eps  one fp32 operation each;  sqrtf, fp32 division: correctly rounded, one u each.
  rsqrtf             2 u (the figure of the Gemma row kernels' derivation, tests/test_gemma_kernels_gpu.py).
  silu               ref_gemm.E_ACT relative (derived there for silu_f = x * rcp(1 + exp2(c x))), flush as above; silu_div
                     (x / (1 + expf(-x)): expf 1 ulp, one add, one IEEE division, ~4 u) lies inside the same figure.
  LayerNorm, GroupNorm   intervals end to end: mean -> x - mean -> centred variance -> rstd -> n.  No linearised
                     cancellation term: on rows of 100 + N(0,1) the intervals are wide, which is the honest bound there.
  PixelNorm          the rounded row statistics m, e, s are intervals too; where s holds two bf16 values the division
                     chain is evaluated for either and the hull is taken (x / s is monotone in s).

Depth of each kernel's own reduction (longest chain of fp32 additions):

  norm_modulate_kernel, norm_modulate2_kernel   D/64 terms per lane (chunk by chunk, element by element) + 6 butterfly levels
  norm_scale_kernel (_ss), norm_scale2_kernel   ceil(NP/64) partials per lane + 6; the partials are fp32 inputs taken as given
  qknorm_rope_kernel<MAXP>     16 elements per lane and pass of 8 heads, ceil(H/8) passes: 16 ceil(H/8) + 6
  qknorm_rope_ss_kernel        ceil(NP/64) + 6, NP = D/64
  qknorm_rope_dh64_kernel      16 elements per lane and pass of 16 heads: 16 ceil(H/16) + 6; with partials (H <= 32 of them,
                               one per lane) 1 + 6
  pixelnorm_act_kernel<LPR, PASSES>   8 PASSES terms per lane + log2(LPR) levels, LPR = min(C/8, 64)
  conv3d fused PixelNorm epilogue     16 terms per lane + 2 levels (wave_row_sum) + Cout/64 partials through LDS
  groupnorm_act_kernel         ceil(n/256) elements per thread + 6 levels + 3 additions of the four waves' sums, n = V C/G

``within(got, iv)`` is the comparator.  The input builders of the GPU cases live here too, so that test_ref_rows_cpu.py
judges the reference on the very inputs the device sees."""
from __future__ import annotations

import itertools
import math
from types import SimpleNamespace
from typing import Optional

import torch

import ref64 as R
from ref_gemm import E_ACT

Tensor = torch.Tensor
F64 = torch.float64
BF = torch.bfloat16
U = 2.0 ** -24
FLUSH = 2.0 ** -126
SILU_ARGMIN = -1.2784645427610737            # where x sigmoid(x) has its minimum


# ------------------------------------------------------------------------------------------------------- intervals
class Iv:
    """An interval of float64 values per element.  Iv(x) is the exact point x."""
    __slots__ = ("lo", "hi")

    def __init__(self, lo, hi=None):
        self.lo = R.f64(lo)
        self.hi = self.lo if hi is None else R.f64(hi)

    def map(self, f) -> "Iv":
        """The same view / gather of both endpoints."""
        return Iv(f(self.lo), f(self.hi))


def _iv(a) -> Iv:
    return a if isinstance(a, Iv) else Iv(a)


def _is_f32(v: Tensor) -> Tensor:
    a = v.abs()
    return (v.float().double() == v) & ((a == 0) | (a >= FLUSH))


def _flushed(lo: Tensor, hi: Tensor) -> Iv:
    """Where the interval reaches into the fp32 subnormals, 0 is admissible too (a flushed result is not an error)."""
    z = torch.zeros_like(lo)
    return Iv(torch.where((lo > 0) & (lo < FLUSH), z, lo), torch.where((hi < 0) & (hi > -FLUSH), z, hi))


def fl(a: Iv) -> Iv:
    """One fp32 rounding of the exact result interval a."""
    exact = _is_f32(a.lo) & _is_f32(a.hi)
    w = U * torch.maximum(a.lo.abs(), a.hi.abs())
    return _flushed(torch.where(exact, a.lo, a.lo - w), torch.where(exact, a.hi, a.hi + w))


def wid(a: Iv, k: float) -> Iv:
    """a widened by k u relative on either side: a reduction of depth k, rsqrtf, silu."""
    w = k * U * torch.maximum(a.lo.abs(), a.hi.abs())
    return _flushed(a.lo - w, a.hi + w)


def rb(a: Iv) -> Iv:
    return Iv(R.rbf(a.lo), R.rbf(a.hi))


def add(a, b) -> Iv:
    a, b = _iv(a), _iv(b)
    return Iv(a.lo + b.lo, a.hi + b.hi)


def sub(a, b) -> Iv:
    a, b = _iv(a), _iv(b)
    return Iv(a.lo - b.hi, a.hi - b.lo)


def _hull4(c) -> Iv:
    lo, hi = c[0], c[0]
    for t in c[1:]:
        lo, hi = torch.minimum(lo, t), torch.maximum(hi, t)
    return Iv(lo, hi)


def mul(a, b) -> Iv:
    a, b = _iv(a), _iv(b)
    return _hull4([a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi])


def div(a, b) -> Iv:
    a, b = _iv(a), _iv(b)
    assert bool(((b.lo > 0) | (b.hi < 0)).all()), "division by an interval that holds 0"
    return _hull4([a.lo / b.lo, a.lo / b.hi, a.hi / b.lo, a.hi / b.hi])


def sqr(a: Iv) -> Iv:
    l2, h2 = a.lo * a.lo, a.hi * a.hi
    lo = torch.where((a.lo <= 0) & (a.hi >= 0), torch.zeros_like(l2), torch.minimum(l2, h2))
    return Iv(lo, torch.maximum(l2, h2))


def sqrt(a: Iv) -> Iv:
    return Iv(torch.sqrt(a.lo.clamp_min(0.0)), torch.sqrt(a.hi.clamp_min(0.0)))


def rsqrt(a: Iv) -> Iv:
    assert bool((a.lo > 0).all())
    return Iv(1.0 / torch.sqrt(a.hi), 1.0 / torch.sqrt(a.lo))


def hull(a: Iv, b: Iv) -> Iv:
    return Iv(torch.minimum(a.lo, b.lo), torch.maximum(a.hi, b.hi))


def stack(ivs, dim) -> Iv:
    return Iv(torch.stack([a.lo for a in ivs], dim), torch.stack([a.hi for a in ivs], dim))


def _quantum(v: Tensor) -> Tensor:
    """The largest power of two that divides each float64 value (inf for 0)."""
    m, e = torch.frexp(v.abs())
    mi = (m * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return torch.where(v == 0, torch.full_like(v, math.inf), low * torch.exp2(e.double() - 53))


def reduce_sum(t: Iv, dims, depth: int) -> Iv:
    """The fp32 sum of the terms t over ``dims`` (keepdim) in any order of chain depth ``depth``."""
    s = Iv(t.lo.sum(dims, keepdim=True), t.hi.sum(dims, keepdim=True))
    mag = torch.maximum(t.lo.abs(), t.hi.abs()).sum(dims, keepdim=True)
    point = (t.lo == t.hi).all()
    if bool(point):                                        # a sum of multiples of q that fits 24 bits is exact
        q = _quantum(t.lo).amin(dims, keepdim=True)
        exact = mag <= 2.0 ** 24 * q
    else:
        exact = torch.zeros_like(mag, dtype=torch.bool)
    w = torch.where(exact, torch.zeros_like(mag), depth * U * mag)
    return Iv(s.lo - w, s.hi + w)


def silu_iv(a: Iv) -> Iv:
    """silu of an interval (the function has one minimum), widened by the device's evaluation error."""
    f = lambda x: x / (1.0 + torch.exp(-x))
    flo, fhi = f(a.lo), f(a.hi)
    lo, hi = torch.minimum(flo, fhi), torch.maximum(flo, fhi)
    inside = (a.lo < SILU_ARGMIN) & (a.hi > SILU_ARGMIN)
    lo = torch.where(inside, torch.full_like(lo, SILU_ARGMIN / (1.0 + math.exp(-SILU_ARGMIN))), lo)
    out = wid(Iv(lo, hi), E_ACT / U)
    zero = (a.lo == 0) & (a.hi == 0)                       # 0 * rcp(2), 0 / 2: exactly 0
    return Iv(torch.where(zero, a.lo, out.lo), torch.where(zero, a.hi, out.hi))


# ------------------------------------------------------------------------------------------------------ comparator
def bf16_ord(v: Tensor) -> Tensor:
    """bf16 values (as float64) -> integers in value order, neighbouring bf16 values one apart; +-0 and the subnormals, which
    a flush makes one value, are all 0."""
    b = v.to(BF).contiguous().view(torch.int16).to(torch.int32)
    mag = ((b & 0x7FFF) - 0x7F).clamp_min(0)
    return torch.where(b < 0, -mag, mag)


def within(got, iv: Iv):
    """((outside, first), ambiguous, widest): the count of elements of ``got`` outside [rbf(lo), rbf(hi)] and the flat
    index of the first (-1 if none); the share of elements whose interval holds more than one bf16 value; the widest
    interval in bf16 steps (0: one admissible value, 1: two neighbours).  NaN in ``got`` is outside."""
    g = R.f64(got).flatten()
    lo, hi = R.rbf(iv.lo).expand_as(R.f64(got)).flatten(), R.rbf(iv.hi).expand_as(R.f64(got)).flatten()
    bad = ~((g >= lo) & (g <= hi))
    n = int(bad.sum())
    first = int(torch.nonzero(bad)[0]) if n else -1
    steps = bf16_ord(hi) - bf16_ord(lo)
    amb = float((steps >= 1).double().mean()) if steps.numel() else 0.0
    return (n, first), amb, int(steps.max()) if steps.numel() else 0


# ---------------------------------------------------------------------------------------------------- DiT row chains
def norm_depth(D: int) -> int:
    return D // 64 + 6


def partials_depth(NP: int) -> int:
    return -(-NP // 64) + 6


def _rstd(ss: Iv, D: int, eps: float) -> Iv:
    """rsqrtf(ss / (float)D + eps)"""
    return wid(rsqrt(fl(add(fl(div(ss, float(D))), eps))), 2)


def _modulate(n: Iv, scale, shift, one_plus: bool) -> Iv:
    one_p = Iv(scale) if one_plus else rb(fl(add(1.0, Iv(scale))))
    return rb(fl(add(rb(fl(mul(n, one_p))), Iv(shift))))


def norm_modulate(x, eps: float, scale=None, shift=None, *, layernorm: bool = False, one_plus: bool = False,
                  partials=None, depth: Optional[int] = None) -> Iv:
    """norm_modulate_kernel<LAYERNORM> / norm_scale_kernel: x (M,D); scale, shift (M,D) as gathered per row, or None;
    partials (M,NP) fp32 (the `_ss` form, rms only)."""
    x = R.f64(x)
    D = x.shape[-1]
    if partials is not None:
        p = R.f64(partials)
        ss = reduce_sum(Iv(p), -1, partials_depth(p.shape[-1]) if depth is None else depth)
        d = Iv(x)
    elif layernorm:
        depth = norm_depth(D) if depth is None else depth
        mean = fl(div(reduce_sum(Iv(x), -1, depth), float(D)))
        d = fl(sub(x, mean))
        ss = reduce_sum(fl(sqr(d)), -1, depth)
    else:
        ss = reduce_sum(Iv(x * x), -1, norm_depth(D) if depth is None else depth)
        d = Iv(x)
    ss = Iv(ss.lo.clamp_min(0.0), ss.hi)
    pre = fl(mul(d, _rstd(ss, D, eps)))
    if scale is None:
        return rb(pre)
    return _modulate(rb(pre), scale, shift, one_plus)


def qknorm_depth(H: int, dh: int = 128, partials: bool = False) -> int:
    if partials:
        return partials_depth(H * dh // 64) if dh == 128 else 1 + 6
    return 16 * (-(-H // (8 if dh == 128 else 16))) + 6


def qknorm_rope(x, weight, cos, sin, T: int, H: int, eps: float, dh: int = 128, partials=None,
                depth: Optional[int] = None) -> Iv:
    """rows.h norm_rope behind qknorm_rope_kernel / _ss_kernel / _dh64_kernel: x (M, nseg*D), weight (nseg, D), cos / sin
    (H, T, dh/2) fp32 or None, row m is token m % T; partials (M, nseg*NP) fp32 or None."""
    x = R.f64(x)
    M = x.shape[0]
    nseg, D = weight.shape
    half = dh // 2
    seg = x.reshape(M, nseg, D)
    depth = qknorm_depth(H, dh, partials is not None) if depth is None else depth
    if partials is not None:
        ss = reduce_sum(Iv(R.f64(partials).reshape(M, nseg, -1)), -1, depth)
    else:
        ss = reduce_sum(Iv(seg * seg), -1, depth)
    ss = Iv(ss.lo.clamp_min(0.0), ss.hi)
    y = rb(fl(mul(fl(mul(seg, _rstd(ss, D, eps))), R.f64(weight)[None])))
    if cos is None:
        return y.map(lambda t: t.reshape(M, nseg * D))
    yh = y.map(lambda t: t.reshape(M, nseg, H, 2, half))
    t = torch.arange(M) % T
    c = R.f64(cos)[:, t].permute(1, 0, 2)[:, None]
    s = R.f64(sin)[:, t].permute(1, 0, 2)[:, None]
    x1, x2 = yh.map(lambda v: v[..., 0, :]), yh.map(lambda v: v[..., 1, :])
    oa = rb(fl(sub(fl(mul(x1, c)), fl(mul(s, x2)))))
    ob = rb(fl(add(fl(mul(x2, c)), fl(mul(s, x1)))))
    return stack([oa, ob], -2).map(lambda v: v.reshape(M, nseg * D))


def _euler_fp32(x: Iv, x0: Iv, sigma: float, sigma_next: float) -> Iv:
    return fl(add(x0, fl(div(fl(mul(sigma_next, fl(sub(x, x0)))), sigma))))


def cfg_euler_step(v_pos, v_neg, latent, sigma: float, sigma_next: float, cfg: float = 1.0, clean=None, mask=None,
                   bf16_euler: bool = False) -> Iv:
    """step_tail_kernel<0, false>: v_* (B,S,C) tokens, latent / clean (B,C,S), mask (B,S) fp32; returns (B,C,S)."""
    vp = Iv(R.f64(v_pos).transpose(1, 2))
    x = Iv(latent)
    v = vp
    if v_neg is not None:
        k = fl(sub(R.f32(cfg), 1.0))                                # cfg - 1.0f
        d = rb(fl(sub(vp, R.f64(v_neg).transpose(1, 2))))
        v = rb(fl(add(vp, rb(fl(mul(k, d))))))
    x0 = rb(fl(sub(x, fl(mul(sigma, v)))))
    if mask is not None:
        m = Iv(R.f64(mask)[:, None, :])
        x0 = rb(fl(add(rb(fl(mul(x0, m))), rb(fl(mul(Iv(clean), rb(fl(sub(1.0, m)))))))))
    if bf16_euler:
        return rb(fl(add(x0, rb(fl(div(rb(fl(mul(sigma_next, rb(fl(sub(x, x0)))))), sigma))))))
    if sigma_next > 0:
        return rb(_euler_fp32(x, x0, sigma, sigma_next))
    return x0


def euler_step(latent, denoised, sigma: float, sigma_next: float) -> Iv:
    """euler_kernel: always the fp32 form."""
    return rb(_euler_fp32(Iv(latent), Iv(denoised), sigma, sigma_next))


def silu(x) -> Iv:
    return rb(silu_iv(Iv(x)))


# ------------------------------------------------------------------------------------------------------- VAE glue
def pixelnorm_depth(C: int) -> int:
    lpr = min(C // 8, 64)
    return 8 * (C // (8 * lpr)) + int(math.log2(lpr))


def fused_pixelnorm_depth(Cout: int) -> int:
    return 16 + 2 + Cout // 64


def pixelnorm_act(x, eps: float, scale=None, shift=None, rows_per_batch: int = 0, silu_on: bool = False,
                  depth: Optional[int] = None) -> Iv:
    """pixelnorm_act_kernel (and conv3d's fused epilogue with depth = fused_pixelnorm_depth): x (V,C); scale / shift
    (B,C) or None, row v using row v // rows_per_batch."""
    x = R.f64(x)
    V, C = x.shape
    S = reduce_sum(Iv(R.rbf(x * x)), -1, pixelnorm_depth(C) if depth is None else depth)
    m = rb(fl(div(Iv(S.lo.clamp_min(0.0), S.hi), float(C))))
    s = rb(fl(sqrt(rb(fl(add(m, eps))))))

    def quotient(sp: Tensor) -> Iv:          # x / s by reciprocal and one Newton step: q0 = x r; q0 + fma(-q0, s, x) r
        rsd = fl(div(1.0, Iv(sp)))
        q0 = fl(mul(x, rsd))
        res = fl(sub(x, mul(q0, Iv(sp))))                  # fmaf: one rounding of the exact residual
        return rb(fl(add(mul(res, rsd), q0)))              # fmaf again

    y = hull(quotient(s.lo), quotient(s.hi))
    if scale is not None:
        b = torch.arange(V) // rows_per_batch
        y = _modulate(y, R.f64(scale)[b], R.f64(shift)[b], False)
    if silu_on:
        y = rb(silu_iv(y))
    return y


def groupnorm_depth(n: int) -> int:
    return -(-n // 256) + 6 + 3


def groupnorm_act(x, gamma, beta, G: int, eps: float, resid=None, apply_silu: bool = False, depth: Optional[int] = None) -> Iv:
    """groupnorm_act_kernel: x (B,V,C) channels-last."""
    x = R.f64(x)
    B, V, C = x.shape
    cg = C // G
    n = V * cg
    depth = groupnorm_depth(n) if depth is None else depth
    xg = x.reshape(B, V, G, cg)
    mean = fl(div(reduce_sum(Iv(xg), (1, 3), depth), float(n)))
    d = fl(sub(xg, mean))
    var = fl(div(reduce_sum(fl(sqr(d)), (1, 3), depth), float(n)))
    sd = fl(sqrt(fl(add(Iv(var.lo.clamp_min(0.0), var.hi), eps))))
    gm, bt = R.f64(gamma).reshape(G, cg), R.f64(beta).reshape(G, cg)
    y = rb(fl(add(fl(mul(fl(div(d, sd)), gm)), bt))).map(lambda t: t.reshape(B, V, C))
    if resid is not None:
        y = rb(fl(add(y, R.f64(resid))))
    if apply_silu:
        y = rb(silu_iv(y))
    return y


def latent_denorm_cl(latent, mean, std, noise=None, noise_scale: float = 0.0) -> Iv:
    """latent_denorm_cl_kernel: (B,C,S) -> (B,S,C)."""
    x = Iv(latent)
    if noise is not None:
        s = R.f32(noise_scale)
        x = rb(fl(add(rb(fl(mul(Iv(noise), s))), rb(fl(mul(fl(sub(1.0, s)), x))))))
    out = rb(fl(add(fl(mul(x, R.f64(std)[None, :, None])), R.f64(mean)[None, :, None])))
    return out.map(lambda t: t.transpose(1, 2).contiguous())


def latent_norm_cf(x, mean, std) -> Iv:
    """latent_norm_cf_kernel: (B,S,C) -> (B,C,S)."""
    out = rb(fl(div(fl(sub(Iv(x), R.f64(mean))), R.f64(std))))
    return out.map(lambda t: t.transpose(1, 2).contiguous())


def tile_blend(tiles, F: int, H: int, W: int) -> Iv:
    """tile_blend_accum_kernel in launch order, then tile_blend_finalize_kernel: acc += v * m and wsum += m in fp32 with
    m = (mt*mh)*mw, out = bf16(acc / max(wsum, 1e-8f))."""
    B, C = tiles[0][0].shape[:2]
    zero = lambda *s: torch.zeros(*s, dtype=F64)
    acc, ws = Iv(zero(B, C, F, H, W), zero(B, C, F, H, W)), Iv(zero(B, 1, F, H, W), zero(B, 1, F, H, W))
    for tile, (at, ah, aw), mt, mh, mw, (t0, h0, w0) in tiles:
        m = fl(mul(fl(mul(R.f64(mt)[:at, None, None], R.f64(mh)[None, :ah, None])), R.f64(mw)[None, None, :aw]))
        box = (slice(None), slice(None), slice(t0, t0 + at), slice(h0, h0 + ah), slice(w0, w0 + aw))
        a = fl(add(acc.map(lambda t: t[box]), fl(mul(R.f64(tile)[:, :, :at, :ah, :aw], m))))
        w = fl(add(ws.map(lambda t: t[box]), m))
        for dst, src in ((acc, a), (ws, w)):
            lo, hi = dst.lo.clone(), dst.hi.clone()
            lo[box], hi[box] = src.lo, src.hi
            dst.lo, dst.hi = lo, hi
    floor = R.f32(1e-8)
    return rb(fl(div(acc, Iv(ws.lo.clamp_min(floor), ws.hi.clamp_min(floor)))))


# ------------------------------------------------------------------------------------------- the GPU cases' inputs
def gen(seed: int):
    return torch.Generator().manual_seed(seed)


def gpu_cases(fn):
    """Every parameter combination of a parametrised pytest function, as dicts (read from its own marks)."""
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    axes = []
    for m in marks:
        names = [n.strip() for n in m.args[0].split(",")]
        axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    return [dict(kv for d in combo for kv in d.items()) for combo in itertools.product(*axes)]


def all_finite_bf16(lo: float, hi: float) -> Tensor:
    b = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF)
    f = b.float()
    return b[torch.isfinite(f) & (f >= lo) & (f <= hi)]


# Seeds.  A salt moves a case to other random inputs; it is chosen on the reference alone (the smallest for which
# test_ref_rows_cpu.py's condition holds: at most 2 % of the elements with two admissible values, none with more), the way
# ref64.PIXELNORM_SEED was.  Cases that are not listed keep the seed they always had.
SALT = 1000003
NORM_SALT = {(1024, 3): 1, (2048, 5): 1, (8192, 3): 1, (8192, 5): 1}          # rms rows, (D, M): no ambiguous element in any mode
SMALL_MEAN_M = 5
SMALL_MEAN_SALT = {512: 5}
CFG_SALT = {('none', 0.725, False, False): 5, ('1', 0.725, False, False): 1, ('1', 0.725, False, True): 16,
            ('1', 0.0, False, True): 4, ('4', 0.0, False, True): 3}                # (cfg, sigma_next, bf16_euler, masked)
GROUPNORM_SALT = {(64, 1, False, True): 3, (96, 7, False, True): 8, (96, 7, True, True): 2, (512, 1, True, True): 1,
                  (512, 7, False, True): 2}                                       # (C, V, resid, silu)


def norm_seed(ln: bool, D: int, M: int) -> int:
    return D + 10 * M + (7 if ln else SALT * NORM_SALT.get((D, M), 0))


def small_mean_seed(D: int) -> int:
    return 300 + D + SALT * SMALL_MEAN_SALT.get(D, 0)


def norm_inputs(ln: bool, M: int, D: int, mode: str, seed: int, special_rows: bool = False, small_mean: bool = False):
    """x (M,D) and the modulation of test_norm_modulate_edges: rows of 100 + N(0,1) for LayerNorm (or 0.5 + 3 N(0,1), the
    small-mean family), 3 N(0,1) for rms; mode 'none' | 'scale_shift' (one row of a (1,2D) table) | 'mod_row' (U = 3 rows of a
    (U,6D) table picked per token).  sc / sh are the gathered (M,D) rows, tab / rows / stride what the launch gets."""
    g = gen(seed)
    if small_mean:
        x = torch.randn(M, D, generator=g) * 3 + 0.5
    else:
        x = (torch.randn(M, D, generator=g) + 100) if ln else torch.randn(M, D, generator=g) * 3
    if special_rows and M >= 2:
        x[0] = 3.0
        x[1] = 0.0
    x = x.to(BF)
    tab = rows = sc = sh = None
    stride = 0
    if mode == "scale_shift":
        tab = torch.randn(1, 2 * D, generator=g).to(BF)
        sc, sh, stride = tab[:, D:].expand(M, D), tab[:, :D].expand(M, D), 2 * D
    elif mode == "mod_row":
        U_ = 3
        tab = torch.randn(U_, 6 * D, generator=g).to(BF)
        rows = torch.randint(0, U_, (M,), generator=g, dtype=torch.int32)
        sc, sh, stride = tab[rows.long(), D:2 * D], tab[rows.long(), :D], 6 * D
    return SimpleNamespace(x=x, tab=tab, rows=rows, sc=sc, sh=sh, stride=stride, mode=mode, ln=ln, D=D, M=M)


def rmsnorm_ss_inputs(D: int, M: int, one_plus: bool):
    """test_rmsnorm_ss_edges: x, the NP = D/64 fp32 partials inside a wider row (garbage behind them), a (3,6D) table."""
    g = gen(100 + D + M)
    U_ = 3
    x = (torch.randn(M, D, generator=g) * 3).to(BF)
    NP = D // 64
    ssld = NP + 5
    ss = torch.full((M, ssld), 1e30)
    ss[:, :NP] = (x.double() ** 2).reshape(M, NP, 64).sum(-1).float()
    tab = torch.randn(U_, 6 * D, generator=g).to(BF)
    rows = torch.randint(0, U_, (M,), generator=g, dtype=torch.int32)
    sc, sh = tab[rows.long(), D:2 * D], tab[rows.long(), :D]
    if one_plus:
        tab[:, D:2 * D] = R.rbf(1.0 + tab[:, D:2 * D].double()).to(BF)
        sc = tab[rows.long(), D:2 * D]
    return SimpleNamespace(x=x, ss=ss, NP=NP, tab=tab, rows=rows, sc=sc, sh=sh, D=D, M=M, one_plus=one_plus)


def qknorm_inputs(H: int, ss: bool, nseg: int, rope: bool, dh: int = 128):
    """test_qknorm_rope_edges (dh 128) / test_qknorm_rope_dh64_edges (dh 64): B = 2, T = 7."""
    g = gen((1000 if dh == 128 else 2000) + 37 * H + 5 * nseg + (2 if rope else 0) + (1 if ss else 0))
    B, T = 2, 7
    M, D = B * T, H * dh
    x = torch.randn(M, nseg * D, generator=g).to(BF)
    w = (1 + 0.3 * torch.randn(nseg, D, generator=g)).to(BF)
    cos = sin = None
    if rope:
        ang = torch.rand(H, T, dh // 2, generator=g) * 8 - 4
        cos, sin = torch.cos(ang), torch.sin(ang)
    sumsq = None
    NP = D // 64
    if ss:
        ssld = nseg * NP + 3
        sumsq = torch.full((M, ssld), 1e30)
        sumsq[:, :nseg * NP] = (x.double() ** 2).reshape(M, nseg * NP, 64).sum(-1).float()
    return SimpleNamespace(x=x, w=w, cos=cos, sin=sin, sumsq=sumsq, NP=NP, B=B, T=T, M=M, D=D, H=H, nseg=nseg, dh=dh)


def qknorm_partials(inp):
    return None if inp.sumsq is None else inp.sumsq[:, :inp.nseg * inp.NP]


def cfg_euler_inputs(cfg: str, sn: float, bf16_euler: bool, masked: bool, salt: Optional[int] = None):
    """test_cfg_euler_edges: B = 2, C = 16, S = 67."""
    salt = CFG_SALT.get((cfg, sn, bool(bf16_euler), bool(masked)), 0) if salt is None else salt
    g = gen(7 + len(cfg) + int(sn * 10) + 2 * bf16_euler + 4 * masked + SALT * salt)
    B, C, S = 2, 16, 67
    vp = torch.randn(B, S, C, generator=g).to(BF)
    vn = torch.randn(B, S, C, generator=g).to(BF) if cfg != "none" else None
    cs = 1.0 if cfg == "none" else float(cfg)
    x = torch.randn(B, C, S, generator=g).to(BF)
    clean = torch.randn(B, C, S, generator=g).to(BF) if masked else None
    mask = torch.tensor([0.0, 1.0, 0.75])[torch.randint(0, 3, (B, S), generator=g)] if masked else None
    return SimpleNamespace(vp=vp, vn=vn, cs=cs, x=x, clean=clean, mask=mask, sig=R.f32(0.909375), sig_n=R.f32(sn), B=B, C=C, S=S,
                           bf16_euler=bf16_euler)


def euler_inputs(sn: float):
    """test_euler_step_edges: n = 8 * (256*3 + 5)."""
    g = gen(int(sn * 10))
    n = 8 * (256 * 3 + 5)
    x, x0 = torch.randn(n, generator=g).to(BF), torch.randn(n, generator=g).to(BF)
    return SimpleNamespace(x=x, x0=x0, n=n, sig=R.f32(0.9), sig_n=R.f32(sn))


def silu_inputs():
    """test_silu_every_value: every finite bf16 in [-100, 100], large values of both signs, zero fill to n = 8*(256k + 3)."""
    big = torch.tensor([1e4, -1e4, 1e30, -1e30, 3.0e38, -3.0e38, -88.5, -88.75, -89.0, -90.0, -91.5, -95.0, -104.0])
    x = torch.cat([all_finite_bf16(-100.0, 100.0), big.to(BF)])
    k = (x.numel() // 8 + 255) // 256
    n = 8 * (256 * k + 3)
    return torch.cat([x, torch.zeros(n - x.numel(), dtype=BF)])


def groupnorm_inputs(C: int, V: int, resid: bool, silu: bool, salt: Optional[int] = None):
    """test_groupnorm_act_edges: B = 2, G = 32, channels at a common offset of 50 (53 in batch 1)."""
    salt = GROUPNORM_SALT.get((C, V, bool(resid), bool(silu)), 0) if salt is None else salt
    g = gen(C + V + 2 * resid + silu + SALT * salt)
    B, G = 2, 32
    x = (torch.randn(B, V, C, generator=g) + 50).to(BF)
    x[1] += 3.0
    x = x.to(BF)
    gam = (1 + 0.3 * torch.randn(C, generator=g)).to(BF)
    bet = (0.3 * torch.randn(C, generator=g)).to(BF)
    r = torch.randn(B, V, C, generator=g).to(BF) if resid else None
    return SimpleNamespace(x=x, gam=gam, bet=bet, r=r, B=B, G=G, V=V, C=C, silu=bool(silu), eps=R.f32(1e-5))


def latent_denorm_inputs(noise_scale: float):
    g = gen(int(noise_scale * 100))
    B, C, S = 2, 128, 65
    lat = torch.randn(B, C, S, generator=g).to(BF)
    noise = torch.randn(B, C, S, generator=g).to(BF) if noise_scale else None
    mean = (0.3 * torch.randn(C, generator=g)).to(BF)
    std = (1 + 0.2 * torch.randn(C, generator=g)).abs().to(BF)
    return SimpleNamespace(lat=lat, noise=noise, mean=mean, std=std, B=B, C=C, S=S, noise_scale=noise_scale)


def latent_norm_inputs(pad: int):
    g = gen(pad + 1)
    B, C, S = 2, 128, 65
    x = torch.randn(B, S, C, generator=g).to(BF)
    mean = (0.3 * torch.randn(C, generator=g)).to(BF)
    std = (1.3 + 0.2 * torch.rand(C, generator=g)).to(BF)
    return SimpleNamespace(x=x, mean=mean, std=std, B=B, C=C, S=S, ldx=C + pad)


def tile_blend_inputs():
    g = gen(11)
    B, C, F, H, W = 2, 3, 5, 9, 11
    Tt, Th, Tw = 3, 6, 7
    tiles = []
    for (at, ah, aw), off in [((3, 6, 7), (0, 0, 0)), ((3, 6, 7), (2, 3, 4)), ((2, 4, 5), (3, 0, 6))]:
        tile = torch.randn(B, C, Tt, Th, Tw, generator=g).to(BF)
        mt, mh, mw = (torch.rand(k, generator=g) * 0.9 + 0.1 for k in (Tt, Th, Tw))
        tiles.append((tile, (at, ah, aw), mt, mh, mw, off))
    return SimpleNamespace(tiles=tiles, B=B, C=C, F=F, H=H, W=W)


# The most the share of ambiguous elements (intervals of more than one bf16 value) may be in a GPU case, asserted on the
# reference alone in test_ref_rows_cpu.py.  The cancellation cases carry no cap (1.0) and have their shares printed there:
# LayerNorm on rows of 100 + N(0,1), euler_step, the bf16 Euler tail; and two of the same kind - GroupNorm on a 12480-voxel
# volume at an offset of 50 (x - mean cancels against a mean of 24960 or 37440 terms), and latent_denorm_cl at noise_scale
# 0.05 (x * fp32(1 - 0.05) lies within 2^-26 of a bf16 tie for every x whose 8-bit significand is a multiple of 10: a
# tenth of all bf16 values, whatever the seed, and the fp32 product and the exact one round to different sides).
AMBIGUOUS_CAP = 2e-2
NO_CAP = 1.0


def cap(cancellation_case: bool) -> float:
    return NO_CAP if cancellation_case else AMBIGUOUS_CAP


def groupnorm_cancels(V: int) -> bool:
    return V >= 12480


def latent_denorm_ties(noise_scale: float) -> bool:
    return noise_scale == 0.05
