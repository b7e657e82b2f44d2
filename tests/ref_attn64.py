"""The float64 restatements of ref64.py that are hard-coded there at head dim 128 (rotation half 64), general in the head
dim: the attention reference with its derived per-element bound, its seeded input families, and the q/k norm + SPLIT rope
row chain.  Used by the head-dim-64 tests (ltxk_flash_attn_dh64, ltxk_qknorm_rope_dh64); at dh = 128 every function here
returns what its ref64 namesake returns (tests/test_audio_dit_cpu.py asserts that).

The bound is ref64.attention_bound's derivation with dh in place of 128 in dx - nothing in it is measured:

    dx    = max_k(c * dh * 2^-24 * smag) + 2^-24 * (2 max_k |x| + 8)
    e1    = 2^-22 + ln2 * dx * 1.001 + Tk * 2^-24
    bound = 1/2 ulp_bf16(out) + ((2^-8 + e1) A + e1 |y|) / (1 - e1) + 2^-22 |y| + 2^-120

fp32 accumulation of dh products in any order gives the first term of dx; the second is the rounding of the one fma
x - M with the integer offset M within 7 of the row maximum (ltxk_flash_attn_dh64 keeps it within 1: a ceil, no deferral).
attention_bound itself does not depend on the head dim and is ref64's."""
import math

import torch

import ref64 as R

Tensor = torch.Tensor
F64 = torch.float64
BF = torch.bfloat16
U24 = 2.0 ** -24
attention_bound = R.attention_bound
attn_c = R.attn_c
ATTN_FAMILIES = R.ATTN_FAMILIES


def _heads(t: Tensor, H: int, dh: int) -> Tensor:
    B, T, _ = t.shape
    return t.to(F64).reshape(B, T, H, dh).transpose(1, 2)                   # (B,H,T,dh)


def attention_probs(q: Tensor, k: Tensor, H: int, scale: float, dh: int):
    """ref64.attention_probs at head dim dh: (P, x, smag), each (B,H,Tq,Tk) float64."""
    qh, kh = _heads(q, H, dh), _heads(k, H, dh)
    x = attn_c(scale) * (qh @ kh.transpose(-1, -2))                       # products of bf16 values, sums of dh: exact in float64
    smag = qh.abs() @ kh.abs().transpose(-1, -2)
    p = torch.exp2(x - x.amax(-1, keepdim=True))
    return p / p.sum(-1, keepdim=True), x, smag


def attention(q: Tensor, k: Tensor, v: Tensor, H: int, scale: float, dh: int):
    """ref64.attention at head dim dh: q (B,Tq,H*dh), k, v (B,Tk,H*dh) bf16 -> (y, A, dx), each (B,Tq,H*dh) float64."""
    B, Tq, D = q.shape
    c = attn_c(scale)
    p, x, smag = attention_probs(q, k, H, scale, dh)
    vh = _heads(v, H, dh)
    y = p @ vh
    A = p @ vh.abs()
    dx = (c * dh * U24 * smag).amax(-1, keepdim=True) + U24 * (2.0 * x.abs().amax(-1, keepdim=True) + 8.0)
    back = lambda t: t.transpose(1, 2).reshape(B, Tq, D)
    return back(y), back(A), back(dx.expand(B, H, Tq, dh))


def attention_inputs(B: int, H: int, Tq: int, Tk: int, family: str, seed: int, dh: int):
    """ref64.attention_inputs at head dim dh (the same seeds, families and planted keys): (q, k, v, planted), bf16."""
    assert family in ATTN_FAMILIES, family
    g = torch.Generator().manual_seed(seed * 1000003 + ((B * 131 + H) * 4099 + Tq) * 4099 + Tk)
    D = H * dh
    q = torch.randn(B, Tq, D, generator=g)
    k = torch.randn(B, Tk, D, generator=g).to(BF)
    v = torch.randn(B, Tk, D, generator=g).to(BF)
    q = (q * 4 if family == "peaked" else q).to(BF)
    planted = []
    if family == "spiked":
        k, planted = R.attention_plant(q, k)
    return q, k, v, planted


def qknorm_rope(x, weight, cos, sin, T: int, H: int, eps: float, dh: int):
    """ref64.qknorm_rope at head dim dh: cos / sin (H, T, dh/2) or None, the rotation partner of channel j of a head is
    j + dh/2.  Returns (out, mag)."""
    x = R.f64(x)
    M = x.shape[0]
    nseg, D = weight.shape
    assert D == H * dh
    half = dh // 2
    seg = x.reshape(M, nseg, D)
    rstd = 1.0 / torch.sqrt((seg * seg).mean(-1, keepdim=True) + eps)
    y = R.rbf(seg * rstd * R.f64(weight)[None])
    if cos is None:
        return y.reshape(M, nseg * D), None
    yh = y.reshape(M, nseg, H, 2, half)
    t = torch.arange(M) % T
    c = R.f64(cos)[:, t].permute(1, 0, 2)[:, None]          # (M,1,H,half)
    s = R.f64(sin)[:, t].permute(1, 0, 2)[:, None]
    x1, x2 = yh[..., 0, :], yh[..., 1, :]
    o = torch.stack([x1 * c - s * x2, x2 * c + s * x1], dim=-2)
    mag = torch.stack([(x1 * c).abs() + (s * x2).abs(), (x2 * c).abs() + (s * x1).abs()], dim=-2)
    return R.rbf(o).reshape(M, nseg * D), mag.reshape(M, nseg * D)


def flash_loop_fp32(q: Tensor, k: Tensor, v: Tensor, H: int, scale: float, dh: int, *, tile: int = 64, fault: str = ""):
    """An fp32 emulation of a flash loop over ``tile``-key tiles with the header's rounding points (S fp32, integer row offset
    M = ceil of the running maximum, P = exp2(fma(S, c, -M)), l sums the un-rounded P, O = bf16((bf16(P) @ V) / l)), on the CPU.
    ``fault`` plants one defect a kernel of this structure can have:
      drop_key   the last key never enters;           pad_slot   one slot past Tk of the ragged tile is live, V^T pad 1024;
      row_off    every row stored one place down;     skip_tile  the second key tile is skipped (needs Tk > tile)."""
    B, Tq, D = q.shape
    Tk = k.shape[1]
    c = torch.tensor(attn_c(scale), dtype=torch.float32)
    qh, kh, vh = (t.reshape(B, -1, H, dh).transpose(1, 2).float() for t in (q, k, v))
    if fault == "drop_key":
        kh, vh, Tk = kh[:, :, :-1], vh[:, :, :-1], Tk - 1
    if fault == "pad_slot":
        kh = torch.cat([kh, kh[:, :, -1:]], 2)
        vh = torch.cat([vh, torch.full_like(vh[:, :, -1:], 1024.0)], 2)
        Tk += 1
    m = torch.full((B, H, Tq, 1), -1e30)
    l = torch.zeros(B, H, Tq, 1)
    o = torch.zeros(B, H, Tq, dh)
    for ti, t0 in enumerate(range(0, Tk, tile)):
        if fault == "skip_tile" and ti == 1:
            continue
        s = qh @ kh[:, :, t0:t0 + tile].transpose(-1, -2)
        m_new = torch.maximum(m, torch.ceil((s * c).amax(-1, keepdim=True)))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(torch.addcmul(-m_new, s, c))
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(BF).float() @ vh[:, :, t0:t0 + tile]
        m = m_new
    out = (o / l).to(BF).transpose(1, 2).reshape(B, Tq, D)
    if fault == "row_off":
        out = torch.roll(out, 1, dims=1)
    return out
