"""Test-side restatement of spatio-temporal guidance (STG) on top of the CPU oracle (oracle/dit.py), which has none.

* ``ltx_forward_stg``: ``oracle.dit.ltx_forward`` in which, for the batch rows in ``rows`` and the blocks in ``blocks``
  (None = every block), the video self-attention (``transformer_blocks.{i}.attn1``) returns its value projection v in place
  of sdpa(q, k, v) - the upstream LTX-2 meaning of PerturbationType.SKIP_VIDEO_SELF_ATTN.  It is composed from the oracle's
  own functions: ``oracle.dit.attention`` is wrapped for the duration of the call and, for a perturbed block, runs with
  ``oracle.dit.sdpa`` replaced by one that hands v back for the perturbed rows.  Nothing under oracle/ is edited.
* ``stg_combine``: the velocity-space guidance with the rounding points of ltxk_guided_euler_step.
* ``denoise_dev_stg``: ``oracle.dit.denoise_dev`` (compiled form) with the perturbed forward and ``stg_combine``."""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import torch

from oracle import dit as O


@contextlib.contextmanager
def skip_self_attention(rows: Sequence[int], blocks: Optional[Sequence[int]]):
    """Inside the block: O.attention of a perturbed block's attn1 returns to_out(v) for the batch rows in ``rows``."""
    rows = set(int(r) for r in rows)
    perturbed = None if blocks is None else {f"transformer_blocks.{int(i)}.attn1" for i in blocks}
    attention, sdpa = O.attention, O.sdpa

    def passthrough_sdpa(q, k, v, heads, p):
        o = sdpa(q, k, v, heads, p)
        for r in rows:
            o[r] = p.r(v[r].to(p.dtype))
        return o

    def attention_stg(x, W, prefix, heads, p, context=None, pe=None, eps=1e-6, taps=None, tag=""):
        hit = context is None and prefix.endswith(".attn1") and (perturbed is None or prefix in perturbed)
        if not hit:
            return attention(x, W, prefix, heads, p, context=context, pe=pe, eps=eps, taps=taps, tag=tag)
        O.sdpa = passthrough_sdpa
        try:
            return attention(x, W, prefix, heads, p, context=context, pe=pe, eps=eps, taps=taps, tag=tag)
        finally:
            O.sdpa = sdpa

    O.attention = attention_stg
    try:
        yield
    finally:
        O.attention, O.sdpa = attention, sdpa


def ltx_forward_stg(latent, timesteps, context, pe, W, cfg, p, rows: Sequence[int], blocks: Optional[Sequence[int]]):
    """O.ltx_forward with the video self-attention of ``blocks`` skipped in batch rows ``rows``."""
    with skip_self_attention(rows, blocks):
        return O.ltx_forward(latent, timesteps, context, pe, W, cfg, p)


def stg_combine(v_pos, v_neg, v_pert, cfg_scale: float, stg_scale: float, p):
    """g = v+ (+ CFG, exactly oracle.dit.cfg_combine); v = r(g + r(stg * r(v+ - vp)))."""
    g = O.cfg_combine(v_pos, v_neg, cfg_scale, p) if v_neg is not None else v_pos
    return p.r(g + p.r(stg_scale * p.r(v_pos - v_pert)))


def denoise_dev_stg(latents, positions, ctx_pos, ctx_neg, W, cfg, sigmas, p, cfg_scale: float, stg_scale: float,
                    stg_blocks: Optional[Sequence[int]], clean_latent=None, denoise_mask=None):
    """O.denoise_dev(compiled=True) with STG: per step v+, v- (cfg_scale != 1) and the perturbed v+ (all its rows skip the
    self-attention of ``stg_blocks``), combined by ``stg_combine``; x0, mask blend and Euler as the oracle's loop."""
    b, c, f, h, w = latents.shape
    n = f * h * w
    pe = O.precompute_freqs_cis(torch.from_numpy(positions), cfg.dim, cfg.theta, cfg.max_pos, cfg.heads)
    if denoise_mask is not None:
        mask_tok = denoise_mask.reshape(b, 1, f, 1, 1).expand(b, 1, f, h, w).reshape(b, n)
    else:
        mask_tok = torch.ones(b, n)
    x = p.r(latents)
    for i in range(len(sigmas) - 1):
        s_m, sn_m = O.bf16_round_scalar(float(sigmas[i])), O.bf16_round_scalar(float(sigmas[i + 1]))
        tok = O.latent_to_tokens(x)
        ts = p.r(s_m * mask_tok)
        vp = O.ltx_forward(tok, ts, ctx_pos, pe, W, cfg, p)
        vn = O.ltx_forward(tok, ts, ctx_neg, pe, W, cfg, p) if cfg_scale != 1.0 else None
        vq = ltx_forward_stg(tok, ts, ctx_pos, pe, W, cfg, p, range(b), stg_blocks)
        v = stg_combine(vp, vn, vq, cfg_scale, stg_scale, p)
        vel = O.tokens_to_latent(v, x.shape)
        x0 = O.to_denoised(x, vel, s_m, p)
        if denoise_mask is not None:
            x0 = O.apply_denoise_mask(x0, p.r(clean_latent), p.r(denoise_mask), p)
        x = p.r(x0 + sn_m * (x - x0) / s_m)
    return x
