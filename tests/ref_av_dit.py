"""Test-side restatement of the AudioVideo transformer and the joint denoise loop (mlx_video/models/ltx/transformer.py:221-361,
ltx.py:161-247, generate.py:1330-1680), written from the reference's source out of oracle.dit's pieces and generic in ``Prec``.
Nothing here touches a device.

Weights are three dicts with the module keys the device models read: the video set and the audio set (``oracle.dit.make_weights``
of each config - the audio tensors under the video names, as ``weights.audio_transformer_weights`` delivers them) and the cross
set (``audio_to_video_attn.*``, ``video_to_audio_attn.*``, ``scale_shift_table_a2v_ca_*``, the four ``av_ca_*`` AdaLN-singles).

``fault``: a planted mistake, for the tests that show the yardstick sees it -
  "v2a_post_a2v": v2a reads the video stream AFTER a2v updated it;  "swap_scale_shift": scale and shift rows of the 5-row table
  swapped;  "k_pe_is_pe": the key side rotated with the query side's table."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from oracle import dit as O

Tensor = torch.Tensor
CROSS_ADALN = {"av_ca_video_scale_shift_adaln_single": ("v", 4), "av_ca_audio_scale_shift_adaln_single": ("a", 4),
               "av_ca_a2v_gate_adaln_single": ("v", 1), "av_ca_v2a_gate_adaln_single": ("a", 1)}


def make_av_weights(cfg_v: O.DiTConfig, cfg_a: O.DiTConfig, seed: int = 7, dtype=torch.bfloat16,
                    ) -> Tuple[Dict[str, Tensor], Dict[str, Tensor], Dict[str, Tensor]]:
    """(video set, audio set, cross set).  The video and audio sets have oracle.dit.make_weights' distributions.  The cross set is
    drawn so that the cross-modal path carries weight in the result, as it does in a trained model - with every tensor at
    N(0, 0.02^2) the gate is ~0.03 and a wrong cross section moves the velocity by less than one bf16 evaluation's own error,
    which no test could see: the 5-row tables are N(0, 0.5^2) with the gate row around 1, to_v / to_out are N(0, 0.06^2), and
    the q/k-norm weights are 1.5 + 0.1 N(0,1) (logits a few units wide, so the rotation tables matter).  The planted-fault test
    of test_av_dit_cpu.py shows that each mistake it plants then moves both velocities by more than 10 policy errors."""
    assert cfg_v.num_layers == cfg_a.num_layers
    Wv, Wa = O.make_weights(cfg_v, seed, dtype), O.make_weights(cfg_a, seed + 1, dtype)
    g = torch.Generator().manual_seed(seed + 2)
    Dv, Da = cfg_v.dim, cfg_a.dim
    Wc: Dict[str, Tensor] = {}

    def lin(name, out_f, in_f):
        Wc[f"{name}.weight"] = (torch.randn(out_f, in_f, generator=g) * 0.02).to(dtype)
        Wc[f"{name}.bias"] = (torch.randn(out_f, generator=g) * 0.01).to(dtype)

    for mod, (side, coeff) in CROSS_ADALN.items():
        D = Dv if side == "v" else Da
        lin(f"{mod}.emb.timestep_embedder.linear1", D, 256)
        lin(f"{mod}.emb.timestep_embedder.linear2", D, D)
        lin(f"{mod}.linear", coeff * D, D)
    for i in range(cfg_v.num_layers):
        pre = f"transformer_blocks.{i}"
        for name, dq, dkv in (("audio_to_video_attn", Dv, Da), ("video_to_audio_attn", Da, Dv)):
            lin(f"{pre}.{name}.to_q", Da, dq)
            lin(f"{pre}.{name}.to_k", Da, dkv)
            lin(f"{pre}.{name}.to_v", Da, dkv)
            lin(f"{pre}.{name}.to_out", dq, Da)
            for nm in ("to_v", "to_out"):
                Wc[f"{pre}.{name}.{nm}.weight"] = (Wc[f"{pre}.{name}.{nm}.weight"].float() * 3.0).to(dtype)
            Wc[f"{pre}.{name}.q_norm.weight"] = (1.5 + 0.1 * torch.randn(Da, generator=g)).to(dtype)
            Wc[f"{pre}.{name}.k_norm.weight"] = (1.5 + 0.1 * torch.randn(Da, generator=g)).to(dtype)
        for side, D in (("video", Dv), ("audio", Da)):
            t = torch.randn(5, D, generator=g) * 0.5
            t[4] += 1.0
            Wc[f"{pre}.scale_shift_table_a2v_ca_{side}"] = t.to(dtype)
    return Wv, Wa, Wc


def zero_cross_out(Wc: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """The cross set with every cross-modal to_out weight and bias zero: the two streams no longer see each other."""
    return {k: (torch.zeros_like(v) if ("_attn.to_out." in k) else v) for k, v in Wc.items()}


def cross_freqs_cis(positions: Tensor, cfg_v: O.DiTConfig, cfg_a: O.DiTConfig, heads: int) -> Tuple[Tensor, Tensor]:
    """ltx.py:207-213: one axis from positions[:, 0:1], dim = audio inner dim, max_pos = max of the first entries."""
    return O.precompute_freqs_cis(positions[:, 0:1], cfg_a.dim, cfg_a.theta, (max(cfg_v.max_pos[0], cfg_a.max_pos[0]),), heads)


def attention_kpe(x: Tensor, W: Dict[str, Tensor], prefix: str, heads: int, p: O.Prec, context: Tensor, pe, k_pe, eps: float) -> Tensor:
    """attention.py:102-142 with a separate table for the keys."""
    q = O.linear(x, W[f"{prefix}.to_q.weight"], W[f"{prefix}.to_q.bias"], p)
    k = O.linear(context, W[f"{prefix}.to_k.weight"], W[f"{prefix}.to_k.bias"], p)
    v = O.linear(context, W[f"{prefix}.to_v.weight"], W[f"{prefix}.to_v.bias"], p)
    q = O.rms_norm(q, p, eps, W[f"{prefix}.q_norm.weight"])
    k = O.rms_norm(k, p, eps, W[f"{prefix}.k_norm.weight"])
    q = O.apply_split_rotary_emb(q, pe[0], pe[1], p)
    k = O.apply_split_rotary_emb(k, k_pe[0], k_pe[1], p)
    o = O.sdpa(q, k, v, heads, p)
    return O.linear(o, W[f"{prefix}.to_out.weight"], W[f"{prefix}.to_out.bias"], p)


def _av_ca_ada_values(table: Tensor, ss_ts: Tensor, gate_ts: Tensor, p: O.Prec):
    """transformer.py:179-219: (scale1, shift1, scale2, shift2, gate)."""
    return O.ada_values(table[:4], ss_ts, 0, 4, p) + O.ada_values(table[4:], gate_ts, 0, 1, p)


class _Stream:
    """One modality's TransformerArgs (ltx.py:129-158, 201-228)."""

    def __init__(self, latent, timesteps, context, pe, cross_pe, W, Wc, cfg: O.DiTConfig, p: O.Prec, ss_mod: str, gate_mod: str,
                 av_ca_factor: float):
        latent, context = p.r(latent), p.r(context)
        b, n, _ = latent.shape
        self.b, self.n, self.W, self.cfg = b, n, W, cfg
        self.x = O.linear(latent, W["patchify_proj.weight"], W["patchify_proj.bias"], p)
        t = p.r(p.r(timesteps) * cfg.timestep_scale_multiplier)
        ss, emb = O.adaln_single(t.reshape(-1), W, "adaln_single", p)
        self.ts, self.emb = ss.reshape(b, n, -1), emb.reshape(b, n, -1)
        ctx = O.linear(context, W["caption_projection.linear1.weight"], W["caption_projection.linear1.bias"], p)
        ctx = O.linear(O.gelu_tanh(ctx, p), W["caption_projection.linear2.weight"], W["caption_projection.linear2.bias"], p)
        self.ctx = ctx.reshape(b, -1, self.x.shape[-1])
        self.pe = tuple(c.expand(b, *c.shape[1:]) if c.shape[0] != b else c for c in pe)
        self.cross_pe = tuple(c.expand(b, *c.shape[1:]) if c.shape[0] != b else c for c in cross_pe)
        # ltx.py:230-247: scale-shift from the timestep, the gate from timestep * av_ca_factor (a bf16 product)
        self.cross_ss = O.adaln_single(t.reshape(-1), Wc, ss_mod, p)[0].reshape(b, n, -1)
        self.cross_gate = O.adaln_single(p.r(t.reshape(-1) * av_ca_factor), Wc, gate_mod, p)[0].reshape(b, n, -1)

    def attn(self, i: int, p: O.Prec) -> None:
        """transformer.py:247-278: self-attention and text attention of block i."""
        pre, cfg, W = f"transformer_blocks.{i}", self.cfg, self.W
        shift, scale, gate = O.ada_values(W[f"{pre}.scale_shift_table"], self.ts, 0, 3, p)
        nx = O.modulate(O.rms_norm(self.x, p, cfg.norm_eps), scale, shift, p)
        x = p.r(self.x + p.r(O.attention(nx, W, f"{pre}.attn1", cfg.heads, p, pe=self.pe, eps=cfg.norm_eps) * gate))
        self.x = p.r(x + O.attention(O.rms_norm(x, p, cfg.norm_eps), W, f"{pre}.attn2", cfg.heads, p, context=self.ctx, eps=cfg.norm_eps))

    def ff(self, i: int, p: O.Prec) -> None:
        pre, cfg, W = f"transformer_blocks.{i}", self.cfg, self.W
        shift, scale, gate = O.ada_values(W[f"{pre}.scale_shift_table"], self.ts, 3, 6, p)
        nx = O.modulate(O.rms_norm(self.x, p, cfg.norm_eps), scale, shift, p)
        self.x = p.r(self.x + p.r(O.feed_forward(nx, W, f"{pre}.ff", p) * gate))

    def head(self, p: O.Prec) -> Tensor:
        W, cfg = self.W, self.cfg
        tab = W["scale_shift_table"].to(p.dtype)
        shift, scale = p.r(tab[0][None, None, :] + self.emb), p.r(tab[1][None, None, :] + self.emb)
        x = O.modulate(O.layer_norm_noaffine(self.x, p, cfg.norm_eps), scale, shift, p)
        return O.linear(x, W["proj_out.weight"], W["proj_out.bias"], p)


def av_forward(vlat: Tensor, vts: Tensor, vctx: Tensor, vpe, vcpe, alat: Tensor, ats: Tensor, actx: Tensor, ape, acpe,
               Wv, Wa, Wc, cfg_v: O.DiTConfig, cfg_a: O.DiTConfig, p: O.Prec, return_hidden: bool = False,
               fault: Optional[str] = None, av_ca_timestep_scale_multiplier: float = 1000.0):
    """LTXModel.__call__(video, audio) of the AudioVideo model.  *lat (B,T,128), *ts (B,T), *ctx (B,S,C), *pe the main table,
    *cpe the cross table (``cross_freqs_cis``).  Returns (video velocity, audio velocity[, video hidden, audio hidden])."""
    eps = cfg_v.norm_eps
    v = _Stream(vlat, vts, vctx, vpe, vcpe, Wv, Wc, cfg_v, p, "av_ca_video_scale_shift_adaln_single", "av_ca_a2v_gate_adaln_single",
                av_ca_timestep_scale_multiplier / cfg_v.timestep_scale_multiplier)
    a = _Stream(alat, ats, actx, ape, acpe, Wa, Wc, cfg_a, p, "av_ca_audio_scale_shift_adaln_single", "av_ca_v2a_gate_adaln_single",
                av_ca_timestep_scale_multiplier / cfg_a.timestep_scale_multiplier)
    hv, ha = [], []
    for i in range(cfg_v.num_layers):
        pre = f"transformer_blocks.{i}"
        v.attn(i, p)
        a.attn(i, p)
        # transformer.py:281-339
        vn, an = O.rms_norm(v.x, p, eps), O.rms_norm(a.x, p, eps)
        sc_a_a2v, sh_a_a2v, sc_a_v2a, sh_a_v2a, gate_v2a = _av_ca_ada_values(Wc[f"{pre}.scale_shift_table_a2v_ca_audio"], a.cross_ss, a.cross_gate, p)
        sc_v_a2v, sh_v_a2v, sc_v_v2a, sh_v_v2a, gate_a2v = _av_ca_ada_values(Wc[f"{pre}.scale_shift_table_a2v_ca_video"], v.cross_ss, v.cross_gate, p)
        if fault == "swap_scale_shift":
            sc_a_a2v, sh_a_a2v, sc_a_v2a, sh_a_v2a = sh_a_a2v, sc_a_a2v, sh_a_v2a, sc_a_v2a
            sc_v_a2v, sh_v_a2v, sc_v_v2a, sh_v_v2a = sh_v_a2v, sc_v_a2v, sh_v_v2a, sc_v_v2a
        k_pe_a2v, k_pe_v2a = a.cross_pe, v.cross_pe
        if fault == "k_pe_is_pe":      # key t rotated with row t of the QUERY side's table (its last row past the end)
            rows = lambda pe, T: tuple(c[:, :, torch.arange(T).clamp_max(c.shape[2] - 1)] for c in pe)
            k_pe_a2v, k_pe_v2a = rows(v.cross_pe, a.n), rows(a.cross_pe, v.n)
        vq, ak = O.modulate(vn, sc_v_a2v, sh_v_a2v, p), O.modulate(an, sc_a_a2v, sh_a_a2v, p)
        v.x = p.r(v.x + p.r(attention_kpe(vq, Wc, f"{pre}.audio_to_video_attn", cfg_a.heads, p, ak, v.cross_pe, k_pe_a2v, eps) * gate_a2v))
        if fault == "v2a_post_a2v":
            vn = O.rms_norm(v.x, p, eps)
        aq, vk = O.modulate(an, sc_a_v2a, sh_a_v2a, p), O.modulate(vn, sc_v_v2a, sh_v_v2a, p)
        a.x = p.r(a.x + p.r(attention_kpe(aq, Wc, f"{pre}.video_to_audio_attn", cfg_a.heads, p, vk, a.cross_pe, k_pe_v2a, eps) * gate_v2a))
        v.ff(i, p)
        a.ff(i, p)
        hv.append(v.x)
        ha.append(a.x)
    out = (v.head(p), a.head(p))
    return out + (hv, ha) if return_hidden else out


def audio_tokens(lat: Tensor) -> Tensor:
    """generate.py:1440-1441: (B,8,T,16) -> (B,T,128)."""
    b, c, t, f = lat.shape
    return lat.permute(0, 2, 1, 3).reshape(b, t, c * f)


def denoise_dev_av(vlat: Tensor, alat: Tensor, vpos: Tensor, apos: Tensor, vctx_pos, vctx_neg, actx_pos, actx_neg, Wv, Wa, Wc,
                   cfg_v: O.DiTConfig, cfg_a: O.DiTConfig, sig, p: O.Prec, cfg_scale: float = 4.0, compiled: bool = False,
                   clean_latent: Optional[Tensor] = None, denoise_mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """generate.py:1330-1680: both modalities share sigma, the audio timestep mask is all ones, CFG on both velocities with each
    modality's own context pair, x0 with the bf16 sigma, Euler with the Python floats (``compiled``: the bf16 sigmas)."""
    b, c, f, h, w = vlat.shape
    n = f * h * w
    ab, ac, at, af = alat.shape
    vpe = O.precompute_freqs_cis(vpos, cfg_v.dim, cfg_v.theta, cfg_v.max_pos, cfg_v.heads)
    ape = O.precompute_freqs_cis(apos, cfg_a.dim, cfg_a.theta, cfg_a.max_pos, cfg_a.heads)
    vcpe, acpe = cross_freqs_cis(vpos, cfg_v, cfg_a, cfg_v.heads), cross_freqs_cis(apos, cfg_v, cfg_a, cfg_a.heads)
    mask_tok = torch.ones(b, n) if denoise_mask is None else denoise_mask.reshape(b, 1, f, 1, 1).expand(b, 1, f, h, w).reshape(b, n)
    xv, xa = p.r(vlat), p.r(alat)
    for i in range(len(sig) - 1):
        s, s_next = float(sig[i]), float(sig[i + 1])
        s_m = O.bf16_round_scalar(s) if p.emulate_bf16 else s
        sn_m = O.bf16_round_scalar(s_next) if p.emulate_bf16 else s_next
        vtok, atok = O.latent_to_tokens(xv), audio_tokens(xa)
        vts, ats = p.r(s_m * mask_tok), torch.full((ab, at), s_m)
        fw = lambda cv_, ca_: av_forward(vtok, vts, cv_, vpe, vcpe, atok, ats, ca_, ape, acpe, Wv, Wa, Wc, cfg_v, cfg_a, p)
        vv, va = fw(vctx_pos, actx_pos)
        if cfg_scale != 1.0:
            nv, na = fw(vctx_neg, actx_neg)
            vv, va = O.cfg_combine(vv, nv, cfg_scale, p), O.cfg_combine(va, na, cfg_scale, p)
        vvel = O.tokens_to_latent(vv, xv.shape)
        avel = va.reshape(ab, at, ac, af).permute(0, 2, 1, 3)
        v0, a0 = O.to_denoised(xv, vvel, s_m, p), O.to_denoised(xa, avel, s_m, p)
        if denoise_mask is not None:
            v0 = O.apply_denoise_mask(v0, p.r(clean_latent), p.r(denoise_mask), p)
        if compiled:
            xv, xa = p.r(v0 + sn_m * (xv - v0) / s_m), p.r(a0 + sn_m * (xa - a0) / s_m)
        else:
            xv, xa = O.euler_step(xv, v0, s, s_next, p), O.euler_step(xa, a0, s, s_next, p)
    return xv, xa
