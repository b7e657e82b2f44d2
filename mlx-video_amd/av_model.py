"""The AudioVideo transformer of joint denoising (mlx_video/models/ltx/ltx.py:161-247,318-336, transformer.py:281-339).

Two ``LTXModel``s - the video transformer and the audio transformer (``LTXModelConfig.audio()``) of one joint checkpoint, each
with its own packed panels - whose blocks exchange information through two cross-modal attentions at head dim 64:
a2v (queries from the video stream, keys / values from the audio stream) and v2a (the mirror image).  ``LTXAVModel`` adds the
cross-modal panels and runs the two forwards block by block through ``LTXModel``'s stage methods:

    prepare both -> per block { video self + text attention; audio self + text attention; a2v; v2a; video ff; audio ff } -> heads

Per block the cross section normalises each residual stream ONCE and modulates it twice (``ops.rmsnorm_modulate(scale2=...)``,
one launch per stream); both normalised pairs are taken before either stream is updated, so v2a reads the pre-a2v video
stream.  The modulation rows come from a per-block (5, D) table in the order (scale_a2v, shift_a2v, scale_v2a, shift_v2a,
gate) - scale first, unlike the main table - combined with four more AdaLN-singles: scale-shift (U, 4D) and gate (U, D) per
modality, concatenated to (U, 5D).  The cross positional tables have one axis (time in seconds, max_pos 20, dim = the audio
inner dim), (H, T, 32) per modality.  DESIGN.md §5o."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .ltx_model import BF16, Linear, LTXModel, LTXModelConfig, TimestepPlan, _freqs_cis_one_axis, _vt_buffer

_ADALN = ("emb.timestep_embedder.linear1", "emb.timestep_embedder.linear2", "linear")
# module -> (which inner dim, embedding coefficient)
_CROSS_ADALN = {"av_ca_video_scale_shift_adaln_single": ("v", 4), "av_ca_audio_scale_shift_adaln_single": ("a", 4),
                "av_ca_a2v_gate_adaln_single": ("v", 1), "av_ca_v2a_gate_adaln_single": ("a", 1)}
_CROSS_ATTN = ("audio_to_video_attn", "video_to_audio_attn")


class _CrossAttn:
    # Linear: to_q, k|v (one (2*Da, K) panel) and to_out; the q/k-norm weights (Da each)
    __slots__ = ("q", "kv", "o", "wqn", "wkn")


class _AdaLN:
    __slots__ = ("t1", "t2", "lin")


class LTXAVModel:
    """``model.forward_tokens(...) -> (video velocity (B,N,128), audio velocity (B,Ta,128))``."""

    def __init__(self, video: LTXModel, audio: LTXModel, cross_weights: Dict[str, torch.Tensor],
                 av_ca_timestep_scale_multiplier: int = 1000):
        cv, ca = video.config, audio.config
        if cv.attention_head_dim != 128 or ca.attention_head_dim != 64:
            raise ValueError("LTXAVModel: `video` is the head-dim-128 model, `audio` the head-dim-64 one (LTXModelConfig.audio())")
        if cv.num_layers != ca.num_layers:
            raise ValueError(f"LTXAVModel: the video model has {cv.num_layers} blocks, the audio model {ca.num_layers}")
        if video.weight_dtype != BF16 or audio.weight_dtype != BF16 or video.fp8_activations or audio.fp8_activations:
            raise ValueError("LTXAVModel: joint denoising runs on bf16 sub-models (no fp8 or MXFP4 weights, no fp8 activations)")
        if video.num_attention_heads != audio.num_attention_heads:
            # the reference builds the video cross table with the VIDEO head count and applies it to a q of AUDIO heads
            raise ValueError(f"LTXAVModel: the cross-modal attentions need one head count, got video {video.num_attention_heads}, "
                             f"audio {audio.num_attention_heads}")
        if cv.norm_eps != ca.norm_eps or cv.positional_embedding_theta != ca.positional_embedding_theta:
            raise ValueError("LTXAVModel: the two sub-models disagree on norm_eps / positional_embedding_theta")
        # The gate AdaLNs take timestep * av_ca_timestep_scale_multiplier / timestep_scale_multiplier (ltx.py:239-244); at the
        # config's defaults the factor is 1 and the gate AdaLN reads the very timestep projection of the scale-shift one.  Any
        # other value would need the reference's two bf16 roundings in order: refused, never computed in another arithmetic.
        for m, who in ((cv.timestep_scale_multiplier, "video"), (ca.timestep_scale_multiplier, "audio")):
            if av_ca_timestep_scale_multiplier != m:
                raise ValueError(f"LTXAVModel: av_ca_timestep_scale_multiplier = {av_ca_timestep_scale_multiplier} differs from the "
                                 f"{who} timestep_scale_multiplier = {m}; only a gate timestep factor of 1 is implemented")
        self.video, self.audio = video, audio
        self.av_ca_timestep_scale_multiplier = av_ca_timestep_scale_multiplier
        self.cross_pe_max_pos = float(max(cv.positional_embedding_max_pos[0], ca.positional_embedding_max_pos[0]))
        # one launch per stream for the two cross modulations (ltxk_rmsnorm_modulate2); False: two single launches - the same bits
        self.modulate2 = True
        self._pack(cross_weights)

    # ------------------------------------------------------------------ weights
    @staticmethod
    def expected_cross_keys(cfg_v: LTXModelConfig, cfg_a: LTXModelConfig) -> List[str]:
        keys = []
        for mod in _CROSS_ADALN:
            for n in _ADALN:
                keys += [f"{mod}.{n}.weight", f"{mod}.{n}.bias"]
        for i in range(cfg_v.num_layers):
            pre = f"transformer_blocks.{i}"
            for a in _CROSS_ATTN:
                for nm in ("to_q", "to_k", "to_v", "to_out"):
                    keys += [f"{pre}.{a}.{nm}.weight", f"{pre}.{a}.{nm}.bias"]
                keys += [f"{pre}.{a}.q_norm.weight", f"{pre}.{a}.k_norm.weight"]
            keys += [f"{pre}.scale_shift_table_a2v_ca_video", f"{pre}.scale_shift_table_a2v_ca_audio"]
        return keys

    def _pack(self, W: Dict[str, torch.Tensor]) -> None:
        cv, ca = self.video.config, self.audio.config
        Dv, Da = cv.inner_dim, ca.inner_dim
        missing = [k for k in self.expected_cross_keys(cv, ca) if k not in W]
        if missing:
            raise ValueError(f"Missing {len(missing)} cross-modal parameters in checkpoint, e.g. {missing[:4]}")

        def g(k, shape):
            t = W[k]
            if t.dtype != BF16 or not t.is_cuda:
                raise TypeError(f"weight {k}: expected a bf16 device tensor")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"weight {k}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
            return t.contiguous()

        def lin(name, o, i):
            return Linear(g(f"{name}.weight", (o, i)), None, g(f"{name}.bias", (o,)))

        self.adaln: Dict[str, _AdaLN] = {}
        for mod, (side, coeff) in _CROSS_ADALN.items():
            D = Dv if side == "v" else Da
            a = _AdaLN()
            a.t1, a.t2, a.lin = lin(f"{mod}.{_ADALN[0]}", D, 256), lin(f"{mod}.{_ADALN[1]}", D, D), lin(f"{mod}.{_ADALN[2]}", coeff * D, D)
            self.adaln[mod] = a
        self.a2v: List[_CrossAttn] = []
        self.v2a: List[_CrossAttn] = []
        tv, ta = [], []
        for i in range(cv.num_layers):
            pre = f"transformer_blocks.{i}"
            for name, dst, dq, dkv in (("audio_to_video_attn", self.a2v, Dv, Da), ("video_to_audio_attn", self.v2a, Da, Dv)):
                c = _CrossAttn()
                c.q = lin(f"{pre}.{name}.to_q", Da, dq)
                c.kv = Linear.cat([lin(f"{pre}.{name}.to_k", Da, dkv), lin(f"{pre}.{name}.to_v", Da, dkv)])     # k | V^T, one launch
                c.o = lin(f"{pre}.{name}.to_out", dq, Da)
                c.wqn, c.wkn = g(f"{pre}.{name}.q_norm.weight", (Da,)), g(f"{pre}.{name}.k_norm.weight", (Da,))
                dst.append(c)
            tv.append(g(f"{pre}.scale_shift_table_a2v_ca_video", (5, Dv)))
            ta.append(g(f"{pre}.scale_shift_table_a2v_ca_audio", (5, Da)))
        self.tables_v = torch.stack(tv, 0).contiguous()      # (L,5,Dv): scale_a2v, shift_a2v, scale_v2a, shift_v2a, gate
        self.tables_a = torch.stack(ta, 0).contiguous()      # (L,5,Da)

    def cross_weight_bytes(self) -> int:
        """Device bytes of the cross-modal part: the four AdaLN-singles, both attentions of every block, the (L,5,D) tables."""
        lins = [l for a in self.adaln.values() for l in (a.t1, a.t2, a.lin)] + [l for c in self.a2v + self.v2a for l in (c.q, c.kv, c.o)]
        held = [t for l in lins for t in (l.w, l.bias)] + [t for c in self.a2v + self.v2a for t in (c.wqn, c.wkn)]
        return sum(t.numel() * t.element_size() for t in held + [self.tables_v, self.tables_a])

    def weight_bytes(self) -> Dict[str, int]:
        """Device bytes of the three parts: {"video", "audio", "cross"}."""
        return {"video": self.video.weight_bytes(), "audio": self.audio.weight_bytes(), "cross": self.cross_weight_bytes()}

    @staticmethod
    def random_cross_weights(cfg_v: LTXModelConfig, cfg_a: LTXModelConfig, device, seed: int = 4321) -> Dict[str, torch.Tensor]:
        """Random cross-modal tensors in ``LTXModel.random_weights``' distributions, module-name keys."""
        g = torch.Generator(device=device).manual_seed(seed)
        Dv, Da = cfg_v.inner_dim, cfg_a.inner_dim
        W: Dict[str, torch.Tensor] = {}

        def rn(*shape, std=1.0, mean=0.0):
            return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * std + mean).to(BF16)

        def lin(name, o, i):
            W[f"{name}.weight"] = rn(o, i, std=0.02)
            W[f"{name}.bias"] = rn(o, std=0.01)

        for mod, (side, coeff) in _CROSS_ADALN.items():
            D = Dv if side == "v" else Da
            lin(f"{mod}.{_ADALN[0]}", D, 256)
            lin(f"{mod}.{_ADALN[1]}", D, D)
            lin(f"{mod}.{_ADALN[2]}", coeff * D, D)
        for i in range(cfg_v.num_layers):
            pre = f"transformer_blocks.{i}"
            for name, dq, dkv in (("audio_to_video_attn", Dv, Da), ("video_to_audio_attn", Da, Dv)):
                lin(f"{pre}.{name}.to_q", Da, dq)
                lin(f"{pre}.{name}.to_k", Da, dkv)
                lin(f"{pre}.{name}.to_v", Da, dkv)
                lin(f"{pre}.{name}.to_out", dq, Da)
                W[f"{pre}.{name}.q_norm.weight"] = rn(Da, std=0.1, mean=1.0)
                W[f"{pre}.{name}.k_norm.weight"] = rn(Da, std=0.1, mean=1.0)
            W[f"{pre}.scale_shift_table_a2v_ca_video"] = rn(5, Dv, std=0.02)
            W[f"{pre}.scale_shift_table_a2v_ca_audio"] = rn(5, Da, std=0.02)
        return W

    @classmethod
    def random_init(cls, cfg_v: LTXModelConfig, cfg_a: LTXModelConfig, device, seed: int = 1234, fuse: int = 15) -> "LTXAVModel":
        return cls(LTXModel.random_init(cfg_v, device, seed, fuse), LTXModel.random_init(cfg_a, device, seed + 1, fuse),
                   cls.random_cross_weights(cfg_v, cfg_a, device, seed + 2))

    # ------------------------------------------------------------------ forward
    def cross_freqs_cis(self, positions: torch.Tensor, heads: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The cross positional table of one modality (ltx.py:207-213): ONE axis built from positions[:, 0:1] (time in seconds),
        dim = the audio inner dim, max_pos = max of the two modalities' first entries, middle-indices grid.  cos, sin
        (B, heads, T, Da/heads/2).  Host arithmetic, once per loop, like the main one-axis table."""
        return _freqs_cis_one_axis(positions[:, 0:1].to(torch.float32), self.audio.inner_dim, self.video.positional_embedding_theta,
                                   self.cross_pe_max_pos, heads)

    def _cross_mods(self, m: LTXModel, st, ss: _AdaLN, gate: _AdaLN, tables: torch.Tensor) -> torch.Tensor:
        """(L,U,5,D): the per-block table plus the (U,5D) row [scale-shift AdaLN (4D) | gate AdaLN (D)] of each timestep row."""
        D = m.inner_dim
        parts = []
        for a in (ss, gate):
            h = m._linear(st.tproj, a.t1, epilogue=ops.EPI_BIAS_SILU)
            parts.append(m._linear(ops.silu(m._linear(h, a.t2)), a.lin))
        ada = torch.cat(parts, 1)                                    # (U, 4D | D)
        return ops.ada_combine(tables, ada, tables.shape[0], st.U, 5, D, one_plus_mask=0b00101 if m.fuse & 2 else 0)

    def _modulate_twice(self, m: LTXModel, st, mod: torch.Tensor, out0: torch.Tensor, out1: torch.Tensor) -> None:
        """out0 / out1 = rms_norm(st.x) under the a2v / the v2a modulation rows of ``mod`` (U,5,D)."""
        eps, ms, fs = m.config.norm_eps, 5 * m.inner_dim, bool(m.fuse & 2)
        if self.modulate2:
            ops.rmsnorm_modulate(st.x, eps, mod[:, 0], mod[:, 1], ms, st.tok2row, out=out0, sumsq=st.s_x, scale_is_one_plus=fs,
                                 scale2=mod[:, 2], shift2=mod[:, 3], out2=out1)
        else:
            ops.rmsnorm_modulate(st.x, eps, mod[:, 0], mod[:, 1], ms, st.tok2row, out=out0, sumsq=st.s_x, scale_is_one_plus=fs)
            ops.rmsnorm_modulate(st.x, eps, mod[:, 2], mod[:, 3], ms, st.tok2row, out=out1, sumsq=st.s_x, scale_is_one_plus=fs)

    def _cross_attn(self, c: _CrossAttn, mq: LTXModel, sq, mk: LTXModel, sk, nq: torch.Tensor, nk: torch.Tensor, pe_q, pe_k,
                    gate: torch.Tensor, buf) -> None:
        """One cross-modal attention (attention.py:102-142 with k_pe) onto the query stream sq.x: q from ``nq`` (the query
        stream's rows), k | V^T from ``nk`` (the key stream's rows), q/k-norm + RoPE with each side's own cross table,
        attention at head dim 64, to_out gated onto the residual stream with its row statistics."""
        Da, H, eps = self.audio.inner_dim, self.audio.num_attention_heads, self.audio.config.norm_eps
        B, Tq, Tk = sq.B, sq.N, sk.N
        q, qss, k, kss, vt, att = buf
        fs = bool(mq.fuse & mk.fuse & 2)
        mq._linear(nq, c.q, out=q, sumsq=qss if fs else None)
        if mk.fuse & 1:
            mk._linear(nk, c.kv, out=k, out2=vt, n_split=Da, out_tokens_per_batch=Tk, sumsq=kss if fs else None)
        else:
            mk._linear(nk, c.kv.rows(None, Da), out=k, sumsq=kss if fs else None)
            mk._linear(nk, c.kv.rows(Da, None), out=vt, out_tokens_per_batch=Tk)
        ops.qknorm_rope(q, 1, Da, c.wqn, pe_q[0], pe_q[1], Tq, H, eps, sumsq=qss if fs else None, head_dim=64)
        ops.qknorm_rope(k, 1, Da, c.wkn, pe_k[0], pe_k[1], Tk, H, eps, sumsq=kss if fs else None, head_dim=64)
        ops.flash_attn(q, k, vt, att, B, H, Tq, Tk, 1.0 / math.sqrt(64), head_dim=64)
        mq._linear(att, c.o, epilogue=ops.EPI_BIAS_GATE_RES, out=sq.x, resid=sq.x, gate=gate, gate_row=sq.tok2row,
                   gate_stride=5 * mq.inner_dim, sumsq=sq.s_x)

    def forward_tokens(self, video_latent: torch.Tensor, video_plan: TimestepPlan, video_context: torch.Tensor,
                       video_pe: Tuple[torch.Tensor, torch.Tensor], video_cross_pe: Tuple[torch.Tensor, torch.Tensor],
                       audio_latent: torch.Tensor, audio_plan: TimestepPlan, audio_context: torch.Tensor,
                       audio_pe: Tuple[torch.Tensor, torch.Tensor], audio_cross_pe: Tuple[torch.Tensor, torch.Tensor],
                       video_hidden: Optional[List[torch.Tensor]] = None, audio_hidden: Optional[List[torch.Tensor]] = None,
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Each modality's operands as ``LTXModel.forward_tokens`` takes them (latent (B,N,128) / (B,Ta,128), plan, context,
        main table), plus its cross table (``cross_freqs_cis``: (1|B,H,T,32) or (H,T,32), shared by every batch row).
        ``*_hidden``: lists that receive each stream's residual state after every block.  Returns the two velocities."""
        V, A = self.video, self.audio
        Da = A.inner_dim
        if video_latent.shape[0] != audio_latent.shape[0]:
            raise ValueError(f"video batch {video_latent.shape[0]} != audio batch {audio_latent.shape[0]}")
        sv = V._fwd_prepare(video_latent, video_plan, video_context, video_pe, None, None)
        sa = A._fwd_prepare(audio_latent, audio_plan, audio_context, audio_pe, None, None)
        dev = sv.x.device
        B, N, Ta = sv.B, sv.N, sa.N

        def table(pe, T):
            c, s = pe
            if c.dim() == 4:
                c, s = c[0], s[0]
            if tuple(c.shape) != (A.num_attention_heads, T, 32):
                raise ValueError(f"cross positional table must be ({A.num_attention_heads},{T},32), got {tuple(c.shape)}")
            return c.contiguous(), s.contiguous()

        cpe_v, cpe_a = table(video_cross_pe, N), table(audio_cross_pe, Ta)
        ad = self.adaln
        cm_v = self._cross_mods(V, sv, ad["av_ca_video_scale_shift_adaln_single"], ad["av_ca_a2v_gate_adaln_single"], self.tables_v)
        cm_a = self._cross_mods(A, sa, ad["av_ca_audio_scale_shift_adaln_single"], ad["av_ca_v2a_gate_adaln_single"], self.tables_a)

        def bufs(Mq, Mk, Tk):        # q, its row statistics, k, its row statistics, V^T, the attention output
            return (torch.empty((Mq, Da), dtype=BF16, device=dev), torch.empty((Mq, Da // 64), dtype=torch.float32, device=dev),
                    torch.empty((Mk, Da), dtype=BF16, device=dev), torch.empty((Mk, Da // 64), dtype=torch.float32, device=dev),
                    _vt_buffer(B, Da, tokens=Tk, device=dev), torch.empty((Mq, Da), dtype=BF16, device=dev))

        buf_a2v, buf_v2a = bufs(sv.M, sa.M, Ta), bufs(sa.M, sv.M, N)
        nv_a2v, nv_v2a = torch.empty_like(sv.x), torch.empty_like(sv.x)
        na_a2v, na_v2a = torch.empty_like(sa.x), torch.empty_like(sa.x)
        for li in range(len(V.blocks)):
            V._fwd_attn(sv, li)
            A._fwd_attn(sa, li)
            mv, ma = cm_v[li], cm_a[li]                               # (U,5,D): scale_a2v, shift_a2v, scale_v2a, shift_v2a, gate
            # both normalised pairs BEFORE either stream is updated: v2a reads the pre-a2v video stream (transformer.py:282-283)
            self._modulate_twice(V, sv, mv, nv_a2v, nv_v2a)
            self._modulate_twice(A, sa, ma, na_a2v, na_v2a)
            self._cross_attn(self.a2v[li], V, sv, A, sa, nv_a2v, na_a2v, cpe_v, cpe_a, mv[:, 4], buf_a2v)
            self._cross_attn(self.v2a[li], A, sa, V, sv, na_v2a, nv_v2a, cpe_a, cpe_v, ma[:, 4], buf_v2a)
            V._fwd_ff(sv, li)
            A._fwd_ff(sa, li)
            if video_hidden is not None:
                video_hidden.append(sv.x.reshape(B, N, V.inner_dim).clone())
            if audio_hidden is not None:
                audio_hidden.append(sa.x.reshape(B, Ta, Da).clone())
        return V._fwd_head(sv), A._fwd_head(sa)
