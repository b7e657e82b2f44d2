"""Host-side mirror of the reference's DiT seam: ``LTXModel.__call__(video: Modality, audio=None)``
(mlx_video/models/ltx/ltx.py:459-506, transformer.py:13-22,247-261,342-347).

Same names, argument meaning and error behaviour as the reference; every numeric op is a
libltxk HIP kernel (``ops``).  One modality per model: the video transformer (head dim 128, three position axes), or - the
same class at ``LTXModelConfig.audio()`` - the audio-only transformer of separate audio generation (head dim 64, one position
axis).  The cross-modal (a2v / v2a) attentions of joint denoising live in av_model.LTXAVModel, which runs two of
these models block by block through the stage methods ``_fwd_*``.

Data layout in HBM (per GPU, bf16 unless noted):
  * weights: one contiguous (out,in) matrix per Linear, with to_q|to_k of the self-attention
    packed into one (8192,4096) panel so q and k come out of one GEMM; 26 GB for L=48;
  * tokens: (B*N, 4096) row-major residual stream, updated in place by the GEMM epilogues;
  * AdaLN: instead of the reference's per-token (B,N,6*4096) tensor (63 MB at N=1280) the
    ``U`` distinct timestep rows are embedded once — (L,U,6,4096) — and every kernel indexes it
    with a (B*N) int32 token->row map.  Values are identical: each row of the reference's
    per-token GEMM depends on that token's timestep only.
  * V is produced transposed, (B, 4096, N_pad64), so attention reads it key-contiguous.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .guidance import BatchedPerturbationConfig, PerturbationType

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
MXFP4 = torch.float4_e2m1fn_x2          # ``weight_dtype`` of a model whose in-block matrices are OCP MXFP4 panels
MXSCALE_SUFFIX = "_mxscale"             # "<name>.weight" (uint8 codes) comes with "<name>.weight_mxscale" ((N, K/32) uint8 e8m0)


def is_mxfp4_weights(weights) -> bool:
    """Whether a module-key weight dict holds MXFP4 matrices (weights.quantize_transformer_weights_mxfp4)."""
    return any(k.endswith(MXSCALE_SUFFIX) for k in weights)


@dataclass(frozen=True)
class Modality:
    """transformer.py:13-22."""
    latent: torch.Tensor                 # (B,N,128)
    timesteps: torch.Tensor              # (B,N)  sigma*mask, model dtype
    positions: Optional[torch.Tensor]    # (B,3,N,2) float32
    context: torch.Tensor                # (B,S,3840)
    enabled: bool = True
    context_mask: Optional[torch.Tensor] = None
    positional_embeddings: Optional[Tuple[torch.Tensor, torch.Tensor]] = None


@dataclass
class LTXModelConfig:
    """Video half of config.py:93-129 with the constants of generate.py:2866-2881."""
    num_attention_heads: int = 32
    attention_head_dim: int = 128
    in_channels: int = 128
    out_channels: int = 128
    num_layers: int = 48
    cross_attention_dim: int = 4096
    caption_channels: int = 3840
    positional_embedding_theta: float = 10000.0
    positional_embedding_max_pos: Sequence[int] = (20, 2048, 2048)
    use_middle_indices_grid: bool = True
    rope_type: str = "split"
    double_precision_rope: bool = True
    timestep_scale_multiplier: int = 1000
    norm_eps: float = 1e-6

    @property
    def inner_dim(self) -> int:
        return self.num_attention_heads * self.attention_head_dim

    @classmethod
    def audio(cls, **overrides) -> "LTXModelConfig":
        """The audio-only transformer of the same checkpoint (config.py AudioOnly: audio_num_attention_heads 32,
        audio_attention_head_dim 64, audio_cross_attention_dim 2048, audio_positional_embedding_max_pos [20], latent
        width 128 = 8 channels x 16 mel bins): the video architecture at other sizes, with ONE position axis."""
        kw = dict(num_attention_heads=32, attention_head_dim=64, in_channels=128, out_channels=128, cross_attention_dim=2048,
                  positional_embedding_max_pos=(20,))
        kw.update(overrides)
        return cls(**kw)


@dataclass
class TimestepPlan:
    """The U distinct timestep values of a forward and the token -> row map."""
    values: torch.Tensor     # (U,) bf16
    tok2row: torch.Tensor    # (B*N,) int32

    @staticmethod
    def from_timesteps(timesteps: torch.Tensor) -> "TimestepPlan":
        vals, inv = torch.unique(timesteps.reshape(-1), sorted=True, return_inverse=True)
        return TimestepPlan(vals.to(BF16).contiguous(), inv.to(torch.int32).contiguous())


def precompute_freqs_cis(positions: torch.Tensor, dim: int, theta: float = 10000.0,
                         max_pos: Sequence[int] = (20, 2048, 2048), num_attention_heads: int = 32,
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """rope.py:364-416 -> 419-529 (SPLIT, double_precision path, middle-indices grid).
    positions (B,3,N,2) float32 on device.  Returns cos, sin (B,H,N,dim/H/2) float32.  The
    per-index frequency vector theta^linspace(0,1,n)*pi/2 (682 floats) is a host table; the
    (N x dim/2) trig table is a HIP kernel.  positions (B,1,N,2) with a one-entry ``max_pos`` (the audio transformer): the
    whole table on the host (``_freqs_cis_one_axis``)."""
    if positions.dtype == BF16:      # rope.py:433-445: warn, then compute from the (already rounded) values in float32
        import warnings
        warnings.warn("Position grid has dtype bfloat16, which causes precision loss in RoPE. "
                      "Use float32 for position grids to avoid quality degradation.", UserWarning, stacklevel=2)
    if positions.dtype != torch.float32:
        positions = positions.to(torch.float32)
    b, nd, n, two = positions.shape
    if nd not in (1, 3) or two != 2:
        raise ValueError(f"positions must be (B,3,N,2), or (B,1,N,2) for one position axis, got {tuple(positions.shape)}")
    if len(max_pos) != nd:
        raise ValueError(f"positions have {nd} axes, max_pos {len(max_pos)}")
    if nd == 1:
        return _freqs_cis_one_axis(positions, dim, theta, float(max_pos[0]), num_attention_heads)
    n_freq = max(dim // (2 * nd), 1)
    lin = torch.linspace(0.0, 1.0, n_freq, dtype=torch.float32)
    freq = (torch.pow(torch.tensor(theta, dtype=torch.float32), lin) * (math.pi / 2)).to(positions.device)
    cos_l, sin_l = [], []
    for i in range(b):
        c, s = ops.rope_table(positions[i].contiguous(), freq, num_attention_heads, dim, max_pos)
        cos_l.append(c)
        sin_l.append(s)
    return torch.stack(cos_l), torch.stack(sin_l)


def _freqs_cis_one_axis(positions: torch.Tensor, dim: int, theta: float, max_pos: float, heads: int,
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The table for ONE position axis (the audio transformer: positions (B,1,N,2) seconds, max_pos 20), on the host in the
    fp32 arithmetic of rope.py:419-529: dim/2 frequencies theta^linspace(0,1,dim/2) * pi/2 (no front pad: every slot has a
    frequency), angle = ((start + end)/2 / max_pos * 2 - 1) * freq, head h takes angles [h*dim/H/2, (h+1)*dim/H/2).
    N x dim/2 values, computed once per denoise loop (the route of text_connector.rope_table_1d): no kernel."""
    pos = positions.detach().to("cpu", torch.float32)
    half = dim // 2
    lin = torch.linspace(0.0, 1.0, half, dtype=torch.float32)
    freq = torch.pow(torch.tensor(theta, dtype=torch.float32), lin) * (math.pi / 2)
    mid = (pos[:, 0, :, 0] + pos[:, 0, :, 1]) / 2.0                       # (B,N)
    ang = ((mid / max_pos) * 2 - 1).unsqueeze(-1) * freq.reshape(1, 1, -1)      # (B,N,dim/2)
    b, n = mid.shape
    out = [f(ang).reshape(b, n, heads, half // heads).transpose(1, 2).contiguous().to(positions.device) for f in (torch.cos, torch.sin)]
    return out[0], out[1]


class Linear:
    """One Linear layer as the GEMMs read it: the (out,in) matrix ``w`` (bf16 or float8_e4m3fn), the per-output-channel fp32
    ``scale`` of an e4m3 matrix (None: a bf16 model, or an unscaled fp8 panel) and ``bias``.  An MXFP4 panel
    (weights.quantize_mxfp4) is ``w`` = the (out, in/2) uint8 codes with ``mx`` = the (out, in/32) uint8 block scales.  Holds what
    it is given: no copy."""
    __slots__ = ("w", "scale", "bias", "mx")

    def __init__(self, w: torch.Tensor, scale: Optional[torch.Tensor], bias: torch.Tensor, mx: Optional[torch.Tensor] = None):
        self.w, self.scale, self.bias, self.mx = w, scale, bias, mx

    @property
    def N(self) -> int:
        return self.w.shape[0]

    @property
    def K(self) -> int:
        return self.w.shape[1] * (2 if self.mx is not None else 1)

    def rows(self, a: Optional[int], b: Optional[int]) -> "Linear":
        """Output channels [a, b) as a Linear of views: one part of a packed panel."""
        return Linear(self.w[a:b], None if self.scale is None else self.scale[a:b], self.bias[a:b],
                      None if self.mx is None else self.mx[a:b])

    @staticmethod
    def cat(parts: Sequence["Linear"]) -> "Linear":
        """The parts packed row-wise into one panel (an fp8 matrix through its bytes).  No part scaled: no scale; otherwise
        one scale vector, with ones for the unscaled parts."""
        ws = [p.w for p in parts]
        if parts[0].mx is not None:         # block scales are per row: a plain concatenation of codes and of scales
            return Linear(torch.cat(ws, 0), None, torch.cat([p.bias for p in parts], 0), torch.cat([p.mx for p in parts], 0))
        w = torch.cat([t.view(torch.uint8) for t in ws], 0).view(FP8) if ws[0].dtype == FP8 else torch.cat(ws, 0)
        scale = None
        if any(p.scale is not None for p in parts):
            scale = torch.cat([torch.ones(p.N, dtype=torch.float32, device=p.w.device) if p.scale is None else p.scale
                               for p in parts], 0).contiguous()
        return Linear(w, scale, torch.cat([p.bias for p in parts], 0))


class _Block:
    # Linear: self-attention q|k|v (one (3D,D) panel) and to_out, text attention to_q, k|v (one (2D,D) panel) and to_out,
    # feed-forward in and out; then the q/k-norm weights (wqkn: wqn | wkn for the launch form that normalises both at once)
    __slots__ = ("qkv", "o", "q2", "kv2", "o2", "ff1", "ff2", "wqn", "wkn", "wqkn", "wqn2", "wkn2")


def _vt_buffer(*lead: int, tokens: int, device) -> torch.Tensor:
    """A V^T buffer (*lead, tokens padded to 64): zero-filled where there is padding, which attention reads."""
    padded = (tokens + 63) // 64 * 64
    return (torch.zeros if padded != tokens else torch.empty)((*lead, padded), dtype=BF16, device=device)


class _Fwd:
    """The state of one forward between its stages (``LTXModel._fwd_*``): sizes, the residual stream ``x`` with its row
    statistics, the modulation tables and the buffers the blocks share.  Plain attributes, set once by ``_fwd_prepare``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class ContextKV:
    """Step-invariant text-side tensors of ONE context: the caption projection (ltx.py:77-89) and every
    block's cross-attention K (q/k-normed) and V^T (attention.py:123-131 with context=text).  Built by
    ``LTXModel.prepare_context`` and owned by the caller: ``prepare_context(context, out=kv)`` recomputes
    it IN PLACE for a new prompt, so a captured step graph that reads these buffers stays valid."""

    def __init__(self, shape: Tuple[int, int, int]):
        self.shape = tuple(shape)           # (B,S,caption_channels) it was built for
        self.ctx: Optional[torch.Tensor] = None
        self.kv: List[tuple] = []           # per block: (k, V^T, sumsq)
        self.stacked: Optional[tuple] = None   # the (L, ...) buffers the entries of kv are slices of, when one grouped launch wrote them


class LTXModel:
    """Velocity model.  ``model(video=Modality(...)) -> (velocity (B,N,128), None)``."""

    def __init__(self, config: LTXModelConfig, weights: Dict[str, torch.Tensor], fuse: int = 15, fp8_activations: bool = False):
        if fp8_activations and not any(torch.is_tensor(v) and v.dtype == FP8 for v in weights.values()):
            raise ValueError("fp8_activations needs float8_e4m3fn weights (weights.transformer_weights(fp8=True) / "
                             "quantize_transformer_weights): fp8 activations multiply fp8 weight panels")
        if is_mxfp4_weights(weights):
            if fp8_activations:
                raise ValueError("fp8_activations on an MXFP4 weight dict: its in-block GEMMs run on MXFP4 operands on both sides "
                                 "(ops.gemm_mxfp4); fp8 activations go with float8_e4m3fn weights")
            if config.attention_head_dim != 128:
                raise ValueError(f"MXFP4 weights with attention_head_dim = {config.attention_head_dim}: the MXFP4 DiT is the video "
                                 "transformer (head dim 128); the head-dim-64 audio configuration is not supported")
        self.config = config
        self.inner_dim = config.inner_dim
        self.num_attention_heads = config.num_attention_heads
        self.positional_embedding_theta = config.positional_embedding_theta
        self.positional_embedding_max_pos = list(config.positional_embedding_max_pos)
        self.use_middle_indices_grid = config.use_middle_indices_grid
        self.rope_type = config.rope_type
        self.timestep_scale_multiplier = config.timestep_scale_multiplier
        # A/B switches of the launch structure (scripts/ab_step.py; all three forms give the same roundings):
        #   1: q|k|v and text k|v as ONE GEMM launch with a split output;  2: row sums of squares carried by the GEMM
        #   epilogues into the norm kernels;  4: q_norm + RoPE of q applied inside the attention kernel (needs 2);
        #   8: self-attention q|k and v as TWO launches after all - q|k (N=8192) then fills exactly one round of the
        #   320x256-tile kernel, 152 + 74 us against 239 us for the one q|k|v launch on 160x256 tiles at M=2560
        #   (profiles/r02_gemm_big_tile_ab.log); the text k|v pair stays one launch (it takes the big tile as it is)
        if config.attention_head_dim not in (64, 128):
            raise ValueError(f"attention_head_dim = {config.attention_head_dim}: the attention kernels take 128 (video) or 64 (audio)")
        # head dim 64 (the audio transformer): ltxk_flash_attn_dh64 has no fused query preparation - bit 4 is off there
        self.fuse = int(fuse) & ~4 if config.attention_head_dim == 64 else int(fuse)
        # every token through the token->row map even when all tokens share one timestep row (A/B runs only)
        self.tok2row_always = False
        # True makes a forward's bits independent of the batch it runs in (B=1 per CFG-pair rank == row b of the B=2
        # cfg_batch forward): every ops.gemm single-pass (no split-K scratch on offer - the split-K slice count depends on M, so at
        # M <= ops.SPLITK_MAX_M a row sums its products in another order when the launch holds more rows) and every
        # attention without the tail split.  Costs the split-K weight stream of small-M launches.
        self.batch_invariant = False
        # ops.flash_attn(tail_split=) alone (attention only; batch_invariant turns it off too): False makes attention's bits
        # independent of the batch, at ~5 % of attention time at N=1280 (attention.hip).  The GEMMs of a forward with
        # M <= ops.SPLITK_MAX_M still depend on it.
        self.attn_tail_split = True
        # the text K / V^T of all blocks by one grouped launch per forward (_context_kv_all); False: one launch pair per block
        # (_context_kv - the same bits; kept as the reference of the equality tests and for A/B timing)
        self.grouped_context_kv = True
        self._pack(weights)
        # W8A8 (opt-in, fp8 weights only): the inputs of the in-block Linear GEMMs - nx, att, hff and the text
        # context - are quantised per row to e4m3 (one ops.quant_rows_fp8 launch in front of the GEMM, the context once per
        # forward) and multiplied fp8 x fp8 (ltxk_gemm_w8a8).  A launch the library would run as split-K (small M: a weight
        # stream that gains nothing from fp8 arithmetic) keeps its W8A16 call; with batch_invariant nothing is split, so every
        # in-block launch is W8A8 and, quantisation being per row, a row's bits stay independent of the batch.  The timestep /
        # AdaLN GEMMs, patchify, the caption projection and the output head stay W8A16.
        self.fp8_activations = bool(fp8_activations)
        self._w8a8_plans: Dict[tuple, bool] = {}
        # the split-K scratch of ops.gemm (small-M launches) must exist before anyone captures a forward into a hipGraph: allocated
        # inside a capture it would come from that graph's private pool
        ops._scratch("gemm_splitk", self.tables.device)

    # ------------------------------------------------------------------ weights
    def _pack(self, W: Dict[str, torch.Tensor]) -> None:
        """Builds the packed panels from ``W`` WITHOUT modifying it (a second model - e.g. the LoRA-merged
        stage-2 transformer, generate.py:3229-3237 - can be constructed from the same dict)."""
        cfg = self.config
        missing = [k for k in self.expected_keys(cfg) if k not in W]
        if missing:   # strict load (ltx.py:874-881)
            raise ValueError(f"Missing {len(missing)} parameters in checkpoint, e.g. {missing[:4]}")

        def g(k):
            t = W[k]
            if t.dtype != BF16 or not t.is_cuda:
                raise TypeError(f"weight {k}: expected a bf16 device tensor")
            return t.contiguous()

        # The (out,in) matrices of the Linear layers are all bf16, or all float8_e4m3fn (weights.transformer_weights(fp8=True)):
        # an fp8 matrix may come with a per-output-channel scale under "<key>_scale" and stays fp8 inside the model - every
        # GEMM over it is ltxk_gemm_w8, no bf16 copy of a panel is ever made.
        mats = [k for k in self.expected_keys(cfg) if k.endswith(".weight") and W[k].ndim == 2]
        # Or the in-block matrices are MXFP4 (weights.quantize_transformer_weights_mxfp4): uint8 codes under the key and the e8m0
        # block scales under "<key>_mxscale"; every GEMM over them is ltxk_gemm_mxfp4 on quantised activations and
        # everything else stays bf16.
        mxfp4 = is_mxfp4_weights(W)
        self.weight_dtype = MXFP4 if mxfp4 else (FP8 if any(W[k].dtype == FP8 for k in mats) else BF16)
        fp8 = self.weight_dtype == FP8

        def load(k):
            """The Linear of one checkpoint ``*.weight`` key: the matrix, its optional ``<key>_scale`` (fp8 model), its ``.bias``."""
            bias = g(k[:-len("weight")] + "bias")
            if mxfp4 and k + MXSCALE_SUFFIX in W:
                c, sc = W[k], W[k + MXSCALE_SUFFIX]
                if c.dtype != torch.uint8 or sc.dtype != torch.uint8 or not c.is_cuda or c.ndim != 2 or sc.device != c.device or \
                        tuple(sc.shape) != (c.shape[0], c.shape[1] // 16) or (2 * c.shape[1]) % ops.MXFP4_KSTEP:
                    raise TypeError(f"weight {k}: an MXFP4 matrix is (N, K/2) uint8 codes with (N, K/32) uint8 block scales under "
                                    f"{k + MXSCALE_SUFFIX!r} on the device, K a multiple of {ops.MXFP4_KSTEP}")
                return Linear(c.contiguous(), None, bias, sc.contiguous())
            if not fp8:
                return Linear(g(k), None, bias)
            t, sc = W[k], W.get(k + "_scale")
            if t.dtype != FP8 or not t.is_cuda:
                raise TypeError(f"weight {k}: an fp8 model takes every Linear matrix as a float8_e4m3fn device tensor, got {t.dtype}")
            if sc is not None and (sc.dtype != torch.float32 or sc.shape != (t.shape[0],) or sc.device != t.device):
                raise TypeError(f"weight {k}_scale: expected a ({t.shape[0]},) float32 device tensor")
            return Linear(t.contiguous(), None if sc is None else sc.contiguous(), bias)

        def lin(*keys):
            """``load`` of one key, or of several packed row-wise into one panel; every key goes into the panel table."""
            parts = [load(k) for k in keys]
            panel = parts[0] if len(parts) == 1 else Linear.cat(parts)
            r = 0
            for k, part in zip(keys, parts):
                self._panels[k] = (panel, r, r + part.N)
                r += part.N
            return panel

        # checkpoint key of every Linear matrix -> (the Linear that holds it, its first row, its end row), in load order
        self._panels: Dict[str, Tuple[Linear, int, int]] = {}
        self.patchify = lin("patchify_proj.weight")
        p = "adaln_single.emb.timestep_embedder"
        self.t1, self.t2 = lin(f"{p}.linear1.weight"), lin(f"{p}.linear2.weight")
        self.ada = lin("adaln_single.linear.weight")
        self.c1, self.c2 = lin("caption_projection.linear1.weight"), lin("caption_projection.linear2.weight")
        self.head_table = g("scale_shift_table").reshape(1, 2, -1)
        self.out = lin("proj_out.weight")
        self.blocks: List[_Block] = []
        tables = []
        for i in range(cfg.num_layers):
            pre = f"transformer_blocks.{i}"
            b = _Block()
            # one (3D,D) panel for to_q|to_k|to_v: a single GEMM launch writes q|k row-major and V^T (split output)
            b.qkv = lin(*(f"{pre}.attn1.to_{n}.weight" for n in "qkv"))
            b.wqn, b.wkn = g(f"{pre}.attn1.q_norm.weight"), g(f"{pre}.attn1.k_norm.weight")
            b.wqkn = torch.cat([b.wqn, b.wkn], 0)
            b.o, b.q2 = lin(f"{pre}.attn1.to_out.weight"), lin(f"{pre}.attn2.to_q.weight")
            b.kv2 = lin(f"{pre}.attn2.to_k.weight", f"{pre}.attn2.to_v.weight")     # text k | V^T, one launch
            b.wqn2, b.wkn2 = g(f"{pre}.attn2.q_norm.weight"), g(f"{pre}.attn2.k_norm.weight")
            b.o2 = lin(f"{pre}.attn2.to_out.weight")
            b.ff1, b.ff2 = lin(f"{pre}.ff.proj_in.weight"), lin(f"{pre}.ff.proj_out.weight")
            tables.append(g(f"{pre}.scale_shift_table"))
            self.blocks.append(b)
        self.tables = torch.stack(tables, 0).contiguous()      # (L,6,D)
        # the text k | V^T projections of all blocks as one grouped launch (_context_kv_all): the k-norm weights stacked into one
        # (L,D) table - the blocks keep rows of it - and device tables of the panels' addresses; the panels stay where they are
        self.wkn2_all = torch.stack([b.wkn2 for b in self.blocks], 0).contiguous()
        for i, b in enumerate(self.blocks):
            b.wkn2 = self.wkn2_all[i]
        self.wkv2_table = ops.pointer_table([b.kv2.w for b in self.blocks])
        self.bkv2_table = ops.pointer_table([b.kv2.bias for b in self.blocks])

    def weight_views(self) -> Dict[str, torch.Tensor]:
        """Checkpoint key -> the (out,in) matrix as it lives inside THIS model: the packed q|k|v and text k|v panels are
        returned as their row ranges.  Writing through these views changes the model (lora.apply_lora_to_weights(...,
        in_place=True): the stage-2 transformer of the distilled pipeline without a second 21-GB replica, generate.py:3229-3283)."""
        if self.weight_dtype != BF16:
            fmt, fn = ("MXFP4", "quantize_transformer_weights_mxfp4") if self.weight_dtype == MXFP4 else ("float8_e4m3fn", "quantize_transformer_weights")
            raise TypeError(f"weight_views: this model keeps its matrices in {fmt}, which cannot take an in-place LoRA merge; "
                            "merge into the bf16 weight dict (lora.apply_lora_to_weights(weights, specs), the fresh-copy path), "
                            f"quantise the result (weights.{fn}) and build a model from it")
        return {k: panel.w[a:b] for k, (panel, a, b) in self._panels.items()}

    def weight_bytes(self) -> int:
        """Device bytes of everything this model holds of its checkpoint: the matrices (bf16, or e4m3 panels plus their scale
        vectors), biases, norm weights and scale-shift tables."""
        held = [t for panel, _, _ in self._panels.values() for t in (panel.w, panel.scale, panel.bias, panel.mx) if t is not None]
        held += [self.head_table, self.tables, self.wkn2_all]
        held += [t for b in self.blocks for t in (b.wqn, b.wkn, b.wqn2)]     # (wkn2: a row of wkn2_all; wqkn: a copy of wqn | wkn)
        once = {}                           # a packed panel is in the table once per key: each tensor counts once, as first seen
        for t in held:
            once.setdefault(t.data_ptr(), t)
        return sum(t.numel() * t.element_size() for t in once.values())

    @staticmethod
    def expected_keys(cfg: LTXModelConfig) -> List[str]:
        keys = []
        for n in ("patchify_proj", "adaln_single.emb.timestep_embedder.linear1",
                  "adaln_single.emb.timestep_embedder.linear2", "adaln_single.linear",
                  "caption_projection.linear1", "caption_projection.linear2", "proj_out"):
            keys += [f"{n}.weight", f"{n}.bias"]
        keys.append("scale_shift_table")
        for i in range(cfg.num_layers):
            pre = f"transformer_blocks.{i}"
            for a in ("attn1", "attn2"):
                for nm in ("to_q", "to_k", "to_v", "to_out"):
                    keys += [f"{pre}.{a}.{nm}.weight", f"{pre}.{a}.{nm}.bias"]
                keys += [f"{pre}.{a}.q_norm.weight", f"{pre}.{a}.k_norm.weight"]
            keys += [f"{pre}.ff.proj_in.weight", f"{pre}.ff.proj_in.bias",
                     f"{pre}.ff.proj_out.weight", f"{pre}.ff.proj_out.bias", f"{pre}.scale_shift_table"]
        return keys

    @staticmethod
    def sanitize(weights: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Checkpoint key map of ltx.py:508-533 (PyTorch LTX-2 names -> module names)."""
        out = {}
        for key, value in weights.items():
            if (not key.startswith("model.diffusion_model.") or "audio_embeddings_connector" in key
                    or "video_embeddings_connector" in key):
                continue
            k = key.replace("model.diffusion_model.", "")
            k = k.replace(".to_out.0.", ".to_out.")
            k = k.replace(".ff.net.0.proj.", ".ff.proj_in.").replace(".ff.net.2.", ".ff.proj_out.")
            k = k.replace(".audio_ff.net.0.proj.", ".audio_ff.proj_in.").replace(".audio_ff.net.2.", ".audio_ff.proj_out.")
            k = k.replace(".linear_1.", ".linear1.").replace(".linear_2.", ".linear2.")
            out[k] = value
        return out

    @staticmethod
    def random_weights(config: LTXModelConfig, device, seed: int = 1234) -> Dict[str, torch.Tensor]:
        """Random weights of the exact architecture, generated on the device (synthetic bench;
        SURVEY.md §8d): Linear N(0,0.02^2), biases 0.01*N(0,1), tables N(0,0.02^2),
        q/k-norm weights 1+0.1*N(0,1).  Module-name keys (what ``sanitize`` produces)."""
        g = torch.Generator(device=device).manual_seed(seed)
        D, FF = config.inner_dim, config.inner_dim * 4
        W: Dict[str, torch.Tensor] = {}

        def rn(*shape, std=1.0, mean=0.0):
            return (torch.randn(*shape, generator=g, device=device, dtype=torch.float32) * std + mean).to(BF16)

        def lin(name, o, i):
            W[f"{name}.weight"] = rn(o, i, std=0.02)
            W[f"{name}.bias"] = rn(o, std=0.01)

        lin("patchify_proj", D, config.in_channels)
        lin("adaln_single.emb.timestep_embedder.linear1", D, 256)
        lin("adaln_single.emb.timestep_embedder.linear2", D, D)
        lin("adaln_single.linear", 6 * D, D)
        lin("caption_projection.linear1", D, config.caption_channels)
        lin("caption_projection.linear2", D, D)
        W["scale_shift_table"] = rn(2, D, std=0.02)
        lin("proj_out", config.out_channels, D)
        for i in range(config.num_layers):
            pre = f"transformer_blocks.{i}"
            for a in ("attn1", "attn2"):
                for nm in ("to_q", "to_k", "to_v", "to_out"):
                    lin(f"{pre}.{a}.{nm}", D, D)
                W[f"{pre}.{a}.q_norm.weight"] = rn(D, std=0.1, mean=1.0)
                W[f"{pre}.{a}.k_norm.weight"] = rn(D, std=0.1, mean=1.0)
            lin(f"{pre}.ff.proj_in", FF, D)
            lin(f"{pre}.ff.proj_out", D, FF)
            W[f"{pre}.scale_shift_table"] = rn(6, D, std=0.02)
        return W

    @classmethod
    def random_init(cls, config: LTXModelConfig, device, seed: int = 1234, fuse: int = 15) -> "LTXModel":
        return cls(config, cls.random_weights(config, device, seed), fuse=fuse)

    # ------------------------------------------------------------------ forward
    @property
    def _split_k(self) -> bool:
        """Whether a GEMM may split K: not in batch_invariant mode.  ``_gemm``, ``_plan`` and the W8A8 memo read it, nothing else."""
        return not self.batch_invariant

    def _w8a8_launch(self, M: int, lin: Linear, epilogue: int = ops.EPI_BIAS, n_split: int = 0, out_tokens_per_batch: int = 0,
                     sumsq: Optional[torch.Tensor] = None, **_) -> bool:
        """Whether the GEMM of ``lin`` over M rows with these keyword arguments runs W8A8: the feature is on and the library would
        run the W8A16 call single-pass (ops.gemm_plan(w8=True)).  The named keywords are those of ops.gemm that decide the launch
        form, with ops.gemm's defaults (keep them in step); the call's others (out, resid, gate ...) pass by, ops.gemm checks them."""
        if not self.fp8_activations or lin.K % 128 != 0:
            return False
        key = (M, lin.N, lin.K, epilogue, n_split, out_tokens_per_batch, sumsq is not None, self._split_k)
        if key not in self._w8a8_plans:
            self._w8a8_plans[key] = not self._plan(M, lin.N, lin.K, epilogue=epilogue, n_split=n_split, sumsq=key[6],
                                                   out_tokens_per_batch=out_tokens_per_batch, w8=True).split_k
        return self._w8a8_plans[key]

    def _gemm(self, a: torch.Tensor, lin: Linear, a_q: Optional[tuple] = None, **kw) -> torch.Tensor:
        """THE ops.gemm call of the model: ``lin`` over ``a``, or over its quantised twin ``a_q`` = (a8, a_scale) (W8A8).
        Split-K as batch_invariant allows and the panel's own scale, for every launch."""
        if lin.mx is not None:
            if a_q is None:
                raise ValueError("an MXFP4 panel multiplies quantised activations only (ops.gemm_mxfp4): no buffers were given")
            return ops.gemm_mxfp4(a_q[0], a_q[1], lin.w, lin.mx, lin.bias, **kw)
        if a_q is not None:
            a, kw["a_scale"] = a_q
        return ops.gemm(a, lin.w, lin.bias, split_k=self._split_k, w_scale=lin.scale, **kw)

    def _plan(self, M: int, N: int, K: int, **kw) -> "ops.GemmPlan":
        """ops.gemm_plan of a launch as ``_gemm`` issues it."""
        return ops.gemm_plan(M, N, K, split_k=self._split_k, **kw)

    def _lin(self, a: torch.Tensor, q: Optional[tuple], launches, fresh: bool = True) -> List[torch.Tensor]:
        """The GEMM launches [(Linear, kwargs)] over one input ``a``.  ``q`` = (a8, a_scale) buffers (None: fp8 activations
        off - exactly the ops.gemm calls): ``a`` is quantised into them by ONE launch if any of the launches runs W8A8
        (``fresh=False``: they already hold ``a`` quantised), and those launches read the quantised copy."""
        if any(lin.mx is not None for lin, _ in launches):
            # MXFP4 panels: every launch is ltxk_gemm_mxfp4 over the one quantised copy, whatever M is (no other GEMM to fall back to)
            if fresh:
                ops.quant_rows_mxfp4(a, out=q)
            return [self._gemm(a, lin, q, **kw) for lin, kw in launches]
        use = [q is not None and self._w8a8_launch(a.shape[0], lin, **kw) for lin, kw in launches]
        if fresh and any(use):
            ops.quant_rows_fp8(a, out=q)
        return [self._gemm(a, lin, q if u else None, **kw) for (lin, kw), u in zip(launches, use)]

    def _linear(self, a: torch.Tensor, lin: Linear, q: Optional[tuple] = None, **kw) -> torch.Tensor:
        """One Linear over ``a``: ``_lin`` with a single launch (without ``q`` it stays W8A16 / bf16)."""
        return self._lin(a, q, [(lin, kw)])[0]

    def _prepare_context(self, context: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ltx.py:77-89: caption_projection, (B,S,3840) -> (B*S,D)."""
        b, s, c = context.shape
        return self._linear(self._linear(context.reshape(b * s, c), self.c1, epilogue=ops.EPI_BIAS_GELU), self.c2, out=out)

    def _context_kv_launches(self, blk: _Block, k2, vt2, st, s: int):
        """The text k | V^T GEMM launches of one block as [(Linear, kwargs)] (one launch with a split output, or two)."""
        D = self.inner_dim
        if self.fuse & 1:
            return [(blk.kv2, dict(out=k2, out2=vt2, n_split=D, out_tokens_per_batch=s, sumsq=st))]
        return [(blk.kv2.rows(None, D), dict(out=k2, sumsq=st)), (blk.kv2.rows(D, None), dict(out=vt2, out_tokens_per_batch=s))]

    def _context_kv_buffers(self, ctx: torch.Tensor, b: int, s: int, *lead: int) -> tuple:
        """(k, V^T, sumsq) buffers of the text side of one block, or with ``lead`` = (L,) of all blocks."""
        D = self.inner_dim
        return (torch.empty((*lead, b * s, D), dtype=BF16, device=ctx.device), _vt_buffer(*lead, b, D, tokens=s, device=ctx.device),
                torch.empty((*lead, b * s, D // 64), dtype=torch.float32, device=ctx.device))

    def _context_kv(self, blk: _Block, ctx: torch.Tensor, b: int, s: int, out: Optional[tuple] = None, ctx_q: Optional[tuple] = None):
        """``ctx_q``: (ctx8, scale) - the context already quantised for the W8A8 launches (once per forward, not per block)."""
        D, H, eps = self.inner_dim, self.num_attention_heads, self.config.norm_eps
        k2, vt2, ss = out if out is not None else self._context_kv_buffers(ctx, b, s)
        # k (row-major, with its per-row sums of squares) and V^T from one launch over the packed k|v panel
        st = ss if self.fuse & 2 else None
        self._lin(ctx, ctx_q, self._context_kv_launches(blk, k2, vt2, st, s), fresh=False)
        ops.qknorm_rope(k2, 1, D, blk.wkn2, None, None, s, H, eps, sumsq=st, head_dim=self.config.attention_head_dim)
        return k2, vt2, ss

    def _quant_context(self, ctx: torch.Tensor, s: int) -> Optional[tuple]:
        """The projected context quantised for the text k | V^T launches of ALL blocks (they share shapes, so one decision and
        one quantiser launch per forward), or None where those launches stay W8A16."""
        if self.weight_dtype == MXFP4:
            return ops.quant_rows_mxfp4(ctx)
        launches = self._context_kv_launches(self.blocks[0], None, None, True if self.fuse & 2 else None, s)
        return ops.quant_rows_fp8(ctx) if any(self._w8a8_launch(ctx.shape[0], lin, **kw) for lin, kw in launches) else None

    def _grouped_context_ok(self, b: int, s: int) -> bool:
        """Whether the grouped launch gives the bits of the per-block ``_context_kv`` calls: it is single-pass, as they are unless
        the library would split K at this row count (small M with the split-K scratch on offer)."""
        D = self.inner_dim
        # (the grouped launch has no weight-fp8 form: an fp8 model goes per block - the same bits; its k-norm launch,
        # ltxk_qknorm_grouped_ss, is head dim 128 only: a head-dim-64 model goes per block too)
        if self.config.attention_head_dim != 128:
            return False
        if not self.grouped_context_kv or (self.fuse & 3) != 3 or D % 256 != 0 or self.weight_dtype != BF16:
            return False
        return not self._plan(b * s, 2 * D, D, n_split=D, out_tokens_per_batch=s, sumsq=True).split_k

    def _context_kv_all(self, ctx: torch.Tensor, b: int, s: int, out: Optional[tuple] = None):
        """``_context_kv`` of every block at once: one grouped GEMM launch over the L packed k|v panels into (L, ...) buffers and
        one k-norm launch over them.  Returns (k (L,b*s,D), V^T (L,b,D,s padded to 64), sumsq (L,b*s,D/64)); block li reads index li."""
        D, H, eps = self.inner_dim, self.num_attention_heads, self.config.norm_eps
        k2, vt2, ss = out if out is not None else self._context_kv_buffers(ctx, b, s, len(self.blocks))
        ops.gemm_grouped(ctx, self.wkv2_table, self.bkv2_table, 2 * D, out=k2, out2=vt2, n_split=D, out_tokens_per_batch=s, sumsq=ss)
        ops.qknorm_grouped(k2, self.wkn2_all, H, eps, ss)
        return k2, vt2, ss

    def prepare_context(self, context: torch.Tensor, out: Optional[ContextKV] = None) -> ContextKV:
        """Everything of the forward that depends on the text context only (3.37 TFLOP at S=1024, SURVEY.md
        §8d).  The reference recomputes it in every forward; a denoise loop may hoist it (an algorithmic
        change, always reported separately).  ``out``: refresh an existing object in place."""
        context = context.to(BF16).contiguous()
        b, s, _ = context.shape
        kv = out if out is not None else ContextKV(context.shape)
        if kv.shape != tuple(context.shape):
            raise ValueError(f"ContextKV was built for context {kv.shape}, got {tuple(context.shape)}")
        kv.ctx = self._prepare_context(context, kv.ctx)
        if self._grouped_context_ok(b, s):
            kv.stacked = k2, vt2, ss = self._context_kv_all(kv.ctx, b, s, kv.stacked)
            kv.kv = [(k2[i], vt2[i], ss[i]) for i in range(len(self.blocks))]
            return kv
        ctx_q = self._quant_context(kv.ctx, s)
        kv.kv = [self._context_kv(blk, kv.ctx, b, s, kv.kv[i] if kv.kv else None, ctx_q) for i, blk in enumerate(self.blocks)]
        kv.stacked = None
        return kv

    def forward_tokens(self, latent: torch.Tensor, plan: TimestepPlan, context: torch.Tensor,
                       pe: Tuple[torch.Tensor, torch.Tensor], ctx_kv: Optional[ContextKV] = None,
                       hidden: Optional[List[torch.Tensor]] = None,
                       perturbations: Optional[BatchedPerturbationConfig] = None) -> torch.Tensor:
        """latent (B,N,128) bf16; context (B,S,3840) bf16; pe = (cos,sin) each (1|B,H,N,head_dim/2) fp32
        (one table shared by every batch row, as in cfg_batch where it is a broadcast,
        generate.py:1196-1202).  ``ctx_kv``: a ContextKV of THIS context (prepare_context); without it the
        caption projection and the text K/V are recomputed here, as the reference does every forward.
        ``hidden``: a list that receives a copy of the residual stream (B,N,D) after every block (the reference's
        debug taps, transformer.py; used by the per-layer parity tests).
        ``perturbations``: one PerturbationConfig per batch row (guidance.py); in a row perturbed with SKIP_VIDEO_SELF_ATTN at
        a block, that block's self-attention returns its value projection v instead of softmax(q k^T) v (then to_out, gate and
        residual as usual) - STG, DESIGN.md "Spatio-temporal guidance".  None: no row is perturbed.
        The forward is four stages over one ``_Fwd`` state - prepare; per block the self- and text attention, then the
        feed-forward; the head - so that the AudioVideo model (av_model.py) can run two of these forwards block by block with
        the cross-modal attentions in between."""
        st = self._fwd_prepare(latent, plan, context, pe, ctx_kv, perturbations)
        for li in range(len(self.blocks)):
            self._fwd_attn(st, li)
            self._fwd_ff(st, li)
            if hidden is not None:
                hidden.append(st.x.reshape(st.B, st.N, self.inner_dim).clone())
        return self._fwd_head(st)

    def _fwd_prepare(self, latent: torch.Tensor, plan: TimestepPlan, context: torch.Tensor, pe: Tuple[torch.Tensor, torch.Tensor],
                     ctx_kv: Optional[ContextKV], perturbations: Optional[BatchedPerturbationConfig]) -> "_Fwd":
        """Everything of ``forward_tokens`` in front of block 0: the residual stream, the modulation tables, the context and
        the buffers the blocks share."""
        cfg = self.config
        D, H, eps = self.inner_dim, self.num_attention_heads, cfg.norm_eps
        B, N, C = latent.shape
        M = B * N
        S = context.shape[1]
        dev = latent.device
        cos, sin = pe
        if cos.dim() == 4:
            cos, sin = cos[0], sin[0]
        cos, sin = cos.contiguous(), sin.contiguous()
        U = plan.values.numel()
        # one timestep row for every token (an unconditioned CFG pair): no per-token row gather - the kernels then skip a
        # dependent load in front of every modulation / gate read
        tok2row = plan.tok2row if (U > 1 or self.tok2row_always) else None
        dh = cfg.attention_head_dim
        scale = 1.0 / math.sqrt(dh)

        # --- prepare (ltx.py:129-158) ---
        # Row statistics travel with the residual stream: every GEMM that writes x also emits the per-row sums of
        # squares of what it stored (64-column partials), so the rms_norm that follows does not re-reduce the row.
        P = D // 64
        xss = torch.empty((M, P), dtype=torch.float32, device=dev)
        x = self._linear(latent.reshape(M, C), self.patchify, sumsq=xss)
        tproj = ops.timestep_embed(plan.values, 256, float(cfg.timestep_scale_multiplier))
        h = self._linear(tproj, self.t1, epilogue=ops.EPI_BIAS_SILU)
        emb = self._linear(h, self.t2)                     # embedded_timestep (U,D)
        ada = self._linear(ops.silu(emb), self.ada)        # (U,6D)
        # (L,U,6,D): shift, 1+scale, gate, shift, 1+scale, gate - the (1 + scale) factor is the same for every token of a row
        # (without the carried row statistics the self-reducing norm kernel takes the raw scale and adds 1 itself)
        mods = ops.ada_combine(self.tables, ada, cfg.num_layers, U, 6, D, one_plus_mask=0b010010 if self.fuse & 2 else 0)
        head = ops.ada_combine(self.head_table, emb.repeat(1, 2), 1, U, 2, D)[0]   # (U,2,D): shift, scale

        if ctx_kv is not None:
            if ctx_kv.shape != tuple(context.shape):
                raise ValueError(f"ctx_kv was built for context {ctx_kv.shape}, got {tuple(context.shape)}")
            ctx = ctx_kv.ctx
        else:
            ctx = self._prepare_context(context)

        vt = _vt_buffer(B, D, tokens=N, device=dev)
        qk = torch.empty((M, 2 * D), dtype=BF16, device=dev)
        qkss = torch.empty((M, 2 * P), dtype=torch.float32, device=dev)
        nx = torch.empty((M, D), dtype=BF16, device=dev)
        att = torch.empty((M, D), dtype=BF16, device=dev)
        q2 = torch.empty((M, D), dtype=BF16, device=dev)
        q2ss = torch.empty((M, P), dtype=torch.float32, device=dev)
        hff = torch.empty((M, 4 * D), dtype=BF16, device=dev)
        nx_q = att_q = hff_q = ctx_q = None
        if self.fp8_activations:           # the quantised twins of the GEMM inputs: e4m3 rows + one fp32 scale per row
            def qbuf(cols):
                return (torch.empty((M, cols), dtype=FP8, device=dev), torch.empty((M,), dtype=torch.float32, device=dev))
            nx_q, att_q, hff_q = qbuf(D), qbuf(D), qbuf(4 * D)
        if self.weight_dtype == MXFP4:     # the quantised twins for ltxk_gemm_mxfp4: code bytes + e8m0 block scales per row
            def qbuf4(cols):
                return (torch.empty((M, cols // 2), dtype=torch.uint8, device=dev), torch.empty((M, cols // 32), dtype=torch.uint8, device=dev))
            nx_q, att_q, hff_q = qbuf4(D), qbuf4(D), qbuf4(4 * D)
        ms = 6 * D
        kv_buf = kv_all = None
        if ctx_kv is None:
            # Text K / V^T are recomputed every forward, as the reference does.  They depend on ctx and the block's weights only,
            # so all L of them are computed HERE, before block 0, by one grouped persistent GEMM launch and one k-norm launch
            # into (L, ...) buffers (0.8 GB each for k and V^T at B=2, S=1024, L=48; allocated per forward like every other
            # activation): over 48 launches' worth of tiles the 320-row tile fills its rounds, which one M=2048 launch cannot,
            # and the launch ramp is paid once.  Same work on the main stream, same bits.
            # Rejected before, and still: block li+1's text K / V^T on a side stream beside block li measured 1.7 % SLOWER eagerly
            # and unchanged in a captured graph - the main kernels leave no CU idle long enough for a 156-KiB-LDS GEMM
            # workgroup (profiles/r02_launch_structure_ab.log); k's q_norm on a side stream beside the V^T GEMM: 1.269 against
            # 1.264 ms per block - forked graph branches cost more than they overlap; one GRID for two independent GEMMs (q|k
            # on 320x256 tiles with v's 160x256 tiles back-filling behind them; text k|v with q2): 1269.6 us per block either way.
            if self._grouped_context_ok(B, S):
                kv_all = self._context_kv_all(ctx, B, S)
            else:
                # per block (the library would split K here, or the fused forms are off): the context is quantised once per
                # forward - every block's text k | V^T launch reads it - and the blocks share one buffer set
                ctx_q = self._quant_context(ctx, S)
                kv_buf = self._context_kv_buffers(ctx, B, S)

        skip_rows = [[] for _ in self.blocks]          # per block: the batch rows whose self-attention is skipped (STG)
        if perturbations is not None:
            if len(perturbations.perturbations) != B:
                raise ValueError(f"perturbations has {len(perturbations.perturbations)} rows, the batch {B}")
            skip_rows = [perturbations.rows(PerturbationType.SKIP_VIDEO_SELF_ATTN, li) for li in range(len(self.blocks))]

        fq, fs, fp = self.fuse & 1, self.fuse & 2, (self.fuse & 6) == 6
        ts_ = self.attn_tail_split and not self.batch_invariant
        s_x, s_qk, s_q2 = (xss, qkss, q2ss) if fs else (None, None, None)
        return _Fwd(B=B, N=N, M=M, S=S, U=U, P=P, x=x, xss=xss, tproj=tproj, mods=mods, head=head, tok2row=tok2row, cos=cos, sin=sin,
                    ctx=ctx, ctx_kv=ctx_kv, kv_all=kv_all, kv_buf=kv_buf, ctx_q=ctx_q, vt=vt, qk=qk, qkss=qkss, nx=nx, att=att, q2=q2,
                    q2ss=q2ss, hff=hff, nx_q=nx_q, att_q=att_q, hff_q=hff_q, skip_rows=skip_rows, ts_=ts_, s_x=s_x, s_qk=s_qk,
                    s_q2=s_q2)

    def _fwd_attn(self, st: "_Fwd", li: int) -> None:
        """Block ``li``'s self-attention and text attention (transformer.py:247-261), onto st.x."""
        cfg, blk = self.config, self.blocks[li]
        D, H, eps, dh = self.inner_dim, self.num_attention_heads, cfg.norm_eps, cfg.attention_head_dim
        B, N, M, S, P, ms, scale = st.B, st.N, st.M, st.S, st.P, 6 * self.inner_dim, 1.0 / math.sqrt(cfg.attention_head_dim)
        x, nx, qk, vt, att, q2, qkss, q2ss = st.x, st.nx, st.qk, st.vt, st.att, st.q2, st.qkss, st.q2ss
        nx_q, att_q, tok2row, cos, sin, ts_ = st.nx_q, st.att_q, st.tok2row, st.cos, st.sin, st.ts_
        s_x, s_qk, s_q2 = st.s_x, st.s_qk, st.s_q2
        fq, fs, fp = self.fuse & 1, self.fuse & 2, (self.fuse & 6) == 6
        mod = st.mods[li]                                        # (U,6,D): shift, 1+scale, gate x2
        # self-attention (transformer.py:248-254).  q|k|v from one launch: q,k row-major with their row statistics,
        # V^T transposed.  k is normalised + rotated in place; q stays RAW in HBM - the attention kernel normalises
        # and rotates its Q fragments in registers (attention.py:129-136).
        ops.rmsnorm_modulate(x, eps, mod[:, 1], mod[:, 0], ms, tok2row, out=nx, sumsq=s_x, scale_is_one_plus=bool(fs))
        # (fuse bit 8: q|k on the 320x256 tile with v as its own launch - a gain only where M is a whole number of 320-row
        # tiles (M=1280: 35.4 against 35.6 ms per forward, M=2560: 60.3 against 61.0); every other row count is 1-4 % faster
        # with q|k|v as ONE launch (M=1296: 39.4 against 41.2 ms, 3328: 87.6 / 89.2, 5184: 141.5 / 143.8, 6656: 161.5 / 164.7;
        # scripts/exp_qkv_one_launch.py), and at small M every launch is a weight stream with ~5 us of fixed cost)
        if fq and (not (self.fuse & 8) or M <= ops.SPLITK_MAX_M or M % 320 != 0):
            self._linear(nx, blk.qkv, nx_q, out=qk, out2=vt, n_split=2 * D, out_tokens_per_batch=N, sumsq=s_qk)
        else:
            self._lin(nx, nx_q, [(blk.qkv.rows(None, 2 * D), dict(out=qk, sumsq=s_qk)),
                                 (blk.qkv.rows(2 * D, None), dict(out=vt, out_tokens_per_batch=N))])
        skip = st.skip_rows[li]
        # the q side of the two attentions: raw q with its row statistics, normalised (and rotated) inside the kernel - or
        # q normalised by a launch of its own in front
        if fp:
            ops.qknorm_rope(qk[:, D:], 1, D, blk.wkn, cos, sin, N, H, eps, sumsq=qkss[:, P:], head_dim=dh)
            fused1, fused2 = dict(q_norm_weight=blk.wqn, cos=cos, sin=sin, eps=eps), dict(q_sumsq=q2ss, q_norm_weight=blk.wqn2, eps=eps)
        else:
            ops.qknorm_rope(qk, 2, D, blk.wqkn, cos, sin, N, H, eps, sumsq=s_qk, head_dim=dh)
            fused1 = fused2 = {}
        # attention over each maximal run of rows that keep it (all B rows in one launch when nothing is skipped)
        for r0, r1 in _runs(B, skip):
            t0, t1 = r0 * N, r1 * N
            ops.flash_attn(qk[t0:t1, :D], qk[t0:t1, D:], vt[r0:r1], att[t0:t1], r1 - r0, H, N, N, scale,
                           q_sumsq=qkss[t0:t1] if fp else None, tail_split=ts_, head_dim=dh, **fused1)
        if skip:          # STG: the skipped rows' attention output is their value projection, v = (V^T)^T
            ops.attn_value_passthrough(vt, att, B, N, sum(1 << r for r in skip))
        self._linear(att, blk.o, att_q, epilogue=ops.EPI_BIAS_GATE_RES, out=x, resid=x,
                     gate=mod[:, 2], gate_row=tok2row, gate_stride=ms, sumsq=s_x)
        # text cross-attention (transformer.py:257-261)
        ops.rmsnorm_modulate(x, eps, out=nx, sumsq=s_x)
        self._linear(nx, blk.q2, nx_q, out=q2, sumsq=s_q2)
        if st.ctx_kv is not None:
            kv = st.ctx_kv.kv[li]
        elif st.kv_all is not None:
            kv = (st.kv_all[0][li], st.kv_all[1][li], st.kv_all[2][li])
        else:
            kv = self._context_kv(blk, st.ctx, B, S, st.kv_buf, st.ctx_q)
        if not fp:
            ops.qknorm_rope(q2, 1, D, blk.wqn2, None, None, N, H, eps, sumsq=s_q2, head_dim=dh)
        ops.flash_attn(q2, kv[0], kv[1], att, B, H, N, S, scale, tail_split=ts_, head_dim=dh, **fused2)
        self._linear(att, blk.o2, att_q, epilogue=ops.EPI_BIAS_RES, out=x, resid=x, sumsq=s_x)

    def _fwd_ff(self, st: "_Fwd", li: int) -> None:
        """Block ``li``'s feed-forward (transformer.py:343-347), onto st.x."""
        blk, mod, eps, ms, fs = self.blocks[li], st.mods[li], self.config.norm_eps, 6 * self.inner_dim, self.fuse & 2
        x, nx, hff, nx_q, hff_q, tok2row, s_x = st.x, st.nx, st.hff, st.nx_q, st.hff_q, st.tok2row, st.s_x
        ops.rmsnorm_modulate(x, eps, mod[:, 4], mod[:, 3], ms, tok2row, out=nx, sumsq=s_x, scale_is_one_plus=bool(fs))
        self._linear(nx, blk.ff1, nx_q, epilogue=ops.EPI_BIAS_GELU, out=hff)
        self._linear(hff, blk.ff2, hff_q, epilogue=ops.EPI_BIAS_GATE_RES, out=x, resid=x,
                     gate=mod[:, 5], gate_row=tok2row, gate_stride=ms, sumsq=s_x)

    def _fwd_head(self, st: "_Fwd") -> torch.Tensor:
        """The output head (ltx.py:432-457): velocity (B,N,out_channels)."""
        ops.layernorm_modulate(st.x, self.config.norm_eps, st.head[:, 1], st.head[:, 0], 2 * self.inner_dim, st.tok2row, out=st.nx)
        v = self._linear(st.nx, self.out)
        return v.reshape(st.B, st.N, self.config.out_channels)

    # --- step cache (denoise.StepCache): the forward cut in front of and behind its blocks ---
    def step_cache_input(self, st: "_Fwd", rows: int, out: torch.Tensor) -> torch.Tensor:
        """Block 0's modulated self-attention input of the first ``rows`` token rows of a prepared forward, into ``out``
        (rows, D): the launch at the top of ``_fwd_attn(st, 0)`` over those rows, in a buffer of its own - a row's bits do not
        depend on the rows beside it, so they are the bits block 0 will compute.  Leaves ``st`` untouched."""
        mod, fs = st.mods[0], self.fuse & 2
        ops.rmsnorm_modulate(st.x[:rows], self.config.norm_eps, mod[:, 1], mod[:, 0], 6 * self.inner_dim,
                             None if st.tok2row is None else st.tok2row[:rows], out=out,
                             sumsq=None if st.s_x is None else st.s_x[:rows], scale_is_one_plus=bool(fs))
        return out

    def forward_cached(self, st: "_Fwd", resid: torch.Tensor, compute: bool) -> torch.Tensor:
        """The rest of a prepared forward under a step cache.  ``compute``: ``resid`` (M, D) takes a copy of the residual stream
        in front of block 0, the blocks run as in ``forward_tokens``, and resid <- rbf(x_out - x_in).  Otherwise the blocks
        are skipped: x <- rbf(x + resid) with the residual of the last computed step.  Then the head, which reduces its rows
        itself (the carried row statistics of ``st`` are not read behind the last block)."""
        if compute:
            resid.copy_(st.x)
            for li in range(len(self.blocks)):
                self._fwd_attn(st, li)
                self._fwd_ff(st, li)
            ops.residual_store(st.x, resid)
        else:
            ops.residual_apply(st.x, resid)
        return self._fwd_head(st)

    def __call__(self, video: Optional[Modality] = None, audio: Optional[Modality] = None,
                 perturbations: Optional[BatchedPerturbationConfig] = None):
        if audio is not None:
            raise ValueError("Audio is not enabled for this model (joint denoising: av_model.LTXAVModel)")      # ltx.py:468-469
        if video is None:
            return None, None
        lat = video.latent
        if lat.dim() != 3 or lat.shape[-1] != self.config.in_channels:
            raise ValueError(f"latent must be (B,N,{self.config.in_channels}), got {tuple(lat.shape)}")
        if video.context_mask is not None:
            raise ValueError("context_mask is not supported on this path (the reference passes None, generate.py:800)")
        pe = video.positional_embeddings
        if pe is None:
            pe = precompute_freqs_cis(video.positions, self.inner_dim, self.positional_embedding_theta,
                                      self.positional_embedding_max_pos, self.num_attention_heads)
        plan = TimestepPlan.from_timesteps(video.timesteps.to(BF16))
        v = self.forward_tokens(lat.to(BF16).contiguous(), plan, video.context.to(BF16).contiguous(), pe,
                                perturbations=perturbations)
        return v, None


def _runs(B: int, skip: Sequence[int]) -> List[Tuple[int, int]]:
    """Maximal [r0, r1) runs of the rows in range(B) that are not in ``skip``."""
    runs, r0 = [], None
    for r in range(B):
        if r in skip:
            if r0 is not None:
                runs.append((r0, r))
            r0 = None
        elif r0 is None:
            r0 = r
    if r0 is not None:
        runs.append((r0, B))
    return runs


class X0Model:
    """ltx.py:888-906: velocity -> denoised wrapper, x0 = latent - timesteps*velocity with the per-token
    timesteps as sigma (utils.py:404-440, fp32 then cast).  Only used by the reference's legacy
    ltx_pipelines/utils helpers; implemented with the step kernel per distinct sigma."""

    def __init__(self, velocity_model: LTXModel):
        self.velocity_model = velocity_model

    def __call__(self, video: Optional[Modality] = None, audio: Optional[Modality] = None,
                 perturbations: Optional[BatchedPerturbationConfig] = None):
        v, _ = self.velocity_model(video, audio, perturbations=perturbations)
        if v is None:
            return None, None
        lat = video.latent.to(BF16)
        B, N, C = lat.shape
        out = torch.empty_like(lat)
        ts = video.timesteps.to(BF16)
        for val in torch.unique(ts).tolist():
            # ltxk_cfg_euler_step with sigma_next = 0 returns x0 = bf16(x - sigma*v); it works on channels-first
            # latents, so view the (B,N,C) tokens as a (B*N, C, 1) "latent" with one position per token row
            sel = (ts == val)
            idx = sel.reshape(-1).nonzero().squeeze(1)
            xs = lat.reshape(B * N, C)[idx].contiguous().reshape(-1, C, 1)
            vs = v.reshape(B * N, C)[idx].contiguous().reshape(-1, 1, C)
            if float(val) == 0.0:
                out.reshape(B * N, C)[idx] = xs.reshape(-1, C)
                continue
            x0 = ops.cfg_euler_step(vs, None, xs, 1.0, float(val), 0.0)
            out.reshape(B * N, C)[idx] = x0.reshape(-1, C)
        return out, None
