"""Text conditioning on the device: from the hidden states of a Gemma-3 forward to the (B, T, D) context of the DiT.

The reference's text path (mlx_video/models/ltx/text_encoder.py) is Gemma-3-12B followed by three LTX-2 modules whose
weights live in the LTX-2 checkpoint: ``norm_and_concat_hidden_states`` (591-639), ``GemmaFeaturesExtractor`` (642-649,
Linear(L*D -> D), no bias) and ``Embeddings1DConnector`` (426-587).  This module runs those three; Gemma itself, the
tokenizer and prompt enhancement are gemma.py's; the audio connector stays outside the package.  The input boundary is therefore "the
L hidden states of a stock Gemma-3 (``output_hidden_states=True``) plus its 0/1 attention mask", left-padded as the
reference tokenises.

What differs from a line-by-line port, and why it computes the same thing:

* Padded rows are never normalised, projected or stored.  The reference zeroes their features, projects the zeros and then
  overwrites those rows with the learnable registers (510-563), so nothing downstream ever sees them.  The valid rows of
  all batch rows form one compact (sum of counts, L*D) matrix; with 120 valid tokens of 1024 the 188160-wide projection runs
  over 120 rows per prompt instead of 1024.
* The compact matrix is layer-major (column l*D + d) where the reference stacks on the last axis (d*L + l).  The K axis
  of ``aggregate_embed.weight`` is permuted to match once, at load (``weights.aggregate_k_to_layer_major``), so the kernel
  that writes the matrix streams whole rows and no transposing store exists.
* Statistics stay in fp32 (the reference keeps them in bf16, including a bf16 denominator of the mean); every stage
  rounds to bf16 once, where the reference materialises a bf16 array.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

BF16 = torch.bfloat16
HEAD_DIM = 128
ROPE_THETA = 10000.0
ROPE_MAX_POS = 4096
NORM_EPS = 1e-6


def rope_table_1d(T: int, H: int, theta: float = ROPE_THETA, max_pos: int = ROPE_MAX_POS) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos, sin (H,T,64) fp32 of the connector's 1-D split RoPE (text_encoder.py:455-508): float64 on the host, positions
    2*t/max_pos - 1, frequencies theta^linspace(0,1,64*H) * pi/2, head h takes frequencies [64h, 64h+64); cast to fp32, rounded
    to bf16 (the reference hands the tables over in the activations' dtype: a rounding point, kept) and widened to fp32."""
    n = H * HEAD_DIM // 2
    freqs = np.power(float(theta), np.linspace(0.0, 1.0, n, dtype=np.float64)) * (np.pi / 2)
    pos = np.arange(T, dtype=np.float64) / float(max_pos) * 2 - 1
    ang = pos[:, None] * freqs[None, :]                                     # (T, 64*H)
    out = []
    for f in (np.cos, np.sin):
        t = torch.from_numpy(f(ang).reshape(T, H, HEAD_DIM // 2).transpose(1, 0, 2).astype(np.float32))
        out.append(t.to(BF16).to(torch.float32).contiguous())
    return out[0], out[1]


def mask_row_counts(attention_mask: torch.Tensor) -> List[int]:
    """Valid tokens per batch row of a (B,T) 0/1 mask, which must be left-padded: a run of zeros followed by a run of ones.
    Anything else is an error here - the reference slices ``hidden[T - sum(mask):]`` whatever the mask looks like."""
    if attention_mask.dim() != 2:
        raise ValueError(f"attention_mask must be (B,T), got {tuple(attention_mask.shape)}")
    m = attention_mask.detach().to("cpu")
    if m.dtype.is_floating_point:
        if not bool(((m == 0) | (m == 1)).all()):
            raise ValueError("attention_mask must hold 0 / 1 only")
    m = m.to(torch.int64)
    if not bool(((m == 0) | (m == 1)).all()):
        raise ValueError("attention_mask must hold 0 / 1 only")
    T = m.shape[1]
    counts = m.sum(dim=1).tolist()
    for b, c in enumerate(counts):
        if not bool(m[b, T - c:].all()):
            raise ValueError(f"attention_mask row {b} is not left-padded (a run of zeros followed by a run of ones): the valid "
                             f"tokens must be the last {c} positions")
    return [int(c) for c in counts]


class TextConnector:
    """``TextConnector(weights)(hidden_states, attention_mask) -> (B,T,D) bf16``: feature extractor + video embeddings
    connector on the device.  ``weights``: the dict of ``weights.text_connector_weights`` (device bf16 tensors):
    ``aggregate_embed.weight_layer_major`` (D, L*D) - or ``aggregate_embed.weight`` in the checkpoint's K order, permuted
    here - ``learnable_registers`` (R,D) and ``transformer_1d_blocks.{i}.{attn1.{to_q,to_k,to_v,to_out,q_norm,k_norm},
    ff.{proj_in,proj_out}}.*``.  Width, heads (D/128), blocks, register count and the number of hidden states L are read off
    the shapes."""

    def __init__(self, weights: Dict[str, torch.Tensor], audio_weights: Optional[Dict[str, torch.Tensor]] = None):
        reg = weights["learnable_registers"]
        self.device = reg.device
        self.R, self.D = (int(v) for v in reg.shape)
        if self.D % HEAD_DIM:
            raise ValueError(f"connector width {self.D} is not a multiple of the head dim {HEAD_DIM}")
        self.H = self.D // HEAD_DIM
        self.registers = reg.to(BF16).contiguous()
        if "aggregate_embed.weight_layer_major" in weights:
            agg = weights["aggregate_embed.weight_layer_major"]
        else:
            from .weights import aggregate_k_to_layer_major
            agg = aggregate_k_to_layer_major(weights["aggregate_embed.weight"], self.D)
        if agg.dim() != 2 or agg.shape[0] != self.D or agg.shape[1] % self.D:
            raise ValueError(f"aggregate_embed.weight must be ({self.D}, L*{self.D}), got {tuple(agg.shape)}")
        self.L = int(agg.shape[1]) // self.D
        self.agg = agg.to(BF16).contiguous()
        self.blocks = self._block_set(weights)
        # the audio embeddings connector (text_encoder.py:698, 838-871, 949-952): the same structure - its own registers and
        # blocks - over the SAME features; ``both`` runs the two sets over features computed once
        self.audio_registers = self.audio_blocks = None
        if audio_weights is not None:
            areg = audio_weights["learnable_registers"]
            if tuple(areg.shape) != (self.R, self.D):
                raise ValueError(f"the audio connector's learnable_registers are {tuple(areg.shape)}, the video connector's {(self.R, self.D)}")
            self.audio_registers = areg.to(BF16).contiguous()
            self.audio_blocks = self._block_set(audio_weights)
        self._rope: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}

    @staticmethod
    def _block_set(weights: Dict[str, torch.Tensor]) -> list:
        """The packed panels of one connector's ``transformer_1d_blocks.*``."""
        n = 1 + max((int(k.split(".")[1]) for k in weights if k.startswith("transformer_1d_blocks.")), default=-1)
        if n <= 0:
            raise ValueError("no transformer_1d_blocks.* in the connector weights")
        blocks = []
        for i in range(n):
            p = f"transformer_1d_blocks.{i}."
            g = lambda name: weights[p + name].to(BF16)
            blocks.append(dict(
                qkv_w=torch.cat([g("attn1.to_q.weight"), g("attn1.to_k.weight"), g("attn1.to_v.weight")], 0).contiguous(),
                qkv_b=torch.cat([g("attn1.to_q.bias"), g("attn1.to_k.bias"), g("attn1.to_v.bias")], 0).contiguous(),
                qkn=torch.stack([g("attn1.q_norm.weight"), g("attn1.k_norm.weight")], 0).contiguous(),
                o_w=g("attn1.to_out.weight").contiguous(), o_b=g("attn1.to_out.bias").contiguous(),
                ff1_w=g("ff.proj_in.weight").contiguous(), ff1_b=g("ff.proj_in.bias").contiguous(),
                ff2_w=g("ff.proj_out.weight").contiguous(), ff2_b=g("ff.proj_out.bias").contiguous()))
        return blocks

    # ------------------------------------------------------------------ stages
    def _tables(self, T: int):
        if T not in self._rope:
            c, s = rope_table_1d(T, self.H)
            self._rope[T] = (c.to(self.device), s.to(self.device))
        return self._rope[T]

    def _stack(self, hidden_states) -> torch.Tensor:
        if isinstance(hidden_states, (list, tuple)):
            hidden_states = torch.stack([h.to(self.device) for h in hidden_states], 0)       # the host stacks a list of layers
        x = hidden_states.to(self.device)
        if x.dim() != 4 or x.shape[0] != self.L or x.shape[3] != self.D:
            raise ValueError(f"hidden_states must be an (L,B,T,D) = ({self.L},B,T,{self.D}) stack or a list of {self.L} (B,T,{self.D}) "
                             f"tensors, got {tuple(x.shape)}")
        x = x.to(BF16)
        return x if x.stride(3) == 1 and all(s % 8 == 0 for s in x.stride()[:3]) and x.data_ptr() % 16 == 0 else x.contiguous()

    def features(self, hidden_states, counts: Sequence[int]) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
        """Compact (sum of counts, D) features of the valid tokens (normalise + aggregate_embed), plus the device tables
        (row0, row_count) that place them.  None when no row has a valid token."""
        x = self._stack(hidden_states)
        L, B, T, D = x.shape
        dev = self.device
        row0 = [0] * B
        for b in range(1, B):
            row0[b] = row0[b - 1] + counts[b - 1]
        rows = row0[-1] + counts[-1]
        cnt = torch.tensor(list(counts), dtype=torch.int32, device=dev)
        start = torch.tensor([T - c for c in counts], dtype=torch.int32, device=dev)
        r0 = torch.tensor(row0, dtype=torch.int32, device=dev)
        if rows == 0:
            return None, r0, cnt
        stats = ops.masked_layer_stats(x, start, cnt, valid_rows=rows)
        normed = torch.empty((rows, L * D), dtype=BF16, device=dev)
        ops.layer_norm_compact(x, start, cnt, r0, stats, normed, rows)
        # (small M over K = L*D: the library may split K - a 1.4-GB weight stream needs every CU; a row's bits then depend on
        # the total row count of the call, never on the run)
        return ops.gemm(normed, self.agg, None), r0, cnt

    def connect(self, x: torch.Tensor, blocks: Optional[list] = None) -> torch.Tensor:
        """Embeddings1DConnector on an assembled (B,T,D) input: the pre-norm blocks and the final unit RMSNorm.  No GEMM here
        is offered split-K and attention runs without its tail split, so a batch row's output does not depend on the batch.
        ``blocks``: the block set to run (None: the video connector's)."""
        B, T, D = x.shape
        H, M = self.H, B * T
        dev = x.device
        cos, sin = self._tables(T)
        x = x.reshape(M, D)
        nx = torch.empty_like(x)
        qk = torch.empty((M, 2 * D), dtype=BF16, device=dev)
        tpad = (T + 63) // 64 * 64
        vt = (torch.zeros if tpad != T else torch.empty)((B, D, tpad), dtype=BF16, device=dev)
        att = torch.empty((M, D), dtype=BF16, device=dev)
        scale = 1.0 / math.sqrt(HEAD_DIM)
        for blk in (self.blocks if blocks is None else blocks):
            ops.rmsnorm_rows(x, NORM_EPS, out=nx)
            ops.gemm(nx, blk["qkv_w"], blk["qkv_b"], out=qk, out2=vt, n_split=2 * D, out_tokens_per_batch=T, split_k=False)
            ops.qknorm_rope_1d(qk, D, blk["qkn"], cos, sin, T, H, NORM_EPS)
            ops.flash_attn(qk[:, :D], qk[:, D:], vt, att, B, H, T, T, scale, tail_split=False)
            ops.gemm(att, blk["o_w"], blk["o_b"], epilogue=ops.EPI_BIAS_RES, out=x, resid=x, split_k=False)
            ops.rmsnorm_rows(x, NORM_EPS, out=nx)
            h = ops.gemm(nx, blk["ff1_w"], blk["ff1_b"], split_k=False)
            ops.gelu_erf_(h)
            ops.gemm(h, blk["ff2_w"], blk["ff2_b"], epilogue=ops.EPI_BIAS_RES, out=x, resid=x, split_k=False)
        return ops.rmsnorm_rows(x, NORM_EPS).view(B, T, D)

    def both(self, hidden_states: Union[torch.Tensor, Sequence[torch.Tensor]], attention_mask: torch.Tensor,
             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(video context, audio context), each (B,T,D): the features are computed once and each connector assembles them with
        its own registers and runs its own blocks (text_encoder.py:943-952).  Needs ``audio_weights``."""
        if self.audio_blocks is None:
            raise ValueError("this TextConnector was built without the audio embeddings connector (audio_weights=)")
        counts, B, T = self._checked(hidden_states, attention_mask)
        feat, row0, cnt = self.features(hidden_states, counts)
        video = self.connect(ops.connector_assemble(feat, self.registers, row0, cnt, B, T))
        audio = self.connect(ops.connector_assemble(feat, self.audio_registers, row0, cnt, B, T), self.audio_blocks)
        return video, audio

    def _checked(self, hidden_states, attention_mask: torch.Tensor):
        counts = mask_row_counts(attention_mask)
        B, T = attention_mask.shape
        if T % self.R:
            raise ValueError(f"sequence length {T} is not a multiple of the {self.R} learnable registers (the reference tiles them "
                             f"T // {self.R} times over the sequence)")
        shape = tuple(hidden_states[0].shape) if isinstance(hidden_states, (list, tuple)) else tuple(hidden_states.shape[1:])
        if shape[:2] != (B, T):
            raise ValueError(f"hidden_states are {shape} per layer but attention_mask is {(B, T)}")
        return counts, B, T

    def __call__(self, hidden_states: Union[torch.Tensor, Sequence[torch.Tensor]], attention_mask: torch.Tensor) -> torch.Tensor:
        counts, B, T = self._checked(hidden_states, attention_mask)
        feat, row0, cnt = self.features(hidden_states, counts)
        return self.connect(ops.connector_assemble(feat, self.registers, row0, cnt, B, T))


def random_connector_weights(device, D: int = 3840, L: int = 49, layers: int = 2, R: int = 128, seed: int = 17,
                             generator_device=None) -> Dict[str, torch.Tensor]:
    """Seeded stand-in weights in the module-key layout (measurement scripts and tests; no checkpoint is read)."""
    g = torch.Generator(device=generator_device or "cpu").manual_seed(seed)

    def rn(*shape, std=1.0, mean=0.0):
        return (torch.randn(shape, generator=g, device=generator_device or "cpu") * std + mean).to(BF16).to(device)

    W = {"aggregate_embed.weight": rn(D, L * D, std=1.0 / math.sqrt(L * D)), "learnable_registers": rn(R, D)}
    for i in range(layers):
        p = f"transformer_1d_blocks.{i}."
        for name in ("to_q", "to_k", "to_v", "to_out"):
            W[p + f"attn1.{name}.weight"], W[p + f"attn1.{name}.bias"] = rn(D, D, std=1.0 / math.sqrt(D)), rn(D, std=0.02)
        W[p + "attn1.q_norm.weight"], W[p + "attn1.k_norm.weight"] = rn(D, std=0.1, mean=1.0), rn(D, std=0.1, mean=1.0)
        W[p + "ff.proj_in.weight"], W[p + "ff.proj_in.bias"] = rn(4 * D, D, std=1.0 / math.sqrt(D)), rn(4 * D, std=0.02)
        W[p + "ff.proj_out.weight"], W[p + "ff.proj_out.bias"] = rn(D, 4 * D, std=1.0 / math.sqrt(4 * D)), rn(D, std=0.02)
    return W
