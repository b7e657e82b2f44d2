"""The Gemma-3 text encoder on the device: token ids to the L+1 hidden states ``TextConnector`` consumes.

The reference wraps ``mlx_vlm``'s Gemma3Model (mlx_video/models/ltx/text_encoder.py:47-152, ``LanguageModel``).  The wrapper is
followed: the embedding scale rounded to bf16 (:107), left padding with the combined causal-and-padding mask (:58-81), and the
list ``[embeddings, h_1 .. h_{L-1}, norm(h_L)]`` of L+1 states (:110-148).  The decoder layer is the Gemma-3 definition as
``transformers`` implements it (``Gemma3TextModel``): (1 + w) RMSNorms before and after attention and feed-forward, per-head
q/k norms, rotate-half RoPE with a local and a (linearly scaled) global base, grouped-query attention at head dim 256 scaled by
``query_pre_attn_scalar ** -0.5``, a tanh-GeGLU feed-forward, no biases.

What differs from the reference's mask, and why it computes the same thing: local layers pass the config's sliding window
to the attention kernel (key j visible to query i iff i - j < window), where the reference uses the full causal mask on every
layer (:116-132).  The two agree for every T <= window, and the reference's tokeniser call (:929-935, max_length 1024, window
1024) never produces another length.

The run stays on the padded (B,T) layout.  Padded rows carry finite values through the row kernels and GEMMs and nothing
reads them: attention never admits a key below row_start and writes zeros to query rows below it.  Every GEMM is called with
``split_k=False`` and the attention kernel never splits keys, so a batch row's bits do not depend on the batch.

FP8 panels (``GemmaEncoder(..., fp8=)``): the projections and the tied embedding table held as e4m3fn with
``weights.quantize_fp8``'s per-row scale - half the resident bytes and half the bytes a decoded token streams.  The encoder's
GEMMs are ltxk_gemm_w8 (fp8 through memory, widened in front of the same MFMAs), the gather is ltxk_embed_rows_fp8; on such an
encoder the generator's M = B-row GEMMs are ltxk_gemv_w8, one launch each instead of a split-K pair.

Decoding (``GemmaCache``, ``GemmaGenerator``, ``enhance_prompt``): the reference's prompt enhancement (text_encoder.py:1023-1135)
generates with ``mlx_lm``; here a prefill is the encoder's own layer loop writing K and V^T into a per-layer cache, and a token is
one pass of M = B-row GEMMs (the weight-streaming split-K form) with the single-position attention step against that cache.
"""
from __future__ import annotations

import json
import math
import re
import warnings
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .text_connector import mask_row_counts
from .weights import FP8_SCALINGS, MXFP4_BLOCK, SCALE_SUFFIX, quantize_fp8, quantize_mxfp4

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
HEAD_DIM = 256
MAX_TOKENS = 1024           # the reference's tokeniser call: max_length 1024, left-padded (text_encoder.py:929-935)


@dataclass(frozen=True)
class GemmaConfig:
    hidden_size: int = 3840
    num_hidden_layers: int = 48
    num_attention_heads: int = 16
    num_key_value_heads: int = 8
    head_dim: int = 256
    intermediate_size: int = 15360
    vocab_size: int = 262208
    sliding_window: int = 1024
    layer_types: Tuple[str, ...] = field(default=())      # "sliding_attention" / "full_attention" per layer; () = by pattern
    sliding_window_pattern: int = 6
    query_pre_attn_scalar: float = 256.0
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1_000_000.0                       # global layers
    rope_local_base_freq: float = 10_000.0                # local (sliding) layers
    rope_scaling_factor: float = 1.0                      # linear position scaling of the global layers
    final_logit_softcapping: Optional[float] = None       # the generator refuses a non-null value (the encoder forms no logits)

    def __post_init__(self):
        if self.head_dim != HEAD_DIM:
            raise ValueError(f"GemmaConfig: head_dim {self.head_dim} is not supported (the attention kernel is built for {HEAD_DIM})")
        if self.num_attention_heads % self.num_key_value_heads:
            raise ValueError(f"GemmaConfig: {self.num_attention_heads} heads are not a multiple of {self.num_key_value_heads} KV heads")
        if self.hidden_size % 8 or self.intermediate_size % 8:
            raise ValueError("GemmaConfig: hidden and intermediate sizes must be multiples of 8")
        if self.layer_types and len(self.layer_types) != self.num_hidden_layers:
            raise ValueError(f"GemmaConfig: {len(self.layer_types)} layer_types for {self.num_hidden_layers} layers")
        bad = set(self.layer_types) - {"sliding_attention", "full_attention"}
        if bad:
            raise ValueError(f"GemmaConfig: unknown layer types {sorted(bad)}")
        if self.sliding_window <= 0 or self.sliding_window_pattern <= 0:
            raise ValueError("GemmaConfig: sliding_window and sliding_window_pattern must be positive")

    def is_global(self, i: int) -> bool:
        """Layer i attends globally: by ``layer_types`` when the config lists them, else i % pattern == pattern - 1
        (text_encoder.py:123-126)."""
        if self.layer_types:
            return self.layer_types[i] == "full_attention"
        return i % self.sliding_window_pattern == self.sliding_window_pattern - 1

    @staticmethod
    def from_dict(cfg: dict) -> "GemmaConfig":
        """From a Gemma-3 ``config.json`` dict: the ``text_config`` entry when there is one, else the top level
        (text_encoder.py:222-227).  Rope fields in either spelling: ``rope_theta`` / ``rope_local_base_freq`` / ``rope_scaling``
        or the ``rope_parameters`` dict of newer ``transformers`` ({"full_attention": {...}, "sliding_attention": {...}})."""
        c = cfg.get("text_config", cfg)
        if c.get("attn_logit_softcapping") is not None:
            raise ValueError(f"GemmaConfig: attn_logit_softcapping={c['attn_logit_softcapping']}: attention soft-capping is not supported")
        d = GemmaConfig()
        theta, local, factor = c.get("rope_theta", d.rope_theta), c.get("rope_local_base_freq", d.rope_local_base_freq), 1.0
        scaling = c.get("rope_scaling")
        rp = c.get("rope_parameters")
        if rp:
            full, slide = rp.get("full_attention") or {}, rp.get("sliding_attention") or {}
            theta, local = full.get("rope_theta", theta), slide.get("rope_theta", local)
            if slide.get("rope_type", "default") != "default":
                raise ValueError(f"GemmaConfig: rope type {slide.get('rope_type')!r} on the local layers is not supported")
            scaling = full if full.get("rope_type", "default") != "default" else scaling
        if scaling:
            kind = scaling.get("rope_type", scaling.get("type", "linear"))
            if kind != "linear":
                raise ValueError(f"GemmaConfig: rope scaling {kind!r} is not supported (Gemma-3 uses linear)")
            factor = float(scaling.get("factor", 1.0))
        lt = c.get("layer_types")
        return GemmaConfig(
            hidden_size=int(c.get("hidden_size", d.hidden_size)), num_hidden_layers=int(c.get("num_hidden_layers", d.num_hidden_layers)),
            num_attention_heads=int(c.get("num_attention_heads", d.num_attention_heads)),
            num_key_value_heads=int(c.get("num_key_value_heads", d.num_key_value_heads)), head_dim=int(c.get("head_dim", d.head_dim)),
            intermediate_size=int(c.get("intermediate_size", d.intermediate_size)), vocab_size=int(c.get("vocab_size", d.vocab_size)),
            sliding_window=int(c.get("sliding_window", d.sliding_window)), layer_types=tuple(lt) if lt else (),
            sliding_window_pattern=int(c.get("sliding_window_pattern", d.sliding_window_pattern)),
            query_pre_attn_scalar=float(c.get("query_pre_attn_scalar", d.query_pre_attn_scalar)),
            rms_norm_eps=float(c.get("rms_norm_eps", d.rms_norm_eps)), rope_theta=float(theta), rope_local_base_freq=float(local),
            rope_scaling_factor=factor,
            final_logit_softcapping=None if c.get("final_logit_softcapping") is None else float(c["final_logit_softcapping"]))

    @staticmethod
    def from_json(path: Union[str, Path]) -> "GemmaConfig":
        p = Path(path)
        p = p / "config.json" if p.is_dir() else p
        with open(p) as f:
            return GemmaConfig.from_dict(json.load(f))


def rope_table_half(T: int, base: float, factor: float = 1.0, dim: int = HEAD_DIM) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos, sin (T, dim/2) fp32 of the rotate-half RoPE: angle(t, i) = (t / factor) * base^(-2i/dim), float64 on the host,
    rounded to bf16 (the model hands the tables over in the activations' dtype: a rounding point, kept) and widened -
    ``rope_table_1d``'s convention."""
    inv = 1.0 / np.power(float(base), np.arange(0, dim, 2, dtype=np.float64) / dim) / float(factor)
    ang = np.arange(T, dtype=np.float64)[:, None] * inv[None, :]
    return tuple(torch.from_numpy(f(ang).astype(np.float32)).to(BF16).to(torch.float32).contiguous() for f in (np.cos, np.sin))


class GemmaEncoder:
    """``GemmaEncoder(weights, config)(input_ids, attention_mask) -> (L+1, B, T, D) bf16`` on the device.  ``weights``: device
    bf16 tensors under the language model's own keys (``embed_tokens.weight``, ``layers.{i}.self_attn.{q,k,v,o}_proj.weight``,
    ``...self_attn.{q,k}_norm.weight``, ``...mlp.{gate,up,down}_proj.weight``, the four layer norms, ``norm.weight``)
    - what ``weights.gemma_weights`` returns.  The q|k|v and gate|up panels are stacked once, here; the dict's own tensors of
    those are not kept.

    ``fp8`` ("channel" / "none", ``weights.FP8_SCALINGS``): q|k|v, o, gate|up, down and the embedding table are kept as e4m3fn
    with ``quantize_fp8``'s per-row scale ("none": the plain cast, no scale); norm weights stay bf16.  Each matrix is quantised
    on its own as the panels are built and its entry is REMOVED from ``weights``, so that with no other reference held the bf16
    source is released before the next one is converted (a full bf16 model and its fp8 copy are never resident together).  A
    per-row scale belongs to its row alone, so the scales of q, k and v concatenated are the scale of the q|k|v panel.  Matrices
    that already are e4m3fn (with their ``key + SCALE_SUFFIX`` scale, or none: ``gemma_weights(..., fp8=)``) are taken as they
    are, with or without ``fp8``.  Gemma-3 ties the output head to the embedding table: its one per-row scale serves the gather
    (row = token) and the logits GEMM (row = output channel)."""

    def __init__(self, weights: Dict[str, torch.Tensor], config: GemmaConfig, fp8: Optional[str] = None):
        self.cfg = c = config
        if fp8 is not None and fp8 not in FP8_SCALINGS:
            raise ValueError(f"GemmaEncoder: fp8={fp8!r}: expected None or one of {FP8_SCALINGS}")
        if "embed_tokens.weight" not in weights:
            raise ValueError("no embed_tokens.weight in the Gemma weights (expected the keys of weights.gemma_weights)")
        given = weights["embed_tokens.weight"].dtype == FP8
        self.weight_dtype = FP8 if (fp8 is not None or given) else BF16
        f8 = self.weight_dtype == FP8
        g = lambda k: weights[k].to(BF16).contiguous()

        def mat(*keys):
            """(panel, per-row fp32 scale or None) of the matrices under ``keys`` stacked along their rows."""
            if not f8:
                return (g(keys[0]) if len(keys) == 1 else torch.cat([g(k) for k in keys], 0).contiguous()), None
            parts = []
            for k in keys:
                w = weights.pop(k)
                if w.dtype == FP8:
                    sc = weights.pop(k + SCALE_SUFFIX, None)
                    parts.append((w.contiguous(), None if sc is None else sc.to(torch.float32).contiguous()))
                elif fp8 is None:
                    raise ValueError(f"{k} is {w.dtype} beside float8_e4m3fn matrices: pass fp8= to have the rest quantised")
                else:
                    parts.append(quantize_fp8(w.to(BF16), fp8))
                del w
            scaled = any(sc is not None for _, sc in parts)
            w8 = parts[0][0] if len(parts) == 1 else torch.cat([w.view(torch.uint8) for w, _ in parts], 0).view(FP8)
            sc = None
            if scaled:
                sc = torch.cat([sc if sc is not None else torch.ones(w.shape[0], dtype=torch.float32, device=w.device) for w, sc in parts], 0)
            return w8.contiguous(), (None if sc is None else sc.contiguous())

        self.embed, self.embed_row_scale = mat("embed_tokens.weight")
        self.device = self.embed.device
        if tuple(self.embed.shape[1:]) != (c.hidden_size,):
            raise ValueError(f"embed_tokens.weight is {tuple(self.embed.shape)}, the config's hidden size {c.hidden_size}")
        if f8 and c.hidden_size % 16:
            raise ValueError(f"GemmaEncoder: fp8 panels need a hidden size that is a multiple of 16, got {c.hidden_size}")
        self.vocab = int(self.embed.shape[0])
        self.norm = g("norm.weight")
        self.embed_scale = float(torch.tensor(c.hidden_size ** 0.5, dtype=BF16))          # text_encoder.py:107
        self.scale = float(c.query_pre_attn_scalar) ** -0.5
        nq, nkv = c.num_attention_heads * HEAD_DIM, c.num_key_value_heads * HEAD_DIM
        self.layers = []
        for i in range(c.num_hidden_layers):
            q = f"layers.{i}."
            qkv, qkv_s = mat(q + "self_attn.q_proj.weight", q + "self_attn.k_proj.weight", q + "self_attn.v_proj.weight")
            gu, gu_s = mat(q + "mlp.gate_proj.weight", q + "mlp.up_proj.weight")
            if tuple(qkv.shape) != (nq + 2 * nkv, c.hidden_size) or tuple(gu.shape) != (2 * c.intermediate_size, c.hidden_size):
                raise ValueError(f"layer {i}: q|k|v panel {tuple(qkv.shape)} / gate|up panel {tuple(gu.shape)} do not match the config")
            o, o_s = mat(q + "self_attn.o_proj.weight")
            down, down_s = mat(q + "mlp.down_proj.weight")
            self.layers.append(dict(
                qkv=qkv, gu=gu, o=o, down=down, qkv_s=qkv_s, gu_s=gu_s, o_s=o_s, down_s=down_s,
                qn=g(q + "self_attn.q_norm.weight"), kn=g(q + "self_attn.k_norm.weight"),
                n_in=g(q + "input_layernorm.weight"), n_post_attn=g(q + "post_attention_layernorm.weight"),
                n_pre_ff=g(q + "pre_feedforward_layernorm.weight"), n_post_ff=g(q + "post_feedforward_layernorm.weight"),
                window=0 if c.is_global(i) else c.sliding_window, is_global=c.is_global(i)))
        self._rope: Dict[Tuple[int, bool], Tuple[torch.Tensor, torch.Tensor]] = {}

    def weight_bytes(self) -> int:
        """Bytes of every resident weight tensor: panels, their scales, the embedding table and the norm weights."""
        ts = [self.embed, self.embed_row_scale, self.norm] + [v for ly in self.layers for v in ly.values()]
        return sum(t.numel() * t.element_size() for t in ts if isinstance(t, torch.Tensor))

    def _tables(self, T: int, is_global: bool):
        key = (T, is_global)
        if key not in self._rope:
            c = self.cfg
            cs = rope_table_half(T, c.rope_theta, c.rope_scaling_factor) if is_global else rope_table_half(T, c.rope_local_base_freq)
            self._rope[key] = tuple(t.to(self.device) for t in cs)
        return self._rope[key]

    def __call__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        return self._forward(input_ids, attention_mask, None)

    def _forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, cache: Optional["GemmaCache"]) -> torch.Tensor:
        """The forward over the padded (B,T) layout.  With a ``cache`` (a prefill) each layer's GEMM writes V^T straight into the
        cache's (B, Hkv*256, cap) buffer instead of the scratch one and the rotated K columns are copied into its K rows; the
        launches, and so the states' bits, are the same."""
        counts = mask_row_counts(attention_mask)
        if input_ids.dim() != 2 or tuple(input_ids.shape) != tuple(attention_mask.shape):
            raise ValueError(f"input_ids {tuple(input_ids.shape)} and attention_mask {tuple(attention_mask.shape)} must be one (B,T) shape")
        if input_ids.dtype.is_floating_point or input_ids.dtype == torch.bool:
            raise TypeError(f"input_ids must be integers, got {input_ids.dtype}")
        c, dev = self.cfg, self.device
        B, T = input_ids.shape
        M, D, F = B * T, c.hidden_size, c.intermediate_size
        Hq, Hkv = c.num_attention_heads, c.num_key_value_heads
        nq, nkv = Hq * HEAD_DIM, Hkv * HEAD_DIM
        ids_host = input_ids.detach().to("cpu").reshape(-1)
        ids = ids_host.to(torch.int32).to(dev)
        row_start = torch.tensor([T - n for n in counts], dtype=torch.int32, device=dev)
        L = c.num_hidden_layers
        states = torch.empty((L + 1, B, T, D), dtype=BF16, device=dev)
        x = ops.embed_rows(self.embed, ids, self.embed_scale, out=states[0].view(M, D), ids_host=ids_host, row_scale=self.embed_row_scale)
        nx = torch.empty((M, D), dtype=BF16, device=dev)
        qk = torch.empty((M, nq + nkv), dtype=BF16, device=dev)
        tpad = (T + 63) // 64 * 64
        vt = None
        if cache is None:
            vt = (torch.zeros if tpad != T else torch.empty)((B, nkv, tpad), dtype=BF16, device=dev)      # pad columns stay finite
        att = torch.empty((M, nq), dtype=BF16, device=dev)
        po = torch.empty((M, D), dtype=BF16, device=dev)
        gu = torch.empty((M, 2 * F), dtype=BF16, device=dev)
        for i, ly in enumerate(self.layers):
            cos, sin = self._tables(T, ly["is_global"])
            if cache is not None:
                vt = cache.vt[i]
            ops.rmsnorm_weight_rows(x, ly["n_in"], c.rms_norm_eps, out=nx)
            ops.gemm(nx, ly["qkv"], None, out=qk, out2=vt, n_split=nq + nkv, out_tokens_per_batch=T, split_k=False, w_scale=ly["qkv_s"])
            ops.headnorm_rope(qk, Hq, Hkv, ly["qn"], ly["kn"], cos, sin, T, c.rms_norm_eps)
            if cache is not None:
                cache.k[i][:, :T].copy_(qk.view(B, T, nq + nkv)[:, :, nq:])
            ops.causal_attn(qk[:, :nq], qk[:, nq:], vt, att, row_start, B, Hq, Hkv, T, self.scale, window=ly["window"])
            ops.gemm(att, ly["o"], None, out=po, split_k=False, w_scale=ly["o_s"])
            # the layer's output goes straight into its slot of the stack (the last layer's into scratch: its slot takes norm(h_L))
            y = states[i + 1].view(M, D) if i + 1 < L else nx.new_empty((M, D))
            ops.rmsnorm_weight_rows(po, ly["n_post_attn"], c.rms_norm_eps, resid=x, out=y)
            ops.rmsnorm_weight_rows(y, ly["n_pre_ff"], c.rms_norm_eps, out=nx)
            ops.gemm(nx, ly["gu"], None, out=gu, split_k=False, w_scale=ly["gu_s"])
            h = ops.geglu_tanh_(gu)
            ops.gemm(h, ly["down"], None, out=po, split_k=False, w_scale=ly["down_s"])
            ops.rmsnorm_weight_rows(po, ly["n_post_ff"], c.rms_norm_eps, resid=y, out=y)
            x = y
        ops.rmsnorm_weight_rows(x, self.norm, c.rms_norm_eps, out=states[L].view(M, D))
        if cache is not None:
            cache.row_start, cache.length = row_start, T
        return states


# ------------------------------------------------------------------------------------------------------------ decoding
class GemmaCache:
    """The KV cache of one generation: per layer K (B, cap, Hkv*256) and V^T (B, Hkv*256, cap) bf16 - the attention kernels'
    own operand layouts, zero-initialised so that positions past the live length are finite - and the attention step's
    fp32 ``partials`` (one buffer: the launches of a stream are ordered, so the layers share it).  ``length``: the live
    length = the padded-sequence position of the next token; ``row_start`` (B) int32 on the device, set by the prefill."""

    def __init__(self, config: GemmaConfig, B: int, capacity: int, device):
        if capacity < 1 or capacity % ops.CAUSAL_ATTN_BK:
            raise ValueError(f"GemmaCache: capacity {capacity} must be a positive multiple of {ops.CAUSAL_ATTN_BK}")
        nkv = config.num_key_value_heads * HEAD_DIM
        L = config.num_hidden_layers
        self.capacity, self.B, self.length = int(capacity), int(B), 0
        self.k = [torch.zeros((B, capacity, nkv), dtype=BF16, device=device) for _ in range(L)]
        self.vt = [torch.zeros((B, nkv, capacity), dtype=BF16, device=device) for _ in range(L)]
        slices = -(-capacity // ops.CAUSAL_ATTN_STEP_SLICE)
        self.partials = torch.empty(B * config.num_attention_heads * slices * ops.CAUSAL_ATTN_STEP_PART, dtype=torch.float32, device=device)
        self.row_start: Optional[torch.Tensor] = None


def apply_repetition_penalty(logits: torch.Tensor, context: Sequence[Sequence[int]], penalty: float) -> torch.Tensor:
    """(B,V) fp32 logits with the ids of ``context[b]`` penalised: a negative logit is multiplied by ``penalty``, any other divided
    by it - the rule of ``transformers``' RepetitionPenaltyLogitsProcessor (and of mlx_lm's make_logits_processors, which the
    reference calls).  A new tensor."""
    out = logits.clone()
    for b, ctx in enumerate(context):
        if len(ctx) and penalty != 1.0:
            idx = torch.tensor(sorted(set(int(t) for t in ctx)), dtype=torch.int64, device=logits.device)
            sc = out[b, idx]
            out[b, idx] = torch.where(sc < 0, sc * penalty, sc / penalty)
    return out


def sample_tokens(logits: torch.Tensor, context: Sequence[Sequence[int]], temperature: float, repetition_penalty: float,
                  generator: Optional[torch.Generator]) -> torch.Tensor:
    """One token per row of (B,V) fp32 host logits: the repetition penalty over ``context[b]``, then argmax at temperature 0,
    else a categorical draw from softmax(logits / temperature) with ``generator``.  (B,) int64."""
    lg = apply_repetition_penalty(logits.detach().to("cpu").to(torch.float32), context, repetition_penalty)
    if temperature == 0:
        return lg.argmax(-1)
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    return torch.multinomial(torch.softmax(lg / temperature, -1), 1, generator=generator)[:, 0]


class GemmaDecodeState:
    """What a decode step reads and writes, all on the device, so that the step is the same launches on the same addresses
    every token and can be recorded once as a graph (``GemmaGenerator.device_step``): the sampler's state (``ops.sample_rows``;
    int32) - ``ctl`` = {n, pos, live}: the draw index, the cache position at which the token drawn now is fed, the rows not
    finished; ``done`` (B), ``next_ids`` (B), ``history`` (B, Hcap) / ``hist_len`` (B) initialised from the prompt's valid tokens,
    ``tokens_out`` (B, max_tokens), ``eos``, ``uniforms`` (max_tokens, B) fp32 = ``torch.rand`` of a CPU generator seeded with
    ``seed``, uploaded once - and the step's static activations: ``x`` (2, B, D) (a layer reads one and writes the other), ``nx``,
    ``qkv``, ``att``, ``po``, ``gu`` and the (B, V) bf16 ``logits`` the sampler reads."""

    def __init__(self, config: GemmaConfig, vocab: int, input_ids: torch.Tensor, attention_mask: torch.Tensor, max_tokens: int,
                 eos_ids: Sequence[int], seed: int, device):
        B, T = input_ids.shape
        if not 1 <= B <= ops.SAMPLE_MAX_B:
            raise ValueError(f"GemmaDecodeState: the device loop takes 1 to {ops.SAMPLE_MAX_B} batch rows, got {B}")
        if max_tokens < 1:
            raise ValueError(f"GemmaDecodeState: max_tokens = {max_tokens} must be positive")
        eos = sorted(set(int(t) for t in eos_ids))
        if len(eos) > ops.SAMPLE_MAX_EOS:
            raise ValueError(f"GemmaDecodeState: at most {ops.SAMPLE_MAX_EOS} EOS ids, got {len(eos)}")
        c = config
        D, F = c.hidden_size, c.intermediate_size
        nq, nkv = c.num_attention_heads * HEAD_DIM, c.num_key_value_heads * HEAD_DIM
        self.B, self.T, self.max_tokens, self.vocab = int(B), int(T), int(max_tokens), int(vocab)
        ids_host, mask_host = input_ids.detach().to("cpu"), attention_mask.detach().to("cpu").bool()
        hcap = T + max_tokens
        hist = torch.zeros((B, hcap), dtype=torch.int32)
        hlen = torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            valid = ids_host[b][mask_host[b]].to(torch.int32)
            hist[b, :valid.numel()] = valid
            hlen[b] = valid.numel()
        i32 = lambda t: t.to(torch.int32).to(device)          # noqa: E731
        self.ctl = i32(torch.tensor([0, T, B]))
        self.done, self.next_ids = i32(torch.zeros(B)), i32(torch.zeros(B))
        self.history, self.hist_len = hist.to(device), hlen.to(device)
        self.tokens_out = torch.full((B, max_tokens), -1, dtype=torch.int32, device=device)
        self.eos = i32(torch.tensor(eos, dtype=torch.int32))
        self.uniforms = torch.rand((max_tokens, B), generator=torch.Generator(device="cpu").manual_seed(int(seed))).to(device)
        self.workspace = torch.empty(ops.sample_workspace_floats(B, vocab), dtype=torch.float32, device=device)
        bf = lambda *shape: torch.empty(shape, dtype=BF16, device=device)          # noqa: E731
        self.x, self.nx, self.qkv, self.att = bf(2, B, D), bf(B, D), bf(B, nq + 2 * nkv), bf(B, nq)
        self.po, self.gu, self.logits = bf(B, D), bf(B, 2 * F), bf(B, vocab)

    @property
    def pos(self) -> torch.Tensor:
        """The (1,) int32 view of ctl's position: what the device-position kernels read."""
        return self.ctl[1:2]

    def read(self) -> Tuple[int, int, int, torch.Tensor]:
        """(n, pos, live, tokens_out on the host): the loop's one small device-to-host copy."""
        ctl = self.ctl.to("cpu")
        return int(ctl[0]), int(ctl[1]), int(ctl[2]), self.tokens_out.to("cpu")


class GemmaGenerator:
    """KV-cached autoregressive decoding on a ``GemmaEncoder``'s panels (nothing is copied; Gemma-3 ties the output head to
    the embedding table).  ``prefill`` runs the encoder's layer loop into a ``GemmaCache``; ``step`` runs one token: per layer
    the input norm, one q|k|v GEMM at M = B rows in the weight-streaming split-K form, norm + RoPE with the table row of the
    token's position, the attention step against the cache (which appends the token's K and V), o-proj, norms, gate|up, GeGLU,
    down; then the final norm and the logits GEMM over the embedding table.  Positions are padded-sequence indices, the
    encoder's convention.

    On an fp8 encoder with B <= ``ops.GEMV_MAX_M`` the GEMMs of ``GEMV_SHAPES`` run as ltxk_gemv_w8 (``ops.gemm(gemv=True)``): one
    launch that streams the e4m3 panel straight to registers, and a batch row's bits then do not depend on B.  ``gemv=False``
    keeps every one of them on the split-K ltxk_gemm_w8 (the measurement's other arm); a bf16 encoder's step is unchanged.

    ``decode_panels="mxfp4"`` (opt-in; None is the generator above, launch for launch): the generator builds, layer by layer, an
    OCP MXFP4 copy (``weights.quantize_mxfp4``: e2m1 codes, one e8m0 scale per 32 k; 4.25 bits per weight) of those of q|k|v, o,
    gate|up, down and the tied table whose ``GEMV4_SHAPES`` entry is true when it is built (``routing4`` keeps that table; a
    subclass with another ``GEMV4_SHAPES`` routes otherwise), from the encoder's panels - a bf16 panel as it is, an fp8 panel
    as code * row scale in fp32, in row chunks, so that never more than one widened chunk is held - and ``step`` / ``device_step`` run a GEMM of ``GEMV4_SHAPES``
    at B <= ``GEMV4_MAX_B`` as ltxk_gemv_w4 on the copy (otherwise the path above, on the encoder's panel).  The table copy
    serves the steps' logits only: the embedding gather and ``prefill`` (its logits included) stay on the encoder's panels, so
    the K / V of the prompt come from the bf16 / fp8 weights and those of the decoded tokens from the MXFP4 ones - the two are
    4-bit roundings apart, as a 4-bit model's cache would be against its 16-bit prefill.  The hidden states that condition the
    DiT never touch the copy.  The routing is host-static and the panels are fixed buffers, so the device loop and its graph
    replay work unchanged.  Every K (hidden size, Hq * 256, intermediate size) must be a multiple of 32."""

    # which of the step's five GEMMs take the row-streaming kernel on fp8 panels (decided per shape by measurement)
    GEMV_SHAPES = {"qkv": True, "o": True, "gu": True, "down": True, "logits": True}
    # which of them take ltxk_gemv_w4 on MXFP4 decode panels (decided per shape by measurement at B = 1 - q|k|v and o
    # are launch-bound 12 - 14 us either way and stay on the encoder's panel), and up to which batch: at 5 - 8 rows ltxk_gemv_w8 is
    # the faster kernel on four of the five shapes.  Both were measured against ltxk_gemv_w8 on an fp8 encoder only; on a bf16
    # encoder the other path is the split-K bf16 GEMM, which nobody has measured against ltxk_gemv_w4
    GEMV4_SHAPES = {"qkv": False, "o": False, "gu": True, "down": True, "logits": True}
    GEMV4_MAX_B = 4
    MXFP4_CHUNK_ROWS = 8192          # rows widened to fp32 at a time while the copy is built

    def __init__(self, encoder: GemmaEncoder, gemv: bool = True, decode_panels: Optional[str] = None):
        if encoder.cfg.final_logit_softcapping is not None:
            raise ValueError(f"GemmaGenerator: final_logit_softcapping={encoder.cfg.final_logit_softcapping}: logit soft-capping is not supported")
        if encoder.cfg.num_attention_heads // encoder.cfg.num_key_value_heads > 16:
            raise ValueError("GemmaGenerator: more than 16 query heads per KV head are not supported by the attention step")
        if encoder.vocab % 8:
            raise ValueError(f"GemmaGenerator: the vocabulary {encoder.vocab} must be a multiple of 8 (the logits GEMM)")
        self.enc, self.cfg = encoder, encoder.cfg
        self.gemv = bool(gemv) and encoder.weight_dtype == FP8
        if decode_panels not in (None, "mxfp4"):
            raise ValueError(f"GemmaGenerator: decode_panels={decode_panels!r}: expected None or 'mxfp4'")
        self.decode_panels = decode_panels
        # per layer {"qkv" | "o" | "gu" | "down": (codes, block_scales)}, and the table's pair; None without decode_panels
        self.panels4: Optional[List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]] = None
        self.table4: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self.routing4: Dict[str, bool] = {}
        if decode_panels == "mxfp4":
            c = encoder.cfg
            for name, k in (("hidden_size", c.hidden_size), ("num_attention_heads * 256", c.num_attention_heads * HEAD_DIM),
                            ("intermediate_size", c.intermediate_size)):
                if k % MXFP4_BLOCK:
                    raise ValueError(f"GemmaGenerator: decode_panels='mxfp4' needs {name} = {k} to be a multiple of {MXFP4_BLOCK}")
            # only the shapes routed to ltxk_gemv_w4 get a copy: the table as it stands when the generator is built
            self.routing4 = dict(self.GEMV4_SHAPES)
            self.panels4 = [{n: self._mxfp4(ly[n], ly[n + "_s"]) for n in ("qkv", "o", "gu", "down") if self.routing4[n]}
                            for ly in encoder.layers]
            if self.routing4["logits"]:
                self.table4 = self._mxfp4(encoder.embed, encoder.embed_row_scale)

    def _mxfp4(self, w: torch.Tensor, row_scale: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The MXFP4 pair of one of the encoder's panels: rows are independent, so it is built ``MXFP4_CHUNK_ROWS`` rows at a time
        from the chunk widened to fp32 (an fp8 chunk times its rows' scales)."""
        codes = torch.empty((w.shape[0], w.shape[1] // 2), dtype=torch.uint8, device=w.device)
        scales = torch.empty((w.shape[0], w.shape[1] // MXFP4_BLOCK), dtype=torch.uint8, device=w.device)
        for r0 in range(0, w.shape[0], self.MXFP4_CHUNK_ROWS):
            r1 = min(r0 + self.MXFP4_CHUNK_ROWS, w.shape[0])
            wide = w[r0:r1].to(torch.float32)
            if row_scale is not None:
                wide = wide * row_scale[r0:r1, None]
            codes[r0:r1], scales[r0:r1] = quantize_mxfp4(wide)
            del wide
        return codes, scales

    def _p4(self, layer: Optional[int], which: str) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """The MXFP4 pair a step's GEMM is routed to (``layer`` None: the table), or None: the encoder's panel."""
        if self.panels4 is None or not self.routing4[which]:
            return None
        return self.table4 if layer is None else self.panels4[layer][which]

    def decode_weight_bytes(self, B: int = 1) -> int:
        """The weight bytes one decoded token of ``B`` batch rows streams: the five GEMMs' panels as ``step`` routes them (an MXFP4
        pair's codes and block scales, or the encoder's panel and its row scales), the norm weights, and the B gathered rows of
        the embedding table."""
        e = self.enc
        nb = lambda *ts: sum(t.numel() * t.element_size() for t in ts if isinstance(t, torch.Tensor))      # noqa: E731
        w4 = B <= min(self.GEMV4_MAX_B, ops.GEMV4_MAX_M)
        total = nb(e.norm) + B * (e.embed.shape[1] * e.embed.element_size() + (4 if e.embed_row_scale is not None else 0))
        for i, ly in enumerate(e.layers):
            total += nb(ly["qn"], ly["kn"], ly["n_in"], ly["n_post_attn"], ly["n_pre_ff"], ly["n_post_ff"])
            for n in ("qkv", "o", "gu", "down"):
                p4 = self._p4(i, n) if w4 else None
                total += nb(*p4) if p4 is not None else nb(ly[n], ly[n + "_s"])
        p4 = self._p4(None, "logits") if w4 else None
        return total + (nb(*p4) if p4 is not None else nb(e.embed, e.embed_row_scale))

    def _gemm(self, which: str, a: torch.Tensor, w: torch.Tensor, w_scale: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
              p4: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
        """One M = B-row GEMM of a step: ltxk_gemv_w4 on the MXFP4 pair ``p4`` when the step hands one over (``_p4``), else
        ltxk_gemv_w8 where the shape is routed there, else the weight-streaming split-K form."""
        if p4 is not None and a.shape[0] <= min(self.GEMV4_MAX_B, ops.GEMV4_MAX_M):
            return ops.gemv_w4(a, p4[0], p4[1], None, out=out)
        if self.gemv and self.GEMV_SHAPES[which] and a.shape[0] <= ops.GEMV_MAX_M and a.shape[1] % 16 == 0:
            return ops.gemm(a, w, None, out=out, w_scale=w_scale, gemv=True)
        return ops.gemm(a, w, None, out=out, split_k=True, w_scale=w_scale)

    def _logits(self, h: torch.Tensor) -> torch.Tensor:
        return self._gemm("logits", h, self.enc.embed, self.enc.embed_row_scale).to(torch.float32)

    def prefill(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, capacity: int, return_states: bool = False,
                logits: bool = True):
        """(cache, logits (B,V) fp32 of the last position) for a left-padded (B,T) prompt, T <= capacity (a multiple of 64);
        with ``return_states`` also the encoder's (L+1, B, T, D) states.  ``logits=False``: (cache, states) and no logits GEMM
        (the device loop writes the logits into its own buffer)."""
        B, T = input_ids.shape
        if T > capacity:
            raise ValueError(f"prefill: {T} prompt positions do not fit a cache of capacity {capacity}")
        cache = GemmaCache(self.cfg, B, capacity, self.enc.device)
        states = self.enc._forward(input_ids, attention_mask, cache)
        if not logits:
            return cache, states
        logits = self._logits(states[-1][:, T - 1])
        return (cache, logits, states) if return_states else (cache, logits)

    def step(self, cache: GemmaCache, token_ids, return_states: bool = False):
        """logits (B,V) fp32 after feeding one token per batch row at position ``cache.length``; the cache grows by one.  With
        ``return_states`` also the token's (L+1, B, D) hidden states, the encoder's list at that position."""
        e, c, dev = self.enc, self.cfg, self.enc.device
        pos, cap, B = cache.length, cache.capacity, cache.B
        if cache.row_start is None:
            raise ValueError("step: the cache has not been prefilled")
        if pos >= cap:
            raise ValueError(f"step: the cache is full ({cap} positions)")
        ids_host = torch.as_tensor(token_ids).detach().to("cpu").reshape(-1).to(torch.int64)
        if ids_host.numel() != B:
            raise ValueError(f"step: {ids_host.numel()} token ids for a cache of {B} batch rows")
        D, F, L = c.hidden_size, c.intermediate_size, c.num_hidden_layers
        Hq, Hkv = c.num_attention_heads, c.num_key_value_heads
        nq, nkv = Hq * HEAD_DIM, Hkv * HEAD_DIM
        states = torch.empty((L + 1, B, D), dtype=BF16, device=dev)
        x = ops.embed_rows(e.embed, ids_host.to(torch.int32).to(dev), e.embed_scale, out=states[0], ids_host=ids_host,
                           row_scale=e.embed_row_scale)
        nx = torch.empty((B, D), dtype=BF16, device=dev)
        qkv = torch.empty((B, nq + 2 * nkv), dtype=BF16, device=dev)
        att = torch.empty((B, nq), dtype=BF16, device=dev)
        po = torch.empty((B, D), dtype=BF16, device=dev)
        gu = torch.empty((B, 2 * F), dtype=BF16, device=dev)
        for i, ly in enumerate(e.layers):
            cos, sin = e._tables(cap, ly["is_global"])
            ops.rmsnorm_weight_rows(x, ly["n_in"], c.rms_norm_eps, out=nx)
            self._gemm("qkv", nx, ly["qkv"], ly["qkv_s"], qkv, self._p4(i, "qkv"))
            ops.headnorm_rope(qkv, Hq, Hkv, ly["qn"], ly["kn"], cos[pos:pos + 1], sin[pos:pos + 1], 1, c.rms_norm_eps)
            ops.causal_attn(qkv[:, :nq], cache.k[i].view(B * cap, nkv), cache.vt[i], att, cache.row_start, B, Hq, Hkv, cap, e.scale,
                            window=ly["window"], step=pos, k_new=qkv[:, nq:nq + nkv], v_new=qkv[:, nq + nkv:], partials=cache.partials)
            self._gemm("o", att, ly["o"], ly["o_s"], po, self._p4(i, "o"))
            y = states[i + 1] if i + 1 < L else nx.new_empty((B, D))
            ops.rmsnorm_weight_rows(po, ly["n_post_attn"], c.rms_norm_eps, resid=x, out=y)
            ops.rmsnorm_weight_rows(y, ly["n_pre_ff"], c.rms_norm_eps, out=nx)
            self._gemm("gu", nx, ly["gu"], ly["gu_s"], gu, self._p4(i, "gu"))
            h = ops.geglu_tanh_(gu)
            self._gemm("down", h, ly["down"], ly["down_s"], po, self._p4(i, "down"))
            ops.rmsnorm_weight_rows(po, ly["n_post_ff"], c.rms_norm_eps, resid=y, out=y)
            x = y
        ops.rmsnorm_weight_rows(x, e.norm, c.rms_norm_eps, out=states[L])
        cache.length = pos + 1
        logits = self._gemm("logits", states[L], e.embed, e.embed_row_scale, None, self._p4(None, "logits")).to(torch.float32)
        return (logits, states) if return_states else logits

    def sample(self, state: GemmaDecodeState, temperature: float, repetition_penalty: float, repetition_context: int,
               draw: bool = True, advance: bool = False) -> None:
        """The sampler on ``state``: a draw from ``state.logits`` (``ops.sample_rows``), the advance of ctl, or both."""
        ops.sample_rows(state.logits, state.ctl, state.done, state.next_ids, state.history, state.hist_len, state.tokens_out, state.eos,
                        state.uniforms if temperature > 0 else None, state.workspace, temperature=float(temperature),
                        penalty=float(repetition_penalty), rep_ctx=max(0, int(repetition_context)), draw=draw, advance=advance)

    def device_step(self, cache: GemmaCache, state: GemmaDecodeState, temperature: float = 0.0, repetition_penalty: float = 1.0,
                    repetition_context: int = 0, draw: bool = True) -> None:
        """One token entirely in stream order, with no host value that changes from token to token: the draw from
        ``state.logits``, ``embed_rows`` of ``state.next_ids``, the L layers of ``step`` - the same launches, the token's position
        read from ``state.ctl`` by ``headnorm_rope(pos=)`` and ``causal_attn(step=<tensor>, max_step=)`` - the final norm, the logits
        GEMM into ``state.logits`` and the advance of ctl.  Nothing is allocated and nothing synchronises, so the call can be
        recorded once (``torch.cuda.graph``) and replayed; fed the same ids it leaves the logits ``step`` returns, bit for bit.
        ``draw=False`` feeds ``state.next_ids`` as they stand (teacher forcing).  The host's ``cache.length`` is not touched: the
        position lives in ``state.ctl``."""
        e, c = self.enc, self.cfg
        cap, B = cache.capacity, cache.B
        if cache.row_start is None:
            raise ValueError("device_step: the cache has not been prefilled")
        if state.B != B or state.T + state.max_tokens > cap:
            raise ValueError(f"device_step: a state of {state.B} rows, {state.T} + {state.max_tokens} positions on a cache of {B} rows, capacity {cap}")
        L = c.num_hidden_layers
        Hq, Hkv = c.num_attention_heads, c.num_key_value_heads
        nq, nkv = Hq * HEAD_DIM, Hkv * HEAD_DIM
        if draw:
            self.sample(state, temperature, repetition_penalty, repetition_context)
        x = ops.embed_rows(e.embed, state.next_ids, e.embed_scale, out=state.x[0], row_scale=e.embed_row_scale, trusted_ids=True)
        nx, qkv, att, po, gu, pos = state.nx, state.qkv, state.att, state.po, state.gu, state.pos
        for i, ly in enumerate(e.layers):
            cos, sin = e._tables(cap, ly["is_global"])
            ops.rmsnorm_weight_rows(x, ly["n_in"], c.rms_norm_eps, out=nx)
            self._gemm("qkv", nx, ly["qkv"], ly["qkv_s"], qkv, self._p4(i, "qkv"))
            ops.headnorm_rope(qkv, Hq, Hkv, ly["qn"], ly["kn"], cos, sin, cap, c.rms_norm_eps, pos=pos)
            ops.causal_attn(qkv[:, :nq], cache.k[i].view(B * cap, nkv), cache.vt[i], att, cache.row_start, B, Hq, Hkv, cap, e.scale,
                            window=ly["window"], step=pos, max_step=cap - 1, k_new=qkv[:, nq:nq + nkv], v_new=qkv[:, nq + nkv:],
                            partials=cache.partials)
            self._gemm("o", att, ly["o"], ly["o_s"], po, self._p4(i, "o"))
            y = state.x[(i + 1) % 2]
            ops.rmsnorm_weight_rows(po, ly["n_post_attn"], c.rms_norm_eps, resid=x, out=y)
            ops.rmsnorm_weight_rows(y, ly["n_pre_ff"], c.rms_norm_eps, out=nx)
            self._gemm("gu", nx, ly["gu"], ly["gu_s"], gu, self._p4(i, "gu"))
            h = ops.geglu_tanh_(gu)
            self._gemm("down", h, ly["down"], ly["down_s"], po, self._p4(i, "down"))
            ops.rmsnorm_weight_rows(po, ly["n_post_ff"], c.rms_norm_eps, resid=y, out=y)
            x = y
        ops.rmsnorm_weight_rows(x, e.norm, c.rms_norm_eps, out=nx)
        self._gemm("logits", nx, e.embed, e.embed_row_scale, state.logits, self._p4(None, "logits"))
        self.sample(state, temperature, repetition_penalty, repetition_context, draw=False, advance=True)

    def _generate_device(self, input_ids, attention_mask, max_tokens, temperature, repetition_penalty, repetition_context, eos_ids, seed,
                         graph: bool, sync_every: int) -> List[List[int]]:
        """``generate(device_loop=True)``."""
        B, T = input_ids.shape
        if temperature < 0:
            raise ValueError(f"temperature must be >= 0, got {temperature}")
        if repetition_context > ops.SAMPLE_MAX_CTX:
            raise ValueError(f"generate: the device loop penalises at most the last {ops.SAMPLE_MAX_CTX} tokens, got "
                             f"repetition_context = {repetition_context}")
        if sync_every < 1:
            raise ValueError(f"generate: sync_every = {sync_every} must be positive")
        state = GemmaDecodeState(self.cfg, self.enc.vocab, input_ids, attention_mask, max_tokens, eos_ids, seed, self.enc.device)
        cache, states = self.prefill(input_ids, attention_mask, (T + max_tokens + 63) // 64 * 64, logits=False)
        self._gemm("logits", states[-1][:, T - 1], self.enc.embed, self.enc.embed_row_scale, state.logits)
        del states
        step = lambda: self.device_step(cache, state, temperature, repetition_penalty, repetition_context)      # noqa: E731
        n = live = 0
        if max_tokens == 1:             # one draw and nothing to feed
            self.sample(state, temperature, repetition_penalty, repetition_context, advance=True)
        else:
            # token 0 eagerly (it also makes the lazy one-time calls: the split-K scratch, a kernel's LDS attribute), then the
            # step recorded once - one chain on one stream - and replayed.  A replay draws token n and feeds it; the feed behind
            # the last draw is wasted.  The host looks at ctl every sync_every steps, so up to that many run past the last EOS.
            step()
            g = None
            if graph:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    step()
            for i in range(1, max_tokens):
                if i % sync_every == 0:
                    n, _, live, _ = state.read()
                    if live == 0:
                        break
                g.replay() if g is not None else step()
        n, pos, live, toks = state.read()
        cache.length = pos
        return [[int(t) for t in toks[b, :n] if int(t) >= 0] for b in range(B)]

    def generate(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, max_tokens: int = 512, temperature: float = 0.7,
                 repetition_penalty: float = 1.3, repetition_context: int = 20, eos_ids: Sequence[int] = (1, 107),
                 seed: int = 42, device_loop: bool = False, graph: bool = True, sync_every: int = 16) -> List[List[int]]:
        """The new tokens of each batch row, its terminating EOS id included (generation of a row ends there, or at
        ``max_tokens``).  The defaults are the reference's call (text_encoder.py:1079-1084, 1123): temperature 0.7, repetition
        penalty 1.3 over the last 20 tokens (the prompt's included), EOS ids 1 and 107.  Sampling is host torch on the fp32
        logits with a ``torch.Generator`` seeded by ``seed``: seeds are NOT cross-compatible with MLX's generator - the same
        seed gives the same tokens here and other tokens there (the project's standing convention for random numbers).

        ``device_loop=True``: the loop stays on the device (``device_step``).  The penalty, the draw and the bookkeeping are
        ``ops.sample_rows`` on the logits GEMM's own bf16 output, the token's position is read from device memory, and with
        ``graph`` the step is recorded once as a graph and replayed (``graph=False``: the same launches, eagerly); every
        ``sync_every`` steps one small copy tells the host whether every row has finished.  At temperature 0 the tokens are the
        host loop's.  At temperature > 0 the device loop consumes ``seed`` differently - one ``torch.rand`` uniform per (draw,
        row) through the inverse CDF, where the host loop calls ``torch.multinomial`` - so the same seed gives OTHER tokens than
        with ``device_loop=False``, as it does against MLX; two device-loop runs of one seed agree.  B <= 8,
        ``repetition_context`` <= 64 and at most 8 EOS ids."""
        B, T = input_ids.shape
        if max_tokens < 1:
            return [[] for _ in range(B)]
        if device_loop:
            return self._generate_device(input_ids, attention_mask, max_tokens, temperature, repetition_penalty, repetition_context,
                                         eos_ids, seed, graph, sync_every)
        cache, logits = self.prefill(input_ids, attention_mask, (T + max_tokens + 63) // 64 * 64)
        ids_host, mask_host = input_ids.detach().to("cpu"), attention_mask.detach().to("cpu").bool()
        history = [[int(t) for t in ids_host[b][mask_host[b]]] for b in range(B)]
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        eos = set(int(t) for t in eos_ids)
        out: List[List[int]] = [[] for _ in range(B)]
        done = [False] * B
        for n in range(max_tokens):
            ctx = [h[-repetition_context:] if repetition_context > 0 else [] for h in history]
            tok = sample_tokens(logits, ctx, temperature, repetition_penalty, gen)
            for b in range(B):
                if not done[b]:
                    t = int(tok[b])
                    out[b].append(t)
                    history[b].append(t)
                    done[b] = t in eos
            if all(done) or n + 1 == max_tokens:
                break
            logits = self.step(cache, tok)          # (a finished row keeps feeding its last token; its output is not kept)
        return out


# ------------------------------------------------------------------------------------------------------ prompt enhancement
DEFAULT_ENHANCE_SYSTEM_PROMPT = (
    "You rewrite short video ideas into one detailed prompt for a text-to-video model. Keep the user's subject and intent. "
    "Describe, in a single flowing paragraph of present-tense sentences and in chronological order: the main subject and its "
    "appearance, the action and how it unfolds, the setting and background, the lighting and colours, and the camera's framing "
    "and movement. Be concrete and visual; do not invent dialogue, titles or on-screen text; do not address the user, add "
    "commentary or use lists. Answer with the rewritten prompt only, in at most 200 words.")


def chat_prompt(system_prompt: str, prompt: str) -> str:
    """The reference's message layout (text_encoder.py:998-1021, 1055-1058) in Gemma-3's turn format: the system text sent as a
    user turn, a user turn ``user prompt: {prompt}``, then the model turn's opener."""
    return (f"<start_of_turn>user\n{system_prompt}<end_of_turn>\n"
            f"<start_of_turn>user\nuser prompt: {prompt}<end_of_turn>\n"
            "<start_of_turn>model\n")


def clean_response(text: str) -> str:
    """Whitespace stripped, then any leading punctuation removed (text_encoder.py:990-996)."""
    return re.sub(r"^[^\w\s]+", "", text.strip())


def enhance_prompt(generator: GemmaGenerator, tokenizer, prompt: str, system_prompt: Optional[str] = None, max_tokens: int = 512,
                   temperature: float = 0.7, seed: int = 42, device_loop: bool = False, mxfp4: bool = False, **sampling) -> str:
    """The user's short prompt rewritten by the model into the long descriptive one LTX-2 was trained on (the reference's
    ``enhance_t2v``, text_encoder.py:1023-1135).  ``tokenizer``: a ``tokenizers.Tokenizer`` (``load_tokenizer``).  Only the new
    tokens are decoded (special tokens skipped) and cleaned; an empty result keeps ``prompt`` and warns.  ``sampling``: further
    keywords of ``GemmaGenerator.generate`` (repetition_penalty, repetition_context, eos_ids, graph, sync_every).
    ``device_loop``: sampling and the token loop on the device, the step replayed as a graph (``generate``); at temperature > 0
    the same ``seed`` then gives other tokens than the host loop does.  ``mxfp4``: decode on 4-bit panels (opt-in; the text encoding is not
    affected) - a ``generator`` built without ``decode_panels="mxfp4"`` is replaced by one with them on the same encoder."""
    if mxfp4 and generator.decode_panels != "mxfp4":
        generator = GemmaGenerator(generator.enc, gemv=generator.gemv, decode_panels="mxfp4")
    text = chat_prompt(system_prompt or DEFAULT_ENHANCE_SYSTEM_PROMPT, prompt)
    tokenizer.no_padding(); tokenizer.no_truncation()
    ids = list(tokenizer.encode(text).ids)
    if not ids:
        raise ValueError("enhance_prompt: the tokenizer produced no tokens for the chat prompt")
    input_ids = torch.tensor([ids], dtype=torch.int64)
    new = generator.generate(input_ids, torch.ones_like(input_ids), max_tokens=max_tokens, temperature=temperature, seed=seed,
                             **({"device_loop": True} if device_loop else {}), **sampling)[0]
    out = clean_response(tokenizer.decode(new, skip_special_tokens=True))
    if not out:
        warnings.warn("prompt enhancement produced an empty result: the original prompt is kept")
        return prompt
    return out


def random_gemma_weights(device, config: GemmaConfig, seed: int = 23, generator_device=None) -> Dict[str, torch.Tensor]:
    """Seeded stand-in weights under the language model's keys (tests and measurement; no checkpoint is read)."""
    gd = generator_device or "cpu"
    g = torch.Generator(device=gd).manual_seed(seed)
    c = config

    def rn(*shape, std=1.0):
        return (torch.randn(shape, generator=g, device=gd) * std).to(BF16).to(device)

    D, F, nq, nkv = c.hidden_size, c.intermediate_size, c.num_attention_heads * HEAD_DIM, c.num_key_value_heads * HEAD_DIM
    W = {"embed_tokens.weight": rn(c.vocab_size, D, std=1.0 / math.sqrt(D)), "norm.weight": rn(D, std=0.1)}
    for i in range(c.num_hidden_layers):
        p = f"layers.{i}."
        W[p + "self_attn.q_proj.weight"] = rn(nq, D, std=1.0 / math.sqrt(D))
        W[p + "self_attn.k_proj.weight"] = rn(nkv, D, std=1.0 / math.sqrt(D))
        W[p + "self_attn.v_proj.weight"] = rn(nkv, D, std=1.0 / math.sqrt(D))
        W[p + "self_attn.o_proj.weight"] = rn(D, nq, std=1.0 / math.sqrt(nq))
        W[p + "self_attn.q_norm.weight"], W[p + "self_attn.k_norm.weight"] = rn(HEAD_DIM, std=0.1), rn(HEAD_DIM, std=0.1)
        W[p + "mlp.gate_proj.weight"], W[p + "mlp.up_proj.weight"] = rn(F, D, std=1.0 / math.sqrt(D)), rn(F, D, std=1.0 / math.sqrt(D))
        W[p + "mlp.down_proj.weight"] = rn(D, F, std=1.0 / math.sqrt(F))
        for n in ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm"):
            W[p + n + ".weight"] = rn(D, std=0.1)
    return W


# ------------------------------------------------------------------------------------------------------------ tokenizer
def load_tokenizer(path: Union[str, Path]):
    """The ``tokenizers.Tokenizer`` of a local directory holding ``tokenizer.json`` (or of that file).  Nothing is fetched and
    repo names are not resolved."""
    p = Path(path)
    f = p / "tokenizer.json" if p.is_dir() else p
    if not f.is_file():
        raise FileNotFoundError(f"no tokenizer.json at {p}: pass tokenizer_path= a local directory that holds one, or tokenise "
                                "elsewhere and pass prompt_tokens=(input_ids, attention_mask)")
    try:
        from tokenizers import Tokenizer
    except ImportError as e:
        raise RuntimeError("the `tokenizers` package is not installed: tokenise elsewhere and pass prompt_tokens=(input_ids, "
                           "attention_mask), or --prompt-tokens FILE") from e
    return Tokenizer.from_file(str(f))


def _pad_id(tok) -> int:
    for name in ("<pad>", "[PAD]", "<|pad|>"):
        i = tok.token_to_id(name)
        if i is not None:
            return int(i)
    return 0                # Gemma's <pad> is id 0


def tokenize(tok, prompts: Sequence[str], max_length: int = MAX_TOKENS, pad_id: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(input_ids, attention_mask), each (len(prompts), max_length) int64: every prompt encoded with the tokenizer's own special
    tokens, truncated to ``max_length`` and LEFT-padded with the pad id, mask 0 on the padding (text_encoder.py:929-935)."""
    pad = _pad_id(tok) if pad_id is None else int(pad_id)
    tok.no_padding(); tok.no_truncation()           # a tokenizer.json may carry its own (right-)padding settings
    ids = torch.full((len(prompts), max_length), pad, dtype=torch.int64)
    mask = torch.zeros((len(prompts), max_length), dtype=torch.int64)
    for b, text in enumerate(prompts):
        e = list(tok.encode(text).ids)[:max_length]
        if e:
            ids[b, max_length - len(e):] = torch.tensor(e, dtype=torch.int64)
            mask[b, max_length - len(e):] = 1
    return ids, mask
