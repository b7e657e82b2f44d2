"""The reference's text path behind Gemma, restated in torch on the CPU from its behaviour (mlx_video/models/ltx/
text_encoder.py:280-639: norm_and_concat_hidden_states, GemmaFeaturesExtractor, Embeddings1DConnector), under two policies:

* ``F64``  - float64 throughout, un-rounded RoPE tables, the exact token count in the mean.  This is the truth.
* ``BF16`` - the reference's own arithmetic: every MLX op on bf16 arrays returns a bf16 array, so each op rounds once
  (fused ops - Linear with bias, mx.fast.rms_norm, mx.fast.scaled_dot_product_attention, the fp32 RoPE - round once at
  their output).  It includes the two accidents of dtype promotion in norm_and_concat_hidden_states: the mean's
  denominator is bf16(count*D) + bf16(1e-6), and the RoPE tables are handed over in bf16.

Values are carried as float64 tensors; a policy is its rounding function ``r`` applied where the reference materialises an
array.  Weights use module keys (``transformer_1d_blocks.{i}.attn1.to_q.weight`` ...), ``aggregate_embed.weight`` in the
CHECKPOINT's K order d*L + l, ``learnable_registers`` (R,D)."""
import math

import numpy as np
import torch

F64 = torch.float64
BF = torch.bfloat16


class Policy:
    def __init__(self, name, bf16):
        self.name, self.bf16 = name, bf16

    def r(self, x):
        return x.to(BF).to(F64) if self.bf16 else x


P64 = Policy("float64", False)
PBF = Policy("bf16", True)


def rope_table(T, H, p, theta=10000.0, max_pos=4096):
    """cos, sin (H,T,64) float64: positions 2t/max_pos - 1 times theta^linspace(0,1,64H) * pi/2, head h owning frequencies
    [64h, 64h + 64).  The bf16 policy rounds the fp32 tables to bf16."""
    n = H * 64
    freqs = np.power(float(theta), np.linspace(0.0, 1.0, n, dtype=np.float64)) * (np.pi / 2)
    pos = np.arange(T, dtype=np.float64) / max_pos * 2 - 1
    ang = torch.from_numpy(pos[:, None] * freqs[None, :]).reshape(T, H, 64).permute(1, 0, 2)
    cos, sin = torch.cos(ang), torch.sin(ang)
    if p.bf16:
        cos, sin = cos.float().to(BF).to(F64), sin.float().to(BF).to(F64)
    return cos.contiguous(), sin.contiguous()


def norm_and_concat(hs, mask, p):
    """hs (L,B,T,D), mask (B,T) 0/1 left-padded -> (B,T,D*L): per (batch row, layer) 8 * (x - mean) / (max - min + 1e-6) over
    the valid tokens x D, layers interleaved on the last axis (feature d*L + l), padded positions zero."""
    L, B, T, D = hs.shape
    x = hs.to(F64).permute(1, 2, 3, 0)                                  # (B,T,D,L): the stack on the last axis
    counts = mask.to(torch.int64).sum(dim=1)
    valid = (torch.arange(T)[None, :] >= (T - counts)[:, None])[:, :, None, None]
    if p.bf16:
        eps = p.r(torch.tensor(1e-6, dtype=F64))
        denom = p.r(p.r((counts * D).to(F64)) + eps)                     # bf16(count*D) + bf16(1e-6): the promotion accident
    else:
        eps = torch.tensor(1e-6, dtype=F64)
        denom = (counts * D).to(F64) + eps
    total = p.r(torch.where(valid, x, torch.zeros_like(x)).sum(dim=(1, 2), keepdim=True))
    mean = p.r(total / denom.reshape(B, 1, 1, 1))
    x_min = torch.where(valid, x, torch.full_like(x, float("inf"))).amin(dim=(1, 2), keepdim=True)
    x_max = torch.where(valid, x, torch.full_like(x, float("-inf"))).amax(dim=(1, 2), keepdim=True)
    rng = p.r(x_max - x_min)
    normed = p.r(p.r(8 * p.r(x - mean)) / p.r(rng + eps))
    normed = normed.reshape(B, T, D * L)
    return torch.where(valid[:, :, :, 0].expand(B, T, D * L), normed, torch.zeros_like(normed))


def linear(x, w, b, p):
    y = x @ w.to(F64).T
    return p.r(y if b is None else y + b.to(F64))


def rms_norm(x, p, weight=None, eps=1e-6):
    y = x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps)
    return p.r(y if weight is None else y * weight.to(F64))


def split_rope(x, cos, sin, p):
    """x (B,H,T,128): first half against second half."""
    x1, x2 = x[..., :64], x[..., 64:]
    return p.r(torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1))


def gelu_erf(x, p):
    """x * (1 + erf(x / sqrt 2)) / 2, one rounding per op under the bf16 policy."""
    if not p.bf16:
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    t = p.r(x / p.r(torch.tensor(math.sqrt(2.0), dtype=F64)))
    return p.r(p.r(x * p.r(1 + p.r(torch.erf(t)))) / 2)


def replace_padded_with_registers(feat, counts, registers):
    """Valid tokens (the last count positions) to the front, registers[t % R] behind them."""
    B, T, D = feat.shape
    R = registers.shape[0]
    tiled = registers.to(F64).repeat(T // R, 1)
    out = []
    for b in range(B):
        c = int(counts[b])
        out.append(torch.cat([feat[b, T - c:], tiled[c:]], dim=0))
    return torch.stack(out, 0)


def connector(x, W, p, H):
    """Embeddings1DConnector after the register replacement: x (B,T,D)."""
    B, T, D = x.shape
    cos, sin = rope_table(T, H, p)
    n = 1 + max(int(k.split(".")[1]) for k in W if k.startswith("transformer_1d_blocks."))
    heads = lambda t: t.reshape(B, T, H, 128).permute(0, 2, 1, 3)
    for i in range(n):
        g = lambda name: W[f"transformer_1d_blocks.{i}.{name}"]
        nx = rms_norm(x, p)
        q = rms_norm(linear(nx, g("attn1.to_q.weight"), g("attn1.to_q.bias"), p), p, g("attn1.q_norm.weight"))
        k = rms_norm(linear(nx, g("attn1.to_k.weight"), g("attn1.to_k.bias"), p), p, g("attn1.k_norm.weight"))
        v = linear(nx, g("attn1.to_v.weight"), g("attn1.to_v.bias"), p)
        q, k, v = split_rope(heads(q), cos, sin, p), split_rope(heads(k), cos, sin, p), heads(v)
        att = p.r(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(128.0), dim=-1) @ v)
        att = att.permute(0, 2, 1, 3).reshape(B, T, D)
        x = p.r(x + linear(att, g("attn1.to_out.weight"), g("attn1.to_out.bias"), p))
        h = gelu_erf(linear(rms_norm(x, p), g("ff.proj_in.weight"), g("ff.proj_in.bias"), p), p)
        x = p.r(x + linear(h, g("ff.proj_out.weight"), g("ff.proj_out.bias"), p))
    return rms_norm(x, p)


def text_stage(hs, mask, W, p):
    """hidden states (L,B,T,D) + mask (B,T) -> the DiT context (B,T,D)."""
    D = W["learnable_registers"].shape[1]
    feat = linear(norm_and_concat(hs, mask, p), W["aggregate_embed.weight"], None, p)
    x = replace_padded_with_registers(feat, mask.to(torch.int64).sum(dim=1), p.r(W["learnable_registers"].to(F64)))
    return connector(x, W, p, D // 128)
