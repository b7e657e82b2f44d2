"""Restatements for KV-cached Gemma-3 decoding (mlx_video_amd/gemma.py GemmaGenerator, csrc/causal_attn_step.hip), built on
tests/ref_gemma.py's pieces.

* ``prefill`` / ``step``: the model with an EXPLICIT cache - per layer the rotated K rows and the V rows of every position fed
  so far - under ref_gemma's two policies ("f64" rounds nothing, "bf16" rounds at the rounding points of include/ltxk.h).
  A step computes one position from the cache; tests/test_gemma_decode_cpu.py holds it to ``ref_gemma.forward`` on the whole
  sequence and to transformers' Gemma3ForCausalLM with ``use_cache``.
* ``step_attention``: ltxk_causal_attn_step in float64 with the terms of ``ref_gemma.attention_bound``.
* ``step_inputs`` / ``attention_step_sliced_fp32``: the kernel test's operands and an fp32 emulation of the kernel's sliced
  evaluation (64-key tiles, 256-key slices, merged in ascending order, bf16 P, k_new / v_new standing in for key ``step``) with
  switches that plant one fault each.
"""
import numpy as np
import torch

import ref_gemma as R
from ref_gemma import BF, DH, F64, f64, rbf


# ------------------------------------------------------------------------------------------------------------ attention step
def step_attention(q1, k, v, Hq, Hkv, row_start, step, window, scale, **kw):
    """One query per batch row at position ``step`` against keys 0 .. step: q1 (B,Hq*256), k, v (B, >= step+1, Hkv*256) whose
    row ``step`` is the new token's.  ``ref_gemma.causal_attention``'s (y, A, dx, nvis) for that row, each (B,Hq*256)."""
    B = q1.shape[0]
    T = step + 1
    q = torch.zeros(B, T, Hq * DH, dtype=q1.dtype)
    q[:, step] = q1
    y, A, dx, nvis = R.causal_attention(q, k[:, :T], v[:, :T], Hq, Hkv, row_start, window, scale, **kw)
    return y[:, step], (None if A is None else A[:, step]), dx[:, step], nvis[:, step]


def step_inputs(B, Hq, Hkv, step, row_start, cap, seed):
    """The operands of one attention step from ``ref_gemma.attention_inputs`` at T = step + 1: q1 (B,Hq*256), k, v
    (B,step+1,Hkv*256) (row ``step`` = k_new, v_new), and the cache k_cache (B,cap,Hkv*256), vt_cache (B,Hkv*256,cap) holding rows
    < step, +-1024 past ``step``, and at position ``step`` itself a STALE finite value (the kernel test overwrites it with NaN).
    K and V rows below row_start hold +-1024 and the K row at row_start - 1 is 1024 * sign(q1) of the group's first query head:
    admitted by mistake, it takes the whole of the row."""
    T = step + 1
    q, k, v, vt = R.attention_inputs(B, Hq, Hkv, T, row_start, seed, ldvt=cap, planted=False)
    q1 = q[:, step].clone()
    for b, rs in enumerate(row_start):
        if 0 < int(rs) <= step:
            qs = q1[b].float().reshape(Hq, DH)[::Hq // Hkv].reshape(-1)
            k[b, rs - 1] = (1024.0 * torch.where(qs >= 0, 1.0, -1.0)).to(BF)
    g = torch.Generator().manual_seed(seed * 7919 + step)
    k_cache = torch.empty(B, cap, Hkv * DH, dtype=BF)
    k_cache[:, :T] = k
    alt = (1024.0 * (1 - 2 * (torch.arange(Hkv * DH) % 2))).to(BF)
    if cap > T:
        k_cache[:, T:] = alt[None, None, :] * (1 - 2 * (torch.arange(cap - T) % 2)).to(BF)[None, :, None]
    vt_cache = vt.clone()                                        # columns >= T alternate +-1024 already
    k_cache[:, step] = (3.0 * torch.randn(B, Hkv * DH, generator=g)).to(BF)
    vt_cache[:, :, step] = (3.0 * torch.randn(B, Hkv * DH, generator=g)).to(BF)
    return q1, k, v, k_cache, vt_cache


STEP_FAULTS = ("drop_key", "admit_below", "window_minus", "window_plus", "head_mod", "stale")


def fault_alters(fault, Hq, Hkv, step, row_start, window):
    """Whether the planted fault changes what some batch row of the case computes."""
    rows = [int(r) for r in row_start if int(r) <= step]
    if not rows:
        return False
    return {"drop_key": True, "stale": True, "admit_below": any(r > 0 for r in rows),
            "window_minus": bool(window) and any(step - window + 1 >= r for r in rows),
            "window_plus": bool(window) and any(step - window >= r for r in rows),
            "head_mod": Hkv > 1 and Hq // Hkv > 1}[fault]


def attention_step_sliced_fp32(q1, k_new, v_new, k_cache, vt_cache, Hq, Hkv, step, row_start, window, scale, fault=None,
                               BK: int = 64, SLICE: int = 256):
    """An fp32 emulation of the kernel's evaluation: per 64-key tile S in fp32, M = ceil(max over the visible keys of S * c),
    P = exp2(fl32(S * c - M)), l = sum P, O = bf16(P) @ V; the tiles of a 256-key slice, then the slices, merged in ascending
    order with the exact factors 2^(M_i - M); out = bf16(O * (1/l)).  Key ``step`` comes from k_new / v_new.  ``fault``:
      drop_key      key ``step`` is skipped
      admit_below   key row_start - 1 is admitted (rows with row_start > 0)
      window_minus / window_plus   the window is one key short / long
      head_mod      query head h reads K/V head h % Hkv
      stale         key ``step`` is read from the cache, not from k_new / v_new."""
    assert fault is None or fault in STEP_FAULTS
    f32 = torch.float32
    B = q1.shape[0]
    c = np.float32(R.attn_c(scale))
    w = window + (fault == "window_plus") - (fault == "window_minus") if window else 0
    kc, vc = k_cache.to(f32).clone(), vt_cache.to(f32).clone()
    if fault != "stale":
        kc[:, step], vc[:, :, step] = k_new.to(f32), v_new.to(f32)
    hm = (lambda h: h % Hkv) if fault == "head_mod" else (lambda h: h // (Hq // Hkv))
    out = torch.zeros(B, Hq, DH, dtype=f32)
    NONE = -1e30

    def merge(parts):
        m = max(p[0] for p in parts)
        if m < -1e29:
            return NONE, f32_zero, torch.zeros(DH, dtype=f32)
        l, o = f32_zero.clone(), torch.zeros(DH, dtype=f32)
        for pm, pl, po in parts:
            a = torch.tensor(2.0 ** (pm - m) if pm > -1e29 else 0.0, dtype=f32)
            l = l + pl * a
            o = o + po * a
        return m, l, o

    f32_zero = torch.zeros((), dtype=f32)
    for b in range(B):
        rs = max(int(row_start[b]), 0)
        j = torch.arange(step // BK * BK + BK)
        vis = (j >= rs) & (j <= step)
        if w:
            vis &= (step - j < w)
        if fault == "drop_key":
            vis[step] = False
        if fault == "admit_below" and 0 < rs <= step:
            vis[rs - 1] = True
        for h in range(Hq):
            qv = q1[b].to(f32).reshape(Hq, DH)[h]
            kh = kc[b, :, hm(h) * DH:(hm(h) + 1) * DH]
            vh = vc[b, hm(h) * DH:(hm(h) + 1) * DH]
            slices = []
            for s0 in range(0, step + 1, SLICE):
                tiles = []
                for t0 in range(s0, min(s0 + SLICE, step + 1), BK):
                    vs = vis[t0:t0 + BK]
                    if not bool(vs.any()):
                        tiles.append((NONE, f32_zero, torch.zeros(DH, dtype=f32)))
                        continue
                    s = kh[t0:t0 + BK] @ qv
                    m = float(torch.ceil(s[vs].max() * c))
                    p = torch.where(vs, torch.exp2((s.double() * float(c) - m).to(f32)), torch.zeros_like(s))
                    tiles.append((m, p.sum(), vh[:, t0:t0 + BK] @ p.to(BF).to(f32)))
                slices.append(merge(tiles))
            m, l, o = merge(slices)
            if m > -1e29 and float(l) > 0:
                out[b, h] = o * (torch.ones((), dtype=f32) / l)
    return out.reshape(B, Hq * DH).to(BF)


# ------------------------------------------------------------------------------------------------------------ whole model
class Cache:
    """Per layer the rotated K rows and the V rows (B,T,Hkv*256) float64 of the positions fed so far, and row_start."""

    def __init__(self, L, row_start):
        self.k, self.v, self.row_start = [None] * L, [None] * L, list(row_start)

    @property
    def length(self):
        return 0 if self.k[0] is None else self.k[0].shape[1]


def _run(W, cfg, ids, cache, policy, T_total, tables=None, embed_scale=None):
    """Feeds the (B,n) token ids at positions cache.length .. cache.length + n - 1: the L+1 states (B,n,D) and the logits
    (B,n,V) of those positions.  ref_gemma.forward's layer, with the keys and values of earlier positions taken from the cache."""
    r = rbf if policy == "bf16" else (lambda t: t)
    g = lambda k: f64(W[k])
    B, n = ids.shape
    p0 = cache.length
    Hq, Hkv, eps = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.rms_norm_eps
    scale = float(cfg.query_pre_attn_scalar) ** -0.5
    tables = tables or {True: R.rope_tables(T_total, cfg.rope_theta, cfg.rope_scaling_factor, round_bf16=policy == "bf16"),
              False: R.rope_tables(T_total, cfg.rope_local_base_freq, round_bf16=policy == "bf16")}
    s = float(torch.tensor(cfg.hidden_size ** 0.5, dtype=BF)) if embed_scale is None else float(embed_scale)
    x = r(g("embed_tokens.weight")[ids.to(torch.int64)] * s)
    states = [x]
    L = cfg.num_hidden_layers
    for i in range(L):
        p = f"layers.{i}."
        glob = cfg.is_global(i)
        cos, sin = (t[p0:p0 + n] for t in tables[glob])
        nx = r(R.rmsnorm(x, g(p + "input_layernorm.weight"), eps))
        q, k, v = (r(nx @ g(p + f"self_attn.{m}_proj.weight").T) for m in "qkv")
        q = R.headnorm_rope(q, Hq, g(p + "self_attn.q_norm.weight"), cos, sin, eps, r)
        k = R.headnorm_rope(k, Hkv, g(p + "self_attn.k_norm.weight"), cos, sin, eps, r)
        cache.k[i] = k if cache.k[i] is None else torch.cat([cache.k[i], k], 1)
        cache.v[i] = v if cache.v[i] is None else torch.cat([cache.v[i], v], 1)
        Tk = p0 + n
        qf = torch.zeros(B, Tk, Hq * DH, dtype=F64)
        qf[:, p0:] = q
        att = R.causal_attention(qf, cache.k[i], cache.v[i], Hq, Hkv, cache.row_start, 0 if glob else cfg.sliding_window, scale,
                                 bf16_p=policy == "bf16", exact_c=policy == "f64")[0][:, p0:]
        po = r(att @ g(p + "self_attn.o_proj.weight").T)
        y = r(x + r(R.rmsnorm(po, g(p + "post_attention_layernorm.weight"), eps)))
        nx = r(R.rmsnorm(y, g(p + "pre_feedforward_layernorm.weight"), eps))
        gate, up = r(nx @ g(p + "mlp.gate_proj.weight").T), r(nx @ g(p + "mlp.up_proj.weight").T)
        h = r(r(R.gelu_tanh(gate)) * up)
        po = r(h @ g(p + "mlp.down_proj.weight").T)
        x = r(y + r(R.rmsnorm(po, g(p + "post_feedforward_layernorm.weight"), eps)))
        if i + 1 < L:
            states.append(x)
    states.append(r(R.rmsnorm(x, g("norm.weight"), eps)))
    logits = r(states[-1] @ g("embed_tokens.weight").T)           # Gemma-3 ties the head to the embedding table
    return states, logits


def prefill(W, cfg, input_ids, attention_mask, policy="f64", T_total=None, **kw):
    """(cache, states [(B,T,D)] * (L+1), logits (B,T,V)) of a left-padded prompt; ``T_total``: the length the rope tables are
    built for (positions are padded-sequence indices, so any length >= the last position fed gives the same rows).  ``tables`` /
    ``embed_scale``: ref_gemma.forward's, tables of at least every position fed."""
    B, T = input_ids.shape
    rs = [T - int(n) for n in attention_mask.to(torch.int64).sum(1)]
    cache = Cache(cfg.num_hidden_layers, rs)
    states, logits = _run(W, cfg, input_ids, cache, policy, T_total or T, **kw)
    return cache, states, logits


def step(W, cfg, cache, token_ids, policy="f64", T_total=None, **kw):
    """(states [(B,D)] * (L+1), logits (B,V)) of one token per batch row at position cache.length; the cache grows by one."""
    ids = torch.as_tensor(token_ids).reshape(-1, 1)
    states, logits = _run(W, cfg, ids, cache, policy, T_total or cache.length + 1, **kw)
    return [s[:, 0] for s in states], logits[:, 0]


def penalised(logits, context, penalty):
    """The repetition penalty on (B,V) logits: the ids of context[b] have a negative logit multiplied by ``penalty``, any other
    divided by it (transformers' RepetitionPenaltyLogitsProcessor)."""
    out = logits.clone()
    for b, ctx in enumerate(context):
        idx = torch.tensor(sorted(set(ctx)), dtype=torch.int64)
        if len(idx):
            out[b, idx] = torch.where(out[b, idx] < 0, out[b, idx] * penalty, out[b, idx] / penalty)
    return out


def greedy(W, cfg, input_ids, attention_mask, n, policy="f64", penalty=1.0, context=20, **kw):
    """n greedy tokens per row: (tokens (B,n) int64, the logits (B,n,V) each was chosen from - after the repetition ``penalty``
    over the last ``context`` tokens of the row, the prompt's valid ones included -, the model's own logits (B,n,V))."""
    T = input_ids.shape[1]
    cache, _, lg = prefill(W, cfg, input_ids, attention_mask, policy, T_total=T + n, **kw)
    history = [[int(t) for t in input_ids[b][attention_mask[b].bool()]] for b in range(input_ids.shape[0])]
    logits, toks = lg[:, -1], []
    all_logits, raw = [], []
    for i in range(n):
        raw.append(logits)
        logits = penalised(logits, [h[-context:] for h in history], penalty) if penalty != 1.0 else logits
        all_logits.append(logits)
        tok = logits.argmax(-1)
        toks.append(tok)
        for b, h in enumerate(history):
            h.append(int(tok[b]))
        if i + 1 < n:
            _, logits = step(W, cfg, cache, tok, policy, T_total=T + n, **kw)
    return torch.stack(toks, 1), torch.stack(all_logits, 1), torch.stack(raw, 1)
