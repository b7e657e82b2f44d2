"""Float64 restatements for the Gemma-3 text encoder (mlx_video_amd/gemma.py, csrc/text_ops.hip, csrc/causal_attn.hip).

* ``forward``: the whole model in torch with a dtype policy - "f64" rounds nothing, "bf16" rounds to bf16 at the rounding
  points include/ltxk.h states and nowhere else (sums in float64 where the kernels sum in fp32).  The architecture is
  transformers' Gemma3TextModel (tests/test_gemma_cpu.py holds the f64 policy to it at 1e-9); the list of states is the
  reference's (text_encoder.py:110-148): [embeddings, h_1 .. h_{L-1}, norm(h_L)].
* ``causal_attention`` / ``attention_bound``: ltxk_causal_attn in float64 and the per-element bound of tests/ref64.py's
  ``attention`` / ``attention_bound`` restated for head dim 256 and the visible keys only.
* ``attention_tiled_fp32``: an fp32 emulation of a tiled online-softmax loop over 64-key tiles, with switches that plant one
  fault each (the CPU test shows that the bound rejects every one of them).
"""
import math

import numpy as np
import torch

F64 = torch.float64
BF = torch.bfloat16
DH = 256
U24 = 2.0 ** -24
LOG2E_F32 = 1.4426950408889634


def f64(x):
    return x.detach().to("cpu").to(F64)


def rbf(x):
    """Round float64 to bf16 once (through fp32: double rounding can differ from a direct rounding only for values within
    2^-29 relative of a bf16 midpoint, which the bounds' slack covers) and widen."""
    return x.to(torch.float32).to(BF).to(F64)


def ulp_bf16(m):
    m = m.abs().to(F64).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(m)) - 7)


def attn_c(scale: float) -> float:
    return float(np.float32(np.float32(scale) * np.float32(LOG2E_F32)))


def gelu_tanh(x):
    """x / (1 + exp(-2u)), u = sqrt(2/pi)(x + 0.044715 x^3) = x (1 + tanh u) / 2, float64."""
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)
    return x * torch.sigmoid(2.0 * u)


def rmsnorm(x, w, eps):
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * (1.0 + w)


def rope_tables(T: int, base: float, factor: float = 1.0, dim: int = DH, round_bf16: bool = False):
    """cos, sin (T, dim/2) float64: angle(t, i) = (t / factor) * base^(-2i/dim)."""
    inv = 1.0 / np.power(float(base), np.arange(0, dim, 2, dtype=np.float64) / dim) / float(factor)
    ang = torch.from_numpy(np.arange(T, dtype=np.float64)[:, None] * inv[None, :])
    c, s = torch.cos(ang), torch.sin(ang)
    return (rbf(c), rbf(s)) if round_bf16 else (c, s)


def headnorm_rope(x, H, w, cos, sin, eps, r):
    """x (B,T,H*256): per-head RMSNorm (1 + w), then rotate-half on the pairs (i, i+128); r = the rounding."""
    B, T, _ = x.shape
    xh = r(rmsnorm(x.reshape(B, T, H, DH), w, eps))
    x1, x2 = xh[..., :128], xh[..., 128:]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    return torch.cat([r(x1 * c - x2 * s), r(x2 * c + x1 * s)], -1).reshape(B, T, H * DH)


def visible(T: int, row_start, window: int):
    """(B,T,T) bool: key j visible to query i iff row_start[b] <= j <= i and (window == 0 or i - j < window)."""
    i = torch.arange(T)[None, :, None]
    j = torch.arange(T)[None, None, :]
    rs = torch.as_tensor(row_start).reshape(-1, 1, 1)
    v = (j >= rs) & (j <= i)
    if window:
        v = v & (i - j < window)
    return v


def _heads(t, H):
    B, T, _ = t.shape
    return t.to(F64).reshape(B, T, H, DH).transpose(1, 2)          # (B,H,T,256)


def _kv_heads(t, Hq, Hkv, head_map=None):
    th = _heads(t, Hkv)
    idx = torch.tensor([(h // (Hq // Hkv)) if head_map is None else head_map(h) for h in range(Hq)])
    return th[:, idx]


def causal_attention(q, k, v, Hq, Hkv, row_start, window, scale, bf16_p: bool = False, vis=None, head_map=None, exact_c: bool = False):
    """ltxk_causal_attn in float64: q (B,T,Hq*256), k, v (B,T,Hkv*256).  Returns (y, A, dx, nvis), each (B,T,Hq*256) float64:
    y = P v exact over the visible keys (zero for a row without one), A = P |v|, dx the most the exponent of one visible key can
    be off in a kernel that forms s in fp32 over 256 products and x - M with one fma,
        dx = max_vis(c * 256 * 2^-24 * |q|.|k|) + 2^-24 * (2 max_vis |x| + 8),
    and nvis the number of visible keys of the row.  ``bf16_p``: the "flash" policy's evaluation instead of the exact one -
    P = exp2(fl32(x - ceil(rowmax))), numerator over bf16(P), denominator over P, one rounding of the quotient.  ``exact_c``: the
    exponent constant scale * log2(e) in float64 instead of the kernel's fp32 product (the model's own softmax, for the
    comparison with transformers; the two differ by 2^-25 |x| in an exponent)."""
    B, T, _ = q.shape
    c = float(scale) * math.log2(math.e) if exact_c else attn_c(scale)
    qh, kh, vh = _heads(q, Hq), _kv_heads(k, Hq, Hkv, head_map), _kv_heads(v, Hq, Hkv, head_map)
    vis = (visible(T, row_start, window) if vis is None else vis)[:, None]           # (B,1,T,T)
    x = c * (qh @ kh.transpose(-1, -2))
    smag = qh.abs() @ kh.abs().transpose(-1, -2)
    any_vis = vis.any(-1, keepdim=True)
    xm = torch.where(vis, x, torch.full_like(x, -math.inf))
    mx = torch.where(any_vis, xm.amax(-1, keepdim=True), torch.zeros_like(x[..., :1]))
    if bf16_p:
        p = torch.where(vis, torch.exp2((x - torch.ceil(mx)).to(torch.float32).to(F64)), torch.zeros_like(x))
        l = p.sum(-1, keepdim=True)
        y = torch.where(any_vis, rbf((rbf(p) @ vh) / l.clamp_min(1e-300)), torch.zeros_like(qh))
        A = None
    else:
        p = torch.where(vis, torch.exp2(x - mx), torch.zeros_like(x))
        p = p / p.sum(-1, keepdim=True).clamp_min(1e-300)
        y, A = p @ vh, p @ vh.abs()
    zero = torch.zeros_like(x)
    dx = (c * DH * U24 * torch.where(vis, smag, zero)).amax(-1, keepdim=True) + \
        U24 * (2.0 * torch.where(vis, x.abs(), zero).amax(-1, keepdim=True) + 8.0)
    nvis = vis.sum(-1, keepdim=True).to(F64).expand(B, Hq, T, 1)
    back = lambda t: t.transpose(1, 2).reshape(B, T, Hq * DH)
    ex = lambda t: back(t.expand(B, Hq, T, DH))
    return back(y), (None if A is None else back(A)), ex(torch.where(any_vis, dx, torch.zeros_like(dx))), ex(nvis)


def attention_bound(out, y, A, dx, nvis):
    """(d, bound), element-wise: the distance of a kernel's bf16 output from ``causal_attention``'s y and the most a correct
    kernel with the rounding points of include/ltxk.h can be away, whatever its tiling and summation order - ref64.py's
    attention_bound with the row's count of VISIBLE keys in the place of Tk:
        e1    = 2^-22 + ln2 * dx * 1.001 + nvis * 2^-24
        e     = 2^-8 + e1
        bound = 1/2 ulp_bf16(out) + (e*A + e1*|y|) / (1 - e1) + 2^-22 |y| + 2^-120
    (the terms are derived there).  A row without a visible key has y = A = 0 and must be zero up to the 2^-120 floor and the
    half ulp of what was written.  NaN (a sentinel, 0/0) is infinitely far."""
    o = out.detach().to("cpu").to(F64)
    e1 = 2.0 ** -22 + math.log(2.0) * dx * 1.001 + nvis * U24
    e = 2.0 ** -8 + e1
    bound = 0.5 * ulp_bf16(torch.nan_to_num(o, nan=0.0)) + (e * A + e1 * y.abs()) / (1.0 - e1) + 2.0 ** -22 * y.abs() + 2.0 ** -120
    d = (o - y).abs()
    return torch.where(torch.isnan(d), torch.full_like(d, math.inf), d), bound


FAULTS = ("drop_key", "admit_below", "admit_above", "window_minus", "window_plus", "head_mod", "vt_pad")


def attention_tiled_fp32(q, k, vt, Hq, Hkv, T, row_start, window, scale, fault=None, BK: int = 64):
    """An fp32 emulation of a tiled online-softmax loop (64-key tiles, integer running offset, bf16 P into the P.V product,
    un-rounded P into l, one rounding of O / l): q (B,T,Hq*256), k (B,T,Hkv*256), vt (B,Hkv*256,ldvt) with whatever its pad
    columns hold.  ``fault`` plants one defect:
      drop_key      the last visible key of every row but the first valid one is skipped
      admit_below   key row_start - 1 is admitted (rows with row_start > 0)
      admit_above   key i + 1 is admitted for query i
      window_minus / window_plus   the window is one key short / long
      head_mod      query head h reads K/V head h % Hkv
      vt_pad        pad column T of V^T is admitted for every query, scored like key T - 1."""
    assert fault is None or fault in FAULTS
    f32 = torch.float32
    B = q.shape[0]
    c = np.float32(attn_c(scale))
    w = window + (fault == "window_plus") - (fault == "window_minus") if window else 0
    vis = visible(T, row_start, w)
    rs = [int(r) for r in row_start]
    for b in range(B):
        for i in range(T):
            if fault == "drop_key" and i > rs[b]:
                vis[b, i, i] = False
            if fault == "admit_below" and rs[b] > 0 and i >= rs[b]:
                vis[b, i, rs[b] - 1] = True
            if fault == "admit_above" and i + 1 < T and i >= rs[b]:
                vis[b, i, i + 1] = True
    hm = (lambda h: h % Hkv) if fault == "head_mod" else (lambda h: h // (Hq // Hkv))
    Tp = -(-T // BK) * BK
    ldvt = vt.shape[2]
    qh = q.to(f32).reshape(B, T, Hq, DH).transpose(1, 2)
    out = torch.zeros(B, Hq, T, DH, dtype=f32)
    for h in range(Hq):
        kh = k.to(f32).reshape(B, T, Hkv, DH)[:, :, hm(h)]                          # (B,T,256)
        vth = vt.to(f32)[:, hm(h) * DH:(hm(h) + 1) * DH]                            # (B,256,ldvt)
        kp = torch.cat([kh, kh[:, -1:].expand(B, Tp - T, DH)], 1) if Tp > T else kh
        vp = torch.zeros(B, DH, Tp, dtype=f32)
        vp[:, :, :min(Tp, ldvt)] = vth[:, :, :min(Tp, ldvt)]
        visp = torch.zeros(B, T, Tp, dtype=torch.bool)
        visp[:, :, :T] = vis
        if fault == "vt_pad" and Tp > T and ldvt > T:
            visp[:, :, T] = torch.tensor([[i >= rs[b] for i in range(T)] for b in range(B)])
        m = torch.full((B, T, 1), -1e30, dtype=f32)
        l = torch.zeros(B, T, 1, dtype=f32)
        o = torch.zeros(B, T, DH, dtype=f32)
        for t in range(Tp // BK):
            vs = visp[:, :, t * BK:(t + 1) * BK]
            if not bool(vs.any()):
                continue
            s = qh[:, h] @ kp[:, t * BK:(t + 1) * BK].transpose(1, 2)                    # fp32
            sm = torch.where(vs, s, torch.full_like(s, -1e30)).amax(-1, keepdim=True) * c
            m_new = torch.where(sm > -1e29, torch.maximum(m, torch.ceil(sm)), m)
            alpha = torch.exp2(m - m_new)
            p = torch.where(vs, torch.exp2((s.double() * float(c) - m_new.double()).to(f32)), torch.zeros_like(s))
            l = l * alpha + p.sum(-1, keepdim=True)
            o = o * alpha + p.to(BF).to(f32) @ vp[:, :, t * BK:(t + 1) * BK].transpose(1, 2)
            m = m_new
        out[:, h] = torch.where(l > 0, o / l.clamp_min(1e-37), torch.zeros_like(o))
    return out.transpose(1, 2).reshape(B, T, Hq * DH).to(BF)


def attention_inputs(B, Hq, Hkv, T, row_start, seed, ldvt=None, planted=True):
    """q (B,T,Hq*256), k, v (B,T,Hkv*256) bf16 randn, and V^T (B,Hkv*256,ldvt) with pad columns alternating +-1024.  K and V rows
    below row_start hold +-1024, and with ``planted`` the K row at row_start - 1 is 1024 * sign(q[row_start]) of the group's
    first query head: admitted by mistake, it takes the whole of that row."""
    g = torch.Generator().manual_seed(seed * 1000003 + ((B * 131 + Hq) * 4099 + Hkv) * 4099 + T)
    q = torch.randn(B, T, Hq * DH, generator=g).to(BF)
    k = torch.randn(B, T, Hkv * DH, generator=g).to(BF)
    v = torch.randn(B, T, Hkv * DH, generator=g).to(BF)
    alt = (1024.0 * (1 - 2 * (torch.arange(Hkv * DH) % 2))).to(BF)
    for b, rs in enumerate(row_start):
        rs = min(int(rs), T)
        if rs > 0:
            sg = (1 - 2 * (torch.arange(rs) % 2)).to(BF)[:, None]
            k[b, :rs] = alt[None, :] * sg
            v[b, :rs] = -alt[None, :] * sg
            if planted and rs < T:
                qs = q[b, rs].float().reshape(Hq, DH)[::Hq // Hkv].reshape(-1)
                k[b, rs - 1] = (1024.0 * torch.where(qs >= 0, 1.0, -1.0)).to(BF)
    ldvt = ldvt or (-(-T // 64) * 64 + 8)
    vt = torch.empty(B, Hkv * DH, ldvt, dtype=BF)
    vt[:, :, :T] = v.transpose(1, 2)
    vt[:, :, T:] = (1024.0 * (1 - 2 * (torch.arange(ldvt - T) % 2))).to(BF)
    return q, k, v, vt


# ------------------------------------------------------------------------------------------------------------ whole model
def forward(W, cfg, input_ids, attention_mask, policy: str = "f64", tables=None, embed_scale=None):
    """The L+1 hidden states [(B,T,D) float64] of the Gemma-3 text encoder for CPU weights W (the keys of
    ``random_gemma_weights``) and a ``GemmaConfig``.  policy "f64": nothing rounded; "bf16": rounded where include/ltxk.h says
    (embedding, every norm, every GEMM output, the norm + rope, P and O of attention, both GeGLU roundings, both residual adds).
    ``tables``: {is_global: (cos, sin)} (T,128) float64 to use instead of the float64 host tables (bf16-rounded ones under the
    bf16 policy).  ``embed_scale``: the embedding scale, by default bf16(sqrt(D)) under both policies - the value the reference
    forms (text_encoder.py:107) and ltxk_embed_rows is handed."""
    assert policy in ("f64", "bf16")
    r = rbf if policy == "bf16" else (lambda t: t)
    g = lambda k: f64(W[k])
    B, T = input_ids.shape
    rs = [T - int(n) for n in attention_mask.to(torch.int64).sum(1)]
    Hq, Hkv, eps = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.rms_norm_eps
    nq, nkv = Hq * DH, Hkv * DH
    scale = float(cfg.query_pre_attn_scalar) ** -0.5
    if tables is None:
        tables = {True: rope_tables(T, cfg.rope_theta, cfg.rope_scaling_factor, round_bf16=policy == "bf16"),
                  False: rope_tables(T, cfg.rope_local_base_freq, round_bf16=policy == "bf16")}
    s = float(torch.tensor(cfg.hidden_size ** 0.5, dtype=BF)) if embed_scale is None else float(embed_scale)
    x = r(g("embed_tokens.weight")[input_ids.to(torch.int64)] * s)
    states = [x]
    L = cfg.num_hidden_layers
    for i in range(L):
        p = f"layers.{i}."
        glob = cfg.is_global(i)
        cos, sin = tables[glob]
        nx = r(rmsnorm(x, g(p + "input_layernorm.weight"), eps))
        q, k, v = (r(nx @ g(p + f"self_attn.{n}_proj.weight").T) for n in "qkv")
        q = headnorm_rope(q, Hq, g(p + "self_attn.q_norm.weight"), cos, sin, eps, r)
        k = headnorm_rope(k, Hkv, g(p + "self_attn.k_norm.weight"), cos, sin, eps, r)
        att = causal_attention(q, k, v, Hq, Hkv, rs, 0 if glob else cfg.sliding_window, scale, bf16_p=policy == "bf16",
                               exact_c=policy == "f64")[0]
        po = r(att @ g(p + "self_attn.o_proj.weight").T)
        y = r(x + r(rmsnorm(po, g(p + "post_attention_layernorm.weight"), eps)))
        nx = r(rmsnorm(y, g(p + "pre_feedforward_layernorm.weight"), eps))
        gate, up = r(nx @ g(p + "mlp.gate_proj.weight").T), r(nx @ g(p + "mlp.up_proj.weight").T)
        h = r(r(gelu_tanh(gate)) * up)
        po = r(h @ g(p + "mlp.down_proj.weight").T)
        x = r(y + r(rmsnorm(po, g(p + "post_feedforward_layernorm.weight"), eps)))
        if i + 1 < L:
            states.append(x)
    states.append(r(rmsnorm(x, g("norm.weight"), eps)))
    return states


def tiny_config(sliding_window: int):
    """The test model: hidden 512, intermediate 1024, 6 layers (5 local + 1 global), 4 heads, 2 KV heads, head dim 256, vocab 512."""
    from mlx_video_amd.gemma import GemmaConfig
    return GemmaConfig(hidden_size=512, num_hidden_layers=6, num_attention_heads=4, num_key_value_heads=2, head_dim=256,
                       intermediate_size=1024, vocab_size=512, sliding_window=sliding_window, sliding_window_pattern=6,
                       query_pre_attn_scalar=256.0, rms_norm_eps=1e-6, rope_theta=1_000_000.0, rope_local_base_freq=10_000.0,
                       rope_scaling_factor=8.0)


def tiny_inputs(B: int = 2, T: int = 96, pad: int = 59, vocab: int = 512, seed: int = 5):
    """ids, mask (B,T) int64: row 0 full, row 1 left-padded by ``pad`` (pad id 0)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.int64)
    if B > 1:
        ids[1, :pad] = 0
        mask[1, :pad] = 0
    return ids, mask


def rel_l2_valid(a, b, mask):
    """rel-L2 of a against b over the valid rows of a (B,T,D) state."""
    m = mask.bool()
    a, b = f64(a)[m], f64(b)[m]
    return float((a - b).norm() / b.norm())
