"""The kernels of the Gemma-3 text encoder (csrc/text_ops.hip, csrc/causal_attn.hip) through mlx_video_amd.ops, each held
element by element to its float64 value.  Every bound is written out from the arithmetic the header states, with u = 2^-24
(one fp32 rounding), ulp_bf16(v) = 2^(floor(log2 |v|) - 7) and a chain of k fp32 additions of positive terms off by at most
k*u relative; nothing in them is a measured tolerance.  Outputs sit inside sentinel (NaN) borders that must survive, inputs
and outputs are strided views, and each case launches twice and requires identical bits.

  embed_rows            table and scale are bf16 values, so table * s is exact in fp32: out == r(table[id] * s) bit for bit.
  rmsnorm_weight_rows   sum of squares: squares of bf16 values are exact, a lane adds at most 128 of them in a row (D <= 8192)
                        and the wave's butterfly 6 more: 134u; /D, +eps: 2u; rsqrt halves that and adds its own 2u: 70u;
                        x*rstd, 1+w, their product: 3u.  73u, stated as E_NORM = 80u:
                            |y - y64| <= 1/2 ulp_bf16(y) + 80u |y64|
                        With resid the normed value n is rounded to bf16 before the add (one more half ulp, of n) and the fp32
                        add rounds once:  |y - (resid + n64)| <= 1/2 ulp_bf16(y) + 1/2 ulp_bf16(n64 (1 + 2^-7)) + 80u |n64| + u |y64|.
  headnorm_rope         the head's 256 squares: 16 per lane and 4 butterfly levels, 20u, + 2u, halved, + 2u + 3u = 16u, stated as
                        E_HEAD = 20u.  The normed x' is rounded to bf16: e(x') = 1/2 ulp_bf16(x'64 (1 + 2^-7)) + 20u |x'64|.  cos / sin
                        are bf16 values, so x' * c is exact in fp32 and the sum rounds once:
                            |o1 - (x1' c - x2' s)| <= 1/2 ulp_bf16(o1) + |c| e(x1') + |s| e(x2') + u (|x1' c| + |x2' s|)
  geglu_tanh            gelu_tanh(g) = g / (1 + exp(-2a)), a = sqrt(2/pi)(g + 0.044715 g^3): a carries <= 6u relative (no
                        cancellation: g and g^3 share a sign), so exp(-2a), finite only for |2a| < 88.8, is off by
                        88.8 * 7u + 2u (expf) relative, the sum, the division and the constant's rounding add 4u: 630u < 2^-14
                        = E_GELU.  h = r(gelu) and h * u is exact in fp32 (two bf16 values):
                            |out - gelu64 * u| <= 1/2 ulp_bf16(out) + |u| (1/2 ulp_bf16(gelu64 (1 + 2^-7)) + 2^-14 |gelu64| + 2^-126)
                        (2^-126: a flushed subnormal).
  causal_attn           ref_gemma.attention_bound (the derivation is tests/ref64.py's, restated for head dim 256 and the visible
                        keys; tests/test_gemma_cpu.py shows what it accepts and rejects).  Worst d / bound is recorded with the
                        stated bound 1.0."""
import parity
import pytest
import torch

import ref_gemma as G
from test_rowops_gpu import _sent_bf16, _untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U = 2.0 ** -24
E_NORM, E_HEAD, E_GELU = 80 * U, 20 * U, 2.0 ** -14
ROWS_PER_WG = 4             # ops.GEMMA_ROWS_PER_WG: one wave per row, four rows per workgroup
BQ, BK = 64, 64             # ops.CAUSAL_ATTN_BQ / CAUSAL_ATTN_BK: query rows per workgroup, keys per tile
ROW_DS = (8, 264, 512, 3840)
ROW_MS = (1, 3, ROWS_PER_WG - 1, ROWS_PER_WG + 1)


def test_constants_are_the_kernels():
    from mlx_video_amd import ops
    assert (ops.GEMMA_ROWS_PER_WG, ops.CAUSAL_ATTN_BQ, ops.CAUSAL_ATTN_BK, ops.GEMMA_HEAD_DIM) == (ROWS_PER_WG, BQ, BK, 256)


def _frame(M, D, dev):
    """A (M,D) bf16 view inside a sentinel buffer: one row above, two below, 8 columns left, 24 right; 16-byte aligned."""
    buf = _sent_bf16((M + 3, D + 32), dev)
    return buf, buf[1:1 + M, 8:8 + D]


def _border_ok(buf, M, D):
    b = buf.clone()
    b[1:1 + M, 8:8 + D] = _sent_bf16((M, D), buf.device)
    return _untouched(b)


def _strided(x, dev):
    """x (M,D) as a view with row stride D + 8 on the device."""
    M, D = x.shape
    buf = _sent_bf16((M, D + 8), dev)
    buf[:, :D] = x.to(dev)
    return buf[:, :D]


def _ratio(d, bound):
    assert not bool(torch.isnan(d).any())
    return float((d / bound).max())


def _hulp(v):
    return 0.5 * G.ulp_bf16(v)


@pytest.mark.parametrize("D", ROW_DS)
def test_embed_rows(dev, D):
    from mlx_video_amd import ops
    V, M = 37, 6
    g = torch.Generator().manual_seed(D)
    table = torch.randn(V, D, generator=g).to(BF)
    ids = torch.tensor([0, V - 1, 5, 5, 17, V - 1], dtype=torch.int32)          # first and last vocabulary row
    s = float(torch.tensor(D ** 0.5, dtype=BF))
    buf, out = _frame(M, D, dev)
    ops.embed_rows(table.to(dev), ids.to(dev), s, out=out, ids_host=ids)
    first = out.clone()
    ops.embed_rows(table.to(dev), ids.to(dev), s, out=out)
    assert torch.equal(first.view(torch.int16), out.view(torch.int16)) and _border_ok(buf, M, D)
    ref = (table.double()[ids.long()] * s).to(torch.float32).to(BF)             # exact product, one rounding
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))
    for bad in ([0, V], [-1, 0]):
        with pytest.raises(ValueError, match="token ids"):
            ops.embed_rows(table.to(dev), torch.tensor(bad, dtype=torch.int32, device=dev), s)


@pytest.mark.parametrize("D", ROW_DS)
@pytest.mark.parametrize("M", sorted(set(ROW_MS)))
def test_rmsnorm_weight_rows(dev, D, M):
    from mlx_video_amd import ops
    eps = 1e-6
    g = torch.Generator().manual_seed(D * 16 + M)
    x = (torch.randn(M, D, generator=g) * 3).to(BF)
    zero_row = M > 1
    if zero_row:
        x[M - 1] = 0                                                              # a zero row: eps alone under the root
    w = (torch.randn(D, generator=g) * 0.3).to(BF)
    res = torch.randn(M, D, generator=g).to(BF)
    n64 = G.rmsnorm(x.double(), w.double(), eps)
    xs, wd = _strided(x, dev), w.to(dev)
    # plain
    buf, out = _frame(M, D, dev)
    ops.rmsnorm_weight_rows(xs, wd, eps, out=out)
    first = out.clone()
    ops.rmsnorm_weight_rows(xs, wd, eps, out=out)
    assert torch.equal(first.view(torch.int16), out.view(torch.int16)) and _border_ok(buf, M, D)
    o = out.cpu().double()
    parity.auto(_ratio((o - n64).abs(), _hulp(o) + E_NORM * n64.abs() + 2.0 ** -126), 1.0, tag="plain")
    assert not zero_row or bool((out[M - 1] == 0).all())
    # with the residual, y aliasing resid (a strided view)
    y64 = res.double() + n64
    bound = lambda o: _hulp(o) + _hulp(n64 * (1 + 2.0 ** -7)) + E_NORM * n64.abs() + U * y64.abs() + 2.0 ** -126
    buf, rv = _frame(M, D, dev)
    rv.copy_(res.to(dev))
    ops.rmsnorm_weight_rows(xs, wd, eps, resid=rv, out=rv)
    assert _border_ok(buf, M, D)
    o = rv.cpu().double()
    parity.auto(_ratio((o - y64).abs(), bound(o)), 1.0, tag="resid_alias")
    # and into a separate output: the same bits
    buf2, out2 = _frame(M, D, dev)
    ops.rmsnorm_weight_rows(xs, wd, eps, resid=_strided(res, dev), out=out2)
    assert torch.equal(out2.view(torch.int16), rv.view(torch.int16)) and _border_ok(buf2, M, D)
    assert not zero_row or bool((rv[M - 1].cpu() == res[M - 1]).all())           # zero row: the residual passes through


@pytest.mark.parametrize("Hq,Hkv", [(1, 1), (4, 2), (16, 8)])
@pytest.mark.parametrize("T", [1, 5, 130])
def test_headnorm_rope(dev, Hq, Hkv, T):
    from mlx_video_amd import ops
    from mlx_video_amd.gemma import rope_table_half
    eps = 1e-6
    M, NH = 2 * T, Hq + Hkv                                                       # M = 2T: m % T wraps
    cols = NH * 256
    g = torch.Generator().manual_seed((Hq * 32 + Hkv) * 1024 + T)
    x = (torch.randn(M, cols, generator=g) * 2).to(BF)
    x[0, :256] = 0                                                                # a zero head
    qw, kw = (torch.randn(256, generator=g) * 0.3).to(BF), (torch.randn(256, generator=g) * 0.3).to(BF)
    cos, sin = rope_table_half(T, 1e6, 8.0)
    extra = 16                                                                    # columns past (Hq+Hkv)*256: untouched
    buf = _sent_bf16((M + 2, cols + extra), dev)
    view = buf[1:1 + M]
    view[:, :cols] = x.to(dev)
    ops.headnorm_rope(view, Hq, Hkv, qw.to(dev), kw.to(dev), cos.to(dev), sin.to(dev), T, eps)
    got = view[:, :cols].cpu()
    chk = buf.clone()
    chk[1:1 + M, :cols] = _sent_bf16((M, cols), dev)
    assert _untouched(chk)
    buf2 = _sent_bf16((M + 2, cols + extra), dev)
    buf2[1:1 + M, :cols] = x.to(dev)
    ops.headnorm_rope(buf2[1:1 + M], Hq, Hkv, qw.to(dev), kw.to(dev), cos.to(dev), sin.to(dev), T, eps)
    assert torch.equal(buf2[1:1 + M, :cols].cpu().view(torch.int16), got.view(torch.int16))
    # float64: the normed head unrounded, then the rotation
    w = torch.cat([qw.double().expand(Hq, 256), kw.double().expand(Hkv, 256)], 0)         # (NH,256)
    xn = G.rmsnorm(x.double().reshape(M, NH, 256), w[None], eps)
    c = cos.double()[torch.arange(M) % T][:, None, :]
    s = sin.double()[torch.arange(M) % T][:, None, :]
    x1, x2 = xn[..., :128], xn[..., 128:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    e = lambda v: _hulp(v * (1 + 2.0 ** -7)) + E_HEAD * v.abs()
    lin = c.abs() * e(x1) + s.abs() * e(x2) + U * ((x1 * c).abs() + (x2 * s).abs())
    lin2 = c.abs() * e(x2) + s.abs() * e(x1) + U * ((x2 * c).abs() + (x1 * s).abs())
    o = got.double().reshape(M, NH, 256)
    bound = _hulp(o) + torch.cat([lin, lin2], -1) + 2.0 ** -126
    parity.auto(_ratio((o - y).abs(), bound), 1.0)
    assert bool((got[0, :256] == 0).all())


@pytest.mark.parametrize("F", [8, 1032])
@pytest.mark.parametrize("M", [1, 5])
def test_geglu_tanh(dev, F, M):
    from mlx_video_amd import ops
    g = torch.Generator().manual_seed(F * 8 + M)
    gate = (torch.randn(M, F, generator=g) * 3).to(BF)
    up = (torch.randn(M, F, generator=g) * 2).to(BF)
    edge = torch.tensor([300.0, -300.0, 12.0, -12.0, -6.0, 0.0, 3e38, -3e38]).to(BF)      # |g| large on both sides
    gate[0, :8] = edge
    up[0, :8] = 0.5                                                               # keeps 3e38 * u inside bf16
    buf = _sent_bf16((M + 2, 2 * F + 8), dev)
    view = buf[1:1 + M, :2 * F]
    view.copy_(torch.cat([gate, up], 1).to(dev))
    out = ops.geglu_tanh_(view)
    assert out.data_ptr() == view.data_ptr() and tuple(out.shape) == (M, F) and out.stride(0) == 2 * F + 8
    got = out.cpu()
    assert torch.equal(view[:, F:].cpu().view(torch.int16), up.view(torch.int16))          # u is only read
    chk = buf.clone()
    chk[1:1 + M, :2 * F] = _sent_bf16((M, 2 * F), dev)
    assert _untouched(chk)
    buf2 = _sent_bf16((M + 2, 2 * F + 8), dev)
    buf2[1:1 + M, :2 * F] = torch.cat([gate, up], 1).to(dev)
    assert torch.equal(ops.geglu_tanh_(buf2[1:1 + M, :2 * F]).cpu().view(torch.int16), got.view(torch.int16))
    ge = G.gelu_tanh(gate.double())
    y = ge * up.double()
    o = got.double()
    bound = _hulp(o) + up.double().abs() * (_hulp(ge * (1 + 2.0 ** -7)) + E_GELU * ge.abs() + 2.0 ** -126) + 2.0 ** -126
    parity.auto(_ratio((o - y).abs(), bound), 1.0)
    assert float(got[0, 1]) == 0.0 and float(got[0, 7]) == 0.0                              # gelu(-300) = gelu(-3e38) = -0
    assert float(got[0, 0]) == float((torch.tensor(300.0).to(BF).float() * up[0, 0].float()).to(BF))


# ------------------------------------------------------------------------------------------------------ causal_attn
# (B, Hq, Hkv, T, row_start, window)
ATTN_CASES = [
    (1, 1, 1, 1, [0], 0),
    (2, 4, 2, 17, [0, 16], 0),                       # one row has a single visible key
    (2, 2, 2, 65, [0, 1], 0),
    (4, 4, 2, 129, [0, 64, 128, 129], 0),            # the last batch row is all padding: all zeros
    (1, 8, 1, 200, [37], 0),
    (1, 8, 1, 200, [37], 64),
    (1, 8, 1, 200, [37], 65),
    (2, 2, 2, 320, [0, 255], 0),
    (2, 1, 1, BK - 1, [0, 5], 0),                    # T one before, at (below: 128 + 1 = 129, 64 + 1 = 65) the tile size
    (2, 1, 1, BK, [0, BK - 1], 0),
]
# row_start and window one before, at and one after every boundary of the key tile (BK) and the query tile (BQ) inside T = 200
_EDGES = sorted({m * s + d for s in (BQ, BK) for m in (1, 2) for d in (-1, 0, 1)})       # 63, 64, 65, 127, 128, 129
ATTN_CASES += [(len(_EDGES), 2, 1, 200, _EDGES, w) for w in [0] + _EDGES]
SCALE = 256.0 ** -0.5


def _attn_launch(dev, q, k, vt, B, Hq, Hkv, T, rs, window):
    """ops.causal_attn on the views the module passes: q | k halves of one fused projection buffer (row stride nq + nkv + 8),
    V^T with ldvt > T and live pad columns, out a view inside a sentinel buffer.  Returns (out on the host, sentinel border ok)."""
    from mlx_video_amd import ops
    nq, nkv = Hq * 256, Hkv * 256
    qk = _sent_bf16((B * T, nq + nkv + 8), dev)
    qk[:, :nq] = q.reshape(B * T, nq).to(dev)
    qk[:, nq:nq + nkv] = k.reshape(B * T, nkv).to(dev)
    buf = _sent_bf16((B * T + 3, nq + 64), dev)
    out = buf[1:1 + B * T, :nq]
    ops.causal_attn(qk[:, :nq], qk[:, nq:nq + nkv], vt.to(dev), out, torch.tensor(rs, dtype=torch.int32, device=dev), B, Hq, Hkv, T,
                    SCALE, window=window)
    got = out.cpu().reshape(B, T, nq)
    buf[1:1 + B * T, :nq] = _sent_bf16((B * T, nq), dev)
    return got, _untouched(buf)


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "B%d_Hq%d_Hkv%d_T%d_rs%s_w%d" % (c[0], c[1], c[2], c[3], "-".join(map(str, c[4])), c[5]))
def test_causal_attn(dev, case):
    B, Hq, Hkv, T, rs, window = case
    q, k, v, vt = G.attention_inputs(B, Hq, Hkv, T, rs, seed=11)
    assert vt.shape[2] > T and float(vt[:, :, T:].abs().min()) == 1024.0
    got, ok = _attn_launch(dev, q, k, vt, B, Hq, Hkv, T, rs, window)
    assert ok, "sentinels around the output view were overwritten"
    again, _ = _attn_launch(dev, q, k, vt, B, Hq, Hkv, T, rs, window)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))
    y, A, dx, nvis = G.causal_attention(q, k, v, Hq, Hkv, rs, window, SCALE)
    d, bound = G.attention_bound(got, y, A, dx, nvis)
    worst = float((d / bound).max())
    print(f"worst d / bound = {worst:.3f}")
    parity.auto(worst, 1.0)
    for b in range(B):
        assert bool((got[b, :min(rs[b], T)] == 0).all()), f"padded query rows of batch row {b} are not exactly zero"
        # the batch row launched alone: the same bits
        one, _ = _attn_launch(dev, q[b:b + 1], k[b:b + 1], vt[b:b + 1], 1, Hq, Hkv, T, rs[b:b + 1], window)
        assert torch.equal(one[0].view(torch.int16), got[b].view(torch.int16)), f"batch row {b} alone gives other bits"


def test_causal_attn_argument_checks(dev):
    from mlx_video_amd import ops
    from mlx_video_amd._lib import LtxkError
    B, Hq, Hkv, T = 1, 2, 1, 8
    q = torch.zeros(B * T, Hq * 256, dtype=BF, device=dev)
    k = torch.zeros(B * T, Hkv * 256, dtype=BF, device=dev)
    vt = torch.zeros(B, Hkv * 256, 64, dtype=BF, device=dev)
    rs = torch.zeros(B, dtype=torch.int32, device=dev)
    with pytest.raises(LtxkError, match="multiple of Hkv"):
        ops.causal_attn(torch.zeros(B * T, 3 * 256, dtype=BF, device=dev), torch.zeros(B * T, 512, dtype=BF, device=dev),
                        torch.zeros(B, 512, 64, dtype=BF, device=dev), torch.zeros(B * T, 3 * 256, dtype=BF, device=dev), rs, B, 3, 2, T, SCALE)
    with pytest.raises(LtxkError, match="window"):
        ops.causal_attn(q, k, vt, torch.empty_like(q), rs, B, Hq, Hkv, T, SCALE, window=-1)
    with pytest.raises(LtxkError, match="scale"):
        ops.causal_attn(q, k, vt, torch.empty_like(q), rs, B, Hq, Hkv, T, 0.0)
    with pytest.raises(ValueError, match="vt"):
        ops.causal_attn(q, k, vt[:, :, :4], torch.empty_like(q), rs, B, Hq, Hkv, T, SCALE)
    with pytest.raises(TypeError):
        ops.causal_attn(q, k, vt, torch.empty_like(q), rs.long(), B, Hq, Hkv, T, SCALE)
