"""The accept side of tests/test_ops_shims_cpu.py on the device: the shims of the DiT block called on the views the model
passes - a row slice [N:2N] of a buffer shared by the batch, a column offset D into the packed q|k buffer, a (U,6,D)
modulation table read through ``mod[:, k]`` and its row stride, a block's slot of the stacked text k / V^T - against the same
call on contiguous copies laid out as a fresh caller would lay them.  The outputs must be bit-equal and a sentinel that
fills everything outside the written region must survive: the operand checks of ``ops`` are not written around contiguous
tensors only, and a view's strides reach the kernels as they are."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
B, H, D, N, S = 2, 4, 512, 64, 32
P, M = D // 64, B * N
SENT = 7.0
SC = 1.0 / math.sqrt(128)


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(BF)


def _sent(dev, *shape, dtype=BF):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _untouched(t):
    return bool((t == SENT).all())


@pytest.fixture(scope="module")
def data(dev):
    g = torch.Generator().manual_seed(77)
    d = dict(qk=_rand(g, M, 2 * D), vt=_rand(g, B, D, N), x=_rand(g, M, D), wide=_rand(g, M, 2 * D), mod=_rand(g, 3, 6, D, scale=0.1),
             wqkv=_rand(g, 3 * D, D, scale=D ** -0.5), bqkv=_rand(g, 3 * D, scale=0.1), wo=_rand(g, D, D, scale=D ** -0.5), bo=_rand(g, D, scale=0.1),
             wn=(1 + 0.1 * torch.randn(D, generator=g)).to(BF), k2=_rand(g, 3, B * S, D), vt2=torch.zeros(3, B, D, 64, dtype=BF))
    d["vt2"][..., :S] = _rand(g, 3, B, D, S)
    ang = torch.rand(H, N, 64, generator=g) * (2 * math.pi)
    d["cos"], d["sin"] = torch.cos(ang), torch.sin(ang)
    d = {k: v.to(dev) for k, v in d.items()}
    d["qkss"] = (d["qk"].float() ** 2).reshape(M, 2 * P, 64).sum(-1)          # per-64-column sums of squares, as the GEMM emits them
    d["xss"] = (d["x"].float() ** 2).reshape(M, P, 64).sum(-1)
    d["rows"] = (torch.arange(M, device=dev, dtype=torch.int32) // 40) % 3      # token -> modulation row
    return d


def test_flash_attn_takes_the_models_views(dev, data):
    from mlx_video_amd import ops
    qk, vt, qkss = data["qk"], data["vt"], data["qkss"]
    rows = slice(N, 2 * N)
    for name, kw_view, kw_flat in (("plain", {}, {}),
                                   ("fused", dict(q_sumsq=qkss[rows], q_norm_weight=data["wn"], cos=data["cos"], sin=data["sin"]),
                                    dict(q_sumsq=qkss[rows, :P].contiguous(), q_norm_weight=data["wn"], cos=data["cos"], sin=data["sin"]))):
        att = _sent(dev, M, D)
        ops.flash_attn(qk[rows, :D], qk[rows, D:], vt[1:2], att[rows], 1, H, N, N, SC, tail_split=False, **kw_view)
        flat = _sent(dev, N, D)
        ops.flash_attn(qk[rows, :D].contiguous(), qk[rows, D:].contiguous(), vt[1:2].contiguous(), flat, 1, H, N, N, SC, tail_split=False, **kw_flat)
        assert _same(att[rows], flat) and not _untouched(flat), name
        assert _untouched(att[:N]), f"{name}: rows outside the slice were written"
    # text cross-attention: a block's slot of the stacked k / V^T (S = 32 keys in a V^T padded to 64), raw q with its statistics
    att = _sent(dev, M + 1, D)
    ops.flash_attn(qk[:, :D], data["k2"][1], data["vt2"][1], att[:M], B, H, N, S, SC, q_sumsq=qkss, q_norm_weight=data["wn"])
    flat = _sent(dev, M, D)
    ops.flash_attn(qk[:, :D].contiguous(), data["k2"][1].clone(), data["vt2"][1].clone(), flat, B, H, N, S, SC,
                   q_sumsq=qkss[:, :P].contiguous(), q_norm_weight=data["wn"])
    assert _same(att[:M], flat) and _untouched(att[M:]) and not bool(torch.isnan(flat.float()).any())


@pytest.mark.parametrize("with_sumsq", [False, True])
def test_qknorm_rope_takes_the_k_half(dev, data, with_sumsq):
    from mlx_video_amd import ops
    qk = data["qk"].clone()
    before = qk.clone()
    flat = qk[:, D:].contiguous()
    ops.qknorm_rope(qk[:, D:], 1, D, data["wn"], data["cos"], data["sin"], N, H, 1e-6, sumsq=data["qkss"][:, P:] if with_sumsq else None)
    ops.qknorm_rope(flat, 1, D, data["wn"], data["cos"], data["sin"], N, H, 1e-6, sumsq=data["qkss"][:, P:].contiguous() if with_sumsq else None)
    assert _same(qk[:, D:], flat) and not _same(flat, before[:, D:])
    assert _same(qk[:, :D], before[:, :D]), "the q half was written"
    # a row slice of the packed buffer, both segments
    qk2, flat2 = before.clone(), before[N:2 * N].contiguous()
    ss = data["qkss"][N:2 * N] if with_sumsq else None
    ops.qknorm_rope(qk2[N:2 * N], 2, D, torch.cat([data["wn"], data["wn"]]), data["cos"], data["sin"], N, H, 1e-6, sumsq=ss)
    ops.qknorm_rope(flat2, 2, D, torch.stack([data["wn"], data["wn"]]), data["cos"], data["sin"], N, H, 1e-6, sumsq=None if ss is None else ss.clone())
    assert _same(qk2[N:2 * N], flat2) and _same(qk2[:N], before[:N])


@pytest.mark.parametrize("with_sumsq", [False, True])
def test_rmsnorm_modulate_reads_the_table_through_its_row_stride(dev, data, with_sumsq):
    from mlx_video_amd import ops
    x, mod, rows = data["x"], data["mod"], data["rows"]
    sl = slice(N, 2 * N)
    nx = _sent(dev, M, D)
    ss_wide = _sent(dev, M, 2 * P, dtype=F32)
    ss_wide[:, :P] = data["xss"]
    kw = dict(sumsq=ss_wide[sl], scale_is_one_plus=True) if with_sumsq else {}
    ops.rmsnorm_modulate(x[sl], 1e-6, mod[:, 1], mod[:, 0], 6 * D, rows[sl], out=nx[sl], **kw)
    kw = dict(sumsq=data["xss"][sl].contiguous(), scale_is_one_plus=True) if with_sumsq else {}
    flat = ops.rmsnorm_modulate(x[sl].clone(), 1e-6, mod[:, 1].contiguous(), mod[:, 0].contiguous(), D, rows[sl].clone(), **kw)
    assert _same(nx[sl], flat) and _untouched(nx[:N])
    # a modulation row other than row 0 was read: the rows differ
    assert not _same(nx[N:N + 8], ops.rmsnorm_modulate(x[N:N + 8].clone(), 1e-6, mod[:1, 1].contiguous(), mod[:1, 0].contiguous(), D, None, **(
        dict(sumsq=data["xss"][N:N + 8].contiguous(), scale_is_one_plus=True) if with_sumsq else {})))


def test_gemm_writes_into_the_models_views(dev, data):
    from mlx_video_amd import ops
    sl = slice(N, 2 * N)
    a = data["wide"][sl, D:]                                   # rows of a wider buffer at a column offset
    # q|k row-major with their statistics and V^T from one launch, into the batch row's slice of three shared buffers
    qk, vt, qkss = _sent(dev, M, 2 * D), _sent(dev, B, D, N), _sent(dev, M, 2 * P, dtype=F32)
    ops.gemm(a, data["wqkv"], data["bqkv"], out=qk[sl], out2=vt[1:2], n_split=2 * D, out_tokens_per_batch=N, sumsq=qkss[sl], split_k=False)
    fqk, fvt, fss = _sent(dev, N, 2 * D), _sent(dev, 1, D, N), _sent(dev, N, 2 * P, dtype=F32)
    ops.gemm(a.contiguous(), data["wqkv"], data["bqkv"], out=fqk, out2=fvt, n_split=2 * D, out_tokens_per_batch=N, sumsq=fss, split_k=False)
    assert _same(qk[sl], fqk) and _same(vt[1:2], fvt) and _same(qkss[sl], fss) and not _untouched(fqk) and not _untouched(fvt)
    assert _untouched(qk[:N]) and _untouched(vt[0]) and _untouched(qkss[:N])
    # gated residual in place on the residual stream, the gate read through mod[:, 2] and the token -> row map
    x, xss = data["x"].clone(), _sent(dev, M, 2 * P, dtype=F32)
    before = x.clone()
    kw = dict(epilogue=ops.EPI_BIAS_GATE_RES, split_k=False)
    ops.gemm(a, data["wo"], data["bo"], out=x[sl], resid=x[sl], gate=data["mod"][:, 2], gate_row=data["rows"][sl], gate_stride=6 * D,
             sumsq=xss[sl], **kw)
    fss = _sent(dev, N, P, dtype=F32)
    flat = ops.gemm(a.contiguous(), data["wo"], data["bo"], resid=before[sl].clone(), gate=data["mod"][:, 2].contiguous(),
                    gate_row=data["rows"][sl].clone(), gate_stride=D, sumsq=fss, **kw)
    assert _same(x[sl], flat) and _same(xss[sl, :P], fss) and not _same(flat, before[sl])
    assert _same(x[:N], before[:N]) and _untouched(xss[:N]) and _untouched(xss[:, P:])
