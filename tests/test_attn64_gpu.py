"""ltxk_flash_attn_dh64 and ltxk_qknorm_rope_dh64 (the audio transformer's head dim) on the device.

Attention: element by element against float64 (ref_attn64.attention / ref64.attention_bound - the derivation of
tests/test_attn_bound_gpu.py with dh = 64 in dx; tests/test_audio_dit_cpu.py shows on the CPU that the bound accepts the
oracle's two policies and an fp32 emulation of a 64-key-tile loop and rejects four planted faults).  Nothing in the bound is
measured.  Operands are the strided views and sentinels of test_attn_bound_gpu._launch at H*64 columns: q with ldq = D + 8,
k the left half of a (B*Tk, 2D) buffer whose right half is NaN, V^T with ldvt = roundup64(Tk) + 8 and pad columns +-1024,
out inside NaN sentinels that must survive; q, k and V^T are exactly sized, so a load past the last batch row's ragged tile
leaves the allocation.  Every case launches twice and requires identical bits.  The kernel has one launch form: no plan.

Row kernel: the cases and the comparator call of test_rowops_gpu.py::test_qknorm_rope_edges against the head-dim-general
restatement (ref_attn64.qknorm_rope)."""
import math

import parity
import pytest
import torch

import ref64 as R
import ref_attn64 as R64
import ref_rows as RR
from test_rowops_gpu import _close, _g, _ops, _sent_bf16, _untouched, _within

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DH = 64
SCALE = 1.0 / math.sqrt(DH)

# (B, H, Tq, Tk): Tk below one key tile (1, 5, 33), exactly one (64), one key into the second (65), ragged in the second (70, 97),
# two whole (128), one into the third (129); Tq ragged inside a 16-row block and across 64-row tiles; the audio workload's own
# shapes (self-attention 126 x 126, text attention 126 x 1024); one long query axis (21 query tiles, the last of 20 rows).
SHAPES = [(1, 1, 1, 1), (1, 2, 77, 5), (1, 4, 200, 33), (1, 3, 200, 70), (2, 3, 129, 65), (1, 4, 130, 64), (1, 2, 16, 97),
          (1, 2, 100, 128), (1, 2, 100, 129), (1, 32, 126, 126), (1, 32, 126, 1024), (1, 4, 1300, 70)]


def _launch(dev, q, k, v, H, scale=SCALE):
    """test_attn_bound_gpu._launch at head dim 64 (see the module docstring).  q, k, v: (B,T,D) on the device."""
    from mlx_video_amd import ops
    B, Tq, D = q.shape
    Tk = k.shape[1]
    qb = _sent_bf16((B * Tq, D + 8), dev)
    qb[:, :D] = q.reshape(B * Tq, D)
    kb = _sent_bf16((B * Tk, 2 * D), dev)
    kb[:, :D] = k.reshape(B * Tk, D)
    ldvt = (Tk + 63) // 64 * 64 + 8
    vt = torch.empty((B, D, ldvt), dtype=BF, device=dev)
    vt[:, :, Tk:] = (1024.0 * (1 - 2 * (torch.arange(ldvt - Tk, device=dev) % 2))).to(BF)
    vt[:, :, :Tk] = v.transpose(1, 2)
    ob = _sent_bf16((B * Tq + 3, D + 64), dev)
    out = ob[1:1 + B * Tq, :D]
    ops.flash_attn(qb[:, :D], kb[:, :D], vt, out, B, H, Tq, Tk, scale, head_dim=DH)
    torch.cuda.synchronize()
    assert _untouched(ob[0]) and _untouched(ob[1 + B * Tq:]) and _untouched(ob[:, D:]), "wrote outside the output view"
    return out.reshape(B, Tq, D)


def _ratio(what, out, ref, Tk):
    assert not bool(torch.isnan(out).any()), f"{what}: NaN inside the output view (rows left unwritten, or 0/0)"
    d, bound = R64.attention_bound(out, *ref, Tk)
    ratio = d / bound
    worst = float(ratio.max())
    print(f"{what}: worst d/bound {worst:.4f}")
    if worst > 1.0:
        b, row, ch = (int(i) for i in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} elements in {int((ratio > 1).any(-1).sum())} of {ratio.shape[0] * ratio.shape[1]} "
                             f"rows beyond the bound, worst d/bound {worst:.4g} at (b, row, head, channel) = ({b}, {row}, {ch // DH}, {ch % DH}): "
                             f"got {float(out[b, row, ch]):.8g}, exact {float(ref[0][b, row, ch]):.8g}")
    return ratio


@pytest.mark.parametrize("family", R64.ATTN_FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_dh64_within_float64_bound(dev, shape, family):
    B, H, Tq, Tk = shape
    q, k, v, planted = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in R64.attention_inputs(B, H, Tq, Tk, family, 0, DH))
    if family == "spiked":
        p = R64.attention_probs(q, k, H, SCALE, DH)[0]
        assert planted and all(float(p[:, :, r, j].min()) >= 0.25 for r, j in planted), "a planted key holds less than 0.25 of its row"
    ref = R64.attention(q, k, v, H, SCALE, DH)
    out = _launch(dev, q, k, v, H)
    ratio = _ratio(f"dh64 {shape} {family}", out, ref, Tk)
    parity.auto(float(ratio.max()), 1.0, tag="d_over_bound")
    assert torch.equal(_launch(dev, q, k, v, H).view(torch.int16), out.view(torch.int16)), "two launches differ"


def test_attention_dh64_batch_rows_independent(dev):
    """One launch form, keys never split: a B = 3 launch is three B = 1 launches bit for bit (and each head's bits those of
    an H = 1 launch of that head)."""
    B, H, Tq, Tk = 3, 5, 77, 130
    q, k, v, _ = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in R64.attention_inputs(B, H, Tq, Tk, "flat", 2, DH))
    whole = _launch(dev, q, k, v, H)
    for b in range(B):
        one = _launch(dev, q[b:b + 1], k[b:b + 1], v[b:b + 1], H)
        assert torch.equal(one.view(torch.int16), whole[b:b + 1].view(torch.int16)), f"batch row {b} depends on the launch it runs in"
    h = 3
    sl = slice(h * DH, (h + 1) * DH)
    one = _launch(dev, q[:1, :, sl].contiguous(), k[:1, :, sl].contiguous(), v[:1, :, sl].contiguous(), 1)
    assert torch.equal(one.view(torch.int16), whole[:1, :, sl].contiguous().view(torch.int16)), "a head depends on the launch it runs in"


def test_attention_dh64_refuses_fused_query_prep(dev):
    """The C entry itself (not only the shim): q_sumsq set is LTXK_EINVAL, nothing is launched."""
    import ctypes
    from mlx_video_amd import _lib
    q = torch.zeros(64, 64, dtype=BF, device=dev)
    vt = torch.zeros(1, 64, 64, dtype=BF, device=dev)
    ss = torch.zeros(64, 4, dtype=torch.float32, device=dev)
    a = _lib.AttnArgs()
    a.q = a.k = a.out = q.data_ptr()
    a.vt = vt.data_ptr()
    a.ldq = a.ldk = a.ldo = a.ldvt = 64
    a.B, a.H, a.Tq, a.Tk, a.scale = 1, 1, 64, 64, SCALE
    a.q_sumsq, a.q_sumsq_ld, a.q_sumsq_n = ss.data_ptr(), 4, 1
    assert _lib.load().ltxk_flash_attn_dh64(ctypes.byref(a), 0) == -1


@pytest.mark.parametrize("rope", [False, True], ids=["norope", "rope"])
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("ss", [False, True], ids=["reduce", "sumsq"])
@pytest.mark.parametrize("H", [8, 16, 24, 32])
def test_qknorm_rope_dh64_edges(dev, H, ss, nseg, rope):
    """test_rowops_gpu.py::test_qknorm_rope_edges at head dim 64: ld = nseg*D + 64, B = 2 so that t = row % T wraps; idle
    lanes of the second 16-head pass (H = 24), a rotation partner other than j + 32, a table indexed at 64 instead of 32 per
    row, a partials reduction over D/128 instead of D/64 entries, writes past nseg*D or past row M."""
    ops = _ops()
    inp = RR.qknorm_inputs(H, ss, nseg, rope, DH)
    T, M, D, x, w, cos, sin = inp.T, inp.M, inp.D, inp.x, inp.w, inp.cos, inp.sin
    ld = nseg * D + 64
    buf = _sent_bf16((M + 2, ld), dev)
    buf[:M, :nseg * D] = x.to(dev)
    sumsq = inp.sumsq.to(dev) if ss else None
    ops.qknorm_rope(buf[:M], nseg, D, w.to(dev), cos.to(dev) if rope else None, sin.to(dev) if rope else None, T, H, 1e-6,
                    sumsq=sumsq, head_dim=DH)
    torch.cuda.synchronize()
    assert _untouched(buf[:M, nseg * D:]), "columns past nseg*D were written"
    assert _untouched(buf[M:]), "a row past M was written"
    ref, mag = R64.qknorm_rope(x, w, cos, sin, T, H, R.f32(1e-6), DH)
    _close(buf[:M, :nseg * D].cpu(), ref, max_ulps=2 if rope else 1, max_frac=1e-2, mag=mag)
    _within(buf[:M, :nseg * D].cpu(), RR.qknorm_rope(x, w, cos, sin, T, H, R.f32(1e-6), DH, RR.qknorm_partials(inp)))
