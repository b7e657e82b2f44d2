"""ltxk_quant_rows_fp8 against a CPU restatement of its rule, bit for bit (codes as raw bytes, scales as raw fp32 bits):

    amax = max|x| ; scale = max(amax, 2^-64) / 448 (fp32) ; q = e4m3_rne_sat(fp32(x) / scale)

Strided input, strided output between sentinel bytes that must survive.  K = 128 leaves most of a workgroup idle, 3840 is no
multiple of the 2048 elements a workgroup covers per pass, 16384 fills the eight register chunks per thread."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
BF16_MAX = 3.3895313892515355e38            # largest finite bf16
# exact ties between e4m3 neighbours once the row's scale is 1 (amax = 448): normal binades, the subnormal grid (step 2^-9)
TIES = [1.0625, 1.1875, 17.0, 19.0, 200.0, 216.0, 0.5 * 2.0 ** -9, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 2.0 ** -6 + 2.0 ** -10]


def _rows(M, K, g):
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-12, 12, (M, 1), generator=g).float())
    kinds = ["last", "zero", "max", "tiny", "ties"]
    for r in range(min(M, len(kinds))):
        kind = kinds[r]
        if kind == "last":                     # the maximum sits in the row's last element
            x[r] = x[r].clamp(-1.0, 1.0)
            x[r, K - 1] = -3.0
        elif kind == "zero":
            x[r] = 0.0
        elif kind == "max":                    # amax = the largest finite bf16
            x[r, K // 3] = BF16_MAX
        elif kind == "tiny":                   # amax = 2^-70, below the 2^-64 clamp of the scale
            x[r] = torch.exp2(torch.randint(-80, -70, (K,), generator=g).float()) * torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
            x[r, 5] = 2.0 ** -70
        elif kind == "ties":
            t = torch.tensor(TIES)
            x[r] = t[torch.arange(K) % len(TIES)] * torch.where(torch.arange(K) % 3 == 0, -1.0, 1.0)
            x[r, 7] = 448.0
    return x.to(BF)


def _reference(x):
    xf = x.float()
    amax = xf.abs().amax(1)
    scale = torch.maximum(amax, torch.tensor(2.0 ** -64)) / 448.0
    q = (xf / scale[:, None]).clamp(-448, 448).to(F8)
    return q, scale


@pytest.mark.parametrize("K", [128, 3840, 16384])
@pytest.mark.parametrize("M", [1, 5, 161])
def test_quant_rows_bit_exact(dev, M, K):
    from mlx_video_amd import ops
    x = _rows(M, K, torch.Generator().manual_seed(M * 31 + K))
    assert bool(torch.isfinite(x.float()).all())
    q_ref, s_ref = _reference(x)
    if M >= 5:                                 # the special rows are what they claim to be
        assert float(x[1].float().abs().max()) == 0.0 and float(x[2].float().abs().max()) == BF16_MAX
        assert float(x[3].float().abs().max()) == 2.0 ** -70 and float(s_ref[4]) == 1.0
        assert int(q_ref[1].view(torch.uint8).max()) == 0
    xin = torch.full((M, K + 24), 9.0, dtype=BF, device=dev)
    xin[:, 8:8 + K] = x.to(dev)
    qbuf = torch.full((M + 1, K + 40), 0xA5, dtype=torch.uint8, device=dev)
    sbuf = torch.full((M + 2,), -7.0, dtype=torch.float32, device=dev)
    q, s = ops.quant_rows_fp8(xin[:, 8:8 + K], out=(qbuf.view(F8)[:M, 16:16 + K], sbuf[1:M + 1]))
    torch.cuda.synchronize()
    assert q.dtype == F8 and s.dtype == torch.float32
    got_s, got_q = sbuf[1:M + 1].cpu(), qbuf[:M, 16:16 + K].cpu()
    bad_s = (got_s.view(torch.int32) != s_ref.view(torch.int32)).nonzero()
    assert bad_s.numel() == 0, f"scale differs in rows {bad_s.flatten().tolist()[:8]}"
    bad = (got_q != q_ref.view(torch.uint8)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} codes differ, first at {bad[0].tolist()}: got {int(got_q[tuple(bad[0])]):#x}, want {int(q_ref.view(torch.uint8)[tuple(bad[0])]):#x}"
    assert bool((qbuf[M] == 0xA5).all()) and bool((qbuf[:, :16] == 0xA5).all()) and bool((qbuf[:, 16 + K:] == 0xA5).all()), "wrote outside the output view"
    assert float(sbuf[0]) == -7.0 and float(sbuf[M + 1]) == -7.0
    # fresh buffers: the same bits
    q2, s2 = ops.quant_rows_fp8(xin[:, 8:8 + K])
    torch.cuda.synchronize()
    assert torch.equal(q2.view(torch.uint8).cpu(), got_q) and torch.equal(s2.cpu(), got_s)
