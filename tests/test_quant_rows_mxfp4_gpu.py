"""ltxk_quant_rows_mxfp4 against its definition, weights.quantize_mxfp4: the code bytes and the scale bytes are EQUAL, on data
with every rounding case planted - each e2m1 midpoint times the block's scale in both signs (ties go to the even index), a block
whose amax is 7 x 2^e (saturates to 6), an all-zero block, -0, bf16 subnormals (the scale byte clamps at 0), the largest finite
bf16, a block with a single non-zero element - and nothing is written outside the output views."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U8 = torch.uint8
MIDS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def _specials():
    """The planted blocks (32 float64 values each)."""
    out = []
    for e in (0, -9, 17, -126, -124, 100):               # block scale 2^e: amax in [4, 8) * 2^e
        b = torch.zeros(32, dtype=torch.float64)
        b[:7] = torch.tensor(MIDS, dtype=torch.float64)
        b[7:14] = -torch.tensor(MIDS, dtype=torch.float64)
        b[14], b[15] = 4.0, -6.0                         # amax 6: the scale is 2^e, so the midpoints are exact ties
        out.append(b * 2.0 ** e)
        b7 = torch.zeros(32, dtype=torch.float64)
        b7[3], b7[4], b7[9] = 7.0, -7.0, 5.0             # amax 7 x 2^e: saturates to 6; 5.0 is a tie (-> 4)
        out.append(b7 * 2.0 ** e)
    z = torch.zeros(32, dtype=torch.float64)
    out.append(z.clone())                                # all-zero block
    nz = z.clone(); nz[1::2] = -0.0
    out.append(nz)                                       # zeros of both signs
    nz2 = z.clone(); nz2[5] = -0.0; nz2[6] = 3.0
    out.append(nz2)                                      # -0 beside a value
    sub = z.clone(); sub[:8] = torch.arange(1, 9, dtype=torch.float64) * 2.0 ** -133; sub[8] = -127 * 2.0 ** -133
    out.append(sub)                                      # bf16 subnormals only: the scale byte clamps at 0
    sub2 = z.clone(); sub2[0] = 2.0 ** -124
    sub2[1:9] = torch.tensor([127, 96, 95, 64, 33, 32, 31, 1], dtype=torch.float64) * 2.0 ** -133
    out.append(sub2)                                     # subnormal elements under a small normal amax (scale byte 1)
    big = z.clone(); big[0], big[1], big[2], big[3] = 3.3895313892515355e38, -3.3895313892515355e38, 2.0 ** 126, 1.5 * 2.0 ** 125
    out.append(big)                                      # the largest finite bf16: scale byte 252
    one = z.clone(); one[17] = -0.3
    out.append(one)                                      # a single non-zero element
    return out


def _planted(M, K, seed, first=0):
    """(M, K) bf16 on the CPU: random blocks over many binades, the special blocks (from number ``first`` on, cyclically) spread
    over the matrix's blocks - all of them where it has that many."""
    g = torch.Generator().manual_seed(seed)
    nb = M * (K // 32)
    blocks = torch.randn((nb, 32), generator=g) * torch.exp2(torch.randint(-20, 20, (nb, 1), generator=g).float())
    sp = _specials()
    step = max(1, nb // len(sp))
    for j in range(min(nb, len(sp))):
        blocks[j * step] = sp[(first + j) % len(sp)].float()
    return blocks.view(M, K).to(BF)


# (1, 32) is a single block: every special one in turn; (5, 96) has 15: two passes plant all of them
@pytest.mark.parametrize("M,K,pad,passes", [(1, 32, 0, len(_specials())), (5, 96, 40, 2), (33, 2304, 0, 1)])
def test_quant_rows_mxfp4_equals_quantize_mxfp4(dev, M, K, pad, passes):
    from mlx_video_amd import ops
    from mlx_video_amd.weights import quantize_mxfp4
    nb = M * (K // 32)
    for i in range(passes):
        x = _planted(M, K, 31 + i, first=i * nb)
        want_c, want_s = quantize_mxfp4(x)
        xb = torch.full((M, K + pad), float("nan"), dtype=BF, device=dev)
        xb[:, :K] = x.to(dev)
        qb = torch.full((M + 1, K // 2 + 16), 0xA5, dtype=U8, device=dev)
        sb = torch.full((M + 1, K // 32 + 8), 0xA5, dtype=U8, device=dev)
        q, s = ops.quant_rows_mxfp4(xb[:, :K], out=(qb[:M, :K // 2], sb[:M, :K // 32]))
        torch.cuda.synchronize()
        assert bool((qb[M:] == 0xA5).all()) and bool((qb[:, K // 2:] == 0xA5).all()), "codes: wrote outside the output view"
        assert bool((sb[M:] == 0xA5).all()) and bool((sb[:, K // 32:] == 0xA5).all()), "scales: wrote outside the output view"
        assert not bool((s == 255).any())
        bad = (s.cpu() != want_s).nonzero()
        assert bad.numel() == 0, f"pass {i}: scale bytes differ, first at {bad[0].tolist()}"
        bad = (q.cpu() != want_c).nonzero()
        assert bad.numel() == 0, f"pass {i}: {bad.shape[0]} code bytes differ, first at {bad[0].tolist()}"
    q2, s2 = ops.quant_rows_mxfp4(x.to(dev))             # the allocating form
    torch.cuda.synchronize()
    assert torch.equal(q2.cpu(), want_c) and torch.equal(s2.cpu(), want_s)


def test_quant_rows_mxfp4_rows_are_independent(dev):
    """A row's bits depend on that row only: row 7 of a 33-row launch equals the 1-row launch on it."""
    from mlx_video_amd import ops
    x = _planted(33, 2304, 5).to(dev)
    q, s = ops.quant_rows_mxfp4(x)
    q1, s1 = ops.quant_rows_mxfp4(x[7:8])
    torch.cuda.synchronize()
    assert torch.equal(q[7:8], q1) and torch.equal(s[7:8], s1)
