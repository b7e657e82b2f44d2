"""ltxk_gemv_w4 (``ops.gemv_w4``: M <= 8 rows of bf16 activations over an OCP MXFP4 panel, csrc/gemv4.hip) against the float64
reference and the element-wise bound of tests/ref_gemm.py, in the shape of tests/test_gemv_w8_gpu.py.

Reference: float64 on the dequantised panel e2m1(code) * 2^(E-127), which is exact.  Bound:
``ref_gemm.bound(EPI_BIAS, out, s, mag, K, bias, acc_err=K * U * mag)`` on EVERY element (``ref_gemm.check``);
tests/test_mxfp4_cpu.py shows that it accepts the kernel's stated order and refuses planted faults.

Shapes: K below (32, 992), at (2048) and past (2080) one wave pass of 2048 k, Gemma's own 3840 (a ragged second pass) and 6176
(a ragged fourth pass; with M = 8 four chunks of the A image, with M = 3 two); N of one row (1), below, at and past one
workgroup's 8 rows (7, 8, 257: odd, so the last wave's second row is clamped) and 1000; M = 1, 2, 3 (padded to 4 row slots), 8
rotated over the cases; every case with and without ``bias`` in rotation; ``a`` with a row stride of K + 8 and NaN pads, ``out``
inside a NaN frame with a row stride of N + 5 that must survive.

Long rows: K = 15360, Gemma's down projection and the one shipped shape whose row is longer than the ring (7.5 passes against 4
slots: at M = 1 the slots are refilled inside one chunk of the A image; at M = 2 the row is two chunks of 4 passes, at M = 3 .. 4
four of 2, at M = 8 eight of 1, the ring requested again at every chunk boundary), at M = 1, 2, 4 inside the bound and, bit
for bit, M = 8, 3 and 2 rows against M = 1.

The kernel's property - the bits of out[m,n] depend on row m of a, row n of the panel, its scale row and bias[n] alone - is
tested directly: rows of an M = 8 and an M = 3 launch against M = 1 launches, the first 1000 columns of N = 1001 against N = 1000."""
import pytest
import torch

import ref_gemm
from test_gemv_w8_gpu import _bits, _strided
from test_mxfp4_cpu import panel

gpu = pytest.mark.gpu
BF, F64, U8 = torch.bfloat16, torch.float64, torch.uint8
U = ref_gemm.U
KS = (32, 992, 2048, 2080, 3840, 4096 + 2048 + 32)
NS = (1, 7, 8, 257, 1000)
MS = (1, 2, 3, 8)
CASES = [(K, N, MS[(i + 3 * j) % 4], (i + j) % 2) for i, K in enumerate(KS) for j, N in enumerate(NS)]


def test_cases_cover_the_grid():
    assert max(KS) <= 16384 and {(c[0], c[1]) for c in CASES} == {(K, N) for K in KS for N in NS}
    for K in KS:
        assert {c[2] for c in CASES if c[0] == K} == set(MS) and {c[3] for c in CASES if c[0] == K} == {0, 1}
    for N in NS:
        assert {c[2] for c in CASES if c[1] == N} == set(MS) and {c[3] for c in CASES if c[1] == N} == {0, 1}


def _check(name, out, s, mag, K, bias):
    d, bnd = ref_gemm.bound(ref_gemm.EPI_BIAS, out, s, mag, K, bias, acc_err=K * U * mag)
    return ref_gemm.check(name, d, bnd)


@gpu
@pytest.mark.parametrize("K,N,M,biased", CASES, ids=lambda v: str(v))
def test_gemv_inside_the_bound(dev, K, N, M, biased):
    from mlx_video_amd import ops
    inp, codes, sc, s, mag = panel(M, N, K, 100 + K + N)
    bias = inp.b if biased else None
    assert inp.a.stride(0) == K + 8 and bool(torch.isnan(inp.a.as_strided((M, 8), (K + 8, 1), K).float()).all())
    fr = ref_gemm.rows_frame(M, N, N + 5, dev)
    got = ops.gemv_w4(_strided(inp.a, dev), codes.to(dev), sc.to(dev), None if bias is None else bias.to(dev), out=fr.view)
    torch.cuda.synchronize()
    assert got is fr.view and fr.intact(), "wrote outside the output view"
    worst = _check(f"gemv_w4 M{M} N{N} K{K} bias{biased}", fr.view.cpu(), s, mag, K, bias)
    print(f"M{M} N{N} K{K} bias {biased}: worst d / bound {worst:.3f}")
    for c, v in inp.edge:           # an edge column is exact: a zero row of codes, so the output IS the bias (or 0)
        want = float(torch.tensor(v if biased else 0.0).to(BF))
        assert bool((fr.view[:, c].float().cpu() == want).all()), f"edge column {c}"


@gpu
@pytest.mark.parametrize("M,biased", [(1, 1), (2, 0), (4, 1)])
def test_long_rows_refill_the_ring(dev, M, biased):
    """K = 15360 (7.5 passes; the module docstring says which path each M takes), N = 263: odd, 33 row sets."""
    from mlx_video_amd import ops
    K, N = 15360, 263
    inp, codes, sc, s, mag = panel(M, N, K, 400 + M)
    bias = inp.b if biased else None
    fr = ref_gemm.rows_frame(M, N, N + 5, dev)
    ops.gemv_w4(_strided(inp.a, dev), codes.to(dev), sc.to(dev), None if bias is None else bias.to(dev), out=fr.view)
    torch.cuda.synchronize()
    assert fr.intact(), "wrote outside the output view"
    worst = _check(f"gemv_w4 long rows M{M}", fr.view.cpu(), s, mag, K, bias)
    print(f"M{M} N{N} K{K} bias {biased}: worst d / bound {worst:.3f}")
    for c, v in inp.edge:
        want = float(torch.tensor(v if biased else 0.0).to(BF))
        assert bool((fr.view[:, c].float().cpu() == want).all()), f"edge column {c}"


@gpu
def test_smallest_scale_bytes(dev):
    """Scale bytes 0 and 1 (2^-127, a subnormal fp32 operand, and 2^-126; the quantiser writes byte 0 for a block whose amax is
    below 2^-124) against activations of 2^100 .. 2^103, so that the outputs are ordinary numbers: inside the bound against
    dequantize_mxfp4 - neither the scale nor a widened subnormal (0.5 x 2^-127) is flushed - and a panel of +0.5 alone is exact."""
    from mlx_video_amd import ops
    from mlx_video_amd.weights import dequantize_mxfp4
    M, N, K = 2, 16, 128
    g = torch.Generator().manual_seed(12)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=U8)
    sc = torch.tensor([0, 1, 1, 0], dtype=U8).repeat(N, 1)
    a = (torch.randn((M, K), generator=g) * 2.0 ** 101).to(BF)
    s, mag = ref_gemm.product(a, dequantize_mxfp4(codes, sc, F64))
    assert float(s.abs().max()) > 2.0 ** -40
    got = ops.gemv_w4(a.to(dev), codes.to(dev), sc.to(dev))
    torch.cuda.synchronize()
    worst = _check("scale bytes 0 and 1", got.cpu(), s, mag, K, None)
    print(f"scale bytes 0 and 1: worst d / bound {worst:.3f}")
    half = torch.full((N, K // 2), 0x11, dtype=U8)
    x = ops.gemv_w4(torch.full((M, K), 2.0 ** 100, dtype=BF, device=dev), half.to(dev), sc.to(dev))
    torch.cuda.synchronize()
    assert bool((x.float() == (64 * 2.0 ** -128 + 64 * 2.0 ** -127) * 2.0 ** 100).all())


@gpu
def test_every_code(dev):
    """The panel's bytes run over all 256 code pairs, each at every byte position of a lane's 16, and the block scale bytes over
    127 +- 20; and a panel of nothing but +0.5 (low nibble) and -0 (high nibble) at scale byte 117 against ones is exact: nothing
    is flushed in the widening or the FMAs, and -0 contributes nothing."""
    from mlx_video_amd import ops
    from mlx_video_amd.weights import dequantize_mxfp4
    M, N, K = 3, 257, 2080
    Kb, Ks = K // 2, K // 32
    idx = torch.arange(N * Kb)
    codes = ((idx * 3 + idx // Kb) % 256).to(U8).reshape(N, Kb)
    assert torch.unique(codes).numel() == 256
    for pos in range(16):
        assert torch.unique(codes[:, pos::16]).numel() == 256
    sc = (107 + (torch.arange(N * Ks) * 7) % 41).to(U8).reshape(N, Ks)
    assert int(sc.min()) == 107 and int(sc.max()) == 147 and torch.unique(sc).numel() == 41
    inp = ref_gemm.inputs(M, N, K, 5)
    a = (inp.a.float() * 2.0 ** -4).to(BF)
    s, mag = ref_gemm.product(a, dequantize_mxfp4(codes, sc, F64))
    got = ops.gemv_w4(a.to(dev), codes.to(dev), sc.to(dev))
    torch.cuda.synchronize()
    worst = _check("every code", got.cpu(), s, mag, K, None)
    print(f"every code: worst d / bound {worst:.3f}")
    tiny = torch.full((N, Kb), 0x81, dtype=U8)
    x = ops.gemv_w4(torch.ones((M, K), dtype=BF, device=dev), tiny.to(dev), torch.full((N, Ks), 117, dtype=U8, device=dev))
    torch.cuda.synchronize()
    assert bool((x.float() == K // 2 * 0.5 * 2.0 ** -10).all()) and not bool(torch.signbit(x.float()).any())


@gpu
@pytest.mark.parametrize("K,N", [(3840, 1001), (15360, 265)])
def test_bits_depend_on_the_row_and_the_column_alone(dev, K, N):
    """K = 15360: the M = 1 launches run the one-chunk ring with refills, the M = 8, 3 and 2 launches reload it at 8, 4 and 2
    chunk boundaries."""
    from mlx_video_amd import ops
    inp, codes, sc, _, _ = panel(8, N, K, 77)
    a, w, scd, b = _strided(inp.a, dev), codes.to(dev), sc.to(dev), inp.b.to(dev)
    run = lambda a_, n=N: ops.gemv_w4(a_, w[:n], scd[:n], b[:n])          # noqa: E731
    full = run(a)
    again = run(a)
    torch.cuda.synchronize()
    assert torch.equal(_bits(full), _bits(again)), "two runs differ"
    for m in range(8):             # M = 8 (one pass per chunk of the A image) against M = 1 (one chunk)
        assert torch.equal(_bits(run(a[m:m + 1])[0]), _bits(full[m])), f"row {m} alone gives other bits"
    three = run(a[2:5])            # M = 3 on 4 row slots
    assert torch.equal(_bits(three), _bits(full[2:5]))
    two = run(a[6:8])
    assert torch.equal(_bits(two), _bits(full[6:8]))
    n1000 = run(a, N - 1)          # an even N (no clamped row) against the odd one's first N - 1 columns
    assert torch.equal(_bits(n1000), _bits(full[:, :N - 1])), "N changes the bits of a column"
    one = run(a[:1], 1)
    assert torch.equal(_bits(one), _bits(full[:1, :1]))


@gpu
@pytest.mark.parametrize("M", [1, 2])
def test_several_row_sets_per_workgroup(dev, M):
    """Past one round of resident workgroups (1024 row sets of 8 rows at M = 1, 768 at M = 2) of a panel whose K fits one chunk of
    the A image a workgroup keeps the image over 2 .. 8 row sets (N = 20001: 2501 row sets, 3 per workgroup at M = 1 and 4 at
    M = 2, the last workgroup's last ones partly and wholly past N).  Inside the bound, and column for column the bits of the
    launches on the first 1000 rows and on the last 9 (one row set each)."""
    from mlx_video_amd import ops
    K, N = 2080, 20001
    inp, codes, sc, s, mag = panel(M, N, K, 9)
    a, w, scd, b = _strided(inp.a, dev), codes.to(dev), sc.to(dev), inp.b.to(dev)
    fr = ref_gemm.rows_frame(M, N, N + 5, dev)
    ops.gemv_w4(a, w, scd, b, out=fr.view)
    torch.cuda.synchronize()
    assert fr.intact()
    _check(f"row sets M{M}", fr.view.cpu(), s, mag, K, inp.b)
    head = ops.gemv_w4(a, w[:1000], scd[:1000], b[:1000])
    tail = ops.gemv_w4(a, w[N - 9:].clone(), scd[N - 9:].clone(), b[N - 9:].clone())
    assert torch.equal(_bits(head), _bits(fr.view[:, :1000])) and torch.equal(_bits(tail), _bits(fr.view[:, N - 9:]))


@gpu
def test_refusals(dev):
    from mlx_video_amd import ops
    z = lambda *sh, dt=BF: torch.zeros(sh, dtype=dt, device=dev)          # noqa: E731
    codes, sc = z(8, 32, dt=U8), torch.full((8, 2), 127, dtype=U8, device=dev)
    with pytest.raises(ValueError, match="`a`"):
        ops.gemv_w4(z(9, 64), codes, sc)
    with pytest.raises(ValueError, match="K"):
        ops.gemv_w4(z(1, 48), z(8, 24, dt=U8), z(8, 1, dt=U8))
    with pytest.raises(TypeError, match="codes"):
        ops.gemv_w4(z(1, 64), codes.view(torch.float8_e4m3fn), sc)
    with pytest.raises(TypeError, match="codes"):
        ops.gemv_w4(z(1, 64), z(8, 32), sc)
    with pytest.raises(ValueError, match="block_scales"):
        ops.gemv_w4(z(1, 64), codes, z(8, 4, dt=U8))
    out = ops.gemv_w4(z(1, 64), codes, sc)          # and the call they were mutations of runs
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 8) and bool((out == 0).all())
