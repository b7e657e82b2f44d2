"""ltxk_gemv_w8 (``ops.gemm(..., gemv=True)``: M <= 8 rows of bf16 activations over an e4m3 panel, csrc/gemv.hip) against the float64
reference and the element-wise bound of tests/ref_gemm.py.

Reference: float64 on the dequantised panel code * scale, which is exact (a 4-bit by a 24-bit significand).  Bound:
``ref_gemm.bound(EPI_BIAS, out, s, mag, K, bias, acc_err=K * U * mag)`` - the accumulator term tests/test_gemm_w8_gpu.py uses for the
scaled fp8 forms (K - 1 fp32 additions in any order plus the one rounding of the scale multiply), the fp32 bias add, half a
bf16 ulp of what was stored - on EVERY element (``ref_gemm.check``).

Shapes: K below (16, 512, 1008), at (1024) and past (1040) one wave pass of 1024 k and Gemma's own 3840 (a ragged fourth
pass; with M = 8 a second chunk of the A image); N of one row (1), below, at and past one workgroup's 8 rows (7, 8, 257: odd, so
the last wave's second row is clamped) and 1000; M = 1, 2, 3 (padded to 4 row slots), 8 rotated over the cases; every case
with and without ``w_scale`` and ``bias`` in rotation; ``a`` with a row stride of K + 8 and NaN pads, ``out`` inside a NaN frame
with a row stride of N + 5 that must survive.

The kernel's property - the bits of out[m,n] depend on row m of a, row n of w, w_scale[n] and bias[n] alone - is tested
directly: rows of an M = 8 and an M = 3 launch against M = 1 launches, the first 1000 columns of N = 1001 against N = 1000."""
import pytest
import torch

import ref_gemm

gpu = pytest.mark.gpu
BF, F8, F64, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.float64, torch.float32
U = ref_gemm.U
KS = (16, 512, 1008, 1024, 1040, 3840)
NS = (1, 7, 8, 257, 1000)
MS = (1, 2, 3, 8)
CASES = [(K, N, MS[(i + 3 * j) % 4], (i + j) % 4) for i, K in enumerate(KS) for j, N in enumerate(NS)]


def test_cases_cover_the_grid():
    assert {(c[0], c[1]) for c in CASES} == {(K, N) for K in KS for N in NS}
    for K in KS:
        assert {c[2] for c in CASES if c[0] == K} == set(MS) and {c[3] for c in CASES if c[0] == K} == {0, 1, 2, 3}
    for N in NS:
        assert {c[2] for c in CASES if c[1] == N} == set(MS) and {c[3] for c in CASES if c[1] == N} == {0, 1, 2, 3}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _case(M, N, K, seed, scaled):
    """ref_gemm.inputs with its panel as e4m3: per-row scaled codes (quantize_fp8: the row's extreme on +-448, a zero edge row
    scale 1) or, unscaled, the plain cast of 16 w.  The scales get random mantissas so that the fp32 multiply rounds."""
    from mlx_video_amd.weights import quantize_fp8
    inp = ref_gemm.inputs(M, N, K, seed)
    if scaled:
        w8, sc = quantize_fp8(inp.w, "channel")
        g = torch.Generator().manual_seed(seed + 1)
        sc = (sc * (1.0 + 0.5 * torch.rand(N, generator=g))).float().contiguous()
    else:
        w8, sc = (inp.w.float() * 16).to(F8), None
    wd = w8.to(F64) * (sc.to(F64)[:, None] if sc is not None else 1.0)
    s, mag = ref_gemm.product(inp.a, wd)
    assert bool(torch.isfinite(s).all())
    return inp, w8, sc, s, mag


def _check(name, out, s, mag, K, bias):
    d, bnd = ref_gemm.bound(ref_gemm.EPI_BIAS, out, s, mag, K, bias, acc_err=K * U * mag)
    return ref_gemm.check(name, d, bnd)


@gpu
@pytest.mark.parametrize("K,N,M,form", CASES, ids=lambda v: str(v))
def test_gemv_inside_the_bound(dev, K, N, M, form):
    from mlx_video_amd import ops
    scaled, biased = bool(form & 1), bool(form & 2)
    inp, w8, sc, s, mag = _case(M, N, K, 100 + K + N, scaled)
    bias = inp.b if biased else None
    assert inp.a.stride(0) == K + 8 and bool(torch.isnan(inp.a.as_strided((M, 8), (K + 8, 1), K).float()).all())
    fr = ref_gemm.rows_frame(M, N, N + 5, dev)
    got = ops.gemm(_strided(inp.a, dev), w8.to(dev), None if bias is None else bias.to(dev), out=fr.view,
                   w_scale=None if sc is None else sc.to(dev), gemv=True)
    torch.cuda.synchronize()
    assert got is fr.view and fr.intact(), "wrote outside the output view"
    worst = _check(f"gemv M{M} N{N} K{K} scale{scaled} bias{biased}", fr.view.cpu(), s, mag, K, bias)
    print(f"M{M} N{N} K{K} scale {scaled} bias {biased}: worst d / bound {worst:.3f}")
    for c, v in inp.edge:           # an edge column is exact: a zero row of codes, so the output IS the bias (or 0)
        want = float(torch.tensor(v if biased else 0.0).to(BF))
        assert bool((fr.view[:, c].float().cpu() == want).all()), f"edge column {c}"


def _strided(a, dev):
    """``a`` (a view with a row stride of K + 8 and NaN pads) on the device with the same strides."""
    M, K = a.shape
    buf = torch.full((M, a.stride(0)), float("nan"), dtype=BF, device=dev)
    buf[:, :K] = a.to(dev)
    return buf[:, :K]


@gpu
def test_every_finite_code(dev):
    """The panel's bytes run over all 254 finite e4m3 codes - subnormals, +-0, +-448 - each at every byte position of a lane's
    16 (1040 and 254 share no factor with 16 beyond 2, and the row shift moves the phase); and a panel of nothing but the
    smallest subnormal and -0 against ones is exact: nothing is flushed in the widening or the FMAs."""
    from mlx_video_amd import ops
    M, N, K = 3, 257, 1040
    codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
    idx = (torch.arange(N * K) * 3 + torch.arange(N * K) // K) % 254
    w8 = codes[idx].reshape(N, K).view(F8)
    assert torch.unique(w8.view(torch.uint8)).numel() == 254 and bool(torch.isfinite(w8.float()).all())
    for pos in range(16):
        assert torch.unique(w8.view(torch.uint8)[:, pos::16]).numel() == 254
    inp = ref_gemm.inputs(M, N, K, 5)
    a = (inp.a.float() * 2.0 ** -4).to(BF)
    s, mag = ref_gemm.product(a, w8.to(F64))
    got = ops.gemm(a.to(dev), w8.to(dev), None, gemv=True)
    torch.cuda.synchronize()
    _check("every code", got.cpu(), s, mag, K, None)
    tiny = torch.tensor([0x01, 0x80], dtype=torch.uint8).repeat(N * K // 2).reshape(N, K).view(F8)
    x = ops.gemm(torch.ones((M, K), dtype=BF, device=dev), tiny.to(dev), None, gemv=True)
    torch.cuda.synchronize()
    assert bool((x.float() == K // 2 * 2.0 ** -9).all())


@gpu
def test_bits_depend_on_the_row_and_the_column_alone(dev):
    from mlx_video_amd import ops
    K, N = 3840, 1001
    inp, w8, sc, _, _ = _case(8, N, K, 77, True)
    a, w, b, scd = _strided(inp.a, dev), w8.to(dev), inp.b.to(dev), sc.to(dev)
    run = lambda a_, n=N: ops.gemm(a_, w[:n], b[:n], w_scale=scd[:n], gemv=True)
    full = run(a)
    again = run(a)
    torch.cuda.synchronize()
    assert torch.equal(_bits(full), _bits(again)), "two runs differ"
    for m in range(8):             # M = 8 (two chunks of the A image at K = 3840) against M = 1 (one chunk)
        assert torch.equal(_bits(run(a[m:m + 1])[0]), _bits(full[m])), f"row {m} alone gives other bits"
    three = run(a[2:5])            # M = 3 on 4 row slots
    assert torch.equal(_bits(three), _bits(full[2:5]))
    two = run(a[6:8])
    assert torch.equal(_bits(two), _bits(full[6:8]))
    n1000 = run(a, 1000)           # an even N (no clamped row) against the odd one's first 1000 columns
    assert torch.equal(_bits(n1000), _bits(full[:, :1000])), "N changes the bits of a column"
    one = run(a[:1], 1)
    assert torch.equal(_bits(one), _bits(full[:1, :1]))


@gpu
@pytest.mark.parametrize("M", [1, 2])
def test_several_row_sets_per_workgroup(dev, M):
    """Past 8192 rows of a panel whose K fits one chunk of the A image a workgroup keeps the image over 2 .. 8 row sets (N = 20001:
    2501 row sets, 3 per workgroup, the last workgroup's second one partly and its third wholly past N).  Inside the bound, and column for column the bits
    of the launches on the first 1000 rows and on the last 9 (one row set each)."""
    from mlx_video_amd import ops
    K, N = 1040, 20001
    inp, w8, sc, s, mag = _case(M, N, K, 9, True)
    a, w, b, scd = _strided(inp.a, dev), w8.to(dev), inp.b.to(dev), sc.to(dev)
    fr = ref_gemm.rows_frame(M, N, N + 5, dev)
    ops.gemm(a, w, b, out=fr.view, w_scale=scd, gemv=True)
    torch.cuda.synchronize()
    assert fr.intact()
    _check(f"row sets M{M}", fr.view.cpu(), s, mag, K, inp.b)
    head = ops.gemm(a, w[:1000], b[:1000], w_scale=scd[:1000], gemv=True)
    tail = ops.gemm(a, w[N - 9:], b[N - 9:].contiguous(), w_scale=scd[N - 9:].contiguous(), gemv=True)
    assert torch.equal(_bits(head), _bits(fr.view[:, :1000])) and torch.equal(_bits(tail), _bits(fr.view[:, N - 9:]))


# ------------------------------------------------------------------------------------------------ planted faults (CPU)
def _emulate(a, w8, sc, bias, fault=None):
    """The kernel's epilogue on a float64 accumulator: fp32(acc), * w_scale (one fp32 rounding), + bias (one), bf16.  Faults:
    "tail": the last 16 k dropped; "scale": w_scale of column n + 1; "order": the bias added before the scale."""
    K = a.shape[1]
    k = K - 16 if fault == "tail" else K
    acc = (a[:, :k].to(F64) @ w8[:, :k].to(F64).t()).to(F32)
    sc = sc.roll(-1) if fault == "scale" else sc
    bf = bias.to(F32)
    if fault == "order":
        return ((acc + bf) * sc).to(BF)
    return (acc * sc + bf).to(BF)


def test_planted_faults_fall_outside_the_bound():
    M, N, K = 3, 257, 1040
    inp, w8, sc, s, mag = _case(M, N, K, 100 + K + N, True)
    d, bnd = ref_gemm.bound(ref_gemm.EPI_BIAS, _emulate(inp.a, w8, sc, inp.b), s, mag, K, inp.b, acc_err=K * U * mag)
    assert not bool(ref_gemm.beyond(d, bnd).any()), "the emulation itself is outside the bound"
    for fault in ("tail", "scale", "order"):
        d, bnd = ref_gemm.bound(ref_gemm.EPI_BIAS, _emulate(inp.a, w8, sc, inp.b, fault), s, mag, K, inp.b, acc_err=K * U * mag)
        n = int(ref_gemm.beyond(d, bnd).sum())
        print(f"fault {fault}: {n} of {d.numel()} outputs beyond the bound")
        assert n >= 1, f"the bound accepts the fault {fault!r}"


@gpu
def test_refusals(dev):
    from mlx_video_amd import ops
    z = lambda *sh, dt=BF: torch.zeros(sh, dtype=dt, device=dev)
    w8 = torch.zeros((8, 32), dtype=torch.uint8, device=dev).view(F8)
    with pytest.raises(ValueError, match="`a`"):
        ops.gemm(z(9, 32), w8, None, gemv=True)
    with pytest.raises(ValueError, match="K"):
        ops.gemm(z(1, 24), torch.zeros((8, 24), dtype=torch.uint8, device=dev).view(F8), None, gemv=True)
    with pytest.raises(ValueError, match="epilogue"):
        ops.gemm(z(1, 32), w8, None, epilogue=1, gemv=True)
    with pytest.raises(TypeError, match="`w`"):
        ops.gemm(z(1, 32), z(8, 32), None, gemv=True)
    out = ops.gemm(z(1, 32), w8, None, gemv=True)          # and the call they were mutations of runs
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 8) and bool((out == 0).all())
