"""ltxk_gemm_w8a8 (e4m3 activations x e4m3 weights on v_mfma_scale_f32_16x16x128_f8f6f4).

1. Exact integer data.  A and W hold e4m3 codes of the integers -4..4, A[m][k] and W[n][k] set by different linear forms mod 9
   (asymmetric under m <-> n, and under any permutation of k inside a 128-wide K-step that is not applied to both operands),
   all scales 1.  Every partial sum is an integer below 2^24, so the accumulator is exact in any order: the plain output is the
   float64 product rounded once to bf16, and every epilogue / output form must give the BITS ltxk_gemm_bf16 gives on the same
   integers as bf16 (its sums are exact too, and the epilogue code is shared).  This pins the lane maps and the A/W k assignment.
2. Random data against float64 under the element-wise bound of tests/test_gemm_w8_gpu.py (its helpers are tests/ref_gemm.py's): half a bf16
   ulp of the output + K * 2^-24 * sum|a_k w_k| * a_scale * w_scale for the fp32 accumulation in any order + two more fp32
   roundings for the two scale multiplies + the fp32 bias add.  Nothing is added to that bound; the worst ratio is printed.
3. Argument errors.   4. quant_rows_fp8 -> gemm composition against the float64 product of the restated quantised operands."""
import ctypes

import pytest
import torch

import ref_gemm

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
F64 = torch.float64
U = 2.0 ** -24


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same(name, x, y):
    assert torch.equal(_bits(x), _bits(y)), (f"{name}: {int((_bits(x) != _bits(y)).sum())} of {x.numel()} elements differ, "
                                             f"first at {tuple(int(i) for i in (_bits(x) != _bits(y)).nonzero()[0])}")


def _int_operands(M, N, K, dev):
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :]
    a = ((3 * m + 5 * k + k // 128) % 9 - 4).float()
    w = ((7 * n + 2 * k + 1) % 9 - 4).float()
    lda = K + 64
    abuf = torch.zeros((M, lda), dtype=BF, device=dev)
    abuf[:, :K] = a.to(dev).to(BF)
    a8buf = torch.zeros((M, lda), dtype=torch.uint8, device=dev).view(F8)
    a8buf[:, :K] = a.to(dev).to(F8)
    assert torch.equal(a8buf[:, :K].float().cpu(), a) and torch.equal(w.to(F8).float(), w)
    return a, w, abuf[:, :K], a8buf[:, :K], w.to(dev).to(F8)


def _epi_operands(M, N, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    b = (torch.randn(N, generator=g, device=dev) * 0.1).to(BF)
    res = torch.randn((M, N), generator=g, device=dev).to(BF)
    gate = torch.randn((3, N), generator=g, device=dev).to(BF)
    grow = torch.randint(0, 3, (M,), generator=g, device=dev, dtype=torch.int32)
    return g, b, res, gate, grow


def _run_all(ops, a, w, b, res, gate, grow, *, sumsq, extra, epilogues=range(6)):
    """Every epilogue (with and without bias, gate rows on and off) and the transposed output.  `extra`: the keyword arguments
    that tell the forms apart (a_scale / w_scale).  Returns name -> (buffer incl. sentinels, sumsq buffer or None)."""
    M, K = a.shape
    N = w.shape[0]
    dev = a.device
    out = {}
    for epi in epilogues:
        for bias in (b, None):
            for gr in ((grow, None) if epi == ops.EPI_BIAS_GATE_RES else (None,)):
                kw = dict(epilogue=epi, split_k=False, **extra)
                if epi in (3, 4, 5):
                    kw["resid"] = res
                if epi == 3:
                    kw.update(gate=gate, gate_row=gr, gate_stride=N)
                if epi == 5:
                    kw["alpha"] = 0.8
                for ss_on in ((True, False) if sumsq else (False,)):
                    buf = torch.full((M + 1, N + 8), 7.0, device=dev, dtype=BF)
                    ss = torch.full((M, N // 64 + 1), -1.0, device=dev, dtype=torch.float32) if ss_on else None
                    ops.gemm(a, w, bias, out=buf[:M, :N], sumsq=ss[:, :N // 64] if ss_on else None, **kw)
                    out[f"epi{epi}.bias{bias is not None}.row{gr is not None}.ss{ss_on}"] = (buf, ss)
    T = M // 2 if M % 2 == 0 else M
    ld = (T // 4 + 2) * 4
    vt = torch.full((M // T, N, ld), 3.0, device=dev, dtype=BF)
    ops.gemm(a, w, b, out=vt[:, :, :T], out_tokens_per_batch=T, split_k=False, **extra)
    out["vt"] = (vt, None)
    torch.cuda.synchronize()
    return out


def _split_output(ops, a, w, b, T, ns, *, sumsq, extra):
    M, N = a.shape[0], w.shape[0]
    ld = (T // 4 + 2) * 4
    k2 = torch.full((M + 1, ns + 64), 7.0, device=a.device, dtype=BF)
    v2 = torch.full((M // T, N - ns, ld), 3.0, device=a.device, dtype=BF)
    ss = torch.full((M, ns // 64 + 1), -1.0, device=a.device, dtype=torch.float32) if sumsq else None
    ops.gemm(a, w, b, out=k2[:M, :ns], out2=v2[:, :, :T], n_split=ns, out_tokens_per_batch=T,
             sumsq=ss[:, :ns // 64] if sumsq else None, split_k=False, **extra)
    torch.cuda.synchronize()
    return {"split.k": (k2, ss), "split.vt": (v2, None)}


def _compare(got, ref):
    assert got.keys() == ref.keys()
    for name in got:
        for x, y in zip(got[name], ref[name]):
            if x is not None:
                _same(name, x, y)


def _ones(n, dev):
    return torch.ones(n, dtype=torch.float32, device=dev)


# every tile height of the 160-row family and a second row tile with one row; N below one 128-column tile, one tile + 8, two
# tiles + 8 (the 256-column tile's edge); K = one K-step, and five (wraps the three-stage ring, past the peeled steps)
@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("N", [8, 136, 264])
@pytest.mark.parametrize("M", [1, 33, 160, 161])
def test_w8a8_exact_integers(dev, M, N, K):
    from mlx_video_amd import _lib, ops
    pl = ops.gemm_plan(M, N, K, lda=K + 64, w8a8=True)
    assert pl.form == _lib.GEMM_FORM_SINGLE and pl.ksteps == K // 128
    a, w, ab, a8, w8 = _int_operands(M, N, K, dev)
    # the plain product: float64, rounded once to bf16 (|sum| <= 16 K < 2^24: the fp32 accumulator is exact in any order)
    want = (a.double() @ w.double().t()).to(BF)
    buf = torch.full((M + 1, N + 8), 7.0, device=dev, dtype=BF)
    ops.gemm(a8, w8, None, out=buf[:M, :N], a_scale=_ones(M, dev))
    torch.cuda.synchronize()
    _same("plain product against float64", buf[:M, :N].cpu(), want)
    assert bool((buf[M:] == 7.0).all()) and bool((buf[:, N:] == 7.0).all()), "wrote outside the output view"
    g, b, res, gate, grow = _epi_operands(M, N, dev, M * 7 + N + K)
    for ws in (None, _ones(N, dev)):                       # no w_scale: no multiply; a scale of 1.0: the same bits
        got = _run_all(ops, a8, w8, b, res, gate, grow, sumsq=False, extra=dict(a_scale=_ones(M, dev), w_scale=ws))
        ref = _run_all(ops, ab, w8.to(BF), b, res, gate, grow, sumsq=False, extra={})
        _compare(got, ref)


# the row statistic (N % 64 == 0) on the 128-column tile (two waves share a 64-column block) and on the 256-column one
@pytest.mark.parametrize("M,N,K", [(161, 192, 640), (33, 512, 128), (160, 1024, 640)])
def test_w8a8_exact_integers_sumsq(dev, M, N, K):
    from mlx_video_amd import ops
    a, w, ab, a8, w8 = _int_operands(M, N, K, dev)
    g, b, res, gate, grow = _epi_operands(M, N, dev, M + N + K)
    got = _run_all(ops, a8, w8, b, res, gate, grow, sumsq=True, extra=dict(a_scale=_ones(M, dev)), epilogues=(0, 3, 4))
    ref = _run_all(ops, ab, w8.to(BF), b, res, gate, grow, sumsq=True, extra={}, epilogues=(0, 3, 4))
    _compare(got, ref)


@pytest.mark.parametrize("sumsq", [True, False])
@pytest.mark.parametrize("M,T", [(80, 40), (161, 161)])
def test_w8a8_exact_integers_split_output(dev, M, T, sumsq):
    """q|k row-major and V^T from one launch: N = 512, n_split = 256."""
    from mlx_video_amd import ops
    N, K, ns = 512, 640, 256
    a, w, ab, a8, w8 = _int_operands(M, N, K, dev)
    g, b, *_ = _epi_operands(M, N, dev, 11)
    _compare(_split_output(ops, a8, w8, b, T, ns, sumsq=sumsq, extra=dict(a_scale=_ones(M, dev))),
             _split_output(ops, ab, w8.to(BF), b, T, ns, sumsq=sumsq, extra={}))


_ulp = ref_gemm.ulp          # (the bound's helpers: tests/ref_gemm.py)


WORST = {}


def _bound_check(name, got, ref, bound):
    d = (got.to(F64) - ref).abs()
    ratio = ref_gemm.worst(d, bound)
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{name}: worst |error| / bound = {ratio:.3f}")
    bad = ref_gemm.beyond(d, bound)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} outputs beyond the rounding bound (worst ratio {ratio:.3f}), worst excess "
                                 f"{float((d - bound).max()):.3e} at {tuple(int(i) for i in bad.nonzero()[0])}")


def _scales(n, g, dev):
    """2^-8 ... 2^4 with random mantissas (so the fp32 multiply rounds), the two ends included."""
    expo = torch.linspace(-8.0, 4.0, n, device=dev)[torch.randperm(n, generator=g, device=dev)]
    s = (torch.exp2(expo) * (1.0 + 0.5 * torch.rand(n, generator=g, device=dev))).float().clamp(2.0 ** -8, 2.0 ** 4)
    s[0], s[-1] = 2.0 ** -8, 2.0 ** 4
    return s


def _check_against_float64(ops, tag, a8, a_scale, w8, w_scale, b, M, N, K):
    dev = a8.device
    ad = a8.to(F64) * a_scale.to(F64)[:, None]
    wd = w8.to(F64) * w_scale.to(F64)[:, None]
    s = ad @ wd.t()
    mag = ad.abs() @ wd.abs().t()
    acc_err = (K + 2) * U * mag                  # K - 1 fp32 additions in any order, and the two scale multiplies
    y = s + b.to(F64)
    ey = acc_err + U * (y.abs() + acc_err)       # the fp32 bias add
    extra = dict(a_scale=a_scale, w_scale=w_scale)
    T = M // 2 if M % 2 == 0 else M
    for bias in (b, None):
        buf = torch.full((M + 1, N + 8), 7.0, device=dev, dtype=BF)
        ops.gemm(a8, w8, bias, out=buf[:M, :N], **extra)
        torch.cuda.synchronize()
        assert bool((buf[M:] == 7.0).all()) and bool((buf[:, N:] == 7.0).all()), "wrote outside the output view"
        out = buf[:M, :N]
        if bias is None:
            _bound_check(f"{tag}.nobias", out, s, 0.5 * _ulp(out.to(F64)) + acc_err)
        else:
            _bound_check(f"{tag}.bias", out, y, 0.5 * _ulp(out.to(F64)) + ey)
    ld = (T // 4 + 2) * 4
    vt = torch.full((M // T, N, ld), 3.0, device=dev, dtype=BF)
    ops.gemm(a8, w8, b, out=vt[:, :, :T], out_tokens_per_batch=T, **extra)
    torch.cuda.synchronize()
    assert bool((vt[:, :, T:] == 3.0).all()), "vt: wrote into the pad columns"
    rows = vt[:, :, :T].permute(0, 2, 1).reshape(M, N)
    _bound_check(f"{tag}.vt", rows, y, 0.5 * _ulp(rows.to(F64)) + ey)
    if N % 256 == 0 and N > 256:
        sp = _split_output(ops, a8, w8, b, T, 256, sumsq=True, extra=extra)
        k = sp["split.k"][0][:M, :256]
        _bound_check(f"{tag}.split.k", k, y[:, :256], 0.5 * _ulp(k.to(F64)) + ey[:, :256])
        v = sp["split.vt"][0][:, :, :T].permute(0, 2, 1).reshape(M, N - 256)
        _bound_check(f"{tag}.split.vt", v, y[:, 256:], 0.5 * _ulp(v.to(F64)) + ey[:, 256:])
        sq64 = k.to(F64).pow(2).reshape(M, -1, 64).sum(-1)
        _bound_check(f"{tag}.split.sumsq", sp["split.k"][1][:, :-1], sq64, 64 * U * sq64 + 1e-30)


@pytest.mark.parametrize("M,N,K", [(33, 136, 640), (161, 264, 640), (160, 1024, 2176)])
def test_w8a8_random_against_float64(dev, M, N, K):
    from mlx_video_amd import ops
    g = torch.Generator(device=dev).manual_seed(M * 3 + N)
    lda = K + 64
    a8 = (torch.randn((M, lda), generator=g, device=dev) * 8).to(F8)[:, :K]            # strided A, most of the e4m3 range
    w8 = (torch.randn((N, K), generator=g, device=dev) * K ** -0.5 * 4).to(F8)
    b = (torch.randn(N, generator=g, device=dev) * 0.1).to(BF)
    _check_against_float64(ops, f"random{M}x{N}x{K}", a8, _scales(M, g, dev), w8, _scales(N, g, dev), b, M, N, K)


def test_w8a8_argument_errors(dev):
    from mlx_video_amd import _lib, ops
    lib = _lib.load()

    def args(**over):
        a = _lib.GemmArgs()
        a.A = a.W = a.out = 1 << 12
        a.M, a.N, a.K, a.lda, a.ldo = 64, 1024, 2176, 2176, 1024
        for k, v in over.items():
            setattr(a, k, v)
        return a

    sc = ctypes.c_void_p(1 << 12)
    pl = _lib.GemmPlan()
    assert lib.ltxk_gemm_w8a8_plan(ctypes.byref(args()), ctypes.byref(pl)) == 0 and pl.form == _lib.GEMM_FORM_SINGLE and pl.ksteps == 17
    for over in (dict(K=2112, lda=2112), dict(lda=2176 + 8), dict(A=(1 << 12) + 8), dict(N=12), dict(epilogue=9)):
        a = args(**over)
        assert lib.ltxk_gemm_w8a8_plan(ctypes.byref(a), ctypes.byref(pl)) == -1, over
        assert lib.ltxk_gemm_w8a8(ctypes.byref(a), sc, None, None) == -1, over            # refused before anything is launched
    assert lib.ltxk_gemm_w8a8(ctypes.byref(args()), None, None, None) == -1 and b"a_scale" in lib.ltxk_last_error()
    assert lib.ltxk_gemm_w8a8(ctypes.byref(args()), ctypes.c_void_p((1 << 12) + 2), None, None) == -1
    a8 = torch.zeros((4, 128), dtype=torch.uint8, device=dev).view(F8)
    w8 = torch.zeros((8, 128), dtype=torch.uint8, device=dev).view(F8)
    with pytest.raises(TypeError, match="a_scale"):
        ops.gemm(a8, w8, None)
    with pytest.raises(TypeError, match="a_scale"):
        ops.gemm(a8.to(BF), w8, None, a_scale=_ones(4, dev))
    with pytest.raises(TypeError, match="float8_e4m3fn weight"):
        ops.gemm(a8, w8.to(BF), None, a_scale=_ones(4, dev))
    with pytest.raises(_lib.LtxkError):                     # K = 192 is no multiple of 128: LTXK_EINVAL through the binding
        ops.gemm(torch.zeros((4, 192), dtype=torch.uint8, device=dev).view(F8), torch.zeros((8, 192), dtype=torch.uint8, device=dev).view(F8),
                 None, a_scale=_ones(4, dev))


@pytest.mark.parametrize("M,N,K", [(161, 264, 640), (160, 1024, 2176)])
def test_quant_then_gemm_composition(dev, M, N, K):
    """ops.gemm(*ops.quant_rows_fp8(a), w8, ...) against the float64 product of the quantised operands restated on the CPU."""
    from mlx_video_amd import ops
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    a = (torch.randn((M, K), generator=g, device=dev) * torch.exp2(torch.randint(-6, 6, (M, 1), generator=g, device=dev).float())).to(BF)
    w8 = (torch.randn((N, K), generator=g, device=dev) * K ** -0.5 * 4).to(F8)
    ws = _scales(N, g, dev)
    b = (torch.randn(N, generator=g, device=dev) * 0.1).to(BF)
    af = a.float().cpu()
    sc = torch.maximum(af.abs().amax(1), torch.tensor(2.0 ** -64)) / 448.0
    q_ref = (af / sc[:, None]).clamp(-448, 448).to(F8)
    q, s = ops.quant_rows_fp8(a)
    out = ops.gemm(q, w8, b, a_scale=s, w_scale=ws)
    torch.cuda.synchronize()
    ad = q_ref.to(F64).to(dev) * sc.to(F64).to(dev)[:, None]
    wd = w8.to(F64) * ws.to(F64)[:, None]
    y = ad @ wd.t() + b.to(F64)
    acc_err = (K + 2) * U * (ad.abs() @ wd.abs().t())
    _bound_check(f"composition{M}x{N}x{K}", out, y, 0.5 * _ulp(out.to(F64)) + acc_err + U * (y.abs() + acc_err))
