"""ltxk_gemm_mxfp4 (e2m1 x e2m1 with e8m0 block scales on v_mfma_scale_f32_16x16x128_f8f6f4).  Operands are generated directly
as code and scale bytes (tests/ref_gemm_mxfp4.py); no quantiser is involved.

1. Exact data.  Codes over all 16 values, scale bytes from {126, 127, 128} drawn independently per (row, block) on both sides:
   every product is a multiple of 2^-4 (0.5 * 0.5 * 2^-1 * 2^-1) and sum |a w| <= 2304 * 144 < 2^19, so every partial sum in any
   order is a multiple of 2^-4 below 2^19 - exact in fp32.  The output is the bf16 rounding of the float64 product, bit for bit,
   row-major, transposed and split.  A derivation, not a tolerance.
2. Scale bytes spread over 110..140, rows whose blocks alternate between the two ends (2^30 apart) included, against float64 under
   ref_gemm.bound for every epilogue and output form: half a bf16 ulp of the output + K 2^-24 sum |a w| (fp32 accumulation of exact
   products in any order) + the roundings of the bias / residual / gate arithmetic.  The worst |error| / bound goes to the ledger.
3. A row's bits do not depend on M or the tile: the first 33 rows of an M = 161 launch equal the M = 33 launch.
4. Scale bytes 0, 1 and 254.   5. The C entry's refusals."""
import ctypes

import pytest
import torch

import parity
import ref_gemm
import ref_gemm_mxfp4 as R4

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
U8 = torch.uint8
KS = 256                                   # LTXK_MXFP4_KSTEP
SHAPES = [(16, 64, KS), (33, 136, 768), (161, 264, 768), (160, 1024, 2304)]


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same(name, x, y):
    assert torch.equal(_bits(x), _bits(y)), (f"{name}: {int((_bits(x) != _bits(y)).sum())} of {x.numel()} elements differ, "
                                             f"first at {tuple(int(i) for i in (_bits(x) != _bits(y)).nonzero()[0])}")


def _strided(t, pad, fill, dev):
    """``t`` as rows of a wider device buffer whose pad columns hold ``fill``."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf[:, :t.shape[1]]


def _operands(M, N, K, seed, scale_bytes, dev):
    """(A codes, A scales, W codes, W scales) on the device - A and its scales as rows of wider buffers (the scale pad is byte 255,
    NaN: nothing may read it) - and the CPU originals."""
    g = torch.Generator().manual_seed(seed)
    ac, asc = R4.random_pair(M, K, g, scale_bytes)
    wc, wsc = R4.random_pair(N, K, g, scale_bytes)
    return (_strided(ac, 64, 0x5A, dev), _strided(asc, 8, 255, dev), wc.to(dev), wsc.to(dev)), (ac, asc, wc, wsc), g


def _T(M):
    return M // 2 if M % 2 == 0 else M


def _vt(ops, ops4, M, N, bias, dev):
    T = _T(M)
    fr = ref_gemm.vt_frame(M // T, N, T, (T // 4 + 2) * 4, dev)
    ops.gemm_mxfp4(*ops4, bias, out=fr.view, out_tokens_per_batch=T)
    torch.cuda.synchronize()
    assert fr.intact(), "vt: wrote outside the output view"
    return ref_gemm.vt_rows(fr.view, T)


def _split(ops, ops4, M, N, bias, ns, sumsq, dev):
    T = _T(M)
    k = ref_gemm.rows_frame(M, ns, ns + 64, dev)
    v = ref_gemm.vt_frame(M // T, N - ns, T, (T // 4 + 2) * 4, dev)
    ss = ref_gemm.rows_frame(M, ns // 64, ns // 64 + 1, dev, dtype=torch.float32, lead=4, sentinel=-1.0) if sumsq else None
    ops.gemm_mxfp4(*ops4, bias, out=k.view, out2=v.view, n_split=ns, out_tokens_per_batch=T, sumsq=ss.view if sumsq else None)
    torch.cuda.synchronize()
    assert k.intact() and v.intact() and (ss is None or ss.intact()), "split output: wrote outside a view"
    return k.view, ref_gemm.vt_rows(v.view, T), (ss.view if sumsq else None)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_mxfp4_exact_data(dev, M, N, K):
    from mlx_video_amd import _lib, ops
    pl = ops.gemm_plan(M, N, K, lda=K // 2 + 64, mxfp4=True)
    assert pl.form == _lib.GEMM_FORM_SINGLE and pl.ksteps == K // KS and pl.slices == 1
    ops4, cpu, _ = _operands(M, N, K, 1000 + M + N + K, (126, 127, 128), dev)
    s, mag = R4.product(*cpu)
    assert float(mag.max()) < 2.0 ** 19 and bool((s * 16 == (s * 16).round()).all())          # the derivation's premises
    want = s.to(BF).to(dev)
    fr = ref_gemm.rows_frame(M, N, N + 8, dev)
    ops.gemm_mxfp4(*ops4, None, out=fr.view)
    torch.cuda.synchronize()
    assert fr.intact(), "wrote outside the output view"
    _same("row-major", fr.view, want)
    _same("transposed", _vt(ops, ops4, M, N, None, dev), want)
    if N % 256 == 0 and N > 256:
        for ns in (256, 512):
            k, v, _ = _split(ops, ops4, M, N, None, ns, False, dev)
            _same(f"split {ns}: row-major part", k, want[:, :ns])
            _same(f"split {ns}: transposed part", v, want[:, ns:])


def _wide_scales(M, N, K, seed, dev):
    """Scale bytes over 110..140; every fourth row (of both operands) alternates 110 / 140 from block to block: neighbouring blocks
    of one row 2^30 apart."""
    ops4, (ac, asc, wc, wsc), g = _operands(M, N, K, seed, range(110, 141), "cpu")
    alt = torch.tensor([110, 140], dtype=U8).repeat(K // 64)
    asc[::4] = alt
    wsc[1::4] = alt.flip(0)
    cpu = (ac, asc, wc, wsc)
    return (_strided(ac, 64, 0x5A, dev), _strided(asc, 8, 255, dev), wc.to(dev), wsc.to(dev)), cpu, g


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_mxfp4_against_float64(dev, M, N, K):
    from mlx_video_amd import ops
    ops4, cpu, g = _wide_scales(M, N, K, 2000 + M + N + K, dev)
    s, mag = (t.to(dev) for t in R4.product(*cpu))
    # epilogue operands of the size of the products' spread, so that none of the terms is idle
    amp = float(s.abs().median()) + 1.0
    b = (torch.randn(N, generator=g) * amp).to(BF).to(dev)
    res = _strided((torch.randn((M, N), generator=g) * amp).to(BF), 4, float("nan"), dev)
    tab = torch.randn((3, 2 * N), generator=g).to(BF).to(dev)
    gate, grow = tab[:, N:], torch.randint(0, 3, (M,), generator=g, dtype=torch.int32).to(dev)
    worst = 0.0
    for epi in range(6):
        for bias in (b, None):
            for gr in ((grow, None) if epi == ops.EPI_BIAS_GATE_RES else (None,)):
                kw = dict(epilogue=epi)
                if epi in (3, 4, 5):
                    kw["resid"] = res
                if epi == 3:
                    kw.update(gate=gate, gate_row=gr, gate_stride=2 * N)
                if epi == 5:
                    kw["alpha"] = 0.8
                fr = ref_gemm.rows_frame(M, N, N + 8, dev)
                ops.gemm_mxfp4(*ops4, bias, out=fr.view, **kw)
                torch.cuda.synchronize()
                assert fr.intact(), f"epilogue {epi}: wrote outside the output view"
                gv = None if epi != 3 else (gate[gr.long()] if gr is not None else gate[0].expand(M, N))
                d, bnd = ref_gemm.bound(epi, fr.view, s, mag, K, bias, res if epi in (3, 4, 5) else None, gv, 0.8)
                if epi in (1, 2):
                    # ref_gemm.bound presumes no pre-activation where 1 + exp2(t) >= 2^126 (its ``premises``); these products span
                    # 60 binades and some land there.  The device's reciprocal is then a subnormal flushed to zero, and x * rcp is
                    # off by at most |y| 2^-126: that term, instead of the premise.
                    bnd = bnd + ref_gemm.FLUSH * (s if bias is None else s + bias.to(F64)).abs()
                name = f"epi{epi}.bias{bias is not None}.row{gr is not None}"
                worst = max(worst, ref_gemm.check(name, d, bnd))
    d, bnd = ref_gemm.bound(0, _vt(ops, ops4, M, N, b, dev), s, mag, K, b)
    worst = max(worst, ref_gemm.check("vt", d, bnd))
    if N % 256 == 0 and N > 256:
        k, v, ss = _split(ops, ops4, M, N, b, 256, True, dev)
        d, bnd = ref_gemm.bound(0, k, s[:, :256], mag[:, :256], K, b[:256])
        worst = max(worst, ref_gemm.check("split.k", d, bnd))
        d, bnd = ref_gemm.bound(0, v, s[:, 256:], mag[:, 256:], K, b[256:])
        worst = max(worst, ref_gemm.check("split.vt", d, bnd))
        ref_gemm.check("split.sumsq", *ref_gemm.sumsq_bound(ss, k))
    print(f"mxfp4 {M}x{N}x{K}: worst |error| / bound = {worst:.3f}")
    parity.auto(worst, 1.0, tag="worst_error_over_bound")


@pytest.mark.parametrize("N,sumsq", [(264, False), (256, False), (256, True)])
def test_mxfp4_row_bits_independent_of_the_launch(dev, N, sumsq):
    """The first 33 rows of the (161, N, 768) call equal the (33, N, 768) call (another grid), as int16 views - with the row
    statistic on (N = 256: it needs N % 64 == 0) and off.  (Other tiles: test_mxfp4_every_tile.)"""
    from mlx_video_amd import ops
    K = 768
    (ac, asc, wc, wsc), _, g = _operands(161, N, K, 77, range(110, 141), dev)
    b = torch.randn(N, generator=g).to(BF).to(dev)
    outs = []
    for M in (161, 33):
        fr = ref_gemm.rows_frame(M, N, N + 8, dev)
        ss = ref_gemm.rows_frame(M, N // 64, N // 64 + 1, dev, dtype=torch.float32, lead=4, sentinel=-1.0) if sumsq else None
        ops.gemm_mxfp4(ac[:M], asc[:M], wc, wsc, b, out=fr.view, sumsq=ss.view if sumsq else None)
        torch.cuda.synchronize()
        assert fr.intact() and (ss is None or ss.intact())
        outs.append((fr.view, ss.view if sumsq else None))
    _same("rows 0..32", outs[0][0][:33], outs[1][0])
    if sumsq:
        _same("sumsq of rows 0..32", outs[0][1][:33], outs[1][1])


@pytest.mark.parametrize("nt", [2, 4], ids=["128col", "256col"])
@pytest.mark.parametrize("tt", [1, 2, 3, 4, 5])
def test_mxfp4_every_tile(dev, tt, nt, monkeypatch, ab_lib):
    """Every tile height and both widths of the 160-row family, forced through the measurement build (the product library picks
    the 32 x 128 tile at these sizes): two row tiles with one row in the second, a ragged column tile.
    Exact data (K = 768 and 2816: 3 and 11 K-steps, the second past the peeled steps of every height) bit for bit in every output
    form; wide-scale data under the float64 bound with the residual epilogues (their operands arrive under the K-steps) and the
    row statistic; and the bits of the forced tile are those of the tile the library picks by itself for the same call (a row's
    bits do not depend on the tile)."""
    from mlx_video_amd import _lib, ops

    def force(on):
        for k, v in (("LTXK_GEMM_TT", tt), ("LTXK_GEMM_NT", nt)):
            monkeypatch.setenv(k, str(v)) if on else monkeypatch.delenv(k, raising=False)

    force(True)
    M = 32 * tt + 1
    for N, K in ((264, 768), (512, 2816)):
        pl = ops.gemm_plan(M, N, K, mxfp4=True)
        assert (pl.form, pl.tile_rows, pl.tile_cols, pl.row_tiles) == (_lib.GEMM_FORM_SINGLE, 32 * tt, 64 * nt, 2), pl
        ops4, cpu, _ = _operands(M, N, K, 3000 + tt + N, (126, 127, 128), dev)
        s, mag = R4.product(*cpu)
        assert float(mag.max()) < 2.0 ** 19
        want = s.to(BF).to(dev)
        fr = ref_gemm.rows_frame(M, N, N + 8, dev)
        ops.gemm_mxfp4(*ops4, None, out=fr.view)
        torch.cuda.synchronize()
        assert fr.intact(), "wrote outside the output view"
        _same(f"{N}x{K} row-major", fr.view, want)
        _same(f"{N}x{K} transposed", _vt(ops, ops4, M, N, None, dev), want)
        if N == 512:
            k, v, _ = _split(ops, ops4, M, N, None, 256, False, dev)
            _same("split: row-major part", k, want[:, :256])
            _same("split: transposed part", v, want[:, 256:])
    M, N, K = 161, 320, 2816                             # the same operands for every tile: 2 to 6 row tiles, the last one ragged
    ops4, cpu, g = _wide_scales(M, N, K, 4000, dev)
    s, mag = (t.to(dev) for t in R4.product(*cpu))
    amp = float(s.abs().median()) + 1.0
    b = (torch.randn(N, generator=g) * amp).to(BF).to(dev)
    res = _strided((torch.randn((M, N), generator=g) * amp).to(BF), 4, float("nan"), dev)
    gate = torch.randn((1, N), generator=g).to(BF).to(dev)
    worst = 0.0
    own = ops.gemm_plan(M, N, K, mxfp4=True)
    force(False)
    free = ops.gemm_plan(M, N, K, mxfp4=True)                # the library's own choice: the 32 x 128 tile at this size
    assert (free.tile_rows, free.tile_cols) == (32, 128) and (own.tile_rows, own.tile_cols) == (32 * tt, 64 * nt)

    def run(kw):
        fr = ref_gemm.rows_frame(M, N, N + 8, dev)
        ss = ref_gemm.rows_frame(M, N // 64, N // 64 + 1, dev, dtype=torch.float32, lead=4, sentinel=-1.0)
        ops.gemm_mxfp4(*ops4, b, out=fr.view, sumsq=ss.view, **kw)
        torch.cuda.synchronize()
        assert fr.intact() and ss.intact(), f"{kw['epilogue']}: wrote outside a view"
        return fr, ss

    for epi in (0, 3, 4, 5):
        kw = dict(epilogue=epi)
        if epi != 0:
            kw["resid"] = res
        if epi == 3:
            kw.update(gate=gate, gate_stride=N)
        if epi == 5:
            kw["alpha"] = 0.8
        force(False)
        fr0, ss0 = run(kw)
        force(True)
        fr, ss = run(kw)
        d, bnd = ref_gemm.bound(epi, fr.view, s, mag, K, b, res if epi != 0 else None, gate.expand(M, N) if epi == 3 else None, 0.8)
        worst = max(worst, ref_gemm.check(f"tile {32 * tt}x{64 * nt} epi{epi}", d, bnd))
        ref_gemm.check(f"tile {32 * tt}x{64 * nt} epi{epi} sumsq", *ref_gemm.sumsq_bound(ss.view, fr.view))
        _same(f"epilogue {epi}: tile {32 * tt}x{64 * nt} against the 32x128 tile", fr.view, fr0.view)
        _same(f"epilogue {epi}: row statistic of tile {32 * tt}x{64 * nt} against the 32x128 tile", ss.view, ss0.view)
    parity.auto(worst, 1.0, tag="worst_error_over_bound")


def test_mxfp4_scale_extremes(dev):
    """Scale bytes 0 (2^-127), 1 and 254 (2^127) on operands that are 0 or +-0.5, paired so that every product is finite in fp32:
    block 0: a at byte 254 x w at byte 0; block 1: a at byte 1 x w at byte 254; block 2: a at byte 0 x w at byte 254; the other
    blocks hold zero codes under bytes 254 (a) and 0 (w).  Compared exactly with the float64 product (multiples of 2^-3)."""
    from mlx_video_amd import ops
    M, N, K = 16, 64, KS
    g = torch.Generator().manual_seed(5)
    half = torch.tensor([0x00, 0x01, 0x09, 0x11, 0x19, 0x91, 0x99, 0x10, 0x90], dtype=U8)      # nibbles from {0, +0.5, -0.5}
    ac = torch.zeros((M, K // 2), dtype=U8)
    wc = torch.zeros((N, K // 2), dtype=U8)
    ac[:, :48] = half[torch.randint(0, len(half), (M, 48), generator=g)]
    wc[:, :48] = half[torch.randint(0, len(half), (N, 48), generator=g)]
    asc = torch.tensor([254, 1, 0] + [254] * 5, dtype=U8).repeat(M, 1)
    wsc = torch.tensor([0, 254, 254] + [0] * 5, dtype=U8).repeat(N, 1)
    s, _ = R4.product(ac, asc, wc, wsc)
    assert bool(torch.isfinite(s).all()) and float(s.abs().max()) > 1.0
    fr = ref_gemm.rows_frame(M, N, N + 8, dev)
    ops.gemm_mxfp4(ac.to(dev), asc.to(dev), wc.to(dev), wsc.to(dev), None, out=fr.view)
    torch.cuda.synchronize()
    assert fr.intact()
    _same("scale extremes", fr.view, s.to(BF).to(dev))


def test_mxfp4_argument_errors(dev):
    from mlx_video_amd import _lib, ops
    lib = _lib.load()

    def args(**over):
        a = _lib.GemmArgs()
        a.A = a.W = a.out = 1 << 12
        a.M, a.N, a.K, a.lda, a.ldo = 64, 1024, 2304, 1152, 1024
        for k, v in over.items():
            setattr(a, k, v)
        return a

    sc, ld = ctypes.c_void_p(1 << 12), 72
    pl = _lib.GemmPlan()
    assert lib.ltxk_gemm_mxfp4_plan(ctypes.byref(args()), ctypes.byref(pl)) == 0 and pl.form == _lib.GEMM_FORM_SINGLE and pl.ksteps == 9
    # refused before anything is launched (the pointers are not memory)
    for over in (dict(K=2176, lda=1088), dict(K=128, lda=64), dict(lda=1152 + 8), dict(lda=1024), dict(A=(1 << 12) + 8),
                 dict(W=(1 << 12) + 8), dict(N=12), dict(epilogue=9)):
        a = args(**over)
        assert lib.ltxk_gemm_mxfp4_plan(ctypes.byref(a), ctypes.byref(pl)) == -1, over
        assert lib.ltxk_gemm_mxfp4(ctypes.byref(a), sc, ld, sc, ld, None) == -1, over
    assert lib.ltxk_gemm_mxfp4(ctypes.byref(args()), None, ld, sc, ld, None) == -1 and b"block-scale" in lib.ltxk_last_error()
    assert lib.ltxk_gemm_mxfp4(ctypes.byref(args()), sc, ld, None, ld, None) == -1
    assert lib.ltxk_gemm_mxfp4(ctypes.byref(args()), ctypes.c_void_p((1 << 12) + 4), ld, sc, ld, None) == -1
    assert lib.ltxk_gemm_mxfp4(ctypes.byref(args()), sc, ld, ctypes.c_void_p((1 << 12) + 4), ld, None) == -1
    assert lib.ltxk_gemm_mxfp4(ctypes.byref(args()), sc, 76, sc, ld, None) == -1            # stride not a multiple of 8
    assert lib.ltxk_gemm_mxfp4(ctypes.byref(args()), sc, 64, sc, ld, None) == -1            # stride below K / 32
    with pytest.raises(ValueError, match="K % 256"):
        ops.gemm_mxfp4(torch.zeros((4, 64), dtype=U8, device=dev), torch.zeros((4, 4), dtype=U8, device=dev),
                       torch.zeros((8, 64), dtype=U8, device=dev), torch.zeros((8, 4), dtype=U8, device=dev))
