"""ltxk_gemm_w8 (FP8 e4m3 weight panel, bf16 activations) against ltxk_gemm_bf16 on the panel converted to bf16.

Every e4m3 value is a bf16 value, the W8 kernels widen the panel in registers and feed the same MFMAs in the same K order, and
ltxk_gemm_w8_plan takes the split-K decision of ltxk_gemm_plan: with no scale the two calls must agree BIT FOR BIT on every
output (out, out2, sumsq) - no tolerance.  Outputs are compared as raw bits (a -0 for a +0 is a difference), over sentinel-
filled buffers (a write outside the view is a difference too).

With a per-output-channel scale the reference is the exact product A x (W8 * scale) in float64 under the element-wise bound of
tests/test_gemm_splitk_gpu.py: half a bf16 ulp of the output, K * 2^-24 * sum|a_k w_k| for the fp32 arithmetic - K - 1
additions in any order and slicing plus ONE more fp32 rounding, which is what the multiplication by the scale adds - and the
fp32 bias add.  Nothing is added to that bound."""
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


def _weights(N, K, g, dev):
    """Weights of a Linear layer's size, already e4m3 values."""
    return (torch.randn((N, K), generator=g, device=dev) * K ** -0.5 * 4).to(F8)


def _operands(M, N, K, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    lda = K + 64
    a = torch.randn((M, lda), generator=g, device=dev).to(BF)[:, :K]          # strided A
    b = (torch.randn(N, generator=g, device=dev) * 0.1).to(BF)
    res = torch.randn((M, N), generator=g, device=dev).to(BF)
    gate = torch.randn((3, N), generator=g, device=dev).to(BF)
    grow = torch.randint(0, 3, (M,), generator=g, device=dev, dtype=torch.int32)
    return g, a, b, res, gate, grow


def _run_all(ops, a, w, b, res, gate, grow, *, sumsq, split_k, w_scale=None, epilogues=range(6)):
    """Every epilogue (with and without bias, gate rows on and off) and the transposed output of one weight panel `w` (bf16 or
    fp8).  Returns name -> (buffer incl. sentinels, sumsq buffer or None)."""
    M, K = a.shape
    N = w.shape[0]
    dev = a.device
    kw8 = {} if w_scale is None else {"w_scale": w_scale}
    out = {}
    for epi in epilogues:
        for bias in (b, None):
            for gr in ((grow, None) if epi == ops.EPI_BIAS_GATE_RES else (None,)):
                kw = dict(epilogue=epi, split_k=split_k, **kw8)
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
    ops.gemm(a, w, b, out=vt[:, :, :T], out_tokens_per_batch=T, split_k=split_k, **kw8)
    out["vt"] = (vt, None)
    torch.cuda.synchronize()
    return out


def _compare(got, ref):
    assert got.keys() == ref.keys()
    for name in got:
        for x, y in zip(got[name], ref[name]):
            if x is not None:
                _same(name, x, y)


# every tile height of the 160-row family (1 -> 32 rows ... 160), a second row tile with one row (161); N below one 128-column
# tile, one tile + 8 and two tiles + 8 (the 256-column tile's edge); one K-step and nine (past every peeled step of the loop)
@pytest.mark.parametrize("K", [64, 576])
@pytest.mark.parametrize("N", [8, 136, 264])
@pytest.mark.parametrize("M", [1, 33, 160, 161])
def test_w8_equals_bf16_on_upcast_panel(dev, M, N, K):
    from mlx_video_amd import _lib, ops
    assert ops.gemm_plan(M, N, K, lda=K + 64, w8=True, split_k=False).form == _lib.GEMM_FORM_SINGLE
    g, a, b, res, gate, grow = _operands(M, N, K, dev, M * 7 + N + K)
    w8 = _weights(N, K, g, dev)
    got = _run_all(ops, a, w8, b, res, gate, grow, sumsq=False, split_k=False)
    ref = _run_all(ops, a, w8.to(BF), b, res, gate, grow, sumsq=False, split_k=False)
    _compare(got, ref)


# the row statistic (N % 64 == 0): on the 128-column tile (two waves share a 64-column block) and on the 256-column one
@pytest.mark.parametrize("M,N,K", [(161, 192, 576), (33, 512, 64), (160, 1024, 576)])
def test_w8_sumsq_on_and_off(dev, M, N, K):
    from mlx_video_amd import ops
    g, a, b, res, gate, grow = _operands(M, N, K, dev, M + N + K)
    w8 = _weights(N, K, g, dev)
    got = _run_all(ops, a, w8, b, res, gate, grow, sumsq=True, split_k=False, epilogues=(0, 3, 4))
    ref = _run_all(ops, a, w8.to(BF), b, res, gate, grow, sumsq=True, split_k=False, epilogues=(0, 3, 4))
    _compare(got, ref)


def _split_output(ops, a, w, b, T, ns, *, sumsq, split_k, w_scale=None):
    M, N = a.shape[0], w.shape[0]
    ld = (T // 4 + 2) * 4
    k2 = torch.full((M + 1, ns + 64), 7.0, device=a.device, dtype=BF)
    v2 = torch.full((M // T, N - ns, ld), 3.0, device=a.device, dtype=BF)
    ss = torch.full((M, ns // 64 + 1), -1.0, device=a.device, dtype=torch.float32) if sumsq else None
    ops.gemm(a, w, b, out=k2[:M, :ns], out2=v2[:, :, :T], n_split=ns, out_tokens_per_batch=T,
             sumsq=ss[:, :ns // 64] if sumsq else None, split_k=split_k, **({} if w_scale is None else {"w_scale": w_scale}))
    torch.cuda.synchronize()
    return {"split.k": (k2, ss), "split.vt": (v2, None)}


@pytest.mark.parametrize("sumsq", [True, False])
def test_w8_split_output(dev, sumsq):
    """q|k row-major and V^T from one launch: N = 512, n_split = 256, two batches of 40 tokens."""
    from mlx_video_amd import ops
    M, N, K, T, ns = 80, 512, 576, 40, 256
    g, a, b, *_ = _operands(M, N, K, dev, 11)
    w8 = _weights(N, K, g, dev)
    _compare(_split_output(ops, a, w8, b, T, ns, sumsq=sumsq, split_k=False),
             _split_output(ops, a, w8.to(BF), b, T, ns, sumsq=sumsq, split_k=False))


def test_w8_every_finite_code(dev):
    """W's bytes run over all 254 finite e4m3 codes - subnormals, +-0 and +-448 included; the two NaN codes (0x7f, 0xff) left
    out - each code at every k position of a fragment (the row length 576 and the code count 254 are coprime to 8)."""
    from mlx_video_amd import ops
    M, N, K = 33, 136, 576
    codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
    assert codes.numel() == 254
    idx = (torch.arange(N * K) * 3 + torch.arange(N * K) // K) % 254           # every code in every row, shifted per row
    w8 = codes[idx].reshape(N, K).to(dev).view(F8)
    wb = w8.to(BF)
    assert bool(torch.isfinite(wb.float()).all()) and torch.unique(w8.view(torch.uint8)).numel() == 254
    assert torch.equal(wb.float(), w8.float()), "e4m3 -> bf16 must be exact on the host side of the comparison too"
    g, a, b, res, gate, grow = _operands(M, N, K, dev, 5)
    a = (a.float() * 2.0 ** -4).to(BF)                                           # keeps |out| far below the bf16 overflow
    got = _run_all(ops, a, w8, b, res, gate, grow, sumsq=False, split_k=False, epilogues=(0, 4, 5))
    ref = _run_all(ops, a, wb, b, res, gate, grow, sumsq=False, split_k=False, epilogues=(0, 4, 5))
    _compare(got, ref)
    # and a panel that is nothing but the smallest subnormal and -0: the product must keep them (no flush in the widening)
    tiny = torch.tensor([0x01, 0x80], dtype=torch.uint8).repeat(N * K // 2).reshape(N, K).to(dev).view(F8)
    ones = torch.ones((M, K), device=dev, dtype=BF)
    x = ops.gemm(ones, tiny, None, split_k=False)
    y = ops.gemm(ones, tiny.to(BF), None, split_k=False)
    torch.cuda.synchronize()
    _same("subnormal panel", x, y)
    assert float(x.float().abs().min()) == K // 2 * 2.0 ** -9


# split-K: M = 64 on the 64-row tile, M = 200 on the 160-row tile plus a 40-row remainder; K = 33 K-steps
SPLITK = [(64, 1024, 2112, 4, 9), (200, 1024, 2112, 2, 17)]


@pytest.mark.parametrize("M,N,K,slices,ksteps", SPLITK)
def test_w8_split_k_equals_bf16(dev, M, N, K, slices, ksteps):
    from mlx_video_amd import _lib, ops
    T = M // 2
    for kw in (dict(), dict(epilogue=ops.EPI_BIAS_GATE_RES, sumsq=True), dict(out_tokens_per_batch=T),
               dict(n_split=256, out_tokens_per_batch=T, sumsq=True, ldo=256 + 64, ldo2=(T // 4 + 2) * 4)):
        pb, p8 = ops.gemm_plan(M, N, K, lda=K + 64, **kw), ops.gemm_plan(M, N, K, lda=K + 64, w8=True, **kw)
        assert pb.form == p8.form == _lib.GEMM_FORM_SPLITK, f"{kw}: plans {pb} / {p8} - re-aim this case at the split-K form"
        assert (p8.slices, p8.ksteps) == (pb.slices, pb.ksteps) == (slices, ksteps)
        assert K // 64 % ksteps != 0, "the last slice is meant to be short"
    g, a, b, res, gate, grow = _operands(M, N, K, dev, M + 1)
    w8 = _weights(N, K, g, dev)
    _compare(_run_all(ops, a, w8, b, res, gate, grow, sumsq=True, split_k=True),
             _run_all(ops, a, w8.to(BF), b, res, gate, grow, sumsq=True, split_k=True))
    _compare(_split_output(ops, a, w8, b, T, 256, sumsq=True, split_k=True),
             _split_output(ops, a, w8.to(BF), b, T, 256, sumsq=True, split_k=True))


_ulp = ref_gemm.ulp          # (the bound's helpers: tests/ref_gemm.py)


def _bound_check(name, got, ref, bound):
    d = (got.to(F64) - ref).abs()
    bad = ref_gemm.beyond(d, bound)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} outputs beyond the rounding bound, worst excess "
                                 f"{float((d - bound).max()):.3e} at {tuple(int(i) for i in bad.nonzero()[0])}")


@pytest.mark.parametrize("M,N,K,split_k", [(33, 136, 576, False), (161, 264, 576, False), (64, 1024, 2112, True)])
def test_w8_channel_scale_against_float64(dev, M, N, K, split_k):
    """Scales 2^-8 ... 2^4, one per output channel (random mantissas, so the fp32 multiply rounds), on the accumulator before the
    bias: row-major with and without bias, transposed, split output where N allows."""
    from mlx_video_amd import _lib, ops
    if split_k:
        assert ops.gemm_plan(M, N, K, lda=K + 64, w8=True).form == _lib.GEMM_FORM_SPLITK
    g, a, b, res, gate, grow = _operands(M, N, K, dev, M * 3 + N)
    w8 = _weights(N, K, g, dev)
    expo = torch.linspace(-8.0, 4.0, N, device=dev)[torch.randperm(N, generator=g, device=dev)]
    scale = (torch.exp2(expo) * (1.0 + 0.5 * torch.rand(N, generator=g, device=dev))).float().clamp(2.0 ** -8, 2.0 ** 4)
    scale[0], scale[-1] = 2.0 ** -8, 2.0 ** 4
    got = _run_all(ops, a, w8, b, res, gate, grow, sumsq=False, split_k=split_k, w_scale=scale, epilogues=(0,))
    wd = w8.to(F64) * scale.to(F64)[:, None]                        # exact: 4-bit x 24-bit significands
    s = a.to(F64) @ wd.t()
    mag = a.to(F64).abs() @ wd.abs().t()
    acc_err = K * U * mag                                           # K - 1 fp32 additions in any order + the scale multiply
    y = s + b.to(F64)
    ey = acc_err + U * (y.abs() + acc_err)
    T = M // 2 if M % 2 == 0 else M
    for name, (buf, _) in got.items():
        if name == "vt":
            assert bool((buf[:, :, T:] == 3.0).all()), "vt: wrote into the pad columns"
            rows = buf[:, :, :T].permute(0, 2, 1).reshape(M, N)
            _bound_check(name, rows, y, 0.5 * _ulp(rows.to(F64)) + ey)
            continue
        assert bool((buf[M:] == 7.0).all()) and bool((buf[:, N:] == 7.0).all()), f"{name}: wrote outside the output view"
        out = buf[:M, :N]
        if "biasTrue" in name:
            _bound_check(name, out, y, 0.5 * _ulp(out.to(F64)) + ey)
        else:
            _bound_check(name, out, s, 0.5 * _ulp(out.to(F64)) + acc_err)
    if N % 256 == 0 and N > 256:
        sp = _split_output(ops, a, w8, b, T, 256, sumsq=True, split_k=split_k, w_scale=scale)
        k = sp["split.k"][0][:M, :256]
        _bound_check("split.k", k, y[:, :256], 0.5 * _ulp(k.to(F64)) + ey[:, :256])
        v = sp["split.vt"][0][:, :, :T].permute(0, 2, 1).reshape(M, N - 256)
        _bound_check("split.vt", v, y[:, 256:], 0.5 * _ulp(v.to(F64)) + ey[:, 256:])
        sq64 = k.to(F64).pow(2).reshape(M, -1, 64).sum(-1)
        _bound_check("split.sumsq", sp["split.k"][1][:, :-1], sq64, 64 * U * sq64 + 1e-30)
