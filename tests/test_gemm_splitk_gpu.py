"""The split-K form of ltxk_gemm_bf16 (small M: fp32 slice tiles in the caller's scratch, then splitk_epilogue_kernel) against
the exact product: the bf16 operands multiplied in float64 on the device, then the epilogue.  Each case first asserts that its
plan is split-K (ops.gemm_plan), with an uneven last slice where K allows; M = 641 is the single-pass control.

Bias, +res and scale*res outputs are held to a rigorous element-wise bound: one bf16 rounding of the output (1/2 ulp), the
fp32 accumulation error K * 2^-24 * sum|a_k w_k| (any summation order, slices included), and the fp32 / bf16 roundings of the
epilogue's own steps (tests/ref_gemm.py: the bound and its helpers).  A dropped, doubled or mis-bounded slice, or a wrong row
of the last partial tile, moves an output by a whole partial sum - orders of magnitude beyond it.  GELU, SiLU and gate outputs
keep the ulp rules of test_gemm_split_k_form, against the float64 reference, and are held to ref_gemm.bound as well (no element
beyond it).  Also: two runs give the same bits, nothing outside the output views
is written (sentinels), and sumsq is the sum of squares of what was stored."""
import pytest
import torch

import ref_gemm

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -24

# M, N, K: N from the model's set (4096, q|k|v 12288, FF1 16384) and not a multiple of 128 (1000, 4104); K = 64*67 leaves the
# last slice short
CASES = [(1, 4096, 4096), (2, 1000, 64 * 67), (2, 16384, 4096), (31, 4104, 64 * 67), (33, 12288, 4096), (159, 4096, 4096),
         (161, 1000, 64 * 67), (320, 4096, 4096), (639, 4096, 16384), (640, 4096, 16384), (641, 4096, 16384)]


_ulp = ref_gemm.ulp


def _ulp_rule(name, got, ref, gate_max):
    """test_gemm_split_k_form's rule: <= 1 ulp on >= 99.8 % of outputs, worst within a few ulps at the row scale."""
    d = (got.to(F64) - ref).abs()
    rms = ref.pow(2).mean().sqrt()
    ulp = torch.maximum(ref.abs(), rms / 64).log2().floor().exp2() * 2.0 ** -7
    ulp_big = torch.maximum(ref.abs(), rms).log2().floor().exp2() * 2.0 ** -7
    worst = 3.001 if name.startswith(("epi1", "epi2")) else (2.001 * max(1.0, gate_max) if name.startswith("epi3") else 2.001)
    frac = float((d > ulp * 1.001).double().mean())
    assert frac <= 2e-3 and float((d / ulp_big).max()) <= worst, f"{name}: beyond 1 ulp on {frac:.2%}, max {float((d / ulp_big).max()):.1f} ulp"


def _bound_check(name, got, ref, bound):
    d = (got.to(F64) - ref).abs()
    bad = ref_gemm.beyond(d, bound)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} outputs beyond the rounding bound, worst excess "
                                 f"{float((d - bound).max()):.3e} at {tuple(int(i) for i in bad.nonzero()[0])}")


@pytest.mark.parametrize("M,N,K", CASES)
def test_gemm_split_k_against_float64(dev, M, N, K):
    from mlx_video_amd import _lib, ops
    lda = K + 64                                                   # strided A
    T = M // 2 if M % 2 == 0 else M                                # V^T / split outputs: 2 batches of T tokens (1 if M is odd)
    nb = M // T
    ld = (T // 4 + 2) * 4                                          # V^T row stride > T: pad columns carry a sentinel
    ns = 256                                                       # split output: k = columns [0, 256), V^T the rest
    want = _lib.GEMM_FORM_SPLITK if M <= ops.SPLITK_MAX_M else _lib.GEMM_FORM_SINGLE
    sq = N % 64 == 0
    for what, kw in [("row-major", dict(epilogue=ops.EPI_BIAS_GATE_RES, sumsq=sq)), ("epi1", dict(epilogue=ops.EPI_BIAS_GELU)),
                     ("vt", dict(out_tokens_per_batch=T, ldo=ld)),
                     ("split", dict(n_split=ns, out_tokens_per_batch=T, ldo=ns + 64, ldo2=ld, sumsq=sq))]:
        pl = ops.gemm_plan(M, N, K, lda=lda, **kw)
        assert pl.form == want, f"{what}: plan {pl} - re-aim this case at the split-K form"
        if want == _lib.GEMM_FORM_SPLITK:
            assert pl.slices >= 2

    g = torch.Generator(device=dev).manual_seed(M * 7 + N + K)
    a = torch.randn((M, lda), generator=g, device=dev).to(BF)[:, :K]
    w = (torch.randn((N, K), generator=g, device=dev) * K ** -0.5).to(BF)
    b = (torch.randn(N, generator=g, device=dev) * 0.1).to(BF)
    res = torch.randn((M, N), generator=g, device=dev).to(BF)
    gate = torch.randn((3, N), generator=g, device=dev).to(BF)
    grow = torch.randint(0, 3, (M,), generator=g, device=dev, dtype=torch.int32)
    alpha = 0.8
    alpha32 = float(torch.tensor(alpha, dtype=torch.float32))

    def run():
        out = {}
        for epi in range(6):
            for bias in (b, None):
                for gr in ((grow, None) if epi == ops.EPI_BIAS_GATE_RES else (None,)):
                    kw = dict(epilogue=epi)
                    if epi in (3, 4, 5):
                        kw["resid"] = res
                    if epi == 3:
                        kw.update(gate=gate, gate_row=gr, gate_stride=N)
                    if epi == 5:
                        kw["alpha"] = alpha
                    buf = torch.full((M + 1, N + 64), 7.0, device=dev, dtype=BF)
                    ss = torch.full((M, N // 64 + 1), -1.0, device=dev, dtype=torch.float32) if sq and epi in (0, 3, 4) else None
                    ops.gemm(a, w, bias, out=buf[:M, :N], sumsq=ss[:, :N // 64] if ss is not None else None, **kw)
                    out[f"epi{epi}.bias{bias is not None}.row{gr is not None}"] = (buf, ss)
        vt = torch.full((nb, N, ld), 3.0, device=dev, dtype=BF)
        ops.gemm(a, w, b, out=vt[:, :, :T], out_tokens_per_batch=T)
        out["vt"] = (vt, None)
        k2 = torch.full((M + 1, ns + 64), 7.0, device=dev, dtype=BF)
        v2 = torch.full((nb, N - ns, ld), 3.0, device=dev, dtype=BF)
        ss2 = torch.full((M, ns // 64 + 1), -1.0, device=dev, dtype=torch.float32) if sq else None
        ops.gemm(a, w, b, out=k2[:M, :ns], out2=v2[:, :, :T], n_split=ns, out_tokens_per_batch=T,
                 sumsq=ss2[:, :ns // 64] if sq else None)
        out["split.k"], out["split.vt"] = (k2, ss2), (v2, None)
        torch.cuda.synchronize()
        return out

    got, again = run(), run()
    for name in got:
        for x, y in zip(got[name], again[name]):
            assert x is None or torch.equal(x, y), f"{name}: results differ between two runs"

    s = a.to(F64) @ w.to(F64).t()                                  # exact: 8-bit significands, K <= 2^20 terms
    mag = a.to(F64).abs() @ w.to(F64).abs().t()                    # sum_k |a_k w_k|
    acc_err = K * U * mag                                          # fp32 accumulation, any order and slicing
    b64, r64 = b.to(F64), res.to(F64)
    gmax = float(gate.abs().max())

    def y_of(bias):
        """(exact pre-rounding value, its error bound) of y = bf16(acc + b) before that rounding."""
        if bias is None:
            return s, acc_err
        y = s + b64
        return y, acc_err + U * (y.abs() + acc_err)                # + the fp32 bias add

    for name, (buf, ss) in got.items():
        if name.startswith("split") or name == "vt":
            continue
        # sentinels: nothing beyond the (M, N) view, nothing beyond the row statistics
        assert bool((buf[M:] == 7.0).all()) and bool((buf[:, N:] == 7.0).all()), f"{name}: wrote outside the output view"
        out = buf[:M, :N]
        epi, bias_on, row_on = int(name[3]), "biasTrue" in name, "rowTrue" in name
        y, ey = y_of(b if bias_on else None)
        if epi == 0:
            _bound_check(name, out, y, 0.5 * _ulp(out.to(F64)) + ey)
        elif epi == 4:                                             # bf16(res + bf16(y)): two roundings and one fp32 add
            e1 = 0.5 * _ulp(y.abs() + ey) + ey
            _bound_check(name, out, r64 + y, 0.5 * _ulp(out.to(F64)) + U * (r64.abs() + y.abs() + e1) + e1)
        elif epi == 5:                                             # bf16(res + bf16(alpha * acc)); no bias
            z = alpha32 * s
            ez = abs(alpha32) * acc_err + U * (z.abs() + abs(alpha32) * acc_err)
            e1 = 0.5 * _ulp(z.abs() + ez) + ez
            _bound_check(name, out, r64 + z, 0.5 * _ulp(out.to(F64)) + U * (r64.abs() + z.abs() + e1) + e1)
        else:
            yb = y.to(torch.float32).to(BF).to(F64)
            if epi == 1:
                ref = torch.nn.functional.gelu(yb, approximate="tanh")
            elif epi == 2:
                ref = torch.nn.functional.silu(yb)
            else:
                gv = gate.to(F64)[grow.long()] if row_on else gate.to(F64)[0].expand(M, N)
                ref = r64 + (yb * gv).to(torch.float32).to(BF).to(F64)
            _ulp_rule(name, out, ref.to(torch.float32).to(BF).to(F64), gmax)
            gv = (gate[grow.long()] if row_on else gate[0].expand(M, N)) if epi == 3 else None
            w = ref_gemm.check(name, *ref_gemm.bound(epi, out, s, mag, K, b if bias_on else None, res if epi == 3 else None, gv))
            print(f"{name}: worst d / bound = {w:.3f}")
        if ss is not None:
            assert bool((ss[:, -1] == -1.0).all()), f"{name}: sumsq written past sumsq_ld's columns"
            sq64 = out.to(F64).pow(2).reshape(M, -1, 64).sum(-1)
            _bound_check(name + ".sumsq", ss[:, :-1], sq64, 64 * U * sq64 + 1e-30)

    # V^T: vt[b, n, t] = bf16(acc[b*T + t, n] + bias[n]); pad columns untouched
    y, ey = y_of(b)
    vt = got["vt"][0]
    assert bool((vt[:, :, T:] == 3.0).all()), "vt: wrote into the pad columns"
    vt_rows = vt[:, :, :T].permute(0, 2, 1).reshape(M, N)
    _bound_check("vt", vt_rows, y, 0.5 * _ulp(vt_rows.to(F64)) + ey)
    # split output: k row-major (with its row statistics), V^T of the remaining columns
    k2, ss2 = got["split.k"]
    v2 = got["split.vt"][0]
    assert bool((k2[M:] == 7.0).all()) and bool((k2[:, ns:] == 7.0).all()), "split.k: wrote outside the output view"
    assert bool((v2[:, :, T:] == 3.0).all()), "split.vt: wrote into the pad columns"
    k = k2[:M, :ns]
    _bound_check("split.k", k, y[:, :ns], 0.5 * _ulp(k.to(F64)) + ey[:, :ns])
    v_rows = v2[:, :, :T].permute(0, 2, 1).reshape(M, N - ns)
    _bound_check("split.vt", v_rows, y[:, ns:], 0.5 * _ulp(v_rows.to(F64)) + ey[:, ns:])
    if ss2 is not None:
        assert bool((ss2[:, -1] == -1.0).all())
        sq64 = k.to(F64).pow(2).reshape(M, -1, 64).sum(-1)
        _bound_check("split.sumsq", ss2[:, :-1], sq64, 64 * U * sq64 + 1e-30)
