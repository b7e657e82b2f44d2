"""What tests/ref_gemm.py's bound accepts and what it rejects, on the inputs the GPU cases use (ref_gemm.inputs is seeded on
the CPU generator), without a GPU.

Accepts: bf16 of an fp32 emulation of csrc/epilogue.h - gelu_tanh_f / silu_f written from csrc/common.h, one IEEE fp32
operation and one round-to-nearest-even per step - on accumulators summed in three orders (one fp32 matmul; K-steps of 64
added last to first; 3 slice sums added in slice order), for the six epilogues with and without bias and gate_row, V^T and
the split output.  The cap on elements beyond the bound is ZERO.  Rejects: seven planted faults of the kind a tile kernel
makes, each of which must put at least one element beyond the bound.  The worst d / bound of each is printed."""
import math

import pytest
import torch

import ref_gemm as R

BF, F64 = R.BF, R.F64
SHAPES = [(33, 136, 64), (145, 264, 192), (337, 1000, 192), (81, 520, 64 * 67)]


def seed_of(M, N, K):
    return M * 7 + N * 3 + K


def rbf32(x):
    return x.to(BF).float()


def gelu_dev(x):
    """gelu_tanh_f: t = fma(c2, x*x, c1) * x (the fma through float64: the product of two floats is exact there), then
    x * rcp(1 + exp2(t))."""
    c1, c2 = torch.tensor(-2.3022082, dtype=torch.float32), torch.tensor(-0.10294324, dtype=torch.float32)
    t = (c2.double() * (x * x).double() + c1.double()).float() * x
    return x * (1.0 / (1.0 + torch.exp2(t)))


def silu_dev(x):
    return x * (1.0 / (1.0 + torch.exp2(torch.tensor(-1.4426950408889634, dtype=torch.float32) * x)))


def accumulate(inp, order):
    a, w, K = inp.a.float(), inp.w.float(), inp.K
    if order == "matmul":
        return a @ w.t()
    if order == "ksteps_reversed":
        acc = torch.zeros((inp.M, inp.N))
        for k0 in reversed(range(0, K, 64)):
            acc = acc + a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()
        return acc
    per = (K // 64 + 2) // 3 * 64                                      # 3 slices, the last one short where K allows
    parts = [a[:, k0:k0 + per] @ w[:, k0:k0 + per].t() for k0 in range(0, K, per)]
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


def epilogue(epi, acc, inp, bias_on, row_on=True, bias=None, res=None, gate=None):
    """csrc/epilogue.h's epi_value in fp32, to the stored bf16.  bias / res / gate override the operands (a planted fault)."""
    b = (inp.b if bias is None else bias).float()
    r = (inp.res if res is None else res).float()
    g = (R.gate_of(inp, row_on) if gate is None else gate).float()
    yb = rbf32(acc + b) if bias_on else rbf32(acc)
    if epi == R.EPI_BIAS_GELU:
        yb = gelu_dev(yb)
    elif epi == R.EPI_BIAS_SILU:
        yb = silu_dev(yb)
    elif epi == R.EPI_BIAS_GATE_RES:
        yb = r + rbf32(yb * g)
    elif epi == R.EPI_BIAS_RES:
        yb = r + yb
    elif epi == R.EPI_SCALE_RES:
        yb = r + rbf32(torch.tensor(inp.alpha, dtype=torch.float32) * acc)
    return yb.to(BF)


def bound_of(epi, out, inp, s, mag, bias_on, row_on=True):
    return R.bound(epi, out, s, mag, inp.K, inp.b if bias_on else None, inp.res if epi >= 3 else None,
                   R.gate_of(inp, row_on) if epi == R.EPI_BIAS_GATE_RES else None, inp.alpha)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    M, N, K = request.param
    inp = R.inputs(M, N, K, seed_of(M, N, K))
    s, mag = R.product(inp.a, inp.w)
    return inp, s, mag


def test_premises(case):
    inp, s, mag = case
    R.premises(inp, s, mag)
    assert len(inp.edge) == 7 and [v for _, v in inp.edge] == list(R.EDGE_BIAS)
    assert R.edge_columns(8) == [] and len(R.edge_columns(64)) == 7 and len(R.edge_columns(24)) == 2
    # the pads of the strided operands are NaN, the operands themselves are not
    assert inp.a.stride(0) == inp.K + 8 and inp.res.stride(0) == inp.N + 4 and inp.gate.stride(0) == 2 * inp.N
    assert bool(torch.isnan(inp.a.as_strided((inp.M, 8), (inp.K + 8, 1), inp.K).float()).all())


def test_lipschitz_constants_and_e_act():
    """L: the largest |f'| on the grid the docstring names (central differences in float64); E_ACT: the operation count."""
    y = torch.arange(-40 * 1024, 40 * 1024 + 1, dtype=F64) / 1024
    h = 2.0 ** -20
    for f, L, at in ((R.gelu64, R.L_GELU, 1.42), (R.silu64, R.L_SILU, 2.40)):
        df = ((f(y + h) - f(y - h)) / (2 * h)).abs()
        i = int(df.argmax())
        print(f"{f.__name__}: max |f'| = {float(df[i]):.5f} at y = {float(y[i]):.3f}")
        assert float(df[i]) <= L and float(df[i]) > L - 0.002 and abs(float(y[i]) - at) < 0.01
    t_err = 3 + 2 * 1.1
    count = 128 * math.log(2) * t_err + 2 + 1 + 2 + 1
    print(f"E_ACT: {count:.1f} u, set to {R.E_ACT / R.U:.0f} u")
    assert count + 0.1 < 468 <= R.E_ACT / R.U == 512


def test_device_activation_emulation_within_e_act():
    """The fp32 emulation itself against the float64 function on a dense grid and at the edge values: within E_ACT relative
    (plus a flushed subnormal) - the term the bound spends on it."""
    x = torch.cat([torch.arange(-9.8 * 4096, 20 * 4096, dtype=torch.float32) / 4096, torch.tensor(R.EDGE_BIAS + (-3e38, 88.0, -80.0))])
    for dev_f, f in ((gelu_dev, R.gelu64), (silu_dev, R.silu64)):
        ref = f(x.double())
        d = (dev_f(x).double() - ref).abs()
        lim = R.E_ACT * ref.abs() + R.FLUSH
        print(f"{f.__name__}: worst emulation error / (E_ACT |f| + 2^-126) = {float((d / lim).max()):.3f}")
        assert bool((d <= lim).all())
    assert math.copysign(1, float(gelu_dev(torch.tensor(-300.0)))) == -1 and float(gelu_dev(torch.tensor(-300.0))) == 0    # the -0 result
    assert float(gelu_dev(torch.tensor(3e38))) == float(torch.tensor(3e38, dtype=torch.float32))


@pytest.mark.parametrize("order", ["matmul", "ksteps_reversed", "three_slices"])
def test_bound_accepts_fp32_emulation(case, order):
    inp, s, mag = case
    M, N = inp.M, inp.N
    acc = accumulate(inp, order)
    worst = {}
    for epi in range(6):
        for bias_on in (True, False):
            for row_on in ((True, False) if epi == R.EPI_BIAS_GATE_RES else (True,)):
                out = epilogue(epi, acc, inp, bias_on, row_on)
                assert bool(torch.isfinite(out.float()).all()), "nothing is infinite unless the formula says so"
                w = R.check(f"epi{epi}.bias{bias_on}.row{row_on}", *bound_of(epi, out, inp, s, mag, bias_on, row_on), tile=(160, 256))
                worst[epi] = max(worst.get(epi, 0.0), w)
    out = epilogue(0, acc, inp, True)
    # V^T (one batch of M tokens) and the split k | V^T output (k = the first 256 columns) hold the same values elsewhere
    vt = R.vt_of(out, M)
    worst["vt"] = R.check("vt", *R.bound(0, R.vt_rows(vt, M), s, mag, inp.K, inp.b))
    if N > 256:
        k, v = out[:, :256].clone(), R.vt_of(out[:, 256:], M)
        worst["split.k"] = R.check("split.k", *R.bound(0, k, s[:, :256], mag[:, :256], inp.K, inp.b[:256]))
        worst["split.vt"] = R.check("split.vt", *R.bound(0, R.vt_rows(v, M), s[:, 256:], mag[:, 256:], inp.K, inp.b[256:]))
    if N % 64 == 0:
        ss = (out.float() ** 2).reshape(M, -1, 64).sum(-1)
        worst["sumsq"] = R.check("sumsq", *R.sumsq_bound(ss, out))
    # the planted columns: y is the bias exactly, so the BIAS output is the bias and the activations are their extremes
    for c, v in inp.edge:
        assert bool((out[:, c] == torch.tensor(v).to(BF)).all())
    ge = epilogue(1, acc, inp, True)
    neg300 = [c for c, v in inp.edge if v == -300.0][0]
    assert bool((ge[:, neg300] == 0).all()) and bool(torch.signbit(ge[:, neg300]).all())
    print(f"{M}x{N}x{inp.K} {order}: worst d / bound " + ", ".join(f"{k}: {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def _rejected(name, d, bnd, results):
    bad = R.beyond(d, bnd)
    finite = bad & torch.isfinite(d)
    w = float((d / bnd)[finite].max()) if bool(finite.any()) else math.inf
    results[name] = (int(bad.sum()), w)
    assert int(bad.sum()) >= 1, f"{name}: the planted fault stays inside the bound"
    return bad


def test_bound_rejects_planted_faults(case):
    inp, s, mag = case
    M, N, K = inp.M, inp.N, inp.K
    acc = accumulate(inp, "matmul")
    a, w = inp.a.float(), inp.w.float()
    res = {}
    live = [c for c in range(N - 8) if c % 4 == 0 and not any(c <= e < c + 8 for e, _ in inp.edge)]
    c0 = live[len(live) // 2]                                          # a 4-column piece (and 8-column group) without planted columns

    # 1. the last K-step dropped for one 16 x 4 fragment of the ragged last row tile (32-row tiles)
    m0 = (M - 1) // 32 * 32
    rows = slice(m0, min(m0 + 16, M))
    acc2 = acc.clone()
    acc2[rows, c0:c0 + 4] -= a[rows, K - 64:] @ w[c0:c0 + 4, K - 64:].t()
    bad = _rejected("K-step dropped in one fragment", *bound_of(0, epilogue(0, acc2, inp, True), inp, s, mag, True), res)
    assert not bool(bad[:m0].any()) and not bool(bad[:, :c0].any()) and not bool(bad[:, c0 + 4:].any()), "and only there"

    # 2. bias taken from 4 columns to the left in the last 8 columns
    b2 = inp.b.clone()
    b2[N - 8:] = inp.b[N - 12:N - 4]
    _rejected("bias from 4 columns to the left", *bound_of(1, epilogue(1, acc, inp, True, bias=b2), inp, s, mag, True), res)

    # 3. residual of row M - 2 used for the last row
    r2 = inp.res.clone()
    r2[M - 1] = inp.res[M - 2]
    bad = _rejected("residual of the row above", *bound_of(4, epilogue(4, acc, inp, True, res=r2), inp, s, mag, True), res)
    assert not bool(bad[:M - 1].any())

    # 4. the gate row of another modulation row for one token
    g2 = R.gate_of(inp, True).clone()
    m = M // 2
    g2[m] = inp.gate[(int(inp.grow[m]) + 1) % inp.gate.shape[0]]
    bad = _rejected("gate row of another modulation row", *bound_of(3, epilogue(3, acc, inp, True, gate=g2), inp, s, mag, True), res)
    assert sorted(set(bad.nonzero()[:, 0].tolist())) == [m]

    # 5. bias added twice in one column group
    out = epilogue(0, acc, inp, True)
    out2 = out.clone()
    out2[:, c0:c0 + 8] = rbf32(acc[:, c0:c0 + 8] + inp.b[c0:c0 + 8].float() + inp.b[c0:c0 + 8].float()).to(BF)
    _rejected("bias added twice in one column group", *bound_of(0, out2, inp, s, mag, True), res)

    # 6. one V^T element stored one token late at a batch boundary (two batches of T tokens)
    M2 = M - M % 2
    T = M2 // 2
    vt = torch.full((2, N, T + 4), math.nan, dtype=BF)
    vt[:, :, :T] = R.vt_of(out[:M2], T)
    vt[1, c0, 0] = vt[0, c0, T - 1]                                    # token T - 1 lands where token T belongs
    bad = _rejected("V^T element one token late", *R.bound(0, R.vt_rows(vt, T), s[:M2], mag[:M2], K, inp.b), res)
    assert bad.nonzero().tolist() == [[T, c0]]

    # 7. one 8-column group of the ragged column tile left at its sentinel
    out7 = out.clone()
    out7[:, N - 8:] = math.nan
    bad = _rejected("8-column group left at its sentinel", *bound_of(0, out7, inp, s, mag, True), res)
    assert int(bad.sum()) == 8 * M

    for name, (n, wr) in res.items():
        print(f"{M}x{N}x{K} {name}: {n} elements beyond the bound, worst finite d / bound {wr:.1f}")


def test_frames_and_layouts():
    f = R.rows_frame(5, 8, 12, "cpu", lead=4)
    assert f.intact() and f.view.shape == (5, 8) and f.view.stride() == (12, 1) and f.view.storage_offset() == 4
    f.view.fill_(1.0)
    assert f.intact()
    f.buf[4 + 8] = 2.0                                                 # a pad column of row 0
    assert not f.intact()
    v = R.vt_frame(2, 3, 5, 8, "cpu")
    rows = torch.arange(30, dtype=torch.float32).reshape(10, 3).to(BF)
    v.view.copy_(R.vt_of(rows, 5))
    assert v.intact() and torch.equal(R.vt_rows(v.view, 5), rows)
    c = R.Frame((4, 2), (2, 1), "cpu", dtype=torch.float32, lead=0, sentinel=-7.0)
    c.view.zero_()
    assert c.intact()
    c.buf[8] = 0.0
    assert not c.intact()
    d, b = R.sumsq_bound(torch.tensor([[math.inf, 64.0]]), torch.cat([torch.full((1, 64), 3e38), torch.ones((1, 64))], 1).to(BF))
    assert d.tolist() == [[0.0, 0.0]] and R.check("sumsq", d, b) == 0.0
    assert R.worst(torch.tensor([math.nan]), torch.tensor([1.0])) == math.inf
    with pytest.raises(AssertionError, match="beyond the rounding bound"):
        R.check("nan", torch.tensor([[math.nan]]), torch.tensor([[1.0]]), tile=(160, 256))
