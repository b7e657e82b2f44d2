"""One float64 reference and one element-wise bound for the GEMM family (ltxk_gemm_bf16 in every launch form, the grouped
launch, ltxk_gemm_w8 / ltxk_gemm_w8a8), in the style of ref64.conv3d / conv3d_bound: everything runs on the device its inputs
live on and nothing is rounded.  tests/test_ref_gemm_cpu.py shows what the bound accepts and what it rejects.

``product(a, w)`` gives s = a @ w^T and mag = |a| @ |w|^T in float64 (products of bf16 values are exact, the sums carry
~2^-53).  ``bound(epi, out, s, mag, K, ...)`` gives (d, bound): d the distance of a stored bf16 output from the exact value
of that LTXK_EPI_* formula, bound the most an implementation that follows csrc/epilogue.h can be away.  Every term is one
rounding point of that file (u = 2^-24, ulp = the bf16 spacing, rbf = round to bf16):

  acc  = K u mag                          the fp32 accumulator against s, in ANY summation order (K-steps, slices, MFMA trees)
  y    = s + bias, ey = acc + u (|y| + acc)            the fp32 bias add; without a bias y = s, ey = acc
  eyb  = ey + 1/2 ulp(|y| + ey)                        the distance of yb = rbf(acc + bias) from y

  BIAS           |out - y|       <= 1/2 ulp(out) + ey                                    (out IS yb)
  BIAS_RES       |out - (r + y)| <= 1/2 ulp(out) + u (|r| + |y| + eyb) + eyb             bf16(r + yb): one fp32 add, one rounding
  SCALE_RES      z = alpha s, ez = |alpha| acc + u (|z| + |alpha| acc), ezb = ez + 1/2 ulp(|z| + ez):
                 |out - (r + z)| <= 1/2 ulp(out) + u (|r| + |z| + ezb) + ezb             bf16(r + rbf(alpha acc)); the bias is not read
  BIAS_GATE_RES  z = y g, ez = |g| eyb, e1 = ez + u (|z| + ez), ezb = e1 + 1/2 ulp(|z| + e1):
                 |out - (r + z)| <= 1/2 ulp(out) + u (|r| + |z| + ezb) + ezb             bf16(r + rbf(yb g))
  BIAS_GELU / BIAS_SILU   with f the float64 function, L its Lipschitz constant and E_ACT the relative error of the device's
                 fp32 evaluation (below):
                 |out - f(y)|    <= 1/2 ulp(out) + L eyb + E_ACT (|f(y)| + L eyb) + 2^-126
                 (|f(yb) - f(y)| <= L eyb; the device value is within E_ACT |f(yb)| <= E_ACT (|f(y)| + L eyb) of f(yb); 2^-126: a
                 subnormal result flushed to zero; the last rounding is half an ulp of what was stored).
  sumsq          |ss - sum out^2| <= 64 u sum out^2   against the squares of what was STORED: each of the 64 squares rounds once (u)
                 and their 63 fp32 additions, in any order, add at most 63 u; where the exact sum is beyond fp32 the statistic is +inf.

L.  The largest |f'| of each function, found on a float64 grid of step 2^-10 over [-40, 40] (test_ref_gemm_cpu.py repeats
the search): tanh-GELU 1.1290 at y = 1.42 -> L_GELU = 1.13; SiLU 1.0998 at y = 2.40 -> L_SILU = 1.1.  Beyond the grid both
derivatives are within 2^-50 of 0 or 1.

E_ACT.  csrc/common.h: gelu_tanh_f(x) = x * rcp(1 + exp2(t)), t = fma(c2, x*x, c1) * x with the literals c1 = -2.3022082f,
c2 = -0.10294324f; silu_f(x) = x * rcp(1 + exp2(c x)).  In units of u, relative:
  t      3 roundings (x*x, the fma, the product with x) + 2 constants (each the nearest fp32 of a decimal literal that is itself
         within 0.1 u of -2 sqrt(2/pi) log2 e and 0.044715 times that: 1.1 u each); the two terms of the fma share a sign, so
         nothing cancels: 5.2 u.  (SiLU: 1 rounding + 1 constant: 2.1 u.)
  exp2   v_exp_f32, 1 ulp = 2 u (common.h), and exp2(t (1 + e)) = exp2(t) (1 + t ln2 e ...): the error of t is amplified by
         |t| ln 2.  exp2 overflows at |t| = 128 (the result is then exactly -0 or x): 128 ln 2 * 5.2 u = 461.4 u.
  1 + .  the sum's own rounding, 1 u; the error of exp2(t) enters it with weight e / (1 + e) <= 1.
  rcp    v_rcp_f32, 1 ulp = 2 u.   The product with x: 1 u.
  sum    461.4 + 2 + 1 + 2 + 1 = 467.4 u, second-order terms < 0.1 u: E_ACT = 468 u < 2^-15.  Set to 2^-15 = 512 u.
(At |t| <= 16, where every output of weight lies, the same count gives 64 u.)  The premise of the 2^-126 term: no y in the
band where 1 + exp2(t) >= 2^126 and the reciprocal itself is subnormal (GELU: -10.3 < y < -9.9, SiLU: -88.8 < y < -87.3);
``premises`` asserts it of the inputs.

``inputs`` builds the operands of one (M, N, K) on the CPU generator (the CPU test and the GPU tests see the same data) and
plants EDGE COLUMNS: columns whose W row is zero and whose bias is one of EDGE_BIAS, so that y equals the bias exactly and the
activations' extremes - an overflowing exp2, the -0 results, 3e38 - pass through the GEMM epilogue itself.  ``Frame`` is an
output view inside a NaN frame that must survive; ``vt_rows`` turns a V^T buffer back into (M, N) rows."""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import torch

Tensor = torch.Tensor
F64 = torch.float64
BF = torch.bfloat16
U = 2.0 ** -24
FLUSH = 2.0 ** -126
FLT_MAX = 3.4028234663852886e38
L_GELU, L_SILU = 1.13, 1.1
E_ACT = 2.0 ** -15
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU, EPI_BIAS_GATE_RES, EPI_BIAS_RES, EPI_SCALE_RES = range(6)      # include/ltxk.h
# what an edge column's bias is, in the order they are planted (the widest first: a narrow N has room for few)
EDGE_BIAS = (3e38, -300.0, -12.0, -0.0, 300.0, 12.0, 0.0)
GATE_AT_3E38 = 0.5          # |gate| in the 3e38 column: rbf(yb * g) stays finite, as the formula then says


def ulp(x: Tensor) -> Tensor:
    """bf16 ulp of |x| (float64), floored at the smallest normal's."""
    m = x.abs().clamp_min(FLUSH)
    e = torch.floor(torch.log2(m))
    e = torch.where(torch.exp2(e) > m, e - 1, e)          # log2 of a value just below a power of two may round up
    return torch.exp2(e - 7)


def gelu64(y: Tensor) -> Tensor:
    """tanh-GELU in float64 as y / (1 + exp(-2 v)), v = sqrt(2/pi) (y + 0.044715 y^3): 0.5 (1 + tanh v) without its
    cancellation at negative y."""
    return y / (1.0 + torch.exp(-2.0 * math.sqrt(2.0 / math.pi) * (y + 0.044715 * y * y * y)))


def silu64(y: Tensor) -> Tensor:
    return y / (1.0 + torch.exp(-y))


def product(a: Tensor, w: Tensor):
    """(s, mag) = (a @ w^T, |a| @ |w|^T) in float64 on the operands' device; a (M, K) any row stride, w (N, K)."""
    a64, w64 = a.to(F64), w.to(F64)
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def bound(epi: int, out: Tensor, s: Tensor, mag: Tensor, K: int, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
          gate_rows: Optional[Tensor] = None, alpha: float = 1.0, acc_err: Optional[Tensor] = None):
    """(d, bound) of the module docstring for one stored output ``out`` (M, N) bf16 - a V^T buffer goes through ``vt_rows``
    first.  bias (N), resid (M, N), gate_rows (M, N) = gate[gate_row[m], n]: the operands as the launch got them, None where it
    got none; alpha as passed (rounded to fp32 here).  ``acc_err`` replaces K u mag where the accumulator is not a plain fp32
    sum of bf16 products (the fp8 forms)."""
    o = out.to(F64)
    acc = K * U * mag if acc_err is None else acc_err
    if epi == EPI_SCALE_RES:
        al = float(torch.tensor(alpha, dtype=torch.float32))
        z = al * s
        ez = abs(al) * acc + U * (z.abs() + abs(al) * acc)
    else:
        if bias is None:
            y, ey = s, acc
        else:
            y = s + bias.to(F64)
            ey = acc + U * (y.abs() + acc)
        if epi == EPI_BIAS:
            return (o - y).abs(), 0.5 * ulp(o) + ey
        eyb = ey + 0.5 * ulp(y.abs() + ey)
        if epi in (EPI_BIAS_GELU, EPI_BIAS_SILU):
            f, L = (gelu64(y), L_GELU) if epi == EPI_BIAS_GELU else (silu64(y), L_SILU)
            return (o - f).abs(), 0.5 * ulp(o) + L * eyb + E_ACT * (f.abs() + L * eyb) + FLUSH
        if epi == EPI_BIAS_RES:
            r = resid.to(F64)
            return (o - (r + y)).abs(), 0.5 * ulp(o) + U * (r.abs() + y.abs() + eyb) + eyb
        g = gate_rows.to(F64)
        z = y * g
        ez = g.abs() * eyb
        ez = ez + U * (z.abs() + ez)
    r = resid.to(F64)
    ezb = ez + 0.5 * ulp(z.abs() + ez)
    return (o - (r + z)).abs(), 0.5 * ulp(o) + U * (r.abs() + z.abs() + ezb) + ezb


def sumsq_bound(ss: Tensor, out: Tensor):
    """(d, bound) of a row statistic ss (M, P) fp32 against the squares of the stored ``out`` (M, 64 P); where the exact
    sum is certainly beyond fp32 the statistic must be +inf (d = 0 then, inf otherwise)."""
    sq = out.to(F64).pow(2).reshape(out.shape[0], -1, 64).sum(-1)
    got = ss.to(F64)
    over = sq * (1 - 64 * U) > FLT_MAX
    d = torch.where(over, torch.where(got == math.inf, 0.0, math.inf), (got - sq).abs())
    return d, 64 * U * sq + 1e-30


def beyond(d: Tensor, bnd: Tensor) -> Tensor:
    """Where an output is beyond its bound; a NaN (an output left at its sentinel, an inf - inf) counts."""
    return ~(d <= bnd)


def worst(d: Tensor, bnd: Tensor) -> float:
    """The largest d / bound; inf where an element is NaN."""
    r = d / bnd
    return float(torch.where(torch.isnan(r), torch.full_like(r, math.inf), r).max())


def check(name: str, d: Tensor, bnd: Tensor, tile=None) -> float:
    """Asserts that NO element is beyond its bound; returns the worst d / bound.  ``tile`` = (rows, columns) of the launch's
    tile: the message then names the tile and the 16 x 4 accumulator fragment of the first failure."""
    bad = beyond(d, bnd)
    n = int(bad.sum())
    w = worst(d, bnd)
    if n:
        i = tuple(int(v) for v in bad.nonzero()[0])
        where = ""
        if tile is not None and len(i) == 2:
            where = (f", tile ({i[0] // tile[0]}, {i[1] // tile[1]}) of {tile[0]} x {tile[1]}, row {i[0] % tile[0]} column {i[1] % tile[1]} "
                     f"of it, fragment rows {i[0] % tile[0] // 16 * 16}.. columns {i[1] % tile[1] // 4 * 4}..")
        raise AssertionError(f"{name}: {n} of {bad.numel()} outputs beyond the rounding bound, worst d / bound {w:.3f}, first at {i}{where}; "
                             f"rows {sorted(set(bad.nonzero()[:, 0].tolist()))[:8]}")
    return w


# ------------------------------------------------------------------------------------------------ frames and layouts

class Frame:
    """A strided view inside a flat buffer of sentinels: ``lead`` elements in front (8 bf16 = a 16-byte aligned view, 4 = one
    that is 8 bytes off), everything between the view's rows, and ``tail`` behind.  ``intact()`` after the launches: no
    element outside the view was written.  The sentinel is NaN unless given (a statistic's canary)."""

    def __init__(self, shape, strides, dev, dtype=BF, lead: int = 8, tail: int = 64, sentinel: float = math.nan):
        self.shape, self.strides, self.lead, self.sentinel = tuple(shape), tuple(strides), lead, sentinel
        span = 1 + sum((n - 1) * st for n, st in zip(shape, strides))
        self.buf = torch.full((lead + span + tail,), sentinel, dtype=dtype, device=dev)
        self.view = self.buf.as_strided(self.shape, self.strides, lead)

    def intact(self) -> bool:
        c = self.buf.clone()
        c.as_strided(self.shape, self.strides, self.lead).fill_(self.sentinel)
        return bool((torch.isnan(c) if math.isnan(self.sentinel) else c == self.sentinel).all())


def rows_frame(M: int, N: int, ld: int, dev, lead: int = 8, **kw) -> Frame:
    """(M, N) row-major output with row stride ld."""
    return Frame((M, N), (ld, 1), dev, lead=lead, **kw)


def vt_frame(nb: int, rows: int, T: int, ld: int, dev, lead: int = 8) -> Frame:
    """(nb, rows, T) V^T output with row stride ld >= T: the pad columns belong to the frame."""
    return Frame((nb, rows, T), (rows * ld, ld, 1), dev, lead=lead)


def vt_rows(vt: Tensor, T: int) -> Tensor:
    """vt (nb, N, >= T) with vt[b, n, t] = row b T + t, column n -> the (nb T, N) rows."""
    return vt[:, :, :T].permute(0, 2, 1).reshape(-1, vt.shape[1])


def vt_of(rows: Tensor, T: int) -> Tensor:
    """The inverse: (M, N) rows -> (M / T, N, T)."""
    return rows.reshape(-1, T, rows.shape[1]).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------ inputs

def edge_columns(N: int):
    """[(column, bias)]: min(7, (N - 8) / 8) planted columns, none in the last 8 (those stay live for the ragged edge) - N = 8
    has room for none.  Spread over the width, each at another offset inside its 4-column piece."""
    n = max(0, min(len(EDGE_BIAS), (N - 8) // 8))
    return [((j * (N - 8)) // n + (3 * j + 1) % 8, EDGE_BIAS[j]) for j in range(n)]


def inputs(M: int, N: int, K: int, seed: int, dev="cpu", gate_rows: int = 3) -> SimpleNamespace:
    """The operands of one case, drawn on the CPU generator and moved to ``dev``: a (M, K) with row stride K + 8, resid (M, N)
    with row stride N + 4 (the pads are NaN: nothing may read them), w (N, K) ~ K^-1/2, bias (N) ~ 0.1, the gate as columns
    [N, 2N) of a (gate_rows, 2N) table (gate_stride = 2N), gate_row (M) int32, alpha = 0.8; edge columns planted."""
    g = torch.Generator().manual_seed(seed)
    a_buf = torch.full((M, K + 8), math.nan, dtype=BF)
    a_buf[:, :K] = torch.randn((M, K), generator=g).to(BF)
    w = (torch.randn((N, K), generator=g) * K ** -0.5).to(BF)
    b = (torch.randn(N, generator=g) * 0.1).to(BF)
    r_buf = torch.full((M, N + 4), math.nan, dtype=BF)
    r_buf[:, :N] = torch.randn((M, N), generator=g).to(BF)
    tab = torch.randn((gate_rows, 2 * N), generator=g).to(BF)
    grow = torch.randint(0, gate_rows, (M,), generator=g, dtype=torch.int32)
    edge = edge_columns(N)
    for c, v in edge:
        w[c] = 0
        b[c] = v
        if abs(v) > 1e38:
            tab[:, N + c] = torch.where(tab[:, N + c] < 0, -GATE_AT_3E38, GATE_AT_3E38).to(BF)
    a_buf, w, b, r_buf, tab, grow = (t.to(dev) for t in (a_buf, w, b, r_buf, tab, grow))
    return SimpleNamespace(M=M, N=N, K=K, a=a_buf[:, :K], w=w, b=b, res=r_buf[:, :N], gate_tab=tab, gate=tab[:, N:], gate_stride=2 * N,
                           grow=grow, alpha=0.8, edge=edge)


def gate_of(inp, row_on: bool) -> Tensor:
    """The (M, N) gate values of a launch: gate[gate_row[m]] with a gate_row, row 0 for every token without one."""
    return inp.gate[inp.grow.long()] if row_on else inp.gate[0].expand(inp.M, inp.N)


def premises(inp, s: Tensor, mag: Tensor) -> None:
    """What the inputs rest on: the planted columns are exact (s = mag = 0 there, y IS the bias), everything is finite, no
    gated product overflows bf16, and no pre-activation lies in the band where the device's reciprocal is subnormal."""
    assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(inp.a.float()).all()) and bool(torch.isfinite(inp.res.float()).all())
    cols = [c for c, _ in inp.edge]
    assert len(set(cols)) == len(cols) and all(0 <= c < inp.N - 8 for c in cols)
    if cols:
        assert float(s[:, cols].abs().max()) == 0.0 and float(mag[:, cols].abs().max()) == 0.0, "an edge column's product is not exactly 0"
        assert inp.b[cols].tolist() == torch.tensor([v for _, v in inp.edge]).to(BF).tolist(), "an edge column's bias was not planted"
    for bias in (inp.b.to(F64), None):
        y = s if bias is None else s + bias
        assert float((y.abs().unsqueeze(0) * inp.gate.to(F64).abs().unsqueeze(1)).max()) < 3.3e38, "a gated product overflows bf16"
        assert not bool(((y > -10.3) & (y < -9.9)).any()) and not bool(((y > -88.8) & (y < -87.3)).any()), \
            "a pre-activation in the band where rcp(1 + exp2(t)) is subnormal"
