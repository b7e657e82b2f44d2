"""The text stage on the GPU: its kernels (csrc/text_ops.hip; q/k norm + RoPE: csrc/elementwise.hip) one by one against float64 on the same inputs, then
text_connector.TextConnector as a whole against tests/ref_text.py, then generate_video through the Gemma-hidden-state route.

Bounds are written out from the arithmetic, with u = 2^-24 (fp32 unit roundoff) and 2^-8 (bf16 unit roundoff: 8 significant
bits); a sum of fp32 additions in which a term passes through at most k additions has |error| <= g(k) * sum|terms| with
g(k) = k u / (1 - k u), whatever the order.  Every check goes to the parity ledger."""
import math

import numpy as np
import parity
import pytest
import torch

import ref_text as RT
from test_rowops_gpu import _sent_bf16, _untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -24
UB = 2.0 ** -8


def _gam(k):
    return k * U / (1 - k * U)


def _hidden(L, B, T, D, seed):
    """Hidden-state stand-ins: per-layer scale and offset (a non-zero mean makes the long sum a real test of the reduction)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(L, B, T, D, generator=g)
    x = x * (1.0 + torch.arange(L).float().reshape(L, 1, 1, 1)) + torch.linspace(-2, 3, L).reshape(L, 1, 1, 1)
    return x.to(BF)


def _tables(counts, T, dev):
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    start = torch.tensor([T - c for c in counts], dtype=torch.int32, device=dev)
    row0 = torch.tensor([sum(counts[:b]) for b in range(len(counts))], dtype=torch.int32, device=dev)
    return start, cnt, row0


def _stats64(x, counts):
    """float64 (sum, min, max, sum|x|) per (b, l); zeros for an empty row."""
    L, B, T, D = x.shape
    out = torch.zeros(B, L, 4, dtype=F64)
    for b, c in enumerate(counts):
        if c:
            v = x[:, b, T - c:].double().reshape(L, -1)
            out[b] = torch.stack([v.sum(1), v.amin(1), v.amax(1), v.abs().sum(1)], 1)
    return out


STAT_CASES = [((5, 2, 256, 384), (256, 37)), ((5, 2, 256, 384), (1, 0)), ((2, 1, 1024, 3840), (1024,))]
_IDS = ["5x2x256x384-256_37", "5x2x256x384-1_0", "2x1x1024x3840-1024"]


@pytest.fixture(scope="module")
def stat_inputs():
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = _hidden(*shape, seed=sum(shape))
        return cache[shape]
    return get


@pytest.mark.parametrize("shape,counts", STAT_CASES, ids=_IDS)
def test_masked_layer_stats(dev, stat_inputs, shape, counts):
    """min and max exact; |sum - sum64| <= g(depth) * sum|x| with depth = ops.layer_stats_depth(count, D), the longest chain of
    additions of the two-stage reduction (30 + 17 at 1024 x 3840); an empty row gives {0, 0, 0}; a launch that holds one batch
    row alone gives that row the same bits."""
    from mlx_video_amd import ops
    L, B, T, D = shape
    x = stat_inputs(shape)
    xd = x.to(dev)
    start, cnt, _ = _tables(counts, T, dev)
    got = ops.masked_layer_stats(xd, start, cnt)
    torch.cuda.synchronize()
    assert got.shape == (B, L, 3) and got.dtype == torch.float32
    ref = _stats64(x, counts)
    g = got.cpu().double()
    assert torch.equal(g[..., 1], ref[..., 1]) and torch.equal(g[..., 2], ref[..., 2]), "min / max are not exact"
    worst = 0.0
    for b, c in enumerate(counts):
        if c == 0:
            assert not bool(got[b].any()), "an empty row must write zeros"
            continue
        bound = _gam(ops.layer_stats_depth(c, D)) * ref[b, :, 3]
        worst = max(worst, float(((g[b, :, 0] - ref[b, :, 0]).abs() / bound).max()))
    parity.auto(worst, 1.0, tag="sum_err_over_bound")
    for b in range(B):                      # the same rows in a launch of another B: identical bits
        alone = ops.masked_layer_stats(xd[:, b:b + 1], start[b:b + 1].contiguous(), cnt[b:b + 1].contiguous())
        assert torch.equal(alone[0], got[b]), f"batch row {b}: statistics depend on what shares the launch"
    if B == 2:                              # and with the rows swapped
        sw = ops.masked_layer_stats(xd.flip(1).contiguous(), start.flip(0).contiguous(), cnt.flip(0).contiguous())
        assert torch.equal(sw.flip(0), got)


@pytest.mark.parametrize("shape,counts", STAT_CASES, ids=_IDS)
def test_layer_norm_compact(dev, stat_inputs, shape, counts):
    """Per element against y = 8 (x - m) / (r + 1e-6), m = S / (n + 1e-6), in float64 on the same inputs.  The kernel computes
    m^ = fl(S^ / fl(n + 1e-6)) from the fp32 sum S^ of ltxk_masked_layer_stats (|S^ - S| <= g(depth) sum|x|): |m^ - m| <= em =
    g(depth) sum|x| / n + 3u |m|.  Then fl(x - m^), an exact scaling by 8, fl(fl(max - min) + 1e-6) and one division: four
    roundings on top of the shifted mean, |y32 - y| <= e32 = 8 em / (r + 1e-6) + 5u (|y| + 8 em / (r + 1e-6)); and one rounding
    to bf16:  |out - y| <= 2^-8 |y| + (1 + 2^-8) e32.
    The matrix is compact and layer-major: row row0[b] + t, column l*D + d; rows past the last valid token and columns past
    L*D keep their sentinel."""
    from mlx_video_amd import ops
    L, B, T, D = shape
    x = stat_inputs(shape)
    xd = x.to(dev)
    start, cnt, row0 = _tables(counts, T, dev)
    rows = sum(counts)
    stats = ops.masked_layer_stats(xd, start, cnt)
    out = _sent_bf16((rows + 3, L * D + 8), dev)
    ops.layer_norm_compact(xd, start, cnt, row0, stats, out, rows)
    torch.cuda.synchronize()
    assert _untouched(out[rows:]) and _untouched(out[:, L * D:]), "rows past the valid tokens or columns past L*D were written"
    got = out[:rows, :L * D].cpu().double()
    assert not bool(torch.isnan(got).any()), "valid rows left unwritten"
    ref = _stats64(x, counts)
    worst, r = 0.0, 0
    for b, c in enumerate(counts):
        if c == 0:
            continue
        n = c * D
        S, mn, mx, sabs = (ref[b, :, i].reshape(L, 1, 1) for i in range(4))
        m = S / (n + 1e-6)
        den = (mx - mn) + 1e-6
        xv = x[:, b, T - c:].double()                                       # (L, c, D)
        y = 8 * (xv - m) / den
        em = _gam(ops.layer_stats_depth(c, D)) * sabs / n + 3 * U * m.abs()
        e32 = 8 * em / den + 5 * U * (y.abs() + 8 * em / den)
        bound = UB * y.abs() + (1 + UB) * e32
        g = got[r:r + c].reshape(c, L, D).permute(1, 0, 2)                  # column l*D + d of row r + t
        worst = max(worst, float(((g - y).abs() / bound).max()))
        r += c
    parity.auto(worst, 1.0, tag="err_over_bound")


def _bf16_bits_rne(y):
    """Bit patterns (0..65535, int32) of float64 -> bf16 round-to-nearest-even.  torch rounds float64 -> float32 -> bf16; the two
    roundings differ from one only when the float32 lands exactly on a bf16 tie the float64 was not on, which is undone here."""
    f = y.to(torch.float32)
    fb = f.view(torch.int32)
    bits = f.to(BF).view(torch.int16).to(torch.int32) & 0xFFFF
    tie = ((fb & 0xFFFF) == 0x8000) & torch.isfinite(f)
    trunc = (fb >> 16) & 0xFFFF
    bits = torch.where(tie & (y.abs() > f.double().abs()), trunc + 1, bits)
    bits = torch.where(tie & (y.abs() < f.double().abs()), trunc, bits)
    return bits


def _ordered(bits):
    """bf16 bit pattern -> an integer that counts representable values along the real line (+0 and -0 coincide)."""
    mag = bits & 0x7FFF
    return torch.where((bits & 0x8000) != 0, -mag, mag)


def test_gelu_erf_all_bf16_patterns(dev):
    """Every bf16 bit pattern.  NaN stays NaN, +inf stays +inf, -inf gives NaN (-inf * 0, as the formula does in IEEE
    arithmetic); every finite result is within one bf16 ulp of the correctly rounded float64 value of
    x (1 + erf(x / sqrt 2)) / 2 (evaluated as (x/2) erfc(-x / sqrt 2): the same function, without the cancellation that costs
    float64 its digits below x = -6).  How many inputs are not correctly rounded is recorded."""
    from mlx_video_amd import ops
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = pat.view(BF)
    xd = x.to(dev).clone()
    ops.gelu_erf_(xd)
    torch.cuda.synchronize()
    got = xd.cpu()
    x64 = x.double()
    y64 = 0.5 * x64 * torch.special.erfc(-x64 / math.sqrt(2.0))
    nan_ref = torch.isnan(y64)
    assert torch.equal(torch.isnan(got), nan_ref), "NaN patterns differ from IEEE evaluation of the formula"
    assert bool(nan_ref[torch.isnan(x)].all()) and bool(nan_ref[x == float("-inf")].all())
    inf_ref = torch.isinf(y64)
    assert torch.equal(torch.isinf(got), inf_ref) and torch.equal(got[inf_ref].double(), y64[inf_ref])
    fin = torch.isfinite(y64)
    gb = got.view(torch.int16).to(torch.int32) & 0xFFFF
    rb = _bf16_bits_rne(y64)
    d = (_ordered(gb) - _ordered(rb)).abs()[fin]
    # a result of exactly zero keeps the sign of the formula's zero
    zero = fin & (y64 == 0)
    assert torch.equal(gb[zero], rb[zero]), "signed zeros differ"
    parity.check("text.gelu_erf.max_bf16_ulps_from_correctly_rounded", float(d.max()), 1.0)
    parity.check("text.gelu_erf.inputs_not_correctly_rounded", float((d > 0).sum()), 65536.0, note="recorded, not gated")


# (D, H, M).  H = 33 is the first head count past the 4-pass instance of the q/k kernel (pass 4 holds 8 live items; D = 4224 is
# no multiple of 512); H = 64 fills all 8 passes and D = 8192 is the widest row ltxk_rmsnorm_rows takes.
ROW_CASES = [(3840, 30, 70), (384, 3, 37), (4224, 33, 5), (8192, 64, 3)]
ROW_IDS = ["3840x70", "384x37", "4224x5", "8192x3"]


@pytest.mark.parametrize("D,H,M", ROW_CASES, ids=ROW_IDS)
def test_rmsnorm_rows(dev, D, H, M):
    """y = x / sqrt(mean(x^2) + eps) in float64.  The kernel: squares of bf16 values are exact in fp32; their sum passes a term
    through k = 8 ceil(D/512) + 6 additions (relative error g(k), all terms positive), then / D, + eps and v_rsq_f32 (1 ulp =
    2u): the factor is off by at most (g(k) + 2u) / 2 + 2u relative; one multiplication, one rounding to bf16:
    |out - y| <= 2^-8 |y| + (1 + 2^-8) (g(k)/2 + 5u) |y|.  Rows past M and columns past D of the padded buffers stay."""
    from mlx_video_amd import ops
    g = torch.Generator().manual_seed(D + M)
    x = (torch.randn(M, D, generator=g) * torch.logspace(-2, 2, M).reshape(M, 1)).to(BF)
    xb = _sent_bf16((M + 2, D + 8), dev)
    xb[:M, :D] = x.to(dev)
    yb = _sent_bf16((M + 2, D + 16), dev)
    ops.rmsnorm_rows(xb[:M, :D], 1e-6, out=yb[:M, :D])
    torch.cuda.synchronize()
    assert _untouched(yb[M:]) and _untouched(yb[:, D:]) and _untouched(xb[M:]) and _untouched(xb[:, D:])
    x64 = x.double()
    y = x64 / torch.sqrt((x64 * x64).mean(1, keepdim=True) + 1e-6)
    k = 8 * -(-D // 512) + 6
    bound = UB * y.abs() + (1 + UB) * (_gam(k) / 2 + 5 * U) * y.abs()
    err = (yb[:M, :D].cpu().double() - y).abs()
    assert bool((err[bound == 0] == 0).all())
    parity.auto(float((err / bound.clamp_min(1e-300)).max()), 1.0, tag="err_over_bound")
    same = xb[:M, :D].clone()
    ops.rmsnorm_rows(same, 1e-6, out=same)                                  # in place
    assert torch.equal(same, yb[:M, :D])


@pytest.mark.parametrize("D,H,M", ROW_CASES, ids=ROW_IDS)
def test_qknorm_rope_1d(dev, D, H, M):
    """In float64 on the same inputs and tables: n = x w / sqrt(mean(x^2) + eps) per segment, o1 = n1 c - n2 s, o2 = n2 c + n1 s.
    The kernel rounds the normalised value to bf16 first (the reference's q_norm returns a bf16 array): n^ = n (1 + rho'),
    |rho'| <= rho = 2^-8 + (1 + 2^-8)(g(k)/2 + 5u) with k = 16 ceil(8H/64) + 6 additions in the sum of squares and two
    multiplications; the rotation in fp32 adds u per product and u for the subtraction, all against mag = |n1 c| + |n2 s|; then
    one rounding to bf16:  |out - o| <= 2^-8 |o| + (1 + 2^-8)(rho + 3u (1 + rho)) mag.
    Head counts 30, 3 and 33 are no multiple of 4, 33 and 64 take the 8-pass instance of the kernel; where T = 32 < M positions
    wrap; rows past M and columns past 2D stay."""
    from mlx_video_amd import ops
    from mlx_video_amd.text_connector import rope_table_1d
    T = 32
    g = torch.Generator().manual_seed(D + M + 1)
    x = (torch.randn(M, 2 * D, generator=g) * torch.logspace(-1, 1, M).reshape(M, 1)).to(BF)
    w = (1.0 + 0.2 * torch.randn(2, D, generator=g)).to(BF)
    cos, sin = rope_table_1d(T, H)
    buf = _sent_bf16((M + 2, 2 * D + 8), dev)
    buf[:M, :2 * D] = x.to(dev)
    ops.qknorm_rope_1d(buf[:M], D, w.to(dev), cos.to(dev), sin.to(dev), T, H, 1e-6)
    torch.cuda.synchronize()
    assert _untouched(buf[M:]) and _untouched(buf[:, 2 * D:]), "rows past M or columns past 2D were written"
    got = buf[:M, :2 * D].cpu().double().reshape(M, 2, H, 2, 64)
    x64 = x.double().reshape(M, 2, D)
    n = x64 / torch.sqrt((x64 * x64).mean(2, keepdim=True) + 1e-6) * w.double().reshape(1, 2, D)
    n = n.reshape(M, 2, H, 2, 64)
    pos = torch.arange(M) % T
    c = cos.double()[:, pos].permute(1, 0, 2).reshape(M, 1, H, 64)          # (H,T,64) -> row m at position m % T
    s = sin.double()[:, pos].permute(1, 0, 2).reshape(M, 1, H, 64)
    n1, n2 = n[:, :, :, 0], n[:, :, :, 1]
    o = torch.stack([n1 * c - n2 * s, n2 * c + n1 * s], 3)
    mag = torch.stack([(n1 * c).abs() + (n2 * s).abs(), (n2 * c).abs() + (n1 * s).abs()], 3)
    k = 16 * -(-8 * H // 64) + 6
    rho = UB + (1 + UB) * (_gam(k) / 2 + 5 * U)
    bound = UB * o.abs() + (1 + UB) * (rho + 3 * U * (1 + rho)) * mag
    err = (got - o).abs()
    assert bool((err[bound == 0] == 0).all())
    parity.auto(float((err / bound.clamp_min(1e-300)).max()), 1.0, tag="err_over_bound")


@pytest.mark.parametrize("M,D", [(5, 8), (5, 264), (3, 3840), (2, 8192)])
def test_rmsnorm_entry_points_share_bits(dev, M, D):
    """ltxk_rmsnorm_rows and ltxk_rmsnorm_weight_rows launch the two instances of one kernel body: with a zero weight 1 + 0 and the multiplication by 1.0f
    are exact, so the two give the same bits.  Strided views inside sentinel borders, which stay."""
    from mlx_video_amd import ops
    g = torch.Generator().manual_seed(7 * D + M)
    x = (torch.randn(M, D, generator=g) * torch.logspace(-2, 2, M).reshape(M, 1)).to(BF)
    xb = _sent_bf16((M + 2, D + 8), dev)
    xb[:M, :D] = x.to(dev)
    ya, yb = _sent_bf16((M + 2, D + 16), dev), _sent_bf16((M + 2, D + 16), dev)
    ops.rmsnorm_rows(xb[:M, :D], 1e-6, out=ya[:M, :D])
    ops.rmsnorm_weight_rows(xb[:M, :D], torch.zeros(D, dtype=BF, device=dev), 1e-6, out=yb[:M, :D])
    torch.cuda.synchronize()
    for y in (ya, yb):
        assert _untouched(y[M:]) and _untouched(y[:, D:])
    assert not bool(torch.isnan(ya[:M, :D]).any())
    assert torch.equal(ya[:M, :D].view(torch.int16), yb[:M, :D].view(torch.int16))


@pytest.mark.parametrize("H", [4, 12, 32])
def test_qknorm_entry_points_share_bits(dev, H):
    """ltxk_qknorm_rope_1d and ltxk_qknorm_rope at nseg = 2 launch one kernel: the same bits on the head counts both take.
    M = 5 rows at T = 3 positions, so positions wrap; rows past M and columns past 2D stay."""
    from mlx_video_amd import ops
    from mlx_video_amd.text_connector import rope_table_1d
    M, T, D = 5, 3, 128 * H
    g = torch.Generator().manual_seed(H)
    x = (torch.randn(M, 2 * D, generator=g) * torch.logspace(-1, 1, M).reshape(M, 1)).to(BF)
    w = (1.0 + 0.2 * torch.randn(2, D, generator=g)).to(BF).to(dev)
    cos, sin = (t.to(dev) for t in rope_table_1d(T, H))
    a, b = _sent_bf16((M + 2, 2 * D + 8), dev), _sent_bf16((M + 2, 2 * D + 8), dev)
    a[:M, :2 * D] = x.to(dev)
    b[:M, :2 * D] = x.to(dev)
    ops.qknorm_rope_1d(a[:M], D, w, cos, sin, T, H, 1e-6)
    ops.qknorm_rope(b[:M], 2, D, w, cos, sin, T, H, 1e-6)
    torch.cuda.synchronize()
    for y in (a, b):
        assert _untouched(y[M:]) and _untouched(y[:, 2 * D:])
    assert not bool(torch.isnan(a[:M, :2 * D]).any()) and not torch.equal(a[:M, :2 * D].cpu(), x)
    assert torch.equal(a[:M, :2 * D].view(torch.int16), b[:M, :2 * D].view(torch.int16))


def test_connector_assemble(dev):
    """Bit-exact against torch indexing: counts 0, 1, 37 and T."""
    from mlx_video_amd import ops
    T, D, R = 256, 384, 128
    counts = [0, 1, 37, T]
    g = torch.Generator().manual_seed(5)
    rows = sum(counts)
    feat = torch.randn(rows, D + 8, generator=g).to(BF).to(dev)[:, :D]       # a row stride above D
    reg = torch.randn(R, D, generator=g).to(BF).to(dev)
    _, cnt, row0 = _tables(counts, T, dev)
    out = ops.connector_assemble(feat, reg, row0, cnt, len(counts), T)
    torch.cuda.synchronize()
    want = reg.repeat(T // R, 1).unsqueeze(0).repeat(len(counts), 1, 1)
    r = 0
    for b, c in enumerate(counts):
        want[b, :c] = feat[r:r + c]
        r += c
    assert out.shape == (len(counts), T, D) and torch.equal(out, want)
    none = ops.connector_assemble(None, reg, row0[:1].contiguous(), cnt[:1].contiguous(), 1, T)
    assert torch.equal(none[0], want[0])


# ------------------------------------------------------------------------------------------- the whole stage
STAGE = dict(D=384, L=5, layers=2, R=128)
STAGE_T = 256


@pytest.fixture(scope="module")
def stage(dev):
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    W = random_connector_weights("cpu", seed=23, **STAGE)
    tc = TextConnector({k: v.to(dev) for k, v in W.items()})
    assert (tc.D, tc.H, tc.R, tc.L, len(tc.blocks)) == (384, 3, 128, 5, 2)
    return W, tc


def _mask(counts, T):
    return torch.stack([torch.cat([torch.zeros(T - c, dtype=torch.int64), torch.ones(c, dtype=torch.int64)]) for c in counts])


@pytest.mark.parametrize("counts", [(256, 37), (1, 0)], ids=["256_37", "1_0"])
def test_whole_stage_against_float64(dev, stage, counts):
    """Relative L2 of TextConnector's output to ref_text's float64 policy, held to 2 x the relative L2 of ref_text's bf16 policy
    (the reference's own arithmetic) to the same truth on the same inputs: the two round at different points, not at fewer (the
    attention kernel rounds its probabilities to bf16, the reference does not; the kernels keep their statistics in fp32, the
    reference does not), and 2 covers two independent errors of equal size (sqrt 2) with headroom - the factor the pins use."""
    W, tc = stage
    hs = _hidden(STAGE["L"], 2, STAGE_T, STAGE["D"], seed=100 + counts[0])
    mask = _mask(counts, STAGE_T)
    out = tc(hs.to(dev), mask.to(dev))
    torch.cuda.synchronize()
    assert out.shape == (2, STAGE_T, STAGE["D"]) and out.dtype == BF and bool(torch.isfinite(out).all())
    ref = RT.text_stage(hs, mask, W, RT.P64)
    ref_bf = RT.text_stage(hs, mask, W, RT.PBF)
    tag = "_".join(map(str, counts))
    ref_err = parity.check(f"text.stage_{tag}.ref_bf16_policy_rel_l2", parity.rel_l2(ref_bf, ref), 5e-2,
                           note="the reference's own distance to float64: the yardstick, not a result")
    parity.check(f"text.stage_{tag}.rel_l2", parity.rel_l2(out, ref), 2.0 * ref_err)
    # the list form of the input is the stack
    again = tc([h for h in hs.to(dev)], mask.to(dev))
    assert torch.equal(again, out)
    if counts[1] == 0:
        # a row without a valid token is the connector run on pure registers, whatever shares its batch
        alone = tc(hs[:, 1:].to(dev), mask[1:].to(dev))
        assert torch.equal(alone[0], out[1]), "the count-0 row differs from the connector on pure registers"
        regs = tc.connect(tc.registers.repeat(STAGE_T // tc.R, 1).unsqueeze(0).clone())
        assert torch.equal(regs[0], out[1])


def test_generate_video_through_gemma_route(dev):
    """generate_video on the tiny pipeline of tests/test_pipeline_gpu.py (context width 256) fed Gemma hidden states + masks
    and a TextConnector gives the frames, bit for bit, of the call fed that connector's output as prompt_embeds."""
    from mlx_video_amd.generate import PipelineType, generate_video
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    from test_pipeline_gpu import _Noise, _mods
    m = _mods(dev)
    L, T, D = 3, 64, 256
    tc = TextConnector({k: v.to(dev) for k, v in random_connector_weights("cpu", D=D, L=L, layers=1, R=32, seed=29).items()})
    hs_pos, hs_neg = _hidden(L, 1, T, D, seed=61), _hidden(L, 1, T, D, seed=62)
    m_pos, m_neg = _mask((23,), T), _mask((9,), T)
    common = dict(prompt="x", pipeline=PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
                  transformer=m["transformer"], vae_decoder=m["vae_decoder"], compile_step=True, cfg_batch=True, device=dev)
    a = generate_video(gemma_hidden_states=hs_pos, gemma_attention_mask=m_pos, negative_gemma_hidden_states=[h for h in hs_neg],
                       negative_gemma_attention_mask=m_neg[0], text_connector=tc, noise_fn=_Noise(7, dev), **common)
    emb = tc(torch.cat([hs_pos, hs_neg], 1).to(dev), torch.cat([m_pos, m_neg], 0).to(dev))
    assert emb.shape == (2, T, D)
    b = generate_video(prompt_embeds=emb[0:1], negative_prompt_embeds=emb[1:2], noise_fn=_Noise(7, dev), **common)
    assert a.shape == (9, 128, 128, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    # prompt_embeds wins when both are given
    c = generate_video(prompt_embeds=emb[0:1], negative_prompt_embeds=emb[1:2], gemma_hidden_states=hs_neg, gemma_attention_mask=m_neg,
                       text_connector=tc, noise_fn=_Noise(7, dev), **common)
    assert np.array_equal(c, b)
    with pytest.raises(ValueError, match="without a text connector"):
        generate_video(gemma_hidden_states=hs_pos, gemma_attention_mask=m_pos, noise_fn=_Noise(7, dev), **common)
