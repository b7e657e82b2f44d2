"""Row and elementwise kernels of the DiT step at their edge shapes, against the float64 references of tests/ref64.py.

The shapes are picked to reach the kernels' tails: ROWS_PER_BLOCK = 4 rows per workgroup (M % 4 != 0, M = 1),
MAX_CHUNKS = 16 chunks of 512 (D = 8192), NP = D/64 > 64 partials (the second pass of the `_ss` reduction), 8-head passes
that leave lanes idle (H = 12, 20, 28), 64-wide grids along S (S % 64 != 0), 8-element vectors with a partial last
workgroup.  Every output is written into a buffer padded with NaN sentinels (rows past M, columns past the operated width
inside a larger ld, the tail of a flat buffer) that must survive bit for bit.

Bounds: ``max_ulps`` bf16 ulps at max(|ref|, mag), where mag is the size of the terms an output inherits a rounding from
(ref64 returns it); 1 for a single fp32 expression rounded once, 2 where an earlier bf16 rounding point can flip and
carry into the next op, 0 for exact maps and bit-identical launch forms.  ``max_frac``: fraction of elements off at all.

Beside that rule every output is held, element by element and with no exempt share, to the admissible bf16 interval of
tests/ref_rows.py (``_within``): a float64 interval carried through the kernel's own chain of operations.  The inputs come
from ref_rows' builders, which tests/test_ref_rows_cpu.py shares."""
import ctypes

import numpy as np
import parity
import pytest
import torch

import ref64 as R
import ref_rows as RR

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT16 = 0x7FA5                  # a bf16 NaN payload no kernel produces
SENT32 = 0x7FA5A5A5              # the same for fp32 outputs


def _ops():
    from mlx_video_amd import ops
    return ops


def _lib():
    from mlx_video_amd import _lib
    return _lib


_g = RR.gen


def _sent_bf16(shape, dev):
    return torch.full(shape, SENT16, dtype=torch.int16, device=dev).view(BF)


def _sent_f32(shape, dev):
    return torch.full(shape, SENT32, dtype=torch.int32, device=dev).view(torch.float32)


def _untouched(t):
    """True if every element of t still holds the sentinel bits."""
    t = t.detach()
    if t.dtype == BF:
        return bool((t.contiguous().view(torch.int16) == SENT16).all())
    return bool((t.contiguous().view(torch.int32) == SENT32).all())


def _close(got, ref, *, max_ulps, max_frac, mag=None, tag=""):
    """ref64's comparator, with both measured numbers recorded in the parity ledger."""
    ulps, frac = R.bf16_stats(got, ref, mag)
    parity.auto(ulps, max_ulps, tag=f"{tag}ulps")
    parity.auto(frac, max_frac, tag=f"{tag}frac")
    R.assert_bf16_close(got, ref, max_ulps=max_ulps, max_frac=max_frac, mag=mag, what=tag)


def _within(got, iv, *, cap=RR.AMBIGUOUS_CAP, tag=""):
    """ref_rows' comparator: every element inside its admissible bf16 interval; the share of elements with two admissible
    values (a property of the reference alone, capped in test_ref_rows_cpu.py) goes into the ledger."""
    (n, first), amb, widest = RR.within(got, iv)
    parity.auto(amb, cap, tag=f"{tag}ambiguous")
    assert n == 0, (f"{tag}: {n} elements outside their admissible bf16 interval, the first at flat index {first} "
                    f"(widest interval {widest} bf16 steps)")


def _ulp_f32(m):
    m = m.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(m)) - 23)


# ------------------------------------------------------------------------------------------- self-reducing row norms
def _norm_case(dev, ln, M, D, mode, seed, special_rows=False, small_mean=False):
    ops = _ops()
    inp = RR.norm_inputs(ln, M, D, mode, seed, special_rows, small_mean)
    x, sc, sh = inp.x, inp.sc, inp.sh
    y = _sent_bf16((M + 3, D), dev)
    if mode == "scale_shift":                   # one modulation row, no row map
        td = inp.tab.to(dev)
        ops_args = (td[:, D:], td[:, :D], inp.stride, None)
    elif mode == "mod_row":                     # U = 3 rows of a (U, 6D) table, picked per token
        td = inp.tab.to(dev)
        ops_args = (td[:, D:2 * D], td[:, :D], inp.stride, inp.rows.to(dev))
    else:
        ops_args = (None, None, 0, None)
    f = ops.layernorm_modulate if ln else ops.rmsnorm_modulate
    f(x.to(dev), 1e-6, *ops_args, out=y[:M])
    torch.cuda.synchronize()
    ref, mag = R.norm_modulate(x, R.f32(1e-6), sc, sh, layernorm=ln)
    assert _untouched(y[M:]), "a row past M was written"
    return y[:M].cpu(), ref, mag, RR.norm_modulate(x, R.f32(1e-6), sc, sh, layernorm=ln)


@pytest.mark.parametrize("mode", ["none", "scale_shift", "mod_row"])
@pytest.mark.parametrize("M", [1, 3, 5])
@pytest.mark.parametrize("D", [512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
def test_norm_modulate_edges(dev, ln, D, M, mode):
    """rms_norm / LayerNorm + modulation, one wave per row.  Catches: a chunk loop that stops short of D/512 (D = 8192 is
    MAX_CHUNKS), a last workgroup whose idle waves store (M % 4 != 0: rows past M must stay NaN), an off-by-one
    `mod_row` or a modulation row read at the wrong stride (U = 3, mod_stride = 6D), and - for LayerNorm, on rows of
    100 + N(0,1) - a one-pass E[x^2] - E[x]^2 variance, which cancels there."""
    got, ref, mag, iv = _norm_case(dev, ln, M, D, mode, seed=RR.norm_seed(ln, D, M))
    # LayerNorm rows of 100 + N(0,1) hold ~30 distinct bf16 values (ulp 0.5 there), so a value that lands near a rounding
    # midpoint flips as a group: measured up to 3.9 % of a row
    _close(got, ref, max_ulps=1 if mode == "none" else 2, max_frac=0.1 if ln else 1e-2, mag=mag)
    _within(got, iv, cap=RR.cap(ln))                                # rows of 100 + N(0,1): the named cancellation case


@pytest.mark.parametrize("mode", ["none", "mod_row"])
@pytest.mark.parametrize("D", [512, 8192])
def test_layernorm_small_mean_edges(dev, D, mode):
    """LayerNorm on rows of 0.5 + 3 N(0,1), M = 5: without the cancellation of the 100 + N(0,1) rows the admissible
    intervals are narrow (at most 2 % of the elements have more than one admissible value), so here the LayerNorm chain -
    mean, centred variance, rstd, n, modulation - is held to its bf16 interval element by element."""
    got, _, _, iv = _norm_case(dev, True, RR.SMALL_MEAN_M, D, mode, seed=RR.small_mean_seed(D), small_mean=True)
    _within(got, iv)


@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
def test_norm_modulate_many_rows_and_flat_rows(dev, ln):
    """M = 4097 rows at D = 512 (a lone row in the last workgroup), and a constant and an all-zero row at D = 2048
    (variance 0 -> rstd = eps^-1/2: a kernel that divides by the variance or skips eps returns inf/NaN there)."""
    cap = RR.cap(ln)
    got, ref, mag, iv = _norm_case(dev, ln, 4097, 512, "mod_row", seed=41)
    _close(got, ref, max_ulps=2, max_frac=1e-2, mag=mag, tag="m4097_")
    _within(got, iv, cap=cap, tag="m4097_")
    got, ref, mag, iv = _norm_case(dev, ln, 5, 2048, "none", seed=42, special_rows=True)
    _close(got, ref, max_ulps=1, max_frac=1e-2, tag="flat_")
    _within(got, iv, cap=cap, tag="flat_")
    assert torch.isfinite(got.float()).all()


# ------------------------------------------------------------------------------------------- rms norm from row partials
@pytest.mark.parametrize("one_plus", [False, True])
@pytest.mark.parametrize("M", [5, 7])
@pytest.mark.parametrize("D", [512, 1536, 2048, 8192])
def test_rmsnorm_ss_edges(dev, D, M, one_plus):
    """rms_norm + modulation from precomputed 64-column partials (sumsq_ld > D/64, garbage in the extra partials).
    Catches: skipping partials 64..127 (D = 8192: NP = 128, the `for (i = lane + 64; ...)` pass), reading past sumsq_n
    into the garbage, a wrong CH = 1 / 2 row split (D = 1536 vs 2048), ONE_PLUS adding 1 twice, and a last partial
    workgroup (M % 4 != 0) that stores."""
    ops = _ops()
    inp = RR.rmsnorm_ss_inputs(D, M, one_plus)
    x, ss, tab, rows, sc, sh = inp.x, inp.ss, inp.tab, inp.rows, inp.sc, inp.sh
    td = tab.to(dev)
    y = _sent_bf16((M + 3, D), dev)
    ops.rmsnorm_modulate(x.to(dev), 1e-6, td[:, D:2 * D], td[:, :D], 6 * D, rows.to(dev), out=y[:M], sumsq=ss.to(dev),
                         scale_is_one_plus=one_plus)
    y2 = _sent_bf16((M + 3, D), dev)
    ops.rmsnorm_modulate(x.to(dev), 1e-6, out=y2[:M], sumsq=ss.to(dev))
    torch.cuda.synchronize()
    assert _untouched(y[M:]) and _untouched(y2[M:])
    ref, mag = R.norm_modulate(x, R.f32(1e-6), sc, sh, one_plus=one_plus)
    _close(y[:M].cpu(), ref, max_ulps=2, max_frac=1e-2, mag=mag, tag="mod_")
    _close(y2[:M].cpu(), R.norm_modulate(x, R.f32(1e-6))[0], max_ulps=1, max_frac=1e-2, tag="plain_")
    part = ss[:, :inp.NP]
    _within(y[:M].cpu(), RR.norm_modulate(x, R.f32(1e-6), sc, sh, one_plus=one_plus, partials=part), tag="mod_")
    _within(y2[:M].cpu(), RR.norm_modulate(x, R.f32(1e-6), partials=part), tag="plain_")


# ------------------------------------------------------------------------------------------- q/k norm + rope
@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("nseg", [1, 2, 3])
@pytest.mark.parametrize("H,ss", [(h, s) for h in (4, 12, 20, 28, 32) for s in (False, True)] + [(40, True)])
def test_qknorm_rope_edges(dev, H, ss, nseg, rope):
    """q/k RMSNorm (learned weight) + SPLIT rope in place on nseg segments of a panel with ld = nseg*D + 64, B = 2 so that
    t = row % T wraps.  Catches: idle lanes of the last 8-head pass (H = 12, 20, 28) contributing to the sum or storing,
    a segment offset or weight row off by one (nseg = 3), writes into the columns past nseg*D, a rope table indexed by
    row instead of row % T, and - for the partials form - a reduction that stops at 64 partials (H = 40: NP = 80) or
    reads another segment's partials.  H = 40 runs in the partials form only: the self-reducing one takes H <= 32."""
    ops = _ops()
    inp = RR.qknorm_inputs(H, ss, nseg, rope)
    T, M, D, x, w, cos, sin = inp.T, inp.M, inp.D, inp.x, inp.w, inp.cos, inp.sin
    ld = nseg * D + 64
    buf = _sent_bf16((M + 2, ld), dev)
    buf[:M, :nseg * D] = x.to(dev)
    sumsq = inp.sumsq.to(dev) if ss else None
    ops.qknorm_rope(buf[:M], nseg, D, w.to(dev), cos.to(dev) if rope else None, sin.to(dev) if rope else None, T, H, 1e-6,
                    sumsq=sumsq)
    torch.cuda.synchronize()
    assert _untouched(buf[:M, nseg * D:]), "columns past nseg*D were written"
    assert _untouched(buf[M:]), "a row past M was written"
    ref, mag = R.qknorm_rope(x, w, cos, sin, T, H, R.f32(1e-6))
    _close(buf[:M, :nseg * D].cpu(), ref, max_ulps=2 if rope else 1, max_frac=1e-2, mag=mag)
    _within(buf[:M, :nseg * D].cpu(), RR.qknorm_rope(x, w, cos, sin, T, H, R.f32(1e-6), partials=RR.qknorm_partials(inp)))


# ------------------------------------------------------------------------------------------- rope table
@pytest.mark.parametrize("H,dim,n_freq", [(1, 120, 20), (1, 120, 18), (4, 48, 8), (4, 48, 7), (32, 4096, 682)])
def test_rope_table_edges(dev, H, dim, n_freq):
    """SPLIT rope table at T = 300 (not a multiple of 256), start != end positions, front pad both 0 and > 0.  Catches:
    a pad region that is not exactly cos = 1 / sin = 0, (idx, axis) interleaving swapped, the per-head regrouping
    off by a column, start instead of the middle of the interval, and stores past H*T*dim/2/H.
    Bound: the fp32 angle error 2^-22 (|ang| + |2 frac freq|) plus two fp32 ulps of the result (cosf/sinf)."""
    L = _lib()
    g = _g(H * 1000 + n_freq)
    T = 300
    st = torch.randint(0, 40, (3, T), generator=g).float()
    pos = torch.stack([st, st + torch.randint(1, 5, (3, T), generator=g).float()], -1).contiguous()
    lin = torch.linspace(0.0, 1.0, n_freq, dtype=torch.float32)
    freq = (torch.pow(torch.tensor(10000.0), lin) * (np.pi / 2)).float()
    mp = (20.0, 2048.0, 2048.0)
    per = dim // 2 // H
    n = H * T * per
    cb, sb = _sent_f32((n + 64,), dev), _sent_f32((n + 64,), dev)
    mpa = (ctypes.c_float * 3)(*mp)
    pd, fd = pos.to(dev), freq.to(dev)
    L.check(L.load().ltxk_rope_table(pd.data_ptr(), fd.data_ptr(), cb.data_ptr(), sb.data_ptr(), T, H, dim, n_freq, mpa,
                                     torch.cuda.current_stream().cuda_stream), "ltxk_rope_table")
    torch.cuda.synchronize()
    assert _untouched(cb[n:]) and _untouched(sb[n:])
    c, s, ang, big = R.rope_table(pos, freq, H, dim, mp)
    gc, gs = cb[:n].reshape(H, T, per).cpu().double(), sb[:n].reshape(H, T, per).cpu().double()
    pad = dim // 2 - 3 * n_freq
    padm = torch.zeros(T, dim // 2, dtype=torch.bool)
    padm[:, :pad] = True
    padm = padm.reshape(T, H, per).permute(1, 0, 2)
    assert bool((gc[padm] == 1.0).all()) and bool((gs[padm] == 0.0).all())
    e_ang = (ang.abs() + big) * 2.0 ** -22
    worst = 0.0
    for got, ref in ((gc, c), (gs, s)):
        bound = e_ang + 2 * _ulp_f32(ref) + 2.0 ** -149
        worst = max(worst, float(((got - ref).abs() / bound).max()))
    parity.auto(worst, 1.0, tag="err_over_bound")


# ------------------------------------------------------------------------------------------- timestep embedding
@pytest.mark.parametrize("mult", [1.0, 1000.0])
@pytest.mark.parametrize("dim", [256, 6])
def test_timestep_embed_edges(dev, dim, mult):
    """Sinusoidal projection of U = 1001 timesteps covering [0, 1000] after the multiplier (t in [0, 1] for mult = 1000).
    Catches: the product t*mult not rounded to bf16 (timestep*1000 stays in the model dtype), cos/sin halves swapped,
    a frequency ladder over `dim` instead of dim/2 (dim = 6: half = 3), and stores past U rows.
    Bound: one bf16 ulp plus the fp32 argument error |ang| (3 * 2^-24 * ln(1e4) i/half + 2^-21)."""
    L = _lib()
    U = 1001
    t = (torch.linspace(0, 1000, U) / mult).to(BF)
    out = _sent_bf16((U + 1, dim), dev)
    t_d = t.to(dev)
    L.check(L.load().ltxk_timestep_embed(t_d.data_ptr(), out.data_ptr(), U, dim, float(mult),
                                         torch.cuda.current_stream().cuda_stream), "ltxk_timestep_embed")
    torch.cuda.synchronize()
    assert _untouched(out[U:])
    ref, ang = R.timestep_embed(t, dim, mult)
    half = dim // 2
    lnexp = (np.log(10000.0) * torch.arange(half, dtype=torch.float64) / half).repeat(2)
    e = ang.abs() * (3 * 2.0 ** -24 * lnexp + 2.0 ** -21)[None] + 2.0 ** -24
    got = out[:U].cpu().double()
    ratio = float(((got - ref).abs() / (R.ulp_bf16(ref.abs() + e) + e)).max())
    parity.auto(ratio, 1.0, tag="err_over_bound")


# ------------------------------------------------------------------------------------------- ada_combine
@pytest.mark.parametrize("D", [8, 24])
def test_ada_combine_edges(dev, D):
    """table (L=2, K=32, D) + ada (U=3, K*D) with one_plus_mask bits 1, 4 and 31.  Catches: a mask shift that loses bit
    31 (signed shift or a 31-bit mask), the k of an 8-element vector taken from the wrong row when D = 8 or 24 (one or
    three vectors per row), and stores past L*U*K*D.  Exact: the inputs keep every sum exact in fp32."""
    L_ = _lib()
    g = _g(D)
    L, U, K = 2, 3, 32
    mag = lambda *s: (torch.rand(*s, generator=g) * 3.9 + 0.1) * torch.sign(torch.randn(*s, generator=g))
    tab, ada = mag(L, K, D).to(BF), mag(U, K * D).to(BF)
    mask = (1 << 31) | (1 << 4) | (1 << 1)
    n = L * U * K * D
    out = _sent_bf16((n + 64,), dev)
    tab_d = tab.to(dev)
    ada_d = ada.to(dev)
    L_.check(L_.load().ltxk_ada_combine(tab_d.data_ptr(), ada_d.data_ptr(), out.data_ptr(), L, U, K, D, mask,
                                        torch.cuda.current_stream().cuda_stream), "ltxk_ada_combine")
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    _close(out[:n].reshape(L, U, K, D).cpu(), R.ada_combine(tab, ada, mask), max_ulps=0, max_frac=0.0)


# ------------------------------------------------------------------------------------------- silu
_all_finite_bf16 = RR.all_finite_bf16


def test_silu_every_value(dev):
    """Every finite bf16 in [-100, 100] plus large values of both signs, n = 8*(256k + 3) so the last workgroup is
    partial.  Catches: a silu whose exp(-x) overflows to inf and flushes results that are still normal numbers
    (x in [-91.8, -88.7]), a wrong rounding, and a last vector group that is skipped or stored past n."""
    L = _lib()
    x = RR.silu_inputs()
    n = x.numel()
    y = _sent_bf16((n + 64,), dev)
    x_d = x.to(dev)
    L.check(L.load().ltxk_silu(x_d.data_ptr(), y.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "ltxk_silu")
    torch.cuda.synchronize()
    assert _untouched(y[n:])
    _close(y[:n].cpu(), R.silu(x), max_ulps=1, max_frac=1e-2)
    _within(y[:n].cpu(), RR.silu(x))


# ------------------------------------------------------------------------------------------- latent -> tokens
def test_latent_to_tokens_edges(dev):
    """(B=2, C=8, S=65) -> (rep=3 * B, S, C).  Catches: the partial last 64-wide block along S, a replica written at the
    wrong batch offset, and stores past rep*B*S*C.  Exact."""
    L = _lib()
    B, C, S, rep = 2, 8, 65, 3
    lat = torch.randn(B, C, S, generator=_g(5)).to(BF)
    n = rep * B * S * C
    out = _sent_bf16((n + 64,), dev)
    lat_d = lat.to(dev)
    L.check(L.load().ltxk_latent_to_tokens(lat_d.data_ptr(), out.data_ptr(), B, C, S, rep,
                                           torch.cuda.current_stream().cuda_stream), "ltxk_latent_to_tokens")
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    want = lat.transpose(1, 2).repeat(rep, 1, 1)
    _close(out[:n].reshape(rep * B, S, C).cpu(), want, max_ulps=0, max_frac=0.0)


# ------------------------------------------------------------------------------------------- cfg + Euler step tail
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("bf16_euler", [False, True], ids=["f32euler", "bf16euler"])
@pytest.mark.parametrize("sn", [0.725, 0.0], ids=["sn", "last"])
@pytest.mark.parametrize("cfg", ["none", "1", "4"])
def test_cfg_euler_edges(dev, cfg, sn, bf16_euler, masked):
    """The step tail on B = 2, C = 16, S = 67 (a partial 64-wide block): no CFG (v_neg = None), cfg 1 and 4, the fp32 and
    the op-by-op bf16 Euler, the last step (sigma_next = 0), a mask of 0 / 1 / 0.75.  Catches: v_neg read when NULL,
    the (cfg-1) factor applied at cfg = 1, the mask blend weights swapped, the bf16 Euler losing a rounding point, the
    last block along S skipped or stored past S.  The in-place form (out is latent) and the device-scalar form (_dev)
    must give the host form's bits exactly."""
    ops = _ops()
    inp = RR.cfg_euler_inputs(cfg, sn, bf16_euler, masked)
    B, C, S, vp, vn, cs, x, clean, mask, sig, sig_n = inp.B, inp.C, inp.S, inp.vp, inp.vn, inp.cs, inp.x, inp.clean, inp.mask, inp.sig, inp.sig_n
    d = lambda t: None if t is None else t.to(dev)
    n = B * C * S
    outs = []
    for form in ("host", "dev", "inplace"):
        buf = _sent_bf16((n + 64,), dev)
        lat = x.to(dev)
        if form == "inplace":
            buf[:n] = lat.flatten()
            lat = buf[:n].view(B, C, S)
        o = buf[:n].view(B, C, S)
        sd = torch.tensor([sig, sig_n], dtype=torch.float32, device=dev) if form == "dev" else None
        ops.cfg_euler_step(vp.to(dev), d(vn), lat, cs, sig, sig_n, d(clean), d(mask), out=o, sigmas_dev=sd,
                           bf16_euler=bf16_euler)
        torch.cuda.synchronize()
        assert _untouched(buf[n:]), form
        outs.append(o.cpu())
    ref, mag = R.cfg_euler_step(vp, vn, x, sig, sig_n, cs, clean, mask, bf16_euler=bf16_euler)
    _close(outs[0], ref, max_ulps=2, max_frac=4e-2 if bf16_euler else 1e-2, mag=mag, tag="ref_")   # bf16 Euler: 1.5 % measured
    _within(outs[0], RR.cfg_euler_step(vp, vn, x, sig, sig_n, cs, clean, mask, bf16_euler=bf16_euler), cap=RR.cap(bf16_euler),
            tag="ref_")                                             # the bf16 Euler tail: a named cancellation case
    _close(outs[1], outs[0], max_ulps=0, max_frac=0.0, tag="dev_")
    _close(outs[2], outs[0], max_ulps=0, max_frac=0.0, tag="inplace_")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("bf16_euler", [False, True], ids=["f32euler", "bf16euler"])
def test_flat_tail_entries_equal_step_tail(dev, bf16_euler, masked):
    """ltxk_cfg_euler_step and ltxk_cfg_euler_step_dev called through the binding (no ops path calls them any more) against
    ops.step_tail, bit for bit, on B = 2, C = 16 (two channel groups), S = 70 (a full wave and a 6-lane tail).  Catches a
    flat entry whose arguments reach the shared launch in another order, or that drops sigmas_dev or the flags."""
    L, ops = _lib(), _ops()
    g = _g(90 + 2 * bf16_euler + masked)
    B, C, S = 2, 16, 70
    n = B * C * S
    vp, vn = (torch.randn(B, S, C, generator=g).to(BF).to(dev) for _ in range(2))
    x = torch.randn(B, C, S, generator=g).to(BF).to(dev)
    clean = torch.randn(B, C, S, generator=g).to(BF).to(dev) if masked else None
    mask = torch.tensor([0.0, 1.0, 0.75])[torch.randint(0, 3, (B, S), generator=g)].to(dev) if masked else None
    cs, sig, sig_n = 4.0, R.f32(0.909375), R.f32(0.725)
    sd = torch.tensor([sig, sig_n], dtype=torch.float32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    want = ops.step_tail(vp, vn, None, x, cfg_scale=cs, sigma=sig, sigma_next=sig_n, clean=clean, mask_tok=mask, bf16_euler=bf16_euler)
    host, devf = _sent_bf16((n + 128,), dev), _sent_bf16((n + 128,), dev)
    L.check(L.load().ltxk_cfg_euler_step(p(vp), p(vn), p(x), host[64:].data_ptr(), p(clean), p(mask), B, C, S, cs, sig, sig_n,
                                         int(bf16_euler), st), "ltxk_cfg_euler_step")
    L.check(L.load().ltxk_cfg_euler_step_dev(p(vp), p(vn), p(x), devf[64:].data_ptr(), p(clean), p(mask), B, C, S, cs, p(sd),
                                             int(bf16_euler), st), "ltxk_cfg_euler_step_dev")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(want.float()).any())
    for tag, buf in (("host", host), ("dev", devf)):
        assert _untouched(buf[:64]) and _untouched(buf[64 + n:]), tag
        assert torch.equal(buf[64:64 + n].view(torch.int16), want.reshape(-1).view(torch.int16)), tag


# ------------------------------------------------------------------------------------------- Euler alone
@pytest.mark.parametrize("sn", [0.3, 0.0])
def test_euler_step_edges(dev, sn):
    """Eager Euler update, n = 8*(256*3 + 5) (not a multiple of 2048: a partial last workgroup).  Catches a tail that is
    skipped or stored past n, and sigma / sigma_next swapped.  One rounding of the fp32 formula: <= 1 ulp."""
    L = _lib()
    inp = RR.euler_inputs(sn)
    n, x, x0, sig = inp.n, inp.x, inp.x0, inp.sig
    out = _sent_bf16((n + 64,), dev)
    x_d = x.to(dev)
    x0_d = x0.to(dev)
    L.check(L.load().ltxk_euler_step(x_d.data_ptr(), x0_d.data_ptr(), out.data_ptr(), n, sig, R.f32(sn),
                                     torch.cuda.current_stream().cuda_stream), "ltxk_euler_step")
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    ref, mag = R.euler_step(x, x0, sig, R.f32(sn))
    # the final add cancels often (x0 and the step have either sign): 1.9 % of the elements sit one ulp (at mag) from the
    # float64 value, exactly as the same formula in float32 on the CPU, which the kernel must match bit for bit
    _close(out[:n].cpu(), ref, max_ulps=1, max_frac=4e-2, mag=mag, tag="f64_")
    _within(out[:n].cpu(), RR.euler_step(x, x0, sig, R.f32(sn)), cap=RR.NO_CAP, tag="f64_")        # a named cancellation case
    s32, sn32 = torch.tensor(sig), torch.tensor(R.f32(sn))
    want = (x0.float() + (sn32 * (x.float() - x0.float())) / s32).to(BF)
    _close(out[:n].cpu(), want, max_ulps=0, max_frac=0.0, tag="f32_")


# ------------------------------------------------------------------------------------------- step scalars
@pytest.mark.parametrize("start", ["0", "n-1", "n", "n+5"])
def test_step_scalars_edges(dev, start):
    """Per-step scalars of a replayed step graph, U = 100 timestep values (more than the kernel's 64-thread stride),
    replayed three times eagerly on one stream from *step in {0, n-1, n, n+5}.  Catches: values 64..99 not copied,
    a step past the table not clamped to row n-1, the counter not advanced to min(step, n-1) + 1, and stores past U / 2."""
    L = _lib()
    g = _g(len(start))
    n, U = 5, 100
    ts_all = torch.randn(n, U, generator=g).to(BF)
    sig_all = torch.rand(n, 2, generator=g)
    s = {"0": 0, "n-1": n - 1, "n": n, "n+5": n + 5}[start]
    step = torch.tensor([s], dtype=torch.int32, device=dev)
    ts, sg = _sent_bf16((U + 8,), dev), _sent_f32((4,), dev)
    tsd, sgd = ts_all.to(dev), sig_all.to(dev)
    for _ in range(3):
        L.check(L.load().ltxk_step_scalars(tsd.data_ptr(), sgd.data_ptr(), step.data_ptr(), ts.data_ptr(), sg.data_ptr(),
                                           U, n, torch.cuda.current_stream().cuda_stream), "ltxk_step_scalars")
        torch.cuda.synchronize()
        row = min(s, n - 1)
        assert torch.equal(ts[:U].cpu().view(torch.int16), ts_all[row].view(torch.int16))
        assert torch.equal(sg[:2].cpu(), sig_all[row])
        assert _untouched(ts[U:]) and _untouched(sg[2:])
        s = row + 1
        assert int(step.item()) == s
    parity.auto(0.0, 0.0, tag="exact")
