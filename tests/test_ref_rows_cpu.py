"""What the set-valued reference of tests/ref_rows.py accepts and rejects, on the very inputs of the GPU cases (the input
builders are shared, the case lists are read from the GPU tests' own parametrisation).  CPU only.

Accepted, in every element: an fp32 emulation of each kernel - the reducing ones in three summation orders (sequential,
reversed, per lane then butterfly) -, the single-valued float64 reference of ref64.py, and the oracle's function where
test_ref64_cpu.py compares against one.  The emulation in the kernel's own order is held to the interval of the kernel's
depth; summed first to last or last to first it is another reduction, with a chain as long as the row, and is held to the
interval of that depth.  Rejected, with at least one element outside: the faults of ``test_rejects_*``, each planted in the
fp32 emulation.  ``test_condition_*`` assert on the reference alone that the check is sharp on every GPU case: at most 2 %
of the elements have more than one admissible bf16 value and no interval holds more than two neighbours - except the
cancellation cases (ref_rows.AMBIGUOUS_CAP), whose shares are printed, and except the width clause where ``_condition``'s
``wide`` says why no seed can meet it ("Row kernels: per-element admissible bf16 interval")."""
import functools

import pytest
import torch

import ref64 as R
import ref_attn64 as R64
import ref_rows as RR
import test_attn64_gpu as GA
import test_rowops_gpu as GR
import test_vae_glue_gpu as GV
from oracle import dit as O
from oracle import vae as OV

BF = torch.bfloat16
F32 = torch.float32
P = O.BF16
ORDERS = ("seq", "rev", "lane")
EPS = R.f32(1e-6)
PN_EPS = R.f32(1e-8)


def r16(t):
    return t.to(BF).float()


def sum32(t, order, lanes=64, vec=8):
    """fp32 sum over the last axis (keepdim): 'seq' first to last, 'rev' last to first, 'lane' - `lanes` lanes that each add
    their `vec`-wide pieces of every lanes*vec chunk in turn, then a butterfly over the lanes (xor lanes/2 .. 1)."""
    t = t.float()
    K = t.shape[-1]
    if order in ("seq", "rev"):
        acc = torch.zeros_like(t[..., 0])
        for k in (range(K) if order == "seq" else range(K - 1, -1, -1)):
            acc = acc + t[..., k]
        return acc[..., None]
    pad = (-K) % (lanes * vec)
    if pad:
        t = torch.cat([t, torch.zeros(*t.shape[:-1], pad)], -1)
    t = t.reshape(*t.shape[:-1], -1, lanes, vec).transpose(-3, -2).reshape(*t.shape[:-1], lanes, -1)
    acc = torch.zeros_like(t[..., 0])
    for k in range(t.shape[-1]):
        acc = acc + t[..., k]
    idx = torch.arange(lanes)
    off = lanes // 2
    while off >= 1:
        acc = acc + acc[..., idx ^ off]
        off //= 2
    return acc[..., :1]


def _outside(got, iv):
    return RR.within(got, iv)[0][0]


# ------------------------------------------------------------------------------------------------- fp32 emulations
def emu_norm(x, eps, sc=None, sh=None, *, ln=False, one_plus=False, partials=None, order="seq", fault=None, pert=0.0):
    xf = x.float()
    D = xf.shape[-1]
    dv = float(D - 1) if fault == "div_dm1" else float(D)
    e = torch.tensor(0.0 if fault == "no_eps" else eps, dtype=F32)
    d = xf
    if partials is not None:
        p = partials.float().clone()
        if fault == "drop_partial":
            p[:, 70] = 0.0
        ss = sum32(p, order, 64, 1)
    elif ln and fault == "one_pass":
        mean = sum32(xf, order) / dv
        ss = sum32(xf * xf, order) - (mean * mean) * dv          # D * (E[x^2] - E[x]^2)
        d = xf - mean
    elif ln:
        mean = sum32(xf, order) / dv
        d = xf - mean
        ss = sum32(d * d, order)
    else:
        ss = sum32(xf * xf, order)
    rstd = torch.rsqrt(ss / dv + e)
    if pert:
        rstd = rstd * torch.tensor(1.0 + pert, dtype=F32)
    pre = d * rstd
    if sc is None:
        return pre.to(BF)
    n = pre if fault == "n_not_rounded" else r16(pre)
    one_p = sc.float() if one_plus else r16(1.0 + sc.float())
    if fault == "one_plus_twice":
        one_p = r16(1.0 + one_p)
    return (r16(n * one_p) + sh.float()).to(BF)


def emu_qknorm(inp, order="seq", fault=None, pert=0.0):
    M, D, H, nseg, T, half = inp.M, inp.D, inp.H, inp.nseg, inp.T, inp.dh // 2
    seg = inp.x.float().reshape(M, nseg, D)
    if inp.sumsq is not None:
        ss = sum32(RR.qknorm_partials(inp).reshape(M, nseg, -1), order, 64, 1)
    else:
        ss = sum32(seg * seg, order)
    dv = float(D - 1) if fault == "div_dm1" else float(D)
    rstd = torch.rsqrt(ss / dv + torch.tensor(EPS, dtype=F32))
    if pert:
        rstd = rstd * torch.tensor(1.0 + pert, dtype=F32)
    y = r16(seg * rstd * inp.w.float()[None])
    if inp.cos is None:
        return y.reshape(M, nseg * D).to(BF)
    yh = y.reshape(M, nseg, H, 2, half)
    t = torch.arange(M) if fault == "no_mod_T" else torch.arange(M) % T
    rows = (torch.arange(H)[None, :] * T + t[:, None]).clamp_max(H * T - 1)            # (M,H): flat table row, as the kernel indexes
    c = inp.cos.reshape(H * T, half)[rows][:, None]
    s = inp.sin.reshape(H * T, half)[rows][:, None]
    x1, x2 = yh[..., 0, :], yh[..., 1, :]
    p2, p1 = (x2.roll(1, -1), x1.roll(1, -1)) if fault == "partner_off" else (x2, x1)
    o = torch.stack([x1 * c - s * p2, x2 * c + s * p1], dim=-2)
    return o.to(BF).reshape(M, nseg * D)


def emu_cfg_euler(inp, fault=None):
    sig, sn = (inp.sig_n, inp.sig) if fault == "sigma_swapped" else (inp.sig, inp.sig_n)
    sig, sn = torch.tensor(sig, dtype=F32), torch.tensor(sn, dtype=F32)
    v = inp.vp.float().transpose(1, 2)
    x = inp.x.float()
    if inp.vn is not None:
        k = torch.tensor(inp.cs, dtype=F32) - 1.0
        v = r16(v + r16(k * r16(v - inp.vn.float().transpose(1, 2))))
    x0 = r16(x - sig * v)
    if inp.mask is not None:
        m = inp.mask.float()[:, None, :]
        om = r16(1.0 - m)
        a, b = (om, m) if fault == "mask_swapped" else (m, om)
        x0 = r16(r16(x0 * a) + r16(inp.clean.float() * b))
    if inp.bf16_euler:
        return (x0 + r16(r16(sn * r16(x - x0)) / sig)).to(BF)
    if float(sn) > 0:
        return (x0 + (sn * (x - x0)) / sig).to(BF)
    return x0.to(BF)


def emu_euler(inp, fault=None):
    sig, sn = (inp.sig_n, inp.sig) if fault == "sigma_swapped" else (inp.sig, inp.sig_n)
    x, x0 = inp.x.float(), inp.x0.float()
    return (x0 + (torch.tensor(sn, dtype=F32) * (x - x0)) / torch.tensor(sig, dtype=F32)).to(BF)


def silu_div32(x):
    e = torch.exp(-x)
    return torch.where(torch.isinf(e), x * torch.exp(x), x / (1.0 + e))


def silu_f32(x):
    return x * (1.0 / (1.0 + torch.exp2(torch.tensor(-1.4426950408889634, dtype=F32) * x)))


def emu_pixelnorm(x, eps, sc=None, sh=None, rpb=0, silu_on=False, order="seq", fault=None, pert=0.0):
    xf = x.float()
    V, C = xf.shape
    lpr = min(C // 8, 64)
    S = sum32(r16(xf * xf), order, lpr, 8)
    m = S / float(C)
    if fault != "m_not_rounded":
        m = r16(m)
    s = torch.sqrt(r16(m + torch.tensor(0.0 if fault == "no_eps" else eps, dtype=F32)))
    if fault != "s_not_rounded":
        s = r16(s)
    rsd = 1.0 / s
    q0 = xf * rsd
    res = (xf.double() - q0.double() * s.double()).float()                       # fmaf(-q0, s, x)
    t = (res.double() * rsd.double() + q0.double()).float()                      # fmaf(res, rsd, q0)
    if pert:
        t = t * torch.tensor(1.0 + pert, dtype=F32)
    t = r16(t)
    if sc is not None:
        b = torch.arange(V) // rpb
        t = r16(r16(t * r16(1.0 + sc.float()[b])) + sh.float()[b])
    if silu_on:
        t = silu_f32(t)
    return t.to(BF)


def emu_groupnorm(inp, order="seq", fault=None, pert=0.0):
    B, V, C, G = inp.B, inp.V, inp.C, inp.G
    cg = C // G
    xf = inp.x.float()
    if fault == "stats_over_C":
        terms = xf.reshape(B, 1, V * C)
        n = V * C
    else:
        terms = xf.reshape(B, V, G, cg).permute(0, 2, 1, 3).reshape(B, G, V * cg)
        n = V * cg
    mean = sum32(terms, order, 256, 1) / float(n)
    d = terms - mean
    var = sum32(d * d, order, 256, 1) / float(n)
    sd = torch.sqrt(var + torch.tensor(inp.eps, dtype=F32))
    q = d / sd
    if pert:
        q = q * torch.tensor(1.0 + pert, dtype=F32)
    q = q.reshape(B, -1, V, cg).permute(0, 2, 1, 3).reshape(B, V, C) if fault != "stats_over_C" else q.reshape(B, V, C)
    y = r16(q * inp.gam.float() + inp.bet.float())
    if inp.r is not None:
        y = r16(y + inp.r.float())
    if inp.silu:
        y = silu_div32(y)
    return y.to(BF)


def emu_latent_denorm(inp):
    x = inp.lat.float()
    if inp.noise is not None:
        s = torch.tensor(inp.noise_scale, dtype=F32)
        x = r16(r16(inp.noise.float() * s) + r16((1.0 - s) * x))
    return (x * inp.std.float()[None, :, None] + inp.mean.float()[None, :, None]).to(BF).transpose(1, 2)


def emu_tile_blend(inp):
    a32 = torch.zeros(inp.B, inp.C, inp.F, inp.H, inp.W)
    w32 = torch.zeros(inp.B, 1, inp.F, inp.H, inp.W)
    for tile, (at, ah, aw), mt, mh, mw, (t0, h0, w0) in inp.tiles:
        m = (mt[:at, None, None] * mh[None, :ah, None]) * mw[None, None, :aw]
        a32[:, :, t0:t0 + at, h0:h0 + ah, w0:w0 + aw] += tile[:, :, :at, :ah, :aw].float() * m
        w32[:, :, t0:t0 + at, h0:h0 + ah, w0:w0 + aw] += m
    return (a32 / w32.clamp_min(1e-8)).to(BF)


# ------------------------------------------------------------------------------- the GPU cases and their references
@functools.lru_cache(maxsize=None)
def norm_case(ln, D, M, mode, seed=None, special=False, small=False):
    inp = RR.norm_inputs(ln, M, D, mode, RR.norm_seed(ln, D, M) if seed is None else seed, special, small)
    return inp, RR.norm_modulate(inp.x, EPS, inp.sc, inp.sh, layernorm=ln)


def norm_cases():
    """(name, excepted, args of norm_case): test_norm_modulate_edges, _many_rows_and_flat_rows, the small-mean LayerNorm family."""
    out = [(f"norm[{'ln' if c['ln'] else 'rms'}-{c['D']}-{c['M']}-{c['mode']}]", c["ln"], (c["ln"], c["D"], c["M"], c["mode"]))
           for c in RR.gpu_cases(GR.test_norm_modulate_edges)]
    for ln in (False, True):
        out.append((f"norm_m4097[{'ln' if ln else 'rms'}]", ln, (ln, 512, 4097, "mod_row", 41)))
        out.append((f"norm_flat[{'ln' if ln else 'rms'}]", ln, (ln, 2048, 5, "none", 42, True)))
    for c in RR.gpu_cases(GR.test_layernorm_small_mean_edges):
        out.append((f"ln_small_mean[{c['D']}-{c['mode']}]", False, (True, c["D"], RR.SMALL_MEAN_M, c["mode"], RR.small_mean_seed(c["D"]), False, True)))
    return out


@functools.lru_cache(maxsize=None)
def ss_case(D, M, one_plus):
    inp = RR.rmsnorm_ss_inputs(D, M, one_plus)
    p = inp.ss[:, :inp.NP]
    return inp, RR.norm_modulate(inp.x, EPS, inp.sc, inp.sh, one_plus=one_plus, partials=p), RR.norm_modulate(inp.x, EPS, partials=p)


@functools.lru_cache(maxsize=None)
def qk_case(H, ss, nseg, rope, dh):
    inp = RR.qknorm_inputs(H, ss, nseg, rope, dh)
    return inp, RR.qknorm_rope(inp.x, inp.w, inp.cos, inp.sin, inp.T, H, EPS, dh, RR.qknorm_partials(inp))


def qk_cases():
    return [(c["H"], c["ss"], c["nseg"], c["rope"], 128) for c in RR.gpu_cases(GR.test_qknorm_rope_edges)] + \
           [(c["H"], c["ss"], c["nseg"], c["rope"], 64) for c in RR.gpu_cases(GA.test_qknorm_rope_dh64_edges)]


@functools.lru_cache(maxsize=None)
def cfg_case(cfg, sn, bf16_euler, masked):
    inp = RR.cfg_euler_inputs(cfg, sn, bf16_euler, masked)
    return inp, RR.cfg_euler_step(inp.vp, inp.vn, inp.x, inp.sig, inp.sig_n, inp.cs, inp.clean, inp.mask, bf16_euler=bf16_euler)


def cfg_cases():
    return [(c["cfg"], c["sn"], c["bf16_euler"], c["masked"]) for c in RR.gpu_cases(GR.test_cfg_euler_edges)]


@functools.lru_cache(maxsize=None)
def pn_case(C, mod, silu):
    x, sc, sh = R.pixelnorm_inputs(C)
    return (x, sc, sh), RR.pixelnorm_act(x, PN_EPS, sc if mod else None, sh if mod else None, R.PIXELNORM_RPB, silu)


def pn_cases():
    return [(c["C"], c["mod"], c["silu"]) for c in RR.gpu_cases(GV.test_pixelnorm_act_edges)]


@functools.lru_cache(maxsize=None)
def gn_case(C, V, resid, silu):
    inp = RR.groupnorm_inputs(C, V, resid, silu)
    return inp, RR.groupnorm_act(inp.x, inp.gam, inp.bet, inp.G, inp.eps, inp.r, inp.silu)


def gn_cases():
    return [(c["C"], c["V"], c["resid"], c["silu"]) for c in RR.gpu_cases(GV.test_groupnorm_act_edges)]


def _accept(name, got, iv):
    (n, first), _, _ = RR.within(got, iv)
    assert n == 0, f"{name}: {n} elements outside, the first at {first}"


# ------------------------------------------------------------------------------------------------------ the rules
def test_interval_rules():
    """fl: an interval with fp32 endpoints stays, any other grows by u max|.| on either side; an interval that reaches into the subnormals is extended to 0.  A reduction of multiples of q that fits 24 bits
    is exact.  within counts NaN and a neighbour of a one-value interval as outside and measures widths in bf16 steps."""
    v = torch.tensor([1.0 + 2.0 ** -8, 0.1, 0.0, 3.0, 2.0 ** -130], dtype=torch.float64)
    a = RR.fl(RR.Iv(v))
    assert a.lo[0] == v[0] == a.hi[0] and a.lo[2] == 0 == a.hi[2] and a.lo[3] == 3 == a.hi[3]
    assert float(0.1 - a.lo[1]) == pytest.approx(RR.U * 0.1) and float(a.hi[1] - 0.1) == pytest.approx(RR.U * 0.1)
    assert float(a.lo[4]) == 0.0 and float(a.hi[4]) == pytest.approx(2.0 ** -130)      # the subnormal or its flush
    b = RR.fl(RR.Iv(torch.tensor([0.1, 1.0], dtype=torch.float64), torch.tensor([0.2, 1.5], dtype=torch.float64)))
    assert float(0.1 - b.lo[0]) == pytest.approx(RR.U * 0.2) and float(b.hi[0] - 0.2) == pytest.approx(RR.U * 0.2)
    assert float(b.lo[1]) == 1.0 and float(b.hi[1]) == 1.5
    s = RR.reduce_sum(RR.Iv(torch.full((1, 2048), 3.0, dtype=torch.float64)), -1, 38)
    assert float(s.lo) == float(s.hi) == 6144.0
    s = RR.reduce_sum(RR.Iv(torch.tensor([[1.0, 2.0 ** -30]], dtype=torch.float64)), -1, 2)
    assert float(s.hi - s.lo) == pytest.approx(2 * 2 * RR.U * (1 + 2.0 ** -30))
    one = torch.tensor([1.0, 1.0, 1.0, 1.0], dtype=torch.float64)
    got = torch.tensor([1.0, 1.0 + 2.0 ** -7, float("nan"), 1.0])
    (n, first), amb, widest = RR.within(got, RR.Iv(one, torch.tensor([1.0, 1.0, 1.0, 1.0 + 2.0 ** -6], dtype=torch.float64)))
    assert (n, first, amb, widest) == (2, 1, 0.25, 2)
    assert RR.within(torch.tensor([-0.0]), RR.Iv(torch.zeros(1, dtype=torch.float64)))[0][0] == 0
    assert RR.within(torch.tensor([0.0]), RR.Iv(torch.tensor([-(2.0 ** -130)], dtype=torch.float64), torch.tensor([2.0 ** -128], dtype=torch.float64)))[2] == 0
    assert RR.E_ACT == 2.0 ** -15


# ------------------------------------------------------------------------------------------------------ acceptance
@pytest.mark.parametrize("name,excepted,args", norm_cases(), ids=[c[0] for c in norm_cases()])
def test_accepts_norm_modulate(name, excepted, args):
    inp, iv = norm_case(*args)
    _accept(f"{name} fp32 lane", emu_norm(inp.x, EPS, inp.sc, inp.sh, ln=inp.ln, order="lane"), iv)
    long_iv = RR.norm_modulate(inp.x, EPS, inp.sc, inp.sh, layernorm=inp.ln, depth=inp.D)
    for order in ("seq", "rev"):
        _accept(f"{name} fp32 {order}", emu_norm(inp.x, EPS, inp.sc, inp.sh, ln=inp.ln, order=order), long_iv)
    _accept(f"{name} ref64", R.norm_modulate(inp.x, EPS, inp.sc, inp.sh, layernorm=inp.ln)[0], iv)
    if inp.M <= 5:
        n = O.layer_norm_noaffine(inp.x.float(), P, 1e-6) if inp.ln else O.rms_norm(inp.x.float(), P, 1e-6)
        _accept(f"{name} oracle", n if inp.sc is None else O.modulate(n, inp.sc.float(), inp.sh.float(), P), iv)


@pytest.mark.parametrize("c", RR.gpu_cases(GR.test_rmsnorm_ss_edges), ids=lambda c: f"{c['D']}-{c['M']}-{c['one_plus']}")
def test_accepts_rmsnorm_ss(c):
    inp, iv_mod, iv_plain = ss_case(c["D"], c["M"], c["one_plus"])
    p = inp.ss[:, :inp.NP]
    long_mod = RR.norm_modulate(inp.x, EPS, inp.sc, inp.sh, one_plus=inp.one_plus, partials=p, depth=inp.NP)
    long_plain = RR.norm_modulate(inp.x, EPS, partials=p, depth=inp.NP)
    for order in ORDERS:
        _accept(f"mod {order}", emu_norm(inp.x, EPS, inp.sc, inp.sh, one_plus=inp.one_plus, partials=p, order=order), iv_mod if order == "lane" else long_mod)
        _accept(f"plain {order}", emu_norm(inp.x, EPS, partials=p, order=order), iv_plain if order == "lane" else long_plain)
    _accept("mod ref64", R.norm_modulate(inp.x, EPS, inp.sc, inp.sh, one_plus=inp.one_plus)[0], iv_mod)
    _accept("plain ref64", R.norm_modulate(inp.x, EPS)[0], iv_plain)
    # the self-reducing emulation of the same rows lies inside the partials form's intervals too (the partials are exact sums)
    _accept("mod self-reducing", emu_norm(inp.x, EPS, inp.sc, inp.sh, one_plus=inp.one_plus, order="lane"), iv_mod)


@pytest.mark.parametrize("args", qk_cases(), ids=lambda a: "-".join(map(str, a)))
def test_accepts_qknorm_rope(args):
    H, ss, nseg, rope, dh = args
    inp, iv = qk_case(*args)
    long_iv = RR.qknorm_rope(inp.x, inp.w, inp.cos, inp.sin, inp.T, H, EPS, dh, RR.qknorm_partials(inp), depth=inp.NP if ss else inp.D)
    for order in ORDERS:
        _accept(f"fp32 {order}", emu_qknorm(inp, order), iv if order == "lane" else long_iv)
    ref = R.qknorm_rope(inp.x, inp.w, inp.cos, inp.sin, inp.T, H, EPS)[0] if dh == 128 else \
        R64.qknorm_rope(inp.x, inp.w, inp.cos, inp.sin, inp.T, H, EPS, dh)[0]
    _accept("ref64", ref, iv)
    if dh == 128 and H <= 12:
        outs = []
        for s in range(nseg):
            y = O.rms_norm(inp.x[:, s * inp.D:(s + 1) * inp.D].float().reshape(inp.B, inp.T, inp.D), P, 1e-6, inp.w[s])
            if rope:
                y = O.apply_split_rotary_emb(y, inp.cos[None].expand(inp.B, -1, -1, -1), inp.sin[None].expand(inp.B, -1, -1, -1), P)
            outs.append(y.reshape(inp.M, inp.D))
        _accept("oracle", torch.cat(outs, 1), iv)


@pytest.mark.parametrize("args", cfg_cases(), ids=lambda a: "-".join(map(str, a)))
def test_accepts_cfg_euler(args):
    inp, iv = cfg_case(*args)
    _accept("fp32", emu_cfg_euler(inp), iv)
    _accept("ref64", R.cfg_euler_step(inp.vp, inp.vn, inp.x, inp.sig, inp.sig_n, inp.cs, inp.clean, inp.mask, bf16_euler=inp.bf16_euler)[0], iv)
    if not inp.bf16_euler:
        v = inp.vp.float() if inp.vn is None else O.cfg_combine(inp.vp.float(), inp.vn.float(), inp.cs, P)
        x0 = O.to_denoised(inp.x.float(), v.transpose(1, 2), inp.sig, P)
        if inp.mask is not None:
            x0 = O.apply_denoise_mask(x0, inp.clean.float(), inp.mask[:, None, :], P)
        _accept("oracle", O.euler_step(inp.x.float(), x0, inp.sig, inp.sig_n, P), iv)


@pytest.mark.parametrize("sn", [c["sn"] for c in RR.gpu_cases(GR.test_euler_step_edges)])
def test_accepts_euler_and_silu(sn):
    inp = RR.euler_inputs(sn)
    iv = RR.euler_step(inp.x, inp.x0, inp.sig, inp.sig_n)
    _accept("euler fp32", emu_euler(inp), iv)
    _accept("euler ref64", R.euler_step(inp.x, inp.x0, inp.sig, inp.sig_n)[0], iv)
    if sn > 0:
        _accept("euler oracle", O.euler_step(inp.x.float(), inp.x0.float(), inp.sig, inp.sig_n, P), iv)
    x = RR.silu_inputs()
    iv = RR.silu(x)
    _accept("silu_div fp32", silu_div32(x.float()).to(BF), iv)
    near = x.float().abs() <= 80
    _accept("silu_f fp32", silu_f32(x.float()[near]).to(BF), RR.silu(x[near]))
    _accept("silu ref64", R.silu(x), iv)
    _accept("silu oracle", O.silu(x.float()[near], P), RR.silu(x[near]))       # x sigmoid(x): beyond, the sigmoid is subnormal and loses bits


@pytest.mark.parametrize("args", pn_cases(), ids=lambda a: "-".join(map(str, a)))
def test_accepts_pixelnorm(args):
    C, mod, silu = args
    (x, sc, sh), iv = pn_case(*args)
    s, h = (sc, sh) if mod else (None, None)
    long_iv = RR.pixelnorm_act(x, PN_EPS, s, h, R.PIXELNORM_RPB, silu, depth=C)
    for order in ORDERS:
        _accept(f"fp32 {order}", emu_pixelnorm(x, PN_EPS, s, h, R.PIXELNORM_RPB, silu, order), iv if order == "lane" else long_iv)
    _accept("ref64", R.pixelnorm_act(x, PN_EPS, s, h, R.PIXELNORM_RPB, silu)[0], iv)
    V = x.shape[0]
    want = OV.pixel_norm(x.float().t().reshape(1, C, V, 1, 1), P, 1e-8).reshape(C, V).t()
    if mod:
        b = torch.arange(V) // R.PIXELNORM_RPB
        want = OV._mod(want, sc.float()[b], sh.float()[b], P)
    if silu:
        want = O.silu(want, P)
    _accept("oracle", want, iv)


@pytest.mark.parametrize("args", gn_cases(), ids=lambda a: "-".join(map(str, a)))
def test_accepts_groupnorm(args):
    C, V, resid, silu = args
    inp, iv = gn_case(*args)
    long_iv = RR.groupnorm_act(inp.x, inp.gam, inp.bet, inp.G, inp.eps, inp.r, inp.silu, depth=V * C // inp.G)
    for order in ORDERS:
        _accept(f"fp32 {order}", emu_groupnorm(inp, order), iv if order == "lane" else long_iv)
    _accept("ref64", R.groupnorm_act(inp.x, inp.gam, inp.bet, inp.G, inp.eps, inp.r, inp.silu)[0], iv)
    if V <= 7:
        want = OV.group_norm3d(inp.x.permute(0, 2, 1).reshape(inp.B, C, V, 1, 1), inp.gam, inp.bet, P).reshape(inp.B, C, V).permute(0, 2, 1)
        if resid:
            want = P.r(want + inp.r.float())
        if silu:
            want = O.silu(want, P)
        _accept("oracle", want, iv)


def test_accepts_latent_and_tile_blend():
    for c in RR.gpu_cases(GV.test_latent_denorm_cl_edges):
        inp = RR.latent_denorm_inputs(c["noise_scale"])
        iv = RR.latent_denorm_cl(inp.lat, inp.mean, inp.std, inp.noise, inp.noise_scale)
        _accept("denorm fp32", emu_latent_denorm(inp), iv)
        _accept("denorm ref64", R.latent_denorm_cl(inp.lat, inp.mean, inp.std, inp.noise, inp.noise_scale)[0], iv)
    for c in RR.gpu_cases(GV.test_latent_norm_cf_edges):
        inp = RR.latent_norm_inputs(c["pad"])
        iv = RR.latent_norm_cf(inp.x, inp.mean, inp.std)
        _accept("norm fp32", ((inp.x.float() - inp.mean.float()) / inp.std.float()).to(BF).transpose(1, 2), iv)
        _accept("norm ref64", R.latent_norm_cf(inp.x, inp.mean, inp.std), iv)
    inp = RR.tile_blend_inputs()
    iv = RR.tile_blend(inp.tiles, inp.F, inp.H, inp.W)
    _accept("tile_blend fp32", emu_tile_blend(inp), iv)
    _accept("tile_blend ref64", R.tile_blend(inp.tiles, inp.F, inp.H, inp.W), iv)


# ------------------------------------------------------------------------------------------------------- rejection
def _reject(name, got, iv):
    n = _outside(got, iv)
    print(f"rejects {name}: {n} of {got.numel()} elements outside")
    assert n >= 1, name


@pytest.mark.parametrize("D", [512, 4096, 8192])
def test_rejects_norm_modulate_faults(D):
    """Divisor D-1, 1 + scale not rounded away under one_plus, n not rounded, and - on the LayerNorm rows of 100 + N(0,1) - the
    one-pass variance; eps dropped shows on the all-zero row of the flat-rows case."""
    inp, iv = norm_case(False, D, 5, "mod_row")
    _reject(f"rms D={D} divisor D-1", emu_norm(inp.x, EPS, inp.sc, inp.sh, fault="div_dm1"), iv)
    _reject(f"rms D={D} n not rounded", emu_norm(inp.x, EPS, inp.sc, inp.sh, fault="n_not_rounded"), iv)
    lin, liv = norm_case(True, D, 5, "mod_row")
    _reject(f"ln(100+N) D={D} one-pass variance", emu_norm(lin.x, EPS, lin.sc, lin.sh, ln=True, fault="one_pass"), liv)
    sin, siv = norm_case(True, D, RR.SMALL_MEAN_M, "mod_row", RR.small_mean_seed(D), False, True) if D != 4096 else (None, None)
    if sin is not None:
        _reject(f"ln(small mean) D={D} divisor D-1", emu_norm(sin.x, EPS, sin.sc, sin.sh, ln=True, fault="div_dm1"), siv)
        _reject(f"ln(small mean) D={D} n not rounded", emu_norm(sin.x, EPS, sin.sc, sin.sh, ln=True, fault="n_not_rounded"), siv)


@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
def test_rejects_eps_dropped(ln):
    inp, iv = norm_case(ln, 2048, 5, "none", 42, True)
    _reject("eps dropped (the all-zero row)", emu_norm(inp.x, EPS, ln=ln, fault="no_eps"), iv)
    (x, sc, sh), piv = pn_case(512, False, False)
    _reject("pixelnorm eps dropped (the all-zero row)", emu_pixelnorm(x, PN_EPS, fault="no_eps"), piv)


def test_rejects_rmsnorm_ss_faults():
    """NP = 128 (D = 8192): one 64-column partial of the second pass dropped; 1 + scale applied twice under one_plus."""
    for M in (5, 7):
        inp, iv_mod, iv_plain = ss_case(8192, M, True)
        p = inp.ss[:, :inp.NP]
        _reject(f"M={M} one partial dropped", emu_norm(inp.x, EPS, inp.sc, inp.sh, one_plus=True, partials=p, fault="drop_partial"), iv_mod)
        _reject(f"M={M} one partial dropped, plain", emu_norm(inp.x, EPS, partials=p, fault="drop_partial"), iv_plain)
        _reject(f"M={M} 1 + scale twice", emu_norm(inp.x, EPS, inp.sc, inp.sh, one_plus=True, partials=p, fault="one_plus_twice"), iv_mod)
        _reject(f"M={M} divisor D-1", emu_norm(inp.x, EPS, inp.sc, inp.sh, one_plus=True, partials=p, fault="div_dm1"), iv_mod)


@pytest.mark.parametrize("dh,H", [(128, 4), (128, 28), (128, 40), (64, 8), (64, 24)])
def test_rejects_qknorm_rope_faults(dh, H):
    ss = H == 40
    inp, iv = qk_case(H, ss, 2, True, dh)
    _reject(f"dh={dh} H={H} rotation partner off by one column", emu_qknorm(inp, fault="partner_off"), iv)
    _reject(f"dh={dh} H={H} table row t in place of t % T", emu_qknorm(inp, fault="no_mod_T"), iv)
    _reject(f"dh={dh} H={H} divisor D-1", emu_qknorm(inp, fault="div_dm1"), iv)


def test_rejects_step_tail_faults():
    inp, iv = cfg_case("4", 0.725, False, True)
    _reject("mask blend weights swapped", emu_cfg_euler(inp, "mask_swapped"), iv)
    _reject("sigma and sigma_next exchanged", emu_cfg_euler(inp, "sigma_swapped"), iv)
    inp, iv = cfg_case("4", 0.725, True, True)
    _reject("bf16 Euler: mask blend weights swapped", emu_cfg_euler(inp, "mask_swapped"), iv)
    _reject("bf16 Euler: sigma and sigma_next exchanged", emu_cfg_euler(inp, "sigma_swapped"), iv)
    e = RR.euler_inputs(0.3)
    _reject("euler_step: sigma and sigma_next exchanged", emu_euler(e, "sigma_swapped"), RR.euler_step(e.x, e.x0, e.sig, e.sig_n))


def test_rejects_vae_glue_faults():
    for C in (128, 2048):
        (x, sc, sh), iv = pn_case(C, True, False)
        # m not rounded: e = bf16(m + eps) rounds right behind it and eps = 1e-8 is far below half an ulp of m, so the
        # fault moves no output bit on these rows (nothing can reject it); s, the next statistic, left unrounded is seen
        good = emu_pixelnorm(x, PN_EPS, sc, sh, R.PIXELNORM_RPB)
        assert torch.equal(emu_pixelnorm(x, PN_EPS, sc, sh, R.PIXELNORM_RPB, fault="m_not_rounded").view(torch.int16), good.view(torch.int16))
        _reject(f"pixelnorm C={C} s not rounded", emu_pixelnorm(x, PN_EPS, sc, sh, R.PIXELNORM_RPB, fault="s_not_rounded"), iv)
    for C, V in ((96, 7), (512, 7)):
        inp, iv = gn_case(C, V, False, False)
        _reject(f"groupnorm C={C} V={V} statistics over C", emu_groupnorm(inp, fault="stats_over_C"), iv)


def _smallest_rejected(f, iv):
    """(is 2^-14 rejected, the smallest power of two p in 2^-14 .. 2^-24 for which f(p) still has an element outside)."""
    rejected = [k for k in range(14, 25) if _outside(f(2.0 ** -k), iv) >= 1]
    return 14 in rejected, (max(rejected) if rejected else None)


def test_rejects_rstd_perturbation():
    """rstd * (1 + 2^-14) puts an element outside in every norm chain; the smallest power of two still rejected is printed."""
    rows = []
    for D in (512, 4096, 8192):
        inp, iv = norm_case(False, D, 5, "mod_row")
        rows.append((f"rms + modulate D={D}", lambda p, i=inp: emu_norm(i.x, EPS, i.sc, i.sh, pert=p), iv))
        inp, iv = norm_case(False, D, 5, "none")
        rows.append((f"rms D={D}", lambda p, i=inp: emu_norm(i.x, EPS, pert=p), iv))
    for D in (512, 8192):
        inp, iv = norm_case(True, D, RR.SMALL_MEAN_M, "mod_row", RR.small_mean_seed(D), False, True)
        rows.append((f"LayerNorm (small mean) + modulate D={D}", lambda p, i=inp: emu_norm(i.x, EPS, i.sc, i.sh, ln=True, pert=p), iv))
        inp, iv_mod, _ = ss_case(D, 7, True)
        rows.append((f"rms from partials, one_plus D={D}", lambda p, i=inp: emu_norm(i.x, EPS, i.sc, i.sh, one_plus=True, partials=i.ss[:, :i.NP], pert=p), iv_mod))
    for dh, H, ss in ((128, 4, False), (128, 32, False), (128, 40, True), (64, 8, False), (64, 32, True)):
        inp, iv = qk_case(H, ss, 2, True, dh)
        rows.append((f"qknorm_rope dh={dh} D={inp.D}{' partials' if ss else ''}", lambda p, i=inp: emu_qknorm(i, pert=p), iv))
    for C in (128, 2048):
        (x, sc, sh), iv = pn_case(C, True, False)
        rows.append((f"pixelnorm + modulate C={C} (x / s perturbed)", lambda p, a=(x, sc, sh): emu_pixelnorm(a[0], PN_EPS, a[1], a[2], R.PIXELNORM_RPB, pert=p), iv))
    for C, V in ((96, 7), (512, 7)):
        inp, iv = gn_case(C, V, False, False)
        rows.append((f"groupnorm C={C} V={V} ((x - mean) / sd perturbed)", lambda p, i=inp: emu_groupnorm(i, pert=p), iv))
    bad = []
    for name, f, iv in rows:
        at14, smallest = _smallest_rejected(f, iv)
        print(f"perturbation {name}: 2^-14 {'rejected' if at14 else 'ACCEPTED'}, smallest rejected 2^-{smallest}")
        if not at14:
            bad.append(name)
    assert not bad, bad


# ------------------------------------------------------------------------------------- the condition on every GPU case
WIDE_M4097 = "2 M elements: some of the ~300 ambiguous n meet a modulation add that cancels"
WIDE_ROPE = "14 nseg D elements: some of the ambiguous normalised values meet a rotation x1 c - s x2 that cancels"
WIDE_LN_8192 = "x - mean cancels for the elements next to the mean, and the mean of 8192 terms carries 134 u"
WIDE_GN_512_7 = "7168 elements at an offset of 50: x - mean cancels for the elements next to the mean"
WIDE_CFG4 = "cfg 4 triples v+ - v-: the ambiguous x0 are many and x0 + step cancels for some"


def _condition(name, iv, excepted=False, wide=""):
    """The share of elements with more than one admissible bf16 value is at most 2 % and no interval holds more than two
    neighbouring values.  excepted: a named cancellation case, printed only.  wide: why no choice of seed can keep every
    interval to two values in this case - the share is still asserted, the width and the share of wider elements printed."""
    steps = RR.bf16_ord(R.rbf(iv.hi)) - RR.bf16_ord(R.rbf(iv.lo))
    amb, widest, wider = float((steps >= 1).double().mean()), int(steps.max()), float((steps >= 2).double().mean())
    note = " (cancellation case: printed, not asserted)" if excepted else (f" ({wider:.4%} wider than two values: {wide})" if wide else "")
    print(f"condition {name}: ambiguous {amb:.4%}, widest {widest} bf16 steps{note}")
    if not excepted:
        assert amb <= RR.AMBIGUOUS_CAP and (wide or widest <= 1), (name, amb, widest)
    return amb, widest


def test_condition_row_kernels():
    """Worst figures here: see DESIGN.md, "Row kernels: per-element admissible bf16 interval"."""
    for name, excepted, args in norm_cases():
        wide = WIDE_M4097 if name == "norm_m4097[rms]" else (WIDE_LN_8192 if name.startswith("ln_small_mean[8192") else "")
        _condition(name, norm_case(*args)[1], excepted, wide)
    for D in (512, 4096, 8192):                                   # the prototype's figure: no ambiguous element at all
        assert _condition(f"norm[rms-{D}-5-mod_row]", norm_case(False, D, 5, "mod_row")[1])[0] == 0.0
    for c in RR.gpu_cases(GR.test_rmsnorm_ss_edges):
        _, iv_mod, iv_plain = ss_case(c["D"], c["M"], c["one_plus"])
        _condition(f"rmsnorm_ss[{c['D']}-{c['M']}-{c['one_plus']}] mod", iv_mod)
        _condition(f"rmsnorm_ss[{c['D']}-{c['M']}-{c['one_plus']}] plain", iv_plain)
    for args in qk_cases():
        _condition(f"qknorm_rope{args}", qk_case(*args)[1], wide=WIDE_ROPE if args[3] else "")
    for args in cfg_cases():
        _condition(f"cfg_euler{args}", cfg_case(*args)[1], excepted=args[2], wide=WIDE_CFG4 if args[:2] == ("4", 0.725) else "")
    for c in RR.gpu_cases(GR.test_euler_step_edges):
        e = RR.euler_inputs(c["sn"])
        _condition(f"euler_step[{c['sn']}]", RR.euler_step(e.x, e.x0, e.sig, e.sig_n), excepted=True)
    _condition("silu", RR.silu(RR.silu_inputs()))


def test_condition_vae_glue():
    for args in pn_cases():
        _condition(f"pixelnorm{args}", pn_case(*args)[1])
    for args in gn_cases():
        _condition(f"groupnorm{args}", gn_case(*args)[1], excepted=RR.groupnorm_cancels(args[1]), wide=WIDE_GN_512_7 if args[:2] == (512, 7) else "")
    for c in RR.gpu_cases(GV.test_latent_denorm_cl_edges):
        inp = RR.latent_denorm_inputs(c["noise_scale"])
        _condition(f"latent_denorm_cl[{c['noise_scale']}]", RR.latent_denorm_cl(inp.lat, inp.mean, inp.std, inp.noise, inp.noise_scale),
                   excepted=RR.latent_denorm_ties(c["noise_scale"]))
    for c in RR.gpu_cases(GV.test_latent_norm_cf_edges):
        inp = RR.latent_norm_inputs(c["pad"])
        _condition(f"latent_norm_cf[{c['pad']}]", RR.latent_norm_cf(inp.x, inp.mean, inp.std))
    inp = RR.tile_blend_inputs()
    _condition("tile_blend", RR.tile_blend(inp.tiles, inp.F, inp.H, inp.W))
