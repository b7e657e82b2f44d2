"""The float64 references of tests/ref64.py against the oracle's restatement of the same op, and the comparator against
planted errors.  CPU only: the GPU edge-shape tests (test_rowops_gpu.py, test_vae_glue_gpu.py) are only as good as
the reference they compare with and the comparator that judges them."""
import math

import numpy as np
import pytest
import torch

import ref64 as R
from oracle import dit as O
from oracle import vae as OV

BF = torch.bfloat16
P = O.BF16


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------- the rounding
def test_rbf_is_round_to_nearest_even_from_float64():
    """rbf must round float64 once: a value a hair above a bf16 midpoint goes up even where float32 would first round it
    onto the midpoint (and then to even, i.e. down)."""
    x = torch.randn(10000, generator=_g(0), dtype=torch.float64) * 10
    assert torch.equal(R.rbf(x.float().double()), x.float().to(BF).double())      # agrees with torch from fp32
    mid = 1.0 + 2.0 ** -8                              # halfway between 1 and 1 + 2^-7: ties to even -> 1
    assert float(R.rbf(torch.tensor([mid], dtype=torch.float64))) == 1.0
    assert float(R.rbf(torch.tensor([mid + 2.0 ** -40], dtype=torch.float64))) == 1.0 + 2.0 ** -7     # float32 would say 1.0
    assert float(R.rbf(torch.tensor([3.0e-40]))) == float(torch.tensor(3.0e-40).to(BF))   # bf16 subnormal
    assert math.isinf(float(R.rbf(torch.tensor([3.5e38]))))
    assert float(R.ulp_bf16(torch.tensor([1.0]))) == 2.0 ** -7
    assert float(R.ulp_bf16(torch.tensor([1.99]))) == 2.0 ** -7
    assert float(R.ulp_bf16(torch.tensor([0.0]))) == 2.0 ** -126


# ---------------------------------------------------------------------------------------------------- the comparator
def _bf16_data(n=4096, seed=1):
    return torch.randn(n, generator=_g(seed)).to(BF).double()


def test_comparator_rejects_systematic_one_ulp():
    """A reference (or kernel) that is one ulp off everywhere passes max_ulps=1 but not the off-at-all fraction."""
    ref = _bf16_data()
    bad = ref + R.ulp_bf16(ref) * torch.sign(ref)
    R.assert_bf16_close(ref, ref, max_ulps=0, max_frac=0)
    with pytest.raises(AssertionError):
        R.assert_bf16_close(bad, ref, max_ulps=1, max_frac=1e-2)


def test_comparator_rejects_two_ulps_in_one_element():
    ref = _bf16_data()
    bad = ref.clone()
    bad[1234] += 2 * R.ulp_bf16(ref[1234])
    ulps, frac = R.bf16_stats(bad, ref)
    assert ulps == 2.0 and frac == 1 / ref.numel()
    with pytest.raises(AssertionError):
        R.assert_bf16_close(bad, ref, max_ulps=1, max_frac=1e-2)
    one = ref.clone()
    one[1234] += R.ulp_bf16(ref[1234])
    R.assert_bf16_close(one, ref, max_ulps=1, max_frac=1e-2)


def test_comparator_rejects_untouched_sentinel_row():
    ref = _bf16_data(8 * 512).reshape(8, 512)
    got = ref.clone()
    got[7] = float("nan")                              # the sentinel a kernel that skipped its last row leaves
    with pytest.raises(AssertionError):
        R.assert_bf16_close(got, ref, max_ulps=1, max_frac=0.2)
    got[7] = -7.0e4                                    # a finite sentinel is caught by the ulp bound too
    with pytest.raises(AssertionError):
        R.assert_bf16_close(got, ref, max_ulps=1, max_frac=0.2)


def test_comparator_forgives_flushed_subnormals_only():
    ref = torch.tensor([2.0 ** -130, -(2.0 ** -127), 2.0 ** -120], dtype=torch.float64)
    got = torch.tensor([0.0, -0.0, 2.0 ** -120])
    R.assert_bf16_close(got, ref, max_ulps=1, max_frac=1.0)
    with pytest.raises(AssertionError):
        R.assert_bf16_close(torch.zeros(3), ref, max_ulps=1, max_frac=1.0)     # 2^-120 flushed: 64 floor-ulps


# ---------------------------------------------------------------------------------------------------- DiT step ops
def test_norm_modulate_matches_oracle():
    g = _g(2)
    M, D, U = 9, 512, 3
    x = (torch.randn(M, D, generator=g) * 3).to(BF)
    tab = torch.randn(U, 2 * D, generator=g).to(BF)
    rows = torch.randint(0, U, (M,), generator=g)
    sc, sh = tab[rows, D:], tab[rows, :D]
    n = O.rms_norm(x.float(), P, 1e-6)
    ref, mag = R.norm_modulate(x, 1e-6, sc, sh)
    R.assert_bf16_close(O.modulate(n, sc.float(), sh.float(), P), ref, max_ulps=2, max_frac=2e-2, mag=mag, what="rms+mod")
    R.assert_bf16_close(n, R.norm_modulate(x, 1e-6)[0], max_ulps=1, max_frac=2e-2, what="rms")
    xl = (torch.randn(M, D, generator=g) + 100).to(BF)
    nl = O.layer_norm_noaffine(xl.float(), P, 1e-6)
    R.assert_bf16_close(nl, R.norm_modulate(xl, 1e-6, layernorm=True)[0], max_ulps=1, max_frac=2e-2, what="layernorm")
    ref, mag = R.norm_modulate(xl, 1e-6, sc, sh, layernorm=True)
    R.assert_bf16_close(O.modulate(nl, sc.float(), sh.float(), P), ref, max_ulps=2, max_frac=2e-2, mag=mag, what="ln+mod")
    # one_plus: the scale already holds bf16(1+scale)
    op = P.r(1.0 + sc.float())
    assert torch.equal(R.norm_modulate(x, 1e-6, op, sh, one_plus=True)[0], R.norm_modulate(x, 1e-6, sc, sh)[0])


def test_qknorm_rope_matches_oracle():
    g = _g(3)
    B, T, H = 2, 5, 4
    D = H * 128
    x = torch.randn(B * T, 2 * D, generator=g).to(BF)
    w = (1 + 0.2 * torch.randn(2, D, generator=g)).to(BF)
    ang = torch.rand(H, T, 64, generator=g) * 6
    cos, sin = torch.cos(ang), torch.sin(ang)
    ref, mag = R.qknorm_rope(x, w, cos, sin, T, H, 1e-6)
    outs = []
    for s in range(2):
        y = O.rms_norm(x[:, s * D:(s + 1) * D].float().reshape(B, T, D), P, 1e-6, w[s])
        y = O.apply_split_rotary_emb(y, cos[None].expand(B, -1, -1, -1), sin[None].expand(B, -1, -1, -1), P)
        outs.append(y.reshape(B * T, D))
    R.assert_bf16_close(torch.cat(outs, 1), ref, max_ulps=2, max_frac=2e-2, mag=mag, what="qknorm_rope")
    nr, _ = R.qknorm_rope(x, w, None, None, T, H, 1e-6)
    on = torch.cat([O.rms_norm(x[:, s * D:(s + 1) * D].float(), P, 1e-6, w[s]) for s in range(2)], 1)
    R.assert_bf16_close(on, nr, max_ulps=1, max_frac=2e-2, what="qknorm")


@pytest.mark.parametrize("dim,H", [(4096, 32), (48, 4)])
def test_rope_table_matches_oracle(dim, H):
    g = _g(4)
    T = 37
    st = torch.randint(0, 15, (3, T), generator=g).float()
    pos = torch.stack([st, st + torch.randint(1, 4, (3, T), generator=g).float()], -1)
    n_freq = dim // 6
    lin = torch.linspace(0.0, 1.0, n_freq, dtype=torch.float32)
    freq = torch.pow(torch.tensor(10000.0), lin) * (math.pi / 2)
    mp = (20, 2048, 2048)
    c, s, ang, big = R.rope_table(pos, freq, H, dim, mp)
    oc, os_ = O.precompute_freqs_cis(pos[None], dim, max_pos=mp, heads=H)
    bound = (ang.abs() + big) * 2.0 ** -22 + 4 * 2.0 ** -24
    assert bool(((oc[0].double() - c).abs() <= bound).all()) and bool(((os_[0].double() - s).abs() <= bound).all())


@pytest.mark.parametrize("dim", [256, 6])
def test_timestep_embed_matches_oracle(dim):
    t = torch.linspace(0, 1000, 101).to(BF)
    ref, ang = R.timestep_embed(t, dim, 1.0)
    o = P.r(O.get_timestep_embedding(t.float(), dim)).double()
    bound = R.ulp_bf16(ref.abs() + ang.abs() * 2.0 ** -21) + ang.abs() * 2.0 ** -21
    assert bool(((o - ref).abs() <= bound).all())


def test_ada_combine_matches_oracle():
    g = _g(5)
    L, U, K, D = 2, 3, 6, 16
    tab = torch.randn(L, K, D, generator=g).to(BF)
    ada = torch.randn(U, K * D, generator=g).to(BF)
    ref = R.ada_combine(tab, ada, 0b10)
    for l in range(L):
        vals = O.ada_values(tab[l], ada.reshape(1, U, K * D), 0, K, P)          # list over k of (1,U,D)
        for k in range(K):
            want = P.r(1.0 + vals[k][0]) if k == 1 else vals[k][0]
            assert torch.equal(ref[l, :, k].float(), want)


def test_cfg_euler_matches_oracle_chain():
    g = _g(6)
    B, C, S = 2, 16, 20
    vp, vn = torch.randn(B, S, C, generator=g).to(BF), torch.randn(B, S, C, generator=g).to(BF)
    x, clean = torch.randn(B, C, S, generator=g).to(BF), torch.randn(B, C, S, generator=g).to(BF)
    mask = torch.tensor([0.0, 1.0, 0.75]).repeat(S)[:S].repeat(B, 1)
    sig, sn = O.bf16_round_scalar(0.909375), O.bf16_round_scalar(0.725)
    v = O.cfg_combine(vp.float(), vn.float(), 4.0, P).transpose(1, 2)
    x0 = O.to_denoised(x.float(), v, sig, P)
    x0 = O.apply_denoise_mask(x0, clean.float(), mask[:, None, :], P)
    want = O.euler_step(x.float(), x0, sig, sn, P)
    ref, mag = R.cfg_euler_step(vp, vn, x, sig, sn, 4.0, clean, mask)
    R.assert_bf16_close(want, ref, max_ulps=2, max_frac=2e-2, mag=mag, what="cfg chain")
    ref0, _ = R.cfg_euler_step(vp, vn, x, sig, 0.0, 4.0, clean, mask)
    R.assert_bf16_close(x0, ref0, max_ulps=2, max_frac=2e-2, mag=mag, what="sigma_next=0")
    e, emag = R.euler_step(x, x0.to(BF), sig, sn)
    R.assert_bf16_close(O.euler_step(x.float(), x0, sig, sn, P), e, max_ulps=1, max_frac=2e-2, mag=emag, what="euler")


def test_silu_matches_oracle():
    x = torch.linspace(-20, 20, 4001).to(BF)
    R.assert_bf16_close(O.silu(x.float(), P), R.silu(x), max_ulps=1, max_frac=2e-2)


# ---------------------------------------------------------------------------------------------------- VAE glue
@pytest.mark.parametrize("resid,silu", [(False, False), (True, True)])
def test_groupnorm_matches_oracle(resid, silu):
    g = _g(7)
    B, C, D, H, W = 2, 64, 2, 3, 5
    x = (torch.randn(B, C, D, H, W, generator=g) + 50).to(BF)
    gam = (1 + 0.3 * torch.randn(C, generator=g)).to(BF)
    bet = (0.3 * torch.randn(C, generator=g)).to(BF)
    r = torch.randn(B, C, D, H, W, generator=g).to(BF)
    want = OV.group_norm3d(x, gam, bet, P)
    if resid:
        want = P.r(want + r.float())
    if silu:
        want = O.silu(want, P)
    cl = lambda t: t.permute(0, 2, 3, 4, 1).reshape(B, -1, C)
    ref, mag = R.groupnorm_act(cl(x), gam, bet, 32, 1e-5, cl(r) if resid else None, silu)
    R.assert_bf16_close(cl(want), ref, max_ulps=2 if resid else 1, max_frac=2e-2, mag=mag, what="groupnorm")


def test_to_uint8_matches_oracle():
    x = torch.cat([torch.linspace(-1.2, 1.2, 2 * 3 * 4 * 5 * 7 - 2), torch.tensor([math.inf, -math.inf])]).to(BF)
    x = x.reshape(2, 3, 4, 5, 7)
    ref = R.to_uint8(x)
    for b in range(2):
        assert torch.equal(ref[b], OV.to_uint8(x[b].float(), P))


@pytest.mark.parametrize("P_", [1, 2, 4])
def test_patchify_matches_oracle(P_):
    v = torch.randn(2, 3, 3, 4 * P_, 2 * P_, generator=_g(8))
    pt = R.patchify(v, P_, 3 * P_ * P_ + 5)
    assert torch.equal(pt[..., :3 * P_ * P_].permute(0, 4, 1, 2, 3), OV.patchify(v, P_))
    assert not pt[..., 3 * P_ * P_:].any()
    up = R.unpatchify(pt[..., :3 * P_ * P_], 3, P_)
    assert torch.equal(up, OV.unpatchify(OV.patchify(v, P_), P_)) and torch.equal(up, v)


def test_latent_norm_denorm_and_tile_blend_restate_the_formulas():
    g = _g(9)
    B, C, S = 2, 8, 11
    lat = torch.randn(B, C, S, generator=g).to(BF)
    mean = (0.1 * torch.randn(C, generator=g)).to(BF)
    std = (1 + 0.1 * torch.randn(C, generator=g)).abs().to(BF)
    want = P.r(lat.float() * std.float()[None, :, None] + mean.float()[None, :, None]).transpose(1, 2)
    R.assert_bf16_close(want, R.latent_denorm_cl(lat, mean, std)[0], max_ulps=1, max_frac=2e-2)
    tok = lat.transpose(1, 2).contiguous()
    want = P.r((tok.float() - mean.float()) / std.float()).transpose(1, 2)
    R.assert_bf16_close(want, R.latent_norm_cf(tok, mean, std), max_ulps=1, max_frac=2e-2)
    # tile blend: one full-volume tile with unit masks is the identity
    tile = torch.randn(B, 3, 2, 3, 4, generator=g).to(BF)
    one = torch.ones(4)
    out = R.tile_blend([(tile, (2, 3, 4), one, one, one, (0, 0, 0))], 2, 3, 4)
    assert torch.equal(out, tile.double())


# ---------------------------------------------------------------------------------------------------- conv3d, PixelNorm
HALO_MODES = [(c, p, t) for c in (0, 1, 2) for p in (0, 1) for t in (3, 1)]


def _conv_data(B, D, H, W, Cin, Cout, taps_d, seed):
    g = _g(seed)
    nt = 27 if taps_d == 3 else 9
    x = torch.randn(B, D, H, W, Cin, generator=g).to(BF)
    w = (torch.randn((Cout, 3, 3, 3, Cin) if taps_d == 3 else (Cout, 3, 3, Cin), generator=g) * (nt * Cin) ** -0.5).to(BF)
    b = (0.1 * torch.randn(Cout, generator=g)).to(BF)
    return x, w, b


def _torch_conv_f32(x, w, b, causal, pad_mode, taps_d):
    """float32 torch convolution of the same bf16 data, halo by torch's own padding ops: (B,D,H,W,Cout) float32."""
    import torch.nn.functional as F
    xc = x.float().permute(0, 4, 1, 2, 3)                                  # (B,C,D,H,W)
    if taps_d == 3:
        if causal == 2:
            xc = F.pad(xc, (0, 0, 0, 0, 1, 1))
        else:
            xc = F.pad(xc, (0, 0, 0, 0, 2, 0) if causal == 1 else (0, 0, 0, 0, 1, 1), mode="replicate")
    xc = F.pad(xc, (1, 1, 1, 1, 0, 0), mode="reflect") if pad_mode == 1 else F.pad(xc, (1, 1, 1, 1))
    wt = w.float().reshape(w.shape[0], 3 if taps_d == 3 else 1, 3, 3, w.shape[-1]).permute(0, 4, 1, 2, 3).contiguous()
    return F.conv3d(xc, wt, b.float()).permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("causal,reflect", [(1, True), (1, False), (0, True), (0, False)])
def test_conv3d_ref_matches_oracle_causal_conv(causal, reflect):
    x, w, b = _conv_data(2, 3, 4, 5, 64, 16, 3, 20 + causal * 2 + reflect)
    y, mag = R.conv3d(x, w, b, causal, int(reflect))
    want = OV.causal_conv3d(x.permute(0, 4, 1, 2, 3).float(), w, b, P, bool(causal), reflect).permute(0, 2, 3, 4, 1)
    R.assert_bf16_close(want, R.rbf(y), max_ulps=1, max_frac=2e-2, what="causal_conv3d")     # fp32 sum, rounded once
    assert bool((mag >= y.sub(b.double()).abs() - 1e-12).all())


def test_conv3d_ref_matches_oracle_zero_conv_and_residual():
    x, w, b = _conv_data(2, 3, 4, 5, 64, 16, 3, 30)
    y, _ = R.conv3d(x, w, b, 2, 0)
    want = OV.conv3d_zero(x.permute(0, 4, 1, 2, 3).float(), w, b, P).permute(0, 2, 3, 4, 1)
    R.assert_bf16_close(want, R.rbf(y), max_ulps=1, max_frac=2e-2, what="conv3d_zero")
    r = torch.randn(2, 3, 4, 5, 16, generator=_g(31)).to(BF)
    yr, _ = R.conv3d(x, w, b, 2, 0, resid=r)
    assert torch.equal(yr, y + r.double())
    # the per-frame kernel is the centre temporal tap of a 3x3x3 kernel whose other temporal taps are zero
    w1 = w[:, 1].contiguous()
    w3 = torch.zeros_like(w)
    w3[:, 1] = w1
    y1, m1 = R.conv3d(x, w1, b, 0, 1, taps_d=1)
    y3, m3 = R.conv3d(x, w3, b, 0, 1)
    assert torch.equal(y1, y3) and torch.equal(m1, m3)
    for causal in (1, 2):                                   # per frame: no temporal halo mode reaches it
        assert torch.equal(R.conv3d(x, w1, b, causal, 1, taps_d=1)[0], y1)


def test_conv3d_halo_small_extents():
    """D = 1 with causal = 0: both temporal halos are the one frame; H = W = 2 with reflect: the reflected sample is the
    opposite edge."""
    x = torch.arange(2 * 2 * 3, dtype=torch.float64).reshape(1, 1, 2, 2, 3)
    h = R.conv3d_halo(x, 0, 1)
    assert h.shape == (1, 3, 4, 4, 3)
    assert torch.equal(h[:, 0], h[:, 1]) and torch.equal(h[:, 2], h[:, 1])
    assert torch.equal(h[0, 1, 0, 1:3], x[0, 0, 1]) and torch.equal(h[0, 1, 3, 1:3], x[0, 0, 0])
    assert torch.equal(h[0, 1, 1:3, 0], x[0, 0, :, 1]) and torch.equal(h[0, 1, 1:3, 3], x[0, 0, :, 0])
    assert not R.conv3d_halo(x, 2, 0)[:, 0].any() and R.conv3d_halo(x, 1, 0, taps_d=1).shape == (1, 1, 4, 4, 3)


@pytest.mark.parametrize("causal,pad_mode,taps_d", HALO_MODES)
def test_conv3d_bound_accepts_a_float32_convolution(causal, pad_mode, taps_d):
    """bf16(float32 torch conv) of the same bf16 data lies inside the element-wise bound in every halo mode, with and
    without a residual: the bound is not too tight for a correct fp32-accumulating implementation."""
    Cin, Cout = 64, 24
    x, w, b = _conv_data(2, 3, 7, 9, Cin, Cout, taps_d, 40 + causal * 4 + pad_mode * 2 + taps_d)
    K = (27 if taps_d == 3 else 9) * Cin
    c32 = _torch_conv_f32(x, w, b, causal, pad_mode, taps_d)
    y, mag = R.conv3d(x, w, b, causal, pad_mode, taps_d)
    d, bound = R.conv3d_bound(c32.to(BF), y, mag, K)
    assert bool((d <= bound).all()), float((d / bound).max())
    assert float((d / bound).max()) > 0.5                    # and it is no loose bound: some element uses half of it
    r = torch.randn(2, 3, 7, 9, Cout, generator=_g(41)).to(BF)
    yr, _ = R.conv3d(x, w, b, causal, pad_mode, taps_d, resid=r)
    d, bound = R.conv3d_bound((c32.to(BF).float() + r.float()).to(BF), yr, mag, K, resid=r)
    assert bool((d <= bound).all()), float((d / bound).max())


@pytest.mark.parametrize("causal", [0, 1])
def test_conv3d_bound_rejects_one_wrong_halo_tap(causal):
    """The same float32 output fails the bound when (a) one corner voxel is recomputed with one zero tap where the mode
    says reflect, (b) the voxels of one frame take their temporal halo from the wrong end - and only those voxels fail."""
    Cin, Cout = 64, 24
    B, D, H, W = 2, 3, 7, 9
    x, w, b = _conv_data(B, D, H, W, Cin, Cout, 3, 50 + causal)
    K = 27 * Cin
    y, mag = R.conv3d(x, w, b, causal, 1)
    good = _torch_conv_f32(x, w, b, causal, 1, 3)
    # (a) voxel (b=1, d=1, h=0, w=0): the tap (kd, kh, kw) = (1, 0, 0) reads reflect sample x[1, 1, 1, 1]; drop it
    bad = good.clone()
    bad[1, 1, 0, 0] -= x[1, 1, 1, 1].float() @ w[:, 1, 0, 0].float().t()
    d, bound = R.conv3d_bound(bad.to(BF), y, mag, K)
    over = (d > bound).any(-1)
    assert bool(over[1, 1, 0, 0]) and int(over.sum()) == 1
    # (b) frame 0 convolved with the halo frames swapped end for end: [last, x, first]
    xs = torch.cat([x[:, -1:], x, x[:, :1]], 1)
    ys, _ = R.conv3d(xs, w, b, 2, 1)                          # zeros in time never reach frames 1 .. D of xs
    bad = good.clone()
    bad[:, 0] = ys[:, 1].float()
    d, bound = R.conv3d_bound(bad.to(BF), y, mag, K)
    over = (d > bound).any(-1)
    assert bool(over[:, 0].all()) and not bool(over[:, 1:].any())


@pytest.mark.parametrize("mod", [False, True], ids=["nomod", "mod"])
@pytest.mark.parametrize("silu_on", [False, True], ids=["nosilu", "silu"])
def test_pixelnorm_act_matches_oracle(mod, silu_on):
    g = _g(60 + 2 * mod + silu_on)
    B, C, V = 2, 128, 30
    x = (torch.randn(B * V, C, generator=g) * 3).to(BF)
    x[3] = 0.0
    sc, sh = (0.5 * torch.randn(B, C, generator=g)).to(BF), torch.randn(B, C, generator=g).to(BF)
    for eps in (1e-8, 1e-6):
        xc = x.float().reshape(B, V, C).permute(0, 2, 1).reshape(B, C, V, 1, 1)
        want = OV.pixel_norm(xc, P, eps)
        if mod:
            want = OV._mod(want, sc.float().reshape(B, C, 1, 1, 1), sh.float().reshape(B, C, 1, 1, 1), P)
        if silu_on:
            want = O.silu(want, P)
        want = want.reshape(B, C, V).permute(0, 2, 1).reshape(B * V, C)
        ref, mag, exempt = R.pixelnorm_act(x, R.f32(eps), sc if mod else None, sh if mod else None, V, silu_on)
        assert not bool(exempt.any())
        R.assert_bf16_close(want, ref, max_ulps=2 if mod else 1, max_frac=1e-2, mag=mag, what="pixelnorm_act")
        assert not bool(ref[3].any()) or mod


@pytest.mark.parametrize("C", [64, 128, 256, 512, 1024, 2048])
def test_pixelnorm_gpu_inputs_have_few_exempt_rows(C):
    """The condition the GPU test's max_frac rests on, for the exact inputs it uses: rows whose statistic sits on a bf16
    rounding boundary (they may flip as a whole row) are at most 1 % of the rows, in every variant."""
    x, sc, sh = R.pixelnorm_inputs(C)
    V = R.pixelnorm_rows(C)
    assert x.shape == (V, C) and V >= 257 and V % 2 == 1
    rows_per_wg = 4 * (64 // min(C // 8, 64))
    assert (V - 1) % (2 * rows_per_wg) == 0 and R.PIXELNORM_RPB % 8 != 0 and R.PIXELNORM_RPB % 2 != 0 and R.PIXELNORM_RPB < V
    assert not bool(x[5].any()) and bool((x[7] == x[7, 0]).all()) and float(x[7, 0]) != 0.0
    _, _, exempt = R.pixelnorm_act(x, R.f32(1e-8), sc, sh, R.PIXELNORM_RPB, True)
    assert int(exempt.sum()) <= V // 100, int(exempt.sum())
    # the detector itself: a value a relative 2^-20 above a midpoint is near it, 2^-16 is not
    mid = torch.tensor([1.0 + 2.0 ** -8, 3.0 + 2.0 ** -7, 2.0 ** -20 * (1.5 + 2.0 ** -8)], dtype=torch.float64)
    assert bool(R.near_bf16_midpoint(mid * (1 + 2.0 ** -20)).all()) and not bool(R.near_bf16_midpoint(mid * (1 + 2.0 ** -16)).any())


# ------------------------------------------------------------------------------------------------ flash attention bound
ATTN_SCALE = 1.0 / math.sqrt(128)
ATTN_SHAPES = [(1, 3, 200, 70), (1, 2, 77, 200), (2, 2, 129, 65), (1, 1, 16, 5), (1, 2, 320, 1296)]
ATTN_SEEDS = (0, 1)
_ATTN_REF = {}


def _attn_ref(shape, family, seed):
    """(q, k, v, planted, (y, A, dx)) of one case, computed once and shared (nothing below writes into it)."""
    key = (shape, family, seed)
    if key not in _ATTN_REF:
        B, H, Tq, Tk = shape
        q, k, v, planted = R.attention_inputs(B, H, Tq, Tk, family, seed)
        _ATTN_REF[key] = (q, k, v, planted, R.attention(q, k, v, H, ATTN_SCALE))
    return _ATTN_REF[key]


def _attn_ratio(out, ref, Tk):
    d, bound = R.attention_bound(out, *ref, Tk)
    return d / bound


def _attn_emulate(q, k, v, H, *, split=False, fault=None, extra_key=None, scale=ATTN_SCALE):
    """What fa_body16 does, in fp32 on the CPU: 64-key tiles, the ragged last tile's slots masked with -1e30, per 16-row
    query block (rows past Tq clamped to Tq-1) an online softmax with an integer offset that is raised - to ceil of the
    block rows' own maxima - only when some row's tile maximum exceeds it by more than 6; P = exp2(fma(s, c, -M)) rounded
    to bf16 for P.V, l summed from the un-rounded fp32 P.  split: the keys of each tile halved (32 | 32) over two
    accumulators that are merged at the end with exp2(m_i - m); a second half that saw only masked keys (Tk <= 32) is
    left out of the merge, as the kernel leaves it out.
    fault: 'skip_block' - the 16-key block that holds key Tk-1 left out for the last 16-row query block;
           'swap_merge' - the two halves' merge weights exchanged;
           'merge_dead_half' - the all-masked second half merged like any other.
    extra_key: (k_row, v_row) appended as one more, unmasked, key."""
    B, Tq, D = q.shape
    Tk = k.shape[1]
    c = R.attn_c(scale)
    qh = q.float().reshape(B, Tq, H, 128).transpose(1, 2)
    kh = k.float().reshape(B, Tk, H, 128).transpose(1, 2)
    vh = v.float().reshape(B, Tk, H, 128).transpose(1, 2)
    if extra_key is not None:
        kh = torch.cat([kh, extra_key[0].float().reshape(B, 1, H, 128).transpose(1, 2)], 2)
        vh = torch.cat([vh, extra_key[1].float().reshape(B, 1, H, 128).transpose(1, 2)], 2)
        Tk += 1
    nb = -(-Tq // 16)
    rows = torch.arange(nb * 16).clamp_max(Tq - 1)
    qh = qh[:, :, rows]                                                       # (B,H,nb*16,128), clamped rows
    nt = -(-Tk // 64)
    pad = nt * 64 - Tk
    s = qh @ kh.transpose(-1, -2)                                             # fp32
    s = torch.cat([s, torch.full((B, H, nb * 16, pad), -1e30)], -1)
    vh = torch.cat([vh, torch.full((B, H, pad, 128), 1024.0)], 2)             # live padding: P must be exactly 0 there
    if fault == "skip_block":
        kb = (Tk - 1) // 16
        s[:, :, (nb - 1) * 16:, kb * 16:(kb + 1) * 16] = -1e30
    s = s.reshape(B, H, nb, 16, nt, 64)
    halves = [(0, 32), (32, 64)] if split else [(0, 64)]
    acc = []
    for lo, hi in halves:
        m = torch.full((B, H, nb, 16, 1), -1e30)
        l = torch.zeros(B, H, nb, 16, 1)
        o = torch.zeros(B, H, nb, 16, 128)
        for t in range(nt):
            st = s[:, :, :, :, t, lo:hi]
            mxc = st.amax(-1, keepdim=True) * np.float32(c)                  # fp32 product, as mx * p.c
            raise_ = ((mxc - m) > 6.0).any(dim=3, keepdim=True)               # one decision per 16-row block
            m_new = torch.where(raise_, torch.maximum(m, torch.ceil(mxc)), m)
            alpha = torch.exp2(m - m_new)
            l, o, m = l * alpha, o * alpha, m_new
            p = torch.exp2((st.double() * c - m.double()).float())            # fma: one rounding of the exponent
            l = l + p.sum(-1, keepdim=True)
            o = o + p.to(BF).float() @ vh[:, :, None, t * 64 + lo:t * 64 + hi]
        acc.append((m, l, o))
    if split:
        (m0, l0, o0), (m1, l1, o1) = acc
        m = torch.maximum(m0, m1)
        a0, a1 = torch.exp2(m0 - m), torch.exp2(m1 - m)
        if fault == "swap_merge":
            a0, a1 = a1, a0
        if Tk > 32 or fault is not None:
            l, o = l0 * a0 + l1 * a1, o0 * a0 + o1 * a1
        else:
            l, o = l0, o0
    else:
        _, l, o = acc[0]
    out = (o * (1.0 / l)).to(BF).reshape(B, H, nb * 16, 128)[:, :, :Tq]
    return out.transpose(1, 2).reshape(B, Tq, D)


def _attn_exact_bf16(q, k, v, H, scale=ATTN_SCALE):
    """bf16 of the exact result: the output of a kernel with no error but the final rounding."""
    return R.rbf(R.attention(q, k, v, H, scale)[0]).to(BF)


@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", R.ATTN_FAMILIES)
def test_attention_bound_accepts_every_correct_computation(shape, family):
    """ref64.attention_bound must pass, on every element, the oracle's flash policy, its fp32-P policy and an fp32
    emulation of the kernel's own loop with and without the key split.  Worst d / bound measured here over the five shapes
    and two seeds, per family (flat, peaked, spiked):
        O.BF16_FLASH      0.692  0.866  0.890
        O.BF16            0.473  0.467  0.472   (P stays fp32: the final rounding alone)
        emulation         0.692  0.866  0.890
        emulation, split  0.692  0.866  0.890
    (the three bf16-P computations agree to the digits shown: the worst element is set by the rounding of P, which the
    integer offset makes the same in all of them; with 2^-9 for that rounding the flash policy reaches 1.1 to 1.33)."""
    B, H, Tq, Tk = shape
    for seed in ATTN_SEEDS:
        q, k, v, planted, ref = _attn_ref(shape, family, seed)
        if family == "spiked":
            p = R.attention_probs(q, k, H, ATTN_SCALE)[0]
            assert planted and all(float(p[:, :, r, j].min()) >= 0.25 for r, j in planted), (shape, seed, planted)
        outs = {"flash": O.sdpa(q.float(), k.float(), v.float(), H, O.BF16_FLASH), "fp32_p": O.sdpa(q.float(), k.float(), v.float(), H, O.BF16),
                "emulation": _attn_emulate(q, k, v, H), "emulation_split": _attn_emulate(q, k, v, H, split=True)}
        for name, out in outs.items():
            worst = float(_attn_ratio(out, ref, Tk).max())
            print(f"attention bound {shape} {family} seed {seed} {name}: worst d/bound {worst:.3f}")
            assert worst <= 1.0, (name, shape, family, seed, worst)


@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", R.ATTN_FAMILIES)
def test_attention_bound_rejects_seeded_faults(shape, family):
    """Each fault a kernel could have must put at least one element beyond the bound: the last key dropped; one more key
    that repeats key Tk-1 with v = 1024 (an unmasked pad slot); the last query row carrying row Tq-2's result; one 16-key
    block skipped for one 16-row query block; the merge weights of the two key halves exchanged.  Measured here over the
    shapes, families and seeds, worst d / bound (fewest rows beyond): key dropped 4.7 - 490 (11), pad slot 350 - 510 (15), row
    moved 36 - 440 (1: the row itself), block skipped 1.1 - NaN (1; 1.1 where the block holds a single live key), weights
    exchanged 56 - NaN (16)."""
    B, H, Tq, Tk = shape
    for seed in ATTN_SEEDS:
        q, k, v, _, ref = _attn_ref(shape, family, seed)
        good = _attn_exact_bf16(q, k, v, H)
        faults = {}
        if Tk > 1:
            faults["last_key_dropped"] = _attn_exact_bf16(q, k[:, :-1], v[:, :-1], H)
        faults["pad_slot_unmasked"] = _attn_emulate(q, k, v, H, extra_key=(k[:, -1:], torch.full_like(v[:, -1:], 1024.0)))
        if Tq > 1:
            moved = good.clone()
            moved[:, -1] = good[:, -2]
            faults["last_row_is_the_row_before"] = moved
        faults["key_block_skipped"] = _attn_emulate(q, k, v, H, fault="skip_block")
        faults["merge_weights_swapped"] = _attn_emulate(q, k, v, H, split=True, fault="swap_merge")
        for name, out in faults.items():
            ratio = _attn_ratio(out, ref, Tk)
            n = int((ratio > 1.0).any(-1).sum())
            print(f"attention bound {shape} {family} seed {seed} {name}: {n} rows beyond, worst {float(ratio.max()):.3g}")
            assert n >= 1, (name, shape, family, seed)


@pytest.mark.parametrize("shape", [(1, 4, 77, 70), (2, 4, 129, 65)], ids=lambda s: "x".join(map(str, s)))
def test_attention_fused_prep_allowance(shape):
    """The fused query preparation is held to the bound centred on attention(q', k, v), q' = qknorm_rope(q), with dx
    enlarged by ref64.attention_fused_dx.  Two one-ulp flips per row and head of q' stay inside it; q' rotated with the
    next row's cos / sin, or scaled with the next head's weight, does not."""
    B, H, Tq, Tk = shape
    D = H * 128
    for seed in ATTN_SEEDS:
        q, k, v, _ = R.attention_inputs(B, H, Tq, Tk, "flat", seed)
        g = _g(seed + 17)
        w = (1 + 0.1 * torch.randn(1, D, generator=g)).to(BF)
        ang = torch.rand(H, Tq, 64, generator=g) * (2 * math.pi)
        cos, sin = torch.cos(ang), torch.sin(ang)
        prep = lambda w_, c_, s_: R.qknorm_rope(q.reshape(B * Tq, D), w_, c_, s_, Tq, H, 1e-6)[0].to(BF).reshape(B, Tq, D)
        qp = prep(w, cos, sin)
        k, _ = R.attention_plant(qp, k)                                     # spiked on q': the flips land on dominant keys too
        y, A, dx = R.attention(qp, k, v, H, ATTN_SCALE)
        ref = (y, A, dx + R.attention_fused_dx(qp, k, H, ATTN_SCALE))
        flipped = qp.clone().reshape(B, Tq, H, 128)
        up = lambda t: (t.view(torch.int16) + 1).view(BF)                  # the next bf16 away from zero
        flipped[..., 3] = up(flipped[..., 3].contiguous())
        flipped[..., 100] = up(flipped[..., 100].contiguous())
        inside = _attn_ratio(_attn_exact_bf16(flipped.reshape(B, Tq, D), k, v, H), ref, Tk)
        assert float(inside.max()) <= 1.0, (shape, seed, float(inside.max()))
        wrong = {"next_row_table": prep(w, cos.roll(-1, 1), sin.roll(-1, 1)), "next_head_weight": prep(w.roll(-128, 1), cos, sin)}
        for name, qw in wrong.items():
            ratio = _attn_ratio(_attn_exact_bf16(qw, k, v, H), ref, Tk)
            assert int((ratio > 1.0).sum()) >= 1, (name, shape, seed)


def test_attention_inputs_planted_keys_dominate_on_every_gpu_case_shape():
    """The spiked family's precondition at every shape tests/test_attn_bound_gpu.py launches (seed 0, the one it uses): from
    the float64 P, each planted key holds at least 0.25 of its row's mass - in every batch and head."""
    import test_attn_bound_gpu as G
    for shape in G.ALL_SHAPES:
        B, H, Tq, Tk = shape
        q, k, _, planted = R.attention_inputs(B, H, Tq, Tk, "spiked", 0)
        assert len(planted) == len({j for j in (0, 31, 32, 63, 64, Tk - 1, 64 * ((Tk - 1) // 64)) if j < Tk})
        p = R.attention_probs(q, k, H, ATTN_SCALE)[0]
        worst = min(float(p[:, :, r, j].min()) for r, j in planted)
        assert worst >= 0.25, (shape, worst)


@pytest.mark.parametrize("scale", [0.1, 0.09, 1.0])
def test_attention_bound_at_other_scales_and_the_all_masked_key_half(scale):
    """The bound is a function of the scale, not fitted to 1/sqrt(128).  At Tk <= 32 the second key half of a split tile sees
    masked keys only: its offset is ceil(fp32(-1e30 * c)) and its P is exp2 of the fma's rounding residual, ~+-1e21 - 0 at
    1/sqrt(128) and 0.09, +inf at 0.1, where merging that half gives inf * 0 (from c = 1 up the offset is never raised
    from its initial -1e30 and P = 0).  The kernel leaves such a half out;
    the bound accepts that at every scale and rejects the merged form wherever the residual is positive."""
    c = R.attn_c(scale)
    masked = float(np.float32(-1e30))
    mxc = float(np.float32(np.float32(masked) * np.float32(c)))
    M = mxc if mxc - masked > 6.0 else masked          # c >= 1: the half's offset stays at its initial -1e30 and P = exp2(-huge) = 0
    residual = masked * c - M                          # exact in float64 (24 x 24 bits)
    for shape in [(1, 1, 16, 5), (1, 2, 77, 32), (2, 2, 129, 65)]:
        B, H, Tq, Tk = shape
        q, k, v, _ = R.attention_inputs(B, H, Tq, Tk, "flat", 0)
        ref = R.attention(q, k, v, H, scale)
        for split in (False, True):
            worst = float(_attn_ratio(_attn_emulate(q, k, v, H, split=split, scale=scale), ref, Tk).max())
            assert worst <= 1.0, (shape, scale, split, worst)
        if Tk <= 32:
            merged = _attn_ratio(_attn_emulate(q, k, v, H, split=True, fault="merge_dead_half", scale=scale), ref, Tk)
            assert bool((merged > 1.0).all()) == (residual > 128), (shape, scale, residual, float(merged.max()))
