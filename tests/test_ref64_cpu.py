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
