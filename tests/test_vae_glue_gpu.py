"""VAE and latent-upsampler glue kernels at their edge shapes, against the float64 references of tests/ref64.py (and,
for the exact ones, against the oracle or a float32 restatement in the kernel's own operation order).  Outputs go into
buffers with a NaN-sentinel tail that must survive bit for bit; bounds as in test_rowops_gpu.py.  The calls go through the
``ops`` shims with ``out=`` a view of the sentinel buffer; ``pixelnorm_act`` and ``groupnorm_act`` allocate their output, so
their two sentinel tests hand the C entry the buffer themselves.  Every bf16 output is also held, element by element, to its
admissible interval of tests/ref_rows.py (``_within``; for PixelNorm every row counts, none is exempt)."""
import math

import parity
import pytest
import torch

import ref64 as R
import ref_rows as RR
from oracle import dit as O
from oracle import vae as OV
from test_rowops_gpu import _all_finite_bf16, _close, _g, _sent_bf16, _untouched, _within

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _lib():
    from mlx_video_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------- PixelNorm (+mod, +SiLU)
@pytest.mark.parametrize("silu", [False, True], ids=["nosilu", "silu"])
@pytest.mark.parametrize("mod", [False, True], ids=["nomod", "mod"])
@pytest.mark.parametrize("C", [64, 128, 256, 512, 1024, 2048])
def test_pixelnorm_act_edges(dev, C, mod, silu):
    """ltxk_pixelnorm_act, LPR = min(C/8, 64) lanes per row and R = 4 * 64/LPR rows per workgroup, at V = 2*R*k + 1 = 257
    rows: whole workgroups plus a lone row in the last one (its idle lanes and waves must not store: sentinel rows follow).
    Two batches of 129 and 128 rows with another modulation row each; 129 is no multiple of the 8, 4 or 2 rows a wave
    holds, so one wave has rows of both.  Row 5 is all zero (eps alone under the root), row 7 constant.  Catches: the
    second pass of C = 1024 / 2048 dropped or doubled in the mean, a row statistic reduced over a neighbour's lanes, the
    batch taken per wave instead of per row, 1 + scale not rounded, and stores past V*C.
    max_ulps 1 without modulation, 2 with it (an earlier rounding point may flip and carry), max_frac 1e-2: the rule of
    test_rowops_gpu.py.  A row whose statistic sits within 2^-18 of a bf16 rounding boundary may flip as a whole: those
    rows (ref64.pixelnorm_act names them) count towards max_ulps only, and test_ref64_cpu.py asserts on these very inputs
    that they are at most 1 % of the rows."""
    L = _lib()
    x, sc, sh = R.pixelnorm_inputs(C)
    V = R.pixelnorm_rows(C)
    eps = 1e-8
    n = V * C
    out = _sent_bf16((n + 4 * C,), dev)
    xd, scd, shd = x.to(dev), sc.to(dev), sh.to(dev)
    L.check(L.load().ltxk_pixelnorm_act(xd.data_ptr(), out.data_ptr(), V, C, eps, scd.data_ptr() if mod else None,
                                        shd.data_ptr() if mod else None, R.PIXELNORM_RPB, int(silu), _st()), "ltxk_pixelnorm_act")
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    ref, mag, exempt = R.pixelnorm_act(x, R.f32(eps), sc if mod else None, sh if mod else None, R.PIXELNORM_RPB, silu)
    assert int(exempt.sum()) <= V // 100
    got = out[:n].view(V, C).cpu()
    if not mod:
        assert not bool(got[5].float().any()), "the all-zero row"
    max_ulps = 2 if mod else 1
    ulps, _ = R.bf16_stats(got, ref, mag)
    _, frac = R.bf16_stats(got[~exempt], ref[~exempt], None if mag is None else mag[~exempt])
    parity.auto(ulps, max_ulps, tag="ulps")
    parity.auto(frac, 1e-2, tag="frac")
    R.assert_rows_close(got, ref, exempt, max_ulps=max_ulps, max_frac=1e-2, mag=mag, what=f"pixelnorm C={C}")
    # every row, none exempt: the rounded row statistics m, e, s are intervals themselves
    _within(got, RR.pixelnorm_act(x, R.f32(eps), sc if mod else None, sh if mod else None, R.PIXELNORM_RPB, silu))


# ------------------------------------------------------------------------------------------- GroupNorm (+res, +SiLU)
@pytest.mark.parametrize("silu", [False, True], ids=["nosilu", "silu"])
@pytest.mark.parametrize("resid", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("C,V", [(64, 1), (96, 7), (512, 1), (512, 7), (64, 12480), (96, 12480)])
def test_groupnorm_act_edges(dev, C, V, resid, silu):
    """GroupNorm3d, G = 32 (C/G = 2, 3, 16), one 256-thread workgroup per (batch, group), B = 2; V = 12480 is a
    13x24x40 post-pixel-shuffle latent.  Channels carry a common offset of 50 with std 1.  Catches: a one-pass variance
    (cancels at offset 50), a strided loop that skips or repeats elements when V*C/G is not a multiple of 256 (V = 1, 7),
    gamma/beta indexed by the in-group channel instead of the channel, the second batch normalised with the first
    batch's statistics, and stores past B*V*C."""
    L = _lib()
    inp = RR.groupnorm_inputs(C, V, resid, silu)
    B, G, x, gam, bet, r = inp.B, inp.G, inp.x, inp.gam, inp.bet, inp.r
    n = B * V * C
    out = _sent_bf16((n + 64,), dev)
    rd = r.to(dev) if resid else None
    x_d = x.to(dev)
    gam_d = gam.to(dev)
    bet_d = bet.to(dev)
    L.check(L.load().ltxk_groupnorm_act(x_d.data_ptr(), out.data_ptr(), gam_d.data_ptr(), bet_d.data_ptr(),
                                        rd.data_ptr() if resid else None, B, V, C, G, 1e-5, int(silu), _st()),
            "ltxk_groupnorm_act")
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    ref, mag = R.groupnorm_act(x, gam, bet, G, R.f32(1e-5), r, silu)
    _close(out[:n].view(B, V, C).cpu(), ref, max_ulps=2 if (resid or silu) else 1, max_frac=1e-2, mag=mag)
    _within(out[:n].view(B, V, C).cpu(), RR.groupnorm_act(x, gam, bet, G, R.f32(1e-5), r, silu), cap=RR.cap(RR.groupnorm_cancels(V)))


# ------------------------------------------------------------------------------------------- latent (de)normalisation
@pytest.mark.parametrize("noise_scale", [0.0, 0.05, 1.0])
def test_latent_denorm_cl_edges(dev, noise_scale):
    """(B=2, C=128, S=65) channels-first -> channels-last with x*std + mean, with the timestep-conditioned noise blend
    at noise_scale 0.05 and 1.0 (0: no noise).  Catches: the partial last 64-wide block along S, mean/std indexed by the
    8-channel group instead of the channel, the blend weights swapped, and stores past B*S*C."""
    from mlx_video_amd import ops
    inp = RR.latent_denorm_inputs(noise_scale)
    B, C, S, lat, noise, mean, std = inp.B, inp.C, inp.S, inp.lat, inp.noise, inp.mean, inp.std
    n = B * S * C
    out = _sent_bf16((n + 64,), dev)
    nd = noise.to(dev) if noise_scale else None
    lat_d = lat.to(dev)
    mean_d = mean.to(dev)
    std_d = std.to(dev)
    ops.latent_denorm_cl(lat_d, mean_d, std_d, nd, noise_scale, out=out[:n].view(B, S, C))
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    ref, mag = R.latent_denorm_cl(lat, mean, std, noise, noise_scale)
    _close(out[:n].view(B, S, C).cpu(), ref, max_ulps=2 if noise_scale else 1, max_frac=4e-2, mag=mag)   # 1.6 % measured
    _within(out[:n].view(B, S, C).cpu(), RR.latent_denorm_cl(lat, mean, std, noise, noise_scale),
            cap=RR.cap(RR.latent_denorm_ties(noise_scale)))


@pytest.mark.parametrize("pad", [0, 64])
def test_latent_norm_cf_edges(dev, pad):
    """(B=2, S=65, ldx = C + pad) channels-last -> (B, C=128, S) with (x - mean)/std, std values that are not powers
    of two.  Catches: rows read at stride C instead of ldx (the pad columns hold NaN), the partial last block along S,
    and stores past B*C*S.  Exact against float32 (x - mean)/std -> bf16; within one ulp of float64."""
    from mlx_video_amd import ops
    inp = RR.latent_norm_inputs(pad)
    B, C, S, ldx, x, mean, std = inp.B, inp.C, inp.S, inp.ldx, inp.x, inp.mean, inp.std
    xb = _sent_bf16((B, S, ldx), dev)
    xb[..., :C] = x.to(dev)
    n = B * C * S
    out = _sent_bf16((n + 64,), dev)
    mean_d = mean.to(dev)
    std_d = std.to(dev)
    ops.latent_norm_cf(xb[..., :C], mean_d, std_d, out=out[:n].view(B, C, S))
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    got = out[:n].view(B, C, S).cpu()
    want = ((x.float() - mean.float()) / std.float()).to(BF).transpose(1, 2)
    _close(got, want, max_ulps=0, max_frac=0.0, tag="f32_")
    _close(got, R.latent_norm_cf(x, mean, std), max_ulps=1, max_frac=1e-2, tag="f64_")
    _within(got, RR.latent_norm_cf(x, mean, std), tag="f64_")


# ------------------------------------------------------------------------------------------- tiled-decode blending
def test_tile_blend_edges(dev):
    """Three overlapping tiles on a (B=2, C=3, 5x9x11) volume, one of them with a partial used box (at < Tt, ah < Th,
    aw < Tw) at the volume border, and voxels that no tile covers.  Catches: the tile indexed with the used box instead
    of its own (Tt, Th, Tw) strides, the masks applied to the wrong axis, a wsum per channel instead of per voxel,
    uncovered voxels coming out NaN/inf instead of 0 (max(wsum, 1e-8)), and stores past B*C*F*H*W.  Bit for bit against a
    float32 restatement in launch order; within one ulp of float64."""
    from mlx_video_amd import ops
    inp = RR.tile_blend_inputs()
    B, C, F, H, W, tiles = inp.B, inp.C, inp.F, inp.H, inp.W, inp.tiles
    S = F * H * W
    acc = torch.zeros((B, C, F, H, W), device=dev)
    ws = torch.zeros((B, 1, F, H, W), device=dev)
    keep = []
    for tile, (at, ah, aw), mt, mh, mw, (t0, h0, w0) in tiles:
        td, md = tile.to(dev), [m.to(dev) for m in (mt, mh, mw)]
        keep += [td] + md
        ops.tile_blend_accum(td, md[0][:at], md[1][:ah], md[2][:aw], acc, ws, t0, h0, w0)
    n = B * C * S
    out = _sent_bf16((n + 64,), dev)
    ops.tile_blend_finalize(acc, ws, out=out[:n].view(B, C, F, H, W))
    torch.cuda.synchronize()
    assert _untouched(out[n:])
    got = out[:n].view(B, C, F, H, W).cpu()
    # float32 restatement, same launch order and the same operation order per voxel
    a32 = torch.zeros(B, C, F, H, W)
    w32 = torch.zeros(B, 1, F, H, W)
    covered = torch.zeros(F, H, W, dtype=torch.bool)
    for tile, (at, ah, aw), mt, mh, mw, (t0, h0, w0) in tiles:
        m = (mt[:at, None, None] * mh[None, :ah, None]) * mw[None, None, :aw]
        a32[:, :, t0:t0 + at, h0:h0 + ah, w0:w0 + aw] += tile[:, :, :at, :ah, :aw].float() * m
        w32[:, :, t0:t0 + at, h0:h0 + ah, w0:w0 + aw] += m
        covered[t0:t0 + at, h0:h0 + ah, w0:w0 + aw] = True
    assert not bool(covered.all())                                   # the case needs uncovered voxels
    assert bool((got[:, :, ~covered] == 0).all())
    want = (a32 / w32.clamp_min(1e-8)).to(BF)
    _close(got, want, max_ulps=0, max_frac=0.0, tag="f32_")
    _close(got, R.tile_blend(tiles, F, H, W), max_ulps=1, max_frac=1e-2, tag="f64_")
    _within(got, RR.tile_blend(tiles, F, H, W), tag="f64_")


# ------------------------------------------------------------------------------------------- uint8 frames
def test_to_uint8_every_value(dev):
    """Every finite bf16 in [-4, 4] plus +-inf, laid out as (B=2, C=3, F=5, H=37, W=33) (odd H and W).  Catches: a
    clamp placed before a rounding point instead of after it, rounding instead of truncating, the (B,C,F,H,W) ->
    (B,F,H,W,C) map wrong at odd extents, and stores past the frame buffer.  Exact against oracle/vae.py::to_uint8."""
    from mlx_video_amd import ops
    B, C, F, H, W = 2, 3, 5, 37, 33
    n = B * C * F * H * W
    vals = torch.cat([_all_finite_bf16(-4.0, 4.0), torch.tensor([math.inf, -math.inf]).to(BF)])
    assert vals.numel() <= n
    x = torch.cat([vals, torch.linspace(-1.5, 1.5, n - vals.numel()).to(BF)])
    x = x[torch.randperm(n, generator=_g(3))].reshape(B, C, F, H, W)
    out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=dev)
    x_d = x.to(dev)
    ops.to_uint8(x_d, out=out[:n].view(B, F, H, W, C))
    torch.cuda.synchronize()
    assert bool((out[n:] == 0xA5).all())
    got = out[:n].view(B, F, H, W, C).cpu()
    want = torch.stack([OV.to_uint8(x[b].float(), O.BF16) for b in range(B)])
    mism = int((got != want).sum())
    parity.auto(float(mism), 0.0, tag="oracle_mismatches")
    assert torch.equal(got, R.to_uint8(x))


# ------------------------------------------------------------------------------------------- (un)patchify
@pytest.mark.parametrize("P", [1, 2, 4])
def test_patchify_roundtrip_edges(dev, P):
    """patchify_cl with Cpad > C*P*P (pad channels must come out 0) and unpatchify_cf, B = 2, C = 3, odd D = 3 and odd
    patch counts (3 x 5).  Catches: the (c, p_w, p_h) channel order swapped to (c, p_h, p_w), pad channels left
    unwritten, the P = 4 vector store misplaced, and stores past either output.  Exact against OV.patchify /
    OV.unpatchify; unpatchify(patchify(x)) == x."""
    from mlx_video_amd import ops
    B, C, D = 2, 3, 3
    H, W = 3 * P, 5 * P
    v = torch.randn(B, C, D, H, W, generator=_g(P)).to(BF)
    cpp = C * P * P
    cpad = cpp + 5
    n1 = B * D * (H // P) * (W // P) * cpad
    pt = _sent_bf16((n1 + 64,), dev)
    vd = v.to(dev)
    ops.patchify_cl(vd, P, cpad, out=pt[:n1].view(B, D, H // P, W // P, cpad))
    n2 = B * D * (H // P) * (W // P) * cpp
    ptc = ops.patchify_cl(vd, P, cpp)
    assert ptc.numel() == n2
    n3 = B * C * D * H * W
    up = _sent_bf16((n3 + 64,), dev)
    ops.unpatchify_cf(ptc, C, P, out=up[:n3].view(B, C, D, H, W))
    torch.cuda.synchronize()
    assert _untouched(pt[n1:]) and _untouched(up[n3:])
    got = pt[:n1].view(B, D, H // P, W // P, cpad).cpu()
    assert not bool(got[..., cpp:].float().any()), "pad channels not zero"
    assert torch.equal(got[..., :cpp].permute(0, 4, 1, 2, 3), OV.patchify(v, P))
    assert torch.equal(got, R.patchify(v, P, cpad))
    upc = up[:n3].view(B, C, D, H, W).cpu()
    assert torch.equal(upc, OV.unpatchify(OV.patchify(v, P), P))
    assert torch.equal(upc, v)
    parity.auto(0.0, 0.0, tag="exact")
