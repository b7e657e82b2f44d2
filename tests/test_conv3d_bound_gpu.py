"""Every launch form of ltxk_conv3d_k3_bf16 at its smallest shapes, held element by element to the float64 bound the GEMMs
already meet (tests/test_gemm_splitk_gpu.py): with y = sum x*w + bias and mag = sum |x*w| in float64 (ref64.conv3d: explicit
halo, one matmul per tap, on the device) and K = taps * Cin,

    |out - y| <= 1/2 ulp_bf16(out) + K 2^-24 mag + 2^-24 (|y| + K 2^-24 mag)

(ref64.conv3d_bound; with a residual the two-rounding form: every epilogue, the split-K finalize included, computes
bf16(bf16(acc + bias) + resid)).  The bound holds for any summation order, so it is the same for the per-tap kernel, the
kw-reuse kernel, K slices and tail launches.  One missing or misplaced halo tap moves a voxel by ~1/sqrt(27) of its size,
hundreds of times the bound; a tail launch that ignores m_base moves whole rows.  tests/test_ref64_cpu.py shows both on the
CPU (the bound accepts a float32 convolution and rejects one wrong tap).

The C ABI is called directly, so workspace, out = NULL and act_out are the test's: every case first asserts the form it aims
at (ltxk_conv3d_plan on the very argument struct it launches; tests/test_conv3d_plan_cpu.py has the rules), writes into a
flat buffer whose rows past the last voxel hold NaN sentinels that must survive, and records its worst d / bound in the
parity ledger.  Case tables: (B, D, H, W); modes = temporal halo {0, 1, 2} x spatial {zeros, reflect} x taps {3, 1}."""
import ctypes

import parity
import pytest
import torch

import ref64 as R
import ref_rows as RR
from test_rowops_gpu import _sent_bf16, _sent_f32, _untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
SENT_ROWS = 3
CP_MODES = [(c, p) for c in (0, 1, 2) for p in (0, 1)]                 # (causal, pad_mode)
HALO_MODES = [(c, p, t) for c, p in CP_MODES for t in (3, 1)]
EPS = 1e-8


def _L():
    from mlx_video_amd import _lib
    return _lib


_ZERO = []


def _zero_page(dev):
    if not _ZERO:
        _ZERO.append(torch.zeros(256, dtype=torch.uint8, device=dev))
    return _ZERO[0]


def _data(dev, vol, Cin, Cout, taps_d, seed):
    """randn activations, weights scaled by (taps*Cin)^-1/2, bias 0.1 randn, a randn residual; device-side generator."""
    g = torch.Generator(device=dev).manual_seed(seed)
    nt = 27 if taps_d == 3 else 9
    x = torch.randn((*vol, Cin), generator=g, device=dev).to(BF)
    w = (torch.randn((Cout, 3, 3, 3, Cin) if taps_d == 3 else (Cout, 3, 3, Cin), generator=g, device=dev) * (nt * Cin) ** -0.5).to(BF)
    b = (0.1 * torch.randn(Cout, generator=g, device=dev)).to(BF)
    r = torch.randn((*vol, Cout), generator=g, device=dev).to(BF)
    return x, w, b, r


def _launch(dev, x, w, b, causal, pad, taps_d=3, resid=None, ws=None, ws_bytes=0, act=None, keep_out=True):
    """One ltxk_conv3d_k3_bf16 call through the C ABI.  Returns (out or None, act_out or None, plan): outputs as
    (B,D,H,W,Cout) views of flat sentinel-tailed buffers (checked here), plan = ltxk_conv3d_plan of the same struct."""
    L = _L()
    lib = L.load()
    B, D, H, W, Cin = x.shape
    Cout = w.shape[0]
    M = B * D * H * W
    n = M * Cout
    out = _sent_bf16((n + SENT_ROWS * Cout,), dev) if keep_out else None
    act_out = _sent_bf16((n + SENT_ROWS * Cout,), dev) if act is not None else None
    a = L.Conv3dArgs()
    a.x, a.w, a.bias = x.data_ptr(), w.data_ptr(), b.data_ptr()
    a.out = out.data_ptr() if keep_out else None
    a.resid = resid.data_ptr() if resid is not None else None
    a.zero_page = _zero_page(dev).data_ptr()
    a.B, a.D, a.H, a.W, a.Cin, a.Cout = B, D, H, W, Cin, Cout
    a.causal, a.pad_mode, a.taps_d = causal, pad, taps_d
    if ws is not None:
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    if act is not None:
        a.act_out = act_out.data_ptr()
        a.act_scale = act["scale"].data_ptr() if act.get("scale") is not None else None
        a.act_shift = act["shift"].data_ptr() if act.get("shift") is not None else None
        a.act_eps, a.act_silu = EPS, int(act["silu"])
    pl = L.Conv3dPlan()
    L.check(lib.ltxk_conv3d_plan(ctypes.byref(a), ctypes.byref(pl)), "ltxk_conv3d_plan")
    L.check(lib.ltxk_conv3d_k3_bf16(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "ltxk_conv3d_k3_bf16")
    torch.cuda.synchronize()
    for buf in (out, act_out):
        assert buf is None or _untouched(buf[n:]), "rows past the last voxel were written"
    view = lambda t: None if t is None else t[:n].view(B, D, H, W, Cout)
    return view(out), view(act_out), pl


def _ratio(what, out, y, mag, K, resid, pl):
    """Worst d / bound of one output; on a miss the assertion names the element, its row and the plan."""
    assert not bool(torch.isnan(out).any()), f"{what}: output rows left unwritten ({_fmt(pl)})"
    d, bound = R.conv3d_bound(out, y, mag, K, resid)
    ratio = d / bound
    worst = float(ratio.max())
    if worst > 1.0:
        idx = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
        B, D, H, W, _ = out.shape
        row = ((idx[0] * D + idx[1]) * H + idx[2]) * W + idx[3]
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} outputs ({int((ratio > 1).any(-1).sum())} voxels) beyond the bound, worst "
                             f"d/bound {worst:.3g} at (b,d,h,w,c) = {idx}, row {row}: got {float(out[idx]):.6g}, exact {float(y[idx]):.6g}; {_fmt(pl)}")
    return worst


def _fmt(pl):
    return (f"plan kernel={pl.kernel} tile={pl.tile_rows}x{pl.tile_cols} tiles={pl.row_tiles}x{pl.col_tiles} slices={pl.slices}x{pl.ksteps} "
            f"tail={pl.tail_tile_rows}@{pl.tail_m_base}x{pl.tail_row_tiles} act={pl.fused_act}")


def _reaim(pl, cond, aim):
    assert cond, f"{_fmt(pl)} - re-aim this case at {aim}"


def _ref(x, w, b, causal, pad, taps_d, r):
    """(y, y + resid, mag) in float64 on the device."""
    y, mag = R.conv3d(x, w, b, causal, pad, taps_d)
    return y, y + r.to(F64), mag


# ------------------------------------------------------------------------------------------- per-tap 256x128, halo sweep
@pytest.mark.parametrize("Cout", [8, 128])
def test_halo_sweep_per_tap_256x128(dev, Cout):
    """Cin 64, no workspace, every mode x residual {off, on}.  (1,1,2,2): D = 1 (both temporal halos of causal = 0 are the
    one frame) and H = W = 2 (the reflected sample is the opposite edge); (2,1,2,3), (2,2,3,5): batch boundaries a few rows
    apart; (1,3,7,9); (2,3,7,9) = 378 rows: two row tiles, the second ragged, the batch boundary inside the first."""
    L = _L()
    Cin = 64
    for vol in [(1, 1, 2, 2), (2, 1, 2, 3), (2, 2, 3, 5), (1, 3, 7, 9), (2, 3, 7, 9)]:
        M = vol[0] * vol[1] * vol[2] * vol[3]
        worst = 0.0
        for causal, pad, taps_d in HALO_MODES:
            x, w, b, r = _data(dev, vol, Cin, Cout, taps_d, 1000 + M + 13 * causal + 7 * pad + taps_d)
            y, yr, mag = _ref(x, w, b, causal, pad, taps_d, r)
            for res in (None, r):
                out, _, pl = _launch(dev, x, w, b, causal, pad, taps_d, resid=res)
                _reaim(pl, pl.kernel == L.CONV_KERNEL_PER_TAP and (pl.tile_rows, pl.tile_cols) == (256, 128) and pl.slices == 1
                       and pl.row_tiles == (M + 255) // 256 and pl.col_tiles == 1 and not pl.tail_row_tiles and not pl.fused_act
                       and pl.ksteps == (27 if taps_d == 3 else 9), "the single-pass per-tap 256x128 tile")
                what = f"{vol} Cout={Cout} causal={causal} pad={pad} taps_d={taps_d} resid={res is not None}"
                worst = max(worst, _ratio(what, out, y if res is None else yr, mag, (27 if taps_d == 3 else 9) * Cin, res, pl))
        parity.auto(worst, 1.0, tag="x".join(map(str, vol)))


# ------------------------------------------------------------------------------------------- per-tap 160x256
@pytest.mark.parametrize("Cout", [256, 264])
def test_per_tap_160x256_tile(dev, Cout):
    """Cin 128, (2,2,5,9) = 180 rows: two row tiles, the second 20 rows; Cout 264: two column tiles, the second 8 columns
    wide.  Every mode, the residual on for half of them."""
    L = _L()
    Cin, vol, M = 128, (2, 2, 5, 9), 180
    worst = 0.0
    for i, (causal, pad, taps_d) in enumerate(HALO_MODES):
        x, w, b, r = _data(dev, vol, Cin, Cout, taps_d, 2000 + Cout + i)
        y, yr, mag = _ref(x, w, b, causal, pad, taps_d, r)
        res = r if (i + causal) % 2 else None
        out, _, pl = _launch(dev, x, w, b, causal, pad, taps_d, resid=res)
        _reaim(pl, pl.kernel == L.CONV_KERNEL_PER_TAP and (pl.tile_rows, pl.tile_cols, pl.row_tiles, pl.col_tiles) == (160, 256, 2, (Cout + 255) // 256)
               and pl.slices == 1 and not pl.tail_row_tiles, "the single-pass per-tap 160x256 tile")
        what = f"Cout={Cout} causal={causal} pad={pad} taps_d={taps_d} resid={res is not None}"
        worst = max(worst, _ratio(what, out, y if res is None else yr, mag, (27 if taps_d == 3 else 9) * Cin, res, pl))
    parity.auto(worst, 1.0, tag="ratio")


# ------------------------------------------------------------------------------------------- split-K
WS_FLOATS = 2 << 20            # 8 MB of scratch on offer; a case uses slices * M * Cout floats of it


@pytest.mark.parametrize("Cin,Cout,taps_d", [(128, 128, 3), (128, 264, 3), (192, 128, 3), (192, 264, 3), (256, 128, 1), (256, 264, 1)])
def test_split_k_against_float64(dev, Cin, Cout, taps_d):
    """A workspace on offer and few tiles: K slices park fp32 slabs, the finalize kernel sums them and applies bias and
    residual.  Cin 128: 54 K-steps in 3 slices of 18; Cin 192: 81 in 5 of 17, the last one 13 short; taps_d = 1 at Cin 256:
    36 in 2.  Volumes (1,2,4,4) = 32 rows (one ragged tile) and (2,3,7,9) = 378; every temporal x spatial halo mode, the
    residual on for half.  Two runs give the same bits; nothing past slices * M * Cout floats of the scratch is written."""
    L = _L()
    nk = (27 if taps_d == 3 else 9) * Cin // 64
    want = {54: (3, 18), 81: (5, 17), 36: (2, 18)}[nk]
    for vol in [(1, 2, 4, 4), (2, 3, 7, 9)]:
        M = vol[0] * vol[1] * vol[2] * vol[3]
        worst = 0.0
        for i, (causal, pad) in enumerate(CP_MODES):
            x, w, b, r = _data(dev, vol, Cin, Cout, taps_d, 3000 + Cin + Cout + M + i)
            y, yr, mag = _ref(x, w, b, causal, pad, taps_d, r)
            res = r if i % 2 else None
            ws = _sent_f32((WS_FLOATS,), dev)
            out, _, pl = _launch(dev, x, w, b, causal, pad, taps_d, resid=res, ws=ws, ws_bytes=WS_FLOATS * 4)
            _reaim(pl, pl.kernel == L.CONV_KERNEL_PER_TAP and (pl.slices, pl.ksteps) == want and pl.tile_rows == (256 if Cout <= 128 else 160)
                   and (pl.slices - 1) * pl.ksteps < nk and (nk == 81) == (pl.slices * pl.ksteps > nk), "split-K" + (" with a short last slice" if nk == 81 else ""))
            used = pl.slices * M * Cout
            assert _untouched(ws[used:]) and not bool(torch.isnan(ws[:used]).any()), "the slabs are not the first slices*M*Cout floats of the scratch"
            what = f"{vol} Cin={Cin} Cout={Cout} causal={causal} pad={pad} taps_d={taps_d} resid={res is not None}"
            worst = max(worst, _ratio(what, out, y if res is None else yr, mag, (27 if taps_d == 3 else 9) * Cin, res, pl))
            ws2 = _sent_f32((WS_FLOATS,), dev)
            again, _, _ = _launch(dev, x, w, b, causal, pad, taps_d, resid=res, ws=ws2, ws_bytes=WS_FLOATS * 4)
            assert torch.equal(out, again), f"{what}: two runs differ"
        parity.auto(worst, 1.0, tag="x".join(map(str, vol)))


def test_split_k_control_one_slab(dev):
    """A workspace of exactly one slab cannot hold two slices: the plan says single pass, nothing is written to it, and the
    bits are those of the launch without a workspace."""
    Cin, Cout, vol, M = 128, 128, (2, 3, 7, 9), 378
    x, w, b, r = _data(dev, vol, Cin, Cout, 3, 3999)
    ws = _sent_f32((M * Cout + 64,), dev)
    for res in (None, r):
        one, _, pl = _launch(dev, x, w, b, 1, 1, resid=res, ws=ws, ws_bytes=M * Cout * 4)
        _reaim(pl, pl.slices == 1 and pl.ksteps == 54 and (pl.tile_rows, pl.row_tiles) == (256, 2), "single pass")
        assert _untouched(ws)
        none, _, pl0 = _launch(dev, x, w, b, 1, 1, resid=res)
        assert (pl0.slices, pl0.ksteps, pl0.tile_rows) == (1, 54, 256)
        assert torch.equal(one, none)
        big = _sent_f32((WS_FLOATS,), dev)
        _, _, pls = _launch(dev, x, w, b, 1, 1, resid=res, ws=big, ws_bytes=WS_FLOATS * 4)
        _reaim(pls, pls.slices == 3, "split-K (the control must differ from it in the workspace alone)")


# ------------------------------------------------------------------------------------------- kw-reuse kernel
# (B, D, H, W), Cin, Cout.  W = 300: the second 256-row tile starts mid-row; W = 257: the tile's first column drifts by one
# voxel per tile; W = 64 / 65: a tile touches 4 + 1 image rows (RUNMAX); B = 2 with D*H*W no multiple of 256: a batch boundary
# inside a tile.
KW_CASES = [((1, 1, 2, 64), 64, 8), ((2, 1, 2, 65), 128, 48), ((2, 3, 3, 65), 64, 128), ((1, 3, 3, 131), 192, 128),
            ((2, 1, 3, 131), 64, 8), ((2, 3, 2, 257), 64, 128), ((1, 1, 3, 257), 192, 48), ((2, 1, 3, 300), 64, 48),
            ((1, 3, 2, 300), 128, 8), ((2, 3, 3, 300), 64, 128)]


@pytest.mark.parametrize("vol,Cin,Cout", KW_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kw_reuse_kernel_small_volumes(dev, vol, Cin, Cout):
    """No workspace, W >= 64, 27 taps, Cout <= 128: the kw-reuse kernel, at volumes of a few tiles.  Every temporal x
    spatial halo mode, the residual on for half."""
    L = _L()
    M = vol[0] * vol[1] * vol[2] * vol[3]
    if vol[0] == 2:
        assert (M // 2) % 256 != 0                                          # the batch boundary lies inside a tile
    worst = 0.0
    for i, (causal, pad) in enumerate(CP_MODES):
        x, w, b, r = _data(dev, vol, Cin, Cout, 3, 4000 + M + Cin + Cout + i)
        y, yr, mag = _ref(x, w, b, causal, pad, 3, r)
        res = r if (i + Cout // 8) % 2 else None
        out, _, pl = _launch(dev, x, w, b, causal, pad, 3, resid=res)
        _reaim(pl, pl.kernel == L.CONV_KERNEL_KW and (pl.tile_rows, pl.tile_cols, pl.row_tiles, pl.col_tiles) == (256, 128, (M + 255) // 256, 1)
               and pl.slices == 1 and pl.ksteps == 9 * Cin // 32 and not pl.tail_row_tiles, "the kw-reuse kernel")
        what = f"{vol} Cin={Cin} Cout={Cout} causal={causal} pad={pad} resid={res is not None}"
        worst = max(worst, _ratio(what, out, y if res is None else yr, mag, 27 * Cin, res, pl))
    parity.auto(worst, 1.0, tag="ratio")


# ------------------------------------------------------------------------------------------- tail launches
@pytest.mark.parametrize("form,vol,Cout,causal,pad,plan", [
    ("kw", (1, 2, 129, 257), 128, 0, 1, (1, 256, 256, 128, 65536, 7)),
    ("per_tap_256", (1, 3, 366, 60), 128, 1, 0, (0, 256, 256, 128, 65536, 3)),
    ("per_tap_160", (1, 2, 342, 60), 256, 1, 1, (0, 160, 256, 96, 40960, 1))], ids=["kw", "per_tap_256", "per_tap_160"])
def test_tail_launches(dev, form, vol, Cout, causal, pad, plan):
    """The rows past the last whole round of 256 workgroups run as a second launch of lower tiles from row m_base on.  The
    only large cases (66306, 65880 and 41040 rows, Cin 64): a tail that ignores m_base, or resolves its halo relative to its
    own first row, moves whole rows.  With and without residual."""
    Cin = 64
    M = vol[0] * vol[1] * vol[2] * vol[3]
    x, w, b, r = _data(dev, vol, Cin, Cout, 3, 5000 + M)
    y, yr, mag = _ref(x, w, b, causal, pad, 3, r)
    worst = 0.0
    for res in (None, r):
        out, _, pl = _launch(dev, x, w, b, causal, pad, 3, resid=res)
        _reaim(pl, (pl.kernel, pl.tile_rows, pl.row_tiles, pl.tail_tile_rows, pl.tail_m_base, pl.tail_row_tiles) == plan and pl.slices == 1
               and pl.tail_m_base < M <= pl.tail_m_base + pl.tail_row_tiles * pl.tail_tile_rows, f"the {form} tail launch {plan}")
        worst = max(worst, _ratio(f"{form} tail resid={res is not None}", out, y if res is None else yr, mag, 27 * Cin, res, pl))
    parity.auto(worst, 1.0, tag="ratio")


# ------------------------------------------------------------------------------------------- fused activation epilogue
@pytest.mark.parametrize("vol", [(2, 2, 5, 9), (2, 3, 7, 9)], ids=["2x2x5x9", "2x3x7x9"])
@pytest.mark.parametrize("Cout", [128, 256])
def test_fused_pixelnorm_act_epilogue(dev, Cout, vol):
    """act_out = silu?(modulate?(pixel_norm(out row))) from the tile that holds the whole row (Cout 128: 256x128, Cout 256:
    160x256), Cin 64, ragged volumes, another modulation row per batch; SiLU x modulation x residual, the halo mode
    rotating through all twelve.  The kept `out` meets the conv bound; act_out with out = NULL has the bits of act_out
    with out kept; act_out meets ltxk_pixelnorm_act's ulp rule (test_vae_glue_gpu.py) against ref64.pixelnorm_act of the
    kernel's OWN kept out, which isolates the epilogue from rounding flips of the convolution.  Every row counts towards
    max_frac here: a row whose statistic sits on a bf16 rounding boundary and flips whole is 1 / 180 or 1 / 378 of the
    elements, and the 1 % holds two or three of them."""
    L = _L()
    Cin = 64
    B, D, H, W = vol
    M = B * D * H * W
    g = torch.Generator(device=dev).manual_seed(6000 + Cout + M)
    scale = (0.5 * torch.randn(B, Cout, generator=g, device=dev)).to(BF)
    shift = torch.randn(B, Cout, generator=g, device=dev).to(BF)
    worst, worst_ulps, worst_frac, worst_amb = 0.0, 0.0, 0.0, 0.0
    combos = [(s, m, rs) for s in (False, True) for m in (False, True) for rs in (False, True)]
    for i, (silu_on, mod, res_on) in enumerate(combos):
        causal, pad, taps_d = HALO_MODES[(i + (Cout // 128) * 3 + M) % len(HALO_MODES)]
        x, w, b, r = _data(dev, vol, Cin, Cout, taps_d, 6100 + Cout + M + i)
        y, yr, mag = _ref(x, w, b, causal, pad, taps_d, r)
        res = r if res_on else None
        act = dict(silu=silu_on, scale=scale if mod else None, shift=shift if mod else None)
        out, act_kept, pl = _launch(dev, x, w, b, causal, pad, taps_d, resid=res, act=act)
        none, act_only, pl2 = _launch(dev, x, w, b, causal, pad, taps_d, resid=res, act=act, keep_out=False)
        for p in (pl, pl2):
            _reaim(p, p.fused_act and p.kernel == L.CONV_KERNEL_PER_TAP and p.slices == 1 and (p.tile_cols, p.col_tiles) == (Cout, 1)
                   and p.tile_rows == (256 if Cout == 128 else 160) and not p.tail_row_tiles, "the fused activation epilogue")
        what = f"{vol} Cout={Cout} causal={causal} pad={pad} taps_d={taps_d} silu={silu_on} mod={mod} resid={res_on}"
        assert none is None and torch.equal(act_kept, act_only), f"{what}: act_out differs between out kept and out = NULL"
        worst = max(worst, _ratio(what, out, y if res is None else yr, mag, (27 if taps_d == 3 else 9) * Cin, res, pl))
        ref, amag, _ = R.pixelnorm_act(out.reshape(M, Cout).cpu(), R.f32(EPS), scale.cpu() if mod else None,
                                       shift.cpu() if mod else None, D * H * W, silu_on)
        ulps, frac = R.assert_bf16_close(act_kept.reshape(M, Cout).cpu(), ref, max_ulps=2 if mod else 1, max_frac=1e-2,
                                         mag=amag, what=what)
        worst_ulps, worst_frac = max(worst_ulps, ulps), max(worst_frac, frac)
        # every element inside its admissible bf16 interval (ref_rows.py), the row statistic reduced at the epilogue's own depth
        iv = RR.pixelnorm_act(out.reshape(M, Cout).cpu(), R.f32(EPS), scale.cpu() if mod else None, shift.cpu() if mod else None,
                              D * H * W, silu_on, depth=RR.fused_pixelnorm_depth(Cout))
        (n_out, first), amb, widest = RR.within(act_kept.reshape(M, Cout).cpu(), iv)
        assert n_out == 0, f"{what}: {n_out} elements of act_out outside their admissible bf16 interval, the first at {first} (widest {widest} steps)"
        worst_amb = max(worst_amb, amb)
    parity.auto(worst, 1.0, tag="ratio")
    parity.auto(worst_ulps, 2.0, tag="act_ulps")
    parity.auto(worst_frac, 1e-2, tag="act_frac")
    # the rows come from the device's own convolution, so this share cannot be asserted on the CPU beforehand; the cap is the
    # one ltxk_pixelnorm_act's own cases meet there (worst 1.52 %, with SiLU: E_ACT = 2^-15 on either side of a value against
    # a bf16 spacing of 2^-8 .. 2^-7 is ~1.1 % by itself).  A row whose statistic sits on a bf16 rounding boundary has two
    # admissible values throughout and is 1 / 180 or 1 / 378 of the elements; the statistic's interval is ~2^-19 wide
    parity.auto(worst_amb, RR.AMBIGUOUS_CAP, tag="ambiguous")
