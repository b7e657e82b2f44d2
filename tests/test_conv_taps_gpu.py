"""ltxk_conv_taps_bf16 through the C ABI at the smallest shapes that can go wrong, element by element against float64.

With c = sum x*w + bias and mag = sum |x*w| in float64 (ref_audio.conv_taps: explicit zero halo, one matmul per tap, on the
device) and K = kh*kw*Cin, the plain and residual forms meet the bound of tests/test_conv3d_bound_gpu.py,

    acc = K 2^-24 mag + 2^-24 (|c| + K 2^-24 mag),     |out - c| <= acc + 1/2 ulp_bf16(|c| + acc),

and each further rounding of the epilogue (include/ltxk.h, steps 2-5) extends it by half a bf16 ulp of that intermediate, each
fp32 operation by 2^-24 of its result (ref_audio.taps_bound has the chain):

    resid:  e2 = e1 + 2^-24 (|c| + |r| + e1) + 1/2 ulp_bf16(|c + r| + e1 + ...)
    mean:   e3 = (e2 + 2^-24 (partial sums)) / n + 2^-24 |v| + 1/2 ulp_bf16(|v| + ...),   v = (c + r + a1 [+ a2]) / n
    leaky:  e_act = max(e, slope e + 2^-24 slope |v| + 1/2 ulp_bf16(slope (|v| + e)))

The bound holds for any summation order: single pass and K slices alike.  One wrong tap, a tap read across a frame boundary or
a dilation off by one moves an output by about 1/sqrt(taps) of its size - hundreds of times the bound (tests/test_audio_cpu.py
shows all three rejected on the host).  The tanh form is the exception: the device tanhf's error is not derivable here, so its
figure (ref_audio.tanh_excess_ulps: fp32 ulps beyond what the accumulation explains) is pinned in tests/golden/audio_pins.json at
twice the value measured on MI355X, as parity_pins.json does.

Every case first asserts the launch form it aims at (ltxk_conv_taps_plan on the struct it launches), writes into flat buffers
whose rows past the last one hold NaN sentinels that must survive, and prints its worst d / bound before it asserts.
Split-K and its single-pass twin walk K in different orders, so their bits may differ in the last place; both are held to the
bound, and each is bit-equal to itself run twice."""
import ctypes
import json
import os

import pytest
import torch

import ref_audio as A
from test_rowops_gpu import _sent_bf16, _sent_f32, _untouched

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64
SENT_ROWS = 3
PINS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_pins.json")))["pins"]


def _L():
    from mlx_video_amd import _lib
    return _lib


_BUF = {}


def _zero_page(dev):
    if "z" not in _BUF:
        _BUF["z"] = torch.zeros(256, dtype=torch.uint8, device=dev)
        _BUF["ws"] = torch.empty(8 << 20, dtype=torch.float32, device=dev)
    return _BUF["z"]


def _data(dev, vol, Cin, Cout, kh, kw, seed, extras=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((*vol, Cin), generator=g, device=dev).to(BF)
    w = (torch.randn((Cout, kh, kw, Cin), generator=g, device=dev) * (kh * kw * Cin) ** -0.5).to(BF)
    b = (0.1 * torch.randn(Cout, generator=g, device=dev)).to(BF)
    ex = [torch.randn((*vol, Cout), generator=g, device=dev).to(BF) for _ in range(extras)]
    return x, w, b, ex


def _launch(dev, x, w, b, dil, pad, resid=None, mean_with=(), slope=None, keep_out=True, tanh=False, split=True):
    """One ltxk_conv_taps_bf16 call.  Returns (out, act_out, out_f32, plan), outputs as (B,D,H,W,Cout) views of sentinel-tailed
    flat buffers (checked here)."""
    L = _L()
    lib = L.load()
    B, D, H, W, Cin = x.shape
    Cout, kh, kw, _ = w.shape
    n = B * D * H * W * Cout
    tail = SENT_ROWS * max(Cout, 8)
    out = _sent_bf16((n + tail,), dev) if keep_out and not tanh else None
    act = _sent_bf16((n + tail,), dev) if slope is not None else None
    o32 = _sent_f32((n + tail,), dev) if tanh else None
    a = L.ConvTapsArgs()
    a.struct_bytes = ctypes.sizeof(L.ConvTapsArgs)
    a.B, a.D, a.H, a.W, a.Cin, a.Cout = B, D, H, W, Cin, Cout
    a.kh, a.kw, a.dil_h = kh, kw, dil
    a.pad_top, a.pad_bottom, a.pad_left, a.pad_right = pad
    a.x, a.w, a.bias, a.zero_page = x.data_ptr(), w.data_ptr(), b.data_ptr(), _zero_page(dev).data_ptr()
    a.resid = resid.data_ptr() if resid is not None else None
    a.n_mean = len(mean_with) + 1 if mean_with else 0
    a.mean_a1 = mean_with[0].data_ptr() if len(mean_with) > 0 else None
    a.mean_a2 = mean_with[1].data_ptr() if len(mean_with) > 1 else None
    a.out = out.data_ptr() if out is not None else None
    a.act_out = act.data_ptr() if act is not None else None
    a.out_f32 = o32.data_ptr() if o32 is not None else None
    a.slope = slope if slope is not None else 0.0
    if split:
        a.workspace, a.workspace_bytes = _BUF["ws"].data_ptr(), _BUF["ws"].numel() * 4
    pl = L.Conv3dPlan()
    L.check(lib.ltxk_conv_taps_plan(ctypes.byref(a), ctypes.byref(pl)), "ltxk_conv_taps_plan")
    assert pl.kernel == L.CONV_KERNEL_TAPS and pl.tile_rows == 256 and pl.tile_cols == (128 if Cout > 64 else 64)
    assert pl.row_tiles == -(-B * D * H * W // 256) and pl.col_tiles == -(-Cout // pl.tile_cols)
    assert pl.tail_row_tiles == 0 and pl.fused_act == 0
    assert pl.slices * pl.ksteps >= -(-kh * kw * Cin // 64) > (pl.slices - 1) * pl.ksteps
    L.check(lib.ltxk_conv_taps_bf16(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "ltxk_conv_taps_bf16")
    torch.cuda.synchronize()
    for buf in (out, act, o32):
        assert buf is None or _untouched(buf[n:]), "rows past the last one were written"
    view = lambda t: None if t is None else t[:n].view(B, D, H, W, Cout)
    return view(out), view(act), view(o32), pl


def _hold(what, got, exact, bound, pl):
    assert not bool(torch.isnan(got).any()), f"{what}: output left unwritten"
    ratio = (got.to(F64) - exact).abs() / bound
    worst = float(ratio.max())
    print(f"[conv_taps] {what}: worst d/bound {worst:.3f} (slices {pl.slices} x {pl.ksteps} K-steps, tiles {pl.row_tiles}x{pl.col_tiles})")
    if worst > 1.0:
        idx = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} outputs beyond the bound, worst d/bound {worst:.3g} at (b,d,h,w,c) = {idx}: "
                             f"got {float(got[idx]):.6g}, exact {float(exact[idx]):.6g}")
    return worst


def _case(dev, what, vol, Cin, Cout, kh, kw, dil, pad, seed, resid=False, nmean=0, slope=None, keep_out=True, split=True, want_split=None):
    x, w, b, ex = _data(dev, vol, Cin, Cout, kh, kw, seed, extras=3)
    r = ex[0] if resid else None
    mw = tuple(ex[1:nmean]) if nmean else ()
    c, mag = A.conv_taps(x, w, b, dil, pad)
    y, act = A.taps_exact(c, r, mw, slope)
    e, e_act = A.taps_bound(c, mag, kh * kw * Cin, r, mw, slope)
    out, aout, _, pl = _launch(dev, x, w, b, dil, pad, r, mw, slope, keep_out, split=split)
    if want_split is not None:
        assert (pl.slices >= 2) == want_split, f"{what}: slices = {pl.slices} - re-aim this case"
    if keep_out:
        _hold(what, out, y, e, pl)
    if slope is not None:
        _hold(what + " act_out", aout, act, e_act, pl)
    return out, aout, pl


def _pad1d(k, dil):
    half = (k - 1) * dil // 2
    return (half, (k - 1) * dil - half, 0, 0)


@pytest.mark.parametrize("k,dil", [(3, 1), (7, 3), (11, 5)])
def test_conv1d_dilated_64(dev, k, dil):
    """Cin = Cout = 64, B = 2; T = 1 and 7 are shorter than the +-25 reach of (11, 5), 33 straddles it, 300 passes one tile
    seam (600 rows: the batch boundary lies inside the second tile).  Residual on and off."""
    for T in (1, 7, 33, 300):
        for res in (False, True):
            _case(dev, f"conv1d k{k} d{dil} T{T} res{int(res)}", (2, 1, T, 1), 64, 64, k, 1, dil, _pad1d(k, dil), 100 * k + T + res, resid=res)


@pytest.mark.parametrize("k,dil", [(3, 1), (7, 3), (4, 1)])
def test_conv1d_cin32(dev, k, dil):
    """Cin = Cout = 32: a K-step is two taps; k = 3 and 7 end in half a step (zero page on both operand sides), k = 4 - uneven
    halo (1, 2) - in a whole one.  Leaky output beside the plain one."""
    half = (k - 1) * dil // 2
    for T in (1, 7, 33, 300):
        _case(dev, f"conv1d Cin32 k{k} d{dil} T{T}", (2, 1, T, 1), 32, 32, k, 1, dil, (half, (k - 1) * dil - half, 0, 0), 7 * k + T,
              resid=True, slope=0.1)


def test_conv_post_tanh(dev):
    """Cout = 2 with the tanh form, Cin = 32, k = 7: fp32 out, only the valid columns stored."""
    worst = 0.0
    for T in (1, 7, 33, 300):
        x, w, b, _ = _data(dev, (2, 1, T, 1), 32, 2, 7, 1, 900 + T)
        c, mag = A.conv_taps(x, w, b, 1, _pad1d(7, 1))
        _, _, o32, pl = _launch(dev, x, w, b, 1, _pad1d(7, 1), tanh=True)
        assert not bool(torch.isnan(o32).any()) and float(o32.abs().max()) <= 1.0
        worst = max(worst, float(A.tanh_excess_ulps(o32, c, mag, 7 * 32)))
    print(f"[conv_taps] tanh form: {worst:.4f} fp32 ulps beyond the accumulation bound (pin {PINS['conv_taps_tanh_excess_ulps']})")
    assert worst <= PINS["conv_taps_tanh_excess_ulps"]


def test_cout2_bf16_and_odd_cout(dev):
    """Cout = 2 and 6 (element stores clipped to Cout; 6 is no multiple of 4) and 20 (a multiple of 4, not of 8) in bf16,
    every operand of the epilogue present."""
    for Cout in (2, 6, 20):
        _case(dev, f"Cout{Cout}", (2, 1, 33, 1), 64, Cout, 3, 1, 1, _pad1d(3, 1), 40 + Cout, resid=True, nmean=3, slope=0.1)


def test_polyphase_panel(dev):
    """The first ConvTranspose1d's packed panel: 6 x 512 columns, Cin = 1024, 3 taps (halo 1 + 1), T = 5, B = 2: 24 column
    tiles on 10 rows, split-K with the scratch on offer and single-pass without."""
    _case(dev, "panel split", (2, 1, 5, 1), 1024, 3072, 3, 1, 1, (1, 1, 0, 0), 5, slope=0.1, want_split=True)
    _case(dev, "panel single", (2, 1, 5, 1), 1024, 3072, 3, 1, 1, (1, 1, 0, 0), 5, slope=0.1, split=False, want_split=False)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 16), (5, 64), (40, 5)])
def test_causal_3x3(dev, H, W):
    """The audio decoder's causal 3x3 (halo 2 above, none below, 1 left and right), 64 -> 128, B = 2.  (40, 5): W does not
    divide the tile, image rows straddle tiles and the batch boundary (row 200) lies inside the first."""
    for res in (False, True):
        _case(dev, f"causal3x3 {H}x{W} res{int(res)}", (2, 1, H, W), 64, 128, 3, 3, 1, (2, 0, 1, 1), 13 * H + W + res, resid=res)
    _case(dev, f"causal3x3 {H}x{W} D2", (1, 2, H, W), 64, 128, 3, 3, 1, (2, 0, 1, 1), 17 * H + W)      # frames of one batch row


@pytest.mark.parametrize("form", ["resid", "mean2", "mean3", "leaky", "leaky_only", "all"])
def test_epilogue_forms(dev, form):
    kw = {"resid": dict(resid=True), "mean2": dict(nmean=2), "mean3": dict(nmean=3), "leaky": dict(slope=0.1),
          "leaky_only": dict(slope=0.01, keep_out=False), "all": dict(resid=True, nmean=3, slope=0.1)}[form]
    for Cout in (64, 128):
        _case(dev, f"{form} Cout{Cout}", (2, 1, 33, 1), 64, Cout, 7, 1, 3, _pad1d(7, 3), 77 + Cout, **kw)


def test_split_k_and_its_single_pass_twin(dev):
    """Cin = 256, k = 7, dil 3: 28 K-steps on one row tile -> 3 slices with the scratch, one pass without; every epilogue
    operand; Cout = 128 and the clipped Cout = 6 (slab rows of 8 floats)."""
    for Cout in (128, 6):
        kw = dict(resid=True, nmean=3, slope=0.1)
        o1, a1, p1 = _case(dev, f"split Cout{Cout}", (2, 1, 33, 1), 256, Cout, 7, 1, 3, _pad1d(7, 3), 3, want_split=True, **kw)
        o2, a2, p2 = _case(dev, f"single Cout{Cout}", (2, 1, 33, 1), 256, Cout, 7, 1, 3, _pad1d(7, 3), 3, split=False, want_split=False, **kw)
        assert p1.slices == 3 and p1.ksteps == 10 and p2.ksteps == 28
    x, w, b, _ = _data(dev, (2, 1, 33, 1), 256, 2, 7, 1, 8)
    c, mag = A.conv_taps(x, w, b, 3, _pad1d(7, 3))
    _, _, o32, pl = _launch(dev, x, w, b, 3, _pad1d(7, 3), tanh=True)
    assert pl.slices == 3
    assert float(A.tanh_excess_ulps(o32, c, mag, 7 * 256)) <= PINS["conv_taps_tanh_excess_ulps"]


def test_two_runs_bit_equal(dev):
    for split in (True, False):
        runs = [_case(dev, f"rerun split{int(split)}", (2, 1, 33, 1), 256, 128, 7, 1, 3, _pad1d(7, 3), 21, resid=True, nmean=3, slope=0.1, split=split)
                for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_refusals(dev):
    """The library refuses what the header rules out (nothing is launched)."""
    L = _L()
    x, w, b, _ = _data(dev, (1, 1, 4, 1), 64, 64, 3, 1, 1)
    with pytest.raises(L.LtxkError, match="pad_top"):
        _launch(dev, x, w, b, 1, (1, 0, 0, 0))
    with pytest.raises(L.LtxkError, match="dil_h"):
        _launch(dev, x, w, b, 9, (9, 9, 0, 0))
    a = L.ConvTapsArgs()
    assert L.load().ltxk_conv_taps_bf16(ctypes.byref(a), None) != 0 and b"struct_bytes" in L.load().ltxk_last_error()
