"""ltxk_flash_attn in every launch form, held element by element to a float64 bound (ref64.attention / attention_bound;
tests/test_ref64_cpu.py shows on the CPU that the bound accepts the oracle's two policies and an fp32 emulation of the kernel's
loop, and rejects a dropped key, an unmasked pad slot, a misplaced row, a skipped key block and exchanged merge weights):

    e1    = 2^-22 + ln2 * dx * 1.001 + Tk * 2^-24
    bound = 1/2 ulp_bf16(out) + ((2^-8 + e1) A + e1 |y|) / (1 - e1) + 2^-22 |y| + 2^-120

with y = P v and A = P |v| exact and dx the worst error of a key's exponent.  Nothing in it is a measured tolerance and it
holds for any tiling, deferral history, key split and summation order, so every form below meets the same bound.

What the norm-based attention tests cannot see, each case here launches: V^T whose pad columns [Tk, ldvt) hold +-1024 (one
unmasked slot of the ragged last tile moves every row by ~1024/Tk of a value), strided q / k / V^T / out views as the model
passes them, an output view inside NaN sentinels, Tk below one key tile, one key into the second, and a key half of the tail
pair that sees masked keys only.  Every case asserts its plan first (ops.flash_attn_plan at 256 CUs, the function the launch
decides by; tests/test_attn_plan_cpu.py asserts the same table without a device), launches twice and requires identical bits,
and records its worst d / bound in the parity ledger with stated bound 1.0.  Two more scales run the shapes whose second key
half is all masked: there the merge of the tail pair once made NaN of inf * 0 (attention.hip, fa_body)."""
import math

import parity
import pytest
import torch

import ref64 as R
from test_rowops_gpu import _sent_bf16, _untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
K128, MIX = 0, 1
SCALE = 1.0 / math.sqrt(128)
ALL = R.ATTN_FAMILIES


def _split(split_tiles, whole=0):
    return dict(kernel=K128, whole_workgroups=whole, split_tiles=split_tiles, workgroups=whole + 2 * split_tiles)


def _whole(n):
    return dict(kernel=K128, whole_workgroups=n, split_tiles=0, workgroups=n)


# id, (B, H, Tq, Tk), families, [(tail_split, expected plan fields)].  128-row tiles per launch = B * H * ceil(Tq / 128); 512 slots.
CASES = [
    # every tile key-split (the short round is the only round), and the same shapes as whole workgroups.  Tk below one key tile
    # (1, 5, 33: at 1 and 5 the second key half of the pair sees masked keys only), exactly one (64), one key into the second
    # (65: the ragged tile's first half holds the one live key), ragged in the second (70, 97), two whole (128), one into the
    # third (129); Tq ragged inside a 16-row block (77, 129, 130, 100, 200) and across tiles.  B*H here is never a multiple of
    # 8: these are the plain tile order, the larger grids below and the fused cases the XCD-aware one.
    ("tk1", (1, 1, 1, 1), ALL, [(True, _split(1)), (False, _whole(1))]),
    ("tk5", (1, 2, 77, 5), ALL, [(True, _split(2)), (False, _whole(2))]),
    ("tk33", (1, 4, 200, 33), ALL, [(True, _split(8)), (False, _whole(8))]),
    ("tk70", (1, 3, 200, 70), ALL, [(True, _split(6)), (False, _whole(6))]),
    ("tk65", (2, 3, 129, 65), ALL, [(True, _split(12)), (False, _whole(12))]),
    ("tk64", (1, 4, 130, 64), ALL, [(True, _split(8)), (False, _whole(8))]),
    ("tk97_tq16", (1, 2, 16, 97), ALL, [(True, _split(2)), (False, _whole(2))]),
    ("tk128", (1, 2, 100, 128), ALL, [(True, _split(2)), (False, _whole(2))]),
    ("tk129", (1, 2, 100, 129), ALL, [(True, _split(2)), (False, _whole(2))]),
    # fill rule: 320 tiles for 512 slots = 128 whole + 192 split; with the flag 320 whole (no_split_by_flag)
    ("fill_rule", (10, 32, 100, 97), ALL, [(True, _split(192, 128)), (False, _whole(320))]),
    # whole rounds plus tail: 640 tiles = 512 whole + 128 split; with the flag 640 whole
    ("whole_rounds_plus_tail", (20, 32, 100, 97), ALL, [(True, _split(128, 512)), (False, _whole(640))]),
    # mixed grid, 192-row tiles only.  (10,32,200,97) is a mixed-grid launch of two 128-row tiles per head and no 192-row one
    # (kept: the mixed kernel's 128-row body alone); the nearest shape with 192-row tiles only is Tq = 190, whose last wave
    # ends inside a 16-row block.
    ("mix_128_only", (10, 32, 200, 97), ALL, [(True, dict(kernel=MIX, tiles_192=0, tiles_128=2, split_tiles=0, workgroups=640))]),
    ("mix_192_only", (10, 32, 190, 97), ALL, [(True, dict(kernel=MIX, tiles_192=1, tiles_128=0, split_tiles=0, workgroups=320))]),
    ("mix_192_only_ragged", (2, 32, 1296, 136), ("flat", "spiked"),
     [(True, dict(kernel=MIX, tiles_192=7, tiles_128=0, split_tiles=0, workgroups=448))]),
    # mixed grid with both tile sizes, the smallest the planner gives at 256 CUs: 192 + 128 + 65 rows, the last 128-row tile
    # ends one row into a 16-row block
    ("mix_both", (5, 32, 385, 72), ALL, [(True, dict(kernel=MIX, tiles_192=1, tiles_128=2, split_tiles=0, workgroups=480))]),
]

# A/B build switches: switch, value, (B, H, Tq, Tk), plan fields the switch must produce.  LTXK_FA_MFMA=32 and LTXK_FA_QB=3 bite
# at the two small shapes; the others only where the default plan has what they change - the smallest such shape each:
# LTXK_FA_QB=2 at the first mixed-grid launch (640 tiles), LTXK_FA_XCD=0 at B*H = 8, LTXK_FA_FILL=0 at the fill-rule shape.
AB_CASES = [
    ("LTXK_FA_MFMA", "32", (1, 4, 200, 33), dict(mfma_k=32, **_split(8))),
    ("LTXK_FA_MFMA", "32", (2, 3, 129, 65), dict(mfma_k=32, **_split(12))),
    ("LTXK_FA_QB", "3", (1, 4, 200, 33), dict(kernel=MIX, tiles_192=2, tiles_128=0, workgroups=8)),
    ("LTXK_FA_QB", "3", (2, 3, 129, 65), dict(kernel=MIX, tiles_192=1, tiles_128=0, workgroups=6)),
    ("LTXK_FA_QB", "2", (10, 32, 129, 97), dict(mfma_k=16, **_split(128, 512))),
    ("LTXK_FA_XCD", "0", (1, 8, 200, 33), dict(xcd_order=0, **_split(16))),
    ("LTXK_FA_XCD", "0", (2, 4, 129, 65), dict(xcd_order=0, **_split(16))),
    ("LTXK_FA_FILL", "0", (10, 32, 100, 97), _whole(320)),
]
AB_DEFAULT = {(10, 32, 129, 97): dict(kernel=MIX, tiles_192=1, tiles_128=0), (1, 8, 200, 33): dict(xcd_order=1), (2, 4, 129, 65): dict(xcd_order=1)}

# fused query preparation (H % 4 == 0), one shape per form: id, shape, tail_split, plan
FUSED_CASES = [
    ("split_all_xcd", (2, 4, 129, 65), True, dict(xcd_order=1, **_split(16))),
    ("split_all", (1, 4, 200, 33), True, dict(xcd_order=0, **_split(8))),
    ("whole_workgroups", (1, 4, 200, 33), False, _whole(8)),
    ("fill_rule", (10, 32, 100, 97), True, _split(192, 128)),
    ("whole_rounds_plus_tail", (20, 32, 100, 97), True, _split(128, 512)),
    ("mix_192_only", (10, 32, 190, 97), True, dict(kernel=MIX, tiles_192=1, tiles_128=0, workgroups=320)),
    ("mix_both", (5, 32, 385, 72), True, dict(kernel=MIX, tiles_192=1, tiles_128=2, workgroups=480)),
]

ALL_SHAPES = sorted({c[1] for c in CASES} | {c[2] for c in AB_CASES} | {c[1] for c in FUSED_CASES})


def _need_256(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if cus != 256:
        pytest.skip(f"the expected plans are those of a 256-CU device; this one has {cus}")


def _plan(shape, tail_split, want, fused_q=False):
    from mlx_video_amd import ops
    pl = ops.flash_attn_plan(*shape, cus=256, tail_split=tail_split, fused_q=fused_q)
    assert {k: getattr(pl, k) for k in want} == want, (shape, tail_split, pl)
    return pl


def _launch(dev, q, k, v, H, tail_split, scale=SCALE, **fused):
    """One ops.flash_attn call on strided views: q with ldq = D + 8, k the left half of a (B*Tk, 2D) buffer (the right half
    NaN), V^T with ldvt = roundup64(Tk) + 8 and pad columns alternating +-1024, out the [1 : 1 + B*Tq, :D] view of a
    (B*Tq + 3, D + 64) buffer of NaN sentinels, which must survive outside the view.  q, k, v: (B,T,D) on the device."""
    from mlx_video_amd import ops
    B, Tq, D = q.shape
    Tk = k.shape[1]
    qb = _sent_bf16((B * Tq, D + 8), dev)
    qb[:, :D] = q.reshape(B * Tq, D)
    kb = _sent_bf16((B * Tk, 2 * D), dev)
    kb[:, :D] = k.reshape(B * Tk, D)
    ldvt = (Tk + 63) // 64 * 64 + 8
    vt = torch.empty((B, D, ldvt), dtype=BF, device=dev)
    vt[:, :, Tk:] = (1024.0 * (1 - 2 * (torch.arange(ldvt - Tk, device=dev) % 2))).to(BF)
    vt[:, :, :Tk] = v.transpose(1, 2)
    ob = _sent_bf16((B * Tq + 3, D + 64), dev)
    out = ob[1:1 + B * Tq, :D]
    ops.flash_attn(qb[:, :D], kb[:, :D], vt, out, B, H, Tq, Tk, scale, tail_split=tail_split, **fused)
    torch.cuda.synchronize()
    assert _untouched(ob[0]) and _untouched(ob[1 + B * Tq:]) and _untouched(ob[:, D:]), "wrote outside the output view"
    return out.reshape(B, Tq, D)


def _ratio(what, out, ref, Tk, H, pl):
    """d / bound of one output; on a miss the assertion names the element, the rows affected and the plan."""
    assert not bool(torch.isnan(out).any()), f"{what}: NaN inside the output view (rows left unwritten, or 0/0); {pl}"
    d, bound = R.attention_bound(out, *ref, Tk)
    ratio = d / bound
    worst = float(ratio.max())
    print(f"{what}: worst d/bound {worst:.4f}")
    if worst > 1.0:
        b, row, ch = (int(i) for i in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} elements in {int((ratio > 1).any(-1).sum())} of {ratio.shape[0] * ratio.shape[1]} "
                             f"rows beyond the bound, worst d/bound {worst:.4g} at (b, row, head, channel) = ({b}, {row}, {ch // 128}, {ch % 128}): "
                             f"got {float(out[b, row, ch]):.8g}, exact {float(ref[0][b, row, ch]):.8g}; {pl}")
    return ratio


def _planted_hold_mass(q, k, H, planted):
    p = R.attention_probs(q, k, H, SCALE)[0]
    assert planted and all(float(p[:, :, r, j].min()) >= 0.25 for r, j in planted), "a planted key holds less than 0.25 of its row"


@pytest.mark.parametrize("name,shape,variants,family", [(c[0], c[1], c[3], f) for c in CASES for f in c[2]],
                         ids=[f"{c[0]}-{f}" for c in CASES for f in c[2]])
def test_attention_within_float64_bound(dev, name, shape, variants, family):
    _need_256(dev)
    B, H, Tq, Tk = shape
    plans = [_plan(shape, ts, want) for ts, want in variants]
    q, k, v, planted = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in R.attention_inputs(B, H, Tq, Tk, family, 0))
    if family == "spiked":
        _planted_hold_mass(q, k, H, planted)
    ref = R.attention(q, k, v, H, SCALE)
    for (ts, _), pl in zip(variants, plans):
        tag = "split" if ts else "no_split"
        out = _launch(dev, q, k, v, H, ts)
        ratio = _ratio(f"{name} {shape} {family} {tag}", out, ref, Tk, H, pl)
        parity.auto(float(ratio.max()), 1.0, tag=f"{tag}_d_over_bound")
        assert torch.equal(_launch(dev, q, k, v, H, ts).view(torch.int16), out.view(torch.int16)), f"{name} {tag}: two launches differ"


@pytest.mark.parametrize("scale", [0.1, 0.09])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 77, 5), (1, 4, 200, 32), (2, 3, 129, 65)], ids=lambda s: "x".join(map(str, s)))
def test_attention_other_scales_within_float64_bound(dev, shape, scale):
    """The scale is the caller's.  At Tk <= 32 the second key half of a split tile sees masked keys only, and its
    P = exp2(fma(-1e30, c, -ceil(-1e30 c))) is exp2 of the fma's rounding residual: 0 at 1/sqrt(128) and 0.09, +inf at 0.1, where
    a merge of that half is inf * 0 (tests/test_ref64_cpu.py).  The kernel leaves a half without a live key out of the merge."""
    _need_256(dev)
    B, H, Tq, Tk = shape
    q, k, v, _ = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in R.attention_inputs(B, H, Tq, Tk, "flat", 0))
    ref = R.attention(q, k, v, H, scale)
    for ts in (True, False):
        pl = _plan(shape, ts, dict(kernel=K128, split_tiles=B * H * ((Tq + 127) // 128) if ts else 0))
        tag = "split" if ts else "no_split"
        out = _launch(dev, q, k, v, H, ts, scale=scale)
        ratio = _ratio(f"scale {scale} {shape} {tag}", out, ref, Tk, H, pl)
        parity.auto(float(ratio.max()), 1.0, tag=f"{tag}_d_over_bound")
        assert torch.equal(_launch(dev, q, k, v, H, ts, scale=scale).view(torch.int16), out.view(torch.int16)), f"{tag}: two launches differ"


@pytest.mark.parametrize("family", ("flat", "spiked"))
@pytest.mark.parametrize("var,val,shape,want", AB_CASES, ids=[f"{c[0]}={c[1]}-{'x'.join(map(str, c[2]))}" for c in AB_CASES])
def test_attention_ab_forms_within_float64_bound(dev, var, val, shape, want, family, monkeypatch, ab_lib):
    """The forms only the measurement build launches (32x32x16 MFMA, 192-row tiles everywhere, the 128-row kernel where the
    mixed grid would run, the plain tile order, no fill rule), against the same bound."""
    _need_256(dev)
    B, H, Tq, Tk = shape
    monkeypatch.delenv(var, raising=False)
    _plan(shape, True, AB_DEFAULT.get(shape, {}))
    monkeypatch.setenv(var, val)
    pl = _plan(shape, True, want)
    q, k, v, planted = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in R.attention_inputs(B, H, Tq, Tk, family, 0))
    if family == "spiked":
        _planted_hold_mass(q, k, H, planted)
    ref = R.attention(q, k, v, H, SCALE)
    out = _launch(dev, q, k, v, H, True)
    ratio = _ratio(f"{var}={val} {shape} {family}", out, ref, Tk, H, pl)
    parity.auto(float(ratio.max()), 1.0, tag="d_over_bound")
    assert torch.equal(_launch(dev, q, k, v, H, True).view(torch.int16), out.view(torch.int16)), "two launches differ"


@pytest.mark.parametrize("family", ("flat", "spiked"))
@pytest.mark.parametrize("name,shape,tail_split,want", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_attention_fused_query_prep_within_float64_bound(dev, name, shape, tail_split, want, family):
    """The fused query preparation (q_norm + SPLIT RoPE on the Q fragments) against attention(q', k, v) with q' from
    ltxk_qknorm_rope (held to float64 by test_rowops_gpu.py; the fused path copies its rounding points).  The fused path sums
    the row's squares in another fp32 order, so a 1-ulp flip of rstd may move a couple of elements of q' by one bf16 ulp: dx is
    enlarged by ref64.attention_fused_dx (derived, not measured); the ledger records the share of rows that also stay inside
    the plain bound.  cos / sin are random per (head, row), so a wrong table row for the clamped rows of a ragged tile, or
    another head's weight, shows; the spiked family plants its keys from q'."""
    from mlx_video_amd import ops
    _need_256(dev)
    B, H, Tq, Tk = shape
    D = H * 128
    pl = _plan(shape, tail_split, want, fused_q=True)
    q, k, v, _ = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in R.attention_inputs(B, H, Tq, Tk, "flat", 1))
    g = torch.Generator().manual_seed(B * 100 + Tq + Tk)
    w = (1 + 0.1 * torch.randn(1, D, generator=g)).to(BF).to(dev)
    ang = torch.rand(H, Tq, 64, generator=g) * (2 * math.pi)
    cos, sin = torch.cos(ang).contiguous().to(dev), torch.sin(ang).contiguous().to(dev)
    ss = (q.float() ** 2).reshape(B * Tq, D // 64, 64).sum(-1)
    qp = q.reshape(B * Tq, D).clone()
    ops.qknorm_rope(qp, 1, D, w, cos, sin, Tq, H, 1e-6)
    qp = qp.reshape(B, Tq, D)
    if family == "spiked":
        k, planted = R.attention_plant(qp, k)
        _planted_hold_mass(qp, k, H, planted)
    y, A, dx = R.attention(qp, k, v, H, SCALE)
    wide = (y, A, dx + R.attention_fused_dx(qp, k, H, SCALE))
    kw = dict(q_sumsq=ss, q_norm_weight=w, cos=cos, sin=sin, eps=1e-6)
    out = _launch(dev, q, k, v, H, tail_split, **kw)
    ratio = _ratio(f"fused {name} {shape} {family}", out, wide, Tk, H, pl)
    parity.auto(float(ratio.max()), 1.0, tag="d_over_enlarged_bound")
    d, bound = R.attention_bound(out, y, A, dx, Tk)
    parity.auto(float((d <= bound).all(-1).double().mean()), 1.0, tag="share_of_rows_inside_plain_bound")
    assert torch.equal(_launch(dev, q, k, v, H, tail_split, **kw).view(torch.int16), out.view(torch.int16)), "two launches differ"
