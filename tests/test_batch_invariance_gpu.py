"""LTXModel.batch_invariant: a forward's bits do not depend on the batch it runs in.  Full width (D=4096), one block, video
token counts inside the GEMM's split-K range (M <= 640) and a 64-token context, so that every GEMM of the forward - text k|v
and the caption projection included - is one whose default plan may split K.  Each T first checks, with ops.gemm_plan, that
the default B=1 and B=2 plans really differ there: the bit-equality below would fail if batch_invariant stopped withholding
the split-K scratch.  The default mode is held to a rel-L2 bound instead."""
import pytest
import torch

import parity
from dit_launches import dit_launches

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GEOM = {32: (2, 4, 4), 128: (2, 8, 8), 160: (5, 4, 8), 320: (5, 8, 8)}     # T = F*H*W video tokens
S_CTX = 64


@pytest.fixture(scope="module")
def model(dev):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    return LTXModel.random_init(LTXModelConfig(num_layers=1), dev, seed=21)


def _plans_differ(T):
    from mlx_video_amd import ops

    def key(p):
        return (p.form, p.slices)
    one = {n: key(ops.gemm_plan(M, N, K, **kw)) for n, M, N, K, kw in dit_launches(ops, 1, T, S_CTX)}
    two = {n: key(ops.gemm_plan(M, N, K, **kw)) for n, M, N, K, kw in dit_launches(ops, 2, T, S_CTX)}
    return [n for n in one if one[n] != two[n]]


def _inputs(dev, T, seed):
    from mlx_video_amd.ltx_model import TimestepPlan, precompute_freqs_cis
    from mlx_video_amd.schedulers import create_position_grid
    g = torch.Generator(device=dev).manual_seed(seed)
    tok = torch.randn((2, T, 128), generator=g, device=dev).to(BF)
    ctx = torch.randn((2, S_CTX, 3840), generator=g, device=dev).to(BF)
    pe = precompute_freqs_cis(create_position_grid(1, *GEOM[T]).to(dev), 4096)
    ts = torch.tensor([0.625], dtype=BF, device=dev)

    def plan(B):
        return TimestepPlan(ts, torch.zeros(B * T, dtype=torch.int32, device=dev))
    return tok, ctx, pe, plan


@pytest.mark.parametrize("T", sorted(GEOM))
def test_forward_rows_do_not_depend_on_the_batch(dev, model, T):
    differ = _plans_differ(T)
    assert differ, f"T={T}: the default B=1 and B=2 plans agree - this T no longer tests batch invariance"
    tok, ctx, pe, plan = _inputs(dev, T, 100 + T)
    try:
        model.batch_invariant = True
        both = model.forward_tokens(tok, plan(2), ctx, pe)
        rows = [model.forward_tokens(tok[b:b + 1].contiguous(), plan(1), ctx[b:b + 1].contiguous(), pe) for b in range(2)]
        fused = {}
        for fuse in (15 | 8, 14):          # q|k and v as two launches (bit 8 / bit 1 off), text k and v as two (bit 1 off)
            model.fuse = fuse
            fused[fuse] = model.forward_tokens(tok, plan(2), ctx, pe)
        model.fuse = 15
        model.batch_invariant = False
        dflt_both = model.forward_tokens(tok, plan(2), ctx, pe)
        dflt_rows = [model.forward_tokens(tok[b:b + 1].contiguous(), plan(1), ctx[b:b + 1].contiguous(), pe) for b in range(2)]
        torch.cuda.synchronize()
    finally:
        model.batch_invariant, model.fuse = False, 15
    assert bool(torch.isfinite(both.float()).all())
    for b in range(2):
        assert torch.equal(both[b], rows[b][0]), f"T={T} row {b}: B=2 differs from B=1 (default plans differ in {differ})"
    for fuse, v in fused.items():
        assert torch.equal(v, both), f"T={T}: fuse={fuse} differs from fuse=15 in batch-invariant mode"
    # default mode: split-K groupings differ between the two batch sizes - close, not equal
    err = max(parity.rel_l2(dflt_both[b], dflt_rows[b][0]) for b in range(2))
    parity.auto(err, 1e-2, tag=f"default_T{T}")
    parity.auto(parity.rel_l2(dflt_both, both), 1e-2, tag=f"default_vs_invariant_T{T}")


@pytest.mark.parametrize("T", [32, 320])
def test_cfg_batch_equals_two_passes(dev, model, T):
    """denoise_dev over two CFG steps: cfg_batch=True (one B=2 forward per step) == cfg_batch=False (two B=1 forwards)."""
    from mlx_video_amd.denoise import denoise_dev
    from mlx_video_amd.schedulers import create_position_grid, ltx2_scheduler
    assert _plans_differ(T)
    F, H, W = GEOM[T]
    g = torch.Generator(device=dev).manual_seed(7 + T)
    lat = torch.randn((1, 128, F, H, W), generator=g, device=dev).to(BF)
    cp = torch.randn((1, S_CTX, 3840), generator=g, device=dev).to(BF)
    cn = torch.randn((1, S_CTX, 3840), generator=g, device=dev).to(BF)
    sig = ltx2_scheduler(30, T)[:3]
    pos = create_position_grid(1, F, H, W).to(dev)
    try:
        model.batch_invariant = True
        a = denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=True)
        b = denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=False)
        torch.cuda.synchronize()
    finally:
        model.batch_invariant = False
    assert bool(torch.isfinite(a.float()).all())
    assert torch.equal(a, b), f"T={T}: cfg_batch changes the bits in batch-invariant mode"
