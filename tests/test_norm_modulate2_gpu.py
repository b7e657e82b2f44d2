"""ltxk_rmsnorm_modulate2 (ops.rmsnorm_modulate(scale2=, shift2=, out2=)): one normalisation pass, two modulations.

The yardstick is the existing single-output entry on the same operands: both outputs are torch.equal to it, in the carried-
statistic form (against ltxk_rmsnorm_modulate_ss, with and without LTXK_NORM_SCALE_IS_ONE_PLUS) and in the self-reducing form
(against ltxk_rmsnorm_modulate).  Shapes: D in {512 (one 512-element piece per row), 2048, 4096 (two 16-byte chunks per lane)}
x M in {1, 5 (not a multiple of the 4 rows / items of a workgroup), 130 (more than one workgroup, ragged)}; modulation row 0
for every token, or a 2-row map; sumsq with a leading dimension larger than D/64 and 1e30 in the slack (a kernel that summed
past sumsq_n would turn every output to zero).  The shim takes contiguous (M,D) outputs, so the sentinels are NaN rows in front
of, between and behind the two outputs inside one allocation: a store outside [0, M*D) of either output lands on one."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EPS = 1e-6


def _case(dev, M, D, rows, with_ss, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, D, generator=g) * 1.7).to(BF)
    U = 2 if rows else 1
    mod = (torch.randn(U, 5, D, generator=g) * 0.5).to(BF).to(dev)      # (U,5,D): the cross-modal table's layout
    mod_row = (torch.arange(M) % 2).to(torch.int32).to(dev) if rows else None
    ss = None
    if with_ss:
        P = D // 64
        ss = torch.full((M, P + 3), 1e30, dtype=torch.float32)
        ss[:, :P] = x.float().reshape(M, P, 64).square().sum(-1)
        ss = ss.to(dev)[:, :P + 3]
    return x.to(dev), mod, mod_row, ss


@pytest.mark.parametrize("form", ["ss_one_plus", "ss", "self"])
@pytest.mark.parametrize("rows", [False, True], ids=["row0", "rowmap"])
@pytest.mark.parametrize("M", [1, 5, 130])
@pytest.mark.parametrize("D", [512, 2048, 4096])
def test_both_outputs_equal_the_single_launches(dev, D, M, rows, form):
    from mlx_video_amd import ops
    x, mod, mod_row, ss = _case(dev, M, D, rows, form != "self", 1000 + D + M)
    kw = dict(sumsq=ss, scale_is_one_plus=form == "ss_one_plus")
    ms = 5 * D
    ref0 = ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], ms, mod_row, **kw)
    ref1 = ops.rmsnorm_modulate(x, EPS, mod[:, 2], mod[:, 3], ms, mod_row, **kw)
    # contiguous (M,D) outputs, each framed by NaN sentinel rows in one allocation and followed by a NaN tail
    frame = torch.full((2 * M + 3, D), float("nan"), dtype=BF, device=dev)
    y0, y1 = frame[1:M + 1], frame[M + 2:2 * M + 2]
    out = ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], ms, mod_row, out=y0, scale2=mod[:, 2], shift2=mod[:, 3], out2=y1, **kw)
    torch.cuda.synchronize()
    assert out[0] is y0 and out[1] is y1
    assert torch.equal(y0, ref0) and torch.equal(y1, ref1)
    assert not torch.equal(ref0, ref1) and bool(torch.isfinite(ref0.float()).all())
    assert bool(torch.isnan(frame[0]).all()) and bool(torch.isnan(frame[M + 1]).all()) and bool(torch.isnan(frame[2 * M + 2]).all())
    # the two outputs do not depend on each other: the pairs swapped give the outputs swapped
    s0, s1 = ops.rmsnorm_modulate(x, EPS, mod[:, 2], mod[:, 3], ms, mod_row, scale2=mod[:, 0], shift2=mod[:, 1], **kw)
    assert torch.equal(s0, ref1) and torch.equal(s1, ref0)


def test_outputs_allocated_by_the_shim_and_columns_past_d_untouched(dev):
    """x, scale and shift as rows of wider tables (stride 5D), D = 1024; the outputs the shim allocates equal the single
    launches; and an x that is the head of a larger allocation leaves what follows it unread (NaN there changes nothing)."""
    from mlx_video_amd import ops
    M, D = 7, 1024
    x, mod, mod_row, ss = _case(dev, M, D, True, True, 77)
    big = torch.full((M + 1, D), float("nan"), dtype=BF, device=dev)
    big[:M] = x
    a0, a1 = ops.rmsnorm_modulate(big[:M], EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, sumsq=ss, scale2=mod[:, 2], shift2=mod[:, 3])
    b0, b1 = ops.rmsnorm_modulate(big[:M], EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, scale2=mod[:, 2], shift2=mod[:, 3])
    for got, sc, sh in ((a0, 0, 1), (a1, 2, 3)):
        assert torch.equal(got, ops.rmsnorm_modulate(x, EPS, mod[:, sc], mod[:, sh], 5 * D, mod_row, sumsq=ss))
    for got, sc, sh in ((b0, 0, 1), (b1, 2, 3)):
        assert torch.equal(got, ops.rmsnorm_modulate(x, EPS, mod[:, sc], mod[:, sh], 5 * D, mod_row))


def test_shim_refusals(dev):
    from mlx_video_amd import ops
    M, D = 5, 512
    x, mod, mod_row, ss = _case(dev, M, D, True, True, 5)
    two = dict(scale2=mod[:, 2], shift2=mod[:, 3])
    with pytest.raises(ValueError, match="out2"):
        ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, out2=torch.empty((M + 1, D), dtype=BF, device=dev), **two)
    with pytest.raises(ValueError, match="out"):
        ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, out=torch.empty((M, 2 * D), dtype=BF, device=dev), **two)
    with pytest.raises(ValueError, match="scale_is_one_plus needs sumsq"):
        ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, scale_is_one_plus=True, **two)
    with pytest.raises(ValueError, match="second modulation"):
        ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, scale2=mod[:, 2])
    with pytest.raises(ValueError, match="second modulation"):
        ops.rmsnorm_modulate(x, EPS, scale2=mod[:, 2], shift2=mod[:, 3])
    with pytest.raises(ValueError, match="out2 goes with"):
        ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, out2=torch.empty_like(x))
    with pytest.raises(TypeError, match="shift2"):
        ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, scale2=mod[:, 2], shift2=mod.float()[:, 3])
    with pytest.raises(ValueError, match="scale2"):
        ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, scale2=mod[:, 2, :256], shift2=mod[:, 3])
    y = torch.empty_like(x)
    with pytest.raises(ValueError, match="two buffers"):
        ops.rmsnorm_modulate(x, EPS, mod[:, 0], mod[:, 1], 5 * D, mod_row, out=y, out2=y, **two)
