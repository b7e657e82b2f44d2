"""ltx_model.Linear on CPU tensors: a Linear layer's matrix, optional per-channel scale and bias as one value; packed panels
(Linear.cat) and their row ranges (rows) without copies."""
import torch

from mlx_video_amd.ltx_model import Linear

BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def _part(n, k, seed, fp8=False, scaled=False):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g).to(F8 if fp8 else BF)
    scale = torch.rand(n, generator=g) + 0.5 if scaled else None
    return Linear(w, scale, torch.randn(n, generator=g).to(BF))


def test_n_and_k():
    p = _part(24, 64, 1)
    assert (p.N, p.K) == (24, 64)
    assert (p.rows(8, None).N, p.rows(8, None).K) == (16, 64)


def test_cat_bf16():
    parts = [_part(16, 64, 1), _part(8, 64, 2), _part(24, 64, 3)]
    p = Linear.cat(parts)
    assert (p.N, p.K) == (48, 64) and p.w.dtype == BF and p.w.is_contiguous() and p.scale is None
    assert torch.equal(p.w, torch.cat([q.w for q in parts], 0))
    assert torch.equal(p.bias, torch.cat([q.bias for q in parts], 0))


def test_cat_fp8_keeps_the_parts_bytes_in_order():
    parts = [_part(16, 128, 4, fp8=True), _part(32, 128, 5, fp8=True)]
    p = Linear.cat(parts)
    assert p.w.dtype == F8 and p.w.shape == (48, 128) and p.w.is_contiguous()
    assert torch.equal(p.w.view(torch.uint8), torch.cat([q.w.view(torch.uint8) for q in parts], 0))
    assert p.scale is None                                  # no part is scaled: the panel is not
    assert torch.equal(p.bias, torch.cat([q.bias for q in parts], 0))


def test_cat_fills_missing_scales_with_ones():
    a, b, c = _part(16, 128, 6, fp8=True, scaled=True), _part(8, 128, 7, fp8=True), _part(8, 128, 8, fp8=True, scaled=True)
    p = Linear.cat([a, b, c])
    assert p.scale.dtype == torch.float32 and p.scale.shape == (32,) and p.scale.is_contiguous()
    assert torch.equal(p.scale[:16], a.scale) and torch.equal(p.scale[24:], c.scale)
    assert torch.equal(p.scale[16:24], torch.ones(8))
    assert b.scale is None                                  # the parts are left as they were


def test_rows_are_views_of_the_panel():
    p = Linear.cat([_part(16, 128, 9, fp8=True, scaled=True), _part(16, 128, 10, fp8=True, scaled=True)])
    r = p.rows(16, None)
    assert (r.N, r.K) == (16, 128)
    for view, whole in ((r.w, p.w), (r.scale, p.scale), (r.bias, p.bias)):
        assert view.untyped_storage().data_ptr() == whole.untyped_storage().data_ptr()
        assert view.storage_offset() == 16 * whole.stride(0)
    r.scale[3] = 7.0
    r.bias[5] = -2.0
    r.w.view(torch.uint8)[2, 9] = 0x38                      # e4m3 1.0
    assert p.scale[19] == 7.0 and p.bias[21] == -2.0 and p.w.view(torch.uint8)[18, 9] == 0x38
    head = p.rows(None, 16)
    assert head.w.storage_offset() == 0 and head.N == 16 and torch.equal(head.w.view(torch.uint8), p.w.view(torch.uint8)[:16])


def test_rows_of_an_unscaled_panel_have_no_scale():
    p = Linear.cat([_part(16, 64, 11), _part(16, 64, 12)])
    r = p.rows(0, 16)
    assert r.scale is None and r.w.dtype == BF
    r.w[1, 2] = 3.0
    assert p.w[1, 2] == 3.0
