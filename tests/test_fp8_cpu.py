"""FP8 (e4m3) weight storage, the parts that need no GPU: the C ABI's new entries and their plans, the quantiser, the
checkpoint loader and the CLI flag."""
import ctypes
import json
import struct

import pytest
import torch

BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def test_w8_entries_exported_and_bound():
    from mlx_video_amd import _lib
    lib = _lib.load()
    for name in ("ltxk_gemm_w8", "ltxk_gemm_w8_plan"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    assert lib.ltxk_version() >= 404
    assert lib.ltxk_abi_sizeof(0) == ctypes.sizeof(_lib.GemmArgs)          # ltxk_gemm_args is unchanged


def _args(M, N, K, ws, /, **over):
    from mlx_video_amd._lib import GemmArgs
    a = GemmArgs()
    a.A = a.W = a.out = 1 << 12
    a.M, a.N, a.K, a.lda, a.ldo = M, N, K, K, N
    if ws:
        a.workspace, a.workspace_bytes = 1 << 12, 64 << 20
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _plan(fn, a):
    from mlx_video_amd import _lib
    pl = _lib.GemmPlan()
    rc = fn(ctypes.byref(a), ctypes.byref(pl))
    return rc, pl


def test_w8_plan_agrees_with_bf16_plan():
    from mlx_video_amd import _lib
    lib = _lib.load()
    seen = set()
    for M in (1, 33, 64, 160, 161, 200, 320, 640, 641, 1280, 2048, 2560):
        for N in (8, 136, 1024, 4096, 8192, 16384):
            for K in (64, 576, 2112, 4096, 16384):
                for ws in (False, True):
                    a = _args(M, N, K, ws)
                    rb, pb = _plan(lib.ltxk_gemm_plan, a)
                    r8, p8 = _plan(lib.ltxk_gemm_w8_plan, a)
                    assert rb == r8 == 0
                    seen.add(pb.form)
                    if pb.form == _lib.GEMM_FORM_BIG:
                        assert p8.form == _lib.GEMM_FORM_SINGLE and p8.slices == 1 and p8.ksteps == K // 64, (M, N, K, ws)
                    else:
                        assert (p8.form, p8.slices, p8.ksteps) == (pb.form, pb.slices, pb.ksteps), (M, N, K, ws)
                        assert (p8.tile_rows, p8.tile_cols, p8.row_tiles, p8.col_tiles) == (pb.tile_rows, pb.tile_cols, pb.row_tiles, pb.col_tiles)
    assert seen == {_lib.GEMM_FORM_SINGLE, _lib.GEMM_FORM_BIG, _lib.GEMM_FORM_SPLITK}       # the grid reaches every form
    # the GPU tests' split-K shapes: four slices with a short last one; the 160-row tile plus a remainder
    for M, want in ((64, (4, 9)), (200, (2, 17))):
        _, p8 = _plan(lib.ltxk_gemm_w8_plan, _args(M, 1024, 2112, True))
        assert p8.form == _lib.GEMM_FORM_SPLITK and (p8.slices, p8.ksteps) == want


def test_w8_argument_errors_match_bf16():
    from mlx_video_amd import _lib
    lib = _lib.load()
    bad = [dict(K=100), dict(N=12), dict(lda=8), dict(A=0), dict(W=(1 << 12) + 8), dict(out=(1 << 12) + 2), dict(epilogue=9),
           dict(epilogue=4), dict(epilogue=3, resid=1 << 12, ldr=1024), dict(n_split=100), dict(out_tokens_per_batch=7),
           dict(sumsq=(1 << 12) + 2, sumsq_ld=16), dict(M=0)]
    for over in bad:
        a = _args(64, 1024, 2112, True, **over)
        rb, _ = _plan(lib.ltxk_gemm_plan, a)
        r8, _ = _plan(lib.ltxk_gemm_w8_plan, a)
        assert rb == r8 == -1, over                                        # LTXK_EINVAL from both
        assert lib.ltxk_gemm_w8(ctypes.byref(a), None, None) == -1         # refused before anything is launched
        assert lib.ltxk_gemm_bf16(ctypes.byref(a), None) == -1
    assert lib.ltxk_gemm_w8_plan(ctypes.byref(_args(64, 1024, 2112, True)), None) == -1
    # a misaligned w_scale is refused on the host, whatever else is right
    assert lib.ltxk_gemm_w8(ctypes.byref(_args(64, 1024, 2112, True)), ctypes.c_void_p((1 << 12) + 2), None) == -1
    assert b"w_scale" in lib.ltxk_last_error()


def test_quantize_fp8_plain_cast():
    from mlx_video_amd.weights import dequantize_fp8, quantize_fp8
    w = (torch.randn(24, 64, generator=torch.Generator().manual_seed(1)) * 0.05).to(BF)
    q, s = quantize_fp8(w, "none")
    assert s is None and q.dtype == F8
    assert torch.equal(q.view(torch.uint8), w.to(F8).view(torch.uint8))
    assert torch.equal(dequantize_fp8(q), w.to(F8).float())
    with pytest.raises(ValueError):
        quantize_fp8(w, "group")


def test_quantize_fp8_channel():
    from mlx_video_amd.weights import dequantize_fp8, quantize_fp8
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(40, 128, generator=g) * torch.logspace(-4, 2, 40)[:, None]).to(BF)
    w[7] = 0                                                       # a zero row
    w[9, 1:] = 0                                                   # a row with one non-zero element
    q, s = quantize_fp8(w, "channel")
    assert q.dtype == F8 and s.dtype == torch.float32 and s.shape == (40,)
    amax = w.float().abs().amax(1)
    assert float(s[7]) == 1.0 and bool((q[7].float() == 0).all()) and bool((dequantize_fp8(q, s)[7] == 0).all())
    nz = amax > 0
    assert torch.equal(q.float().abs().amax(1)[nz], torch.full((int(nz.sum()),), 448.0))     # amax -> +-448 exactly
    top = w.float().abs() == amax[:, None]
    assert torch.equal(q.float()[top & nz[:, None]], 448.0 * torch.sign(w.float()[top & nz[:, None]]))
    assert bool(torch.isfinite(q.float()).all())
    err = (w.double() - dequantize_fp8(q, s, torch.float64)).abs()
    assert bool((err <= amax.double()[:, None] * 2.0 ** -4).all()), float((err / amax.clamp_min(1e-30)[:, None]).max())
    assert dequantize_fp8(q, s, BF).dtype == BF


def _write_safetensors(path, tensors):
    """A safetensors file by hand (8-byte header length + JSON + raw bytes)."""
    names = {torch.bfloat16: "BF16", torch.float8_e4m3fn: "F8_E4M3"}
    header, blobs, off = {}, [], 0
    for k, t in tensors.items():
        raw = t.contiguous().view(torch.uint8).numpy().tobytes()
        header[k] = {"dtype": names[t.dtype], "shape": list(t.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    h = json.dumps(header).encode()
    h += b" " * (-len(h) % 8)
    path.write_bytes(struct.pack("<Q", len(h)) + h + b"".join(blobs))


def test_loader_keeps_fp8_and_quantises_bf16(tmp_path):
    from mlx_video_amd.weights import read_safetensors, transformer_weights
    g = torch.Generator().manual_seed(3)
    w8 = (torch.randn(16, 64, generator=g) * 0.1).to(F8)
    wb = (torch.randn(8, 64, generator=g) * 0.1).to(BF)
    bias = torch.randn(8, generator=g).to(BF)
    table = torch.randn(6, 64, generator=g).to(BF)
    f = tmp_path / "t.safetensors"
    _write_safetensors(f, {"transformer.proj_out.weight": w8, "transformer.patchify_proj.weight": wb,
                           "transformer.patchify_proj.bias": bias, "transformer.transformer_blocks.0.scale_shift_table": table})
    raw = read_safetensors([f])
    assert raw["transformer.proj_out.weight"].dtype == F8                 # safetensors reads F8_E4M3
    on = transformer_weights(raw, "cpu", fp8=True)
    assert on["proj_out.weight"].dtype == F8 and "proj_out.weight_scale" not in on
    assert torch.equal(on["proj_out.weight"].view(torch.uint8), w8.view(torch.uint8))         # kept byte for byte, no scale
    assert on["patchify_proj.weight"].dtype == F8 and on["patchify_proj.weight_scale"].shape == (8,)
    assert on["patchify_proj.bias"].dtype == BF and on["transformer_blocks.0.scale_shift_table"].dtype == BF
    plain = transformer_weights(raw, "cpu", fp8=True, fp8_scaling="none")
    assert torch.equal(plain["patchify_proj.weight"].view(torch.uint8), wb.to(F8).view(torch.uint8)) and "patchify_proj.weight_scale" not in plain
    off = transformer_weights(raw, "cpu")
    assert set(off) == {"proj_out.weight", "patchify_proj.weight", "patchify_proj.bias", "transformer_blocks.0.scale_shift_table"}
    assert all(v.dtype == BF for v in off.values())
    assert torch.equal(off["proj_out.weight"], w8.to(BF)) and torch.equal(off["patchify_proj.weight"], wb)


def test_cli_enable_fp8_reaches_generate_video(monkeypatch):
    import inspect

    from mlx_video_amd import generate as G
    from mlx_video_amd.pipelines import MLXPipelineConfig
    sig = inspect.signature(G.generate_video).parameters
    assert sig["enable_fp8"].default is False and sig["fp8_scaling"].default == "channel"
    assert MLXPipelineConfig().fp8transformer is False
    ap = G.build_parser()
    assert ap.parse_args([]).enable_fp8 is False and ap.parse_args([]).fp8_scaling == "channel"
    assert ap.parse_args(["--enable-fp8", "--fp8-scaling", "none"]).fp8_scaling == "none"
    with pytest.raises(SystemExit):
        ap.parse_args(["--fp8-scaling", "group"])
    seen = {}
    monkeypatch.setattr(G, "generate_video", lambda **kw: seen.update(kw))
    G.main(["--prompt", "x", "--model-repo", "/nonexistent", "--enable-fp8"])
    assert seen["enable_fp8"] is True and seen["fp8_scaling"] == "channel"
    seen.clear()
    G.main(["--prompt", "x", "--model-repo", "/nonexistent"])
    assert seen["enable_fp8"] is False
