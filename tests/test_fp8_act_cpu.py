"""FP8 activations, the parts that need no GPU: the flag's argument rules, the operand validation of ops.gemm (which runs before
any library call), and the C header against the ctypes binding for the new entry points."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def test_cli_and_generate_video_argument_rules(monkeypatch):
    import inspect

    from mlx_video_amd import generate as G
    from mlx_video_amd.pipelines import MLXPipelineConfig
    assert inspect.signature(G.generate_video).parameters["fp8_activations"].default is False
    assert MLXPipelineConfig().fp8activations is False
    ap = G.build_parser()
    assert ap.parse_args([]).fp8_activations is False
    assert ap.parse_args(["--enable-fp8", "--fp8-activations"]).fp8_activations is True
    seen = {}
    monkeypatch.setattr(G, "generate_video", lambda **kw: seen.update(kw))
    G.main(["--prompt", "x", "--model-repo", "/nonexistent", "--enable-fp8", "--fp8-activations"])
    assert seen["enable_fp8"] is True and seen["fp8_activations"] is True
    seen.clear()
    G.main(["--prompt", "x", "--model-repo", "/nonexistent", "--enable-fp8"])
    assert seen["fp8_activations"] is False
    seen.clear()
    with pytest.raises(ValueError, match="--enable-fp8"):
        G.main(["--prompt", "x", "--model-repo", "/nonexistent", "--fp8-activations"])
    assert not seen                                        # refused before generate_video is reached
    monkeypatch.undo()
    with pytest.raises(ValueError, match="enable_fp8"):    # and by generate_video itself, before anything is loaded
        G.generate_video(prompt="x", model_repo="/nonexistent", fp8_activations=True)


def test_pipeline_config_passes_the_flag(monkeypatch):
    from mlx_video_amd import pipelines as P
    assert {f.name for f in P.fields(P.MLXPipelineConfig)} >= {"fp8transformer", "fp8activations"}
    assert P._Base().fp8activations is False
    assert P._Base(fp8transformer=True, fp8activations=True)._cfg().fp8activations is True


def test_model_argument_check():
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    mc = LTXModelConfig(num_attention_heads=4, num_layers=1, caption_channels=256, cross_attention_dim=512)
    with pytest.raises(ValueError, match="fp8_activations"):              # before any weight is looked at
        LTXModel(mc, {"patchify_proj.weight": torch.zeros(512, 128, dtype=BF)}, fp8_activations=True)


def test_gemm_operand_validation_runs_before_the_library():
    from mlx_video_amd import ops
    a8, ab = torch.zeros(4, 128, dtype=torch.uint8).view(F8), torch.zeros(4, 128, dtype=BF)
    w8, wb = torch.zeros(8, 128, dtype=torch.uint8).view(F8), torch.zeros(8, 128, dtype=BF)
    sc = torch.ones(4)
    with pytest.raises(TypeError, match="a_scale"):
        ops.gemm(a8, w8, None)                                            # fp8 activations without their scales
    with pytest.raises(TypeError, match="a_scale"):
        ops.gemm(ab, w8, None, a_scale=sc)                                # scales without fp8 activations
    with pytest.raises(TypeError, match="float8_e4m3fn weight"):
        ops.gemm(a8, wb, None, a_scale=sc)
    with pytest.raises(TypeError, match="float32"):
        ops.gemm(a8, w8, None, a_scale=sc.to(BF))
    with pytest.raises(ValueError, match="a_scale"):
        ops.gemm(a8, w8, None, a_scale=torch.ones(5))


def _c_params(name):
    hdr = open(os.path.join(ROOT, "include", "ltxk.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in ltxk.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_matches_binding_for_the_new_entries():
    from mlx_video_amd import _lib
    lib = _lib.load()
    assert lib.ltxk_version() >= 405

    def kind(p):
        if "*" in p:
            return "ptr"
        return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[p.split()[0]]

    for name in ("ltxk_gemm_w8a8", "ltxk_gemm_w8a8_plan", "ltxk_quant_rows_fp8"):
        res, argtypes = _lib.SIGNATURES[name]
        params = _c_params(name)
        assert res is ctypes.c_int32 and len(params) == len(argtypes), (name, params)
        for p, t in zip(params, argtypes):
            if kind(p) == "ptr":
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, p, t)
            else:
                assert t is kind(p), (name, p, t)
        assert getattr(lib, name).argtypes is not None
    assert lib.ltxk_abi_sizeof(0) == ctypes.sizeof(_lib.GemmArgs)            # ltxk_gemm_args is unchanged


def _args(**over):
    from mlx_video_amd._lib import GemmArgs
    a = GemmArgs()
    a.A = a.W = a.out = 1 << 12
    a.M, a.N, a.K, a.lda, a.ldo = 2560, 4096, 4096, 4096, 4096
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_w8a8_plan_is_single_pass_on_pick_tiles_tile():
    from mlx_video_amd import _lib, ops
    lib = _lib.load()
    for M in (1, 64, 161, 640, 1280, 2560):
        for N in (136, 4096, 16384):
            for K in (128, 4096, 16384):
                pa = ops.gemm_plan(M, N, K, w8a8=True)                   # the split-K scratch on offer: never taken
                assert pa.form == _lib.GEMM_FORM_SINGLE and pa.slices == 1 and pa.ksteps == K // 128
                p8 = ops.gemm_plan(M, N, K, w8=True, split_k=False)
                assert (pa.tile_rows, pa.tile_cols, pa.row_tiles, pa.col_tiles) == (p8.tile_rows, p8.tile_cols, p8.row_tiles, p8.col_tiles)
    pl = _lib.GemmPlan()
    for over in (dict(K=4096 + 64, lda=4096 + 64), dict(lda=4096 + 8), dict(A=(1 << 12) + 8)):
        assert lib.ltxk_gemm_w8a8_plan(ctypes.byref(_args(**over)), ctypes.byref(pl)) == -1, over
        assert lib.ltxk_gemm_w8a8(ctypes.byref(_args(**over)), ctypes.c_void_p(1 << 12), None, None) == -1, over
    assert lib.ltxk_gemm_w8a8(ctypes.byref(_args()), None, None, None) == -1 and b"a_scale" in lib.ltxk_last_error()
    assert lib.ltxk_quant_rows_fp8(ctypes.c_void_p(1 << 12), 100, ctypes.c_void_p(1 << 12), 128, ctypes.c_void_p(1 << 12), 4, 100, None) == -1
