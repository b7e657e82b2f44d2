"""The MXFP4 DiT, the parts that need no GPU: the quantised weight dict, the refusals of the two new shims on CPU tensors (they run
before any library call), the argument rules of --enable-mxfp4 / generate_video(enable_mxfp4=), the float64 GEMM emulation the
GPU tests rest on, and the C header against the ctypes binding."""
import ctypes
import os
import re

import pytest
import torch

import ref_gemm_mxfp4 as R4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
U8 = torch.uint8
IN_BLOCK = [f"{a}.{n}.weight" for a in ("attn1", "attn2") for n in ("to_q", "to_k", "to_v", "to_out")] + \
    ["ff.proj_in.weight", "ff.proj_out.weight"]


def _weights():
    """A 2-block bf16 module-key dict at D = 256 on the CPU (the shapes of LTXModel.random_weights)."""
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    cfg = LTXModelConfig(num_attention_heads=2, num_layers=2, caption_channels=64, cross_attention_dim=256)
    return cfg, LTXModel.random_weights(cfg, torch.device("cpu"), seed=3)


def test_quantised_weight_dict():
    from mlx_video_amd import weights as Wt
    from mlx_video_amd.ltx_model import MXSCALE_SUFFIX, is_mxfp4_weights
    assert Wt.MXSCALE_SUFFIX == MXSCALE_SUFFIX == "_mxscale"
    cfg, W = _weights()
    Q = Wt.quantize_transformer_weights_mxfp4(W)
    want = {f"transformer_blocks.{i}.{k}" for i in range(cfg.num_layers) for k in IN_BLOCK}
    assert {k for k in Q if k.endswith("_mxscale")} == {k + "_mxscale" for k in want}
    assert set(Q) == set(W) | {k + "_mxscale" for k in want} and is_mxfp4_weights(Q) and not is_mxfp4_weights(W)
    for k, v in W.items():
        if k in want:
            N, K = v.shape
            assert Q[k].dtype == U8 and tuple(Q[k].shape) == (N, K // 2)
            assert Q[k + "_mxscale"].dtype == U8 and tuple(Q[k + "_mxscale"].shape) == (N, K // 32)
            c, s = Wt.quantize_mxfp4(v)
            assert torch.equal(Wt.dequantize_mxfp4(Q[k], Q[k + "_mxscale"]), Wt.dequantize_mxfp4(c, s))
        else:
            assert Q[k] is v, f"{k} was touched"                       # patchify, AdaLN, caption projection, proj_out, biases, norms, tables
    assert all(v.dtype == BF for v in W.values())                      # the input is kept
    Q2 = Wt.quantize_transformer_weights_mxfp4(Q)                      # quantising a quantised dict is the identity
    assert set(Q2) == set(Q) and all(Q2[k] is Q[k] for k in Q)
    # transformer_weights(mxfp4=True) gives the same dict from raw module keys
    T = Wt.transformer_weights(W, "cpu", mxfp4=True)
    assert set(T) == set(Q) and all(torch.equal(T[k], Q[k]) for k in Q)
    with pytest.raises(ValueError, match="fp8 and mxfp4"):
        Wt.transformer_weights(W, "cpu", fp8=True, mxfp4=True)
    with pytest.raises(ValueError, match="fp8 and mxfp4"):
        Wt.load_pipeline_modules("/nonexistent", "cpu", fp8=True, mxfp4=True)


def test_model_refusals():
    from mlx_video_amd import weights as Wt
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    cfg, W = _weights()
    Q = Wt.quantize_transformer_weights_mxfp4(W)
    with pytest.raises(ValueError, match="fp8_activations"):
        LTXModel(cfg, Q, fp8_activations=True)
    with pytest.raises(ValueError, match="head-dim-64|attention_head_dim = 64"):
        LTXModel(LTXModelConfig.audio(num_layers=2), Q)


def _good(M=4, N=8, K=256):
    z = lambda *s: torch.zeros(s, dtype=U8)                            # noqa: E731
    return [z(M, K // 2), z(M, K // 32), z(N, K // 2), z(N, K // 32)]


GEMM_REFUSALS = [
    # (what, positional operands, keywords, exception, message)
    ("K not a multiple of the K-step", lambda: [t[:, :t.shape[1] // 2].contiguous() for t in _good()], {}, ValueError, "K % 256"),
    ("K = 384", lambda: _good(K=384), {}, ValueError, "K % 256"),
    ("N not a multiple of 8", lambda: _good(N=12), {}, ValueError, "N % 8"),
    ("a_scales of the wrong shape", lambda: [_good()[0], torch.zeros((4, 7), dtype=U8)] + _good()[2:], {}, ValueError, "a_scales"),
    ("w_scales of the wrong shape", lambda: _good()[:3] + [torch.zeros((9, 8), dtype=U8)], {}, ValueError, "w_scales"),
    ("codes not uint8 (a)", lambda: [_good()[0].to(torch.int8)] + _good()[1:], {}, TypeError, "a must be"),
    ("codes not uint8 (w)", lambda: _good()[:2] + [_good()[2].view(torch.float8_e4m3fn)] + _good()[3:], {}, TypeError, "w must be"),
    ("scales not uint8", lambda: [_good()[0], _good()[1].to(torch.int32)] + _good()[2:], {}, TypeError, "a_scales"),
    ("no scales", lambda: [_good()[0], None] + _good()[2:], {}, TypeError, "block-scale"),
    ("rows of a 8 bytes off a 16-byte stride", lambda: [torch.zeros((4, 136), dtype=U8)[:, :128]] + _good()[1:], {}, ValueError, "16 bytes apart"),
    ("rows of a_scales 4 bytes off", lambda: [_good()[0], torch.zeros((4, 12), dtype=U8)[:, :8]] + _good()[2:], {}, ValueError, "8 bytes apart"),
    ("a misaligned", lambda: [torch.zeros(4 * 128 + 8, dtype=U8)[8:].view(4, 128)] + _good()[1:], {}, ValueError, "a must be 16-byte aligned"),
    ("w not contiguous", lambda: _good()[:2] + [torch.zeros((8, 256), dtype=U8)[:, :128]] + _good()[3:], {}, ValueError, "w must be contiguous"),
    ("out of the wrong shape", _good, dict(out=torch.zeros((4, 16), dtype=BF)), ValueError, "out"),
    ("out not bf16", _good, dict(out=torch.zeros((4, 8))), TypeError, "out"),
    ("split output without out2", _good, dict(n_split=256, out_tokens_per_batch=4), ValueError, "out2"),
]


@pytest.mark.parametrize("what,operands,kw,exc,msg", GEMM_REFUSALS, ids=[r[0] for r in GEMM_REFUSALS])
def test_gemm_mxfp4_refusals(what, operands, kw, exc, msg):
    from mlx_video_amd import ops
    with pytest.raises(exc, match=msg):
        ops.gemm_mxfp4(*operands(), **kw)


def test_shims_pass_well_formed_cpu_operands_up_to_the_device():
    from mlx_video_amd import _lib, ops
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        ops.gemm_mxfp4(*_good())
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        ops.quant_rows_mxfp4(torch.zeros((4, 64), dtype=BF))


QUANT_REFUSALS = [
    ("not bf16", lambda: torch.zeros((4, 64)), None, TypeError, "a must be"),
    ("K not a multiple of 32", lambda: torch.zeros((4, 48), dtype=BF), None, ValueError, "K % 32"),
    ("row stride", lambda: torch.zeros((4, 68), dtype=BF)[:, :64], None, ValueError, "8 elements apart"),
    ("codes of the wrong shape", lambda: torch.zeros((4, 64), dtype=BF), lambda: (torch.zeros((4, 64), dtype=U8), torch.zeros((4, 2), dtype=U8)),
     ValueError, r"out\[0\]"),
    ("scales of the wrong shape", lambda: torch.zeros((4, 64), dtype=BF), lambda: (torch.zeros((4, 32), dtype=U8), torch.zeros((4, 3), dtype=U8)),
     ValueError, r"out\[1\]"),
    ("codes not uint8", lambda: torch.zeros((4, 64), dtype=BF), lambda: (torch.zeros((4, 32), dtype=torch.int8), torch.zeros((4, 2), dtype=U8)),
     TypeError, r"out\[0\]"),
    ("code rows 8 bytes off", lambda: torch.zeros((4, 64), dtype=BF), lambda: (torch.zeros((4, 40), dtype=U8)[:, :32], torch.zeros((4, 2), dtype=U8)),
     ValueError, "16 bytes apart"),
]


@pytest.mark.parametrize("what,a,out,exc,msg", QUANT_REFUSALS, ids=[r[0] for r in QUANT_REFUSALS])
def test_quant_rows_mxfp4_refusals(what, a, out, exc, msg):
    from mlx_video_amd import ops
    with pytest.raises(exc, match=msg):
        ops.quant_rows_mxfp4(a(), out=None if out is None else out())


def test_cli_and_generate_video_argument_rules(monkeypatch):
    import inspect

    from mlx_video_amd import generate as G
    assert inspect.signature(G.generate_video).parameters["enable_mxfp4"].default is False
    ap = G.build_parser()
    assert ap.parse_args([]).enable_mxfp4 is False and ap.parse_args(["--enable-mxfp4"]).enable_mxfp4 is True
    seen = {}
    monkeypatch.setattr(G, "generate_video", lambda **kw: seen.update(kw))
    G.main(["--prompt", "x", "--model-repo", "/nonexistent"])
    assert "enable_mxfp4" not in seen                                  # the default adds no keyword to today's call
    seen.clear()
    G.main(["--prompt", "x", "--model-repo", "/nonexistent", "--enable-mxfp4"])
    assert seen["enable_mxfp4"] is True and seen["enable_fp8"] is False
    seen.clear()
    for other in (["--enable-fp8"], ["--enable-fp8", "--fp8-activations"]):
        with pytest.raises(ValueError, match="--enable-mxfp4.*--enable-fp8"):
            G.main(["--prompt", "x", "--model-repo", "/nonexistent", "--enable-mxfp4"] + other)
    assert not seen                                                    # refused before generate_video is reached
    monkeypatch.undo()
    for kw in (dict(enable_fp8=True), dict(enable_fp8=True, fp8_activations=True), dict(fp8_activations=True)):
        with pytest.raises(ValueError, match="enable_mxfp4.*enable_fp8"):          # names both, before anything is loaded
            G.generate_video(prompt="x", model_repo="/nonexistent", enable_mxfp4=True, **kw)
    with pytest.raises(ValueError, match="joint.*enable_mxfp4"):
        G.generate_video(prompt="x", model_repo="/nonexistent", enable_mxfp4=True, audio=True, audio_mode="joint", pipeline=G.PipelineType.DEV)


def test_defaults_add_no_keyword_to_the_loader(monkeypatch, tmp_path):
    """generate_video without enable_mxfp4 calls load_pipeline_modules with today's keywords; with it, ``mxfp4=True`` is added."""
    from mlx_video_amd import generate as G
    from mlx_video_amd import weights as Wt

    class Stop(Exception):
        pass

    seen = {}

    def loader(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(Wt, "load_pipeline_modules", loader)
    with pytest.raises(Stop):
        G.generate_video(prompt="x", model_repo=str(tmp_path), prompt_embeds=torch.zeros(1, 4, 8))
    assert "mxfp4" not in seen and seen["fp8"] is False
    seen.clear()
    with pytest.raises(Stop):
        G.generate_video(prompt="x", model_repo=str(tmp_path), prompt_embeds=torch.zeros(1, 4, 8), enable_mxfp4=True)
    assert seen["mxfp4"] is True and seen["fp8"] is False


def test_float64_emulation_reproduces_a_hand_computed_case():
    """2 x 2 x 32.  a0 = [+0.5, -6, 1.5, 0 ...] at scale byte 128 (x2); a1 = [-0.0, 3, 0 ...] at byte 126 (x0.5);
    w0 = [4, 1, -2, 0 ...] at byte 127; w1 = [-1.5, 0.5, 6, 0 ...] at byte 129 (x4).  Codes: 0.5 = 1, 1 = 2, 1.5 = 3, 2 = 4, 3 = 5,
    4 = 6, 6 = 7, sign = 8; element 2i in the low nibble."""
    def row(*codes):
        r = torch.zeros(16, dtype=U8)
        for i, c in enumerate(codes):
            r[i // 2] |= c << (4 * (i % 2))
        return r
    a = torch.stack([row(0x1, 0xF, 0x3), row(0x8, 0x5)])
    w = torch.stack([row(0x6, 0x2, 0xC), row(0xB, 0x1, 0x7)])
    asc, wsc = torch.tensor([[128], [126]], dtype=U8), torch.tensor([[127], [129]], dtype=U8)
    da, dw = R4.dequant(a, asc), R4.dequant(w, wsc)
    assert da[0, :4].tolist() == [1.0, -12.0, 3.0, 0.0] and da[1, :3].tolist() == [-0.0, 1.5, 0.0]
    assert str(float(da[1, 0])) == "-0.0"
    assert dw[0, :4].tolist() == [4.0, 1.0, -2.0, 0.0] and dw[1, :3].tolist() == [-6.0, 2.0, 24.0]
    s, mag = R4.product(a, asc, w, wsc)
    # s00 = 1*4 - 12*1 + 3*(-2) = -14;  s01 = 1*(-6) - 12*2 + 3*24 = 42;  s10 = 1.5*1 = 1.5;  s11 = 1.5*2 = 3
    assert s.tolist() == [[-14.0, 42.0], [1.5, 3.0]]
    assert mag.tolist() == [[22.0, 102.0], [1.5, 3.0]]
    from mlx_video_amd.weights import dequantize_mxfp4
    assert torch.equal(dequantize_mxfp4(a, asc, torch.float64), da)    # and agrees with the product's own dequantiser


def test_header_matches_binding_for_the_new_entries():
    from mlx_video_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "ltxk.h")).read()
    assert int(re.search(r"#define LTXK_MXFP4_KSTEP (\d+)", hdr).group(1)) == ops.MXFP4_KSTEP == 256
    lib = _lib.load()

    def kind(p):
        if "*" in p:
            return "ptr"
        return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[p.split()[0]]

    for name in ("ltxk_gemm_mxfp4", "ltxk_gemm_mxfp4_plan", "ltxk_quant_rows_mxfp4"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in ltxk.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(params) == len(argtypes), (name, params)
        for p, t in zip(params, argtypes):
            assert (t is ctypes.c_void_p or issubclass(t, ctypes._Pointer)) if kind(p) == "ptr" else t is kind(p), (name, p, t)
        assert getattr(lib, name).argtypes is not None
    assert lib.ltxk_abi_sizeof(0) == ctypes.sizeof(_lib.GemmArgs)      # ltxk_gemm_args is unchanged


def test_plan_is_single_pass_on_pick_tiles_tile():
    from mlx_video_amd import _lib, ops
    for M in (1, 64, 161, 640, 1280, 2560):
        for N in (136, 4096, 16384):
            for K in (256, 4096, 16384):
                p4 = ops.gemm_plan(M, N, K, mxfp4=True)                  # the split-K scratch on offer: never taken
                assert p4.form == _lib.GEMM_FORM_SINGLE and p4.slices == 1 and p4.ksteps == K // 256
                pb = ops.gemm_plan(M, N, K, w8=True, split_k=False)
                assert (p4.tile_rows, p4.tile_cols, p4.row_tiles, p4.col_tiles) == (pb.tile_rows, pb.tile_cols, pb.row_tiles, pb.col_tiles)
    with pytest.raises(_lib.LtxkError):
        ops.gemm_plan(64, 1024, 2176, mxfp4=True)                        # K = 2176 is a multiple of 128, not of the K-step
    lib = _lib.load()
    q = ctypes.c_void_p(1 << 12)
    assert lib.ltxk_quant_rows_mxfp4(q, 96, q, 48, q, 3, 4, 96 + 16, None) == -1     # K % 32, refused before any launch
    assert lib.ltxk_quant_rows_mxfp4(q, 96, q, 40, q, 3, 4, 96, None) == -1          # ldq below K / 2


def _integer_rule(x):
    """The quantiser kernel's arithmetic (the header of csrc/quant_mxfp4.hip), transcribed: integer operations on the bf16 bit
    patterns only.  x (M, K) bf16 -> (codes, scale bytes)."""
    h = x.view(torch.int16).to(torch.int64) & 0xFFFF
    M, K = h.shape
    mag = h & 0x7FFF
    amax = mag.view(M, K // 32, 32).amax(dim=2)
    E = torch.where(amax == 0, torch.full_like(amax, 127), ((amax >> 7) - 2).clamp_min(0))
    Ee = E.repeat_interleave(32, dim=1)
    sub = (mag.to(torch.float32).view(torch.int32).to(torch.int64) >> 16) - (6 << 7)      # pattern(float(mag)) - (6 << 7)
    P = torch.where(mag >= 0x80, mag + (127 << 7), sub)
    xb = P - (Ee << 7)
    idx = sum(((xb >= m) if up else (xb > m)).to(torch.int64)
              for m, up in ((0x3E80, 0), (0x3F40, 1), (0x3FA0, 0), (0x3FE0, 1), (0x4020, 0), (0x4060, 1), (0x40A0, 0)))
    code = idx | ((h >> 12) & 8)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).to(U8), E.to(U8)


def test_quantiser_integer_rule_equals_quantize_mxfp4_on_every_finite_bf16():
    """Every finite bf16 pattern as an element, in blocks of like magnitude (sorted: the pattern lands in every position of its
    binade relative to the block's scale) and in blocks of mixed magnitude (shuffled: far below its block's scale)."""
    from mlx_video_amd.weights import quantize_mxfp4
    pats = torch.arange(65536, dtype=torch.int32)
    pats = pats[(pats & 0x7F80) != 0x7F80]                             # no Inf / NaN
    n = len(pats) // 256 * 256
    g = torch.Generator().manual_seed(0)
    for trial in range(6):
        if trial % 2 == 0:
            order = torch.argsort((pats & 0x7FFF) * 4 + torch.randint(0, 4, (len(pats),), generator=g, dtype=torch.int32))
        else:
            order = torch.randperm(len(pats), generator=g)
        x = pats[order][trial:trial + n - 256].to(torch.int16).view(-1, 256).view(BF)
        c, s = quantize_mxfp4(x)
        c2, s2 = _integer_rule(x)
        assert torch.equal(s, s2), f"trial {trial}: scale bytes differ at {(s != s2).nonzero()[0].tolist()}"
        assert torch.equal(c, c2), f"trial {trial}: code bytes differ at {(c != c2).nonzero()[0].tolist()}"
