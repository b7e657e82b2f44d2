"""OCP MXFP4 decode panels, the parts that need no GPU: ``weights.quantize_mxfp4`` / ``dequantize_mxfp4`` against the format's
rule, the float64 bound of tests/ref_gemm.py against an fp32 emulation of ltxk_gemv_w4's stated order (faithful: inside; planted
faults: outside), the C entry and its host-side refusals, ``ops.gemv_w4``'s refusals on CPU tensors, and the public option.

Reference of the bound: float64 on the DEQUANTISED panel e2m1(code) * 2^(E-127), which is exact (a 2-bit significand times a
power of two).  Bound: ``ref_gemm.bound(EPI_BIAS, out, s, mag, K, bias, acc_err=K * U * mag)`` - K fp32 roundings of the
accumulation in any order (the products themselves are exact in fp32: 8 x 2 significand bits), the fp32 bias add, half a bf16
ulp of what was stored."""
import ctypes
import inspect

import pytest
import torch

import ref_gemm

BF, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
U = ref_gemm.U
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _q():
    from mlx_video_amd import weights
    return weights.quantize_mxfp4, weights.dequantize_mxfp4, weights.MXFP4_BLOCK


# ---------------------------------------------------------------------------------------------------------- the quantiser
def _rule_scale_byte(amax: float) -> int:
    """The OCP rule on one block's amax, restated with Python floats (math.frexp reads the exponent field)."""
    import math
    if amax == 0:
        return 127
    return max(-127, min(127, math.frexp(amax)[1] - 1 - 2)) + 127


def test_every_block_within_a_quarter_of_its_amax_and_the_scale_byte_is_the_rules():
    quantize, dequantize, BLK = _q()
    assert BLK == 32
    g = torch.Generator().manual_seed(1)
    N, K = 96, 256
    expo = torch.randint(-20, 11, (N, K // 32), generator=g).float()                # block amax spread over 2^-20 .. 2^10
    w = torch.randn((N, K), generator=g) * torch.exp2(expo).repeat_interleave(32, 1)
    for m in (w, w.to(BF)):
        codes, sc = quantize(m)
        assert codes.dtype == U8 and tuple(codes.shape) == (N, K // 2) and sc.dtype == U8 and tuple(sc.shape) == (N, K // 32)
        assert codes.is_contiguous() and sc.is_contiguous() and int(sc.max()) < 255
        m64 = m.to(F64)
        amax = m64.view(N, K // 32, 32).abs().amax(2)
        err = (dequantize(codes, sc, F64) - m64).abs().view(N, K // 32, 32).amax(2)
        assert bool((err <= amax / 4).all()), float((err / amax).max())
        want = torch.tensor([[_rule_scale_byte(float(v)) for v in row] for row in amax], dtype=U8)
        assert torch.equal(sc, want)
        # exact in fp32: the fp32 and the float64 dequantisation agree bit for bit
        assert torch.equal(dequantize(codes, sc, F32).to(F64), dequantize(codes, sc, F64))
    print(f"worst |w - dequantised| / amax_block: {float((err / amax).max()):.4f}")


def test_known_answers():
    quantize, dequantize, _ = _q()
    vals = torch.tensor([v for v in E2M1] + [-v for v in E2M1] + [v for v in E2M1] + [-v for v in E2M1]).view(1, 32)
    codes, sc = quantize(vals)
    assert sc.tolist() == [[127]]                                      # amax 6: floor(log2 6) - 2 = 0
    nib = torch.stack([codes & 0xF, codes >> 4], 2).view(-1).tolist()
    assert nib == (list(range(8)) + list(range(8, 16))) * 2            # the 16 codes, sign bit 8: -0 is code 8
    back = dequantize(codes, sc)
    assert torch.equal(back, vals) and torch.equal(torch.signbit(back), torch.signbit(vals)), "-0 lost its sign"
    # ties go to the even 3-bit index; 6 keeps the block's scale at 1
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0] * 4).view(1, 32)
    codes, sc = quantize(torch.cat([ties, -ties]))
    assert sc.tolist() == [[127], [127]]
    want = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0] * 4)
    assert torch.equal(dequantize(codes, sc), torch.stack([want, -want]))
    # saturation: amax 7 has floor(log2) = 2, scale 1, and 7 clamps to 6; an element 100 x the rest leaves them at 0
    sat = torch.full((1, 32), 0.01)
    sat[0, 3], sat[0, 4] = 7.0, -7.9
    codes, sc = quantize(sat)
    d = dequantize(codes, sc)
    assert sc.tolist() == [[127]] and float(d[0, 3]) == 6.0 and float(d[0, 4]) == -6.0 and float(d[0, 0]) == 0.0
    out = torch.ones((1, 64)) * 0.3
    out[0, 40] = 30.0                                                   # 100 x its block: floor(log2 30) = 4, scale 4, 30 / 4 = 7.5 -> 6
    codes, sc = quantize(out)
    d = dequantize(codes, sc)
    assert sc.tolist() == [[123, 129]] and float(d[0, 40]) == 24.0 and float(d[0, 33]) == 0.0 and float(d[0, 0]) == 0.25
    # a zero block: byte 127, zero codes, signs kept
    z = torch.zeros((2, 32))
    z[1, 5] = -0.0
    codes, sc = quantize(z)
    assert sc.tolist() == [[127], [127]] and int(codes[0].max()) == 0 and codes[1].tolist() == [0, 0, 0x80] + [0] * 13
    # the extremes of fp32 stay inside the byte range 0 .. 254
    ext = torch.zeros((2, 32))
    ext[0, 0], ext[1, 0] = 3e38, 2.0 ** -149
    codes, sc = quantize(ext)
    assert sc.tolist() == [[127 + 125], [0]] and float(dequantize(codes, sc, F64)[0, 0]) == 1.5 * 2.0 ** 127


def test_refusals_of_the_quantiser():
    quantize, dequantize, _ = _q()
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = torch.zeros((2, 32))
        w[1, 7] = bad
        with pytest.raises(ValueError, match="NaN or Inf"):
            quantize(w)
    for shape in ((2, 48), (2, 16), (32,), (1, 2, 32), (2, 0)):
        with pytest.raises(ValueError, match="multiple of 32"):
            quantize(torch.zeros(shape))
    with pytest.raises(ValueError, match="pair"):
        dequantize(torch.zeros((2, 16), dtype=U8), torch.zeros((2, 2), dtype=U8))


def test_nibble_order_is_float4_e2m1fn_x2s():
    """torch documents float4_e2m1fn_x2 as two e2m1 values per byte with the FIRST element in bits 0 .. 3.  A block whose even
    elements are 0.5 and odd elements are -6 therefore packs to bytes 0xF1; the dtype view is accepted by the dequantiser."""
    quantize, dequantize, _ = _q()
    w = torch.tensor([0.5, -6.0] * 16).view(1, 32)
    codes, sc = quantize(w)
    assert codes.tolist() == [[0xF1] * 16]
    assert hasattr(torch, "float4_e2m1fn_x2")
    view = codes.view(torch.float4_e2m1fn_x2)
    assert view.dtype == torch.float4_e2m1fn_x2 and tuple(view.shape) == (1, 16)
    assert torch.equal(dequantize(view, sc), w)


# ------------------------------------------------------------------------------------------- the bound and the kernel's order
def emulate(a, codes, sc, bias, fault=None):
    """ltxk_gemv_w4's stated order in fp32 (csrc/gemv4.hip): lane l of pass p holds k = 2048 p + 32 l .. + 31; per lane one
    fp32 product-and-add per k into an even-k and an odd-k accumulator, ascending k over the passes; even + odd; the butterfly
    (32, 16, 8, 4, 2, 1); + bias; bf16.  Unfused: a bf16 times an e2m1 * 2^e is exact in fp32, so the FMA rounds as the add does.
    Lanes past K in the ragged last pass add zeros (x + 0 = x).  Faults: "tail" the last 32 k dropped; "nibbles" the two codes of
    every byte swapped; "scale" every block read with the next block's scale."""
    _, dequantize, _ = _q()
    if fault == "nibbles":
        codes = ((codes << 4) | (codes >> 4)).to(U8)
    if fault == "scale":
        sc = sc.roll(-1, 1)
    w = dequantize(codes, sc, F32)
    M, K = a.shape
    N = w.shape[0]
    af = a.to(F32).clone()
    if fault == "tail":
        af[:, K - 32:] = 0
    P = -(-K // 2048)
    ap, wp = torch.zeros((M, P * 2048), dtype=F32), torch.zeros((N, P * 2048), dtype=F32)
    ap[:, :K], wp[:, :K] = af, w
    ap, wp = ap.view(M, 1, P, 64, 16, 2), wp.view(1, N, P, 64, 16, 2)
    acc = torch.zeros((M, N, 64, 2), dtype=F32)
    for p in range(P):
        for i in range(16):
            acc = acc + ap[:, :, p, :, i] * wp[:, :, p, :, i]
    v = acc[..., 0] + acc[..., 1]
    lanes = torch.arange(64)
    for k in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ k]
    out = v[..., 0]
    if bias is not None:
        out = out + bias.to(F32)
    return out.to(BF)


EMU_CASES = [(1, 7, 32), (3, 257, 2080), (2, 8, 3840), (8, 37, 4096)]


def panel(M, N, K, seed):
    """ref_gemm.inputs with its panel quantised: (inp, codes, block_scales, s, mag) - s, mag on the dequantised panel, float64."""
    quantize, dequantize, _ = _q()
    inp = ref_gemm.inputs(M, N, K, seed)
    codes, sc = quantize(inp.w)
    s, mag = ref_gemm.product(inp.a, dequantize(codes, sc, F64))
    assert bool(torch.isfinite(s).all())
    return inp, codes, sc, s, mag


@pytest.mark.parametrize("M,N,K", EMU_CASES, ids=lambda v: str(v))
def test_bound_accepts_the_stated_order_and_refuses_planted_faults(M, N, K):
    inp, codes, sc, s, mag = panel(M, N, K, 300 + K + N)
    for bias in (inp.b, None):
        d, bnd = ref_gemm.bound(ref_gemm.EPI_BIAS, emulate(inp.a, codes, sc, bias), s, mag, K, bias, acc_err=K * U * mag)
        worst = ref_gemm.check(f"emulation M{M} N{N} K{K}", d, bnd)
        print(f"M{M} N{N} K{K} bias {bias is not None}: worst d / bound {worst:.3f}")
    # K = 32 is one block: there is no next block whose scale could be taken
    for fault in ("tail", "nibbles") + (("scale",) if K > 32 else ()):
        d, bnd = ref_gemm.bound(ref_gemm.EPI_BIAS, emulate(inp.a, codes, sc, inp.b, fault), s, mag, K, inp.b, acc_err=K * U * mag)
        n = int(ref_gemm.beyond(d, bnd).sum())
        print(f"M{M} N{N} K{K} fault {fault}: {n} of {d.numel()} outputs beyond the bound")
        assert n >= 1, f"the bound accepts the fault {fault!r}"


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_exported_bound_and_in_the_header():
    from mlx_video_amd import _lib
    lib = _lib.load()
    assert "ltxk_gemv_w4" in _lib.SIGNATURES and hasattr(lib, "ltxk_gemv_w4") and lib.ltxk_gemv_w4.argtypes is not None
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "ltxk.h")).read()
    assert "int ltxk_gemv_w4(" in hdr and "#define LTXK_VERSION 412" in hdr
    assert lib.ltxk_abi_sizeof(0) == ctypes.sizeof(_lib.GemmArgs)          # ltxk_gemm_args is unchanged


def _args(M, N, K, /, **over):
    from mlx_video_amd._lib import GemmArgs
    a = GemmArgs()
    a.A = a.W = a.out = 1 << 12
    a.M, a.N, a.K, a.lda, a.ldo = M, N, K, K, N
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_entry_refuses_on_the_host():
    """Every argument outside the entry's contract is LTXK_EINVAL with a message that begins with the entry's name, before
    anything is launched (no device here)."""
    from mlx_video_amd import _lib
    lib = _lib.load()
    sc = ctypes.c_void_p(1 << 13)
    bad = [dict(M=0), dict(M=9), dict(N=0), dict(K=16), dict(K=48), dict(K=0), dict(epilogue=1), dict(epilogue=4, resid=1 << 12, ldr=64),
           dict(resid=1 << 12), dict(gate=1 << 12), dict(gate_row=1 << 12), dict(out2=1 << 12), dict(n_split=8),
           dict(out_tokens_per_batch=1), dict(sumsq=1 << 12), dict(workspace=1 << 12, workspace_bytes=1 << 20), dict(lda=16),
           dict(lda=36), dict(ldo=4), dict(A=0), dict(W=0), dict(out=0), dict(A=(1 << 12) + 8), dict(W=(1 << 12) + 8)]
    for over in bad:
        assert lib.ltxk_gemv_w4(ctypes.byref(_args(2, 8, 32, **over)), sc, None) == -1, over
        assert lib.ltxk_last_error().startswith(b"ltxk_gemv_w4"), over
    assert lib.ltxk_gemv_w4(None, sc, None) == -1 and lib.ltxk_last_error().startswith(b"ltxk_gemv_w4")
    for scales in (None, ctypes.c_void_p((1 << 13) + 2)):
        assert lib.ltxk_gemv_w4(ctypes.byref(_args(2, 8, 32)), scales, None) == -1
        assert lib.ltxk_last_error().startswith(b"ltxk_gemv_w4") and b"w_block_scales" in lib.ltxk_last_error()


# --------------------------------------------------------------------------------------------------------------- the shim
def test_shim_refusals_name_the_operand_before_the_device():
    from mlx_video_amd import _lib, ops
    z = lambda *shape, dtype=BF: torch.zeros(shape, dtype=dtype)          # noqa: E731
    assert ops.GEMV4_MAX_M == 8 and ops.MXFP4_BLOCK == 32
    a, codes, sc, b = z(2, 64), z(8, 32, dtype=U8), z(8, 2, dtype=U8), z(8)
    with pytest.raises(_lib.LtxkError, match="device tensor"):              # the call these are mutations of: only the device refuses
        ops.gemv_w4(a, codes, sc, b, out=z(2, 8))
    with pytest.raises(ValueError, match="1 to 8 rows"):
        ops.gemv_w4(z(9, 64), codes, sc)
    with pytest.raises(ValueError, match="K % 32"):
        ops.gemv_w4(z(2, 48), z(8, 24, dtype=U8), z(8, 1, dtype=U8))
    for wrong in (torch.zeros((8, 32), dtype=U8).view(torch.float8_e4m3fn), z(8, 32)):
        with pytest.raises(TypeError, match="codes must be"):
            ops.gemv_w4(a, wrong, sc)
    with pytest.raises(TypeError, match="a must be"):
        ops.gemv_w4(z(2, 64, dtype=F32), codes, sc)
    with pytest.raises(ValueError, match="codes must be"):
        ops.gemv_w4(a, z(8, 64, dtype=U8), sc)                              # (N, K) instead of (N, K/2)
    with pytest.raises(TypeError, match="block_scales must be"):
        ops.gemv_w4(a, codes, z(8, 2, dtype=F32))
    for shape in ((8, 1), (8, 4), (7, 2), (16,)):
        with pytest.raises(ValueError, match="block_scales must"):
            ops.gemv_w4(a, codes, z(*shape, dtype=U8))
    with pytest.raises(ValueError, match="bias must be"):
        ops.gemv_w4(a, codes, sc, z(7))
    with pytest.raises(ValueError, match="out must be"):
        ops.gemv_w4(a, codes, sc, out=z(2, 9))
    with pytest.raises(ValueError, match="out must be"):
        ops.gemv_w4(a, codes, sc, out=z(2, 16)[:, ::2])                      # a strided inner dimension
    with pytest.raises(ValueError, match="codes must be"):
        ops.gemv_w4(a, z(8, 64, dtype=U8)[:, :32], sc)                       # a row stride on the panel
    with pytest.raises(ValueError, match="a must be 16-byte aligned"):
        ops.gemv_w4(z(2, 72)[:, 4:68], codes, sc)
    with pytest.raises(ValueError, match="rows of `a`"):
        ops.gemv_w4(z(2, 68)[:, :64], codes, sc)
    with pytest.raises(_lib.LtxkError, match="device tensor"):              # a row stride of K + 8 and an out with a leading dimension are fine
        ops.gemv_w4(z(2, 72)[:, :64], codes, sc, out=z(2, 13)[:, :8])
    # ops.gemm is the call it was: gemv=True still wants an e4m3 panel
    with pytest.raises(TypeError, match="`w`"):
        ops.gemm(a, codes, None, gemv=True)


# -------------------------------------------------------------------------------------------------- the generator, the option
def test_generator_builds_mxfp4_panels_from_bf16_and_fp8_encoders():
    """On the CPU (no launch): the copy is the quantiser's on the encoder's panel - a bf16 panel as it is, an fp8 panel as code *
    row scale in fp32 - row chunking included; the encoder's bytes are untouched; decode_weight_bytes counts what is routed."""
    from mlx_video_amd.gemma import GemmaConfig, GemmaEncoder, GemmaGenerator, random_gemma_weights
    from mlx_video_amd.weights import dequantize_fp8, quantize_mxfp4
    cfg = GemmaConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, head_dim=256,
                      intermediate_size=96, vocab_size=40, sliding_window=8, sliding_window_pattern=2)
    W = random_gemma_weights("cpu", cfg, seed=11)

    class Chunked(GemmaGenerator):
        MXFP4_CHUNK_ROWS = 24          # several chunks per panel, a ragged last one: the copy must be the whole matrix's
        GEMV4_SHAPES = dict.fromkeys(GemmaGenerator.GEMV4_SHAPES, True)          # every shape gets a copy

    for fp8 in (None, "channel"):
        enc = GemmaEncoder(dict(W), cfg, **({"fp8": fp8} if fp8 else {}))
        before = enc.weight_bytes()
        plain = GemmaGenerator(enc)
        assert plain.decode_panels is None and plain.panels4 is None and plain.table4 is None
        gen = Chunked(enc, decode_panels="mxfp4")
        assert enc.weight_bytes() == before and len(gen.panels4) == 2
        for name in ("qkv", "o", "gu", "down"):
            src = enc.layers[1][name]
            wide = dequantize_fp8(src, enc.layers[1][name + "_s"]) if fp8 else src.float()
            codes, sc = quantize_mxfp4(wide)
            assert torch.equal(gen.panels4[1][name][0], codes) and torch.equal(gen.panels4[1][name][1], sc)
        assert tuple(gen.table4[0].shape) == (40, 32) and tuple(gen.table4[1].shape) == (40, 2)
        mats = sum(v.numel() for v in W.values() if v.ndim == 2)
        small = sum(v.numel() * 2 for v in W.values() if v.ndim == 1)
        row = 64 * (1 if fp8 else 2) + (4 if fp8 else 0)
        assert gen.decode_weight_bytes() == mats // 2 + mats // 32 + small + row
        # the shipped table: only the routed shapes are copied, the others stream the encoder's panel
        dflt = GemmaGenerator(enc, decode_panels="mxfp4")
        on = {n for n, v in GemmaGenerator.GEMV4_SHAPES.items() if v}
        assert dflt.routing4 == GemmaGenerator.GEMV4_SHAPES and all(set(p) == on - {"logits"} for p in dflt.panels4)
        assert (dflt.table4 is not None) == ("logits" in on)
        for name in on - {"logits"}:
            assert torch.equal(dflt.panels4[1][name][0], gen.panels4[1][name][0]) and torch.equal(dflt.panels4[1][name][1], gen.panels4[1][name][1])
        assert gen.decode_weight_bytes() <= dflt.decode_weight_bytes() < plain.decode_weight_bytes()
        assert gen.decode_weight_bytes(B=GemmaGenerator.GEMV4_MAX_B + 1) == plain.decode_weight_bytes() + GemmaGenerator.GEMV4_MAX_B * row
        rows = sum(v.shape[0] for v in W.values() if v.ndim == 2)
        assert plain.decode_weight_bytes() == (mats + 4 * rows if fp8 else 2 * mats) + small + row
    with pytest.raises(ValueError, match="decode_panels"):
        GemmaGenerator(enc, decode_panels="int4")
    odd = GemmaConfig(hidden_size=48, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1, head_dim=256,
                      intermediate_size=64, vocab_size=16, sliding_window=8, sliding_window_pattern=2)
    with pytest.raises(ValueError, match="multiple of 32"):
        GemmaGenerator(GemmaEncoder(random_gemma_weights("cpu", odd, seed=1), odd), decode_panels="mxfp4")


def test_cli_flag_and_refusals(monkeypatch):
    from mlx_video_amd import gemma
    from mlx_video_amd import generate as GV
    assert inspect.signature(GV.generate_video).parameters["enhance_mxfp4"].default is False
    assert inspect.signature(gemma.enhance_prompt).parameters["mxfp4"].default is False
    assert inspect.signature(gemma.GemmaGenerator.__init__).parameters["decode_panels"].default is None
    ap = GV.build_parser()
    assert ap.parse_args([]).enhance_mxfp4 is False and ap.parse_args(["--enhance-mxfp4"]).enhance_mxfp4 is True
    text = " ".join(ap.format_help().split())
    assert "--enhance-mxfp4" in text and "4-bit" in text and "opt-in" in text and "text encoding is unaffected" in text
    seen = {}
    monkeypatch.setattr(GV, "generate_video", lambda **kw: seen.update(kw))
    common = ["--prompt", "x", "--model-repo", "/nonexistent", "--gemma-repo", "/nonexistent-gemma"]
    GV.main(common + ["--enhance-prompt", "--enhance-mxfp4", "--fp8-text-encoder", "--enhance-device-loop"])          # it composes
    assert seen["enhance_mxfp4"] is True and seen["enhance_prompt"] is True and seen["fp8_text_encoder"] is True and seen["enhance_device_loop"] is True
    seen.clear()
    GV.main(common + ["--enhance-prompt"])                                   # off adds no keyword: the call it was
    assert "enhance_mxfp4" not in seen
    with pytest.raises(ValueError, match="--enhance-prompt"):
        GV.main(common + ["--enhance-mxfp4"])
    monkeypatch.undo()
    base = dict(prompt="x", transformer=object(), vae_decoder=object(), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="enhance_mxfp4.*enhance_prompt"):
        GV.generate_video(enhance_mxfp4=True, **base)
