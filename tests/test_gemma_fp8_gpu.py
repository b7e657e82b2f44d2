"""FP8 Gemma-3 panels on the device: ltxk_embed_rows_fp8, ``GemmaEncoder(fp8=)``, KV-cached decoding on ltxk_gemv_w8, and
``generate_video(fp8_text_encoder=True)``.

The model is tests/ref_gemma.py's tiny one (hidden 512, 6 layers, 4 / 2 heads of 256, vocabulary 512; B = 2, T = 96, row 1
left-padded by 59) with sliding_window 1024 and 16.  What fp8 storage costs is NOT what is tested - that is a property of
e4m3, recorded in DESIGN.md 5p - but that the device computes the model its panels stand for: the references run on ``Wd``,
the DEQUANTISED weights code * scale (exact in float64).  The yardstick is tests/test_gemma_model_gpu.py's: per hidden state
err(device, f64) <= 1.25 x err(bf16-policy restatement, f64), both restatements on ``Wd``, computed here.  Under "none" every
panel value is a bf16 value and the GEMMs are the bf16 ones bit for bit, so the states must EQUAL those of the bf16 encoder
built on the cast panels."""
import functools

import parity
import pytest
import torch

import ref_gemm
import ref_gemma as G
import ref_gemma_decode as D

pytestmark = pytest.mark.gpu
BF, F8, F64 = torch.bfloat16, torch.float8_e4m3fn, torch.float64
U = 2.0 ** -24


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _weights(scaling, seed=3):
    """(W: the bf16 stand-in weights, Q: the same with every matrix as e4m3 + ``_scale`` keys, Wd: what Q stands for, float64),
    all on the CPU; the tiny model's matrices do not depend on the window."""
    from mlx_video_amd.gemma import random_gemma_weights
    from mlx_video_amd.weights import SCALE_SUFFIX, quantize_fp8
    W = random_gemma_weights("cpu", G.tiny_config(1024), seed=seed)
    Q, Wd = {}, {}
    for k, v in W.items():
        if v.ndim == 2:
            w8, sc = quantize_fp8(v, scaling)
            Q[k] = w8
            if sc is not None:
                Q[k + SCALE_SUFFIX] = sc
            Wd[k] = w8.to(F64) * (sc.to(F64)[:, None] if sc is not None else 1.0)
        else:
            Q[k], Wd[k] = v, v
    return W, Q, Wd


def _to(dev, d):
    return {k: v.to(dev) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("D_", [16, 512])
def test_embed_rows_fp8(dev, D_):
    """"none": the bf16 kernel on the widened table, bit for bit.  With a row scale: every element within half a bf16 ulp of what
    was stored plus the two fp32 roundings in front of it of exact = code * row_scale * s.  Ids outside the table raise."""
    from mlx_video_amd import ops
    V, s = 37, 22.625
    g = torch.Generator().manual_seed(D_)
    codes = torch.randint(0, 256, (V, D_), generator=g, dtype=torch.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0x7e                     # no NaN codes
    codes[0, :16] = torch.tensor([0x00, 0x80, 0x01, 0x81, 0x7e, 0xfe, 0x08, 0x88] * 2, dtype=torch.uint8)      # +-0, subnormal, +-448, 2^-6
    table = codes.view(F8)
    ids = torch.tensor([0, V - 1, 5, 5, 36, 1, 0, 17, 2], dtype=torch.int32)
    rs = (torch.exp2(torch.linspace(-9, 3, V)) * (1 + 0.5 * torch.rand(V, generator=g))).float()
    fr = ref_gemm.rows_frame(ids.numel(), D_, D_ + 8, dev)
    got = ops.embed_rows(table.to(dev), ids.to(dev), s, out=fr.view, ids_host=ids)
    want = ops.embed_rows(table.to(BF).to(dev), ids.to(dev), s, ids_host=ids)
    torch.cuda.synchronize()
    assert fr.intact() and torch.equal(_bits(got), _bits(want)), "an unscaled fp8 table is not the bf16 kernel on the widened table"
    fr = ref_gemm.rows_frame(ids.numel(), D_, D_ + 8, dev)
    got = ops.embed_rows(table.to(dev), ids.to(dev), s, out=fr.view, ids_host=ids, row_scale=rs.to(dev)).cpu()
    assert fr.intact()
    exact = table.to(F64)[ids.long()] * rs.to(F64)[ids.long(), None] * s
    d, bnd = (got.to(F64) - exact).abs(), 0.5 * ref_gemm.ulp(got.to(F64)) + 2 * U * exact.abs()
    worst = ref_gemm.check(f"embed_rows_fp8 D{D_}", d, bnd)
    print(f"D {D_}: worst d / bound {worst:.3f}")
    for bad in (-1, V):
        with pytest.raises(ValueError, match="token ids"):
            ops.embed_rows(table.to(dev), torch.tensor([0, bad], dtype=torch.int32, device=dev), s, row_scale=rs.to(dev))


# -------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("window", [1024, 16])
def test_encoder_accuracy_on_dequantised_weights(dev, window):
    from mlx_video_amd.gemma import GemmaEncoder
    cfg = G.tiny_config(window)
    W, Q, Wd = _weights("channel")
    # e4m3 matrices with their scales, quantised on the CPU where the references' Wd comes from, taken as they are (torch's
    # division on the device may round a quotient the other way, so a panel quantised there can differ in a code)
    enc = GemmaEncoder(_to(dev, Q), cfg)
    assert enc.weight_dtype == F8 and enc.embed.dtype == F8 and enc.layers[0]["qkv"].dtype == F8 and enc.layers[0]["n_in"].dtype == BF
    ids, mask = G.tiny_inputs()
    got = enc(ids, mask)
    L = cfg.num_hidden_layers
    assert tuple(got.shape) == (L + 1, 2, 96, cfg.hidden_size) and bool(torch.isfinite(got.float()).all())
    f64, pol = G.forward(Wd, cfg, ids, mask, "f64"), G.forward(Wd, cfg, ids, mask, "bf16")
    rows = [(l, G.rel_l2_valid(pol[l], f64[l], mask), G.rel_l2_valid(got[l], f64[l], mask)) for l in range(L + 1)]
    for l, e_ref, e_dev in rows:
        print(f"window {window} state {l}: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    for l, e_ref, e_dev in rows:
        parity.auto(e_dev, 1.25 * e_ref, tag=f"state{l}")


def test_encoder_plain_cast_equals_bf16_encoder_on_cast_panels(dev):
    from mlx_video_amd.gemma import GemmaEncoder
    cfg = G.tiny_config(16)
    W, _, _ = _weights("none")
    enc8 = GemmaEncoder(_to(dev, W), cfg, fp8="none")
    assert enc8.embed_row_scale is None and enc8.layers[0]["qkv_s"] is None and enc8.weight_dtype == F8
    enc16 = GemmaEncoder(_to(dev, {k: (v.to(F8).to(BF) if v.ndim == 2 else v) for k, v in W.items()}), cfg)
    assert enc16.weight_dtype == BF
    ids, mask = G.tiny_inputs()
    assert torch.equal(_bits(enc8(ids, mask)), _bits(enc16(ids, mask)))
    assert enc8.weight_bytes() < 0.51 * enc16.weight_bytes()


def test_encoder_batch_invariance(dev):
    from mlx_video_amd.gemma import GemmaEncoder
    cfg = G.tiny_config(16)
    enc = GemmaEncoder(_to(dev, _weights("channel")[1]), cfg)
    ids, mask = G.tiny_inputs()
    both = enc(ids, mask)
    for b in range(2):
        one = enc(ids[b:b + 1], mask[b:b + 1])
        n = int(mask[b].sum())
        assert torch.equal(_bits(one[:, 0, 96 - n:]), _bits(both[:, b, 96 - n:])), f"row {b} alone gives other bits"
    swapped = enc(ids.flip(0), mask.flip(0))
    assert torch.equal(_bits(swapped.flip(1)), _bits(both))


# ------------------------------------------------------------------------------------------------------------- decoding
T_PRE, T_ALL = 72, 96


def _rel(a, b):
    a, b = G.f64(a), G.f64(b)
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def _decode_reference(window):
    """(f64, bf16-policy) states (L+1,B,24,D) and logits (B,24,V) of the decoded rows 72 .. 95 on Wd, teacher-forced; once."""
    cfg = G.tiny_config(window)
    Wd = _weights("channel")[2]
    ids, mask = G.tiny_inputs()
    out = []
    for policy in ("f64", "bf16"):
        cache, _, _ = D.prefill(Wd, cfg, ids[:, :T_PRE], mask[:, :T_PRE], policy, T_total=T_ALL)
        st, lg = [], []
        for t in range(T_PRE, T_ALL):
            s, l = D.step(Wd, cfg, cache, ids[:, t], policy, T_total=T_ALL)
            st.append(torch.stack(s))
            lg.append(l)
        out.append((torch.stack(st, 2), torch.stack(lg, 1)))
    return out


def _generator(dev, cfg, scaling="channel", seed=3):
    from mlx_video_amd.gemma import GemmaEncoder, GemmaGenerator
    enc = GemmaEncoder(_to(dev, _weights(scaling, seed)[1]), cfg)
    return enc, GemmaGenerator(enc)


@pytest.mark.parametrize("window", [1024, 16])
def test_prefill_and_teacher_forced_steps(dev, window):
    """Prefill: the fp8 encoder's states bit for bit.  24 teacher-forced steps on ltxk_gemv_w8: states and logits within 1.25 x the
    bf16-policy restatement's own error against float64, both on the dequantised weights.  And the kernel's row property at
    the model's level: the B = 2 steps give each row the bits two B = 1 generators give it."""
    from mlx_video_amd import ops
    cfg = G.tiny_config(window)
    enc, gen = _generator(dev, cfg)
    assert gen.gemv and all(gen.GEMV_SHAPES.values())
    ids, mask = G.tiny_inputs()
    cache, logits0, pre = gen.prefill(ids[:, :T_PRE], mask[:, :T_PRE], 128, return_states=True)
    assert torch.equal(_bits(pre), _bits(enc(ids[:, :T_PRE], mask[:, :T_PRE]))), "the prefill's states are not the encoder's"
    singles = [gen.prefill(ids[b:b + 1, :T_PRE], mask[b:b + 1, :T_PRE], 128)[0] for b in range(2)]
    L = cfg.num_hidden_layers
    st, lg = [], []
    ops.TIMER = ops.KernelTimer()
    for t in range(T_PRE, T_ALL):
        l, s = gen.step(cache, ids[:, t], return_states=True)
        for b in range(2):
            l1, s1 = gen.step(singles[b], ids[b:b + 1, t], return_states=True)
            assert torch.equal(_bits(s1[:, 0]), _bits(s[:, b])) and torch.equal(l1[0], l[b]), f"step {t}: row {b} alone gives other bits"
        st.append(s.cpu())
        lg.append(l.cpu())
    fams = ops.TIMER.summary()
    ops.TIMER = None
    assert "gemv_w8" in fams and "gemm_w8" not in fams and "gemm_bf16" not in fams, f"the steps' GEMMs ran as {sorted(fams)}"
    assert fams["gemv_w8"]["launches"] == 3 * (T_ALL - T_PRE) * (4 * L + 1)
    st, lg = torch.stack(st, 2), torch.stack(lg, 1)
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (2, T_ALL - T_PRE, cfg.vocab_size) and bool(torch.isfinite(lg).all())
    (f_st, f_lg), (p_st, p_lg) = _decode_reference(window)
    rows = [(f"state{l}", _rel(p_st[l], f_st[l]), _rel(st[l], f_st[l])) for l in range(L + 1)] + [("logits", _rel(p_lg, f_lg), _rel(lg, f_lg))]
    for name, e_ref, e_dev in rows:
        print(f"window {window} {name}: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    for name, e_ref, e_dev in rows:
        parity.auto(e_dev, 1.25 * e_ref, tag=name)


GREEDY_SEED = 4           # of the weights; picked on the CPU, where both restatements run (see test_greedy_generation)
N_GREEDY = 12
PENALTY = 100.0           # tests/test_gemma_decode_gpu.py::test_greedy_generation says why


def test_greedy_generation(dev):
    """12 tokens at temperature 0 against the float64 restatement's (on the dequantised weights), per batch row up to the first
    step whose f64 top-two gap is below 4 x the bf16-policy restatement's worst logit error at that step: before it the choice
    is decided beyond what bf16 arithmetic can move.  The seed was picked on the CPU (of seeds 1 .. 8: decided [1, 11] of the two
    rows' 12 steps; the others decide 4 or fewer) so that at least half of the 2 x 12 steps are decided and the bf16-policy
    restatement agrees on them; that is asserted, then the device is held to the same tokens."""
    cfg = G.tiny_config(1024)
    ids, mask = G.tiny_inputs()
    ids, mask = ids[:, :T_PRE], mask[:, :T_PRE]
    Wd = _weights("channel", GREEDY_SEED)[2]
    tf, lf, rf = D.greedy(Wd, cfg, ids, mask, N_GREEDY, "f64", penalty=PENALTY)
    tp, _, rp = D.greedy(Wd, cfg, ids, mask, N_GREEDY, "bf16", penalty=PENALTY)
    decided = []
    for b in range(2):
        n = 0
        for i in range(N_GREEDY):
            top = lf[b, i].topk(2).values
            if float(top[0] - top[1]) < 4.0 * float((rp[b, i] - rf[b, i]).abs().max()):
                break
            assert int(tp[b, i]) == int(tf[b, i]), "the bf16-policy restatement departs on a decided token"
            n += 1
        decided.append(n)
    print(f"decided tokens per row: {decided}; f64 tokens {tf.tolist()}")
    assert sum(decided) >= N_GREEDY, decided
    _, gen = _generator(dev, cfg, seed=GREEDY_SEED)
    got = gen.generate(ids, mask, max_tokens=N_GREEDY, temperature=0.0, repetition_penalty=PENALTY, eos_ids=())
    print(f"device tokens {got}")
    for b in range(2):
        assert got[b][:decided[b]] == tf[b, :decided[b]].tolist(), (b, got[b], tf[b].tolist())


# ------------------------------------------------------------------------------------------------------- generate_video
def test_generate_video_fp8_text_encoder(dev, tmp_path):
    """gemma_repo= a directory written here + fp8_text_encoder=True (with prompt enhancement on the same encoder) gives the
    latents of passing an fp8 GemmaEncoder built from that directory's weights as gemma=; the encoder it builds holds at most
    0.51 of the bf16 encoder's bytes; a bf16 gemma= with the flag is refused."""
    pytest.importorskip("tokenizers")
    from mlx_video_amd import generate as GV
    from mlx_video_amd.gemma import GemmaConfig, GemmaEncoder, random_gemma_weights
    from mlx_video_amd.generate import PipelineType, generate_video
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    from mlx_video_amd.weights import gemma_weights
    from test_gemma_model_gpu import _write_gemma_dir
    from test_pipeline_gpu import _mods, _Noise
    m = _mods(dev)
    # test_generate_video_text_route's 2-layer model with a feed-forward wide enough that the per-row scales and the bf16 norm
    # weights are the small share of the bytes they are at the real size (intermediate 64: 0.5115 of the bf16 bytes; 1024: 0.507)
    cfg = GemmaConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1, head_dim=256,
                      intermediate_size=1024, vocab_size=64, sliding_window=8, sliding_window_pattern=2, query_pre_attn_scalar=256.0,
                      rope_scaling_factor=8.0)
    root = tmp_path / "gemma"
    _write_gemma_dir(root, cfg, random_gemma_weights("cpu", cfg, seed=9), with_tokenizer=True)
    conn = TextConnector(random_connector_weights(dev, D=256, L=cfg.num_hidden_layers + 1, layers=1, R=16))
    common = dict(prompt="w5 w9 w11", pipeline=PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
                  transformer=m["transformer"], vae_decoder=m["vae_decoder"], compile_step=True, cfg_batch=True, device=dev,
                  return_latents=True, text_connector=conn, enhance_prompt=True, max_tokens=6, temperature=0.0, tokenizer_path=str(root))
    built = []
    real = GV._encode_gemma

    def spy(gemma, *a, **kw):
        built.append(gemma)
        return real(gemma, *a, **kw)

    GV._encode_gemma = spy
    try:
        a = generate_video(gemma_repo=str(root), fp8_text_encoder=True, noise_fn=_Noise(7, dev), **common)
    finally:
        GV._encode_gemma = real
    enc8 = GemmaEncoder(gemma_weights(root, dev, fp8="channel"), GemmaConfig.from_json(root))
    enc16 = GemmaEncoder(gemma_weights(root, dev), GemmaConfig.from_json(root))
    assert len(built) == 1 and built[0].weight_dtype == F8, "the encoder generate_video built (and enhanced the prompt on) is not an fp8 one"
    assert built[0].weight_bytes() == enc8.weight_bytes() <= 0.51 * enc16.weight_bytes()
    b = generate_video(gemma=enc8, noise_fn=_Noise(7, dev), **common)
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    c = generate_video(gemma=enc8, fp8_text_encoder=True, noise_fn=_Noise(7, dev), **common)       # an fp8 gemma= is taken as it is
    assert torch.equal(a, c)
    with pytest.raises(ValueError, match="drop"):
        generate_video(gemma=enc16, fp8_text_encoder=True, noise_fn=_Noise(7, dev), **common)
