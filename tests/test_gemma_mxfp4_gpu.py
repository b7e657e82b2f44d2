"""Gemma-3 decoding on OCP MXFP4 panels (``GemmaGenerator(decode_panels="mxfp4")``, ltxk_gemv_w4) and
``generate_video(enhance_mxfp4=True)``.

The model is tests/ref_gemma.py's tiny one (hidden 512, 6 layers, 4 / 2 heads of 256, vocabulary 512; B = 2, T = 96, row 1
left-padded by 59) with sliding_window 1024 and 16, on a bf16 encoder and on an fp8 "channel" one.  What 4-bit storage costs is
NOT what is tested - that is a property of e2m1, recorded in DESIGN.md 5r - but that the device computes the model its panels
stand for.  The yardstick is tests/test_gemma_fp8_gpu.py's, on two weight sets, both through ref_gemma_decode's public
functions: the 72-position prefill runs on ``Wd_enc``, the encoder's weights (bf16 values, or e4m3 code * scale), and the 24
teacher-forced steps on ``Wd_dec``, the generator's OWN MXFP4 codes read back and dequantised (exact in float64), with the
embedding table left at the encoder's, since the gather stays on it.  The steps' logits are the tied head on the MXFP4 table:
``r(norm(h_L) @ table_dec^T)`` restated here in the same policy.  Per hidden state and for the logits:
err(device, f64) <= 1.25 x err(bf16-policy restatement, f64).

The tests route all five GEMMs to ltxk_gemv_w4 (a subclass whose ``GEMV4_SHAPES`` is all true), whatever the shipped table says
for the full-size model; one teacher-forced case and the CLI test run the shipped table, where the unrouted shapes stay on the
encoder's panel and the reference keeps the encoder's weights for them."""
import parity
import pytest
import torch

import ref_gemma as G
import ref_gemma_decode as D
from test_gemma_fp8_gpu import T_ALL, T_PRE, _bits, _rel, _to, _weights

pytestmark = pytest.mark.gpu
BF, F8, F64 = torch.bfloat16, torch.float8_e4m3fn, torch.float64
ALL = {"qkv": True, "o": True, "gu": True, "down": True, "logits": True}
CASES = [("bf16", 1024), ("bf16", 16), ("fp8", 1024), ("fp8", 16)]


def _encoder(dev, kind, window, seed=3):
    """(encoder, Wd_enc): a bf16 encoder on the stand-in weights, or an fp8 one on their CPU-quantised e4m3 form."""
    from mlx_video_amd.gemma import GemmaEncoder
    W, Q, Wd = _weights("channel", seed)
    cfg = G.tiny_config(window)
    if kind == "bf16":
        return GemmaEncoder(_to(dev, W), cfg), W
    return GemmaEncoder(_to(dev, Q), cfg), Wd


def _all_w4():
    from mlx_video_amd.gemma import GemmaGenerator

    class AllW4(GemmaGenerator):
        GEMV4_SHAPES = dict(ALL)

    return AllW4


def _generator(dev, kind, window, seed=3, shipped=False):
    """``shipped``: the generator as users build it, on ``GemmaGenerator.GEMV4_SHAPES``; else every shape on ltxk_gemv_w4."""
    from mlx_video_amd.gemma import GemmaGenerator
    enc, Wd_enc = _encoder(dev, kind, window, seed)
    gen = (GemmaGenerator if shipped else _all_w4())(enc, decode_panels="mxfp4")
    return enc, gen, Wd_enc


def _decode_weights(gen, Wd_enc):
    """(Wd_dec, table_dec): Wd_enc with every projection that is routed to an MXFP4 pair replaced by what the pair stands for,
    float64; an unrouted one (and an unrouted table) stays the encoder's."""
    from mlx_video_amd.weights import dequantize_mxfp4
    c = gen.cfg
    nq, nkv, F = c.num_attention_heads * 256, c.num_key_value_heads * 256, c.intermediate_size
    Wd = dict(Wd_enc)
    deq = lambda pair: dequantize_mxfp4(pair[0].cpu(), pair[1].cpu(), F64)          # noqa: E731
    for i, p4 in enumerate(gen.panels4):
        p = f"layers.{i}."
        if "qkv" in p4:
            qkv = deq(p4["qkv"])
            Wd[p + "self_attn.q_proj.weight"], Wd[p + "self_attn.k_proj.weight"], Wd[p + "self_attn.v_proj.weight"] = qkv[:nq], qkv[nq:nq + nkv], qkv[nq + nkv:]
        if "gu" in p4:
            gu = deq(p4["gu"])
            Wd[p + "mlp.gate_proj.weight"], Wd[p + "mlp.up_proj.weight"] = gu[:F], gu[F:]
        for n, key in (("o", "self_attn.o_proj.weight"), ("down", "mlp.down_proj.weight")):
            if n in p4:
                Wd[p + key] = deq(p4[n])
    return Wd, (deq(gen.table4) if gen.table4 is not None else G.f64(Wd_enc["embed_tokens.weight"]))


def _reference(Wd_enc, Wd_dec, table_dec, window):
    """(f64, bf16-policy) states (L+1,B,24,D) and logits (B,24,V) of the decoded rows 72 .. 95, teacher-forced: the prefill on
    Wd_enc, the steps on Wd_dec, the steps' logits on table_dec."""
    cfg = G.tiny_config(window)
    ids, mask = G.tiny_inputs()
    out = []
    for policy in ("f64", "bf16"):
        r = G.rbf if policy == "bf16" else (lambda t: t)
        cache, _, _ = D.prefill(Wd_enc, cfg, ids[:, :T_PRE], mask[:, :T_PRE], policy, T_total=T_ALL)
        st, lg = [], []
        for t in range(T_PRE, T_ALL):
            s, _ = D.step(Wd_dec, cfg, cache, ids[:, t], policy, T_total=T_ALL)
            st.append(torch.stack(s))
            lg.append(r(G.f64(s[-1]) @ table_dec.T))
        out.append((torch.stack(st, 2), torch.stack(lg, 1)))
    return out


@pytest.mark.parametrize("kind,window,shipped", [c + (False,) for c in CASES] + [("fp8", 16, True), ("bf16", 1024, True)], ids=lambda v: str(v))
def test_teacher_forced_steps_on_mxfp4_panels(dev, kind, window, shipped):
    """``shipped``: on the routing table users get (the other shapes on the encoder's panel: ltxk_gemv_w8 on an fp8 encoder, the
    split-K bf16 GEMM on a bf16 one, where a row's bits may depend on the batch and are not compared); else all five GEMMs on
    ltxk_gemv_w4.  Prefill: the encoder's states bit for bit (it stays on the encoder's panels).  24 teacher-forced steps with all five GEMMs
    on ltxk_gemv_w4: states and logits within 1.25 x the bf16-policy restatement's own error against float64.  And the kernel's
    row property at the model's level: the B = 2 steps give each row the bits two B = 1 caches give it."""
    from mlx_video_amd import ops
    enc, gen, Wd_enc = _generator(dev, kind, window, shipped=shipped)
    cfg, L = gen.cfg, gen.cfg.num_hidden_layers
    on = [n for n, v in gen.routing4.items() if v]
    assert set(on) == set(ALL) or shipped
    rows_alone = not shipped or kind == "fp8"
    before = enc.weight_bytes()
    ids, mask = G.tiny_inputs()
    cache, _, pre = gen.prefill(ids[:, :T_PRE], mask[:, :T_PRE], 128, return_states=True)
    assert torch.equal(_bits(pre), _bits(enc(ids[:, :T_PRE], mask[:, :T_PRE]))), "the prefill's states are not the encoder's"
    singles = [gen.prefill(ids[b:b + 1, :T_PRE], mask[b:b + 1, :T_PRE], 128)[0] for b in range(2)]
    st, lg = [], []
    ops.TIMER = ops.KernelTimer()
    for t in range(T_PRE, T_ALL):
        l, s = gen.step(cache, ids[:, t], return_states=True)
        for b in range(2):
            l1, s1 = gen.step(singles[b], ids[b:b + 1, t], return_states=True)
            assert not rows_alone or (torch.equal(_bits(s1[:, 0]), _bits(s[:, b])) and torch.equal(l1[0], l[b])), f"step {t}: row {b} alone gives other bits"
        st.append(s.cpu())
        lg.append(l.cpu())
    fams = ops.TIMER.summary()
    ops.TIMER = None
    other = {"gemv_w8", "gemm_w8", "gemm_bf16"} & set(fams)
    assert other == (set() if len(on) == 5 else {"gemv_w8"} if kind == "fp8" else {"gemm_bf16"}), f"the steps' GEMMs ran as {sorted(fams)}"
    per_step = L * sum(n != "logits" for n in on) + ("logits" in on)
    assert fams["gemv_w4"]["launches"] == 3 * (T_ALL - T_PRE) * per_step
    if other == {"gemv_w8"}:
        assert fams["gemv_w8"]["launches"] == 3 * (T_ALL - T_PRE) * (4 * L + 1 - per_step)
    assert enc.weight_bytes() == before
    st, lg = torch.stack(st, 2), torch.stack(lg, 1)
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (2, T_ALL - T_PRE, cfg.vocab_size) and bool(torch.isfinite(lg).all())
    Wd_dec, table_dec = _decode_weights(gen, Wd_enc)
    (f_st, f_lg), (p_st, p_lg) = _reference(Wd_enc, Wd_dec, table_dec, window)
    rows = [(f"state{l}", _rel(p_st[l], f_st[l]), _rel(st[l], f_st[l])) for l in range(L + 1)] + [("logits", _rel(p_lg, f_lg), _rel(lg, f_lg))]
    for name, e_ref, e_dev in rows:
        print(f"{kind} window {window} shipped {shipped} {name}: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    for name, e_ref, e_dev in rows:
        parity.auto(e_dev, 1.25 * e_ref, tag=name)


N_STEPS = 8


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_device_step_logits_equal_step(dev, kind):
    """The logits ``device_step`` leaves on MXFP4 panels - run eagerly, and recorded once and replayed - equal ``step()``'s bit for
    bit at every step, and so do the caches at the end."""
    from mlx_video_amd.gemma import GemmaDecodeState
    _, gen, _ = _generator(dev, kind, 16)
    ids, mask = G.tiny_inputs()
    ids, mask = ids[:, :T_PRE], mask[:, :T_PRE]
    feed = torch.randint(1, 512, (N_STEPS, 2), generator=torch.Generator().manual_seed(16))
    cache, _ = gen.prefill(ids, mask, 128)
    want = [gen.step(cache, feed[i]).cpu() for i in range(N_STEPS)]
    for graph in (False, True):
        c2, _ = gen.prefill(ids, mask, 128)
        st = GemmaDecodeState(gen.cfg, gen.enc.vocab, ids, mask, N_STEPS, (), 0, dev)
        g = None
        for i in range(N_STEPS):
            st.next_ids.copy_(feed[i].to(torch.int32))
            if g is None or not graph:
                gen.device_step(c2, st, draw=False)
                if graph and i == 0:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        gen.device_step(c2, st, draw=False)
            else:
                g.replay()
            got = st.logits.float().cpu()
            assert torch.equal(got.view(torch.int32), want[i].view(torch.int32)), (graph, i)
        for l in range(gen.cfg.num_hidden_layers):
            assert torch.equal(_bits(c2.k[l].cpu()), _bits(cache.k[l].cpu())) and torch.equal(_bits(c2.vt[l].cpu()), _bits(cache.vt[l].cpu())), (graph, l)


def test_generate_device_loop_equals_host_loop_at_temperature_zero(dev):
    _, gen, _ = _generator(dev, "fp8", 1024)
    ids, mask = G.tiny_inputs()
    ids, mask = ids[:, :T_PRE], mask[:, :T_PRE]
    kw = dict(max_tokens=12, temperature=0.0, repetition_penalty=100.0, eos_ids=())
    host = gen.generate(ids, mask, **kw)
    assert [len(h) for h in host] == [12, 12]
    for graph in (True, False):
        assert gen.generate(ids, mask, device_loop=True, graph=graph, **kw) == host, graph


def test_decode_panels_none_is_the_generator_it_was(dev):
    """``decode_panels=None`` leaves ``step()``'s logits bit-identical to a generator built without the argument; the MXFP4
    generator's differ (its GEMMs run on other weights), and its streamed bytes are below 0.30 of the bf16 generator's."""
    from mlx_video_amd.gemma import GemmaGenerator
    enc, gen4, _ = _generator(dev, "bf16", 16)
    ids, mask = G.tiny_inputs()
    ids, mask = ids[:, :T_PRE], mask[:, :T_PRE]
    outs = []
    for gen in (GemmaGenerator(enc), GemmaGenerator(enc, decode_panels=None), gen4):
        cache, _ = gen.prefill(ids, mask, 128)
        outs.append(torch.stack([gen.step(cache, torch.tensor([7 + i, 9 + i])) for i in range(3)]).cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert not torch.equal(outs[0], outs[2]) and bool(torch.isfinite(outs[2]).all())
    plain = GemmaGenerator(enc)
    assert plain.panels4 is None and plain.decode_weight_bytes() == enc.weight_bytes() + 2 * enc.cfg.hidden_size          # + a gathered row
    assert gen4.decode_weight_bytes() < 0.30 * plain.decode_weight_bytes() and gen4.decode_weight_bytes() < 0.30 * enc.weight_bytes()


def test_generate_video_enhance_mxfp4(dev, tmp_path, monkeypatch):
    """generate_video(enhance_prompt=True, enhance_mxfp4=True) enhances on an MXFP4 generator - with and without the fp8 text
    encoder and the device loop - and returns finite latents; the text encoder it builds is the one it builds without the option."""
    pytest.importorskip("tokenizers")
    from mlx_video_amd import gemma as GM
    from mlx_video_amd import generate as GV
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    from test_gemma_decode_gpu import _gemma_dir
    from test_pipeline_gpu import _mods, _Noise
    m = _mods(dev)
    root = tmp_path / "gemma"
    cfg = _gemma_dir(root, 256, seed=9)
    conn = TextConnector(random_connector_weights(dev, D=256, L=cfg.num_hidden_layers + 1, layers=1, R=16))
    built = []
    real = GM.GemmaGenerator.__init__

    def spy(self, encoder, *a, **kw):
        real(self, encoder, *a, **kw)
        built.append((self.decode_panels, encoder.weight_dtype))

    monkeypatch.setattr(GM.GemmaGenerator, "__init__", spy)
    monkeypatch.setattr(GM.GemmaGenerator, "GEMV4_SHAPES", dict(ALL))
    common = dict(pipeline=GV.PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
                  transformer=m["transformer"], vae_decoder=m["vae_decoder"], compile_step=True, cfg_batch=True, device=dev,
                  return_latents=True, gemma_repo=str(root), text_connector=conn, negative_prompt="w9", prompt="w4 w5",
                  enhance_prompt=True, max_tokens=8, temperature=0.0)
    a = GV.generate_video(noise_fn=_Noise(7, dev), enhance_mxfp4=True, **common)
    b = GV.generate_video(noise_fn=_Noise(7, dev), enhance_mxfp4=True, enhance_device_loop=True, **common)
    c = GV.generate_video(noise_fn=_Noise(7, dev), enhance_mxfp4=True, fp8_text_encoder=True, **common)
    GV.generate_video(noise_fn=_Noise(7, dev), **common)
    assert built == [("mxfp4", BF), ("mxfp4", BF), ("mxfp4", F8), (None, BF)]
    for lat in (a, b, c):
        assert bool(torch.isfinite(lat.float()).all())
    assert torch.equal(a, b), "the device loop at temperature 0 gives another rewrite than the host loop"
    with pytest.raises(ValueError, match="enhance_mxfp4"):
        GV.generate_video(noise_fn=_Noise(7, dev), **dict(common, enhance_prompt=False, enhance_mxfp4=True))


def test_cli_enhance_mxfp4(dev, tmp_path):
    """`generate --synthetic --gemma-repo DIR --enhance-prompt --enhance-mxfp4 [--fp8-text-encoder --enhance-device-loop]` on a
    directory written here (a 2-layer Gemma of the real width, the routing as measured) writes a video of the right shape."""
    pytest.importorskip("tokenizers")
    import numpy as np
    from mlx_video_amd import generate as GV
    from test_gemma_decode_gpu import _gemma_dir
    root = tmp_path / "gemma"
    _gemma_dir(root, 3840, seed=4)
    for i, more in enumerate(([], ["--fp8-text-encoder", "--enhance-device-loop"])):
        out = tmp_path / f"enh{i}.npy"
        GV.main(["--synthetic", "--layers", "1", "--pipeline", "distilled", "--height", "128", "--width", "128", "--num-frames", "9",
                 "--stage1-steps", "1", "--stage2-steps", "1", "--tiling", "none", "--gemma-repo", str(root), "--prompt", "w4 w5",
                 "--negative-prompt", "w6", "--enhance-prompt", "--enhance-mxfp4", "--max-tokens", "8", "--temperature", "0",
                 "--output-path", str(out)] + more)
        frames = np.load(out)
        assert frames.shape == (9, 128, 128, 3) and frames.dtype == np.uint8
