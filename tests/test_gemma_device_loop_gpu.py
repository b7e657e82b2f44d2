"""The decode step with its position on the device: ``ops.causal_attn(step=<tensor>, max_step=)`` and
``ops.headnorm_rope(pos=)`` against their host-scalar forms bit for bit, ``GemmaGenerator.device_step`` - eager and as a
replayed graph, on bf16 and on fp8 panels - against ``step()``'s logits bit for bit, ``generate(device_loop=True)`` against the
host loop token for token at temperature 0, inside ``ref_gemma_sample.admissible`` at temperature 0.7, and through
generate_video."""
import functools

import numpy as np
import pytest
import torch

import ref_gemma as G
import ref_gemma_decode as D
import ref_gemma_sample as S
from test_gemma_decode_gpu import KERNEL_CASES, SCALE

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")


def _i32(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _attn(dev, case, step_arg, max_step=None):
    """One launch on fresh device copies of the case's operands: (out, K cache, V^T cache, partials) on the host.  ``out`` and
    ``partials`` start as NaN, so what a launch leaves alone shows."""
    from mlx_video_amd import ops
    B, Hq, Hkv, step, rs, window, cap = case
    q1, k, v, kc, vtc = _inputs(case)
    nq, nkv = Hq * 256, Hkv * 256
    qkv = torch.cat([q1, k[:, step], v[:, step]], 1).to(dev)
    kc, vtc = kc.to(dev), vtc.to(dev)
    out = torch.full((B, nq), NAN, dtype=BF, device=dev)
    partials = torch.full((B * Hq * (-(-cap // 256)) * 258,), NAN, dtype=torch.float32, device=dev)
    kw = {} if max_step is None else dict(max_step=max_step)
    if max_step is not None:
        step_arg = torch.tensor([step_arg], dtype=torch.int32, device=dev)
    ops.causal_attn(qkv[:, :nq], kc.view(B * cap, nkv), vtc, out, torch.tensor(rs, dtype=torch.int32, device=dev), B, Hq, Hkv, cap, SCALE,
                    window=window, step=step_arg, k_new=qkv[:, nq:nq + nkv], v_new=qkv[:, nq + nkv:], partials=partials, **kw)
    torch.cuda.synchronize()
    return out.cpu(), kc.cpu(), vtc.cpu(), partials.cpu()


@functools.lru_cache(maxsize=None)
def _inputs(case):
    B, Hq, Hkv, step, rs, window, cap = case
    return D.step_inputs(B, Hq, Hkv, step, list(rs), cap, seed=3)


CASES = [(c[0], c[1], c[2], c[3], tuple(c[4]), c[5], c[6]) for c in KERNEL_CASES]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-Hq{}-Hkv{}-step{}-rs{}-w{}-cap{}".format(c[0], c[1], c[2], c[3], "_".join(map(str, c[4])), c[5], c[6]))
def test_attention_step_device_position(dev, case):
    """The device-position form against the host-scalar form on the existing case grid, with the launch sized for the step
    itself and for the whole cache: out, the appended K row and V^T column, the untouched rest of the cache and the live
    partials are equal bit for bit (what lies past the live partials is the NaN both started from).  A position one past
    max_step, and -1, change nothing at all."""
    B, Hq, Hkv, step, rs, window, cap = case
    want = _attn(dev, case, step)
    s0 = max(0, step - window + 1) // 256 if window else 0
    live = B * Hq * (step // 256 + 1 - s0) * 258
    assert not bool(torch.isnan(want[3][:live]).any()) and bool(torch.isnan(want[3][live:]).all())
    for max_step in sorted({step, cap - 1}):
        got = _attn(dev, case, step, max_step=max_step)
        for name, a, b in zip(("out", "k_cache", "vt_cache", "partials"), got, want):
            assert torch.equal(_i32(a), _i32(b)), (name, max_step)
    _, _, _, kc, vtc = _inputs(case)
    for bad, max_step in ((step + 1, step), (-1, cap - 1), (cap, cap - 1)):
        out, kc2, vtc2, part = _attn(dev, case, bad, max_step=max_step)
        assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(part).all()), (bad, max_step)
        assert torch.equal(_i32(kc2), _i32(kc)) and torch.equal(_i32(vtc2), _i32(vtc)), (bad, max_step)


@pytest.mark.parametrize("M", [1, 8])
def test_headnorm_rope_at_position(dev, M):
    """``headnorm_rope(pos=)`` against the call on the sliced tables with T = 1, bit for bit, at positions 0, 1 and T - 1;
    position T (and -1) stores nothing."""
    from mlx_video_amd import ops
    from mlx_video_amd.gemma import rope_table_half
    T, Hq, Hkv = 40, 4, 2
    g = torch.Generator().manual_seed(M)
    buf = (torch.randn(M, (Hq + 2 * Hkv) * 256, generator=g) * 2).to(BF).to(dev)
    qw, kw = [(torch.randn(256, generator=g) * 0.1).to(BF).to(dev) for _ in range(2)]
    cos, sin = [t.to(dev) for t in rope_table_half(T, 10_000.0)]
    for p in (0, 1, T - 1):
        want = ops.headnorm_rope(buf.clone(), Hq, Hkv, qw, kw, cos[p:p + 1], sin[p:p + 1], 1)
        got = ops.headnorm_rope(buf.clone(), Hq, Hkv, qw, kw, cos, sin, T, pos=torch.tensor([p], dtype=torch.int32, device=dev))
        assert torch.equal(_i32(got.cpu()), _i32(want.cpu())) and not torch.equal(_i32(got.cpu()), _i32(buf.cpu())), p
    for p in (T, -1):
        got = ops.headnorm_rope(buf.clone(), Hq, Hkv, qw, kw, cos, sin, T, pos=torch.tensor([p], dtype=torch.int32, device=dev))
        assert torch.equal(_i32(got.cpu()), _i32(buf.cpu())), p


# ------------------------------------------------------------------------------------------------------------ the model
T_PROMPT, CAP, N_STEPS = 250, 320, 24          # positions 250 .. 273: across 255 / 256 / 257; with window 16 s0 becomes 1 at 271


def _prompt():
    return G.tiny_inputs(T=T_PROMPT, pad=59)


@functools.lru_cache(maxsize=None)
def _generator(dev, window, fp8, seed=3):
    from mlx_video_amd.gemma import GemmaEncoder, GemmaGenerator, random_gemma_weights
    cfg = G.tiny_config(window)
    W = random_gemma_weights("cpu", cfg, seed=seed)
    return GemmaGenerator(GemmaEncoder({k: v.to(dev) for k, v in W.items()}, cfg, fp8="channel" if fp8 else None))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("window", [1024, 16])
def test_device_step_logits_equal_step(dev, window, fp8):
    """24 teacher-forced tokens after a 250-position prefill (row 1 left-padded by 59) at capacity 320: the logits ``device_step``
    leaves - run eagerly, and recorded once and replayed - equal ``step()``'s bit for bit at every step, and so do the caches at
    the end."""
    from mlx_video_amd.gemma import GemmaDecodeState
    gen = _generator(dev, window, fp8)
    ids, mask = _prompt()
    feed = torch.randint(1, 512, (N_STEPS, 2), generator=torch.Generator().manual_seed(window))
    cache, _ = gen.prefill(ids, mask, CAP)
    want = [gen.step(cache, feed[i]).cpu() for i in range(N_STEPS)]
    assert cache.length == T_PROMPT + N_STEPS
    for graph in (False, True):
        c2, _ = gen.prefill(ids, mask, CAP)
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
        assert st.ctl.cpu().tolist() == [N_STEPS, T_PROMPT + N_STEPS, 2]
        for l in range(gen.cfg.num_hidden_layers):
            assert torch.equal(_i32(c2.k[l].cpu()), _i32(cache.k[l].cpu())) and torch.equal(_i32(c2.vt[l].cpu()), _i32(cache.vt[l].cpu())), (graph, l)


N_GEN, PENALTY = 12, 100.0          # test_gemma_decode_gpu.test_greedy_generation's: the penalty makes every step pick a new token


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_generate_device_loop_equals_host_loop_at_temperature_zero(dev, fp8):
    """``generate(device_loop=True, temperature=0, repetition_penalty=100)`` gives the host loop's tokens, row for row - also
    when ``eos_ids`` is row 0's third token - as a graph and eagerly, with the host looking every step and every 16."""
    gen = _generator(dev, 1024, fp8)
    ids, mask = _prompt()
    kw = dict(max_tokens=N_GEN, temperature=0.0, repetition_penalty=PENALTY)
    host = gen.generate(ids, mask, eos_ids=(), **kw)
    third = host[0][2]
    host_stop = gen.generate(ids, mask, eos_ids=(third,), **kw)
    assert [len(h) for h in host] == [N_GEN] * 2 and len(host_stop[0]) == 3
    for graph in (True, False):
        for sync_every in (1, 16):
            assert gen.generate(ids, mask, eos_ids=(), device_loop=True, graph=graph, sync_every=sync_every, **kw) == host, (graph, sync_every)
            assert gen.generate(ids, mask, eos_ids=(third,), device_loop=True, graph=graph, sync_every=sync_every, **kw) == host_stop, (graph, sync_every)
    assert gen.generate(ids, mask, eos_ids=(), device_loop=True, max_tokens=1, temperature=0.0, repetition_penalty=PENALTY) == [h[:1] for h in host]


def test_generate_device_loop_at_temperature(dev):
    """Temperature 0.7, penalty 1.3 over 20 tokens, a seed: two runs give the same tokens, the graph and the eager loop agree, and
    every token lies in admissible(...) of that step's logits under the uniform the state recorded for it - the host restatement
    is ``prefill`` / ``step`` teacher-forced with the device's tokens."""
    gen = _generator(dev, 1024, False)
    ids, mask = _prompt()
    kw = dict(max_tokens=N_GEN, temperature=0.7, repetition_penalty=1.3, repetition_context=20, eos_ids=(), seed=11, device_loop=True)
    toks = gen.generate(ids, mask, **kw)
    assert toks == gen.generate(ids, mask, **kw) == gen.generate(ids, mask, graph=False, **kw)
    assert [len(t) for t in toks] == [N_GEN] * 2 and toks != gen.generate(ids, mask, **dict(kw, seed=12))
    us = torch.rand((N_GEN, 2), generator=torch.Generator().manual_seed(11))
    cache, logits = gen.prefill(ids, mask, CAP)
    history = [[int(t) for t in ids[b][mask[b].bool()]] for b in range(2)]
    for n in range(N_GEN):
        lg = logits.cpu().numpy()
        for b in range(2):
            ok = S.admissible(lg[b], history[b][-20:], 1.3, 0.7, float(us[n, b]))
            assert toks[b][n] in ok, (n, b, toks[b][n], sorted(ok))
            history[b].append(toks[b][n])
        if n + 1 < N_GEN:
            logits = gen.step(cache, torch.tensor([toks[0][n], toks[1][n]]))


def test_generate_video_enhance_device_loop(dev, tmp_path, monkeypatch):
    """generate_video(enhance_prompt=True, enhance_device_loop=True, temperature=0) enhances to the host loop's string and gives
    its latents."""
    pytest.importorskip("tokenizers")
    from mlx_video_amd import generate as GV
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    from test_gemma_decode_gpu import _gemma_dir
    from test_pipeline_gpu import _mods, _Noise
    m = _mods(dev)
    root = tmp_path / "gemma"
    cfg = _gemma_dir(root, 256, seed=9)
    conn = TextConnector(random_connector_weights(dev, D=256, L=cfg.num_hidden_layers + 1, layers=1, R=16))
    seen = []
    real = GV._enhance_prompt

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((out[1], kw.get("device_loop", False)))
        return out

    monkeypatch.setattr(GV, "_enhance_prompt", spy)
    common = dict(pipeline=GV.PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
                  transformer=m["transformer"], vae_decoder=m["vae_decoder"], compile_step=True, cfg_batch=True, device=dev,
                  return_latents=True, gemma_repo=str(root), text_connector=conn, negative_prompt="w9", prompt="w4 w5",
                  enhance_prompt=True, max_tokens=8, temperature=0.0)
    a = GV.generate_video(noise_fn=_Noise(7, dev), **common)
    b = GV.generate_video(noise_fn=_Noise(7, dev), enhance_device_loop=True, **common)
    assert [s[1] for s in seen] == [False, True] and seen[0][0] == seen[1][0] and seen[0][0] != "w4 w5"
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
