"""The step cache in the denoise loop on the device (denoise.StepCache), tiny model (L = 2, D = 512, caption 256,
grid (3,5,6): N = 90 tokens, S = 70 text tokens), 6 or 8 steps:
  (a) off: the forward's launch table is unchanged and no step-cache launch happens;
  (b) threshold 0: latents bit-identical to the loop without the cache - eager and captured, cfg_batch on and off, once with STG;
  (c) a forced schedule C,S,S,C,S,C: latents bit-identical to a restatement built here from the model's own stage functions and
      torch arithmetic; eager equals captured; a second call through the same graph_cache with other latents, contexts and
      another schedule equals a fresh run;
  (d) adaptive: threshold 1.5 x the median rel of the threshold-0 run; 0 < skipped < n - 2, and StepCache.decide replayed on the
      host over the reported sums reproduces the device loop's flags;
  (e) parity: the float64 restatement (tests/ref_step_cache.py) teacher-forced with the device's decisions; device error <=
      1.25 e_ref, e_ref the bf16-policy restatement's own error (computed here, not pinned), and every reported rel within
      1.25 e_ref (relative) of the bf16-policy restatement's rel;
  (f) generate_video(step_cache_threshold=...) end to end, and the refusals of the joint, audio-only and sharded loops."""
import json
import statistics

import parity
import pytest
import torch

import ref_step_cache as R
from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CFG = O.DiTConfig(num_layers=2, heads=4, caption_channels=256)
GRID, S = (3, 5, 6), 70
N = GRID[0] * GRID[1] * GRID[2]
SCALE = 4.0


@pytest.fixture(scope="module")
def tiny(dev):
    """(weights, model): built once, never modified."""
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    W = R.make_weights(CFG, seed=7, **R.LIVELY)
    mc = LTXModelConfig(num_attention_heads=4, num_layers=2, caption_channels=256, cross_attention_dim=CFG.dim)
    return W, LTXModel(mc, {k: v.to(dev) for k, v in W.items()})


def _inputs(seed, b=1):
    g = torch.Generator().manual_seed(seed)
    return dict(lat=torch.randn(b, 128, *GRID, generator=g).to(BF), pos=torch.from_numpy(O.create_position_grid(b, *GRID)),
                cp=torch.randn(b, S, 256, generator=g).to(BF), cn=torch.randn(b, S, 256, generator=g).to(BF))


def _sig(n):
    from mlx_video_amd.schedulers import ltx2_scheduler
    sig = ltx2_scheduler(n, N).tolist()
    assert len(sig) == n + 1
    return sig


def _run(dev, model, c, sig, **kw):
    from mlx_video_amd.denoise import denoise_dev
    kw.setdefault("compile_step", True)
    out = denoise_dev(c["lat"].to(dev), c["pos"].to(dev), c["cp"].to(dev), c["cn"].to(dev), model, torch.tensor(sig), cfg_scale=SCALE, **kw)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def plain(dev, tiny):
    """The loop without the cache, 8 steps, inputs 21: computed once, shared, never modified."""
    return _run(dev, tiny[1], _inputs(21), _sig(8))


# ------------------------------------------------------------------------------------------------ (a) off
def test_off_is_todays_forward_and_loop(dev, monkeypatch):
    import test_dit_launch_trace_gpu as T
    from mlx_video_amd import ops
    weights = T.make_weights(dev)
    for name in ("bf16_fuse15", "hoisted_context"):
        m, args, n_tok, hoisted = T.build_case(name, weights, dev)
        want_prepare, want = T._expected(ops, name, n_tok)
        kv = m.prepare_context(args[2]) if hoisted else None
        with monkeypatch.context() as mp:
            calls = []
            T._trace(mp, ops, calls)
            v = m.forward_tokens(*args, ctx_kv=kv)
            assert calls == want, T._first_difference(calls, want)
            if hoisted:                # a computed step under the cache: the same GEMM launches, the same bits
                calls.clear()
                st = m._fwd_prepare(args[0], args[1], args[2], args[3], kv, None)
                probe = m.step_cache_input(st, args[0].shape[1], torch.empty((args[0].shape[1], m.inner_dim), dtype=BF, device=dev))
                resid = torch.empty_like(st.x)
                x_in = st.x.clone()
                v2 = m.forward_cached(st, resid, True)
                assert calls == want, T._first_difference(calls, want)
                assert torch.equal(v, v2)
                assert torch.equal(resid, (st.x.float() - x_in.float()).to(BF))
                assert bool(torch.isfinite(probe.float()).all())
    # the loop without a cache launches nothing of it
    def boom(*a, **k):
        raise AssertionError("a step-cache launch without a step cache")
    with monkeypatch.context() as mp:
        for fn in ("step_cache_probe", "residual_store", "residual_apply"):
            mp.setattr(ops, fn, boom)
        from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
        mc = LTXModelConfig(num_attention_heads=4, num_layers=2, caption_channels=256, cross_attention_dim=512)
        model = LTXModel(mc, weights[False])
        c, sig = _inputs(3), _sig(2)
        a = _run(dev, model, c, sig)
        b = _run(dev, model, c, sig, use_graph=True)
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ (b) threshold 0
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("batch", [False, True], ids=["two_forwards", "cfg_batch"])
def test_threshold_zero_is_the_plain_loop(dev, tiny, plain, graph, batch):
    from mlx_video_amd.denoise import StepCache
    sc = StepCache(0.0)
    out = _run(dev, tiny[1], _inputs(21), _sig(8), cfg_batch=batch, use_graph=graph, step_cache=sc)
    assert torch.equal(out, plain), "threshold 0 changed the latents"
    assert len(sc.report) == 8 and all(r["computed"] for r in sc.report) and sc.report[0]["rel"] is None
    rels = [r["rel"] for r in sc.report[1:]]
    assert len(rels) == 7 and all(r is not None and r > 0 for r in rels)
    assert sc.counts == {"steps": 8, "computed": 8, "skipped": 0}


def test_threshold_zero_with_stg(dev, tiny):
    from mlx_video_amd.denoise import StepCache
    c, sig = _inputs(22), _sig(6)
    for batch in (False, True):
        kw = dict(stg_scale=1.0, stg_blocks=[1], cfg_batch=batch)
        want = _run(dev, tiny[1], c, sig, **kw)
        for graph in (False, True):
            sc = StepCache(0.0)
            assert torch.equal(_run(dev, tiny[1], c, sig, use_graph=graph, step_cache=sc, **kw), want)
            assert len(sc.report) == 6


# ------------------------------------------------------------------------------------------------ (c) forced schedule
def _restated(dev, model, c, sig, schedule, batch):
    """The cached loop out of the model's stage functions: prepare; on a computed step the blocks and
    R = bf16(f32(x_out) - f32(x_in)); on a skipped step x = bf16(f32(x) + f32(R)); the head; the loop's own fused tail."""
    from mlx_video_amd import ops
    from mlx_video_amd.denoise import _Guidance, _StepPlan
    from mlx_video_amd.ltx_model import precompute_freqs_cis
    lat = c["lat"].to(dev).contiguous()
    cp, cn = c["cp"].to(dev), c["cn"].to(dev)
    b = lat.shape[0]
    gd = _Guidance(b, SCALE, batch, 0.0, None, None)
    pe = precompute_freqs_cis(c["pos"][:1].to(dev).contiguous(), model.inner_dim, model.positional_embedding_theta,
                              model.positional_embedding_max_pos, model.num_attention_heads)
    plan = _StepPlan(lat, None, gd.reps, sig)
    ctxs = [torch.cat([cp, cn], 0).contiguous()] if batch else [cp, cn]
    kvs = [model.prepare_context(x) for x in ctxs]
    resid = [None] * len(ctxs)
    for i in range(len(sig) - 1):
        tp = plan.timestep_plan(i)
        tok = ops.latent_to_tokens(lat, rep=gd.reps)
        vs = []
        for f, (ctx, kv) in enumerate(zip(ctxs, kvs)):
            st = model._fwd_prepare(tok, tp, ctx, pe, kv, None)
            if schedule[i]:
                x_in = st.x.clone()
                for li in range(len(model.blocks)):
                    model._fwd_attn(st, li)
                    model._fwd_ff(st, li)
                resid[f] = (st.x.float() - x_in.float()).to(BF)
            else:
                st.x.copy_((st.x.float() + resid[f].float()).to(BF))
            vs.append(model._fwd_head(st))
        v_pos, v_neg = (vs[0][:b], vs[0][b:]) if batch else vs
        lat = gd.tail(v_pos, v_neg, None, lat, plan.sig_bf[i], plan.sig_bf[i + 1], None, None)
    torch.cuda.synchronize()
    return lat


SCHEDULE = [True, False, False, True, False, True]
SCHEDULE_2 = [True, False, True, False, False, True]


@pytest.mark.parametrize("batch", [False, True], ids=["two_forwards", "cfg_batch"])
def test_forced_schedule_equals_the_restatement(dev, tiny, batch):
    from mlx_video_amd.denoise import StepCache
    model = tiny[1]
    sig = _sig(6)
    cache = {}
    for c, schedule in ((_inputs(31), SCHEDULE), (_inputs(32), SCHEDULE_2)):      # the second pair goes through the same graph_cache
        want = _restated(dev, model, c, sig, schedule, batch)
        sc = StepCache(0.0, schedule=schedule)
        eager = _run(dev, model, c, sig, cfg_batch=batch, step_cache=sc)
        assert [r["computed"] for r in sc.report] == schedule
        assert torch.equal(eager, want), "the eager cached loop differs from its restatement"
        sg = StepCache(0.0, schedule=schedule)
        graph = _run(dev, model, c, sig, cfg_batch=batch, use_graph=True, graph_cache=cache, step_cache=sg)
        assert torch.equal(graph, want), "the captured cached loop differs from the eager one"
        assert [(r["s_d"], r["s_p"]) for r in sg.report] == [(r["s_d"], r["s_p"]) for r in sc.report]
        assert not torch.equal(want, _run(dev, model, c, sig, cfg_batch=batch)), "the schedule skipped nothing that matters"
    assert len(cache) == 1
    with pytest.raises(ValueError, match="schedule"):
        _run(dev, model, _inputs(31), sig, step_cache=StepCache(0.0, schedule=SCHEDULE[:-1]))


# ------------------------------------------------------------------------------------------------ (d), (e) adaptive, parity
@pytest.fixture(scope="module")
def adaptive(dev, tiny):
    """One adaptive run at 1.5 x the median rel of the threshold-0 run (inputs 21, 8 steps): (StepCache, latents)."""
    from mlx_video_amd.denoise import StepCache
    c, sig = _inputs(21), _sig(8)
    s0 = StepCache(0.0)
    _run(dev, tiny[1], c, sig, cfg_batch=True, step_cache=s0)
    tau = 1.5 * statistics.median(r["rel"] for r in s0.report[1:])
    sc = StepCache(tau)
    out = _run(dev, tiny[1], c, sig, cfg_batch=True, use_graph=True, step_cache=sc)
    return sc, out.cpu()


def test_adaptive_policy_skips_and_replays_on_the_host(adaptive):
    from mlx_video_amd.denoise import StepCache
    sc, _ = adaptive
    n = len(sc.report)
    flags = [r["computed"] for r in sc.report]
    print("adaptive:", "".join("CS"[not f] for f in flags), [r["rel"] for r in sc.report])
    assert 0 < sc.counts["skipped"] < n - 2 and flags[0] and flags[-1]
    acc, replay = 0.0, []
    for i, r in enumerate(sc.report):
        compute, a, rel = StepCache.decide(i, n, r["s_d"], r["s_p"], acc, sc.threshold, sc.coefficients)
        assert rel == r["rel"] and a == r["acc"]
        acc = 0.0 if compute else a
        replay.append(compute)
    assert replay == flags


def test_cached_loop_against_float64(adaptive, tiny):
    sc, out = adaptive
    W = tiny[0]
    c, sig = _inputs(21), _sig(8)
    dec = [r["computed"] for r in sc.report]
    ref = lambda p: R.cached_loop(c["lat"].float(), c["pos"].numpy(), c["cp"].float(), c["cn"].float(), W, CFG, sig, p, SCALE, decisions=dec)
    (x64, _), (xpol, rpol) = ref(O.F64), ref(O.BF16_FLASH)
    e_ref, e_dev = parity.rel_l2(xpol, x64), parity.rel_l2(out, x64)
    print(f"cached loop: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    worst = max(abs(d["rel"] / p["rel"] - 1.0) for d, p in zip(sc.report[1:], rpol[1:]))
    print(f"reported rel against the bf16-policy restatement's: worst relative difference {worst:.3e} (band {1.25 * e_ref:.3e})")
    parity.auto(e_ref, 1.0, tag="e_ref")
    parity.auto(e_dev, 1.25 * e_ref, tag="device")
    parity.auto(worst, 1.25 * e_ref, tag="rel")


# ------------------------------------------------------------------------------------------------ (f) surface
def test_generate_video_with_a_step_cache(dev, tmp_path):
    from mlx_video_amd.generate import generate_video
    from mlx_video_amd.pipelines import PipelineType
    from test_pipeline_gpu import _Noise, _mods
    g = torch.Generator().manual_seed(50)
    emb = torch.randn(2, 64, 256, generator=g).to(BF)
    prof = tmp_path / "clip.profile.json"
    m = _mods(dev)
    kw = dict(prompt="x", pipeline=PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=6, cfg_scale=4.0,
              prompt_embeds=emb[0:1], negative_prompt_embeds=emb[1:2], device=dev, output_path=str(tmp_path / "clip.npy"),
              transformer=m["transformer"], vae_decoder=m["vae_decoder"])
    plain = generate_video(noise_fn=_Noise(7, dev), **kw)
    zero = generate_video(noise_fn=_Noise(7, dev), step_cache_threshold=0.0, **kw)
    assert (plain == zero).all(), "threshold 0 changed the frames"
    frames = generate_video(noise_fn=_Noise(7, dev), step_cache_threshold=float("inf"), step_cache_coefficients=[1.0, 0.0],
                            profile_json_path=str(prof), **kw)
    assert frames.shape == plain.shape
    rep = json.loads(prof.read_text())
    assert rep["step_cache"]["threshold"] == float("inf") and rep["step_cache"]["calls"] == [{"steps": 6, "computed": 2, "skipped": 4}]


def test_other_loops_refuse_a_step_cache(dev, tiny):
    from mlx_video_amd.denoise import StepCache, denoise_audio_only, denoise_dev_av
    from mlx_video_amd.sharding import CfgPairSharding
    sc = StepCache(0.1)
    with pytest.raises(ValueError, match="step cache"):
        denoise_dev_av(None, None, None, None, None, None, None, None, None, [1.0, 0.0], step_cache=sc)
    with pytest.raises(ValueError, match="step cache"):
        denoise_audio_only(None, None, None, None, [1.0, 0.0], step_cache=sc)
    sh = CfgPairSharding.__new__(CfgPairSharding)
    with pytest.raises(ValueError, match="step cache"):
        sh.denoise_dev(None, None, None, None, None, [1.0, 0.0], step_cache=sc)
    with pytest.raises(TypeError, match="StepCache"):
        _run(dev, tiny[1], _inputs(3), _sig(2), step_cache=0.1)
