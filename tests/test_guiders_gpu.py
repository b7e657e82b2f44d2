"""The CFG* and APG guiders on the GPU: the device-side sums against float64 and for determinism, the step tail bit for bit
against its restatement (ref_guiders.py), plain CFG unchanged, the denoise loop in its eager / graph / cfg_batch forms, and
the generate_video plumbing."""
import numpy as np
import pytest
import torch

import ref_guiders as RG
from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PAD = 64                     # elements of NaN on either side of every input (a multiple of 16 bytes in both dtypes)
KINDS = [("cfg_star", 1.0, 0.0), ("apg", 0.5, 0.0), ("apg", 0.5, 50.0)]          # (kind, eta, norm_threshold); 50 bites below
KIND_IDS = ["cfg_star", "apg", "apg_clamp"]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _fbits(t):
    return t.contiguous().view(torch.int32)


def _fenced(t, dev):
    """``t`` on the device inside a NaN-filled buffer: a read outside the tensor puts a NaN into a sum or an output."""
    n = t.numel()
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=t.dtype, device=dev)
    buf[PAD:PAD + n] = t.reshape(-1).to(dev)
    return buf[PAD:PAD + n].view(t.shape)


def _nan_scratch(B, C, S, dev):
    from mlx_video_amd import ops
    ws = torch.full((ops.guidance_sums_workspace_bytes(B, C, S) // 4,), float("nan"), dtype=torch.float32, device=dev)
    return torch.full((B, RG.REC), float("nan"), dtype=torch.float32, device=dev), ws


def _sums(dev, vp, vn, x, kind, sigma, thr, sigmas_dev=None):
    """One guidance_sums call on fenced inputs with NaN-filled record and workspace -> the record on the host."""
    from mlx_video_amd import ops
    B, C, S = x.shape
    rec, ws = _nan_scratch(B, C, S, dev)
    ops.guidance_sums(_fenced(vp, dev), _fenced(vn, dev), _fenced(x, dev), kind, sigma, thr, record=rec, workspace=ws,
                      sigmas_dev=sigmas_dev)
    torch.cuda.synchronize()
    return rec.cpu()


def _ord(t):
    """bf16 values -> integers in which neighbouring bf16 numbers differ by one."""
    assert torch.equal(t.to(BF).float(), t), f"not a bf16 value: {t}"
    b = t.to(BF).view(torch.int16).int()
    return torch.where(b < 0, -(b & 0x7FFF), b)


def _within_one_ulp(dev_val, ref_val, what):
    assert bool(torch.isfinite(dev_val).all()), f"{what}: {dev_val}"
    d = (_ord(dev_val) - _ord(ref_val)).abs()
    assert int(d.max()) <= 1, f"{what}: device {dev_val.tolist()} restatement {ref_val.tolist()}"


def _within_sum_bound(dev_sum, ref, what):
    s, a = ref
    err = (dev_sum.double() - s).abs()
    assert bool((err <= 1e-5 * a).all()), f"{what}: device {dev_sum.tolist()} float64 {s.tolist()} bound {(1e-5 * a).tolist()}"


def _check_record(rec, vp, vn, x, kind, sigma, thr, tag):
    """Every raw sum within 1e-5 * sum|term| of the float64 sum of the same bf16 products; every derived scalar within one
    bf16 ulp of the restatement evaluated on the float64 sums; the fields the guider does not use at their stated values."""
    assert bool(torch.isfinite(rec).all()), f"{tag}: {rec}"
    p, n = RG.denoised(vp, x, sigma), RG.denoised(vn, x, sigma)
    zero = torch.zeros(rec.shape[0])
    if kind == "cfg_star":
        sm = RG.sums_f64(p, n, kind)
        _within_sum_bound(rec[:, 0], sm["pn"], f"{tag} sum p*n")
        _within_sum_bound(rec[:, 1], sm["nn"], f"{tag} sum n*n")
        _within_one_ulp(rec[:, 5], RG.coef(sm["pn"][0], sm["nn"][0]), f"{tag} a")
        assert torch.equal(rec[:, 2], zero) and torch.equal(rec[:, 3], zero) and torch.equal(rec[:, 4], zero + 1)
    else:
        # the rescaled g of sum r(g*p) is built with the device's own f (f itself is checked against the restatement)
        sm = RG.sums_f64(p, n, kind, thr, rec[:, 4])
        if thr > 0:
            _within_sum_bound(rec[:, 0], sm["gg"], f"{tag} sum g*g")
            nrm, f = RG.clamp_scalars(sm["gg"][0], thr)
            _within_one_ulp(rec[:, 3], nrm, f"{tag} nrm")
            _within_one_ulp(rec[:, 4], f, f"{tag} f")
            assert bool((rec[:, 4] <= 1.0).all())
        else:
            assert torch.equal(rec[:, 0], zero) and torch.equal(rec[:, 3], zero) and torch.equal(rec[:, 4], zero + 1)
        _within_sum_bound(rec[:, 1], sm["gp"], f"{tag} sum g*p")
        _within_sum_bound(rec[:, 2], sm["pp"], f"{tag} sum p*p")
        _within_one_ulp(rec[:, 5], RG.coef(sm["gp"][0], sm["pp"][0]), f"{tag} c")
    assert torch.equal(rec[:, 6], zero) and torch.equal(rec[:, 7], zero)


def _inputs(B, C, S, seed):
    g = torch.Generator().manual_seed(seed)
    vp, vn = (torch.randn(B, S, C, generator=g).to(BF) for _ in range(2))
    x = torch.randn(B, C, S, generator=g).to(BF)
    return vp, vn, x


# -------------------------------------------------------------------------------------------------------------- sums
# lane (1), wave (63 / 64 / 65) and multi-workgroup edges, the bench shape (1280), and a 2^20-element sample (8190 * 128) for
# the accumulation bound
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 200, 1280, 8190])
def test_sums_against_float64(dev, S, B):
    C, sigma = 128, 0.75
    vp, vn, x = _inputs(B, C, S, 100 + S)
    _check_record(_sums(dev, vp, vn, x, "cfg_star", sigma, 0.0), vp, vn, x, "cfg_star", sigma, 0.0, f"cfg_star S={S} B={B}")
    _check_record(_sums(dev, vp, vn, x, "apg", sigma, 0.0), vp, vn, x, "apg", sigma, 0.0, f"apg S={S} B={B}")
    # the clamp: a threshold of half the measured norm bites (f < 1), twice the norm does not (f == 1)
    nrm = float(_sums(dev, vp, vn, x, "apg", sigma, 1.0)[0, 3])
    assert nrm > 0
    for factor in (0.5, 2.0):
        thr = factor * nrm
        rec = _sums(dev, vp, vn, x, "apg", sigma, thr)
        _check_record(rec, vp, vn, x, "apg", sigma, thr, f"apg clamp x{factor} S={S} B={B}")
        assert bool((rec[:, 4] < 1.0).all()) == (factor < 1.0) and bool((rec[:, 4] == 1.0).all()) == (factor > 1.0)
    # sigma from device memory: the same bits
    sig = torch.tensor([sigma, 0.5], dtype=torch.float32, device=dev)
    assert torch.equal(_fbits(_sums(dev, vp, vn, x, "apg", 123.0, 0.5 * nrm, sigmas_dev=sig)),
                       _fbits(_sums(dev, vp, vn, x, "apg", sigma, 0.5 * nrm)))


@pytest.mark.parametrize("S", [65, 200])
def test_sums_of_a_zero_negative_prediction(dev, S):
    """x = 0 and v- = 0, so n = 0: a = 0 / r(0 + 1e-8) = 0, finite; APG projects onto p, which is not zero.  And p = 0."""
    B, C, sigma = 2, 128, 0.5
    vp, _, _ = _inputs(B, C, S, 7)
    z_tok, z_lat = torch.zeros(B, S, C).to(BF), torch.zeros(B, C, S).to(BF)
    rec = _sums(dev, vp, z_tok, z_lat, "cfg_star", sigma, 0.0)
    assert bool(torch.isfinite(rec).all()) and torch.equal(rec[:, 5], torch.zeros(B)) and torch.equal(rec[:, 1], torch.zeros(B))
    _check_record(rec, vp, z_tok, z_lat, "cfg_star", sigma, 0.0, "n = 0")
    for thr in (0.0, 3.0):
        _check_record(_sums(dev, vp, z_tok, z_lat, "apg", sigma, thr), vp, z_tok, z_lat, "apg", sigma, thr, "n = 0 apg")
        rec = _sums(dev, z_tok, z_tok, z_lat, "apg", sigma, thr)          # p = n = g = 0
        assert bool(torch.isfinite(rec).all()) and torch.equal(rec[:, 5], torch.zeros(B))
        if thr > 0:
            assert torch.equal(rec[:, 4], torch.ones(B))                  # min(1, thr / r(sqrt(1e-8)))


@pytest.mark.parametrize("kind,eta,thr", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("S", [65, 1280])
def test_sums_are_deterministic_and_batch_independent(dev, S, kind, eta, thr):
    C, sigma = 128, 0.75
    vp, vn, x = _inputs(3, C, S, 300 + S)
    thr = thr * (S / 200) ** 0.5            # keeps the clamp biting at both sizes (|g| grows as sqrt(S))
    three = _sums(dev, vp, vn, x, kind, sigma, thr)
    again = _sums(dev, vp, vn, x, kind, sigma, thr)
    assert bool(torch.isfinite(three).all())
    assert torch.equal(_fbits(three), _fbits(again)), "two launches of the same inputs differ"
    if thr > 0:
        assert bool((three[:, 4] < 1.0).all())
    for b in range(3):
        one = _sums(dev, vp[b:b + 1], vn[b:b + 1], x[b:b + 1], kind, sigma, thr)
        assert torch.equal(_fbits(one[0]), _fbits(three[b])), f"sample {b} of the B=3 launch differs from the sample launched alone"


# -------------------------------------------------------------------------------------------------------------- tail
@pytest.fixture(scope="module")
def tail_case():
    B, C, S = 2, 128, 200
    g = torch.Generator().manual_seed(3)
    vp, vn, vq = (torch.randn(B, S, C, generator=g).to(BF) for _ in range(3))
    x = torch.randn(B, C, S, generator=g).to(BF)
    clean = torch.randn(B, C, S, generator=g).to(BF)
    mask = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (B, S), generator=g)]
    return vp, vn, vq, x, clean, mask


@pytest.mark.parametrize("s,sn", [(0.75, 0.5), (0.5, 0.0)])
@pytest.mark.parametrize("dev_sig", [False, True])
@pytest.mark.parametrize("bf16_euler", [False, True])
@pytest.mark.parametrize("with_stg", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind,eta,thr", KINDS, ids=KIND_IDS)
def test_guider_tail_bits(dev, tail_case, kind, eta, thr, masked, with_stg, bf16_euler, dev_sig, s, sn):
    from mlx_video_amd import ops
    vp, vn, vq, x, clean, mask = tail_case
    cfg, stg = 6.0, 1.5
    B, C, S = x.shape
    d_vp, d_vn, d_x = _fenced(vp, dev), _fenced(vn, dev), _fenced(x, dev)
    d_vq = _fenced(vq, dev) if with_stg else None
    d = dict(clean=_fenced(clean, dev) if masked else None, mask_tok=_fenced(mask, dev) if masked else None, bf16_euler=bf16_euler)
    sig = torch.tensor([s, sn], dtype=torch.float32, device=dev) if dev_sig else None
    hs, hsn = (123.0, 45.0) if dev_sig else (s, sn)              # with device sigmas the host values are not used
    rec, ws = _nan_scratch(B, C, S, dev)
    ops.guidance_sums(d_vp, d_vn, d_x, kind, hs, thr, record=rec, workspace=ws, sigmas_dev=sig)
    out = ops.guider_euler_step(d_vp, d_vn, d_vq, d_x, rec, kind, cfg, stg, hs, hsn, eta, thr, sigmas_dev=sig, **d)
    today = ops.guided_euler_step(d_vp, d_vn, d_vq, d_x, cfg, stg, hs, hsn, sigmas_dev=sig, **d)
    inplace = d_x.clone()
    ops.guider_euler_step(d_vp, d_vn, d_vq, inplace, rec, kind, cfg, stg, hs, hsn, eta, thr, out=inplace, sigmas_dev=sig, **d)
    torch.cuda.synchronize()
    rec = rec.cpu()
    _check_record(rec, vp, vn, x, kind, s, thr, kind)
    if thr > 0:
        assert bool((rec[:, 4] < 1.0).all()), "the clamp of this case is meant to bite"
    ref = RG.tail(vp, vn, vq if with_stg else None, x, rec, kind, cfg, stg, s, sn, eta, thr, clean if masked else None,
                  mask if masked else None, bf16_euler)
    assert torch.equal(_bits(out.cpu()), _bits(ref))
    assert torch.equal(_bits(inplace), _bits(out)), "out = latent gives other bits"
    assert not torch.equal(out, today), "the guider's tail equals the plain CFG tail"


# ------------------------------------------------------------------------------------------------------------- loop
F_, H_, W_, S_CTX = 2, 4, 4, 64


@pytest.fixture(scope="module")
def small(dev):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    from mlx_video_amd.schedulers import create_position_grid, ltx2_scheduler
    cfg = O.DiTConfig(num_layers=3, heads=4, caption_channels=256)
    W = O.make_weights(cfg, seed=71)
    mc = LTXModelConfig(num_attention_heads=cfg.heads, num_layers=cfg.num_layers, caption_channels=cfg.caption_channels,
                        cross_attention_dim=cfg.dim)
    model = LTXModel(mc, {k: v.to(dev) for k, v in W.items()})
    g = torch.Generator().manual_seed(72)
    lat = torch.randn(1, 128, F_, H_, W_, generator=g).to(BF).to(dev)
    cp, cn = (torch.randn(1, S_CTX, cfg.caption_channels, generator=g).to(BF).to(dev) for _ in range(2))
    clean = torch.randn(1, 128, F_, H_, W_, generator=g).to(BF).to(dev)
    mask = torch.ones(1, 1, F_, 1, 1)
    mask[:, :, 0] = 0.0                                      # a clean first frame
    return dict(model=model, lat=lat, cp=cp, cn=cn, clean=clean, mask=mask.to(BF).to(dev),
                pos=create_position_grid(1, F_, H_, W_).to(dev), sig=ltx2_scheduler(3, F_ * H_ * W_))


def _state(m):
    from mlx_video_amd.conditioning import LatentState
    return LatentState(m["lat"], m["clean"], m["mask"])


def _run(m, **kw):
    from mlx_video_amd.denoise import denoise_dev
    kw.setdefault("cfg_scale", 6.0)
    kw.setdefault("compile_step", True)
    out = denoise_dev(m["lat"], m["pos"], m["cp"], m["cn"], m["model"], m["sig"], state=_state(m), **kw)
    torch.cuda.synchronize()
    return out


def test_plain_cfg_is_unchanged(dev, small):
    """guider="cfg" (whatever the APG numbers say) and a disabled guider (cfg_scale == 1) are today's loop: equal bits, eager and
    graph, and the same graph cache keys."""
    for kw in (dict(cfg_batch=True), dict(cfg_batch=False), dict(cfg_batch=False, compile_step=False)):
        assert torch.equal(_run(small, **kw), _run(small, guider="cfg", apg_eta=0.5, apg_norm_threshold=3.0, **kw))
    eager = _run(small, cfg_batch=True)
    c0, c1 = {}, {}
    a = _run(small, cfg_batch=True, use_graph=True, graph_cache=c0)
    b = _run(small, cfg_batch=True, use_graph=True, graph_cache=c1, guider="cfg", apg_eta=0.5, apg_norm_threshold=3.0)
    assert torch.equal(a, b) and torch.equal(a, eager)
    assert set(c0) == set(c1) and len(c0) == 1
    # cfg_scale == 1: every guider is disabled - no negative forward, no error, today's key
    _run(small, cfg_scale=1.0, use_graph=True, graph_cache=c0)
    off = _run(small, cfg_scale=1.0, use_graph=True, graph_cache=c1, guider="apg", apg_norm_threshold=3.0)
    assert set(c0) == set(c1) and len(c0) == 2
    assert torch.equal(off, _run(small, cfg_scale=1.0)) and torch.equal(off, _run(small, cfg_scale=1.0, guider="cfg_star"))
    # a guider that is on adds its own key
    _run(small, cfg_batch=True, use_graph=True, graph_cache=c1, guider="apg", apg_norm_threshold=3.0)
    _run(small, cfg_batch=True, use_graph=True, graph_cache=c1, guider="apg", apg_norm_threshold=4.0)
    assert len(c1) == 4 and set(c0) < set(c1)


def test_cached_graph_refreshes_every_step_input(dev, small):
    """Two calls through one cached step graph, same geometry, other latents, clean latent and mask (other mask values, so
    other timestep tables and another token -> row map): each equals the eager loop of its own inputs bit for bit.  Catches a
    persistent step input (denoise._StepInputs) that a later call does not refresh."""
    g = torch.Generator().manual_seed(73)
    lat2, clean2 = (torch.randn(1, 128, F_, H_, W_, generator=g).to(BF).to(dev) for _ in range(2))
    mask2 = torch.ones(1, 1, F_, 1, 1)
    mask2[:, :, 1] = 0.5                                     # first call: frame 0 clean; this one: frame 1 half denoised
    other = dict(small, lat=lat2, clean=clean2, mask=mask2.to(BF).to(dev))
    cache = {}
    for m in (small, other, small):
        got = _run(m, cfg_batch=True, use_graph=True, graph_cache=cache)
        assert torch.equal(_bits(got), _bits(_run(m, cfg_batch=True)))
    assert len(cache) == 1
    assert not torch.equal(_run(other, cfg_batch=True), _run(small, cfg_batch=True))


def _host_loop(m, kind, eta, thr, cfg_scale=6.0, steps=None):
    """The loop restated: forward_tokens twice, ops.guidance_sums, and the CPU restatement of the tail, per step.
    Returns the latents and the per-step records (steps, B, 8)."""
    from mlx_video_amd import ops
    from mlx_video_amd.denoise import _StepPlan
    from mlx_video_amd.ltx_model import precompute_freqs_cis
    tr = m["model"]
    st = _state(m)
    lat = st.latent.to(BF).contiguous()
    sig = [float(s) for s in m["sig"].tolist()]
    plan = _StepPlan(lat, st, 1, sig)
    pe = precompute_freqs_cis(m["pos"][:1].contiguous(), tr.inner_dim, tr.positional_embedding_theta,
                              tr.positional_embedding_max_pos, tr.num_attention_heads)
    B, C = lat.shape[:2]
    clean, mask = plan.clean.reshape(B, C, -1).cpu(), plan.mask_tok_f32.cpu()
    recs = []
    for i in range(len(sig) - 1 if steps is None else steps):
        s, sn = plan.sig_bf[i], plan.sig_bf[i + 1]
        tp = plan.timestep_plan(i)
        tok = ops.latent_to_tokens(lat, rep=1)
        vp = tr.forward_tokens(tok, tp, m["cp"], pe, None)
        vn = tr.forward_tokens(tok, tp, m["cn"], pe, None)
        rec = ops.guidance_sums(vp, vn, lat, kind, s, thr)
        torch.cuda.synchronize()
        out = RG.tail(vp.cpu(), vn.cpu(), None, lat.reshape(B, C, -1).cpu(), rec.cpu(), kind, cfg_scale, 0.0, s, sn, eta, thr,
                      clean, mask)
        lat = out.reshape(lat.shape).to(lat.device)
        recs.append(rec.cpu())
    return lat, torch.stack(recs)


# clamp: the APG norm threshold as a fraction of the guidance norm this model gives in the first step (measured in the test: it
# depends on the random weights), so that the clamp is known to bite there; None = no clamp
@pytest.mark.parametrize("kind,eta,clamp", [("cfg_star", 1.0, None), ("apg", 0.5, None), ("apg", 0.5, 0.25)], ids=KIND_IDS)
def test_guider_loop_forms_agree(dev, small, kind, eta, clamp):
    m = small
    model = m["model"]
    try:
        model.batch_invariant = True                 # also turns attention's tail split off: a row's bits do not depend on B
        thr = 0.0
        if clamp is not None:
            nrm0 = float(_host_loop(m, kind, eta, 1.0, steps=1)[1][0, 0, 3])       # the first step's velocities do not depend on thr
            assert nrm0 > 0
            thr = clamp * nrm0
        kw = dict(guider=kind, apg_eta=eta, apg_norm_threshold=thr)
        ref, recs = _host_loop(m, kind, eta, thr)
        print(f"{kind} thr={thr}: per-step nrm {recs[:, 0, 3].tolist()} f {recs[:, 0, 4].tolist()} coef {recs[:, 0, 5].tolist()}")
        separate = _run(m, cfg_batch=False, **kw)
        batched = _run(m, cfg_batch=True, **kw)
        cache = {}
        graph = _run(m, cfg_batch=True, use_graph=True, graph_cache=cache, **kw)
        graph2 = _run(m, cfg_batch=True, use_graph=True, graph_cache=cache, **kw)
        graph_sep = _run(m, cfg_batch=False, use_graph=True, **kw)
        plain = _run(m, cfg_batch=True)
        stg = _run(m, cfg_batch=True, stg_scale=1.0, stg_blocks=[1], **kw)
        stg_graph = _run(m, cfg_batch=True, stg_scale=1.0, stg_blocks=[1], use_graph=True, **kw)
        eager_form = _run(m, cfg_batch=True, compile_step=False, **kw)           # sums + x0-only tail, then euler_only
    finally:
        model.batch_invariant = False
    assert bool(torch.isfinite(separate.float()).all())
    assert torch.equal(_bits(separate), _bits(ref)), "denoise_dev differs from the host loop"
    assert torch.equal(batched, separate), "cfg_batch changes the bits in batch-invariant mode"
    assert torch.equal(graph, batched) and torch.equal(graph2, batched) and torch.equal(graph_sep, batched), "graph replay differs from eager"
    assert len(cache) == 1
    assert not torch.equal(batched, plain), "the guider's loop equals the plain CFG loop"
    assert bool(torch.isfinite(stg.float()).all()) and not torch.equal(stg, batched) and torch.equal(stg_graph, stg)
    assert bool(torch.isfinite(eager_form.float()).all())
    assert torch.equal(separate[:, :, 0], m["clean"][:, :, 0]), "the clean first frame was not kept"
    f = recs[:, :, 4]
    if clamp is not None:      # bites in the first step by construction of thr; the later steps are printed above
        assert float(f[0].max()) < 1.0, f"the clamp does not bite in the first step: f = {f.tolist()}"
        assert not torch.equal(batched, _run(m, cfg_batch=True, guider=kind, apg_eta=eta)), "the clamp changes nothing"
    else:
        assert bool((f == 1.0).all())


# ---------------------------------------------------------------------------------------------------------- pipeline
def _pipeline_mods(dev):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    from mlx_video_amd.upsampler import LatentUpsampler
    from mlx_video_amd.video_vae import LTX2VideoDecoder
    from oracle import vae as OV
    cfg = O.DiTConfig(num_layers=2, heads=4, caption_channels=256)
    W = O.make_weights(cfg, seed=31)
    mc = LTXModelConfig(num_attention_heads=4, num_layers=2, caption_channels=256, cross_attention_dim=cfg.dim)
    Wd = OV.make_decoder_weights(seed=32, layers_per_block=1)
    Wu = OV.make_upsampler_weights(mid=128, nb=1)
    return dict(transformer=LTXModel(mc, {k: v.to(dev) for k, v in W.items()}),
                vae_decoder=LTX2VideoDecoder({k: v.to(dev) for k, v in Wd.items()}, num_layers_per_block=1),
                upsampler=LatentUpsampler({k: v.to(dev) for k, v in Wu.items()}, num_blocks_per_stage=1))


def test_pipelines_run_with_a_guider(dev):
    from mlx_video_amd.generate import PipelineType, generate_video
    m = _pipeline_mods(dev)
    g = torch.Generator().manual_seed(52)
    pe_pos = torch.randn(1, 64, 256, generator=g).to(BF)
    pe_neg = torch.randn(1, 64, 256, generator=g).to(BF)
    kw = dict(prompt="x", height=128, width=128, num_frames=9, cfg_scale=6.0, prompt_embeds=pe_pos, negative_prompt_embeds=pe_neg,
              device=dev, seed=5, compile_step=True, cfg_batch=True, num_inference_steps=2, return_latents=True, **m)
    apg = dict(guider="apg", apg_eta=0.5, apg_norm_threshold=4.0)
    cfg = generate_video(pipeline=PipelineType.DEV, guider="cfg", **kw)
    on = generate_video(pipeline=PipelineType.DEV, **apg, **kw)
    on2 = generate_video(pipeline=PipelineType.DEV, **apg, **kw)
    star = generate_video(pipeline=PipelineType.DEV, guider="cfg_star", **kw)
    assert bool(torch.isfinite(on.float()).all()) and bool(torch.isfinite(star.float()).all())
    assert torch.equal(on, on2), "repeated calls differ"
    assert not torch.equal(on, cfg) and not torch.equal(star, cfg) and not torch.equal(on, star)
    assert torch.equal(cfg, generate_video(pipeline=PipelineType.DEV, **kw))
    frames = generate_video(pipeline=PipelineType.DEV, **apg, **dict(kw, return_latents=False))
    assert frames.shape == (9, 128, 128, 3) and frames.dtype == np.uint8
    # the distilled pipeline's guided stage 2 (stage2_dev) runs the guider too; without a guided stage it is refused
    s2kw = dict(kw, stage1_steps=2, stage2_steps=1)
    s2 = generate_video(pipeline=PipelineType.DISTILLED, stage2_dev=True, **apg, **s2kw)
    s2_cfg = generate_video(pipeline=PipelineType.DISTILLED, stage2_dev=True, **s2kw)
    assert bool(torch.isfinite(s2.float()).all()) and not torch.equal(s2, s2_cfg)
    with pytest.raises(ValueError, match="guided denoise stage"):
        generate_video(pipeline=PipelineType.DISTILLED, **apg, **s2kw)
