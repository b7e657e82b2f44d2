"""The CFG* and APG guiders without a GPU: the test-side restatement (ref_guiders.py) against the host-side guiders of
``components`` in float64, the config, the CLI and keyword surface, argument errors raised before any launch, and the C-ABI
binding of the new entry points."""
import ctypes
import os
import re
import types

import pytest
import torch

import ref_guiders as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("ltxk_guidance_sums", "ltxk_guider_euler_step", "ltxk_guider_args_sizeof", "ltxk_guidance_sums_workspace_bytes")


# ------------------------------------------------------------------------------------------------------------ algebra
def _pair(seed=5, shape=(3, 16, 6, 10)):
    # 4-D (B,C,H,W): the axes (-1,-2,-3) of components._l2_norm then cover one whole sample, as the kernels' sums do
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("scale", [6.0, 2.5])
def test_cfg_star_f64_equals_components(scale):
    from mlx_video_amd import components as C
    p, n = _pair()
    ref = p + C.CFGStarRescalingGuider(scale).delta(p, n)
    assert float((RG.guided_x0_f64(p, n, "cfg_star", scale) - ref).abs().max()) < 1e-12
    assert float((RG.guided_x0_f64(p, n, "cfg", scale) - (p + C.CFGGuider(scale).delta(p, n))).abs().max()) < 1e-12


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("clamp", [None, "bites", "idle"])
def test_apg_f64_equals_components(eta, clamp):
    from mlx_video_amd import components as C
    p, n = _pair(seed=6)
    nrm = float((p - n)[0].norm())
    thr = {None: 0.0, "bites": 0.5 * nrm, "idle": 100.0 * nrm}[clamp]
    ref = p + C.LtxAPGGuider(6.0, eta, thr).delta(p, n)
    out = RG.guided_x0_f64(p, n, "apg", 6.0, eta, thr)
    assert float((out - ref).abs().max()) < 1e-12
    if clamp == "bites":
        assert float((out - RG.guided_x0_f64(p, n, "apg", 6.0, eta, 0.0)).abs().max()) > 1e-3
    if clamp == "idle":
        assert float((out - RG.guided_x0_f64(p, n, "apg", 6.0, eta, 0.0)).abs().max()) < 1e-12
    if eta == 1.0 and clamp is None:          # eta = 1 keeps the whole guidance vector: plain CFG
        assert float((out - RG.guided_x0_f64(p, n, "cfg", 6.0)).abs().max()) < 1e-12


def test_cfg_star_with_unit_coefficient_is_velocity_space_cfg():
    """x0 = x - sigma*v is affine in v with weights summing to one, so with a = 1 the x0-space form is the fused CFG tail."""
    g = torch.Generator().manual_seed(7)
    x, vp, vn = (torch.randn(2, 16, 40, generator=g, dtype=torch.float64) for _ in range(3))
    for scale, sigma in ((6.0, 0.9), (1.0, 0.3), (3.5, 1.0)):
        v = vp + (scale - 1.0) * (vp - vn)
        star = RG.cfg_star_x0_f64(x - sigma * vp, x - sigma * vn, 1.0, scale)
        assert float((star - (x - sigma * v)).abs().max()) < 1e-12


def test_rounded_restatement_follows_the_f64_form():
    """The bf16 form is the float64 form up to bf16 rounding: a few 2^-8 of the largest magnitude over a 6-op chain."""
    g = torch.Generator().manual_seed(8)
    B, C, S = 2, 16, 50
    vp, vn = (torch.randn(B, S, C, generator=g).to(RG.BF) for _ in range(2))
    x = torch.randn(B, C, S, generator=g).to(RG.BF)
    sigma = 0.75
    p, n = RG.denoised(vp, x, sigma).double(), RG.denoised(vn, x, sigma).double()
    for kind, eta, thr in (("cfg_star", 1.0, 0.0), ("apg", 0.5, 0.0), ("apg", 0.5, 10.0)):
        rec = RG.record(vp, vn, x, sigma, kind, thr)
        assert bool(torch.isfinite(rec).all())
        out = RG.tail(vp, vn, None, x, rec, kind, 6.0, 0.0, sigma, 0.0, eta, thr).double()
        ref = RG.guided_x0_f64(p, n, kind, 6.0, eta, thr)
        assert float((out - ref).abs().max()) < 8 * 2.0 ** -8 * float(ref.abs().max())
    rec = RG.record(vp, vn, x, sigma, "apg", 10.0)
    assert 0.0 < float(rec[0, 4]) < 1.0 and float(RG.record(vp, vn, x, sigma, "apg", 1e4)[0, 4]) == 1.0


def test_record_of_a_zero_negative_prediction_is_finite():
    vp = torch.ones(1, 8, 8).to(RG.BF)
    z = torch.zeros(1, 8, 8).to(RG.BF)
    rec = RG.record(vp, z, z, 0.5, "cfg_star")
    assert bool(torch.isfinite(rec).all()) and float(rec[0, 5]) == 0.0


# ------------------------------------------------------------------------------------------------------------- config
def test_guider_config_validation():
    from mlx_video_amd import components as C
    from mlx_video_amd.guidance import GuiderConfig
    assert GuiderConfig() == GuiderConfig("cfg", 1.0, 0.0) and GuiderConfig().is_default
    assert not GuiderConfig("apg").is_default and not GuiderConfig("cfg_star").is_default
    assert GuiderConfig("apg", 1, 2).key == ("apg", 1.0, 2.0)
    with pytest.raises(Exception):
        GuiderConfig().kind = "apg"                       # frozen
    for bad in (dict(kind="apg_legacy"), dict(kind="apg", eta=float("nan")), dict(kind="apg", eta=float("inf")),
                dict(kind="apg", norm_threshold=-1.0), dict(kind="apg", norm_threshold=float("inf")), dict(kind=None),
                dict(kind="apg", eta="much")):
        with pytest.raises(ValueError):
            GuiderConfig(**bad)
    # field for field what the host-side guiders are built from
    assert GuiderConfig("apg", 0.5, 2.0).component(6.0) == C.LtxAPGGuider(6.0, 0.5, 2.0)
    assert GuiderConfig("apg").component(3.0) == C.LtxAPGGuider(3.0)
    assert GuiderConfig("cfg_star").component(6.0) == C.CFGStarRescalingGuider(6.0)
    assert GuiderConfig().component(4.0) == C.CFGGuider(4.0)
    assert not GuiderConfig("apg").component(1.0).enabled()


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_parser_takes_the_guider_flags():
    from mlx_video_amd.generate import build_parser
    a = build_parser().parse_args([])
    assert a.guider == "cfg" and a.apg_eta == 1.0 and a.apg_norm_threshold == 0.0
    a = build_parser().parse_args(["--guider", "apg", "--apg-eta", "0.5", "--apg-norm-threshold", "12.5"])
    assert a.guider == "apg" and a.apg_eta == 0.5 and a.apg_norm_threshold == 12.5
    assert build_parser().parse_args(["--guider", "cfg_star"]).guider == "cfg_star"
    for bad in (["--guider", "apg_legacy"], ["--apg-eta", "nan"], ["--apg-eta", "x"], ["--apg-norm-threshold", "-1"],
                ["--apg-norm-threshold", "inf"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)


def test_main_passes_the_guider_flags_through(monkeypatch):
    from mlx_video_amd import generate as G
    seen = {}
    monkeypatch.setattr(G, "generate_video", lambda **kw: seen.update(kw))
    G.main(["--pipeline", "dev", "--guider", "apg", "--apg-eta", "0.25", "--apg-norm-threshold", "3"])
    assert (seen["guider"], seen["apg_eta"], seen["apg_norm_threshold"]) == ("apg", 0.25, 3.0)
    seen.clear()
    G.main(["--pipeline", "dev"])
    assert (seen["guider"], seen["apg_eta"], seen["apg_norm_threshold"]) == ("cfg", 1.0, 0.0)


def test_pipelines_carry_the_guider_fields(monkeypatch):
    from mlx_video_amd import pipelines as P
    assert {f.name for f in P.fields(P.MLXPipelineConfig)} >= {"guider", "apg_eta", "apg_norm_threshold"}
    assert P.MLXPipelineConfig().guider == "cfg"
    seen = {}
    monkeypatch.setattr(P, "generate_video", lambda **kw: seen.update(kw))
    P.TI2VidOneStagePipeline(guider="apg", apg_eta=0.5, apg_norm_threshold=4.0)("x", output_path=None)
    assert (seen["guider"], seen["apg_eta"], seen["apg_norm_threshold"]) == ("apg", 0.5, 4.0)
    seen.clear()
    P.DistilledPipeline()("x", output_path=None)
    assert (seen["guider"], seen["apg_eta"], seen["apg_norm_threshold"]) == ("cfg", 1.0, 0.0)


# ------------------------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("pipe,extra", [("distilled", {}), ("keyframe", {}), ("ic_lora", {"video_conditionings": [("v.mp4", 0, 1.0)]})])
@pytest.mark.parametrize("guider", ["cfg_star", "apg"])
def test_generate_video_refuses_a_guider_without_a_guided_stage(pipe, extra, guider):
    from mlx_video_amd.generate import PipelineType, generate_video
    with pytest.raises(ValueError, match="guided denoise stage"):
        generate_video(pipeline=PipelineType(pipe), guider=guider, **extra)


def test_generate_video_refuses_bad_guider_arguments():
    from mlx_video_amd.generate import PipelineType, generate_video
    with pytest.raises(ValueError, match="Unknown guider"):
        generate_video(pipeline=PipelineType.DEV, guider="apg_legacy")
    with pytest.raises(ValueError, match="apg_norm_threshold"):
        generate_video(pipeline=PipelineType.DEV, guider="apg", apg_norm_threshold=-1.0)
    with pytest.raises(ValueError, match="apg_eta"):
        generate_video(pipeline=PipelineType.DEV, guider="apg", apg_eta=float("nan"))


@pytest.mark.parametrize("kw", [dict(guider="apg_legacy"), dict(guider="apg", apg_eta=float("inf")),
                                dict(guider="apg", apg_norm_threshold=-0.5), dict(guider="cfg", apg_norm_threshold=-0.5)])
def test_denoise_dev_refuses_bad_guider_arguments(kw):
    from mlx_video_amd.denoise import denoise_dev
    model = types.SimpleNamespace(config=types.SimpleNamespace(num_layers=4))
    lat = torch.zeros(1, 128, 1, 2, 2, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        denoise_dev(lat, None, None, None, model, [1.0, 0.5, 0.0], cfg_scale=6.0, **kw)


def test_sharded_loop_refuses_a_guider():
    from mlx_video_amd.sharding import CfgPairSharding
    sh = CfgPairSharding(types.SimpleNamespace(new_group=lambda ranks: None), 0, 2)
    with pytest.raises(ValueError, match="sharded path"):
        sh.denoise_dev(None, None, None, None, None, [1.0, 0.0], guider="cfg_star")


def test_ops_refuse_bad_arguments_before_any_launch():
    from mlx_video_amd import _lib, ops
    x = torch.zeros(1, 128, 4, dtype=torch.bfloat16)
    v = torch.zeros(1, 4, 128, dtype=torch.bfloat16)
    rec = torch.zeros(1, 8)
    with pytest.raises(_lib.LtxkError):                         # CPU tensors: no fallback
        ops.guidance_sums(v, v, x, "apg", 0.5)
    with pytest.raises(_lib.LtxkError):
        ops.guider_euler_step(v, v, None, x, rec, "cfg_star", 6.0, 0.0, 0.5, 0.25)
    for call in (lambda: ops.guidance_sums(v, v, x, "cfg", 0.5),                                      # plain CFG is not a guider id
                 lambda: ops.guidance_sums(v, v, x, "apg", 0.5, norm_threshold=-1.0),
                 lambda: ops.guidance_sums(v, None, x, "apg", 0.5),
                 lambda: ops.guider_euler_step(v, v, None, x, rec, "apg", 6.0, 0.0, 0.5, 0.25, eta=float("nan")),
                 lambda: ops.guider_euler_step(v, None, None, x, rec, "apg", 6.0, 0.0, 0.5, 0.25),
                 lambda: ops.guider_euler_step(v, v, None, x, rec, "bogus", 6.0, 0.0, 0.5, 0.25)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        ops.guidance_sums_workspace_bytes(1, 12, 4)
    assert ops.guidance_sums_workspace_bytes(1, 128, 1280) == 2 * 16 * 20 * 4
    assert ops.guidance_sums_workspace_bytes(3, 128, 65) == 3 * 2 * 16 * 2 * 4


def test_library_refuses_bad_guider_structs():
    """The C entry points check their arguments on the host and return LTXK_EINVAL before any launch (no GPU is touched)."""
    from mlx_video_amd import _lib
    lib = _lib.load()

    def args(**over):
        a = _lib.GuiderArgs()
        buf = 4096                        # never dereferenced: every case below is refused by the host checks
        a.v_pos = a.v_neg = a.latent = a.out = a.record = a.workspace = buf
        a.workspace_bytes = 1 << 20
        a.B, a.C, a.S, a.guider = 1, 128, 64, _lib.GUIDER_APG
        a.cfg_scale, a.sigma, a.sigma_next, a.eta = 6.0, 0.5, 0.25, 1.0
        for k, v in over.items():
            setattr(a, k, v)
        return a
    bad = [dict(guider=0), dict(guider=3), dict(eta=float("nan")), dict(eta=float("inf")), dict(norm_threshold=-1.0),
           dict(v_neg=None), dict(C=12), dict(sigma=0.0), dict(record=None), dict(v_pos=4100)]
    for over in bad:
        for fn in (lib.ltxk_guidance_sums, lib.ltxk_guider_euler_step):
            assert fn(ctypes.byref(args(**over)), None) == -1, over
            assert lib.ltxk_last_error()
    assert lib.ltxk_guidance_sums(ctypes.byref(args(workspace_bytes=16)), None) == -1
    assert lib.ltxk_guidance_sums(ctypes.byref(args(workspace=None)), None) == -1
    assert lib.ltxk_guider_euler_step(ctypes.byref(args(clean=4096)), None) == -1          # clean without mask
    assert lib.ltxk_guider_euler_step(ctypes.byref(args(out=None)), None) == -1
    assert lib.ltxk_guidance_sums(None, None) == -1 and lib.ltxk_guider_euler_step(None, None) == -1


def test_every_tail_entry_refuses_grid_overflow_and_misaligned_tokens():
    """The four step-tail entries share one host check: B or C/8 past a grid dimension and a token pointer off a 16-byte
    boundary are LTXK_EINVAL under the entry's own name, before any launch (stand-in pointers, no GPU is touched).  And the
    host wrapper of the plain tail refuses what the kernel would misread."""
    from mlx_video_amd import _lib, ops
    lib = _lib.load()
    buf = 4096

    def call(entry, B=1, C=128, v_pos=buf, v_neg=buf):
        if entry == "ltxk_cfg_euler_step":
            return lib.ltxk_cfg_euler_step(v_pos, v_neg, buf, buf, None, None, B, C, 64, 6.0, 0.5, 0.25, 0, None)
        if entry == "ltxk_cfg_euler_step_dev":
            return lib.ltxk_cfg_euler_step_dev(v_pos, v_neg, buf, buf, None, None, B, C, 64, 6.0, buf, 0, None)
        a = _lib.StepArgs() if entry == "ltxk_guided_euler_step" else _lib.GuiderArgs()
        a.v_pos, a.v_neg, a.latent, a.out = v_pos, v_neg, buf, buf
        a.B, a.C, a.S = B, C, 64
        a.cfg_scale, a.sigma, a.sigma_next = 6.0, 0.5, 0.25
        if entry == "ltxk_guider_euler_step":
            a.record, a.guider, a.eta = buf, _lib.GUIDER_APG, 1.0
        return getattr(lib, entry)(ctypes.byref(a), None)

    for entry in ("ltxk_cfg_euler_step", "ltxk_cfg_euler_step_dev", "ltxk_guided_euler_step", "ltxk_guider_euler_step"):
        for over, why in ((dict(B=65536), "grid dimension"), (dict(C=8 * 65536), "grid dimension"),
                          (dict(v_pos=buf + 8), "16-byte"), (dict(v_neg=buf + 2), "16-byte")):
            assert call(entry, **over) == -1, (entry, over)
            msg = lib.ltxk_last_error().decode()
            assert msg.startswith(entry + ":") and why in msg, (entry, over, msg)
    x = torch.zeros(1, 128, 4, dtype=torch.bfloat16)
    v = torch.zeros(1, 4, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="step_tail: v_pos must be contiguous"):
        ops.cfg_euler_step(torch.zeros(1, 128, 4, dtype=torch.bfloat16).transpose(1, 2), v, x, 4.0, 0.5, 0.25)
    with pytest.raises(ValueError, match=r"step_tail: v_neg must be \(1, 4, 128\)"):
        ops.cfg_euler_step(v, torch.zeros(1, 3, 128, dtype=torch.bfloat16), x, 4.0, 0.5, 0.25)


# -------------------------------------------------------------------------------------------------------------- C ABI
def test_header_binding_and_library_agree_on_the_guider_entries():
    from mlx_video_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ltxk.h")).read()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"^int(64_t)? %s\(" % name, hdr, re.M), f"{name} is not declared in ltxk.h"
    assert _lib.SIGNATURES["ltxk_guidance_sums_workspace_bytes"][0] is ctypes.c_int64
    for name in ("ltxk_guidance_sums", "ltxk_guider_euler_step"):
        assert _lib.SIGNATURES[name][1][0]._type_ is _lib.GuiderArgs
    # the struct as the header declares it, field by field
    body = re.search(r"typedef struct ltxk_guider_args \{(.*?)\} ltxk_guider_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [first.split()[-1].lstrip("*")] + [x.strip().lstrip("*") for x in rest]
    assert names == [f[0] for f in _lib.GuiderArgs._fields_]
    assert int(re.search(r"enum \{ LTXK_GUIDER_CFG_STAR = (\d+)", hdr).group(1)) == _lib.GUIDER_CFG_STAR
    assert int(re.search(r"LTXK_GUIDER_APG = (\d+)", hdr).group(1)) == _lib.GUIDER_APG
    assert int(re.search(r"#define LTXK_GUIDER_RECORD_FLOATS (\d+)", hdr).group(1)) == _lib.GUIDER_RECORD_FLOATS == RG.REC


def test_abi_index_list_stays_closed_and_the_new_struct_reports_its_size():
    from mlx_video_amd import _lib
    lib = _lib.load()
    assert lib.ltxk_abi_sizeof(4) == ctypes.sizeof(_lib.StepArgs) == 96 and _lib.ABI_STRUCTS[4] is _lib.StepArgs
    assert len(_lib.ABI_STRUCTS) == 5 and lib.ltxk_abi_sizeof(5) == -1
    assert lib.ltxk_guider_args_sizeof() == ctypes.sizeof(_lib.GuiderArgs)
    assert lib.ltxk_version() >= 409
