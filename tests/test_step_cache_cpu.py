"""The step cache without a GPU (denoise.StepCache, csrc/step_cache.hip):
  * the policy's known answers (StepCache.decide, a pure host function);
  * the numpy float32 emulation of the probe's documented summation order (tests/ref_step_cache.py) against the float64 sum and
    the bound gamma_(depth + 1) * sum |t_i|, with planted faults (a dropped chunk, a merge in the wrong order);
  * the float64 restatement of the cached loop out of oracle.dit's pieces, the yardstick e_ref (the same restatement under the
    bf16 policy against float64; computed, not pinned) and four planted algorithm faults, each of which must move the float64
    latents by at least 2.5 e_ref - twice the 1.25 e_ref band the device is held to;
  * the host surface: CLI, generate_video's refusals, the header, the version literal, _lib.SIGNATURES, the shims' refusals."""
import math
import os
import re
import statistics
import types

import numpy as np
import pytest
import torch

import parity
import ref_step_cache as R
from oracle import dit as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32
INF = math.inf


def _decide(*a, **k):
    from mlx_video_amd.denoise import StepCache
    return StepCache.decide(*a, **k)


def _flags(rels, tau, coefficients=(1.0, 0.0), s_p=1.0):
    """The decisions over a call whose steps 1.. have the relative distances ``rels``."""
    n, acc, out = len(rels) + 1, 0.0, []
    for i in range(n):
        c, a, _ = _decide(i, n, None if i == 0 else rels[i - 1] * s_p, None if i == 0 else s_p, acc, tau, coefficients)
        acc = 0.0 if c else a
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ the policy
def test_policy_known_answers():
    rels = [0.1] * 7                                                     # n = 8
    assert _flags(rels, 0.0) == [True] * 8
    assert _flags([0.0] * 7, 0.0) == [True] * 8                          # tau = 0 never skips, rel = 0 included (0 < 0 is false)
    assert _flags(rels, INF) == [True] + [False] * 6 + [True]
    assert _flags(rels, 0.25) == [True, False, False, True, False, False, True, True]     # 0.1, 0.2, 0.3 >= 0.25: compute, reset
    # the accumulator resets on compute and is carried over a skip
    assert _decide(3, 8, 1.0, 10.0, 0.2, 0.25) == (True, pytest.approx(0.3), 0.1)
    assert _decide(4, 8, 1.0, 10.0, 0.0, 0.25) == (False, 0.1, 0.1)
    # the first and the last step are computed whatever the sums say, and carry no accumulator
    assert _decide(0, 8, 0.0, 1.0, 5.0, INF) == (True, 0.0, None)
    assert _decide(7, 8, 0.0, 1.0, 0.0, INF) == (True, 0.0, 0.0)
    # S_p == 0 and sums that are not finite: compute
    for s_d, s_p in ((1.0, 0.0), (0.0, 0.0), (math.nan, 1.0), (1.0, math.nan), (INF, 1.0), (1.0, INF), (None, None)):
        assert _decide(3, 8, s_d, s_p, 0.0, INF) == (True, 0.0, None)
    # n = 1 and n = 2: nothing to skip
    assert _flags([], INF) == [True] and _flags([0.0], INF) == [True, True]


def test_policy_polynomial_is_numpy_polyval():
    c = (3.5, -2.0, 0.25, 1.5, 0.01)                                     # degree 4, highest first
    for rel in (0.0, 0.013, 0.2, 1.7):
        compute, acc, r = _decide(2, 9, rel * 4.0, 4.0, 0.125, INF, c)
        assert not compute and r == rel and acc == pytest.approx(0.125 + float(np.polyval(c, rel)), rel=1e-14, abs=1e-300)
    assert _decide(2, 9, 1.0, 4.0, 0.0, 1.0, (0.0, 2.0)) == (True, 2.0, 0.25)      # a constant polynomial


def test_step_cache_object():
    from mlx_video_amd.denoise import StepCache
    for bad in (-0.1, math.nan):
        with pytest.raises(ValueError, match="threshold"):
            StepCache(bad)
    for bad in ((), (1.0, math.inf)):
        with pytest.raises(ValueError, match="coefficients"):
            StepCache(0.1, bad)
    with pytest.raises(ValueError, match="schedule"):
        StepCache(0.1, schedule=[False, True])
    sc = StepCache(0.25)
    sc.reset(4)
    assert [sc.step(0, None, None), sc.step(1, 1.0, 10.0), sc.step(2, 2.0, 10.0), sc.step(3, 0.0, 10.0)] == [True, False, True, True]
    assert [r["acc"] for r in sc.report] == [0.0, 0.1, pytest.approx(0.3), 0.0] and sc.counts == {"steps": 4, "computed": 3, "skipped": 1}
    forced = StepCache(0.0, schedule=[True, False, False, True])         # the schedule overrides, the report still carries the policy's numbers
    forced.reset(4)
    assert [forced.step(i, *(s or (None, None))) for i, s in enumerate([None, (1.0, 10.0), (1.0, 10.0), (1.0, 10.0)])] == [True, False, False, True]
    assert [r["rel"] for r in forced.report] == [None, 0.1, 0.1, 0.1]
    with pytest.raises(ValueError, match="schedule"):
        forced.reset(5)


# ------------------------------------------------------------------------------------------------ the summation order
def _spread(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (torch.randn(rows, D, generator=g) * torch.exp2(torch.randint(-12, 9, (rows, D), generator=g).float())).to(BF)
    return mk(), mk()


@pytest.mark.parametrize("rows,D", [(1, 512), (2, 4096), (1025, 8), (5, 4096), (130, 512), (130, 4096)])
def test_order_emulation_inside_the_float64_bound(rows, D):
    cur, prev = _spread(rows, D, rows + D)
    (s_d, s_p), (d64, p64), (b_d, b_p) = R.probe_emulation(cur, prev)
    from mlx_video_amd import ops
    assert (R.CHUNK, R.DEPTH_BASE) == (ops.STEP_CACHE_CHUNK, ops.STEP_CACHE_DEPTH_BASE)       # the emulation is the product's order
    assert R.depth(rows, D) == 40 + -(-rows * D // 8192) - 1 == ops.step_cache_depth(rows, D)
    assert abs(float(s_d) - d64) <= b_d and abs(float(s_p) - p64) <= b_p
    assert b_d < 1e-4 * d64                                               # the bound says something: far below a step's rel
    same = R.probe_emulation(cur, cur)
    assert float(same[0][0]) == 0.0 and same[0][1].tobytes() == R.probe_emulation(prev, cur)[0][1].tobytes()


def test_planted_order_faults_leave_the_bound_or_change_the_bits():
    from mlx_video_amd import ops
    rows, D = 130, 4096                                                  # 65 chunks
    assert R.chunks(rows * D) * 8 == ops.step_cache_workspace_bytes(rows, D) and R.CHUNK == ops.STEP_CACHE_CHUNK
    cur, prev = _spread(rows, D, 9)
    (s_d, s_p), (d64, p64), (b_d, b_p) = R.probe_emulation(cur, prev)
    (f_d, f_p), _, _ = R.probe_emulation(cur, prev, drop_chunk=17)
    assert abs(float(f_d) - d64) > b_d and abs(float(f_p) - p64) > b_p, "a dropped chunk stayed inside the bound"
    (r_d, r_p), _, _ = R.probe_emulation(cur, prev, reverse_merge=True)
    assert r_d.tobytes() != s_d.tobytes() or r_p.tobytes() != s_p.tobytes(), "a merge in descending order gave the same bits"


# ------------------------------------------------------------------------------------------------ the restated loop
CFG = O.DiTConfig(num_layers=2, heads=4, caption_channels=256)
GRID = (2, 6, 6)
SCALE = 4.0


def _loop_inputs(seed=42):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    return mk(1, 128, *GRID), O.create_position_grid(1, *GRID), mk(1, 64, 256), mk(1, 64, 256)


def _sig(n):
    from mlx_video_amd.schedulers import ltx2_scheduler
    return ltx2_scheduler(n, GRID[0] * GRID[1] * GRID[2]).tolist()


def test_restated_pieces_equal_the_oracle():
    """prepare -> blocks -> head is oracle.dit.ltx_forward, bit for bit, under both policies; with every step computed the
    cached loop is oracle.dit.denoise_dev."""
    lat, pos, cp, cn = _loop_inputs()
    W = R.make_weights(CFG, **R.LIVELY)
    pe = O.precompute_freqs_cis(torch.from_numpy(pos), CFG.dim, CFG.theta, CFG.max_pos, CFG.heads)
    tok = O.latent_to_tokens(lat)
    ts = torch.full(tok.shape[:2], 0.71875)
    for p in (O.F64, O.BF16_FLASH):
        st = R.fwd_prepare(tok, ts, cp, pe, W, CFG, p)
        v, hidden = O.ltx_forward(tok, ts, cp, pe, W, CFG, p, return_hidden=True)
        x = R.fwd_blocks(st, W, CFG, p)
        assert torch.equal(x, hidden[-1]) and torch.equal(R.fwd_head(st, x, W, CFG, p), v)
        taps = {}
        O.transformer_block(st["x"], st["ts"], st["ctx"], st["pe"], W, 0, CFG, p, taps=taps)
        assert torch.equal(R.block0_input(st, W, CFG, p), taps["nx1"])
        sig = _sig(3)
        got, rep = R.cached_loop(lat, pos, cp, cn, W, CFG, sig, p, SCALE, decisions=[True] * 3)
        assert torch.equal(got, O.denoise_dev(lat, pos, cp, cn, W, CFG, sig, p, SCALE)) and all(r["computed"] for r in rep)


def _scenario(weights, n, tau_of):
    """(inputs, W, sig, tau, float64 latents, decisions, e_ref) of one correct adaptive run."""
    from mlx_video_amd.denoise import StepCache
    lat, pos, cp, cn = _loop_inputs()
    W, sig = R.make_weights(CFG, **weights), _sig(n)
    run = lambda p, **kw: R.cached_loop(lat, pos, cp, cn, W, CFG, sig, p, SCALE, **kw)
    _, rep0 = run(O.F64, decide=StepCache.decide, threshold=0.0)
    tau = tau_of([r["rel"] for r in rep0[1:]])
    x64, rep = run(O.F64, decide=StepCache.decide, threshold=tau)
    dec = [r["computed"] for r in rep]
    xpol, _ = run(O.BF16_FLASH, decisions=dec)
    return run, tau, x64, dec, parity.rel_l2(xpol, x64)


# fault -> (weights, steps, threshold from the threshold-0 run's rels | None = the forced schedule C S..S C)
FAULT_SCENARIOS = {
    "cache_behind_head": (R.LIVELY, 8, None),
    "shared_residual": (R.LIVELY, 8, None),
    "acc_no_reset": (R.QUIET, 8, lambda rels: 3.3 * statistics.median(rels)),
    "prev_on_computed": (R.QUIET, 8, lambda rels: 4.3 * statistics.median(rels)),
}


@pytest.mark.parametrize("fault", sorted(FAULT_SCENARIOS))
def test_planted_algorithm_faults_move_the_latents(fault):
    """Each planted fault must move the float64 latents by >= 2.5 e_ref, twice the 1.25 e_ref band the device is held to.
    The arithmetic faults run under the forced schedule C S S S S S S C (teacher-forced, so only the arithmetic differs); the
    policy faults decide for themselves, at 3.3 x (accumulator not reset: C SSS C SS C becomes C SSS CCCC) and 4.3 x (prev
    updated on computed steps only: the distances then span several steps and C SSSS C S C becomes C SS C SS C C) the median
    rel of the threshold-0 run, on the QUIET weights, where the latents' drift and not the timestep moves block 0's input."""
    from mlx_video_amd.denoise import StepCache
    weights, n, tau_of = FAULT_SCENARIOS[fault]
    if tau_of is None:
        run, tau, x64, dec, e_ref = _scenario(weights, n, lambda rels: INF)
        assert dec == [True] + [False] * (n - 2) + [True]
        bad, rep = run(O.F64, decisions=dec, fault=fault)
    else:
        run, tau, x64, dec, e_ref = _scenario(weights, n, tau_of)
        bad, rep = run(O.F64, decide=StepCache.decide, threshold=tau, fault=fault)
        assert [r["computed"] for r in rep] != dec, "the fault did not change a decision: the scenario does not aim at it"
    moved = parity.rel_l2(bad, x64)
    print(f"{fault}: e_ref {e_ref:.3e}  moved {moved:.3e}  ratio {moved / e_ref:.2f}  "
          f"{''.join('CS'[not d] for d in dec)} -> {''.join('CS'[not r['computed']] for r in rep)}")
    assert moved >= 2.5 * e_ref


# ------------------------------------------------------------------------------------------------ the host surface
def test_cli_flags():
    from mlx_video_amd.generate import build_parser
    ap = build_parser()
    base = ["--prompt", "x"]
    a = ap.parse_args(base)
    assert a.step_cache_threshold is None and a.step_cache_coefficients is None
    a = ap.parse_args(base + ["--step-cache-threshold", "0.15", "--step-cache-coefficients", "2.5", "-1", "0.5"])
    assert a.step_cache_threshold == 0.15 and a.step_cache_coefficients == [2.5, -1.0, 0.5]
    assert ap.parse_args(base + ["--step-cache-threshold", "inf"]).step_cache_threshold == INF
    for bad in (["--step-cache-threshold", "-1"], ["--step-cache-threshold", "nan"], ["--step-cache-coefficients", "inf"],
                ["--step-cache-coefficients"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad)


def test_generate_video_and_pipeline_config_surface():
    import inspect
    from mlx_video_amd import pipelines
    from mlx_video_amd.generate import generate_video
    sig = inspect.signature(generate_video)
    assert sig.parameters["step_cache_threshold"].default is None and sig.parameters["step_cache_coefficients"].default is None
    with pytest.raises(ValueError, match="step_cache_threshold"):
        generate_video(prompt="x", step_cache_coefficients=[1.0, 0.0])
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError, match="threshold"):
            generate_video(prompt="x", step_cache_threshold=bad)
    with pytest.raises(ValueError, match="coefficients"):             # an empty polynomial is refused, not read as the default
        generate_video(prompt="x", step_cache_threshold=0.1, step_cache_coefficients=[])
    with pytest.raises(ValueError, match="joint.*step cache"):
        generate_video(prompt="x", pipeline="dev", audio=True, audio_mode="joint",
                       av_transformer=types.SimpleNamespace(video=object()), step_cache_threshold=0.1)
    seen = {}
    cfg = pipelines.MLXPipelineConfig(step_cache_threshold=0.2, step_cache_coefficients=(1.0, 0.0))
    orig = pipelines.generate_video
    pipelines.generate_video = lambda **kw: seen.update(kw)
    try:
        pipelines.run_generate("x", pipelines.PipelineType.DEV, cfg, "out.npy")
        assert seen["step_cache_threshold"] == 0.2 and seen["step_cache_coefficients"] == (1.0, 0.0)
        seen.clear()
        pipelines.run_generate("x", pipelines.PipelineType.DEV, pipelines.MLXPipelineConfig(), "out.npy")
        assert "step_cache_threshold" not in seen and "step_cache_coefficients" not in seen        # off: today's call
    finally:
        pipelines.generate_video = orig
    assert pipelines.DistilledPipeline(step_cache_threshold=0.3)._cfg().step_cache_threshold == 0.3


def test_loops_that_refuse_a_step_cache():
    from mlx_video_amd.denoise import StepCache, denoise_audio_only, denoise_dev_av
    from mlx_video_amd.sharding import CfgPairSharding
    sc = StepCache(0.1)
    with pytest.raises(ValueError, match="joint.*step cache"):
        denoise_dev_av(None, None, None, None, None, None, None, None, None, [1.0, 0.0], step_cache=sc)
    with pytest.raises(ValueError, match="audio-only.*step cache"):
        denoise_audio_only(None, None, None, None, [1.0, 0.0], step_cache=sc)
    with pytest.raises(ValueError, match="step cache.*sharded"):
        CfgPairSharding.__new__(CfgPairSharding).denoise_dev(None, None, None, None, None, [1.0, 0.0], step_cache=sc)


def test_header_version_and_signatures():
    import ctypes
    from mlx_video_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ltxk.h")).read()
    assert "#define LTXK_VERSION 412" in hdr
    assert re.search(r"enum \{ LTXK_PROBE_INIT = 1 \}", hdr) and _lib.PROBE_INIT == 1
    lib = _lib.load()
    for name in ("ltxk_step_cache_workspace_bytes", "ltxk_step_cache_depth", "ltxk_step_cache_probe", "ltxk_residual_store",
                 "ltxk_residual_apply"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf"\b{name}\(", hdr), name
    assert _lib.SIGNATURES["ltxk_step_cache_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32])
    assert _lib.SIGNATURES["ltxk_step_cache_depth"] == (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int32])
    assert len(_lib.SIGNATURES["ltxk_step_cache_probe"][1]) == 9 and _lib.SIGNATURES["ltxk_step_cache_probe"][1][2] is ctypes.c_int64
    assert "step_cache.hip" in open(os.path.join(ROOT, "mlx-video_amd", "csrc", "Makefile")).read()
    # the size functions: the library, the binding and the tests' emulation cut (rows, D) alike; bad shapes are -1 / ValueError
    from mlx_video_amd import ops
    for rows, D in ((1, 8), (1, 512), (2, 4096), (1025, 8), (130, 4096), (2560, 4096)):
        assert lib.ltxk_step_cache_workspace_bytes(rows, D) == ops.step_cache_workspace_bytes(rows, D) == 8 * R.chunks(rows * D)
        assert lib.ltxk_step_cache_depth(rows, D) == ops.step_cache_depth(rows, D) == R.depth(rows, D)
    for rows, D in ((0, 512), (4, 12), (4, 0), (1 << 33, 8)):
        assert lib.ltxk_step_cache_workspace_bytes(rows, D) == -1 and lib.ltxk_step_cache_depth(rows, D) == -1
        with pytest.raises(ValueError, match="step_cache_workspace_bytes"):
            ops.step_cache_workspace_bytes(rows, D)
        with pytest.raises(ValueError, match="step_cache_depth"):
            ops.step_cache_depth(rows, D)


def _z(*shape, dtype=BF):
    return torch.zeros(shape, dtype=dtype)


def _odd(t):
    """The same shape, one element past a 16-byte boundary."""
    flat = torch.zeros(t.numel() + 8, dtype=t.dtype)
    out = flat[1:1 + t.numel()].view(t.shape)
    assert flat.data_ptr() % 16 == 0 and out.data_ptr() % 16 != 0
    return out


def test_probe_shim_refusals():
    from mlx_video_amd import _lib, ops
    rows, D = 5, 4096
    nws = ops.step_cache_workspace_bytes(rows, D) // 4
    good = lambda: dict(cur=_z(rows, D), prev=_z(rows, D), sums=_z(2, dtype=F32), workspace=_z(nws, dtype=F32))
    call = lambda **over: ops.step_cache_probe(**{**good(), **over})
    with pytest.raises(_lib.LtxkError, match="step_cache_probe: cur must be a device tensor.*no CPU fallback"):
        call()
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        ops.step_cache_probe(_z(rows, D), _z(rows, D), None, None, init=True)
    with pytest.raises(ValueError, match="sums and workspace are required"):
        ops.step_cache_probe(_z(rows, D), _z(rows, D), None, None)
    for over, exc, msg in ((dict(cur=_z(rows, D, dtype=F32)), TypeError, "cur must be torch.bfloat16"),
                           (dict(prev=_z(rows, D, dtype=torch.float16)), TypeError, "prev must be torch.bfloat16"),
                           (dict(sums=_z(2)), TypeError, "sums must be torch.float32"),
                           (dict(workspace=_z(nws, dtype=torch.int32)), TypeError, "workspace must be torch.float32"),
                           (dict(cur=_z(rows * D)), ValueError, "cur must have 2 dimensions"),
                           (dict(prev=_z(rows + 1, D)), ValueError, r"prev must be \(5, 4096\)"),
                           (dict(sums=_z(3, dtype=F32)), ValueError, r"sums must be \(2,\)"),
                           (dict(workspace=_z(nws - 1, dtype=F32)), ValueError, rf"workspace must be \(>={nws},\)"),
                           (dict(cur=_z(rows, 2 * D)[:, :D]), ValueError, "cur must be contiguous"),
                           (dict(prev=_z(D, rows).t()), ValueError, "prev must be contiguous"),
                           (dict(cur=_odd(_z(rows, D))), ValueError, "cur must be 16-byte aligned"),
                           (dict(prev=_odd(_z(rows, D))), ValueError, "prev must be 16-byte aligned"),
                           (dict(cur=_z(rows, 12), prev=_z(rows, 12)), ValueError, "D = 12 a positive multiple of 8"),
                           (dict(cur=_z(0, D), prev=_z(0, D)), ValueError, "rows = 0 must be positive"),
                           (dict(cur="x"), TypeError, "cur and prev must be tensors")):
        with pytest.raises(exc, match=msg):
            call(**over)


@pytest.mark.parametrize("shim", ["residual_store", "residual_apply"])
def test_residual_shim_refusals(shim):
    from mlx_video_amd import _lib, ops
    fn = getattr(ops, shim)
    with pytest.raises(_lib.LtxkError, match=f"{shim}: x must be a device tensor.*no CPU fallback"):
        fn(_z(4, 512), _z(4, 512))
    for x, r, exc, msg in ((_z(4, 512, dtype=F32), _z(4, 512), TypeError, "x must be torch.bfloat16"),
                           (_z(4, 512), _z(4, 512, dtype=F32), TypeError, "r must be torch.bfloat16"),
                           (_z(4, 512), _z(4, 256), ValueError, r"r must be \(4, 512\)"),
                           (_z(4, 512), _z(2048), ValueError, "r must have 2 dimensions"),
                           (_z(3, 4), _z(3, 4), ValueError, "positive multiple of 8 elements"),
                           (_z(0, 8), _z(0, 8), ValueError, "positive multiple of 8 elements"),
                           (_z(4, 1024)[:, :512], _z(4, 512), ValueError, "x must be contiguous"),
                           (_z(4, 512), _z(512, 4).t(), ValueError, "r must be contiguous"),
                           (_odd(_z(4, 512)), _z(4, 512), ValueError, "x must be 16-byte aligned"),
                           (_z(4, 512), _odd(_z(4, 512)), ValueError, "r must be 16-byte aligned"),
                           (None, _z(4, 512), TypeError, "x and r must be tensors")):
        with pytest.raises(exc, match=msg):
            fn(x, r)
