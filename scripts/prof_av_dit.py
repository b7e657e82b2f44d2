"""Joint audio-video denoising at full size on random weights: L = 48, B = 2 (cfg_batch), N = 1280 video tokens
(512x512x33), Ta = compute_audio_frames(33, 24) audio frames, S = 1024.

  python3 scripts/prof_av_dit.py [--layers 48] [--out profiles/av_dit.json]     the timing report
  python3 scripts/prof_av_dit.py --trace                                        three eager joint steps and nothing else (to run
                                                                                under rocprofv3 --kernel-trace --stats)
Timing: warm-up, then device-synchronised windows (perf_counter around a synchronised run of ``reps`` steps), median with
min-max over ``rounds`` windows.  Arms that are compared alternate inside one process, and the baseline is also compared with
itself (two interleaved series of the same arm) to show the spread a difference has to exceed."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mlx_video_amd import ops
from mlx_video_amd.av_model import LTXAVModel
from mlx_video_amd.denoise import _AVStep, _AVStepGraph, _Guidance, _StepPlan, audio_latent_to_volume
from mlx_video_amd.ltx_model import LTXModelConfig, precompute_freqs_cis
from mlx_video_amd.schedulers import compute_audio_frames, create_audio_position_grid, create_position_grid, ltx2_scheduler

BF = torch.bfloat16
dev = torch.device("cuda:0")


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def series(fns, reps, rounds, warm=2):
    """fns: {name: callable}; the arms alternate round by round.  -> {name: {"median", "min", "max"}} in ms per call."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(window(fn, reps))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    L, F, H, W, S = a.layers, 5, 16, 16, 1024
    N, Ta = F * H * W, compute_audio_frames(33, 24.0)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev).to(BF)
    model = LTXAVModel.random_init(LTXModelConfig(num_layers=L), LTXModelConfig.audio(num_layers=L), dev)
    V, A = model.video, model.audio
    lat_v, lat_a = rnd(1, 128, F, H, W), rnd(1, 8, Ta, 16)
    vol_a = audio_latent_to_volume(lat_a)
    ctx = [rnd(1, S, 3840) for _ in range(4)]
    sig = [float(s) for s in ltx2_scheduler(8, N).tolist()]
    vpos, apos = create_position_grid(1, F, H, W).to(dev), create_audio_position_grid(1, Ta).to(dev)
    tables = (precompute_freqs_cis(vpos, V.inner_dim, V.positional_embedding_theta, V.positional_embedding_max_pos, V.num_attention_heads),
              model.cross_freqs_cis(vpos, V.num_attention_heads),
              precompute_freqs_cis(apos, A.inner_dim, A.positional_embedding_theta, A.positional_embedding_max_pos, A.num_attention_heads),
              model.cross_freqs_cis(apos, A.num_attention_heads))
    gd = _Guidance(1, 4.0, True, 0.0, None, None)
    plan_v, plan_a = _StepPlan(lat_v, None, gd.reps, sig), _StepPlan(vol_a, None, gd.reps, sig)
    ctx_v, ctx_a = [torch.cat(ctx[0:2], 0)], [torch.cat(ctx[2:4], 0)]
    step = _AVStep(model, gd)

    def joint_eager():
        (vp, vn), (ap_, an) = step.velocities(lat_v, vol_a, plan_v.timestep_plan(0), plan_a.timestep_plan(0), ctx_v, ctx_a, tables)
        gd.tail(vp, vn, None, lat_v, plan_v.sig_bf[0], plan_v.sig_bf[1], None, None)
        gd.tail(ap_, an, None, vol_a, plan_v.sig_bf[0], plan_v.sig_bf[1], None, None)

    if a.trace:
        for _ in range(3):
            joint_eager()
        torch.cuda.synchronize()
        return

    def video_eager():
        vp, vn, _ = gd.velocities(V, lat_v, plan_v.timestep_plan(0), tables[0], ctx_v[0], None, None, None, None, None)
        gd.tail(vp, vn, None, lat_v, plan_v.sig_bf[0], plan_v.sig_bf[1], None, None)

    gd1 = _Guidance(1, 1.0, False, 0.0, None, None)
    plan_a1 = _StepPlan(vol_a, None, 1, sig)

    def audio_eager():                                   # one step of the separate audio phase: B = 1, no CFG
        vp, _, _ = gd1.velocities(A, vol_a, plan_a1.timestep_plan(0), tables[2], None, None, ctx[2], None, None, None)
        gd1.tail(vp, None, None, vol_a, plan_v.sig_bf[0], plan_v.sig_bf[1], None, None)

    rep = {"shape": {"layers": L, "B": 2, "N": N, "Ta": Ta, "S": S}, "weight_bytes": model.weight_bytes()}
    rep["step_ms"] = series({"joint_eager": joint_eager, "video_only_eager": video_eager, "audio_only_b1_eager": audio_eager,
                             "joint_eager_again": joint_eager}, 2, a.rounds)
    # the captured joint step: one run builds the graph (8 steps), then bare replays
    ent = _AVStepGraph(lat_v, vol_a, plan_v, plan_a, model, ctx_v, ctx_a, gd)
    ent.run(lat_v, vol_a, plan_v, plan_a, ctx_v, ctx_a, tables)
    ent.inp_v.step.zero_()
    ent.inp_a.step.zero_()
    rep["step_ms"].update(series({"joint_graph": ent.graph.replay}, 4, a.rounds))
    # launch count and per-family kernel time of one eager joint step (HIP events around every launch)
    ops.TIMER = ops.KernelTimer()
    joint_eager()
    fam = ops.TIMER.summary()
    ops.TIMER = None
    rep["families_one_eager_step"] = {k: {"launches": v["launches"], "ms": v["ms"]} for k, v in sorted(fam.items())}
    rep["launches_timed_families"] = sum(v["launches"] for v in fam.values())
    # the two cross attentions alone, and v2a's shape at Tk = 5184
    Da, Hh = A.inner_dim, A.num_attention_heads

    def attn(Tq, Tk):
        q, k, o = rnd(2 * Tq, Da), rnd(2 * Tk, Da), torch.empty((2 * Tq, Da), dtype=BF, device=dev)
        vt = rnd(2, Da, (Tk + 63) // 64 * 64)
        return lambda: ops.flash_attn(q, k, vt, o, 2, Hh, Tq, Tk, 1 / math.sqrt(64), head_dim=64)

    rep["cross_attn_us"] = {k: {m: x * 1e3 for m, x in v.items()} for k, v in series(
        {f"a2v_{N}x{Ta}": attn(N, Ta), f"v2a_{Ta}x{N}": attn(Ta, N), f"v2a_{Ta}x5184": attn(Ta, 5184)}, 200, a.rounds).items()}
    # ltxk_rmsnorm_modulate2 against the two ltxk_rmsnorm_modulate_ss launches it replaces
    rep["modulate2_us"] = {}
    for M, D in ((2 * N, 4096), (2 * Ta, 2048)):
        xs = [rnd(M, D) for _ in range(8)]
        ss = [(x.float() ** 2).reshape(M, D // 64, 64).sum(-1).contiguous() for x in xs]
        mod = rnd(1, 5, D)
        y0, y1 = torch.empty_like(xs[0]), torch.empty_like(xs[0])
        it = [0]

        def two():
            i = it[0] = (it[0] + 1) % 8
            ops.rmsnorm_modulate(xs[i], 1e-6, mod[:, 0], mod[:, 1], 5 * D, None, out=y0, sumsq=ss[i], scale_is_one_plus=True)
            ops.rmsnorm_modulate(xs[i], 1e-6, mod[:, 2], mod[:, 3], 5 * D, None, out=y1, sumsq=ss[i], scale_is_one_plus=True)

        def one():
            i = it[0] = (it[0] + 1) % 8
            ops.rmsnorm_modulate(xs[i], 1e-6, mod[:, 0], mod[:, 1], 5 * D, None, out=y0, sumsq=ss[i], scale_is_one_plus=True,
                                 scale2=mod[:, 2], shift2=mod[:, 3], out2=y1)

        r = series({"two_launches": two, "modulate2": one, "two_launches_again": two}, 200, 7)
        rep["modulate2_us"][f"{M}x{D}"] = {k: {m: x * 1e3 for m, x in v.items()} for k, v in r.items()}
    print(json.dumps(rep, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
