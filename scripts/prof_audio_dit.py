"""Separate audio generation at full size on the device: step times of the audio-only transformer, its kernel families, and the
head-dim-64 attention kernel against the only route the dh = 128 kernel offers for the same mathematics.

    python scripts/prof_audio_dit.py [--out profiles/audio_dit.json] [--no-trace] [--no-video]

Full-size random weights (LTXModelConfig.audio(), L = 48), B = 1, T = 126 latent frames (5 s), S = 1024 context tokens.
  step     ms per denoise step of denoise_audio_only (8 steps per call, a device-synchronised window around each call, median of
           --reps calls after --warmup): eager; with cache_context; with use_graph (and cache_context, as a compiled run hoists it).
  floor    weight_bytes() / 6.3 TB/s: every step streams every weight once - the least time a step can take at M = 126 rows.
  trace    a fresh child process under `rocprofv3 --kernel-trace --stats` runs --trace-steps eager steps; launches per step and
           time per kernel family come from its kernel_stats.csv (the profiler is off in every timed window above).
  attn     ltxk_flash_attn_dh64 against ltxk_flash_attn on q, k, v zero-padded to 128 channels per head (the same scores and, in
           the first 64 channels of each head, the same outputs), alternately in one process: per shape, rounds of --attn-iters
           launches of each arm between events; median, min and max per launch.
  video    a 40-step 512x512x33 guided (CFG) video denoise loop on a full-size random video transformer, timed the same way, and
           the 8-step audio loop as a share of it.
The JSON is rewritten after every section; progress goes to stderr."""
import argparse
import csv
import glob
import json
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT]

import torch

from mlx_video_amd import ops
from mlx_video_amd.denoise import denoise_audio_only, denoise_dev
from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
from mlx_video_amd.schedulers import STAGE_1_SIGMAS, create_audio_position_grid, create_position_grid, ltx2_scheduler

BF = torch.bfloat16
HBM_TBPS = 6.3                       # MI355X achievable HBM3E stream rate used across this project's floors
ATTN_SHAPES = [(1, 32, 126, 126), (1, 32, 126, 1024), (1, 32, 2560, 126)]
FAMILIES = (("gemm", r"gemm|splitk"), ("attention", r"flash_attn"), ("qknorm_rope", r"qknorm"), ("norm_modulate", r"norm_modulate|norm_scale"),
            ("step_tail", r"step|euler|latent_to_tokens"), ("adaln", r"ada_combine|timestep_embed|silu"))


def say(msg):
    print(f"[prof_audio_dit] {msg}", file=sys.stderr, flush=True)


def window(fn, warmup, reps):
    ts = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(s.elapsed_time(e))
    return ts


def audio_inputs(dev, T, S, cfg):
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(1, 8, T, 16, generator=g).to(BF).to(dev)
    ctx = torch.randn(1, S, cfg.caption_channels, generator=g).to(BF).to(dev)
    return lat, create_audio_position_grid(1, T).to(dev), ctx


def family_split(stats_csv, steps):
    rows = list(csv.DictReader(open(stats_csv, newline="")))
    fam = {}
    for r in rows:
        name = next((f for f, pat in FAMILIES if re.search(pat, r["Name"])), "other")
        d = fam.setdefault(name, {"launches_per_step": 0.0, "us_per_step": 0.0})
        d["launches_per_step"] += int(r["Calls"]) / steps
        d["us_per_step"] += float(r["TotalDurationNs"]) / steps / 1e3
    return fam


def attn_ab(dev, iters, rounds):
    out = {}
    for B, H, Tq, Tk in ATTN_SHAPES:
        g = torch.Generator().manual_seed(Tq * 7 + Tk)
        q, k, v = (torch.randn(B, t, H, 64, generator=g).to(BF).to(dev) for t in (Tq, Tk, Tk))
        tkp = (Tk + 63) // 64 * 64

        def operands(dh):
            pad = lambda t: torch.nn.functional.pad(t, (0, dh - 64)).reshape(B * t.shape[1], H * dh).contiguous()
            vt = torch.zeros(B, H * dh, tkp, dtype=BF, device=dev)
            vt[:, :, :Tk] = torch.nn.functional.pad(v, (0, dh - 64)).reshape(B, Tk, H * dh).transpose(1, 2)
            return pad(q), pad(k), vt, torch.empty(B * Tq, H * dh, dtype=BF, device=dev)

        arms = {"dh64": (operands(64), 64), "padded_128": (operands(128), 128)}
        scale = 1.0 / math.sqrt(64)
        run = {n: (lambda o=o, dh=dh: ops.flash_attn(o[0], o[1], o[2], o[3], B, H, Tq, Tk, scale, head_dim=dh)) for n, (o, dh) in arms.items()}
        for f in run.values():
            f()
        torch.cuda.synchronize()
        a = arms["dh64"][0][3].reshape(B, Tq, H, 64).float()
        b = arms["padded_128"][0][3].reshape(B, Tq, H, 128)[..., :64].float()
        ts = {n: [] for n in run}
        for _ in range(rounds):
            for n, f in run.items():                      # alternately, one window of `iters` launches per arm and round
                ts[n] += [t / iters for t in window(lambda: [f() for _ in range(iters)], 1, 1)]
        res = {n: {"us_median": 1e3 * statistics.median(v), "us_min": 1e3 * min(v), "us_max": 1e3 * max(v)} for n, v in ts.items()}
        res["dh64_over_padded_128"] = res["dh64"]["us_median"] / res["padded_128"]["us_median"]
        res["rel_l2_between_arms"] = float((a - b).norm() / b.norm())
        out["x".join(map(str, (B, H, Tq, Tk)))] = res
        say(f"attention {(B, H, Tq, Tk)}: dh64 {res['dh64']['us_median']:.1f} us [{res['dh64']['us_min']:.1f}, {res['dh64']['us_max']:.1f}]  "
            f"padded 128 {res['padded_128']['us_median']:.1f} us [{res['padded_128']['us_min']:.1f}, {res['padded_128']['us_max']:.1f}]  "
            f"ratio {res['dh64_over_padded_128']:.3f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--frames", type=int, default=126)
    ap.add_argument("--context", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--attn-iters", type=int, default=200)
    ap.add_argument("--attn-rounds", type=int, default=7)
    ap.add_argument("--trace-steps", type=int, default=4)
    ap.add_argument("--trace", action="store_true", help="child mode: --trace-steps eager steps and nothing else (run under rocprofv3)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-video", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_dit.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = LTXModelConfig.audio(num_layers=args.layers)
    model = LTXModel.random_init(cfg, dev, seed=5)
    lat, pos, ctx = audio_inputs(dev, args.frames, args.context, cfg)
    if args.trace:
        sig = [1.0 - 0.1 * i for i in range(args.trace_steps + 1)]
        denoise_audio_only(lat, pos, ctx, model, sig, compile_step=True)
        torch.cuda.synchronize()
        return

    def dump(rep):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)

    sig = list(STAGE_1_SIGMAS)
    steps = len(sig) - 1
    rep = {"device": torch.cuda.get_device_name(0), "layers": args.layers, "latent_frames": args.frames, "context_tokens": args.context,
           "steps_per_call": steps, "weight_bytes": model.weight_bytes(), "hbm_tbps_assumed": HBM_TBPS}
    rep["weight_stream_floor_ms_per_step"] = model.weight_bytes() / (HBM_TBPS * 1e12) * 1e3
    cache = {}
    modes = {"eager": dict(compile_step=True), "cache_context": dict(compile_step=True, cache_context=True),
             "use_graph": dict(compile_step=True, use_graph=True, cache_context=True, graph_cache=cache)}
    rep["step_ms"] = {}
    for name, kw in modes.items():
        ts = [t / steps for t in window(lambda: denoise_audio_only(lat, pos, ctx, model, sig, **kw), args.warmup, args.reps)]
        rep["step_ms"][name] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
        say(f"audio step, {name}: {statistics.median(ts):.3f} ms [{min(ts):.3f}, {max(ts):.3f}]; floor {rep['weight_stream_floor_ms_per_step']:.3f} ms")
    rep["audio_loop_ms"] = {k: v["median"] * steps for k, v in rep["step_ms"].items()}
    dump(rep)

    rep["attention_dh64_vs_padded_128"] = attn_ab(dev, args.attn_iters, args.attn_rounds)
    dump(rep)

    if not args.no_trace:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--", sys.executable,
                   os.path.abspath(__file__), "--trace", "--layers", str(args.layers), "--frames", str(args.frames),
                   "--context", str(args.context), "--trace-steps", str(args.trace_steps)]
            rc = subprocess.run(cmd, timeout=280, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if rc != 0 or not files:
                rep["kernel_trace"] = {"error": f"rocprofv3 ended with {rc}, stats files {files}"}
            else:
                fam = family_split(files[0], args.trace_steps)
                rep["kernel_trace"] = {"steps": args.trace_steps, "families": fam,
                                       "launches_per_step": sum(v["launches_per_step"] for k, v in fam.items() if k != "other"),
                                       "kernel_us_per_step": sum(v["us_per_step"] for k, v in fam.items() if k != "other"),
                                       "note": "eager steps, context recomputed every step; the totals leave out `other`, which holds the "
                                               "child process's random-weight construction beside the loop's few torch copies"}
        say(f"kernel trace: {json.dumps(rep['kernel_trace'])}")
        dump(rep)

    if not args.no_video:
        del model
        torch.cuda.empty_cache()
        vcfg = LTXModelConfig(num_layers=args.layers)
        vmodel = LTXModel.random_init(vcfg, dev, seed=6)
        g = torch.Generator().manual_seed(9)
        vlat = torch.randn(1, 128, 5, 16, 16, generator=g).to(BF).to(dev)
        cp, cn = (torch.randn(1, args.context, vcfg.caption_channels, generator=g).to(BF).to(dev) for _ in range(2))
        vpos = create_position_grid(1, 5, 16, 16).to(dev)
        vsig = ltx2_scheduler(40, 5 * 16 * 16)
        ts = window(lambda: denoise_dev(vlat, vpos, cp, cn, vmodel, vsig, cfg_scale=4.0, compile_step=True), 1, 3)
        rep["video_denoise_40_steps_512x512x33_ms"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts),
                                                        "what": "denoise_dev, CFG 4.0, two forwards per step, eager, full-size random weights"}
        rep["audio_loop_share_of_video_denoise"] = {k: v / statistics.median(ts) for k, v in rep["audio_loop_ms"].items()}
        say(f"video denoise loop {statistics.median(ts):.1f} ms; audio loop share {rep['audio_loop_share_of_video_denoise']}")
        dump(rep)
    print(json.dumps(rep, sort_keys=True))


if __name__ == "__main__":
    main()
