"""Step cache (denoise.StepCache): what a computed step, a skipped step and the probe cost at the bench shape.

Full-size random weights (L = 48), 512x512x33 (N = 1280 tokens, S = 1024 text tokens), 40 steps, cfg_batch, the captured step.
The arms alternate in ONE process, each window bracketed by device synchronisation:
  off       the parent's loop (measured twice: the second series against the first is the spread every difference is read against)
  zero      threshold 0: every step computed, plus the probe graph and the host read of the two sums
  every2    forced schedule C S C S ... C C
  ends      forced schedule C S S ... S C
From the four: ms per computed step (off / 40), the probe's cost per step (zero - off) / 40 - a cost only where it exceeds the
off arm's own spread (the min - max over both off series, and the difference of their medians) -, ms per skipped step from
`ends`, once with the step's probe replay and host read in it (what a skipped step costs the loop) and once with the probe's
measured cost taken out (the skip body alone), and the time per video of each arm.  The off arm runs with cache_context, which
a step cache implies, so that the arms differ by the cache alone.  With random weights the
ADAPTIVE skip rate says nothing about real prompts, so no adaptive arm is timed.  Writes profiles/step_cache.json.

    python scripts/ab_step_cache.py [--layers 48] [--steps 40] [--rounds 5] [--out profiles/step_cache.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_cache.json"))
    a = ap.parse_args()
    from mlx_video_amd.denoise import StepCache, denoise_dev
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    from mlx_video_amd.schedulers import create_position_grid, ltx2_scheduler
    dev = torch.device("cuda:0")
    model = LTXModel.random_init(LTXModelConfig(num_layers=a.layers), dev)
    g = torch.Generator(device=dev).manual_seed(43)
    F, H, W, n = 5, 16, 16, a.steps
    lat = torch.randn((1, 128, F, H, W), generator=g, device=dev).to(torch.bfloat16)
    cp = torch.randn((1, 1024, 3840), generator=g, device=dev).to(torch.bfloat16)
    cn = torch.randn((1, 1024, 3840), generator=g, device=dev).to(torch.bfloat16)
    pos = create_position_grid(1, F, H, W).to(dev)
    sig = ltx2_scheduler(n, F * H * W)
    every2 = [i % 2 == 0 or i == n - 1 for i in range(n)]
    ends = [i == 0 or i == n - 1 for i in range(n)]
    arms = {"off": None, "zero": lambda: StepCache(0.0), "every2": lambda: StepCache(0.0, schedule=every2),
            "ends": lambda: StepCache(0.0, schedule=ends), "off_again": None}
    caches = {k: {} for k in arms}

    def run(name):
        sc = arms[name]() if arms[name] is not None else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=True, use_graph=True,
                    graph_cache=caches[name], cache_context=True, step_cache=sc)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, (sc.counts if sc is not None else None)

    for name in arms:                      # warm-up: the captures
        run(name)
    ms = {k: [] for k in arms}
    counts = {}
    for _ in range(a.rounds):
        for name in arms:
            t, c = run(name)
            ms[name].append(t)
            counts[name] = c
    stat = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "counts": counts[k]} for k, v in ms.items()}
    off = stat["off"]["median_ms"]
    both_off = ms["off"] + ms["off_again"]
    spread = max(max(both_off) - min(both_off), abs(stat["off_again"]["median_ms"] - off))
    skipped_ends = n - 2
    per_computed = off / n
    probe = (stat["zero"]["median_ms"] - off) / n
    per_skipped_with_probe = (stat["ends"]["median_ms"] - 2 * (per_computed + max(probe, 0.0))) / skipped_ends
    per_skipped = per_skipped_with_probe - max(probe, 0.0)
    out = {"shape": {"layers": a.layers, "tokens": F * H * W, "text_tokens": 1024, "steps": n, "cfg_batch": True, "graph": True},
           "rounds": a.rounds, "arms": stat, "off_spread_ms": spread, "off_min_ms": min(both_off), "off_max_ms": max(both_off),
           "off_median_difference_ms": abs(stat["off_again"]["median_ms"] - off),
           "ms_per_computed_step": per_computed, "ms_probe_and_host_read_per_step": probe,
           "probe_exceeds_off_spread": bool(stat["zero"]["median_ms"] - off > spread),
           "ms_per_skipped_step_with_probe_and_host_read": per_skipped_with_probe,
           "ms_per_skipped_step_body_alone": per_skipped,
           "ms_per_video": {k: v["median_ms"] for k, v in stat.items()},
           "note": "random weights: the adaptive policy's skip rate says nothing about real prompts and is not timed"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
