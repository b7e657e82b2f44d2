"""Cost of spatio-temporal guidance (STG) per dev denoise step: 512x512x33 (1280 video tokens), synthetic weights, cfg_batch,
whole-step graph replay.  Three forms in interleaved rounds in one process:
  cfg       - CFG only: one B=2 forward [pos, neg] per step (today's step)
  stg29     - CFG + STG with stg_blocks=[29]: one B=3 forward [pos, neg, pos+]; block 29 of the perturbed row skips attention
  stg_all   - CFG + STG with every block skipped in the perturbed row
Prints one JSON line per form (median / min ms per step over the rounds) and the ratios to `cfg`.
  python scripts/prof_stg_step.py [--layers 48] [--steps 8] [--rounds 3] [--only stg29]
Under `rocprofv3 --kernel-trace --stats -- python scripts/prof_stg_step.py --only stg29 --rounds 1` the stats list the
value-passthrough kernel (value_passthrough_kernel) and the step tail (step_tail_kernel<0, true>; <0, false> for `cfg`) beside the
step's other kernels."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mlx_video_amd.denoise import denoise_dev  # noqa: E402
from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig  # noqa: E402
from mlx_video_amd.schedulers import create_position_grid, ltx2_scheduler  # noqa: E402

FORMS = {"cfg": dict(stg_scale=0.0), "stg29": dict(stg_scale=1.0, stg_blocks=[29]), "stg_all": dict(stg_scale=1.0, stg_blocks=None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=sorted(FORMS), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    forms = {a.only: FORMS[a.only]} if a.only else FORMS
    if a.layers <= 29:
        forms = {k: (dict(v, stg_blocks=[a.layers - 1]) if v.get("stg_blocks") else v) for k, v in forms.items()}
    model = LTXModel.random_init(LTXModelConfig(num_layers=a.layers), dev, seed=1234)
    F, H, W = 5, 16, 16                                   # 33 frames, 512x512 -> 5 x 16 x 16 latent
    g = torch.Generator(device=dev).manual_seed(1)
    lat = torch.randn((1, 128, F, H, W), generator=g, device=dev).to(torch.bfloat16)
    cp = torch.randn((1, 1024, 3840), generator=g, device=dev).to(torch.bfloat16)
    cn = torch.randn((1, 1024, 3840), generator=g, device=dev).to(torch.bfloat16)
    pos = create_position_grid(1, F, H, W).to(dev)
    sig = ltx2_scheduler(40, F * H * W)[: a.steps + 1]
    cache = {}

    def run(kw):
        return denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=4.0, compile_step=True, cfg_batch=True, use_graph=True,
                           graph_cache=cache, **kw)

    for kw in forms.values():           # capture every form's step graph (its first step runs eagerly)
        run(kw)
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, kw in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(kw)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
            assert bool(torch.isfinite(out.float()).all()), k
    res = {}
    for k, t in times.items():
        t = sorted(t)
        res[k] = {"form": k, "layers": a.layers, "tokens": F * H * W, "steps": a.steps, "rounds": a.rounds,
                  "ms_per_step_median": t[len(t) // 2], "ms_per_step_min": t[0], "stg_blocks": forms[k].get("stg_blocks", "-")}
    if "cfg" in res:
        for k in res:
            res[k]["ratio_to_cfg"] = res[k]["ms_per_step_median"] / res["cfg"]["ms_per_step_median"]
    for r in res.values():
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
