"""Cost of the CFG* / APG guiders per dev denoise step: 512x512x33 (1280 video tokens), synthetic weights, cfg_batch, whole-step
graph replay.  Forms, in interleaved rounds in one process:
  cfg        - plain CFG: today's fused step tail (one launch)
  cfg_star   - CFGStarRescalingGuider: one reduction pass (2 launches) + the guider tail
  apg        - LtxAPGGuider, eta 0.5, no norm clamp: one reduction pass + the guider tail
  apg_clamp  - LtxAPGGuider, eta 0.5, norm_threshold 10: two reduction passes (4 launches) + the guider tail
Prints one JSON line per form (median / min ms per step over the rounds) and the differences to `cfg`.
  python scripts/prof_guiders_step.py [--layers 48] [--steps 8] [--rounds 5] [--forms cfg apg] [--root OTHER_CHECKOUT]
`--root`: import the package from another checkout (built there) - `--forms cfg --root <parent commit>` measures the parent's
CFG step with the same script; `cfg` passes no guider keyword, so it runs on a commit that has none.
Under `rocprofv3 --kernel-trace --stats -- python scripts/prof_guiders_step.py --forms cfg_star apg_clamp --rounds 1` the stats
list guider_partial_kernel, guider_finish_kernel and the step tail (step_tail_kernel<guider, STG>; 0 = plain CFG) beside the step's
other kernels."""
import argparse
import json
import os
import sys
import time

FORMS = {"cfg": {}, "cfg_star": dict(guider="cfg_star"), "apg": dict(guider="apg", apg_eta=0.5),
         "apg_clamp": dict(guider="apg", apg_eta=0.5, apg_norm_threshold=10.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cfg-scale", type=float, default=6.0)
    ap.add_argument("--forms", nargs="+", choices=sorted(FORMS), default=list(FORMS))
    ap.add_argument("--root", type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", type=str, default="this")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from mlx_video_amd.denoise import denoise_dev
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    from mlx_video_amd.schedulers import create_position_grid, ltx2_scheduler

    dev = torch.device("cuda:0")
    forms = {k: FORMS[k] for k in a.forms}
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
        return denoise_dev(lat, pos, cp, cn, model, sig, cfg_scale=a.cfg_scale, compile_step=True, cfg_batch=True, use_graph=True,
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
        res[k] = {"tree": a.tag, "form": k, "layers": a.layers, "tokens": F * H * W, "steps": a.steps, "rounds": a.rounds,
                  "cfg_scale": a.cfg_scale, "ms_per_step_median": t[len(t) // 2], "ms_per_step_min": t[0], "ms_per_step_max": t[-1]}
    if "cfg" in res:
        for k in res:
            res[k]["us_over_cfg"] = (res[k]["ms_per_step_median"] - res["cfg"]["ms_per_step_median"]) * 1e3
    for r in res.values():
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
