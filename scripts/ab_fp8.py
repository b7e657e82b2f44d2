"""Interleaved A/B of the whole L=48 DiT forward with bf16 weights against FP8 (e4m3, per-channel scale) weight panels
(DESIGN.md 5g): graph replays at M = 64 and M = 320 rows (B=1: the small-M split-K weight streams) and at the bench shape
M = 2560 (B=2, N=1280), S = 1024 text tokens.  One process, the two models interleaved round by round; median / min / max per
variant, the fp8 / bf16 ratio, and both models' weight_bytes().  The whole run is under a time limit (SIGALRM).
usage: python scripts/ab_fp8.py [--layers 48] [--rounds 9] [--limit 420] [--out FILE.json]"""
import argparse, json, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
BF = torch.bfloat16
dev = torch.device("cuda:0")
def say(*a):
    print(" ".join(str(x) for x in a), flush=True)

def timeit(fn, rounds, variants):
    ts = {k: [] for k in variants}
    for r in range(rounds):
        for k in variants:
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(k); e.record(); torch.cuda.synchronize()
            ts[k].append(s.elapsed_time(e))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--limit", type=int, default=420, help="seconds after which the run is abandoned")
    ap.add_argument("--scaling", default="channel", choices=["channel", "none"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    def expired(*_):
        say(f"time limit of {args.limit} s reached: abandoning the run")
        os._exit(3)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig, TimestepPlan, precompute_freqs_cis
    from mlx_video_amd.schedulers import create_position_grid
    from mlx_video_amd.weights import quantize_transformer_weights
    t0 = time.time()
    cfg = LTXModelConfig(num_layers=args.layers)
    W = LTXModel.random_weights(cfg, dev, seed=1234)
    models = {"bf16": LTXModel(cfg, W), "fp8": LTXModel(cfg, quantize_transformer_weights(W, args.scaling))}
    del W
    torch.cuda.empty_cache()
    res = {"layers": args.layers, "scaling": args.scaling, "weight_bytes": {k: m.weight_bytes() for k, m in models.items()}, "shapes": {}}
    say(f"models built in {time.time() - t0:.1f} s; weight_bytes bf16 {res['weight_bytes']['bf16']}  fp8 {res['weight_bytes']['fp8']}  "
        f"ratio {res['weight_bytes']['fp8'] / res['weight_bytes']['bf16']:.4f}")
    S = 1024
    for B, F, Hh, Ww in ((1, 1, 8, 8), (1, 5, 8, 8), (2, 5, 16, 16)):
        N = F * Hh * Ww
        pe = precompute_freqs_cis(create_position_grid(1, F, Hh, Ww).to(dev), 4096)
        g = torch.Generator(device=dev).manual_seed(B * 1000 + N)
        tok = torch.randn((B, N, 128), generator=g, device=dev).to(BF)
        ctx = torch.randn((B, S, 3840), generator=g, device=dev).to(BF)
        plan = TimestepPlan(torch.tensor([0.625], dtype=BF, device=dev), torch.zeros(B * N, dtype=torch.int32, device=dev))
        graphs, outs = {}, {}
        for name, model in models.items():
            s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                model.forward_tokens(tok, plan, ctx, pe)
            torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                outs[name] = model.forward_tokens(tok, plan, ctx, pe)
            graphs[name] = gr
        for n_ in graphs: graphs[n_].replay()
        torch.cuda.synchronize()
        rel = float((outs["fp8"].float() - outs["bf16"].float()).norm() / outs["bf16"].float().norm())
        t = timeit(lambda k_: graphs[k_].replay(), args.rounds, list(graphs))
        for kname, (med, mn, mx) in t.items():
            say(f"forward M={B * N:5d} (B={B} N={N}) S={S} {kname:5s} median {med:8.3f} ms  min {mn:8.3f}  max {mx:8.3f}")
        ratio = t["fp8"][0] / t["bf16"][0]
        say(f"forward M={B * N:5d} fp8 / bf16 = {ratio:.4f}   rel-L2(fp8 output, bf16 output) = {rel:.3e}")
        res["shapes"][str(B * N)] = {"B": B, "N": N, "bf16_ms": t["bf16"], "fp8_ms": t["fp8"], "ratio": ratio, "rel_l2": rel}
        del graphs, outs
        torch.cuda.empty_cache()
    signal.alarm(0)
    say(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

if __name__ == "__main__":
    main()
