"""Interleaved three-arm A/B of the whole L=48 DiT forward: bf16 weights, FP8 weights with FP8 activations (W8A8,
--enable-fp8 --fp8-activations) and MXFP4 in-block GEMMs (--enable-mxfp4).  Random N(0, 0.02^2) weights, D = 4096, S = 1024 text
tokens; graph replays at M = 2560 (B=2, N=1280: the bench shape), M = 1280 and M = 320; one process, the arms interleaved round by
round; median / min / max per arm, the ratios to bf16 and to W8A8, the relative L2 of each quantised arm's output to the bf16
output, and weight_bytes() of the three models.
--profile: afterwards, one `rocprofv3 --kernel-trace --stats` run per arm of the M = 2560 forward (a fresh child process each,
this script with --trace ARM after `--`) and the per-family split of its kernel time (GEMM family, quantiser family, attention,
the rest).  No counter pass is made here.  The whole run is under a time limit (SIGALRM); every child has its own.
usage: python scripts/ab_mxfp4_dit.py [--layers 48] [--rounds 9] [--limit 540] [--profile] [--out profiles/mxfp4_dit.json]"""
import argparse, csv, glob, json, os, signal, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
BF = torch.bfloat16
dev = torch.device("cuda:0")
ARMS = ("bf16", "w8a8", "mxfp4")
SHAPES = ((2, 5, 16, 16), (1, 5, 16, 16), (1, 5, 8, 8))          # M = 2560, 1280, 320
def family(name):
    """Kernel family by name (mangled or demangled spelling of the W8 / A8 template flags of the GEMM kernels)."""
    if "quant_rows_mxfp4" in name:
        return "quant_rows_mxfp4"
    if "quant_rows_fp8" in name:
        return "quant_rows_fp8"
    if "gemm_mxfp4_kernel" in name:
        return "gemm_mxfp4"
    if "gemm_bf16_kernel" in name:
        if "Lb1ELb1E" in name or "true, true>" in name:
            return "gemm_w8a8"
        return "gemm_w8a16" if ("Lb1ELb0E" in name or "true, false>" in name) else "gemm_bf16"
    if "gemm_stream_kernel" in name:
        return "gemm_w8a16" if ("ELb1E" in name or "true>" in name) else "gemm_bf16"
    if "gemm_" in name or "splitk_epilogue" in name:
        return "gemm_bf16"
    if "flash" in name or "attn" in name:
        return "attention"
    return "other (norms, rope; and the child's model construction and quantisation)"

def say(*a):
    print(" ".join(str(x) for x in a), flush=True)

def build(arms, layers):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    from mlx_video_amd.weights import quantize_transformer_weights, quantize_transformer_weights_mxfp4
    cfg = LTXModelConfig(num_layers=layers)
    W = LTXModel.random_weights(cfg, dev, seed=1234)
    models = {}
    for a in arms:
        if a == "bf16":
            models[a] = LTXModel(cfg, W)
        elif a == "w8a8":
            models[a] = LTXModel(cfg, quantize_transformer_weights(W, "channel"), fp8_activations=True)
        else:
            models[a] = LTXModel(cfg, quantize_transformer_weights_mxfp4(W))
    return models

def inputs(B, F, Hh, Ww, S=1024):
    from mlx_video_amd.ltx_model import TimestepPlan, precompute_freqs_cis
    from mlx_video_amd.schedulers import create_position_grid
    N = F * Hh * Ww
    pe = precompute_freqs_cis(create_position_grid(1, F, Hh, Ww).to(dev), 4096)
    g = torch.Generator(device=dev).manual_seed(B * 1000 + N)
    tok = torch.randn((B, N, 128), generator=g, device=dev).to(BF)
    ctx = torch.randn((B, S, 3840), generator=g, device=dev).to(BF)
    plan = TimestepPlan(torch.tensor([0.625], dtype=BF, device=dev), torch.zeros(B * N, dtype=torch.int32, device=dev))
    return tok, plan, ctx, pe

def capture(model, inp):
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.forward_tokens(*inp)
    torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = model.forward_tokens(*inp)
    return gr, out

def trace_arm(arm, layers):
    """The M = 2560 forward of one arm, eagerly (every launch a kernel-trace record), three times."""
    model = build((arm,), layers)[arm]
    inp = inputs(*SHAPES[0])
    for _ in range(3):
        model.forward_tokens(*inp)
    torch.cuda.synchronize()

def family_split(stats_csv):
    fam = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            name, ns = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
            fam[family(name)] = fam.get(family(name), 0.0) + ns
    # (no shares: the child also builds and quantises its model, and those kernels are in "other")
    return {k: {"ms_per_forward": v / 3e6} for k, v in sorted(fam.items(), key=lambda kv: -kv[1])}

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--limit", type=int, default=540, help="seconds after which the run is abandoned")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--trace", choices=ARMS, default=None, help="(child of --profile) run one arm's M = 2560 forward and exit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    def expired(*_):
        say(f"time limit of {args.limit} s reached: abandoning the run")
        os._exit(3)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)
    if args.trace:
        trace_arm(args.trace, args.layers)
        return
    t0 = time.time()
    models = build(ARMS, args.layers)
    res = {"layers": args.layers, "weight_bytes": {k: m.weight_bytes() for k, m in models.items()}, "shapes": {}}
    say(f"models built in {time.time() - t0:.1f} s")
    for shape in SHAPES:
        B, N = shape[0], shape[1] * shape[2] * shape[3]
        inp = inputs(*shape)
        graphs, outs = {}, {}
        for name, model in models.items():
            graphs[name], outs[name] = capture(model, inp)
        for g_ in graphs.values(): g_.replay()
        torch.cuda.synchronize()
        ref = outs["bf16"].float()
        rel = {k: float((outs[k].float() - ref).norm() / ref.norm()) for k in ("w8a8", "mxfp4")}
        ts = {k: [] for k in ARMS}
        for _ in range(args.rounds):
            for k in ARMS:
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); graphs[k].replay(); e.record(); torch.cuda.synchronize()
                ts[k].append(s.elapsed_time(e))
        t = {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}
        for k in ARMS:
            say(f"forward M={B * N:5d} (B={B} N={N}) {k:6s} median {t[k][0]:8.3f} ms  min {t[k][1]:8.3f}  max {t[k][2]:8.3f}  / bf16 = {t[k][0] / t['bf16'][0]:.4f}"
                f"  / w8a8 = {t[k][0] / t['w8a8'][0]:.4f}")
        say(f"forward M={B * N:5d} rel-L2 to the bf16 output: W8A8 = {rel['w8a8']:.3e}  MXFP4 = {rel['mxfp4']:.3e}")
        res["shapes"][str(B * N)] = {"B": B, "N": N, "ms": t, "ratio_to_bf16": {k: t[k][0] / t["bf16"][0] for k in ARMS},
                                     "ratio_to_w8a8": {k: t[k][0] / t["w8a8"][0] for k in ARMS}, "rel_l2_to_bf16": rel}
        del graphs, outs
        torch.cuda.empty_cache()
    if args.profile:
        del models
        torch.cuda.empty_cache()
        res["kernel_trace_M2560"] = {}
        for arm in ARMS:
            with tempfile.TemporaryDirectory() as d:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--",
                       sys.executable, os.path.abspath(__file__), "--trace", arm, "--layers", str(args.layers), "--limit", "150"]
                rc = subprocess.run(cmd, timeout=170, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
                files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
                if rc != 0 or not files:
                    say(f"kernel trace of {arm}: rocprofv3 ended with {rc}, stats files {files}: stopping the profile runs")
                    break
                res["kernel_trace_M2560"][arm] = family_split(files[0])
                say(f"kernel trace M=2560 {arm}: " + "  ".join(f"{k} {v['ms_per_forward']:.2f} ms" for k, v in res["kernel_trace_M2560"][arm].items()))
    signal.alarm(0)
    say(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

if __name__ == "__main__":
    main()
