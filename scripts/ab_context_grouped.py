"""Interleaved A/B of the text k | V^T projections: the 48 per-block launches + k-norms against the grouped
persistent launch in its tile variants (measurement build: LTXK_GEMM_GROUPED_RB / LTXK_GEMM_GROUPED_FULLREM), then whole L=48
forwards as graph replays with LTXModel.grouped_context_kv off / on, at B=2 and B=1, N=1280, S=1024.  One process, variants
interleaved round by round; median / min / max per variant.   usage: python scripts/ab_context_grouped.py [micro|forward|all]"""
import os, sys, statistics, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from mlx_video_amd import ops, _lib
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

def micro(B, S, rounds=9):
    D, L, H = 4096, 48, 32
    g = torch.Generator(device=dev).manual_seed(1)
    w = [(torch.randn((2 * D, D), generator=g, device=dev) * 0.02).to(BF) for _ in range(L)]
    b = [(torch.randn((2 * D,), generator=g, device=dev) * 0.01).to(BF) for _ in range(L)]
    wn = (1 + 0.1 * torch.randn((L, D), generator=g, device=dev)).to(BF)
    a = torch.randn((B * S, D), generator=g, device=dev).to(BF)
    k = torch.empty((L, B * S, D), dtype=BF, device=dev); vt = torch.empty((L, B, D, S), dtype=BF, device=dev)
    ss = torch.empty((L, B * S, D // 64), dtype=torch.float32, device=dev)
    wt, bt = ops.pointer_table(w), ops.pointer_table(b)
    envs = {"grouped_auto": {}, "grouped_rb4": {"LTXK_GEMM_GROUPED_RB": "4"}, "grouped_rb5": {"LTXK_GEMM_GROUPED_RB": "5"},
            "grouped_rb5_fullrem": {"LTXK_GEMM_GROUPED_RB": "5", "LTXK_GEMM_GROUPED_FULLREM": "1"}}
    def run(kind):
        if kind == "per_block":
            for i in range(L):
                ops.gemm(a, w[i], b[i], out=k[i], out2=vt[i], n_split=D, out_tokens_per_batch=S, sumsq=ss[i])
        elif kind == "per_block_norm":
            for i in range(L):
                ops.qknorm_rope(k[i], 1, D, wn[i], None, None, S, H, 1e-6, sumsq=ss[i])
        elif kind == "grouped_norm":
            ops.qknorm_grouped(k, wn, H, 1e-6, ss)
        else:
            for kk in ("LTXK_GEMM_GROUPED_RB", "LTXK_GEMM_GROUPED_FULLREM"):
                os.environ.pop(kk, None)
            os.environ.update(envs[kind])
            ops.gemm_grouped(a, wt, bt, 2 * D, out=k, out2=vt, n_split=D, out_tokens_per_batch=S, sumsq=ss)
    with _lib.use_library(_lib.AB_LIB_PATH):
        variants = ["per_block"] + list(envs) + ["per_block_norm", "grouped_norm"]
        for v in variants: run(v)
        res = timeit(run, rounds, variants)
    flops = 2.0 * L * B * S * 2 * D * D
    for kname, (med, mn, mx) in res.items():
        say(f"micro B={B} S={S} {kname:22s} median {med:8.3f} ms  min {mn:8.3f}  max {mx:8.3f}" + (f"  {flops / med / 1e9:7.1f} TF/s" if "norm" not in kname else ""))
    del w, b, k, vt, ss
    torch.cuda.empty_cache()

def forward_ab(rounds=9):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig, TimestepPlan, precompute_freqs_cis
    from mlx_video_amd.schedulers import create_position_grid
    t0 = time.time()
    model = LTXModel.random_init(LTXModelConfig(), dev, seed=1234)
    say(f"model built in {time.time() - t0:.1f} s")
    F, Hh, Ww = 5, 16, 16
    N, S = F * Hh * Ww, 1024
    pe = precompute_freqs_cis(create_position_grid(1, F, Hh, Ww).to(dev), 4096)
    for B in (2, 1):
        g = torch.Generator(device=dev).manual_seed(B)
        tok = torch.randn((B, N, 128), generator=g, device=dev).to(BF)
        ctx = torch.randn((B, S, 3840), generator=g, device=dev).to(BF)
        plan = TimestepPlan(torch.tensor([0.625], dtype=BF, device=dev), torch.zeros(B * N, dtype=torch.int32, device=dev))
        graphs, outs = {}, {}
        for name, flag in (("per_block", False), ("grouped", True)):
            model.grouped_context_kv = flag
            s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                model.forward_tokens(tok, plan, ctx, pe)
            torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                outs[name] = model.forward_tokens(tok, plan, ctx, pe)
            graphs[name] = gr
        model.grouped_context_kv = True
        for n_ in graphs: graphs[n_].replay()
        torch.cuda.synchronize()
        say(f"forward B={B}: grouped == per_block bits: {torch.equal(outs['grouped'], outs['per_block'])}")
        res = timeit(lambda k_: graphs[k_].replay(), rounds, list(graphs))
        for kname, (med, mn, mx) in res.items():
            say(f"forward B={B} N={N} S={S} {kname:10s} median {med:8.3f} ms  min {mn:8.3f}  max {mx:8.3f}")
        del graphs, outs
        torch.cuda.empty_cache()

if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("micro", "all"):
        micro(2, 1024); micro(1, 1024)
    if what in ("forward", "all"):
        forward_ab()
