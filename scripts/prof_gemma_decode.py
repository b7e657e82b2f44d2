"""KV-cached Gemma-3 decoding at its real size on random weights (recorded in DESIGN.md 5l; not a gate): 48 layers, hidden 3840,
16 / 8 heads of 256, intermediate 15360, vocabulary 262208, B = 1, a 1024-token prefill and STEPS (64) decode steps.  Reported:
ms per token (device events around whole steps, after two warm steps), launches per token and the GEMM share (ops.KernelTimer
in a step of its own: its per-launch events add host time between launches, so the split stands next to the whole-step time,
not inside it), the attention step alone on a local (window 1024) and a global layer at step 1024 and 1535, and two
yardsticks from the same run: the encoder's forward at the same length (what a token costs without a cache) and the
weight-stream floor, the bytes a token must read (every layer panel and the tied embedding table once) over 6.3 TB/s.
usage: python scripts/prof_gemma_decode.py [STEPS] [OUT.json]   -> one JSON document"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlx_video_amd import ops                                                                          # noqa: E402
from mlx_video_amd.gemma import HEAD_DIM, GemmaConfig, GemmaEncoder, GemmaGenerator, random_gemma_weights   # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def timed(fn, reps):
    """Sorted milliseconds of ``reps`` calls, device events around each."""
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return sorted(out)


def stats(v):
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def attn_step_ms(cfg, dev, step, window, cap=1536, reps=30):
    """ltxk_causal_attn_step alone, B = 1, on a random cache of capacity 1536 (the append rewrites position ``step`` each time)."""
    Hq, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    nq, nkv = Hq * HEAD_DIM, Hkv * HEAD_DIM
    g = torch.Generator(device=dev).manual_seed(5)
    rn = lambda *s: torch.randn(s, generator=g, device=dev).to(torch.bfloat16)          # noqa: E731
    qkv, k, vt, out = rn(1, nq + 2 * nkv), rn(cap, nkv), rn(1, nkv, cap), torch.empty((1, nq), dtype=torch.bfloat16, device=dev)
    rs = torch.zeros(1, dtype=torch.int32, device=dev)
    partials = torch.empty(Hq * (cap // 256) * ops.CAUSAL_ATTN_STEP_PART, dtype=torch.float32, device=dev)
    call = lambda: ops.causal_attn(qkv[:, :nq], k, vt, out, rs, 1, Hq, Hkv, cap, 0.0625, window=window, step=step,          # noqa: E731
                                   k_new=qkv[:, nq:nq + nkv], v_new=qkv[:, nq + nkv:], partials=partials)
    timed(call, 3)
    live = min(step + 1, window) if window else step + 1
    ms = timed(call, reps)
    return dict(stats(ms), step=step, window=window, live_keys=live, kv_bytes=4 * live * nkv,
                GBps_at_median=round(4 * live * nkv / (ms[len(ms) // 2] * 1e-3) / 1e9, 1))


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    layers = int(os.environ.get("GD_LAYERS", 48))
    T = int(os.environ.get("GD_T", 1024))
    dev = torch.device("cuda:0")
    cfg = GemmaConfig(num_hidden_layers=layers, rope_scaling_factor=8.0)
    enc = GemmaEncoder(random_gemma_weights(dev, cfg, seed=23, generator_device=dev), cfg)
    torch.cuda.empty_cache()
    gen = GemmaGenerator(enc)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, cfg.vocab_size, (1, T), generator=g)
    mask = torch.ones_like(ids)
    toks = torch.randint(1, cfg.vocab_size, (steps + 3,), generator=g)
    panel_bytes = sum(ly[k].numel() * 2 for ly in enc.layers for k in ("qkv", "o", "gu", "down"))
    stream_bytes = panel_bytes + enc.embed.numel() * 2
    enc(ids, mask)                                              # warm
    fwd = timed(lambda: enc(ids, mask), 3)
    cache, _ = gen.prefill(ids, mask, (T + steps + 3 + 63) // 64 * 64)
    pre = timed(lambda: gen.prefill(ids, mask, cache.capacity), 3)
    for i in range(2):                                          # warm steps
        gen.step(cache, toks[i:i + 1])
    per = []
    for i in range(steps):
        per += timed(lambda: gen.step(cache, toks[2 + i:3 + i]), 1)
    per.sort()
    ops.TIMER = ops.KernelTimer()
    gen.step(cache, toks[-1:])
    split = ops.TIMER.summary()
    ops.TIMER = None
    # launches: one per library call, plus the combine of the attention step and of every GEMM the plan function splits
    D, F = cfg.hidden_size, cfg.intermediate_size
    nq, nkv = cfg.num_attention_heads * HEAD_DIM, cfg.num_key_value_heads * HEAD_DIM
    gemms = [(nq + 2 * nkv, D), (D, nq), (2 * F, D), (D, F)]
    split_gemms = layers * sum(ops.gemm_plan(1, N, K, lda=2 * F if K == F else K).split_k for N, K in gemms) + \
        int(ops.gemm_plan(1, cfg.vocab_size, D).split_k)
    calls = sum(d["launches"] for d in split.values())
    launches = calls + split.get("causal_attn_step", {"launches": 0})["launches"] + split_gemms
    total = sum(d["ms"] for d in split.values())
    med = per[len(per) // 2]
    floor_ms = stream_bytes / HBM_BYTES_PER_S * 1e3
    res = {"shape": {"layers": layers, "hidden": cfg.hidden_size, "heads": [cfg.num_attention_heads, cfg.num_key_value_heads],
                     "intermediate": cfg.intermediate_size, "vocab": cfg.vocab_size, "B": 1, "prefill_tokens": T, "steps": steps},
           "device": torch.cuda.get_device_name(dev),
           "ms_per_token": stats(per), "tokens_per_s": round(1e3 / med, 1), "library_calls_per_token": calls, "launches_per_token": launches,
           "split_k_gemms_per_token": split_gemms,
           "kernel_ms_per_token": {f: round(d["ms"], 4) for f, d in split.items()},
           "gemm_share_of_kernel_time": round(split.get("gemm_bf16", {"ms": 0.0})["ms"] / total, 3) if total > 0 else None,
           "attention_step_ms": [attn_step_ms(cfg, dev, s, w) for s in (1024, 1535) for w in (cfg.sliding_window, 0)],
           "yardsticks": {"encoder_forward_ms_same_length": stats(fwd), "prefill_ms": stats(pre),
                          "reforward_over_step": round(fwd[len(fwd) // 2] / med, 1),
                          "bytes_streamed_per_token": stream_bytes, "weight_stream_floor_ms": round(floor_ms, 3),
                          "step_over_floor": round(med / floor_ms, 2)}}
    doc = json.dumps(res, indent=1)
    print(doc, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
