"""FP8 Gemma-3 panels against bf16 ones at the model's real size on random weights (recorded in DESIGN.md 5p; not a gate): 48
layers, hidden 3840, 16 / 8 heads of 256, intermediate 15360, vocabulary 262208, B = 1, a 1024-token prefill and STEPS (64)
decode steps.  Three arms, interleaved in one process, ROUNDS (9) rounds each, median with min and max:
  a  bf16 panels, the decode GEMMs on split-K ltxk_gemm_bf16 (the path before fp8 panels, re-timed in this run)
  b  fp8 panels, the decode GEMMs on split-K ltxk_gemm_w8
  c  fp8 panels, the decode GEMMs on ltxk_gemv_w8 (``GemmaGenerator``'s routing)
Per arm: ms per token (device events around a round of STEPS steps), launches per token, the five GEMM shapes of a step each
on their own (ops.KernelTimer around the call, the median over the 48 layers' panels in turn so that no panel is read from a
cache it was left in; the logits panel is larger than every cache), their achieved GB/s against 6.3 TB/s, the encoder's forward at
T = 1024, B = 2, and weight_bytes().  Also recorded: the tiny test model's final context (the connector's output) under fp8
Gemma against bf16 Gemma, rel-L2.
usage: python scripts/ab_gemma_fp8.py [STEPS] [OUT.json]   -> one JSON document"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlx_video_amd import ops                                                                          # noqa: E402
from mlx_video_amd.gemma import HEAD_DIM, GemmaConfig, GemmaEncoder, GemmaGenerator, random_gemma_weights   # noqa: E402

HBM_BYTES_PER_S = 6.3e12
BF = torch.bfloat16


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def shape_ms(enc, which, gemv, x, out):
    """Kernel milliseconds of ONE GEMM of shape ``which`` at M = 1: the median over the layers' panels (the logits: the one table,
    five times).  The median, not the mean: an event pair around a launch also spans the host's submission of it, and one late
    submission among the 48 would otherwise move the sample."""
    ops.TIMER = ops.KernelTimer()
    if which == "logits":
        panels = [(enc.embed, enc.embed_row_scale)] * 5
    else:
        panels = [(ly[which], ly[which + "_s"]) for ly in enc.layers]
    for w, sc in panels:
        if gemv:
            ops.gemm(x, w, None, out=out, w_scale=sc, gemv=True)
        else:
            ops.gemm(x, w, None, out=out, w_scale=sc, split_k=True)
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for _, _, _, s, e in ops.TIMER.records)
    ops.TIMER = None
    return ms[len(ms) // 2]


def tiny_context_rel_l2(dev):
    """rel-L2 of the connector's output on the tiny test model (hidden 512, 6 layers) under fp8 Gemma against bf16 Gemma."""
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    cfg = GemmaConfig(hidden_size=512, num_hidden_layers=6, num_attention_heads=4, num_key_value_heads=2, head_dim=256,
                      intermediate_size=1024, vocab_size=512, sliding_window=1024, sliding_window_pattern=6, rope_scaling_factor=8.0)
    W = random_gemma_weights("cpu", cfg, seed=3)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, 512, (2, 96), generator=g)
    mask = torch.ones(2, 96, dtype=torch.int64)
    ids[1, :59], mask[1, :59] = 0, 0
    conn = TextConnector(random_connector_weights(dev, D=512, L=cfg.num_hidden_layers + 1, layers=1, R=16))
    out = {}
    ref = conn(GemmaEncoder({k: v.to(dev) for k, v in W.items()}, cfg)(ids, mask), mask.to(dev)).double()
    for scaling in ("channel", "none"):
        got = conn(GemmaEncoder({k: v.to(dev) for k, v in W.items()}, cfg, fp8=scaling)(ids, mask), mask.to(dev)).double()
        out[scaling] = float((got - ref).norm() / ref.norm())
    return out


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    layers = int(os.environ.get("GD_LAYERS", 48))
    T = int(os.environ.get("GD_T", 1024))
    rounds = int(os.environ.get("GD_ROUNDS", 9))
    dev = torch.device("cuda:0")
    cfg = GemmaConfig(num_hidden_layers=layers, rope_scaling_factor=8.0)
    enc16 = GemmaEncoder(random_gemma_weights(dev, cfg, seed=23, generator_device=dev), cfg)
    torch.cuda.empty_cache()
    enc8 = GemmaEncoder(random_gemma_weights(dev, cfg, seed=23, generator_device=dev), cfg, fp8="channel")
    torch.cuda.empty_cache()
    arms = {"a_bf16_splitk": (enc16, GemmaGenerator(enc16), False), "b_fp8_splitk": (enc8, GemmaGenerator(enc8, gemv=False), False),
            "c_fp8_gemv": (enc8, GemmaGenerator(enc8), True)}
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, cfg.vocab_size, (1, T), generator=g)
    mask = torch.ones_like(ids)
    toks = torch.randint(1, cfg.vocab_size, (steps + 3,), generator=g)
    D, F = cfg.hidden_size, cfg.intermediate_size
    nq, nkv = cfg.num_attention_heads * HEAD_DIM, cfg.num_key_value_heads * HEAD_DIM
    shapes = {"qkv": (nq + 2 * nkv, D), "o": (D, nq), "gu": (2 * F, D), "down": (D, F), "logits": (cfg.vocab_size, D)}
    caches = {}
    for name, (enc, gen, _) in arms.items():
        caches[name], _ = gen.prefill(ids, mask, (T + steps + 3 + 63) // 64 * 64)
        for i in range(2):
            gen.step(caches[name], toks[i:i + 1])
    per = {name: [] for name in arms}
    per_shape = {name: {s: [] for s in shapes} for name in arms}
    g2 = torch.Generator(device=dev).manual_seed(2)
    xs = {K: torch.randn((1, K), generator=g2, device=dev).to(BF) for K in {k for _, k in shapes.values()}}
    outs = {N: torch.empty((1, N), dtype=BF, device=dev) for N in {n for n, _ in shapes.values()}}

    def run_steps(gen, cache):
        cache.length = T + 2
        for i in range(steps):
            gen.step(cache, toks[2 + i:3 + i])

    for name, (enc, gen, gemv) in arms.items():              # every timed shape once, untimed: first launches load code objects
        for s, (N, K) in shapes.items():
            shape_ms(enc, s, gemv, xs[K], outs[N])
    for _ in range(rounds):
        for name, (enc, gen, gemv) in arms.items():
            per[name].append(event_ms(lambda: run_steps(gen, caches[name])) / steps)
        for name, (enc, gen, gemv) in arms.items():
            for s, (N, K) in shapes.items():
                per_shape[name][s].append(shape_ms(enc, s, gemv, xs[K], outs[N]))
    ids2, mask2 = torch.cat([ids, ids.flip(1)]), torch.cat([mask, mask])
    fwd = {"bf16": [], "fp8": []}
    for e in (enc16, enc8):
        e(ids2, mask2)
    for _ in range(rounds):
        fwd["bf16"].append(event_ms(lambda: enc16(ids2, mask2)))
        fwd["fp8"].append(event_ms(lambda: enc8(ids2, mask2)))
    res = {"shape": {"layers": layers, "hidden": D, "heads": [cfg.num_attention_heads, cfg.num_key_value_heads], "intermediate": F,
                     "vocab": cfg.vocab_size, "B": 1, "prefill_tokens": T, "steps": steps, "rounds": rounds},
           "device": torch.cuda.get_device_name(dev), "arms": {}}
    for name, (enc, gen, gemv) in arms.items():
        w8 = enc.weight_dtype != BF
        ops.TIMER = ops.KernelTimer()
        caches[name].length = T + 2
        gen.step(caches[name], toks[-1:])
        split = ops.TIMER.summary()
        ops.TIMER = None
        calls = sum(d["launches"] for d in split.values())
        split_gemms = 0 if gemv else layers * sum(ops.gemm_plan(1, N, K, lda=2 * F if K == F else K, w8=w8).split_k
                                                  for s, (N, K) in shapes.items() if s != "logits") + \
            int(ops.gemm_plan(1, cfg.vocab_size, D, w8=w8).split_k)
        stream = sum(ly[k].numel() * ly[k].element_size() for ly in enc.layers for k in ("qkv", "o", "gu", "down")) + \
            enc.embed.numel() * enc.embed.element_size()
        floor_ms = stream / HBM_BYTES_PER_S * 1e3
        rows = {}
        for s, (N, K) in shapes.items():
            st = stats(per_shape[name][s])
            nbytes = N * K * (1 if w8 else 2)
            rows[s] = dict(st, N=N, K=K, panel_bytes=nbytes, GBps_at_median=round(nbytes / (st["median"] * 1e-3) / 1e9, 1),
                           share_of_6300_GBps=round(nbytes / (st["median"] * 1e-3) / HBM_BYTES_PER_S, 3))
        res["arms"][name] = {"ms_per_token": stats(per[name]), "library_calls_per_token": calls,
                             "launches_per_token": calls + split.get("causal_attn_step", {"launches": 0})["launches"] + split_gemms,
                             "kernel_ms_per_token": {f: round(d["ms"], 4) for f, d in split.items()}, "gemm_shapes_ms": rows,
                             "weight_bytes": enc.weight_bytes(), "bytes_streamed_per_token": stream,
                             "weight_stream_floor_ms": round(floor_ms, 3),
                             "step_over_floor": round(stats(per[name])["median"] / floor_ms, 2)}
    res["encoder_forward_ms_T1024_B2"] = {k: stats(v) for k, v in fwd.items()}
    # the routing rule: a shape keeps gemv=True only where arm c beats arm b by more than the two arms' min-max spread
    b, c = res["arms"]["b_fp8_splitk"]["gemm_shapes_ms"], res["arms"]["c_fp8_gemv"]["gemm_shapes_ms"]
    res["routing"] = {s: {"b_minus_c_ms": round(b[s]["median"] - c[s]["median"], 4),
                          "spread_ms": round(max(b[s]["max"] - b[s]["min"], c[s]["max"] - c[s]["min"]), 4),
                          "gemv": bool(b[s]["median"] - c[s]["median"] > max(b[s]["max"] - b[s]["min"], c[s]["max"] - c[s]["min"]))}
                      for s in shapes}
    try:
        res["tiny_model_context_rel_l2_fp8_vs_bf16"] = tiny_context_rel_l2(dev)
    except Exception as e:          # recorded, not a gate
        res["tiny_model_context_rel_l2_fp8_vs_bf16"] = f"{type(e).__name__}: {e}"
    doc = json.dumps(res, indent=1)
    print(doc, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
