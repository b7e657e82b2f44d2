"""The Gemma-3 text encoder at its real size on random weights (recorded in DESIGN.md 5k; not a gate): 48 layers, hidden 3840,
16 / 8 heads of 256, intermediate 15360, B = 2 (positive + negative prompt), T = 1024, with 120 and with 1024 valid tokens.
The two mask settings are warmed, then timed alternately with device events around whole forwards; the split into GEMMs,
attention and row kernels comes from ops.KernelTimer in a pass of its own (its per-launch events add host time between
launches, so the split is reported next to the whole-forward time, not summed into it).  The GEMM family is also given as a
fraction of the dense bf16 MFMA peak (2.5 PFLOP/s: the DiT's GEMMs hold 0.49), the device memory held after construction is
noted, and the sclk the driver reports right after the timed window where the runtime exposes it.
usage: python scripts/prof_gemma_encoder.py [REPS] [OUT.json]   -> one JSON document"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlx_video_amd import ops                                                              # noqa: E402
from mlx_video_amd.gemma import GemmaConfig, GemmaEncoder, random_gemma_weights            # noqa: E402

BF16_MFMA_PEAK = 2.5e15
ROW_FAMILIES = ("embed_rows", "rmsnorm_weight_rows", "headnorm_rope", "geglu_tanh")


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def forward_ms(enc, ids, mask):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); enc(ids, mask); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    layers = int(os.environ.get("GE_LAYERS", 48))
    B, T = 2, int(os.environ.get("GE_T", 1024))
    dev = torch.device("cuda:0")
    cfg = GemmaConfig(num_hidden_layers=layers, rope_scaling_factor=8.0)
    base = torch.cuda.memory_allocated(dev)
    W = random_gemma_weights(dev, cfg, seed=23, generator_device=dev)
    enc = GemmaEncoder(W, cfg)
    del W
    torch.cuda.empty_cache()
    held = torch.cuda.memory_allocated(dev) - base
    g = torch.Generator().manual_seed(1)
    counts = sorted({min(120, T), T})
    inputs = {}
    for n in counts:
        ids = torch.zeros((B, T), dtype=torch.int64)
        mask = torch.zeros((B, T), dtype=torch.int64)
        ids[:, T - n:] = torch.randint(1, cfg.vocab_size, (B, n), generator=g)
        mask[:, T - n:] = 1
        inputs[n] = (ids, mask)
    for n in counts:                                           # warm every shape and both masks
        for _ in range(2):
            forward_ms(enc, *inputs[n])
    ms = {n: [] for n in counts}
    for _ in range(reps):                                      # alternate the two settings
        for n in counts:
            ms[n].append(forward_ms(enc, *inputs[n]))
    mhz = clock_mhz()
    res = {"shape": {"layers": layers, "hidden": cfg.hidden_size, "heads": [cfg.num_attention_heads, cfg.num_key_value_heads],
                     "intermediate": cfg.intermediate_size, "B": B, "T": T}, "reps": reps, "device": torch.cuda.get_device_name(dev),
           "device_memory_held_GB": round(held / 1e9, 2), "sclk_MHz_after_timed_window": mhz, "runs": []}
    for n in counts:
        v = sorted(ms[n])
        ops.TIMER = ops.KernelTimer()
        enc(*inputs[n])
        split = ops.TIMER.summary()
        ops.TIMER = None
        gemm = split.get("gemm_bf16", {"ms": 0.0, "flops": 0.0, "launches": 0})
        rows = sum(split[f]["ms"] for f in ROW_FAMILIES if f in split)
        res["runs"].append({
            "valid_tokens": n, "forward_ms": {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3), "n": len(v)},
            "kernel_ms": {"gemm": round(gemm["ms"], 3), "causal_attn": round(split.get("causal_attn", {"ms": 0.0})["ms"], 3),
                          "row_kernels": round(rows, 3)},
            "launches": {f: d["launches"] for f, d in split.items()},
            "gemm_TFLOPs": round(gemm["flops"] / (gemm["ms"] * 1e-3) / 1e12, 1) if gemm["ms"] > 0 else None,
            "gemm_fraction_of_bf16_mfma_peak": round(gemm["flops"] / (gemm["ms"] * 1e-3) / BF16_MFMA_PEAK, 3) if gemm["ms"] > 0 else None})
    doc = json.dumps(res, indent=1)
    print(doc, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
