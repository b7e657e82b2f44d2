"""The text stage at its real size, against the same computation in plain torch ops (recorded in DESIGN.md 5i; not a gate).
L = 49 hidden states, T = 1024, D = 3840, B = 2 (positive + negative prompt), random weights; 120 and 1024 valid tokens.
Both paths are warmed, then timed alternately with device events around whole calls; the per-kernel split of the product
path comes from ops.KernelTimer in a pass of its own.  The stats / normalise kernels are also given as a share of the HBM rate
(bytes the algorithm moves over kernel time, against the 8 TB/s peak).
usage: python scripts/ab_text_stage.py [REPS]   -> one JSON line per valid-token count"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlx_video_amd import ops                                                              # noqa: E402
from mlx_video_amd.text_connector import TextConnector, random_connector_weights, rope_table_1d     # noqa: E402
from mlx_video_amd.weights import aggregate_k_to_layer_major                              # noqa: E402

BF = torch.bfloat16
HBM_PEAK = 8.0e12


def torch_stage(hs, mask, W, H, cos, sin):
    """norm_and_concat_hidden_states + aggregate_embed + Embeddings1DConnector as the reference computes them - every padded
    row included - in torch ops on the device.  hs (L,B,T,D) bf16, mask (B,T) int64."""
    L, B, T, D = hs.shape
    x = hs.permute(1, 2, 3, 0)                                           # (B,T,D,L)
    counts = mask.sum(1)
    valid = (torch.arange(T, device=hs.device)[None] >= (T - counts)[:, None])[:, :, None, None]
    xf = x.float()
    mean = torch.where(valid, xf, 0.0).sum((1, 2), keepdim=True) / ((counts * D).float().reshape(B, 1, 1, 1) + 1e-6)
    mn = torch.where(valid, xf, float("inf")).amin((1, 2), keepdim=True)
    mx = torch.where(valid, xf, float("-inf")).amax((1, 2), keepdim=True)
    normed = (8 * (xf - mean) / (mx - mn + 1e-6)).to(BF).reshape(B, T, D * L)
    normed = torch.where(valid[:, :, :, 0], normed, 0.0)
    feat = normed @ W["aggregate_embed.weight"].T
    R = W["learnable_registers"].shape[0]
    tiled = W["learnable_registers"].repeat(T // R, 1)
    x = torch.stack([torch.cat([feat[b, T - int(c):], tiled[int(c):]], 0) for b, c in enumerate(counts.tolist())], 0)

    def rms(t, w=None):
        y = t.float() * torch.rsqrt(t.float().pow(2).mean(-1, keepdim=True) + 1e-6)
        return (y if w is None else y * w.float()).to(BF)

    def rope(t):
        t = t.reshape(B, T, H, 128).permute(0, 2, 1, 3).float()
        a, b = t[..., :64], t[..., 64:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], -1).to(BF)

    n = 1 + max(int(k.split(".")[1]) for k in W if k.startswith("transformer_1d_blocks."))
    for i in range(n):
        g = lambda name: W[f"transformer_1d_blocks.{i}.{name}"]
        nx = rms(x)
        q = rope(rms(F.linear(nx, g("attn1.to_q.weight"), g("attn1.to_q.bias")), g("attn1.q_norm.weight")))
        k = rope(rms(F.linear(nx, g("attn1.to_k.weight"), g("attn1.to_k.bias")), g("attn1.k_norm.weight")))
        v = F.linear(nx, g("attn1.to_v.weight"), g("attn1.to_v.bias")).reshape(B, T, H, 128).permute(0, 2, 1, 3)
        att = F.scaled_dot_product_attention(q, k, v, scale=1.0 / math.sqrt(128)).permute(0, 2, 1, 3).reshape(B, T, D)
        x = x + F.linear(att, g("attn1.to_out.weight"), g("attn1.to_out.bias"))
        h = F.gelu(F.linear(rms(x), g("ff.proj_in.weight"), g("ff.proj_in.bias")))
        x = x + F.linear(h, g("ff.proj_out.weight"), g("ff.proj_out.bias"))
    return rms(x)


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    t = sorted(s.elapsed_time(e) for s, e in ev)
    return t[len(t) // 2], t[0]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L, T, D, B = (int(os.environ.get(k, v)) for k, v in (("TS_L", 49), ("TS_T", 1024), ("TS_D", 3840), ("TS_B", 2)))
    dev = torch.device("cuda:0")
    W = random_connector_weights(dev, D=D, L=L, layers=2, R=128, seed=17, generator_device=dev)
    tc = TextConnector({**{k: v for k, v in W.items() if k != "aggregate_embed.weight"},
                        "aggregate_embed.weight_layer_major": aggregate_k_to_layer_major(W["aggregate_embed.weight"], D)})
    cos, sin = (t.to(dev)[None] for t in rope_table_1d(T, tc.H))
    g = torch.Generator(device=dev).manual_seed(1)
    hs = (torch.randn((L, B, T, D), generator=g, device=dev) * 3 + 0.5).to(BF)
    for count in (120, T):
        mask = torch.zeros((B, T), dtype=torch.int64, device=dev)
        mask[:, T - count:] = 1
        ours = lambda: tc(hs, mask)
        theirs = lambda: torch_stage(hs, mask, W, tc.H, cos, sin)
        a, b = ours(), theirs()
        rel = float((a.float() - b.float()).norm() / b.float().norm())
        for _ in range(2):
            ours(); theirs()
        torch.cuda.synchronize()
        res = {"valid_tokens": count, "shape": [L, B, T, D], "rel_l2_product_vs_torch": rel, "product_ms": [], "torch_ms": []}
        for _ in range(reps):                                   # alternate the two paths
            res["product_ms"].append(timed(ours, 1)[0])
            res["torch_ms"].append(timed(theirs, 1)[0])
        for k in ("product_ms", "torch_ms"):
            v = sorted(res[k])
            res[k] = {"median": v[len(v) // 2], "min": v[0], "n": len(v)}
        ops.TIMER = ops.KernelTimer()
        ours()
        split = ops.TIMER.summary()
        ops.TIMER = None
        res["kernels"] = {fam: {"launches": d["launches"], "ms": round(d["ms"], 4),
                                "TB_per_s": round(d["bytes"] / (d["ms"] * 1e-3) / 1e12, 3) if d["bytes"] and d["ms"] > 0 else None}
                          for fam, d in split.items()}
        for fam in ("text_layer_stats", "text_layer_norm"):
            if fam in split and split[fam]["ms"] > 0:
                res[fam + "_share_of_hbm_peak"] = round(split[fam]["bytes"] / (split[fam]["ms"] * 1e-3) / HBM_PEAK, 3)
        res["aggregate_gemm_rows"] = {"product": B * count, "reference": B * T}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
