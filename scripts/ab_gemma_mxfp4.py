"""Gemma-3 decoding on fp8 panels against decoding on OCP MXFP4 decode panels, at the model's real size on random weights
(recorded in DESIGN.md 5r; not a gate): 48 layers, hidden 3840, vocabulary 262208, B = 1, a 1024-token prefill and STEPS (64)
tokens at temperature 0.7 and repetition penalty 1.3 over 20 tokens, no EOS.  One fp8 ("channel") encoder serves every arm.
  a  fp8 panels, the step replayed as a graph (GemmaGenerator(enc): the five GEMMs on ltxk_gemv_w8)
  b  MXFP4 decode panels, the step replayed as a graph (GemmaGenerator(enc, decode_panels="mxfp4"), ALL five GEMMs on ltxk_gemv_w4)
  c  the same with only the shapes routed to ltxk_gemv_w4 that the per-shape table below lets win (run only when that is not all five)
The arms run interleaved in one process, ROUNDS (9) rounds each: wall time of STEPS replays divided by STEPS, median (min - max).
Per shape (q|k|v, o, gate|up, down: one launch on each of the 48 layers' panels, so that every panel comes from memory as it does
inside a token; the logits: the one table, the two arms' launches alternating), ops.KernelTimer times of ltxk_gemv_w8 against
ltxk_gemv_w4 at M = 1 (ROUNDS rounds) and at M = 2, 4, 8 (3 rounds), with the achieved TB/s of the panel bytes.  Routing rule (5p's):
a shape goes to ltxk_gemv_w4 only where it beats ltxk_gemv_w8 by more than the larger of the two arms' min - max spreads.
Also recorded: decode_weight_bytes() of both generators and the weight-stream floor at 6.3 TB/s, the library calls of a step and
the graph's kernel-node count (null where torch offers no dot dump of a captured graph, as on the ROCm build measured), and - on the tiny test model (hidden 512, 6 layers, vocabulary 512), recorded and not gated - what 4-bit storage
costs: rel-L2 of 24 teacher-forced steps' logits on MXFP4 panels against the bf16 generator's, and the share of 64 greedy tokens
on which the two agree.
usage: python scripts/ab_gemma_mxfp4.py [STEPS] [OUT.json]   -> one JSON document"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_gemma_graph import Arms, stats, wall_ms                                                              # noqa: E402
from mlx_video_amd import ops                                                                                  # noqa: E402
from mlx_video_amd.gemma import GemmaConfig, GemmaEncoder, GemmaGenerator, random_gemma_weights                # noqa: E402

BF16 = torch.bfloat16
HBM_TBS = 6.3
SHAPES = ("qkv", "o", "gu", "down", "logits")
ALL = dict.fromkeys(SHAPES, True)


class AllW4(GemmaGenerator):
    """Every shape copied to MXFP4 and routed to ltxk_gemv_w4, whatever the shipped table says: the arm to measure."""
    GEMV4_SHAPES = dict(ALL)


def shape_times(enc, gen4, M, rounds):
    """{shape: {"N", "K", "w8": stats ms, "w4": stats ms, TB/s of the medians}} at M rows."""
    dev = enc.device
    g = torch.Generator(device=dev).manual_seed(M)
    out = {}
    for name in SHAPES:
        if name == "logits":
            p8 = [(enc.embed, enc.embed_row_scale)]
            p4 = [gen4.table4]
        else:
            p8 = [(ly[name], ly[name + "_s"]) for ly in enc.layers]
            p4 = [p[name] for p in gen4.panels4]
        N, K = p8[0][0].shape
        a = torch.randn((M, K), generator=g, device=dev).to(BF16)
        y = torch.empty((M, N), dtype=BF16, device=dev)
        ms = {"w8": [], "w4": []}
        for _ in range(rounds):
            for arm in ("w8", "w4"):
                ops.TIMER = ops.KernelTimer()
                for i in range(len(p8)):
                    if arm == "w8":
                        ops.gemm(a, p8[i][0], None, out=y, w_scale=p8[i][1], gemv=True)
                    else:
                        ops.gemv_w4(a, p4[i][0], p4[i][1], None, out=y)
                s = ops.TIMER.summary()["gemv_" + arm]
                ops.TIMER = None
                ms[arm].append(s["ms"] / s["launches"])
        st8, st4 = stats(ms["w8"]), stats(ms["w4"])
        b8, b4 = N * K + 4 * N, N * K // 2 + N * K // 32
        gain = st8["median"] - st4["median"]
        spread = max(st8["max"] - st8["min"], st4["max"] - st4["min"])
        out[name] = {"N": N, "K": K, "w8_ms": st8, "w4_ms": st4, "w8_bytes": b8, "w4_bytes": b4,
                     "w8_TBs": round(b8 / st8["median"] * 1e-9, 3), "w4_TBs": round(b4 / st4["median"] * 1e-9, 3),
                     "w8_minus_w4_ms": round(gain, 4), "larger_spread_ms": round(spread, 4), "w4_wins": bool(gain > spread)}
    return out


def tiny_cost(dev):
    """What 4-bit storage costs on the tiny test model: MXFP4 decode panels against the bf16 generator they were built from."""
    cfg = GemmaConfig(hidden_size=512, num_hidden_layers=6, num_attention_heads=4, num_key_value_heads=2, head_dim=256,
                      intermediate_size=1024, vocab_size=512, sliding_window=1024, sliding_window_pattern=6, rope_scaling_factor=8.0)
    enc = GemmaEncoder(random_gemma_weights(dev, cfg, seed=3), cfg)
    g16, g4 = GemmaGenerator(enc), AllW4(enc, decode_panels="mxfp4")
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, cfg.vocab_size, (2, 96), generator=g)
    mask = torch.ones_like(ids)
    lg = {}
    for name, gen in (("bf16", g16), ("mxfp4", g4)):
        cache, _ = gen.prefill(ids[:, :72], mask[:, :72], 128)
        lg[name] = torch.stack([gen.step(cache, ids[:, t]) for t in range(72, 96)]).double().cpu()
    rel = float((lg["mxfp4"] - lg["bf16"]).norm() / lg["bf16"].norm())
    kw = dict(max_tokens=64, temperature=0.0, repetition_penalty=1.3, repetition_context=20, eos_ids=())
    t16, t4 = g16.generate(ids[:, :72], mask[:, :72], **kw), g4.generate(ids[:, :72], mask[:, :72], **kw)
    same = [sum(x == y for x, y in zip(r16, r4)) for r16, r4 in zip(t16, t4)]
    first = [next((i for i, (x, y) in enumerate(zip(r16, r4)) if x != y), len(r16)) for r16, r4 in zip(t16, t4)]
    return {"logits_rel_l2_vs_bf16_generator_24_teacher_forced_steps": round(rel, 5),
            "greedy_tokens_agreeing_of_64_per_row": same, "first_differing_token_per_row": first,
            "decode_weight_bytes": {"bf16": g16.decode_weight_bytes(), "mxfp4": g4.decode_weight_bytes()}}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    layers = int(os.environ.get("GD_LAYERS", 48))
    T = int(os.environ.get("GD_T", 1024))
    rounds = int(os.environ.get("GD_ROUNDS", 9))
    dev = torch.device("cuda:0")
    cfg = GemmaConfig(num_hidden_layers=layers, rope_scaling_factor=8.0)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, cfg.vocab_size, (1, T), generator=g)
    mask = torch.ones_like(ids)
    res = {"shape": {"layers": layers, "hidden": cfg.hidden_size, "vocab": cfg.vocab_size, "B": 1, "prefill_tokens": T, "steps": steps,
                     "rounds": rounds, "temperature": 0.7, "repetition_penalty": 1.3, "repetition_context": 20},
           "device": torch.cuda.get_device_name(dev)}
    enc = GemmaEncoder(random_gemma_weights(dev, cfg, seed=23, generator_device=dev), cfg, fp8="channel")
    torch.cuda.empty_cache()
    gen8 = GemmaGenerator(enc)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gen4 = AllW4(enc, decode_panels="mxfp4")
    torch.cuda.synchronize()
    res["build_mxfp4_panels_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    torch.cuda.empty_cache()
    print("panels built", flush=True)

    # per shape, ltxk_gemv_w8 against ltxk_gemv_w4
    per_m = {}
    for M, r in ((1, rounds), (2, 3), (4, 3), (8, 3)):
        shape_times(enc, gen4, M, 1)                      # untimed: code objects
        per_m[f"M{M}"] = shape_times(enc, gen4, M, r)
        print(f"shapes at M = {M} done", flush=True)
    res["gemm_shapes"] = per_m
    routing = {name: per_m["M1"][name]["w4_wins"] for name in SHAPES}
    res["routing_GEMV4_SHAPES"] = routing
    res["gemms_of_a_token_ms_M1"] = {arm: round(sum(per_m["M1"][n][arm + "_ms"]["median"] * (1 if n == "logits" else layers) for n in SHAPES), 4)
                                     for arm in ("w8", "w4")}

    # the token: replayed graphs, interleaved
    gens = {"a_fp8": gen8, "b_mxfp4_all": gen4}
    if not all(routing.values()) and any(routing.values()):
        gen_r = GemmaGenerator.__new__(GemmaGenerator)          # the same encoder and MXFP4 panels, another routing table
        gen_r.__dict__.update(gen4.__dict__)
        gen_r.routing4 = dict(routing)
        gens["c_mxfp4_routed"] = gen_r
    arms = {}
    for name, gen in gens.items():
        arms[name] = a = Arms(gen, ids, mask, steps, seed=1)
        a.reset(); a.eager()
        a.capture()
    print("graphs captured", flush=True)
    per = {name: [] for name in arms}
    for _ in range(rounds):
        for name, a in arms.items():
            a.reset()
            per[name].append(wall_ms(a.replay) / steps)
    res["ms_per_token_graph"] = {name: stats(v) for name, v in per.items()}
    st = res["ms_per_token_graph"]
    for name in arms:
        if name != "a_fp8":
            gain = st["a_fp8"]["median"] - st[name]["median"]
            spread = max(st["a_fp8"]["max"] - st["a_fp8"]["min"], st[name]["max"] - st[name]["min"])
            res[name + "_vs_a"] = {"a_minus_arm_ms": round(gain, 4), "larger_spread_ms": round(spread, 4),
                                   "beats_a_by_more_than_the_spread": bool(gain > spread)}
    res["step"] = {}
    for name, a in arms.items():
        a.reset()
        ops.TIMER = ops.KernelTimer()
        a._step()
        split = ops.TIMER.summary()
        ops.TIMER = None
        nbytes = gens[name].decode_weight_bytes()
        res["step"][name] = {"library_calls": sum(d["launches"] for d in split.values()), "graph_nodes": a.nodes,
                             "kernel_ms": {f: round(d["ms"], 4) for f, d in split.items()},
                             "kernel_ms_sum": round(sum(d["ms"] for d in split.values()), 4),
                             "decode_weight_bytes": nbytes, "weight_stream_floor_ms_at_6.3TBs": round(nbytes / (HBM_TBS * 1e9), 4)}
    res["encoder_weight_bytes"] = enc.weight_bytes()
    del arms, gens, gen4, gen8, enc
    torch.cuda.empty_cache()
    res["tiny_model_cost_of_4_bit_storage"] = tiny_cost(dev)
    doc = json.dumps(res, indent=1)
    print(doc, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
