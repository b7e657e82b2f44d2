"""The Gemma-3 decode loop on the host against the loop on the device, at the model's real size on random weights (recorded in
DESIGN.md 5q; not a gate): 48 layers, hidden 3840, vocabulary 262208, B = 1, a 1024-token prefill and STEPS (64) tokens at
temperature 0.7 and repetition penalty 1.3 over 20 tokens, no EOS.  Three arms, interleaved in one process, ROUNDS (9) rounds
each, median with min and max, for bf16 and for fp8 panels:
  host    sample_tokens on the host's copy of the logits + GemmaGenerator.step: the loop of generate(device_loop=False)
  eager   GemmaGenerator.device_step launched from Python every token
  graph   device_step recorded once and replayed, the host reading ctl every 16 tokens: the loop of generate(device_loop=True)
A round is wall time from the first token's sampling to the synchronisation behind the last step, divided by STEPS: the loops
are host-bound, so host time is what is being measured.  The prefill is run once per panel kind and is not timed; every arm
starts from its cache and logits.  Also recorded: the capture's wall time and the graph's kernel-node count (from its debug
dump, where torch offers one), the sampler alone at V = 262208 (ops.KernelTimer, median of 20), the sum of the kernel times
inside one step (KernelTimer around an eager device_step) as the graph's floor, and whole generate() calls of both loops.
usage: python scripts/ab_gemma_graph.py [STEPS] [OUT.json]   -> one JSON document"""
import json
import os
import re
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlx_video_amd import ops                                                                                  # noqa: E402
from mlx_video_amd.gemma import GemmaConfig, GemmaDecodeState, GemmaEncoder, GemmaGenerator, random_gemma_weights, sample_tokens   # noqa: E402

TEMPERATURE, PENALTY, CONTEXT, SYNC_EVERY = 0.7, 1.3, 20, 16


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def graph_nodes(g):
    """Kernel nodes of a captured graph, counted in its dot dump; None where the dump is not available."""
    try:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "step.dot")
            g.debug_dump(path)
            return len(re.findall(r"^\s*\"?\w+\"?\s*\[", open(path).read(), re.M))
    except Exception:
        return None


class Arms:
    """The three loops of one panel kind on one cache: each starts from the prefill's logits and position."""

    def __init__(self, gen, ids, mask, steps, seed):
        self.gen, self.steps, self.T = gen, steps, ids.shape[1]
        self.state = GemmaDecodeState(gen.cfg, gen.enc.vocab, ids, mask, steps, (), seed, gen.enc.device)
        self.cache, states = gen.prefill(ids, mask, (self.T + steps + 63) // 64 * 64, logits=False)
        gen._gemm("logits", states[-1][:, self.T - 1], gen.enc.embed, gen.enc.embed_row_scale, self.state.logits)
        self.logits0 = self.state.logits.clone()
        self.saved = {k: getattr(self.state, k).clone() for k in ("ctl", "done", "next_ids", "history", "hist_len", "tokens_out")}
        self.prompt = [int(t) for t in ids[0]]
        self.graph, self.capture_ms, self.nodes = None, None, None

    def reset(self):
        for k, v in self.saved.items():
            getattr(self.state, k).copy_(v)
        self.state.logits.copy_(self.logits0)
        self.cache.length = self.T

    def _step(self):
        self.gen.device_step(self.cache, self.state, TEMPERATURE, PENALTY, CONTEXT)

    def host(self):
        logits, history = self.logits0.to(torch.float32), [list(self.prompt)]
        g = torch.Generator(device="cpu").manual_seed(1)
        for n in range(self.steps):
            tok = sample_tokens(logits, [history[0][-CONTEXT:]], TEMPERATURE, PENALTY, g)
            history[0].append(int(tok[0]))
            logits = self.gen.step(self.cache, tok)

    def eager(self):
        for _ in range(self.steps):
            self._step()

    def capture(self):
        self.reset()
        self._step()
        g = torch.cuda.CUDAGraph()
        g.enable_debug_mode()
        t0 = time.perf_counter()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._step()
        self.capture_ms = (time.perf_counter() - t0) * 1e3
        self.graph, self.nodes = g, graph_nodes(g)

    def replay(self):
        for i in range(self.steps):
            if i and i % SYNC_EVERY == 0:
                self.state.read()
            self.graph.replay()


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
                     "rounds": rounds, "temperature": TEMPERATURE, "repetition_penalty": PENALTY, "repetition_context": CONTEXT,
                     "sync_every": SYNC_EVERY},
           "device": torch.cuda.get_device_name(dev), "panels": {}}
    arms = {}
    for kind, fp8 in (("bf16", None), ("fp8", "channel")):
        enc = GemmaEncoder(random_gemma_weights(dev, cfg, seed=23, generator_device=dev), cfg, fp8=fp8)
        torch.cuda.empty_cache()
        arms[kind] = a = Arms(GemmaGenerator(enc), ids, mask, steps, seed=1)
        a.host()                                  # every loop once, untimed: code objects, the split-K scratch, the tables
        a.reset(); a.eager()
        a.capture()
    per = {kind: {"host": [], "eager": [], "graph": []} for kind in arms}
    for _ in range(rounds):
        for kind, a in arms.items():
            for name, fn in (("host", a.host), ("eager", a.eager), ("graph", a.replay)):
                a.reset()
                per[kind][name].append(wall_ms(fn) / steps)
    for kind, a in arms.items():
        # the sampler alone, and the kernels of one step
        ops.TIMER = ops.KernelTimer()
        for _ in range(20):
            a.reset()
            a.gen.sample(a.state, TEMPERATURE, PENALTY, CONTEXT)
        torch.cuda.synchronize()
        sampler = sorted(s.elapsed_time(e) for _, _, _, s, e in ops.TIMER.records)
        a.reset()
        ops.TIMER = ops.KernelTimer()
        a._step()
        split = ops.TIMER.summary()
        ops.TIMER = None
        st = {k: stats(v) for k, v in per[kind].items()}
        gain = st["host"]["median"] - st["graph"]["median"]
        spread = max(st["host"]["max"] - st["host"]["min"], st["graph"]["max"] - st["graph"]["min"])
        # whole calls of generate(): prefill, capture and loop
        gen_ms = {}
        for name, kw in (("host", {}), ("device_graph", dict(device_loop=True)), ("device_eager", dict(device_loop=True, graph=False))):
            call = lambda: a.gen.generate(ids, mask, max_tokens=steps, temperature=TEMPERATURE, repetition_penalty=PENALTY,          # noqa: E731
                                          repetition_context=CONTEXT, eos_ids=(), seed=1, **kw)
            gen_ms[name] = round(min(wall_ms(call) for _ in range(2)), 2)
        res["panels"][kind] = {"ms_per_token": st, "host_minus_graph_ms": round(gain, 4), "larger_spread_ms": round(spread, 4),
                               "graph_beats_host_by_more_than_the_spread": bool(gain > spread),
                               "graph_nodes": a.nodes, "capture_ms": round(a.capture_ms, 2),
                               "library_calls_per_step": sum(d["launches"] for d in split.values()),
                               "kernel_ms_in_a_step": {f: round(d["ms"], 4) for f, d in split.items()},
                               "kernel_ms_in_a_step_sum": round(sum(d["ms"] for d in split.values()), 4),
                               "sampler_ms_V262208": {"median": round(sampler[len(sampler) // 2], 4), "min": round(sampler[0], 4),
                                                      "max": round(sampler[-1], 4)},
                               "generate_call_ms": gen_ms}
    doc = json.dumps(res, indent=1)
    print(doc, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
