"""Audio decode at full size on the device: per-stage kernel times, fraction of the bf16 MFMA peak, and the same graph through
torch's own bf16 convolutions (MIOpen) in the same process.

    python scripts/prof_audio_decode.py [--frames 126] [--out profiles/audio_decode.json]

Full-size random weights (fan-in^-1/2), 126 latent frames = 501 mel frames = 5.01 s of 24 kHz stereo.  Per stage: the sum of
the HIP-event times of its launches (ops.KernelTimer), the algorithmic FLOPs of its convolutions, FLOPs / time against the dense
bf16 MFMA peak.  The totals are wall times between two events around the whole decode, median of --reps runs after --warmup.
The torch graph is the reference's module structure (pad + conv2d, PixelNorm, SiLU; conv1d / conv_transpose1d, leaky ReLU, the
mean of three blocks, tanh) on channels-first bf16 tensors, stage times between events at the same boundaries.  torch's build
carries no precompiled MIOpen kernels for gfx950, so its first pass compiles one per convolution shape; that pass runs stage by
stage against --torch-budget-s, and where it does not finish the JSON says so, names the stages that did, and carries the
roofline fractions alone.  The JSON is written once after this package's leg and again at the end; progress goes to stderr."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch
import torch.nn.functional as F

import ref_audio as A
from mlx_video_amd import ops
from mlx_video_amd.audio_vae import AudioDecoder, Vocoder

PEAK_BF16_DENSE_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (bench.py)
BF = torch.bfloat16


def stage_of(name):
    """Stage label of a ``_note`` name: decoder levels and vocoder stages, one row each."""
    if name.startswith("up."):
        return "dec." + ".".join(name.split(".")[:2])
    if name.startswith(("conv_in", "mid.")):
        return "dec.in+mid"
    if name == "conv_out":
        return "dec.conv_out"
    if name == "conv_pre.leaky":
        return "voc.conv_pre"
    i = name.split(".")[1]
    return f"voc.stage{i}"


def run_ours(dec, voc, lat, timer_on):
    marks = []
    ops.TIMER = ops.KernelTimer() if timer_on else None

    def hook(name, t):
        if timer_on:
            marks.append((name, len(ops.TIMER.records)))

    dec._note = hook
    voc._note = hook
    wav = voc(dec(lat))
    if timer_on:
        marks.append(("voc.conv_post", len(ops.TIMER.records)))
    timer, ops.TIMER = ops.TIMER, None
    return wav, timer, marks


def torch_graph(Wd, Wv, lat, ev):
    """The reference's modules on torch bf16 convolutions, channels-first; ev(name) records an event at a stage boundary."""
    def conv2(x, name):
        w = Wd[f"{name}.conv.weight"]
        if w.shape[1] == 3:
            x = F.pad(x, (1, 1, 2, 0))
        return F.conv2d(x, w.permute(0, 3, 1, 2), Wd[f"{name}.conv.bias"])

    def pn_silu(x):
        return F.silu(x / torch.sqrt((x * x).mean(1, keepdim=True) + 1e-6))

    def block(x, name):
        h = conv2(pn_silu(x), f"{name}.conv1")
        h = conv2(pn_silu(h), f"{name}.conv2")
        if f"{name}.nin_shortcut.conv.weight" in Wd:
            x = conv2(x, f"{name}.nin_shortcut")
        return x + h

    B, C, T, Fb = lat.shape
    x = lat * Wd["per_channel_statistics._std_of_means"].view(1, C, 1, Fb) + Wd["per_channel_statistics._mean_of_means"].view(1, C, 1, Fb)
    h = conv2(x, "conv_in")
    for i in (1, 2):
        h = block(h, f"mid.block_{i}")
    ev("dec.in+mid")
    for level in (2, 1, 0):
        for i in range(3):
            h = block(h, f"up.{level}.block.{i}")
        if level:
            h = h.repeat_interleave(2, 2).repeat_interleave(2, 3)
            h = conv2(h, f"up.{level}.upsample.conv")[:, :, 1:]
        ev(f"dec.up.{level}")
    h = conv2(pn_silu(h), "conv_out")[:, :, :4 * T - 3, :64]
    ev("dec.conv_out")
    x = h.permute(0, 1, 3, 2).reshape(B, 128, -1)

    def c1(x, name, d=1):
        w = Wv[f"{name}.weight"]
        return F.conv1d(x, w.permute(0, 2, 1), Wv[f"{name}.bias"], padding=(w.shape[1] - 1) * d // 2, dilation=d)

    x = c1(x, "conv_pre")
    ev("voc.conv_pre")
    for i, s in enumerate(A.VOC_RATES):
        w = Wv[f"ups.{i}.weight"]
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), w.permute(2, 0, 1), Wv[f"ups.{i}.bias"], stride=s, padding=(w.shape[1] - s) // 2)
        outs = []
        for k in range(3):
            y = x
            for d, dil in enumerate(A.VOC_DILATIONS[k]):
                t = c1(F.leaky_relu(y, 0.1), f"resblocks.{3 * i + k}.convs1.{d}", dil)
                t = c1(F.leaky_relu(t, 0.1), f"resblocks.{3 * i + k}.convs2.{d}")
                y = t + y
            outs.append(y)
        x = (outs[0] + outs[1] + outs[2]) / 3
        ev(f"voc.stage{i}")
    x = torch.tanh(c1(F.leaky_relu(x, 0.01), "conv_post").float())
    ev("voc.conv_post")
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=126)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_decode.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-budget-s", type=float, default=300.0, help="time the torch leg's first (kernel-compiling) pass may take")
    args = ap.parse_args()
    dev = torch.device("cuda:0")

    def say(msg):
        print(f"[prof_audio_decode] {msg}", file=sys.stderr, flush=True)

    def dump(rep):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)

    Wd = {k: v.to(dev) for k, v in A.make_decoder_weights(seed=1).items()}
    Wv = {k: v.to(dev) for k, v in A.make_vocoder_weights(seed=2).items()}
    dec, voc = AudioDecoder(Wd), Vocoder(Wv)
    lat = torch.randn(1, 8, args.frames, 16, generator=torch.Generator().manual_seed(3)).to(BF).to(dev)

    def wall(fn):
        ts = []
        for i in range(args.warmup + args.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(s.elapsed_time(e))
        return statistics.median(ts), ts

    say("weights on the device; timing this package's decode")
    ours_ms, ours_all = wall(lambda: run_ours(dec, voc, lat, False))
    say(f"decode wall {ours_ms:.3f} ms; per-launch events")
    wav, timer, marks = run_ours(dec, voc, lat, True)
    torch.cuda.synchronize()
    stages, lo = {}, 0
    for name, hi in marks:
        st = stages.setdefault(name if name == "voc.conv_post" else stage_of(name), {"launches": 0, "kernel_ms": 0.0, "conv_flops": 0.0})
        for fam, flops, nbytes, s, e in timer.records[lo:hi]:
            st["launches"] += 1
            st["kernel_ms"] += s.elapsed_time(e)
            st["conv_flops"] += flops
        lo = hi
    for st in stages.values():
        st["tflops"] = st["conv_flops"] / (st["kernel_ms"] * 1e-3) / 1e12 if st["kernel_ms"] else 0.0
        st["frac_of_bf16_mfma_peak"] = st["tflops"] / PEAK_BF16_DENSE_TFLOPS
    total_flops = sum(st["conv_flops"] for st in stages.values())
    kernel_ms = sum(st["kernel_ms"] for st in stages.values())
    rep = {"latent_frames": args.frames, "samples": int(wav.shape[-1]), "seconds_of_audio": wav.shape[-1] / 24000.0,
           "device": torch.cuda.get_device_name(0), "peak_bf16_dense_tflops": PEAK_BF16_DENSE_TFLOPS,
           "ours": {"wall_ms_median": ours_ms, "wall_ms_runs": ours_all, "kernel_ms_sum": kernel_ms, "conv_tflop": total_flops / 1e12,
                    "frac_of_bf16_mfma_peak_kernel_time": total_flops / (kernel_ms * 1e-3) / 1e12 / PEAK_BF16_DENSE_TFLOPS,
                    "stages": stages}}
    dump(rep)
    say(f"kernel time {kernel_ms:.3f} ms, {total_flops / 1e12:.3f} TFLOP; written {args.out}")
    if not args.no_torch:
        done, t0 = [], time.perf_counter()

        def first_pass(name):
            torch.cuda.synchronize()
            done.append(name)
            say(f"torch first pass: {name} done at {time.perf_counter() - t0:.1f} s")
            if time.perf_counter() - t0 > args.torch_budget_s:
                raise TimeoutError(f"the first pass (MIOpen compiling a kernel per convolution shape) passed {args.torch_budget_s:.0f} s "
                                   f"after {len(done)} of 12 stages: {', '.join(done)}")

        try:
            torch_graph(Wd, Wv, lat, first_pass)
            evs = []

            def ev(name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                evs.append((name, e))

            t_ms, t_all = wall(lambda: torch_graph(Wd, Wv, lat, lambda n: None))
            s0 = torch.cuda.Event(enable_timing=True)
            s0.record()
            ref = torch_graph(Wd, Wv, lat, ev)
            torch.cuda.synchronize()
            tst, prev = {}, s0
            for name, e in evs:
                tst[name] = prev.elapsed_time(e)
                prev = e
            rel = float((wav[0].double() - ref[0].double()).norm() / ref[0].double().norm())
            ours_stage_wall = {k: v["kernel_ms"] for k, v in stages.items()}
            rep["torch_bf16"] = {"wall_ms_median": t_ms, "wall_ms_runs": t_all, "stage_ms": tst, "waveform_rel_l2_ours_vs_torch": rel,
                                 "stages_where_ours_is_slower": sorted(k for k in tst if ours_stage_wall.get(k, 0.0) > tst[k])}
            rep["ours_over_torch"] = ours_ms / t_ms
        except Exception as exc:                                       # torch's conv path cannot run here: say so
            rep["torch_bf16"] = {"error": f"{type(exc).__name__}: {exc}"}
    dump(rep)
    print(json.dumps({k: rep[k] for k in rep if k != "ours"} | {"ours_wall_ms": ours_ms, "ours_kernel_ms": kernel_ms}, sort_keys=True))


if __name__ == "__main__":
    main()
