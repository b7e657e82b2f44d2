"""Host cost of the VAE call shims: the 33x512x512 decode of bench.py (video_vae.bench_decode) and the small-tile
temporal tiled decode of 97 frames (13 x 2 x 2 latent, one res block per stage - the shape of
tests/test_configs_gpu.py, where launches are tiny and host time shows first), one JSON line per process.
usage: python scripts/ab_vae_shims.py [--root TREE] [--iters N]   (alternate TREE between two checkouts: profiles/vae_shims_ab.log)"""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
sys.path[:0] = [os.path.abspath(args.root), HERE]
from mlx_video_amd import video_vae as V                                                   # noqa: E402

if __name__ == "__main__":
    dev = torch.device("cuda:0")
    out = {"root": os.path.abspath(args.root), "vae_decode_ms": V.bench_decode(dev, 5, 16, 16)["vae_decode_ms"]}
    dec = V.LTX2VideoDecoder(V.random_decoder_weights(dev, layers=1), num_layers_per_block=1)
    lat = torch.randn((1, 128, 13, 2, 2), generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(dev)
    tc = V.TilingConfig.auto(512, 512, 97)
    times = []
    for i in range(args.iters + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.decode_tiled(lat, tiling_config=tc, tiling_mode="auto")
        torch.cuda.synchronize()
        if i >= 3:
            times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    out.update(tiled_decode_97f_ms_median=times[len(times) // 2], tiled_decode_97f_ms_min=times[0])
    print(json.dumps(out), flush=True)
