"""Host cost of the operand checks of ``ops``, where it shows first: wall time of one EAGER ``forward_tokens`` of a
full-width model (D = 4096, 4 blocks) over M = 64 token rows (B = 1), so small that the kernels wait for the host.  (The
benchmark's step is one captured graph: host code is not in it.)  Median of 20 forwards after 3 warm-ups, each forward
synchronised; run it in alternating fresh processes for two trees: profiles/ops_shims_ab.log.
usage: python scripts/ab_ops_shims.py [--root TREE]   (TREE: the checkout whose mlx_video_amd is imported; default this one)
-> one line `eager_forward_ms median min max`"""
import argparse
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
sys.path[:0] = [os.path.abspath(ap.parse_args().root), HERE]
from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig, TimestepPlan, precompute_freqs_cis       # noqa: E402
from mlx_video_amd.schedulers import create_position_grid                                              # noqa: E402

if __name__ == "__main__":
    dev = torch.device("cuda:0")
    model = LTXModel.random_init(LTXModelConfig(num_layers=4), dev, seed=33)
    g = torch.Generator(device=dev).manual_seed(5)
    N, S = 64, 128
    tok = torch.randn((1, N, 128), generator=g, device=dev).to(torch.bfloat16)
    ctx = torch.randn((1, S, 3840), generator=g, device=dev).to(torch.bfloat16)
    pe = precompute_freqs_cis(create_position_grid(1, 1, 8, 8).to(dev), 4096)
    plan = TimestepPlan(torch.tensor([0.625], dtype=torch.bfloat16, device=dev), torch.zeros(N, dtype=torch.int32, device=dev))
    times = []
    for i in range(23):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.forward_tokens(tok, plan, ctx, pe)
        torch.cuda.synchronize()
        if i >= 3:
            times.append((time.perf_counter() - t0) * 1e3)
    print(f"eager_forward_ms {statistics.median(times):.4f} {min(times):.4f} {max(times):.4f}", flush=True)
