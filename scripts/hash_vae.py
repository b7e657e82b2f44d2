"""SHA-256 of what the VAE half writes on seeded inputs: the decoder (1 and 5 res blocks per stage, causal and not,
timestep-conditioned), uint8 frames, the encoder at 9x64x64, the latent upsampler with its (de)normalisation, and one
tiled decode with ragged tiles on every axis.  Inputs and weights are seeded, so two trees of host code over one
library must print identical lines: profiles/vae_shims_bits.txt.
usage: python scripts/hash_vae.py [--root TREE]   (TREE: the checkout whose mlx_video_amd is imported; default this one)
-> one `name shape sha256` line per case"""
import argparse
import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
sys.path[:0] = [os.path.abspath(ap.parse_args().root), HERE]
from mlx_video_amd import upsampler as U, video_vae as V                                   # noqa: E402
from oracle import vae as OV                                                               # noqa: E402

BF = torch.bfloat16
dev = torch.device("cuda:0")


def emit(name, t):
    torch.cuda.synchronize()
    h = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
    print(f"{name} {tuple(t.shape)} {h}", flush=True)


def lat(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF).to(dev)


def to_dev(W):
    return {k: v.to(dev) for k, v in W.items()}


if __name__ == "__main__":
    for layers in (1, 5):
        dec = V.LTX2VideoDecoder(V.random_decoder_weights(dev, layers=layers), num_layers_per_block=layers)
        for causal in (False, True):
            vid = dec(lat((1, 128, 2, 4, 4), 10 + layers), causal=causal)
            emit(f"decode.layers{layers}.causal{int(causal)}", vid)
        emit(f"to_uint8_frames.layers{layers}", V.to_uint8_frames(vid))
    dec = V.LTX2VideoDecoder(to_dev(OV.make_decoder_weights(seed=22, layers_per_block=1, timestep_conditioning=True)),
                             timestep_conditioning=True, num_layers_per_block=1)
    emit("decode.timestep_conditioned", dec(lat((2, 128, 1, 2, 2), 5), noise=lat((2, 128, 1, 2, 2), 6)))
    dec = V.LTX2VideoDecoder(V.random_decoder_weights(dev, layers=1), num_layers_per_block=1)
    tc = V.TilingConfig(V.SpatialTilingConfig(64, 32), V.TemporalTilingConfig(16, 8))
    emit("decode_tiled.s64_32.t16_8", dec.decode_tiled(lat((1, 128, 4, 3, 5), 7), tc))
    enc = V.VideoEncoder(V.random_encoder_weights(dev))
    vid = (torch.rand((1, 3, 9, 64, 64), generator=torch.Generator().manual_seed(8)) * 2 - 1).to(BF).to(dev)
    emit("encode.9x64x64", enc(vid))
    up = U.LatentUpsampler(to_dev(OV.make_upsampler_weights(mid=128, nb=2)), num_blocks_per_stage=2)
    g = torch.Generator().manual_seed(9)
    mean = (torch.randn(128, generator=g) * 0.1).to(BF).to(dev)
    std = (1 + 0.1 * torch.randn(128, generator=g)).abs().to(BF).to(dev)
    emit("upsample_latents", U.upsample_latents(lat((1, 128, 3, 4, 5), 8), up, mean, std))
