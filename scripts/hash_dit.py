"""SHA-256 of what the DiT half writes on seeded inputs: ``forward_tokens`` of a 2-block model at D = 512 under every ``fuse``
setting the tests use, with and without a ContextKV, with bf16 weights, fp8 weights and fp8 activations, with an STG-skipped
row and with the per-block (non-grouped) context path; the step tail under cfg, cfg_star and apg, with and without mask
blend and device sigmas; the text connector and a two-layer Gemma encoder at test size.  Inputs and weights are seeded, so
two trees of host code over one library must print identical lines: profiles/ops_shims_bits.txt.
usage: python scripts/hash_dit.py [--root TREE]   (TREE: the checkout whose mlx_video_amd is imported; default this one)
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
from mlx_video_amd import ops                                                                                          # noqa: E402
from mlx_video_amd.gemma import GemmaConfig, GemmaEncoder, random_gemma_weights                                        # noqa: E402
from mlx_video_amd.guidance import BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType      # noqa: E402
from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig, TimestepPlan, precompute_freqs_cis                       # noqa: E402
from mlx_video_amd.text_connector import TextConnector, random_connector_weights                                       # noqa: E402
from mlx_video_amd.weights import transformer_weights                                                                  # noqa: E402
from oracle import dit as O                                                                                            # noqa: E402

BF = torch.bfloat16
dev = torch.device("cuda:0")


def emit(name, t):
    torch.cuda.synchronize()
    h = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
    print(f"{name} {tuple(t.shape)} {h}", flush=True)


def rnd(gen, *shape):
    return torch.randn(shape, generator=gen).to(BF).to(dev)


def dit():
    cfg = O.DiTConfig(num_layers=2, heads=4, caption_channels=256)
    mc = LTXModelConfig(num_attention_heads=4, num_layers=2, caption_channels=256, cross_attention_dim=cfg.dim)
    W = O.make_weights(cfg, seed=11)
    B, F, Hh, Ww, S = 2, 3, 5, 6, 100
    N = F * Hh * Ww
    g = torch.Generator().manual_seed(42)
    lat, ctx = rnd(g, B, N, 128), rnd(g, B, S, cfg.caption_channels)
    ts = torch.full((B, N), 0.909375).to(BF)
    ts[:, : Hh * Ww] = 0.0                                        # two timestep rows: the token -> row map is read
    plan = TimestepPlan.from_timesteps(ts.to(dev))
    pos = torch.from_numpy(O.create_position_grid(B, F, Hh, Ww)).to(dev)
    weights = {"bf16": {k: v.to(dev) for k, v in W.items()}, "fp8": transformer_weights(W, dev, fp8=True, fp8_scaling="channel")}
    skip = PerturbationConfig([Perturbation(PerturbationType.SKIP_VIDEO_SELF_ATTN, [1])])
    pert = BatchedPerturbationConfig([PerturbationConfig.empty(), skip])
    for tag, wkey, kw in (("bf16", "bf16", {}), ("fp8", "fp8", {}), ("fp8act", "fp8", dict(fp8_activations=True))):
        for fuse in (15, 0, 7, 14, 15 | 8):
            m = LTXModel(mc, weights[wkey], fuse=fuse, **kw)
            pe = precompute_freqs_cis(pos, m.inner_dim, m.positional_embedding_theta, m.positional_embedding_max_pos, m.num_attention_heads)
            emit(f"forward.{tag}.fuse{fuse}", m.forward_tokens(lat, plan, ctx, pe))
            emit(f"forward.{tag}.fuse{fuse}.context_kv", m.forward_tokens(lat, plan, ctx, pe, ctx_kv=m.prepare_context(ctx)))
            emit(f"forward.{tag}.fuse{fuse}.stg_row1", m.forward_tokens(lat, plan, ctx, pe, perturbations=pert))
        m = LTXModel(mc, weights[wkey], **kw)
        m.grouped_context_kv = False
        emit(f"forward.{tag}.per_block_context", m.forward_tokens(lat, plan, ctx, pe))
        m.grouped_context_kv, m.batch_invariant = True, True
        emit(f"forward.{tag}.batch_invariant", m.forward_tokens(lat, plan, ctx, pe))


def step_tails():
    B, C, S = 2, 128, 3 * 5 * 6
    g = torch.Generator().manual_seed(43)
    vp, vn, vq = rnd(g, B, S, C), rnd(g, B, S, C), rnd(g, B, S, C)
    x, clean = rnd(g, B, C, 3, 5, 6), rnd(g, B, C, 3, 5, 6)
    mask = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (B, S), generator=g)].to(dev)
    sig = torch.tensor([0.7, 0.4], dtype=torch.float32, device=dev)
    for masked in (False, True):
        for dev_sig in (False, True):
            kw = dict(clean=clean if masked else None, mask_tok=mask if masked else None, sigmas_dev=sig if dev_sig else None)
            tag = f"mask{int(masked)}.devsig{int(dev_sig)}"
            emit(f"step_tail.cfg.{tag}", ops.step_tail(vp, vn, vq, x, cfg_scale=4.0, stg_scale=1.5, sigma=0.7, sigma_next=0.4, **kw))
            emit(f"step_tail.cfg.no_stg.{tag}", ops.cfg_euler_step(vp, vn, x, 4.0, 0.7, 0.4, **kw))
            for guider, thr in (("cfg_star", 0.0), ("apg", 0.0), ("apg", 12.0)):
                rec = ops.guidance_sums(vp, vn, x, guider, 0.7, thr, sigmas_dev=kw["sigmas_dev"])
                emit(f"guidance_sums.{guider}.thr{thr:g}.{tag}", rec)
                emit(f"step_tail.{guider}.thr{thr:g}.{tag}", ops.step_tail(vp, vn, vq, x, cfg_scale=4.0, stg_scale=1.5, sigma=0.7, sigma_next=0.4,
                                                                       guider=guider, record=rec, eta=0.8, norm_threshold=thr, **kw))
    emit("euler_only", ops.euler_only(x, clean, 0.7, 0.4))
    emit("latent_to_tokens.rep2", ops.latent_to_tokens(x, rep=2))


def text():
    D, L, T = 256, 3, 32
    tc = TextConnector(random_connector_weights(dev, D=D, L=L, layers=2, R=16, seed=29))
    g = torch.Generator().manual_seed(44)
    hs = rnd(g, L, 2, T, D)
    mask = torch.ones(2, T, dtype=torch.int64)
    mask[1, :21] = 0
    emit("text_connector", tc(hs, mask))
    emit("text_connector.batch_row_view", tc(hs[:, 1:2], mask[1:2]))
    cfg = GemmaConfig(hidden_size=D, num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1, head_dim=256, intermediate_size=64,
                      vocab_size=64, sliding_window=8, sliding_window_pattern=2, query_pre_attn_scalar=256.0, rope_scaling_factor=8.0)
    enc = GemmaEncoder({k: v.to(dev) for k, v in random_gemma_weights("cpu", cfg, seed=9).items()}, cfg)
    ids = torch.randint(1, 64, (2, T), generator=g)
    ids[1, :21] = 0
    states = enc(ids, mask)
    emit("gemma_encoder.2_layers", states)
    emit("gemma_encoder.then_connector", tc(states, mask))


if __name__ == "__main__":
    dit()
    step_tails()
    text()
