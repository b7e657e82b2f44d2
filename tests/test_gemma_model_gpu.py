"""mlx_video_amd.gemma.GemmaEncoder on the device: whole-model accuracy against the float64 restatement, batch invariance, and
the text route of generate_video / the CLI from token ids to the DiT's context.

Accuracy.  The tiny model of tests/test_gemma_cpu.py's comparison with transformers (hidden 512, 6 layers = 5 local + 1
global, 4 / 2 heads of 256; B = 2, T = 96, row 1 left-padded by 59), once with sliding_window 1024 and once with 16, where the
window mask bites.  The yardstick is computed here on the CPU, not pinned: e_ref[l] = rel-L2 on the valid rows of the bf16-policy
restatement (rounding at the header's rounding points, sums in float64) against float64, and the device must satisfy
err_device[l] <= 1.25 * e_ref[l] for every hidden state l.  The 1.25 exists because two bf16 evaluations with different
summation orders are samples of one error size, not ordered; it leaves no room for a fault - a wrong mask or head mapping moves a
state by >= 1e-1 against e_ref ~ 1e-2.  Both columns are printed and recorded in the parity ledger."""
import json

import numpy as np
import parity
import pytest
import torch

import ref_gemma as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _encoder(dev, cfg, seed=3):
    from mlx_video_amd.gemma import GemmaEncoder, random_gemma_weights
    W = random_gemma_weights("cpu", cfg, seed=seed)
    return W, GemmaEncoder({k: v.to(dev) for k, v in W.items()}, cfg)


@pytest.mark.parametrize("window", [1024, 16])
def test_whole_model_accuracy(dev, window):
    cfg = G.tiny_config(window)
    W, enc = _encoder(dev, cfg)
    ids, mask = G.tiny_inputs()
    got = enc(ids, mask)
    L = cfg.num_hidden_layers
    assert tuple(got.shape) == (L + 1, 2, 96, cfg.hidden_size) and got.dtype == BF and got.is_cuda
    again = enc(ids.to(dev), mask.to(dev))
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))
    f64 = G.forward(W, cfg, ids, mask, "f64")
    pol = G.forward(W, cfg, ids, mask, "bf16")
    assert bool(torch.isfinite(got.float()).all()), "padded rows must stay finite"
    rows = []
    for l in range(L + 1):
        e_ref, e_dev = G.rel_l2_valid(pol[l], f64[l], mask), G.rel_l2_valid(got[l], f64[l], mask)
        rows.append((l, e_ref, e_dev))
        print(f"window {window} state {l}: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    for l, e_ref, e_dev in rows:
        parity.auto(e_dev, 1.25 * e_ref, tag=f"state{l}")
    if window == 16:            # the window is really applied: the full-causal restatement is far away
        full = G.forward(W, G.tiny_config(1024), ids, mask, "f64")
        assert G.rel_l2_valid(got[L], full[L], mask) > 10 * rows[L][1]


def test_batch_invariance(dev):
    cfg = G.tiny_config(16)
    _, enc = _encoder(dev, cfg)
    ids, mask = G.tiny_inputs()
    both = enc(ids, mask)
    for b in range(2):
        one = enc(ids[b:b + 1], mask[b:b + 1])
        n = int(mask[b].sum())
        assert torch.equal(one[:, 0, 96 - n:].view(torch.int16), both[:, b, 96 - n:].view(torch.int16)), f"row {b} alone gives other bits"
    swapped = enc(ids.flip(0), mask.flip(0))
    for b in range(2):
        n = int(mask[b].sum())
        assert torch.equal(swapped[:, 1 - b, 96 - n:].view(torch.int16), both[:, b, 96 - n:].view(torch.int16))
    # (padded rows are compared too where they are defined: the whole tensor is a function of the row alone)
    assert torch.equal(swapped.flip(1).view(torch.int16), both.view(torch.int16))


# ------------------------------------------------------------------------------------------------ generate_video / CLI
def _small_gemma_cfg(hidden=256):
    from mlx_video_amd.gemma import GemmaConfig
    return GemmaConfig(hidden_size=hidden, num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1, head_dim=256,
                       intermediate_size=64, vocab_size=64, sliding_window=8, sliding_window_pattern=2, query_pre_attn_scalar=256.0,
                       rope_scaling_factor=8.0)


def _tokens(T, n, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(1, T, dtype=torch.int64)
    mask = torch.zeros(1, T, dtype=torch.int64)
    ids[0, T - n:] = torch.randint(1, 64, (n,), generator=g)
    mask[0, T - n:] = 1
    return ids, mask


def test_generate_video_text_route(dev):
    """tokens -> GemmaEncoder -> TextConnector -> context inside generate_video gives the latents of feeding the same encoder's
    output through gemma_hidden_states=; the older routes give the bits they give with the new arguments absent."""
    from mlx_video_amd.generate import PipelineType, generate_video
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    from test_pipeline_gpu import _mods, _Noise
    m = _mods(dev)
    cfg = _small_gemma_cfg()
    _, enc = _encoder(dev, cfg, seed=9)
    conn = TextConnector(random_connector_weights(dev, D=256, L=cfg.num_hidden_layers + 1, layers=1, R=16))
    T = 32
    pos, neg = _tokens(T, 11, 1), _tokens(T, 5, 2)
    common = dict(prompt="x", pipeline=PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
                  transformer=m["transformer"], vae_decoder=m["vae_decoder"], compile_step=True, cfg_batch=True, device=dev,
                  return_latents=True)
    a = generate_video(gemma=enc, prompt_tokens=pos, negative_prompt_tokens=neg, text_connector=conn, noise_fn=_Noise(7, dev), **common)
    hs = enc(torch.cat([pos[0], neg[0]]), torch.cat([pos[1], neg[1]]))
    hidden = dict(gemma_hidden_states=hs[:, 0:1], gemma_attention_mask=pos[1], negative_gemma_hidden_states=hs[:, 1:2],
                  negative_gemma_attention_mask=neg[1], text_connector=conn)
    b = generate_video(noise_fn=_Noise(7, dev), **hidden, **common)
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    # the context depends on the prompt: other tokens, other latents
    c = generate_video(gemma=enc, prompt_tokens=_tokens(T, 11, 3), negative_prompt_tokens=neg, text_connector=conn, noise_fn=_Noise(7, dev), **common)
    assert not torch.equal(a, c)
    # the older routes keep their bits (and their precedence) with the new arguments present
    b2 = generate_video(noise_fn=_Noise(7, dev), gemma=enc, prompt_tokens=_tokens(T, 11, 3), negative_prompt_tokens=neg, **hidden, **common)
    assert torch.equal(b, b2)
    g = torch.Generator().manual_seed(50)
    pe = dict(prompt_embeds=torch.randn(1, 64, 256, generator=g).to(BF), negative_prompt_embeds=torch.randn(1, 64, 256, generator=g).to(BF))
    d = generate_video(noise_fn=_Noise(7, dev), **pe, **common)
    d2 = generate_video(noise_fn=_Noise(7, dev), gemma=enc, prompt_tokens=pos, negative_prompt_tokens=neg, text_connector=conn, **pe, **common)
    assert torch.equal(d, d2) and not torch.equal(d, a)


def _write_gemma_dir(root, cfg, W, with_tokenizer):
    from safetensors.torch import save_file
    root.mkdir(parents=True, exist_ok=True)
    save_file({"language_model.model." + k: v.contiguous() for k, v in W.items()}, str(root / "model.safetensors"))
    (root / "config.json").write_text(json.dumps({"text_config": dict(
        hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        num_key_value_heads=cfg.num_key_value_heads, head_dim=256, intermediate_size=cfg.intermediate_size, vocab_size=cfg.vocab_size,
        sliding_window=cfg.sliding_window, sliding_window_pattern=cfg.sliding_window_pattern, query_pre_attn_scalar=256,
        rms_norm_eps=1e-6, rope_theta=1e6, rope_local_base_freq=1e4, rope_scaling={"rope_type": "linear", "factor": 8.0})}))
    if with_tokenizer:
        from test_gemma_cpu import _write_tokenizer
        _write_tokenizer(root)


def test_cli_gemma_repo(dev, tmp_path, monkeypatch):
    """`generate --synthetic --gemma-repo DIR --prompt-tokens FILE` on a directory written here (a 2-layer Gemma of the real
    width, so that its context fits the synthetic DiT) runs to a video of the right shape, and `--prompt` with the directory's
    tokenizer.json takes the tokenizer route."""
    pytest.importorskip("tokenizers")
    from mlx_video_amd import generate as GV
    from mlx_video_amd.gemma import random_gemma_weights
    cfg = _small_gemma_cfg(hidden=3840)
    root = tmp_path / "gemma"
    _write_gemma_dir(root, cfg, random_gemma_weights("cpu", cfg, seed=4), with_tokenizer=True)
    T = 128
    for name, n, seed in (("pos", 9, 1), ("neg", 4, 2)):
        ids, mask = _tokens(T, n, seed)
        np.savez(tmp_path / f"{name}.npz", input_ids=ids.numpy(), attention_mask=mask.numpy())
    seen = []
    real = GV._encode_gemma

    def spy(*a):
        out = real(*a)
        seen.append(tuple(out[1].shape))
        return out

    monkeypatch.setattr(GV, "_encode_gemma", spy)
    base = ["--synthetic", "--layers", "1", "--pipeline", "distilled", "--height", "128", "--width", "128", "--num-frames", "9",
            "--stage1-steps", "1", "--stage2-steps", "1", "--tiling", "none", "--gemma-repo", str(root)]
    out = tmp_path / "tok.npy"
    GV.main(base + ["--prompt-tokens", str(tmp_path / "pos.npz"), "--negative-prompt-tokens", str(tmp_path / "neg.npz"), "--output-path", str(out)])
    frames = np.load(out)
    assert frames.shape == (9, 128, 128, 3) and frames.dtype == np.uint8 and seen == [(2, T)]
    out2 = tmp_path / "prompt.npy"
    GV.main(base + ["--prompt", "a b c", "--negative-prompt", "c", "--output-path", str(out2)])
    assert np.load(out2).shape == (9, 128, 128, 3) and seen[1] == (2, 1024)            # tokenised and left-padded to 1024
