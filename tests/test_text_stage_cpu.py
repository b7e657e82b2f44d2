"""Host side of the text stage (text_connector.py, weights.text_connector_weights, the generate CLI) and the CPU
restatement the GPU tests measure against (ref_text.py).  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

import ref_text as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
F64 = torch.float64
TEXT_SYMBOLS = ("ltxk_masked_layer_stats", "ltxk_layer_norm_compact", "ltxk_rmsnorm_rows", "ltxk_qknorm_rope_1d", "ltxk_gelu_erf",
                "ltxk_connector_assemble")


def test_symbols_exported_and_bound():
    import __graft_entry__ as ge
    from mlx_video_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ltxk.h")).read()
    for name in TEXT_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"int {name}(" in hdr
    for name in ("masked_layer_stats", "layer_norm_compact", "rmsnorm_rows", "qknorm_rope_1d", "gelu_erf_", "connector_assemble"):
        assert callable(getattr(ops, name))
    assert lib.ltxk_version() >= 408
    # the depth the sum's bound is derived from: 30 terms per slot at the full prompt, plus the fixed trees
    assert ops.layer_stats_depth(1024, 3840) == 30 + 17 and ops.layer_stats_depth(1, 384) == 1 + 17
    # argument checks run on the host before anything is launched
    assert lib.ltxk_gelu_erf(None, 8, None) == -1
    assert lib.ltxk_rmsnorm_rows(4096, 3844, 4096, 3844, 1, 3844, 1e-6, None) == -1          # D % 8
    assert lib.ltxk_qknorm_rope_1d(4096, 768, 1, 384, 4096, 4096, 4096, 4, 4, 1e-6, None) == -1    # D != 128 H
    with pytest.raises(_lib.LtxkError, match="no CPU fallback"):
        ops.rmsnorm_rows(torch.zeros(2, 384, dtype=BF))


def test_rope_table_matches_float64_formula():
    from mlx_video_amd.text_connector import rope_table_1d
    for T, H in ((256, 3), (1024, 30)):
        cos, sin = rope_table_1d(T, H)
        assert cos.shape == sin.shape == (H, T, 64) and cos.dtype == torch.float32 and cos.is_contiguous()
        # written out again: frequency i of head h is theta^((64h + i) / (64H - 1)) * pi/2, position 2t/4096 - 1
        h, t, i = H - 1, T - 3, 17
        f = 10000.0 ** ((64 * h + i) / (64 * H - 1)) * math.pi / 2
        a = (2 * t / 4096 - 1) * f
        want_c = float(torch.tensor(math.cos(a), dtype=torch.float32).to(BF))
        want_s = float(torch.tensor(math.sin(a), dtype=torch.float32).to(BF))
        assert float(cos[h, t, i]) == want_c and float(sin[h, t, i]) == want_s
        c64, s64 = RT.rope_table(T, H, RT.P64)
        cb, sb = RT.rope_table(T, H, RT.PBF)
        assert torch.equal(cos.double(), cb) and torch.equal(sin.double(), sb)          # the tables carry the bf16 rounding point
        tol = 2.0 ** -9 + 2.0 ** -24              # |value| <= 1: half a bf16 ulp below 1, on top of the fp32 cast
        assert float((cos.double() - c64).abs().max()) <= tol and float((sin.double() - s64).abs().max()) <= tol
        assert torch.equal(cos.to(BF).float(), cos)


def _connector_sd(D=128, L=3, R=4, layers=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(BF)
    sd = {"learnable_registers": rn(R, D)}
    for i in range(layers):
        p = f"transformer_1d_blocks.{i}."
        for n in ("to_q", "to_k", "to_v"):
            sd[p + f"attn1.{n}.weight"], sd[p + f"attn1.{n}.bias"] = rn(D, D), rn(D)
        sd[p + "attn1.to_out.0.weight"], sd[p + "attn1.to_out.0.bias"] = rn(D, D), rn(D)
        sd[p + "attn1.q_norm.weight"], sd[p + "attn1.k_norm.weight"] = rn(D), rn(D)
        sd[p + "ff.net.0.proj.weight"], sd[p + "ff.net.0.proj.bias"] = rn(4 * D, D), rn(4 * D)
        sd[p + "ff.net.2.weight"], sd[p + "ff.net.2.bias"] = rn(D, 4 * D), rn(D)
    return sd, rn(D, D * L)


@pytest.mark.parametrize("family", [0, 1, 2])
def test_key_families_load(tmp_path, family):
    from safetensors.torch import save_file
    from mlx_video_amd.weights import aggregate_k_from_layer_major, text_connector_weights
    D, L = 128, 3
    sd, agg = _connector_sd(D, L)
    agg_key, prefix = [("text_embedding_projection.aggregate_embed.weight", "model.diffusion_model.video_embeddings_connector."),
                       ("text_embedding_projection.aggregate_embed.weight", "connector.video_embeddings_connector."),
                       ("text_proj_in.weight", "video_connector.")][family]
    audio = ["model.diffusion_model.audio_embeddings_connector.", "connector.audio_embeddings_connector.", "audio_connector."][family]
    raw = {prefix + k: v for k, v in sd.items()}
    raw[agg_key] = agg
    raw.update({audio + k: torch.full_like(v, 7.0) for k, v in sd.items()})                 # must be ignored
    raw["model.diffusion_model.transformer_blocks.0.attn1.to_q.weight"] = torch.zeros(8, 8, dtype=BF)
    path = tmp_path / ("diffusion_pytorch_model.safetensors" if family == 2 else "ltx-2-synthetic.safetensors")
    save_file({k: v.contiguous() for k, v in raw.items()}, str(path))
    W = text_connector_weights([path], "cpu")
    want = {k.replace(".to_out.0.", ".to_out.").replace(".ff.net.0.proj.", ".ff.proj_in.").replace(".ff.net.2.", ".ff.proj_out."): v
            for k, v in sd.items()}
    assert set(W) == set(want) | {"aggregate_embed.weight_layer_major"}
    for k, v in want.items():
        assert torch.equal(W[k], v), k
    lm = W["aggregate_embed.weight_layer_major"]
    assert lm.shape == agg.shape and torch.equal(aggregate_k_from_layer_major(lm, D), agg)        # the permutation round-trips
    l, d, n = 2, 77, 5
    assert lm[n, l * D + d] == agg[n, d * L + l]                                                  # and is the stated one
    with pytest.raises(ValueError, match="no text connector"):
        other = tmp_path / "other.safetensors"
        save_file({"x": torch.zeros(2)}, str(other))
        text_connector_weights([other], "cpu")


def test_first_family_wins_over_connectors_file(tmp_path):
    from safetensors.torch import save_file
    from mlx_video_amd.weights import text_connector_weights
    sd, agg = _connector_sd(seed=1)
    sd2, agg2 = _connector_sd(seed=2)
    a, b = tmp_path / "main.safetensors", tmp_path / "diffusion_pytorch_model.safetensors"
    save_file({**{"model.diffusion_model.video_embeddings_connector." + k: v for k, v in sd.items()},
               "text_embedding_projection.aggregate_embed.weight": agg}, str(a))
    save_file({**{"video_connector." + k: v for k, v in sd2.items()}, "text_proj_in.weight": agg2}, str(b))
    W = text_connector_weights([b, a], "cpu")
    assert torch.equal(W["learnable_registers"], sd["learnable_registers"])


def test_mask_validation():
    from mlx_video_amd.text_connector import TextConnector, mask_row_counts, random_connector_weights
    assert mask_row_counts(torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0]])) == [2, 4, 0]
    assert mask_row_counts(torch.tensor([[0.0, 1.0]])) == [1]
    for bad in ([[1, 1, 0, 0]], [[0, 1, 0, 1]], [[1, 0, 1, 1]]):
        with pytest.raises(ValueError, match="left-padded"):
            mask_row_counts(torch.tensor(bad))
    with pytest.raises(ValueError, match="0 / 1"):
        mask_row_counts(torch.tensor([[0, 2]]))
    tc = TextConnector(random_connector_weights("cpu", D=128, L=2, layers=1, R=8))
    assert (tc.D, tc.H, tc.R, tc.L, len(tc.blocks)) == (128, 1, 8, 2, 1)
    hs = torch.zeros(2, 1, 12, 128, dtype=BF)
    with pytest.raises(ValueError, match="not a multiple of the 8 learnable registers"):
        tc(hs, torch.ones(1, 12, dtype=torch.int64))
    with pytest.raises(ValueError, match="left-padded"):
        tc(torch.zeros(2, 1, 16, 128, dtype=BF), torch.tensor([[1] * 8 + [0] * 8]))
    with pytest.raises(ValueError, match="per layer"):
        tc(torch.zeros(2, 1, 8, 128, dtype=BF), torch.ones(1, 16, dtype=torch.int64))


def test_cli_parses_gemma_flags(tmp_path):
    from safetensors.torch import save_file
    from mlx_video_amd import generate as G
    args = G.build_parser().parse_args(["--gemma-hidden-states", "p.pt", "--negative-gemma-hidden-states", "n.safetensors"])
    assert args.gemma_hidden_states == "p.pt" and args.negative_gemma_hidden_states == "n.safetensors"
    assert G.build_parser().parse_args([]).gemma_hidden_states is None
    hs, mask = torch.randn(3, 8, 16).to(BF), torch.tensor([0, 0, 0, 1, 1, 1, 1, 1])
    torch.save({"hidden_states": hs, "attention_mask": mask}, tmp_path / "p.pt")
    save_file({"hidden_states": hs[:, None].contiguous(), "attention_mask": mask}, str(tmp_path / "n.safetensors"))
    for f in ("p.pt", "n.safetensors"):
        h, m = G.load_gemma_hidden_states(str(tmp_path / f))
        assert h.shape == (3, 1, 8, 16) and m.shape == (1, 8) and torch.equal(h[:, 0], hs) and torch.equal(m[0], mask)
    torch.save({"hidden_states": hs, "attention_mask": mask[:5]}, tmp_path / "bad.pt")
    with pytest.raises(ValueError, match="positions"):
        G.load_gemma_hidden_states(str(tmp_path / "bad.pt"))
    import inspect
    sig = inspect.signature(G.generate_video).parameters
    for name in ("gemma_hidden_states", "gemma_attention_mask", "negative_gemma_hidden_states", "negative_gemma_attention_mask",
                 "text_connector"):
        assert name in sig and sig[name].default is None


def test_ref_text_hand_computed():
    """2 tokens, 2 layers, D = 8, one batch row whose first token is padding.  Layer 0's valid row is 0..7: sum 28, mean 3.5,
    range 7; layer 1's is all 2 except one 6: sum 20, mean 2.5, range 4."""
    hs = torch.zeros(2, 1, 2, 8, dtype=F64)
    hs[0, 0, 0] = 100.0                                   # padding: must not reach any statistic
    hs[1, 0, 0] = -100.0
    hs[0, 0, 1] = torch.arange(8, dtype=F64)
    hs[1, 0, 1] = torch.tensor([2, 2, 2, 6, 2, 2, 2, 2], dtype=F64)
    mask = torch.tensor([[0, 1]])
    out = RT.norm_and_concat(hs, mask, RT.P64)
    assert out.shape == (1, 2, 16) and not bool(out[0, 0].any())
    m0, m1 = 28 / (8 + 1e-6), 20 / (8 + 1e-6)
    for d in range(8):
        assert out[0, 1, d * 2 + 0] == pytest.approx(8 * (d - m0) / (7 + 1e-6), rel=1e-14)
        assert out[0, 1, d * 2 + 1] == pytest.approx(8 * ((6 if d == 3 else 2) - m1) / (4 + 1e-6), rel=1e-14)
    # the bf16 policy on the same case: bf16(1e-6) vanishes against 8 and against the ranges, every quotient rounds once
    ob = RT.norm_and_concat(hs, mask, RT.PBF)
    rb = lambda v: float(torch.tensor(v, dtype=F64).to(BF))
    for d in range(8):
        assert float(ob[0, 1, d * 2]) == rb(8 * rb(d - 3.5) / 7.0)
        assert float(ob[0, 1, d * 2 + 1]) == rb(8 * rb((6 if d == 3 else 2) - 2.5) / 4.0)
    # the feature extractor sees features in the checkpoint's order d*L + l
    W = torch.zeros(8, 16, dtype=F64)
    W[0, 3 * 2 + 1] = 1.0                                  # picks layer 1, d = 3
    feat = RT.linear(out, W, None, RT.P64)
    assert feat[0, 1, 0] == pytest.approx(8 * (6 - m1) / (4 + 1e-6), rel=1e-14) and float(feat[0, 0, 0]) == 0.0
    # registers: valid token to the front, registers[t % R] behind
    reg = torch.arange(16, dtype=F64).reshape(2, 8)
    x = RT.replace_padded_with_registers(feat, torch.tensor([1]), reg)
    assert torch.equal(x[0, 0], feat[0, 1]) and torch.equal(x[0, 1], reg[1])
    # split RoPE at angle pi/2 swaps the halves with a sign; exact GELU at 0 and far out
    xq = torch.zeros(1, 1, 1, 128, dtype=F64)
    xq[..., 0], xq[..., 64] = 1.0, 2.0
    o = RT.split_rope(xq, torch.zeros(1, 1, 64, dtype=F64), torch.ones(1, 1, 64, dtype=F64), RT.P64)
    assert float(o[0, 0, 0, 0]) == -2.0 and float(o[0, 0, 0, 64]) == 1.0
    g = RT.gelu_erf(torch.tensor([0.0, 1.0, -1.0, 10.0], dtype=F64), RT.P64)
    assert g[1] == pytest.approx(0.8413447460685429, rel=1e-14) and g[2] == pytest.approx(-0.15865525393145707, rel=1e-13)
    assert float(g[0]) == 0.0 and float(g[3]) == 10.0
    # unit RMSNorm
    n = RT.rms_norm(torch.tensor([[3.0, 4.0]], dtype=F64), RT.P64, eps=0.0)
    assert n[0, 0] == pytest.approx(3 / math.sqrt(12.5)) and n[0, 1] == pytest.approx(4 / math.sqrt(12.5))


def test_ref_policies_agree_to_bf16_precision():
    """The bf16 policy is the float64 one plus roundings: on a small stage they differ by a few bf16 ulps in relative L2."""
    from mlx_video_amd.text_connector import random_connector_weights
    W = random_connector_weights("cpu", D=128, L=3, layers=1, R=8, seed=3)
    from mlx_video_amd.weights import aggregate_k_from_layer_major  # noqa: F401  (W holds the checkpoint order already)
    g = torch.Generator().manual_seed(4)
    hs = torch.randn(3, 2, 16, 128, generator=g).to(BF)
    mask = torch.tensor([[0] * 6 + [1] * 10, [1] * 16])
    a, b = RT.text_stage(hs, mask, W, RT.P64), RT.text_stage(hs, mask, W, RT.PBF)
    rel = float((a - b).norm() / a.norm())
    assert a.shape == (2, 16, 128) and 1e-4 < rel < 3e-2, rel
