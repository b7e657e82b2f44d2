"""The Gemma-3 text encoder without a GPU: the float64 restatement (tests/ref_gemma.py) against transformers' Gemma3TextModel,
the attention bound's power to discriminate, and the host logic (ABI, config parsing, checkpoint loading, tokenizer,
generate_video's argument handling)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import ref_gemma as G

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------- against transformers
def _hf_model(cfg, W, monkeypatch):
    """transformers' Gemma3TextModel in float64 with the weights W.  Its RMSNorm hard-codes fp32 (`x.float()`), which would
    cap a float64 run at 1e-7; the class's forward is replaced by the same formula without the cast.  Nothing else is touched:
    masks, layer types, rope, GQA, the MLP and the layer structure are the package's own (attention through torch's SDPA,
    float64 on the CPU - the eager path casts its softmax to fp32)."""
    tf = pytest.importorskip("transformers")
    MG = pytest.importorskip("transformers.models.gemma3.modeling_gemma3")

    def norm64(self, x):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * (1.0 + self.weight)

    monkeypatch.setattr(MG.Gemma3RMSNorm, "forward", norm64)
    hc = tf.Gemma3TextConfig(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
        num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
        num_key_value_heads=cfg.num_key_value_heads, head_dim=cfg.head_dim, sliding_window=cfg.sliding_window,
        query_pre_attn_scalar=int(cfg.query_pre_attn_scalar), rms_norm_eps=cfg.rms_norm_eps, max_position_embeddings=2048, pad_token_id=0,
        rope_parameters={"full_attention": {"rope_type": "linear", "factor": cfg.rope_scaling_factor, "rope_theta": cfg.rope_theta},
                         "sliding_attention": {"rope_type": "default", "rope_theta": cfg.rope_local_base_freq}},
        attn_implementation="sdpa")
    assert list(hc.layer_types) == ["sliding_attention"] * 5 + ["full_attention"] and hc.sliding_window == cfg.sliding_window
    m = tf.Gemma3TextModel(hc).double().eval()
    res = m.load_state_dict({k: v.double() for k, v in W.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m


@pytest.mark.parametrize("window", [1024, 16])
def test_float64_restatement_equals_transformers(window, monkeypatch):
    """ref_gemma.forward (policy f64) against Gemma3TextModel in float64: hidden 512, intermediate 1024, 6 layers (5 local +
    1 global), 4 heads, 2 KV heads, head dim 256, vocab 512; B = 2, T = 96, the second row left-padded by 59; default
    positions.  rel-L2 <= 1e-9 per hidden state on the valid rows, the L + 1 states in the reference's order with the last one
    normed.  With sliding_window 16 the window rule bites (T = 96 > 16); with 1024 every layer is full causal.
    transformers forms its cos / sin tables and its embedding scale in fp32 whatever the model's dtype; the restatement is
    handed exactly those (its own float64 tables are held to them at fp32 accuracy below), so that 1e-9 is about the network."""
    from mlx_video_amd.gemma import random_gemma_weights
    cfg = G.tiny_config(window)
    W = random_gemma_weights("cpu", cfg, seed=3)
    m = _hf_model(cfg, W, monkeypatch)
    ids, mask = G.tiny_inputs()
    T = ids.shape[1]
    with torch.no_grad():
        out = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        hs = list(out.hidden_states)
        tables = {}
        for glob, lt in ((True, "full_attention"), (False, "sliding_attention")):
            c, s = m.rotary_emb(hs[0], torch.arange(T)[None], lt)
            assert torch.equal(c[0, :, :128], c[0, :, 128:])                      # the rotate-half layout: both halves share a table
            tables[glob] = (c[0, :, :128].double(), s[0, :, :128].double())
            c64, s64 = G.rope_tables(T, cfg.rope_theta if glob else cfg.rope_local_base_freq, cfg.rope_scaling_factor if glob else 1.0)
            # fp32 angle (|angle| <= T) and fp32 cos: T * 2^-23 covers both
            assert float((c64 - tables[glob][0]).abs().max()) <= T * 2.0 ** -23 and float((s64 - tables[glob][1]).abs().max()) <= T * 2.0 ** -23
    L = cfg.num_hidden_layers
    assert len(hs) == L + 1
    ref = hs                    # transformers' list is the reference's: [embeddings, h_1 .. h_{L-1}, norm(h_L)] - its last entry is
    assert torch.equal(hs[L], out.last_hidden_state)          # the final norm's output, not h_L
    got = G.forward(W, cfg, ids, mask, "f64", tables=tables, embed_scale=float(m.embed_tokens.embed_scale))
    assert len(got) == L + 1
    for l, (a, b) in enumerate(zip(got, ref)):
        e = G.rel_l2_valid(a, b, mask)
        print(f"window {window} state {l}: rel-L2 {e:.3e}")
        assert e <= 1e-9, (window, l, e)
    # and the two windows differ where the window bites
    if window == 16:
        full = G.forward(W, G.tiny_config(1024), ids, mask, "f64", tables=tables, embed_scale=float(m.embed_tokens.embed_scale))
        assert G.rel_l2_valid(got[1], full[1], mask) > 1e-3


def test_bf16_policy_error_and_padded_rows():
    """The bf16 policy against float64: 1.7e-3 at the embeddings rising to ~1.3e-2 at the last state (what transformers' own
    bf16 forward shows on this model), and padded rows stay finite."""
    from mlx_video_amd.gemma import random_gemma_weights
    cfg = G.tiny_config(16)
    W = random_gemma_weights("cpu", cfg, seed=3)
    ids, mask = G.tiny_inputs()
    a, b = G.forward(W, cfg, ids, mask, "bf16"), G.forward(W, cfg, ids, mask, "f64", embed_scale=float(torch.tensor(512 ** 0.5, dtype=BF)))
    errs = [G.rel_l2_valid(x, y, mask) for x, y in zip(a, b)]
    assert 5e-4 < errs[0] < 4e-3 and 2e-3 < errs[-1] < 4e-2, errs
    assert all(bool(torch.isfinite(x).all()) for x in a)


# --------------------------------------------------------------------------------------------- the attention bound
B_, HQ, HKV, T_ = 2, 4, 2, 70
RS = [0, 37]
WIN = 3
SCALE = 256.0 ** -0.5


@pytest.fixture(scope="module")
def attn_case():
    q, k, v, vt = G.attention_inputs(B_, HQ, HKV, T_, RS, seed=7)
    y, A, dx, nvis = G.causal_attention(q, k, v, HQ, HKV, RS, WIN, SCALE)
    return q, k, v, vt, (y, A, dx, nvis)


def _worst(out, ref):
    d, bound = G.attention_bound(out, *ref)
    return float((d / bound).max())


def test_attention_bound_accepts_correct_evaluations(attn_case):
    """The bf16 ("flash") policy evaluation and an fp32 emulation of a tiled online-softmax loop sit inside the bound, with no
    exempt element; masked K / V rows and the V^T pad columns hold +-1024."""
    q, k, v, vt, ref = attn_case
    assert float(k[1, :RS[1]].abs().min()) == 1024.0 and float(vt[:, :, T_:].abs().min()) == 1024.0
    pol = G.causal_attention(q, k, v, HQ, HKV, RS, WIN, SCALE, bf16_p=True)[0].to(BF)
    assert _worst(pol, ref) <= 1.0
    emu = G.attention_tiled_fp32(q, k, vt, HQ, HKV, T_, RS, WIN, SCALE)
    assert _worst(emu, ref) <= 1.0
    assert bool((emu[1, :RS[1]] == 0).all()) and bool((pol[1, :RS[1]] == 0).all())
    for window in (0, 64, 65):                              # and without a window / across the tile size
        r = G.causal_attention(q, k, v, HQ, HKV, RS, window, SCALE)
        assert _worst(G.attention_tiled_fp32(q, k, vt, HQ, HKV, T_, RS, window, SCALE), r) <= 1.0


@pytest.mark.parametrize("fault", G.FAULTS)
def test_attention_bound_rejects(fault, attn_case):
    """Each planted fault moves some element past its bound: a dropped visible key, one admitted key at row_start - 1, one at
    i + 1, a window off by one in either direction, K/V heads mapped h % Hkv, an unmasked V^T pad column."""
    q, k, v, vt, ref = attn_case
    bad = G.attention_tiled_fp32(q, k, vt, HQ, HKV, T_, RS, WIN, SCALE, fault=fault)
    w = _worst(bad, ref)
    print(f"{fault}: worst d / bound = {w:.3e}")
    assert w > 1.0, (fault, w)


# --------------------------------------------------------------------------------------------- ABI
NEW = ("ltxk_embed_rows", "ltxk_rmsnorm_weight_rows", "ltxk_headnorm_rope", "ltxk_geglu_tanh", "ltxk_causal_attn",
       "ltxk_causal_attn_args_sizeof")


def test_abi_entries_and_struct():
    from mlx_video_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ltxk.h")).read()
    assert int(re.search(r"#define LTXK_VERSION (\d+)", hdr).group(1)) >= 410
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    # the struct, field by field: names, order and C types against the ctypes binding
    body = re.search(r"typedef struct ltxk_causal_attn_args \{(.*?)\} ltxk_causal_attn_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const void\*|void\*|const int32_t\*|int32_t|float)\s+(.*)", decl)
        assert m, decl
        for nm in m.group(2).split(","):
            fields.append((nm.strip(), m.group(1)))
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int32_t": ctypes.c_int32,
             "float": ctypes.c_float}
    assert [(n, ctype[t]) for n, t in fields] == list(_lib.CausalAttnArgs._fields_)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.ltxk_version() >= 410
        assert lib.ltxk_causal_attn_args_sizeof() == ctypes.sizeof(_lib.CausalAttnArgs)
        for name in NEW:
            assert hasattr(lib, name)
        assert lib.ltxk_abi_sizeof(5) == -1                  # the index list stays closed


def test_ops_wrappers_validate_on_the_host():
    """The argument checks that need no device: dtype / layout errors are raised before any library call."""
    from mlx_video_amd import ops
    from mlx_video_amd._lib import LtxkError
    for name in ("embed_rows", "rmsnorm_weight_rows", "headnorm_rope", "geglu_tanh_", "causal_attn"):
        assert callable(getattr(ops, name))
    with pytest.raises(LtxkError):
        ops.rmsnorm_weight_rows(torch.zeros(2, 8, dtype=BF), torch.zeros(8, dtype=BF))
    with pytest.raises(LtxkError):
        ops.embed_rows(torch.zeros(4, 8, dtype=BF), torch.zeros(2, dtype=torch.int32), 1.0)


# --------------------------------------------------------------------------------------------- config
BASE_CFG = dict(hidden_size=3840, num_hidden_layers=48, num_attention_heads=16, num_key_value_heads=8, head_dim=256,
                intermediate_size=15360, sliding_window=1024, query_pre_attn_scalar=256, rms_norm_eps=1e-6, vocab_size=262208)


def test_config_both_rope_spellings_and_rejections(tmp_path):
    from mlx_video_amd.gemma import GemmaConfig
    old = dict(BASE_CFG, rope_theta=1000000.0, rope_local_base_freq=10000.0, rope_scaling={"factor": 8.0, "rope_type": "linear"},
               sliding_window_pattern=6)
    new = dict(BASE_CFG, layer_types=(["sliding_attention"] * 5 + ["full_attention"]) * 8,
               rope_parameters={"full_attention": {"rope_type": "linear", "factor": 8.0, "rope_theta": 1000000.0},
                                "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}})
    a = GemmaConfig.from_dict({"text_config": old, "vision_config": {}})           # nested, as Gemma-3 multimodal repos have it
    b = GemmaConfig.from_dict(new)                                                  # top level, as text-only repos have it
    for c in (a, b):
        assert (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim) == (3840, 48, 16, 8, 256)
        assert (c.intermediate_size, c.sliding_window, c.query_pre_attn_scalar, c.rms_norm_eps) == (15360, 1024, 256.0, 1e-6)
        assert (c.rope_theta, c.rope_local_base_freq, c.rope_scaling_factor) == (1e6, 1e4, 8.0)
        assert [c.is_global(i) for i in range(12)] == [False] * 5 + [True] + [False] * 5 + [True]
    (tmp_path / "config.json").write_text(json.dumps({"text_config": old}))
    assert GemmaConfig.from_json(tmp_path) == a
    # other spellings of the same values must not leak defaults
    c = GemmaConfig.from_dict(dict(BASE_CFG, rope_theta=5e5, rope_local_base_freq=2e4, sliding_window_pattern=4, num_hidden_layers=8))
    assert (c.rope_theta, c.rope_local_base_freq, c.rope_scaling_factor) == (5e5, 2e4, 1.0)
    assert [c.is_global(i) for i in range(8)] == [False, False, False, True] * 2
    with pytest.raises(ValueError, match="head_dim"):
        GemmaConfig.from_dict(dict(BASE_CFG, head_dim=128))
    with pytest.raises(ValueError, match="soft-capping"):
        GemmaConfig.from_dict(dict(BASE_CFG, attn_logit_softcapping=50.0))
    with pytest.raises(ValueError, match="rope scaling"):
        GemmaConfig.from_dict(dict(BASE_CFG, rope_scaling={"rope_type": "yarn", "factor": 8.0}))
    with pytest.raises(ValueError, match="layer_types"):
        GemmaConfig.from_dict(dict(BASE_CFG, layer_types=["full_attention"]))
    assert GemmaConfig.from_dict(dict(BASE_CFG, final_logit_softcapping=30.0)).hidden_size == 3840      # logits are not computed here


def test_rope_tables_convention():
    from mlx_video_amd.gemma import rope_table_half
    c, s = rope_table_half(130, 1e6, 8.0)
    c64, s64 = G.rope_tables(130, 1e6, 8.0, round_bf16=True)
    assert c.dtype == torch.float32 and tuple(c.shape) == (130, 128)
    assert torch.equal(c.double(), c64) and torch.equal(s.double(), s64)
    assert torch.equal(c, c.to(BF).float())                   # bf16 values, widened
    assert float(c[0].min()) == 1.0 and float(s[0].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- loading
def _tensors(prefix, extra=()):
    g = torch.Generator().manual_seed(1)
    d = {prefix + "embed_tokens.weight": torch.randn(8, 16, generator=g),                     # fp32: must come back bf16
         prefix + "layers.0.self_attn.q_proj.weight": torch.randn(4, 16, generator=g).to(BF),
         prefix + "norm.weight": torch.randn(16, generator=g).to(BF)}
    for k in extra:
        d[k] = torch.zeros(4, dtype=BF)
    return d


@pytest.mark.parametrize("prefix", ["language_model.", "model.language_model.", "language_model.model.", "model.", ""])
def test_gemma_weights_key_prefixes(prefix, tmp_path):
    from safetensors.torch import save_file
    from mlx_video_amd.weights import gemma_weights
    d = _tensors(prefix, extra=("vision_tower.vision_model.x.weight", "model.vision_tower.y.weight", "multi_modal_projector.w", "lm_head.weight"))
    save_file(d, str(tmp_path / "model.safetensors"))
    W = gemma_weights(tmp_path, "cpu")
    assert sorted(W) == ["embed_tokens.weight", "layers.0.self_attn.q_proj.weight", "norm.weight"]
    assert all(v.dtype == BF for v in W.values())
    assert torch.equal(W["embed_tokens.weight"], d[prefix + "embed_tokens.weight"].to(BF))


def test_gemma_weights_shard_preference_and_rejections(tmp_path):
    from safetensors.torch import save_file
    from mlx_video_amd.weights import gemma_shard_files, gemma_weights
    a, b = _tensors("language_model."), _tensors("language_model.")
    b["language_model.norm.weight"] = b["language_model.norm.weight"] + 1
    # two complete shard sets: the indexed diffusion_pytorch_model-* set wins over model-*, which wins over stray files
    save_file(a, str(tmp_path / "diffusion_pytorch_model-00001-of-00001.safetensors"))
    save_file(b, str(tmp_path / "model-00001-of-00001.safetensors"))
    (tmp_path / "model.safetensors.index.json").write_text("{}")
    assert [f.name for f in gemma_shard_files(tmp_path)] == ["model-00001-of-00001.safetensors"]
    assert torch.equal(gemma_weights(tmp_path, "cpu")["norm.weight"], b["language_model.norm.weight"])
    (tmp_path / "diffusion_pytorch_model.safetensors.index.json").write_text("{}")
    assert [f.name for f in gemma_shard_files(tmp_path)] == ["diffusion_pytorch_model-00001-of-00001.safetensors"]
    assert torch.equal(gemma_weights(tmp_path, "cpu")["norm.weight"], a["language_model.norm.weight"])
    # single files, then anything
    one = tmp_path / "one"
    one.mkdir()
    save_file(a, str(one / "model.safetensors"))
    save_file(b, str(one / "other.safetensors"))
    assert [f.name for f in gemma_shard_files(one)] == ["model.safetensors"]
    save_file(a, str(one / "diffusion_pytorch_model.safetensors"))
    assert [f.name for f in gemma_shard_files(one)] == ["diffusion_pytorch_model.safetensors"]
    # a pre-quantised checkpoint, a directory without tensors, a repo name
    q = tmp_path / "quant"
    q.mkdir()
    save_file(dict(a, **{"language_model.layers.0.self_attn.q_proj.scales": torch.zeros(4, dtype=BF)}), str(q / "model.safetensors"))
    with pytest.raises(ValueError, match="pre-quantised"):
        gemma_weights(q, "cpu")
    e = tmp_path / "empty"
    e.mkdir()
    with pytest.raises(FileNotFoundError):
        gemma_weights(e, "cpu")
    with pytest.raises(FileNotFoundError, match="not a local directory"):
        gemma_weights("google/gemma-3-12b-it", "cpu")


# --------------------------------------------------------------------------------------------- tokenizer
def _write_tokenizer(path):
    tk = pytest.importorskip("tokenizers")
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.processors import TemplateProcessing
    vocab = {"<pad>": 0, "<eos>": 1, "<bos>": 2, "<unk>": 3, "a": 4, "b": 5, "c": 6}
    tok = tk.Tokenizer(WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = Whitespace()
    tok.post_processor = TemplateProcessing(single="<bos> $A", special_tokens=[("<bos>", 2)])
    tok.enable_padding(pad_id=0, pad_token="<pad>", length=12)        # a tokenizer.json with its own (right) padding: must be ignored
    tok.save(str(path / "tokenizer.json"))


def test_tokenizer_left_padding_and_truncation(tmp_path):
    from mlx_video_amd.gemma import load_tokenizer, tokenize
    _write_tokenizer(tmp_path)
    tok = load_tokenizer(tmp_path)
    ids, mask = tokenize(tok, ["a b c", "c " * 20, ""], max_length=8)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (3, 8)
    assert ids[0].tolist() == [0, 0, 0, 0, 2, 4, 5, 6] and mask[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert ids[1].tolist() == [2] + [6] * 7 and mask[1].tolist() == [1] * 8                    # truncated to max_length, no padding
    assert ids[2].tolist() == [0] * 7 + [2] and mask[2].tolist() == [0] * 7 + [1]
    assert tuple(tokenize(tok, ["a"])[0].shape) == (1, 1024)                                   # the reference's max_length
    from mlx_video_amd.text_connector import mask_row_counts
    assert mask_row_counts(mask) == [4, 8, 1]
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        load_tokenizer(tmp_path / "nowhere")


# --------------------------------------------------------------------------------------------- generate_video
class _Stop(Exception):
    pass


def test_generate_video_argument_precedence_and_errors(monkeypatch, tmp_path):
    """Which text route generate_video takes, without a device: the route functions are replaced by recorders and the call is
    cut short right behind the text stage."""
    from mlx_video_amd import generate as GV
    calls = []

    class FakeTransformer:
        class tables:
            device = torch.device("cpu")

    def fake_encode(gemma, gemma_repo, tokenizer_path, prompt, negative_prompt, pt, npt, dev):
        calls.append(("gemma", gemma, gemma_repo, tokenizer_path, pt is not None, npt is not None))
        return torch.zeros(3, 2, 4, 8), torch.ones(2, 4, dtype=torch.int64)

    def fake_connect(hs, mask, nhs, nmask, text_connector, model_repo, dev):
        calls.append(("connect", tuple(hs.shape), tuple(nhs.shape) if nhs is not None else None))
        raise _Stop

    monkeypatch.setattr(GV, "_encode_gemma", fake_encode)
    monkeypatch.setattr(GV, "_connect_gemma", fake_connect)
    base = dict(transformer=FakeTransformer(), vae_decoder=object(), device=torch.device("cpu"), noise_fn=lambda s: None)

    def run(**kw):
        calls.clear()
        try:
            GV.generate_video(**base, **kw)
        except _Stop:
            return list(calls)
        except Exception as e:                                # the call went past the text stage (no real modules behind it)
            return list(calls) + [("past", type(e).__name__)]
        return list(calls)

    enc = object()
    toks = (torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64))
    # the new route: one B = 2 encoder call, then the connector on the two halves
    got = run(gemma=enc, prompt_tokens=toks, negative_prompt_tokens=toks)
    assert got == [("gemma", enc, None, None, True, True), ("connect", (3, 1, 4, 8), (3, 1, 4, 8))]
    got = run(gemma_repo="dir", tokenizer_path="tok", prompt="x")
    assert got[0] == ("gemma", None, "dir", "tok", False, False)
    # prompt_embeds wins over everything; gemma_hidden_states over the encoder; a text_encoder callable over the encoder
    pe = torch.zeros(1, 4, 8)
    assert [c[0] for c in run(gemma=enc, prompt_tokens=toks, negative_prompt_tokens=toks, prompt_embeds=pe, negative_prompt_embeds=pe)] == ["past"]
    got = run(gemma=enc, prompt_tokens=toks, negative_prompt_tokens=toks, gemma_hidden_states=torch.zeros(3, 1, 4, 8),
              gemma_attention_mask=torch.ones(1, 4))
    assert got == [("connect", (3, 1, 4, 8), None)]
    seen = []
    got = run(gemma=enc, prompt_tokens=toks, negative_prompt_tokens=toks, text_encoder=lambda p: seen.append(p) or pe, prompt="p",
              negative_prompt="n")
    assert seen == ["p", "n"] and [c[0] for c in got] == ["past"]
    # nothing given: the error names the new route
    with pytest.raises(ValueError, match="gemma_repo"):
        GV.generate_video(**base)


def test_encode_gemma_errors_and_cli_flags(tmp_path):
    from mlx_video_amd import generate as GV
    enc = lambda ids, mask: (ids, mask)
    with pytest.raises(ValueError, match="without tokens"):
        GV._encode_gemma(enc, None, None, "p", "n", None, None, "cpu")
    t4 = (torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64))
    t5 = (torch.zeros(1, 5, dtype=torch.int64), torch.ones(1, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="one length"):
        GV._encode_gemma(enc, None, None, "p", "n", t4, t5, "cpu")
    with pytest.raises(ValueError, match="pair"):
        GV._encode_gemma(enc, None, None, "p", "n", torch.zeros(4), t4, "cpu")
    (ids, mask), m2 = GV._encode_gemma(enc, None, None, "p", "n", t4, t4, "cpu")
    assert tuple(ids.shape) == (2, 4) and torch.equal(mask, m2)                # positive and negative as one B = 2 call
    # with a tokenizer and no tokens, the prompts are tokenised (left-padded to 1024)
    _write_tokenizer(tmp_path)
    (ids, mask), _ = GV._encode_gemma(enc, None, str(tmp_path), "a b", "c", None, None, "cpu")
    assert tuple(ids.shape) == (2, 1024) and ids[0, -3:].tolist() == [2, 4, 5] and ids[1, -2:].tolist() == [2, 6] and int(mask.sum()) == 5
    # CLI: --text-encoder-repo is an alias of --gemma-repo; token files are .npz
    ap = GV.build_parser()
    assert ap.parse_args(["--text-encoder-repo", "d"]).gemma_repo == "d" and ap.parse_args(["--gemma-repo", "e", "--tokenizer", "t"]).tokenizer == "t"
    np.savez(tmp_path / "p.npz", input_ids=np.arange(4, dtype=np.int32), attention_mask=np.array([0, 1, 1, 1], dtype=np.int8))
    ids, mask = GV.load_prompt_tokens(str(tmp_path / "p.npz"))
    assert tuple(ids.shape) == (1, 4) and ids.dtype == torch.int64 and mask.tolist() == [[0, 1, 1, 1]]
    np.savez(tmp_path / "bad.npz", input_ids=np.arange(4))
    with pytest.raises(ValueError, match="attention_mask"):
        GV.load_prompt_tokens(str(tmp_path / "bad.npz"))
