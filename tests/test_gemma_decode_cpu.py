"""KV-cached Gemma-3 decoding without a GPU: the cached restatement (tests/ref_gemma_decode.py) against the full-sequence one and
against transformers' Gemma3ForCausalLM with ``use_cache``; the attention step's bound against an fp32 emulation of the kernel's
sliced evaluation and against planted faults; the sampler and the prompt-enhancement host logic; the CLI flags, generate_video's
argument handling, the ABI entry and the step form of ``ops.causal_attn``."""
import ctypes
import os
import re
import warnings

import pytest
import torch

import ref_gemma as G
import ref_gemma_decode as D

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 256.0 ** -0.5
T_PRE, T_ALL = 72, 96


# ------------------------------------------------------------------------------------------------ the cached restatement
@pytest.mark.parametrize("window", [1024, 16])
def test_cached_restatement_equals_the_full_forward(window):
    """Prefill on the first 72 columns of tiny_inputs, then 24 teacher-forced steps: the f64 hidden states and logits of the
    decoded rows equal ref_gemma.forward on the whole sequence to 1e-12 (window 16: the window bites from the first step)."""
    from mlx_video_amd.gemma import random_gemma_weights
    cfg = G.tiny_config(window)
    W = random_gemma_weights("cpu", cfg, seed=3)
    ids, mask = G.tiny_inputs()
    full = G.forward(W, cfg, ids, mask, "f64")
    full_logits = full[-1] @ G.f64(W["embed_tokens.weight"]).T
    cache, pre, pre_logits = D.prefill(W, cfg, ids[:, :T_PRE], mask[:, :T_PRE], "f64", T_total=T_ALL)
    worst = max(float((a - b[:, :T_PRE]).abs().max()) for a, b in zip(pre, full))
    for t in range(T_PRE, T_ALL):
        st, lg = D.step(W, cfg, cache, ids[:, t], "f64", T_total=T_ALL)
        worst = max([worst] + [float((a - b[:, t]).abs().max()) for a, b in zip(st, full)])
        worst = max(worst, float((lg - full_logits[:, t]).abs().max()) / float(full_logits[:, t].abs().max()))
    assert cache.length == T_ALL
    print(f"window {window}: worst difference {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("window", [1024, 16])
def test_cached_restatement_equals_transformers_with_use_cache(window, monkeypatch):
    """Logits (rel-L2 <= 1e-9 on the valid rows) and 16 greedy tokens (exactly) against Gemma3ForCausalLM in float64 with the tied
    head and its own KV cache.  The restatement is handed transformers' fp32 rope tables and embedding scale, as in
    test_gemma_cpu.py, so that 1e-9 is about the network."""
    tf = pytest.importorskip("transformers")
    MG = pytest.importorskip("transformers.models.gemma3.modeling_gemma3")
    from mlx_video_amd.gemma import random_gemma_weights
    cfg = G.tiny_config(window)
    W = random_gemma_weights("cpu", cfg, seed=3)

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
        attn_implementation="sdpa", tie_word_embeddings=True, final_logit_softcapping=None)
    m = tf.Gemma3ForCausalLM(hc).double().eval()
    res = m.model.load_state_dict({k: v.double() for k, v in W.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m.tie_weights()
    assert m.lm_head.weight.data_ptr() == m.model.embed_tokens.weight.data_ptr()
    ids, mask = G.tiny_inputs()
    ids, mask = ids[:, :T_PRE], mask[:, :T_PRE]
    N = 16
    with torch.no_grad():
        tables = {}
        for glob, lt in ((True, "full_attention"), (False, "sliding_attention")):
            c, s = m.model.rotary_emb(torch.zeros(1, 1, cfg.hidden_size, dtype=torch.float64), torch.arange(T_PRE + N)[None], lt)
            tables[glob] = (c[0, :, :128].double(), s[0, :, :128].double())
        out = m(input_ids=ids, attention_mask=mask, use_cache=True)
        past, hf_logits, hf_toks = out.past_key_values, [out.logits[:, -1]], []
        am = mask
        for i in range(N):
            tok = hf_logits[-1].argmax(-1)
            hf_toks.append(tok)
            if i + 1 < N:
                am = torch.cat([am, torch.ones(2, 1, dtype=am.dtype)], 1)
                out = m(input_ids=tok[:, None], attention_mask=am, past_key_values=past, use_cache=True)
                past = out.past_key_values
                hf_logits.append(out.logits[:, -1])
    toks, logits, _ = D.greedy(W, cfg, ids, mask, N, "f64", tables=tables, embed_scale=float(m.model.embed_tokens.embed_scale))
    assert torch.equal(toks, torch.stack(hf_toks, 1))
    for i in range(N):
        e = float((logits[:, i] - hf_logits[i]).norm() / hf_logits[i].norm())
        assert e <= 1e-9, (i, e)


# ------------------------------------------------------------------------------------------------ the attention step's bound
# (B, Hq, Hkv, step, row_start, window)
CASES = [(2, 4, 2, 300, [0, 37], 0), (2, 4, 2, 300, [0, 37], 16), (2, 2, 2, 63, [0, 63], 0), (2, 4, 1, 64, [5, 64], 64),
         (1, 16, 1, 257, [0], 1024), (2, 4, 2, 0, [0, 0], 0), (2, 4, 2, 255, [3, 200], 65)]


@pytest.fixture(scope="module")
def step_cases():
    out = []
    for i, (B, Hq, Hkv, step, rs, window) in enumerate(CASES):
        cap = (step + 64) // 64 * 64
        q1, k, v, kc, vtc = D.step_inputs(B, Hq, Hkv, step, rs, cap, seed=11 + i)
        ref = D.step_attention(q1, k, v, Hq, Hkv, rs, step, window, SCALE)
        out.append((q1, k, v, kc, vtc, ref))
    return out


def _worst(out, ref):
    d, bound = G.attention_bound(out, *ref)
    return float((d / bound).max())


def test_step_bound_accepts_the_sliced_evaluation(step_cases):
    """The fp32 emulation of the kernel's evaluation sits inside ref_gemma.attention_bound in all seven cases, with no exempt
    element; a row with row_start > step is exactly zero; masked K / V positions hold +-1024 and the cache a stale value at
    position ``step``."""
    worst = 0.0
    for (B, Hq, Hkv, step, rs, window), (q1, k, v, kc, vtc, ref) in zip(CASES, step_cases):
        emu = D.attention_step_sliced_fp32(q1, k[:, step], v[:, step], kc, vtc, Hq, Hkv, step, rs, window, SCALE)
        w = _worst(emu, ref)
        print(f"{(B, Hq, Hkv, step, rs, window)}: worst d / bound = {w:.3f}")
        worst = max(worst, w)
        assert w <= 1.0
        pol = D.step_attention(q1, k, v, Hq, Hkv, rs, step, window, SCALE, bf16_p=True)[0].to(BF)
        assert _worst(pol, ref) <= 1.0
        for b in range(B):
            if rs[b] > step:
                assert bool((emu[b] == 0).all())
    assert worst > 0.05          # the bound is not loose by orders of magnitude


@pytest.mark.parametrize("fault", D.STEP_FAULTS)
def test_step_bound_rejects(fault, step_cases):
    """Each planted fault moves some element past its bound in every case where it alters what is computed."""
    hit = 0
    for (B, Hq, Hkv, step, rs, window), (q1, k, v, kc, vtc, ref) in zip(CASES, step_cases):
        if not D.fault_alters(fault, Hq, Hkv, step, rs, window):
            continue
        hit += 1
        bad = D.attention_step_sliced_fp32(q1, k[:, step], v[:, step], kc, vtc, Hq, Hkv, step, rs, window, SCALE, fault=fault)
        w = _worst(bad, ref)
        print(f"{fault} {(B, Hq, Hkv, step, rs, window)}: worst d / bound = {w:.3e}")
        assert w > 1.0, (fault, (B, Hq, Hkv, step, rs, window), w)
    assert hit >= 1


# ------------------------------------------------------------------------------------------------ sampler and host logic
def test_repetition_penalty_is_transformers_rule():
    tf = pytest.importorskip("transformers")
    from mlx_video_amd.gemma import apply_repetition_penalty
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(2, 50, generator=g) * 3
    ctx = [[3, 7, 7, 11, 49], [0, 1, 2]]
    got = apply_repetition_penalty(logits, ctx, 1.3)
    proc = tf.RepetitionPenaltyLogitsProcessor(1.3)
    for b in range(2):
        want = proc(torch.tensor([ctx[b]]), logits[b:b + 1].clone())
        assert torch.equal(got[b:b + 1], want)
    assert bool((logits[0, [3, 7, 11, 49]] != got[0, [3, 7, 11, 49]]).all()) and torch.equal(got[0, 12:49], logits[0, 12:49])
    assert torch.equal(apply_repetition_penalty(logits, [[], []], 1.3), logits)


class _Canned:
    """A GemmaGenerator whose model is a table: the logits after n fed tokens are ``table[n]`` (B,V)."""

    def __new__(cls, table):
        from mlx_video_amd.gemma import GemmaGenerator

        class Fake(GemmaGenerator):
            def __init__(self, table):
                self.table, self.fed = table, []

            def prefill(self, input_ids, attention_mask, capacity, return_states=False):
                self.capacity, self.n = capacity, 0
                return object(), self.table[0]

            def step(self, cache, token_ids, return_states=False):
                self.n += 1
                self.fed.append([int(t) for t in token_ids])
                return self.table[self.n]

        return Fake(table)


def _table(n, B=1, V=32, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, V, generator=g) * 2 for _ in range(n)]


def test_generate_temperature_zero_is_argmax_and_seed_repeats():
    tab = _table(8)
    ids, mask = torch.tensor([[0, 0, 5, 6]]), torch.tensor([[0, 0, 1, 1]])
    gen = _Canned(tab)
    out = gen.generate(ids, mask, max_tokens=6, temperature=0.0, repetition_penalty=1.0, eos_ids=())
    assert out == [[int(t[0].argmax()) for t in tab[:6]]]
    assert gen.capacity == 64 and gen.fed == [[t] for t in out[0][:5]]          # the last token is not fed
    a = _Canned(tab).generate(ids, mask, max_tokens=6, temperature=0.7, eos_ids=(), seed=42)
    b = _Canned(tab).generate(ids, mask, max_tokens=6, temperature=0.7, eos_ids=(), seed=42)
    c = [_Canned(tab).generate(ids, mask, max_tokens=6, temperature=5.0, eos_ids=(), seed=s) for s in range(4)]
    assert a == b and len(a[0]) == 6 and len({tuple(x[0]) for x in c}) > 1
    # the penalty sees the prompt's valid tokens: with a huge penalty a prompt token that would win is never chosen
    tab2 = [torch.full((1, 32), -1.0) for _ in range(3)]
    for t in tab2:
        t[0, 5], t[0, 9] = 4.0, 3.0
    assert _Canned(tab2).generate(ids, mask, max_tokens=1, temperature=0.0, repetition_penalty=100.0, eos_ids=())[0] == [9]
    assert _Canned(tab2).generate(ids, mask, max_tokens=1, temperature=0.0, repetition_penalty=1.0, eos_ids=())[0] == [5]
    # pad ids are no context: id 0 sits under the mask only
    tab3 = [torch.full((1, 32), -1.0)]
    tab3[0][0, 0] = 4.0
    assert _Canned(tab3).generate(ids, mask, max_tokens=1, temperature=0.0, repetition_penalty=100.0, eos_ids=())[0] == [0]


def test_generate_stops_at_eos():
    tab = _table(8, B=2, seed=3)
    ids, mask = torch.tensor([[1, 2], [0, 3]]), torch.tensor([[1, 1], [0, 1]])
    free = _Canned(tab).generate(ids, mask, max_tokens=6, temperature=0.0, repetition_penalty=1.0, eos_ids=())
    third = free[0][2]
    out = _Canned(tab).generate(ids, mask, max_tokens=6, temperature=0.0, repetition_penalty=1.0, eos_ids=(third,))
    n0 = free[0].index(third) + 1
    assert 2 <= n0 <= 3 and out[0] == free[0][:n0]                # the EOS id is kept, nothing after it
    n1 = free[1].index(third) + 1 if third in free[1] else 6
    assert out[1] == free[1][:n1]


def test_chat_layout_cleaning_and_fallback():
    from mlx_video_amd import gemma as GM
    assert GM.chat_prompt("SYS", "a cat") == ("<start_of_turn>user\nSYS<end_of_turn>\n<start_of_turn>user\nuser prompt: a cat<end_of_turn>\n"
                                              "<start_of_turn>model\n")
    assert GM.clean_response('  "...A cat. ') == "A cat."
    assert GM.clean_response("\n  two words\n") == "two words" and GM.clean_response(" ?! ") == ""
    assert len(GM.DEFAULT_ENHANCE_SYSTEM_PROMPT) > 100

    class Tok:
        def __init__(self, text):
            self.text, self.seen = text, None

        def no_padding(self):
            pass

        def no_truncation(self):
            pass

        def encode(self, text):
            self.seen = text
            return type("E", (), {"ids": [2, 4, 5]})()

        def decode(self, ids, skip_special_tokens=False):
            assert skip_special_tokens
            self.decoded = list(ids)
            return self.text

    tab = _table(4)
    want = [int(t[0].argmax()) for t in tab[:3]]
    tok = Tok(' "A long prompt. ')
    got = GM.enhance_prompt(_Canned(tab), tok, "a cat", "SYS", max_tokens=3, temperature=0.0, repetition_penalty=1.0, eos_ids=())
    assert got == "A long prompt." and tok.seen == GM.chat_prompt("SYS", "a cat") and tok.decoded == want     # the new tokens only
    t = Tok("y")
    GM.enhance_prompt(_Canned(tab), t, "x", max_tokens=1)
    assert t.seen == GM.chat_prompt(GM.DEFAULT_ENHANCE_SYSTEM_PROMPT, "x")          # no system prompt given: the package's own
    with pytest.warns(UserWarning, match="empty"):
        assert GM.enhance_prompt(_Canned(tab), Tok("  ... "), "a cat", "SYS", max_tokens=2, temperature=0.0) == "a cat"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        GM.enhance_prompt(_Canned(tab), Tok("fine"), "a cat", "SYS", max_tokens=2, temperature=0.0)


def test_config_reads_final_logit_softcapping():
    from mlx_video_amd.gemma import GemmaConfig, GemmaGenerator
    assert GemmaConfig().final_logit_softcapping is None and GemmaConfig.from_dict({}).final_logit_softcapping is None
    cfg = GemmaConfig.from_dict({"text_config": {"final_logit_softcapping": 30.0}})
    assert cfg.final_logit_softcapping == 30.0
    enc = type("E", (), {"cfg": cfg, "vocab": 64})()
    with pytest.raises(ValueError, match="final_logit_softcapping"):
        GemmaGenerator(enc)


# ------------------------------------------------------------------------------------------------ surface
def test_cli_flags_parse_with_the_reference_defaults(tmp_path):
    from mlx_video_amd.generate import build_parser
    a = build_parser().parse_args([])
    assert a.enhance_prompt is False and a.max_tokens == 512 and a.temperature == 0.7 and a.enhance_system_prompt is None
    a = build_parser().parse_args(["--enhance-prompt", "--max-tokens", "8", "--temperature", "0", "--enhance-system-prompt", "f.txt"])
    assert a.enhance_prompt is True and a.max_tokens == 8 and a.temperature == 0.0 and a.enhance_system_prompt == "f.txt"


def test_generate_video_enhance_needs_gemma_and_tokenizer(tmp_path):
    from mlx_video_amd.generate import generate_video
    with pytest.raises(ValueError, match=r"enhance_prompt .*needs a Gemma-3 model.* and a tokenizer"):
        generate_video(prompt="a cat", enhance_prompt=True)
    with pytest.raises(ValueError, match=r"enhance_prompt .*needs a tokenizer"):
        generate_video(prompt="a cat", enhance_prompt=True, gemma=object())
    with pytest.raises(ValueError, match=r"enhance_prompt .*needs a Gemma-3 model: gemma=.*gemma_repo=") as e:
        generate_video(prompt="a cat", enhance_prompt=True, tokenizer_path=str(tmp_path))
    assert "tokenizer" not in str(e.value).split("needs", 1)[1].replace("GemmaEncoder", "")
    with pytest.raises(ValueError, match="enhance_prompt .*prompt_tokens"):
        generate_video(prompt="a cat", enhance_prompt=True, gemma=object(), tokenizer_path=str(tmp_path), prompt_tokens=([1], [1]))


C2CTYPE = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "float*": ctypes.c_void_p,
           "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def test_abi_entry_header_binding_and_library_agree():
    from mlx_video_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ltxk.h")).read()
    assert int(re.search(r"#define LTXK_VERSION (\d+)", hdr).group(1)) >= 411
    proto = re.search(r"\bint ltxk_causal_attn_step\((.*?)\);", hdr, re.S).group(1)
    params = [re.match(r"(.*?)\s*(\w+)$", p.strip()).groups() for p in proto.split(",")]
    names = [n for _, n in params]
    assert names == ["q", "ldq", "k_new", "ldkn", "v_new", "ldvn", "k_cache", "ldk", "vt_cache", "ldvt", "out", "ldo", "row_start", "B", "Hq",
                     "Hkv", "cap", "step", "window", "scale", "partials", "partials_floats", "stream"]
    res, args = _lib.SIGNATURES["ltxk_causal_attn_step"]
    assert res is ctypes.c_int32 and [C2CTYPE[t] for t, _ in params] == list(args)
    assert not [n for n in _lib.SIGNATURES if n.startswith("ltxk_causal_attn_step") and n != "ltxk_causal_attn_step"]      # no sizeof entry
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.ltxk_version() >= 411 and hasattr(lib, "ltxk_causal_attn_step")


def _step_call(**over):
    """A well-formed step-form call on CPU tensors (B = 2, Hq = 4, Hkv = 2, cap = 64): only the device refuses it."""
    z = lambda *s, dtype=BF: torch.zeros(s, dtype=dtype)          # noqa: E731
    B, Hq, Hkv, cap = 2, 4, 2, 64
    qkv = z(B, (Hq + 2 * Hkv) * 256)
    a = dict(q=qkv[:, :1024], k=z(B * cap, 512), vt=z(B, 512, cap), out=z(B, 1024), row_start=z(B, dtype=torch.int32), B=B, Hq=Hq, Hkv=Hkv,
             T=cap, scale=0.0625, window=0, step=5, k_new=qkv[:, 1024:1536], v_new=qkv[:, 1536:], partials=z(B * Hq * 258, dtype=torch.float32))
    a.update(over)
    pos = [a.pop(n) for n in ("q", "k", "vt", "out", "row_start", "B", "Hq", "Hkv", "T", "scale")]
    return pos, a


def test_step_form_refuses_bad_calls_before_any_launch():
    from mlx_video_amd import ops
    from mlx_video_amd._lib import LtxkError
    z = lambda *s, dtype=BF: torch.zeros(s, dtype=dtype)          # noqa: E731

    def call(**over):
        pos, kw = _step_call(**over)
        return ops.causal_attn(*pos, **kw)

    with pytest.raises(LtxkError, match="causal_attn: .* device tensor.*no CPU fallback"):
        call()
    off = lambda *s, dtype=BF: torch.zeros(s[0] * s[1] + 1, dtype=dtype)[1:].view(s)          # noqa: E731
    for name, shape in (("q", (2, 1024)), ("out", (2, 1024)), ("k_new", (2, 512)), ("v_new", (2, 512)), ("k", (128, 512))):
        with pytest.raises(TypeError, match=f"causal_attn: {name} "):
            call(**{name: z(*shape, dtype=torch.float32)})
        with pytest.raises(ValueError, match=f"causal_attn: {name} "):
            call(**{name: z(shape[0] + 1, shape[1])})                                       # a bad shape
        with pytest.raises(ValueError, match=f"causal_attn: {name} .*stride"):
            call(**{name: z(shape[0], 2 * shape[1])[:, ::2]})                               # strided
        with pytest.raises(ValueError, match=f"causal_attn: {name} .*aligned"):
            call(**{name: off(*shape)})                                                     # misaligned
    with pytest.raises(ValueError, match="causal_attn: q "):
        call(q=z(2, 1016))                                                                  # fewer columns than Hq * 256
    with pytest.raises(TypeError, match="causal_attn: partials "):
        call(partials=z(2 * 4 * 258))
    with pytest.raises(ValueError, match="causal_attn: partials "):
        call(partials=z(2 * 4 * 258 - 1, dtype=torch.float32))
    with pytest.raises(ValueError, match="causal_attn: partials .*aligned"):
        call(partials=torch.zeros(2 * 4 * 258 + 1, dtype=torch.float32)[1:])
    with pytest.raises(ValueError, match="causal_attn: partials "):
        call(step=300, T=320, k=z(2 * 320, 512), vt=z(2, 512, 320))                          # two slices need twice the floats
    with pytest.raises(TypeError, match="causal_attn: row_start "):
        call(row_start=z(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="causal_attn: vt "):
        call(vt=z(2, 512, 56))                                                              # fewer columns than the capacity
    for missing in ("k_new", "v_new", "partials"):
        with pytest.raises(ValueError, match=f"causal_attn: the step form needs {missing}"):
            call(**{missing: None})
    with pytest.raises(ValueError, match="causal_attn: step = 64 must lie in"):
        call(step=64)
    with pytest.raises(ValueError, match="causal_attn: step = -1 must lie in"):
        call(step=-1)
    with pytest.raises(ValueError, match="causal_attn: the cache capacity T = 72"):
        call(T=72, k=z(2 * 72, 512), vt=z(2, 512, 72))
    with pytest.raises(ValueError, match="causal_attn: .*at most 16 times"):
        call(Hq=17, Hkv=1, q=z(2, 17 * 256), out=z(2, 17 * 256), k=z(128, 256), vt=z(2, 256, 64), k_new=z(2, 256), v_new=z(2, 256),
             partials=z(2 * 17 * 258, dtype=torch.float32))
    with pytest.raises(ValueError, match="causal_attn: k_new, v_new and partials belong to the step form"):
        call(step=None)
    # a window shortens what a step needs: slices below the window are not launched
    pos, kw = _step_call(step=300, T=320, window=16, k=z(2 * 320, 512), vt=z(2, 512, 320))
    with pytest.raises(LtxkError, match="device tensor"):
        ops.causal_attn(*pos, **kw)
