"""KV-cached Gemma-3 decoding on the device: the attention step (csrc/causal_attn_step.hip) through ``ops.causal_attn(step=)``
against float64 inside ``ref_gemma.attention_bound`` with its cache append checked bit for bit, its invariances, the
GemmaGenerator's prefill and steps against the restatements of tests/ref_gemma_decode.py, greedy generation, and prompt
enhancement through generate_video and the CLI.

Shapes are the smallest at which the kernel can still go wrong: ``step`` one before, at and one after the 64-key tile and the
256-key slice, a second slice (300), ``row_start`` at 0, inside, at ``step`` and past it, windows that end before, at and past a
tile edge, a query group of 1, 2, 4 and 16 heads, caches of 1, 5 and 8 tiles."""
import functools

import numpy as np
import parity
import pytest
import torch

import ref_gemma as G
import ref_gemma_decode as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SCALE = 256.0 ** -0.5
NAN = float("nan")

STEPS = (0, 1, 63, 64, 255, 256, 257, 300)
WINDOWS = (0, 16, 64, 65, 1024)
HEADS = ((2, 2), (4, 2), (4, 1), (16, 1))
CAPS = (64, 320, 512)


def _kernel_cases():
    """Every step with every window; heads, capacity, batch and the row_start pair rotate through their values."""
    out = []
    for si, step in enumerate(STEPS):
        for wi, window in enumerate(WINDOWS):
            i = si * len(WINDOWS) + wi
            Hq, Hkv = HEADS[(si + wi) % 4]
            caps = [c for c in CAPS if step < c]
            cap = caps[(si + 2 * wi) % len(caps)]
            pair = ((0, 5), (step, step + 1), (5, step), (step + 1, 0))[(i + si) % 4]
            B = 1 if i % 5 == 3 else 2
            out.append((B, Hq, Hkv, step, list(pair[:B]), window, cap))
    return out


KERNEL_CASES = _kernel_cases()


def test_kernel_cases_cover_the_grid():
    for idx, want in ((1, set(h[0] for h in HEADS)), (6, set(CAPS)), (0, {1, 2})):
        assert {c[idx] for c in KERNEL_CASES} == want
    assert {(c[3], c[5]) for c in KERNEL_CASES} == {(s, w) for s in STEPS for w in WINDOWS}
    for step in STEPS:
        rs = {r for c in KERNEL_CASES if c[3] == step for r in c[4]}
        assert {0, 5, step, step + 1} <= rs, (step, rs)
    assert {(c[1], c[2]) for c in KERNEL_CASES} == set(HEADS)


def _launch(dev, q1, k_new, v_new, k_cache, vt_cache, Hq, Hkv, step, rs, window, partials=None):
    """ops.causal_attn's step form on the views the module passes: q | k_new | v_new thirds of one projection buffer.  Returns
    (out, k_cache after, vt_cache after) on the host; the caches handed in are not modified."""
    from mlx_video_amd import ops
    B, cap = k_cache.shape[0], k_cache.shape[1]
    nq, nkv = Hq * 256, Hkv * 256
    qkv = torch.cat([q1, k_new, v_new], 1).to(dev)
    kc, vtc = k_cache.to(dev), vt_cache.to(dev)
    out = torch.full((B, nq), NAN, dtype=BF, device=dev)
    if partials is None:
        partials = torch.full((B * Hq * (-(-cap // 256)) * 258,), NAN, dtype=torch.float32, device=dev)
    ops.causal_attn(qkv[:, :nq], kc.view(B * cap, nkv), vtc, out, torch.tensor(rs, dtype=torch.int32, device=dev), B, Hq, Hkv, cap, SCALE,
                    window=window, step=step, k_new=qkv[:, nq:nq + nkv], v_new=qkv[:, nq + nkv:], partials=partials)
    torch.cuda.synchronize()
    return out.cpu(), kc.cpu(), vtc.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "B{}-Hq{}-Hkv{}-step{}-rs{}-w{}-cap{}".format(c[0], c[1], c[2], c[3], "_".join(map(str, c[4])), c[5], c[6]))
def test_attention_step(dev, case):
    """Every output element inside attention_bound of the float64 answer; +-1024 below row_start, the planted key at
    row_start - 1, +-1024 past ``step`` and NaN at cache position ``step`` change nothing; rows with row_start > step are exactly
    zero; after the call K row ``step`` and V^T column ``step`` hold k_new / v_new bit for bit and the rest of the cache its bits."""
    B, Hq, Hkv, step, rs, window, cap = case
    q1, k, v, kc, vtc = D.step_inputs(B, Hq, Hkv, step, rs, cap, seed=3)
    kc[:, step], vtc[:, :, step] = NAN, NAN
    out, kc2, vtc2 = _launch(dev, q1, k[:, step], v[:, step], kc, vtc, Hq, Hkv, step, rs, window)
    ref = D.step_attention(q1, k, v, Hq, Hkv, rs, step, window, SCALE)
    d, bound = G.attention_bound(out, *ref)
    worst = float((d / bound).max())
    print(f"{case}: worst d / bound = {worst:.3f}")
    parity.auto(worst, 1.0)
    for b in range(B):
        if rs[b] > step:
            assert bool((_bits(out[b]) == 0).all()), f"row {b} (row_start {rs[b]} > step {step}) is not exactly zero"
    assert torch.equal(_bits(kc2[:, step]), _bits(k[:, step])) and torch.equal(_bits(vtc2[:, :, step]), _bits(v[:, step]))
    keep = torch.arange(cap) != step
    assert torch.equal(_bits(kc2[:, keep]), _bits(kc[:, keep])) and torch.equal(_bits(vtc2[:, :, keep]), _bits(vtc[:, :, keep]))


@pytest.mark.parametrize("window", [0, 16])
def test_attention_step_bits(dev, window):
    """The same data at capacity 320 and 512 gives equal bits; a batch row alone gives the bits it gives in a batch of two;
    swapping the rows swaps the bits; two runs are equal."""
    B, Hq, Hkv, step, rs = 2, 4, 2, 300, [0, 37]
    q1, k, v, kc, vtc = D.step_inputs(B, Hq, Hkv, step, rs, 320, seed=5)
    args = (Hq, Hkv, step)
    a, _, _ = _launch(dev, q1, k[:, step], v[:, step], kc, vtc, *args, rs, window)
    again, _, _ = _launch(dev, q1, k[:, step], v[:, step], kc, vtc, *args, rs, window)
    assert torch.equal(_bits(a), _bits(again)) and bool(torch.isfinite(a.float()).all())
    kc5 = torch.cat([kc, torch.full((B, 192, Hkv * 256), 7.0, dtype=BF)], 1)
    vtc5 = torch.cat([vtc, torch.full((B, Hkv * 256, 192), -7.0, dtype=BF)], 2)
    wide, _, _ = _launch(dev, q1, k[:, step], v[:, step], kc5, vtc5, *args, rs, window)
    assert torch.equal(_bits(a), _bits(wide)), "the capacity changes the bits"
    for b in range(B):
        one, _, _ = _launch(dev, q1[b:b + 1], k[b:b + 1, step], v[b:b + 1, step], kc[b:b + 1], vtc[b:b + 1], *args, rs[b:b + 1], window)
        assert torch.equal(_bits(one[0]), _bits(a[b])), f"row {b} alone gives other bits"
    sw, _, _ = _launch(dev, q1.flip(0), k[:, step].flip(0), v[:, step].flip(0), kc.flip(0), vtc.flip(0), *args, rs[::-1], window)
    assert torch.equal(_bits(sw.flip(0)), _bits(a))


# ------------------------------------------------------------------------------------------------------------ the model
T_PRE, T_ALL = 72, 96


def _generator(dev, cfg, seed=3):
    from mlx_video_amd.gemma import GemmaEncoder, GemmaGenerator, random_gemma_weights
    W = random_gemma_weights("cpu", cfg, seed=seed)
    enc = GemmaEncoder({k: v.to(dev) for k, v in W.items()}, cfg)
    return W, enc, GemmaGenerator(enc)


def _rel(a, b):
    a, b = G.f64(a), G.f64(b)
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def _decode_reference(window):
    """(f64, bf16-policy) states (L+1,B,24,D) and logits (B,24,V) of the decoded rows 72 .. 95, teacher-forced; computed once."""
    from mlx_video_amd.gemma import random_gemma_weights
    cfg = G.tiny_config(window)
    W = random_gemma_weights("cpu", cfg, seed=3)
    ids, mask = G.tiny_inputs()
    out = []
    for policy in ("f64", "bf16"):
        cache, _, _ = D.prefill(W, cfg, ids[:, :T_PRE], mask[:, :T_PRE], policy, T_total=T_ALL)
        st, lg = [], []
        for t in range(T_PRE, T_ALL):
            s, l = D.step(W, cfg, cache, ids[:, t], policy, T_total=T_ALL)
            st.append(torch.stack(s))
            lg.append(l)
        out.append((torch.stack(st, 2), torch.stack(lg, 1)))
    return out


@pytest.mark.parametrize("window", [1024, 16])
def test_prefill_and_teacher_forced_steps(dev, window):
    """Prefill on the first 72 columns of tiny_inputs (row 1 left-padded by 59): the encoder's states bit for bit.  Then 24
    teacher-forced steps: over the decoded rows each of the L+1 states and the logits satisfies err(device, f64) <= 1.25 x
    err(bf16-policy restatement, f64), both computed here on those rows (1.25: tests/test_gemma_model_gpu.py's margin, for its
    reason).  With window 16 the result is also far from the full-causal restatement."""
    cfg = G.tiny_config(window)
    W, enc, gen = _generator(dev, cfg)
    ids, mask = G.tiny_inputs()
    cache, logits0, pre = gen.prefill(ids[:, :T_PRE], mask[:, :T_PRE], 128, return_states=True)
    want = enc(ids[:, :T_PRE], mask[:, :T_PRE])
    assert torch.equal(_bits(pre), _bits(want)), "the prefill's states are not the encoder's"
    assert cache.length == T_PRE and cache.capacity == 128 and cache.row_start.tolist() == [0, 59]
    L = cfg.num_hidden_layers
    st, lg = [], []
    for t in range(T_PRE, T_ALL):
        l, s = gen.step(cache, ids[:, t], return_states=True)
        st.append(s.cpu())
        lg.append(l.cpu())
    assert cache.length == T_ALL
    st, lg = torch.stack(st, 2), torch.stack(lg, 1)                   # (L+1,B,24,D), (B,24,V)
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (2, T_ALL - T_PRE, cfg.vocab_size) and bool(torch.isfinite(lg).all())
    (f_st, f_lg), (p_st, p_lg) = _decode_reference(window)
    rows = [(f"state{l}", _rel(p_st[l], f_st[l]), _rel(st[l], f_st[l])) for l in range(L + 1)] + [("logits", _rel(p_lg, f_lg), _rel(lg, f_lg))]
    for name, e_ref, e_dev in rows:
        print(f"window {window} {name}: e_ref {e_ref:.3e}  device {e_dev:.3e}  ratio {e_dev / e_ref:.3f}")
    for name, e_ref, e_dev in rows:
        parity.auto(e_dev, 1.25 * e_ref, tag=name)
    if window == 16:
        full = _decode_reference(1024)[0][0]
        assert _rel(st[L], full[L]) > 10 * rows[L][1]


GREEDY_SEED = 3           # of the weights; picked on the CPU (see test_greedy_generation)
N_GREEDY = 12
PENALTY = 100.0           # see test_greedy_generation


def test_greedy_generation(dev):
    """12 tokens at temperature 0 against the f64 restatement's greedy tokens, per batch row up to the first step whose f64 top-2
    logit margin is below 4x the bf16-policy restatement's largest logit error on that row: before it the choice is decided
    beyond what bf16 arithmetic can move.  A random model with a tied head repeats its last input token for ever (the residual
    stream carries that token's embedding, whose product with itself dwarfs every other logit), which would decide every step and
    test nothing; the repetition penalty is therefore set to 100 over the default 20 tokens, so that every step must pick a new
    token among the ~500 others.  The margin is taken on the penalised f64 logits and the error on the model's own logits: a
    token that can win is either outside the context (its logit untouched) or a positive one inside it (its error divided by
    the penalty).  The weights' seed was picked on the CPU so that the bf16-policy restatement itself agrees with f64 on at
    least 8 decided tokens over the two rows; that count is asserted, then the device is held to the same tokens.
    And: eos_ids = row 0's third token stops row 0 after three."""
    from mlx_video_amd.gemma import random_gemma_weights
    cfg = G.tiny_config(1024)
    ids, mask = G.tiny_inputs()
    ids, mask = ids[:, :T_PRE], mask[:, :T_PRE]
    Wc = random_gemma_weights("cpu", cfg, seed=GREEDY_SEED)
    tf, lf, rf = D.greedy(Wc, cfg, ids, mask, N_GREEDY, "f64", penalty=PENALTY)
    tp, _, rp = D.greedy(Wc, cfg, ids, mask, N_GREEDY, "bf16", penalty=PENALTY)
    decided = []
    for b in range(2):
        n = 0
        for i in range(N_GREEDY):
            top = lf[b, i].topk(2).values
            if float(top[0] - top[1]) < 4.0 * float((rp[b, i] - rf[b, i]).abs().max()):
                break
            assert int(tp[b, i]) == int(tf[b, i]), "the bf16-policy restatement departs on a decided token"
            n += 1
        decided.append(n)
    print(f"decided tokens per row: {decided}; f64 tokens {tf.tolist()}")
    assert sum(decided) >= 8, decided
    _, _, gen = _generator(dev, cfg, seed=GREEDY_SEED)
    got = gen.generate(ids, mask, max_tokens=N_GREEDY, temperature=0.0, repetition_penalty=PENALTY, eos_ids=())
    print(f"device tokens {got}")
    assert [len(g) for g in got] == [N_GREEDY] * 2
    for b in range(2):
        assert got[b][:decided[b]] == tf[b, :decided[b]].tolist(), (b, got[b], tf[b].tolist())
    third = got[0][2]
    assert third not in got[0][:2]                                 # (the penalty: no token of the last 20 comes again)
    stop = gen.generate(ids, mask, max_tokens=N_GREEDY, temperature=0.0, repetition_penalty=PENALTY, eos_ids=(third,))
    n1 = got[1].index(third) + 1 if third in got[1] else N_GREEDY
    assert stop[0] == got[0][:3] and stop[1] == got[1][:n1]


# ------------------------------------------------------------------------------------------------ generate_video / CLI
def _write_tokenizer(path, vocab_size=64):
    """A word-level tokenizer over the whole (tiny) vocabulary, so that whatever the model generates decodes to words; a piece
    it does not know (the chat markup) is an ordinary word too, not a special token that decoding would skip."""
    tk = pytest.importorskip("tokenizers")
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import WhitespaceSplit
    from tokenizers.processors import TemplateProcessing
    vocab = {"<pad>": 0, "<eos>": 1, "<bos>": 2}
    vocab.update({f"w{i}": i for i in range(3, vocab_size)})
    tok = tk.Tokenizer(WordLevel(vocab, unk_token=f"w{vocab_size - 1}"))
    tok.pre_tokenizer = WhitespaceSplit()
    tok.add_special_tokens(["<pad>", "<eos>", "<bos>"])
    tok.post_processor = TemplateProcessing(single="<bos> $A", special_tokens=[("<bos>", 2)])
    tok.save(str(path / "tokenizer.json"))


def _gemma_dir(root, hidden, seed):
    from mlx_video_amd.gemma import random_gemma_weights
    from test_gemma_model_gpu import _small_gemma_cfg, _write_gemma_dir
    cfg = _small_gemma_cfg(hidden=hidden)
    _write_gemma_dir(root, cfg, random_gemma_weights("cpu", cfg, seed=seed), with_tokenizer=False)
    _write_tokenizer(root)
    return cfg


def test_generate_video_enhance_prompt(dev, tmp_path, monkeypatch):
    """generate_video(enhance_prompt=True) gives the latents of passing the enhanced string as ``prompt``, and those differ from
    the un-enhanced run's."""
    pytest.importorskip("tokenizers")
    from mlx_video_amd import generate as GV
    from mlx_video_amd.text_connector import TextConnector, random_connector_weights
    from test_pipeline_gpu import _mods, _Noise
    m = _mods(dev)
    root = tmp_path / "gemma"
    cfg = _gemma_dir(root, 256, seed=9)
    conn = TextConnector(random_connector_weights(dev, D=256, L=cfg.num_hidden_layers + 1, layers=1, R=16))
    seen = []
    real = GV._enhance_prompt

    def spy(*a):
        out = real(*a)
        seen.append(out[1])
        return out

    monkeypatch.setattr(GV, "_enhance_prompt", spy)
    common = dict(pipeline=GV.PipelineType.DEV, height=128, width=128, num_frames=9, num_inference_steps=2, cfg_scale=4.0,
                  transformer=m["transformer"], vae_decoder=m["vae_decoder"], compile_step=True, cfg_batch=True, device=dev,
                  return_latents=True, gemma_repo=str(root), text_connector=conn, negative_prompt="w9")
    a = GV.generate_video(prompt="w4 w5", enhance_prompt=True, max_tokens=8, temperature=0.0, noise_fn=_Noise(7, dev), **common)
    assert len(seen) == 1 and seen[0] and seen[0] != "w4 w5" and 1 <= len(seen[0].split()) <= 8
    b = GV.generate_video(prompt=seen[0], noise_fn=_Noise(7, dev), **common)
    c = GV.generate_video(prompt="w4 w5", noise_fn=_Noise(7, dev), **common)
    assert len(seen) == 1                                           # off by default: nothing of it runs
    assert torch.equal(a, b) and not torch.equal(a, c) and bool(torch.isfinite(a.float()).all())
    # another system prompt is another chat prompt: the argument reaches the model
    GV.generate_video(prompt="w4 w5", enhance_prompt=True, max_tokens=8, temperature=0.0, enhance_system_prompt="w7 w8 w9",
                      noise_fn=_Noise(7, dev), **common)
    assert len(seen) == 2 and seen[1]


def test_cli_enhance_prompt(dev, tmp_path):
    """`generate --synthetic --gemma-repo DIR --prompt ... --enhance-prompt --max-tokens 8 --temperature 0` on a directory written
    here (a 2-layer Gemma of the real width) writes a video of the right shape."""
    pytest.importorskip("tokenizers")
    from mlx_video_amd import generate as GV
    root = tmp_path / "gemma"
    _gemma_dir(root, 3840, seed=4)
    sysfile = tmp_path / "system.txt"
    sysfile.write_text("w10 w11")
    out = tmp_path / "enh.npy"
    GV.main(["--synthetic", "--layers", "1", "--pipeline", "distilled", "--height", "128", "--width", "128", "--num-frames", "9",
             "--stage1-steps", "1", "--stage2-steps", "1", "--tiling", "none", "--gemma-repo", str(root), "--prompt", "w4 w5",
             "--negative-prompt", "w6", "--enhance-prompt", "--max-tokens", "8", "--temperature", "0", "--enhance-system-prompt", str(sysfile),
             "--output-path", str(out)])
    frames = np.load(out)
    assert frames.shape == (9, 128, 128, 3) and frames.dtype == np.uint8
