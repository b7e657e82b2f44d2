"""The GEMM launch sequence of LTXModel.forward_tokens, pinned: ops.gemm, ops.gemm_grouped and ops.quant_rows_fp8 are wrapped,
one forward runs, and the ordered list of calls - shapes, epilogue, output split, row statistics, split_k, operand dtypes, weight
scale - must be the one built from the dit_launches table that aims test_gemm_plan_cpu.py, test_batch_invariance_gpu.py and
test_gemm_splitk_gpu.py.  A forgotten split_k or w_scale, a launch out of order or a second context quantisation fails here.

Small config (heads 4 -> D = 512, L = 2, caption 256; B = 2, N = 90, S = 100, two timestep rows) as in test_fp8_act_model_gpu;
one case at N = 480 (M = 960 > ops.SPLITK_MAX_M, a multiple of 320) where fuse bit 8 splits q|k|v into q|k + v."""
import pytest
import torch

from dit_launches import dit_launches
from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F8 = torch.float8_e4m3fn
B, S, L, DIM = 2, 100, 2, 512
IN_BLOCK = ("qkv", "qk", "v", "out", "q2", "text_kv", "text_k", "text_v", "o2", "ff1", "ff2")   # the launches fp8_activations may run W8A8

# name -> model switches; "geom": (F,H,W) of the video tokens, "hoisted": text K/V from prepare_context (traced too)
CASES = {
    "bf16_fuse15": dict(),
    "bf16_fuse0": dict(fuse=0),
    "bf16_fuse7": dict(fuse=7),
    "batch_invariant": dict(batch_invariant=True),
    "per_block_context": dict(grouped_context_kv=False),
    "hoisted_context": dict(hoisted=True),
    "fp8_channel_scales": dict(fp8=True),
    "fp8_activations": dict(fp8=True, fp8_activations=True),
    "fp8_activations_hoisted": dict(fp8=True, fp8_activations=True, hoisted=True),
    "bf16_m960_fuse15": dict(geom=(5, 8, 12)),
}


def make_weights(dev):
    """{fp8?: weight dict}: bf16 weights on the device and their channel-scaled fp8 dict."""
    from mlx_video_amd.weights import transformer_weights
    W = O.make_weights(O.DiTConfig(num_layers=L, heads=4, caption_channels=256), seed=11)
    return {False: {k: v.to(dev) for k, v in W.items()}, True: transformer_weights(W, dev, fp8=True, fp8_scaling="channel")}


@pytest.fixture(scope="module")
def weights(dev):
    """Built once, never modified."""
    return make_weights(dev)


def build_case(name, weights, dev):
    """-> (model, forward_tokens arguments, N, hoisted) of one case; also what a bit-comparison script runs."""
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig, TimestepPlan, precompute_freqs_cis
    c = CASES[name]
    mc = LTXModelConfig(num_attention_heads=4, num_layers=L, caption_channels=256, cross_attention_dim=DIM)
    m = LTXModel(mc, weights[c.get("fp8", False)], fuse=c.get("fuse", 15), fp8_activations=c.get("fp8_activations", False))
    m.batch_invariant = c.get("batch_invariant", False)
    m.grouped_context_kv = c.get("grouped_context_kv", True)
    F, Hh, Ww = c.get("geom", (3, 5, 6))
    N = F * Hh * Ww
    g = torch.Generator().manual_seed(42)
    lat = torch.randn(B, N, 128, generator=g).to(BF).to(dev)
    ctx = torch.randn(B, S, 256, generator=g).to(BF).to(dev)
    ts = torch.full((B, N), 0.909375).to(BF)
    ts[:, : Hh * Ww] = 0.0                                   # two distinct timestep rows
    pos = torch.from_numpy(O.create_position_grid(B, F, Hh, Ww)).to(dev)
    pe = precompute_freqs_cis(pos, m.inner_dim, m.positional_embedding_theta, m.positional_embedding_max_pos, m.num_attention_heads)
    return m, (lat, TimestepPlan.from_timesteps(ts.to(dev)), ctx, pe), N, c.get("hoisted", False)


def _trace(monkeypatch, ops, calls):
    real_gemm, real_grouped, real_quant = ops.gemm, ops.gemm_grouped, ops.quant_rows_fp8

    def gemm(a, w, bias, **kw):
        calls.append(("gemm", a.shape[0], w.shape[0], a.shape[1], kw.get("epilogue", ops.EPI_BIAS), kw.get("n_split", 0),
                      kw.get("out_tokens_per_batch", 0), kw.get("sumsq") is not None, kw.get("split_k", True), w.dtype, a.dtype,
                      kw.get("w_scale") is not None))
        assert (a.dtype == F8) == (kw.get("a_scale") is not None)
        return real_gemm(a, w, bias, **kw)

    def gemm_grouped(a, w_table, bias_table, N, **kw):
        calls.append(("gemm_grouped", w_table.numel(), a.shape[0], N, a.shape[1], kw["n_split"], kw["out_tokens_per_batch"],
                      kw.get("sumsq") is not None))
        return real_grouped(a, w_table, bias_table, N, **kw)

    def quant_rows_fp8(a, out=None):
        calls.append(("quant_rows_fp8",) + tuple(a.shape))
        return real_quant(a, out=out)

    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "gemm_grouped", gemm_grouped)
    monkeypatch.setattr(ops, "quant_rows_fp8", quant_rows_fp8)


def _expected(ops, name, N):
    """(the calls of prepare_context, the calls of forward_tokens) for one case, from the dit_launches table."""
    c = CASES[name]
    fuse, fp8, act = c.get("fuse", 15), c.get("fp8", False), c.get("fp8_activations", False)
    sk = not c.get("batch_invariant", False)
    M = B * N
    table = {n: (m, nn, k, kw) for n, m, nn, k, kw in dit_launches(ops, B, N, S, D=DIM, caption=256, U=2)}

    def opts(n):
        m, nn, k, kw = table[n]
        return m, nn, k, dict(kw, sumsq=bool(kw.get("sumsq")) and (n == "patchify" or bool(fuse & 2)))

    def w8a8(n):         # LTXModel: fp8 activations where the W8A16 launch would be single-pass
        m, nn, k, kw = opts(n)
        return act and n in IN_BLOCK and k % 128 == 0 and not ops.gemm_plan(m, nn, k, split_k=sk, w8=True, **kw).split_k

    def group(*names):   # the launches over one input: one quantiser launch in front if any of them runs W8A8
        out = [("quant_rows_fp8", table[names[0]][0], table[names[0]][2])] if any(w8a8(n) for n in names) else []
        for n in names:
            m, nn, k, kw = opts(n)
            out.append(("gemm", m, nn, k, kw.get("epilogue", ops.EPI_BIAS), kw.get("n_split", 0), kw.get("out_tokens_per_batch", 0),
                        kw["sumsq"], sk, F8 if fp8 else BF, F8 if w8a8(n) else BF, fp8))
        return out

    text = ("text_kv",) if fuse & 1 else ("text_k", "text_v")
    qkv = ("qkv",) if fuse & 1 and (not fuse & 8 or M <= ops.SPLITK_MAX_M or M % 320 != 0) else ("qk", "v")
    # one grouped launch for all blocks where LTXModel._grouped_context_ok: bf16 panels, the fused forms, and a single-pass plan
    m, nn, k, kw = table["text_kv"]
    grouped = c.get("grouped_context_kv", True) and (fuse & 3) == 3 and not fp8 and not ops.gemm_plan(m, nn, k, split_k=sk, **kw).split_k
    text_q = group(*text)[:-len(text)]                               # the context is quantised once, in front of block 0
    text_l = group(*text)[-len(text):]
    if grouped:
        context = [("gemm_grouped", L, m, nn, k, kw["n_split"], kw["out_tokens_per_batch"], True)]
    else:
        context = text_q
    caption = group("caption1") + group("caption2")
    prepare = caption + context + ([] if grouped else text_l * L)
    fwd = group("patchify") + group("timestep1") + group("timestep2") + group("adaln")
    hoisted = c.get("hoisted", False)
    if not hoisted:
        fwd += caption + context
    for _ in range(L):
        fwd += group(*qkv) + group("out") + group("q2") + ([] if hoisted or grouped else text_l) + group("o2") + group("ff1") + group("ff2")
    return prepare, fwd + group("proj_out")


def _check_aim(ops, name, N):
    """What each case relies on, asked of ops.gemm_plan first: when a heuristic moves, this says which case to re-aim."""
    c = CASES[name]
    sk = not c.get("batch_invariant", False)
    table = {n: (m, nn, k, kw) for n, m, nn, k, kw in dit_launches(ops, B, N, S, D=DIM, caption=256, U=2)}
    m, nn, k, kw = table["text_kv"]
    assert not ops.gemm_plan(m, nn, k, split_k=sk, **kw).split_k, "the text k|v launch splits K here: no case takes the grouped launch"
    if c.get("fp8_activations"):
        for n in IN_BLOCK:
            m, nn, k, kw = table[n]
            assert not ops.gemm_plan(m, nn, k, split_k=sk, w8=True, **kw).split_k, f"{n} would split K at M={m}: it stays W8A16"
    if "geom" in c:
        assert B * N > ops.SPLITK_MAX_M and B * N % 320 == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_launch_sequence(dev, weights, monkeypatch, name):
    from mlx_video_amd import ops
    m, args, N, hoisted = build_case(name, weights, dev)
    _check_aim(ops, name, N)
    want_prepare, want = _expected(ops, name, N)
    calls = []
    _trace(monkeypatch, ops, calls)
    kv, prepared = None, []
    if hoisted:
        kv = m.prepare_context(args[2])
        assert calls == want_prepare, _first_difference(calls, want_prepare)
        prepared = list(calls)
        calls.clear()
    v = m.forward_tokens(*args, ctx_kv=kv)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v.float()).all())
    assert calls == want, _first_difference(calls, want)
    # the sequence says what the case is meant to show
    kinds = [c[0] for c in calls]
    if name in ("bf16_fuse15", "bf16_fuse7", "batch_invariant", "bf16_m960_fuse15"):
        assert kinds.count("gemm_grouped") == 1
    if name == "bf16_m960_fuse15":
        assert sum(1 for c in calls if c[:4] == ("gemm", B * N, 2 * DIM, DIM)) == L          # q|k as its own launch
    if name.startswith("fp8_activations"):
        assert kinds.count("quant_rows_fp8") == 6 * L + (0 if hoisted else 1)
        assert sum(1 for c in calls if c[0] == "gemm" and c[10] == F8) == (6 if hoisted else 7) * L
        if hoisted:              # prepare_context quantised the context, once; the forward then not at all
            assert [c for c in prepared if c[0] == "quant_rows_fp8"] == [("quant_rows_fp8", B * S, DIM)]
            assert ("quant_rows_fp8", B * S, DIM) not in calls


def _first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"call {i}: got {g}, expected {w}"
    return f"{len(got)} calls, expected {len(want)}; the first {min(len(got), len(want))} agree"
