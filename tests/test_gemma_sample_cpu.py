"""The device sampler without a GPU: the float64 reference ``ref_gemma_sample.admissible`` against an fp32 emulation of the
kernel's chunked order (csrc/sample.hip) at the full vocabulary, planted faults on the small inputs, temperature 0 against
``gemma.sample_tokens``, the binding, the shim's refusals and the public switches of the device loop."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ref_gemma_sample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_FULL = 262208


def test_depth_constant_is_shared():
    """The chain length the tolerance is built on is one number in three places: the reference, ops and the kernel's comment."""
    from mlx_video_amd import ops
    src = open(os.path.join(ROOT, "mlx-video_amd", "csrc", "sample.hip")).read()
    assert ops.SAMPLE_CHUNK == S.SAMPLE_CHUNK == 2048 and ops.SAMPLE_DEPTH_BASE == S.SAMPLE_DEPTH_BASE == 17
    assert "SAMPLE_DEPTH_BASE = 17" in src and "depth(V) = 17 + ceil(V / 2048), 146 at V = 262208" in src
    assert ops.sample_depth(V_FULL) == S.sample_depth(V_FULL) == 146 and S.sample_depth(8) == 18 and S.sample_depth(4104) == 20
    assert re.search(r"constexpr int SP_CHUNK = SP_THREADS \* 8;", src) and "constexpr int SP_THREADS = 256;" in src


@pytest.mark.parametrize("std,temperature", [(3.0, 0.7), (8.0, 0.7), (1.0, 1.5)])
def test_emulation_lands_in_the_admissible_set(std, temperature):
    """V = 262208 bf16-rounded normal logits, a context of 20 ids with a duplicate at penalty 1.3, 2000 uniforms: the fp32
    emulation's token is admissible at every one of them, and its total is far inside the tolerance."""
    g = np.random.default_rng(int(std * 10 + temperature * 100))
    logits = S.bf16_round(g.standard_normal(V_FULL) * std)
    ctx = list(g.integers(0, V_FULL, 19)) + [int(np.argmax(logits))]
    ctx.append(ctx[3])
    cdf = S.cdf64(logits, ctx, 1.3, temperature)
    emu = S.Emulation(logits, ctx, 1.3, temperature)
    err, tol = abs(float(emu.S) - cdf[3]) / cdf[3], cdf[4] / cdf[3]
    print(f"std {std} T {temperature}: |S_fp32 - S| / S = {err:.2e}, tol / S = {tol:.2e}")
    assert err < tol
    us = torch.rand(2000, generator=torch.Generator().manual_seed(11)).numpy()
    us[:4] = (0.0, np.float32(1.0) - np.float32(2.0 ** -24), 0.5, 2.0 ** -20)
    sizes = []
    for u in us:
        ok = S.admissible(logits, ctx, 1.3, temperature, u, cdf)
        t = emu.token(u)
        assert t in ok, (float(u), t, sorted(ok)[:4])
        sizes.append(len(ok))
    print(f"admissible set sizes: min {min(sizes)} median {int(np.median(sizes))} max {max(sizes)}")


SMALL = [(8, 2), (264, 130)]          # (V, index of the first dominant token)


def _small(V, at):
    """logits, context (the middle dominant id twice, a floor id, an id past the row), penalty, temperature."""
    return S.dominant_logits(V, at), [at + 1, 0, at + 1, V + 5], 1.3, 0.7


def _moved(honest_cdf, fault_cdf):
    """(measure, runs) of the u in [0, 1) at which the float64 inverse CDF of the faulty distribution returns another token than
    the honest one's: the total length and the number of maximal intervals."""
    edges = np.unique(np.concatenate([[0.0, 1.0], honest_cdf[2] / honest_cdf[3], fault_cdf[2] / fault_cdf[3]]).clip(0.0, 1.0))
    mid = (edges[:-1] + edges[1:]) / 2
    tok = lambda cdf: np.searchsorted(cdf[2] / cdf[3], mid, side="right")          # noqa: E731
    differs = tok(honest_cdf) != tok(fault_cdf)
    runs = int(np.count_nonzero(differs[1:] & ~differs[:-1]) + bool(differs[0]))
    return float((edges[1:] - edges[:-1])[differs].sum()), runs


@pytest.mark.parametrize("V,at", SMALL)
def test_planted_faults_fall_outside(V, at):
    """Three dominant neighbours (p > 4 tol each, asserted).  On the grid u_i = (i + 1/2) / 256 the honest emulation is admissible
    throughout and all but a few sets are single; the next and the previous token are outside the set at every uniform whose
    set is single.  The temperature left out, the penalty left out and the penalty applied per occurrence move the float64
    inverse CDF on a set of u of measure mu made of k intervals (computed here): a grid of 256 points has at least 256 mu - k
    of them inside it, and the fault must be outside the admissible set at that many, less the points whose set is not single.
    The uniform of draw n +- 1 on 257 seeded uniforms: two independent uniforms land in different tokens with probability
    P = 1 - sum q^2; the count of caught pairs is held to its mean less four standard deviations."""
    logits, ctx, pen, T = _small(V, at)
    cdf = S.cdf64(logits, ctx, pen, T)
    p, _, _, Ssum, tol = cdf
    assert all(p[at + i] > 4 * tol for i in range(3)) and tol / Ssum < 1e-5
    grid = ((np.arange(256) + 0.5) / 256).astype(np.float32)
    sets = [S.admissible(logits, ctx, pen, T, u, cdf) for u in grid]
    many = sum(len(s) != 1 for s in sets)
    assert many <= 2 * V * tol / Ssum * 256 + 3                       # (a set is not single only within tol of one of <= V edges)
    honest = S.Emulation(logits, ctx, pen, T)
    assert all(honest.token(u) in ok for u, ok in zip(grid, sets))
    for fault in ("next", "prev"):
        emu = S.Emulation(logits, ctx, pen, T, fault)
        assert all(emu.token(u) not in ok for u, ok in zip(grid, sets) if len(ok) == 1), fault
    for fault, fcdf in (("no_temperature", S.cdf64(logits, ctx, pen, 1.0)), ("no_penalty", S.cdf64(logits, [], pen, T)),
                        ("penalty_twice", S.cdf64(S.penalised(logits, [at + 1], pen), ctx, pen, T))):
        mu, k = _moved(cdf, fcdf)
        emu = S.Emulation(logits, ctx, pen, T, fault)
        caught = sum(emu.token(u) not in ok for u, ok in zip(grid, sets))
        print(f"V {V} {fault}: moved measure {mu:.4f} in {k} intervals, caught at {caught} of 256 grid points")
        assert mu > 0.02 and caught >= 256 * mu - k - many, (fault, mu, k, caught)
    us = torch.rand(257, generator=torch.Generator().manual_seed(V)).numpy()
    usets = [S.admissible(logits, ctx, pen, T, u, cdf) for u in us]
    q = p / Ssum
    P = 1.0 - float((q * q).sum())
    floor = 256 * P - 4 * (256 * P * (1 - P)) ** 0.5
    for name, pairs in (("uniform n+1", zip(us[1:], usets[:-1])), ("uniform n-1", zip(us[:-1], usets[1:]))):
        caught = sum(honest.token(u) not in ok for u, ok in pairs)
        print(f"V {V} {name}: caught at {caught} of 256 draws, floor {floor:.1f}")
        assert caught >= floor, (name, caught, floor)


def test_temperature_zero_is_sample_tokens():
    """Greedy: the reference and the emulation equal ``gemma.sample_tokens`` exactly - ties included, the lowest index winning,
    which is asserted of torch.argmax on this build once - with the context empty, duplicated, and at penalties 1, 1.3, 100."""
    from mlx_video_amd.gemma import sample_tokens
    assert int(torch.tensor([1.0, 3.0, 3.0, 2.0, 3.0]).argmax()) == 1 and int(torch.zeros(4104).argmax()) == 0
    g = np.random.default_rng(5)
    for V in (8, 264, 4104):
        base = S.bf16_round(g.standard_normal(V) * 3)
        rows = {"plain": base, "max_first": base.copy(), "max_last": base.copy(), "tie": base.copy(), "negative": S.bf16_round(-np.abs(base) - 1)}
        rows["max_first"][0], rows["max_last"][V - 1] = 50.0, 50.0
        rows["tie"][[1, V // 2, V - 2]] = 40.0
        top = int(np.argmax(base))
        for name, l in rows.items():
            for ctx in ([], [top, 1, V // 2, top, V - 2] * 12 + [0, 0, V - 1, 3]):
                for pen in (1.0, 1.3, 100.0):
                    want = int(sample_tokens(torch.from_numpy(l)[None], [ctx], 0.0, pen, None)[0])
                    assert S.admissible(l, ctx, pen, 0.0, 0.3) == {want}, (V, name, pen)
                    assert S.Emulation(l, ctx, pen, 0.0).token(0.3) == want
    # the penalty's fp32 arithmetic is apply_repetition_penalty's, bit for bit
    from mlx_video_amd.gemma import apply_repetition_penalty
    l = S.bf16_round(g.standard_normal(264) * 5)
    ctx = list(range(0, 264, 3)) + [3, 3]
    for pen in (1.3, 100.0, 0.7):
        got = S.penalised(l, ctx, pen)
        assert np.array_equal(got.view(np.int32), apply_repetition_penalty(torch.from_numpy(l)[None], [ctx], pen)[0].numpy().view(np.int32))


# ------------------------------------------------------------------------------------------------------ binding and shims
def test_binding_and_header():
    from mlx_video_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ltxk.h")).read()
    lib = _lib.load()
    for name in ("ltxk_sample_rows", "ltxk_causal_attn_dev_step", "ltxk_headnorm_rope_at"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf"\bint {name}\(", hdr), name
    assert "LTXK_SAMPLE_DRAW = 1, LTXK_SAMPLE_ADVANCE = 2" in hdr and (_lib.SAMPLE_DRAW, _lib.SAMPLE_ADVANCE) == (1, 2)
    # the struct's layout is checked by the library itself: a wrong struct_bytes is refused before anything else is read
    a = _lib.SampleArgs()
    a.struct_bytes = ctypes.sizeof(_lib.SampleArgs) + 8
    assert lib.ltxk_sample_rows(ctypes.byref(a), None) == -1 and b"struct_bytes" in lib.ltxk_last_error()
    a.struct_bytes = ctypes.sizeof(_lib.SampleArgs)
    assert lib.ltxk_sample_rows(ctypes.byref(a), None) == -1 and b"flags" in lib.ltxk_last_error()
    a.flags = _lib.SAMPLE_ADVANCE
    assert lib.ltxk_sample_rows(ctypes.byref(a), None) == -1 and b"ctl" in lib.ltxk_last_error()
    # null pointers and a max_step past the cache are refused on the host
    assert lib.ltxk_causal_attn_dev_step(*([None, 0] * 6), None, 1, 2, 2, 64, None, 0, 0, 1.0, None, 0, None) == -1
    assert lib.ltxk_headnorm_rope_at(None, 0, 1, 1, 1, None, None, None, None, 1, None, 1e-6, None) == -1


def _state(B=2, V=264, Nmax=4, Hcap=32, n_eos=2):
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)          # noqa: E731
    from mlx_video_amd import ops
    return dict(logits=torch.zeros(B, V, dtype=torch.bfloat16), ctl=i32(3), done=i32(B), next_ids=i32(B), history=i32(B, Hcap),
                hist_len=i32(B), tokens_out=i32(B, Nmax), eos=i32(n_eos), uniforms=torch.zeros(Nmax, B),
                workspace=torch.zeros(ops.sample_workspace_floats(B, V)))


def test_sample_rows_refuses_bad_operands_before_any_launch():
    """Every tensor of ``ops.sample_rows`` with the wrong dtype, a wrong extent and a non-contiguous layout, on CPU tensors - so a
    refusal other than the device's comes before the device check; a well-formed CPU call is refused for the device only."""
    from mlx_video_amd import _lib, ops
    good = _state()
    call = lambda st, **kw: ops.sample_rows(*st.values(), **dict(dict(temperature=0.7, penalty=1.3, rep_ctx=20), **kw))       # noqa: E731
    with pytest.raises(_lib.LtxkError, match="sample_rows: .* device tensor.*no CPU fallback"):
        call(good)
    assert ops.sample_workspace_floats(2, 264) == 6 and ops.sample_workspace_floats(8, 262208) == 3 * 8 * 129
    for name, t in good.items():
        other = torch.float32 if t.dtype != torch.float32 else torch.int32
        with pytest.raises(TypeError, match=f"sample_rows: .*{name}"):
            call(dict(good, **{name: torch.zeros(t.shape, dtype=other)}))
        if name not in ("logits", "tokens_out", "history", "eos"):          # (the operands the sizes come from: reported under a partner)
            with pytest.raises(ValueError, match=f"sample_rows: .*{name}"):
                call(dict(good, **{name: torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] - 1,), dtype=t.dtype)}))
        if t.numel() > 1:
            with pytest.raises(ValueError, match="sample_rows: "):
                call(dict(good, **{name: torch.stack([t, t], -1)[..., 0]}))
    for bad, match in ((dict(logits=torch.zeros(9, 264, dtype=torch.bfloat16)), "1 <= B <= 8"), (dict(logits=torch.zeros(2, 260, dtype=torch.bfloat16)), "multiple of 8"),
                       (dict(eos=torch.zeros(9, dtype=torch.int32)), "eos"), (dict(tokens_out=torch.zeros(3, 4, dtype=torch.int32)), "tokens_out"),
                       (dict(history=torch.zeros(3, 32, dtype=torch.int32)), "history"), (dict(uniforms=None), "uniforms")):
        with pytest.raises(ValueError, match=f"sample_rows: .*{match}"):
            call(dict(good, **bad))
    for kw, match in ((dict(rep_ctx=65), "rep_ctx"), (dict(temperature=-0.1), "temperature"), (dict(penalty=0.0), "penalty"),
                      (dict(draw=False, advance=False), "neither")):
        with pytest.raises(ValueError, match=f"sample_rows: .*{match}"):
            call(good, **kw)
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        call(dict(good, uniforms=None), temperature=0.0)                    # greedy needs no uniforms


def test_device_position_forms_refuse_before_any_launch():
    from mlx_video_amd import _lib, ops
    BF = torch.bfloat16
    z = lambda *s, dtype=BF: torch.zeros(s, dtype=dtype)          # noqa: E731
    pos = z(1, dtype=torch.int32)
    hn = (z(8, 1024), 2, 1, z(256), z(256), z(4, 128, dtype=torch.float32), z(4, 128, dtype=torch.float32), 4)
    with pytest.raises(_lib.LtxkError, match="headnorm_rope: .* device tensor"):
        ops.headnorm_rope(*hn, pos=pos)
    with pytest.raises(TypeError, match="headnorm_rope: pos"):
        ops.headnorm_rope(*hn, pos=z(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="headnorm_rope: pos"):
        ops.headnorm_rope(*hn, pos=z(2, dtype=torch.int32))
    B, Hq, Hkv, cap = 2, 4, 2, 320
    need = B * Hq * 2 * 258
    ca = lambda **kw: ops.causal_attn(z(B, 1024), z(B * cap, 512), z(B, 512, cap), z(B, 1024), z(B, dtype=torch.int32), B, Hq, Hkv, cap, 0.0625,        # noqa: E731
                                      **dict(dict(step=pos, max_step=cap - 1, k_new=z(B, 512), v_new=z(B, 512), partials=z(need, dtype=torch.float32)), **kw))
    with pytest.raises(_lib.LtxkError, match="causal_attn: .* device tensor"):
        ca()
    with pytest.raises(ValueError, match="causal_attn: .*partials"):
        ca(partials=z(need - 1, dtype=torch.float32))
    with pytest.raises(_lib.LtxkError, match="device tensor"):
        ca(window=16, partials=z(B * Hq * 2 * 258, dtype=torch.float32))       # a window of 16 keys touches at most 2 slices
    with pytest.raises(ValueError, match="causal_attn: .*partials"):
        ca(window=16, partials=z(B * Hq * 1 * 258, dtype=torch.float32))
    with pytest.raises(ValueError, match="causal_attn: .*max_step"):
        ca(max_step=None)
    with pytest.raises(ValueError, match="causal_attn: .*max_step"):
        ca(step=3, max_step=5)
    with pytest.raises(ValueError, match="causal_attn: max_step = 320"):
        ca(max_step=cap)
    with pytest.raises(TypeError, match="causal_attn: step"):
        ca(step=z(1, dtype=torch.int64))
    assert [ops.causal_attn_step_slices(m, w) for m, w in ((0, 0), (255, 0), (256, 0), (1023, 0), (1023, 16), (1023, 1), (1023, 1024), (100, 1024), (1023, 258))] == \
        [1, 1, 2, 4, 2, 1, 4, 1, 3]
    # every slice count a step can have fits the launch's count
    for w in (1, 2, 16, 255, 256, 257, 258, 513, 1024):
        most = max(s // 256 + 1 - max(0, s - w + 1) // 256 for s in range(2048))
        assert most == ops.causal_attn_step_slices(2047, w), w
    with pytest.raises(_lib.LtxkError, match="embed_rows: .* device tensor"):
        ops.embed_rows(z(16, 512), z(8, dtype=torch.int32), 22.0, trusted_ids=True)


def test_public_switches():
    """The device loop is off by default at every level and documented as consuming its seed differently."""
    from mlx_video_amd import gemma as GM, generate as GV
    sig = inspect.signature(GM.GemmaGenerator.generate).parameters
    assert (sig["device_loop"].default, sig["graph"].default, sig["sync_every"].default) == (False, True, 16)
    assert inspect.signature(GM.enhance_prompt).parameters["device_loop"].default is False
    assert inspect.signature(GV.generate_video).parameters["enhance_device_loop"].default is False
    assert GV.build_parser().parse_args(["--enhance-prompt", "--enhance-device-loop"]).enhance_device_loop is True
    assert GV.build_parser().parse_args([]).enhance_device_loop is False
    for doc in (GM.GemmaGenerator.generate.__doc__, GM.enhance_prompt.__doc__, GV.generate_video.__doc__):
        assert "seed" in doc and "other" in doc
    with pytest.raises(ValueError, match="enhance_device_loop"):
        GV.generate_video(prompt="x", enhance_device_loop=True)
    cfg = GM.GemmaConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1, intermediate_size=64, vocab_size=64)
    ids = torch.tensor([[0, 0, 5, 6, 7], [1, 2, 3, 4, 5]])
    st = GM.GemmaDecodeState(cfg, 64, ids, (ids > 0).long(), 6, (1, 107, 1), seed=3, device="cpu")
    assert st.ctl.tolist() == [0, 5, 2] and st.hist_len.tolist() == [3, 5] and st.history[0, :3].tolist() == [5, 6, 7]
    assert st.history.shape == (2, 11) and st.eos.tolist() == [1, 107] and st.tokens_out.shape == (2, 6) and st.logits.shape == (2, 64)
    assert torch.equal(st.uniforms, torch.rand((6, 2), generator=torch.Generator().manual_seed(3))) and st.pos.data_ptr() == st.ctl.data_ptr() + 4
    for bad in (dict(max_tokens=0), dict(eos_ids=range(9))):
        with pytest.raises(ValueError, match="GemmaDecodeState"):
            GM.GemmaDecodeState(cfg, 64, ids, (ids > 0).long(), **dict(dict(max_tokens=6, eos_ids=(1,), seed=3, device="cpu"), **bad))
    with pytest.raises(ValueError, match="1 to 8 batch rows"):
        GM.GemmaDecodeState(cfg, 64, ids.repeat(5, 1), (ids > 0).long().repeat(5, 1), 6, (1,), 3, "cpu")
