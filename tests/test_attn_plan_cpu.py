"""The attention launch plan on the host (ltxk_flash_attn_plan through ops.flash_attn_plan; no GPU): which kernel, how many
192- and 128-row tiles per (batch, head), and the key-split tail.  ltxk_flash_attn decides its form by the same host function
(fa_form, csrc/attention.hip) with the device's own CU count, so these plans are the launches' forms.
tests/test_attn_forms_gpu.py asserts the plan of every case before it relies on it; when a rule here moves, re-aim those."""
import ctypes
import functools
import os

import numpy as np
import pytest

K128, MIX = 0, 1
NO_TAIL_SPLIT = 1
A = 1 << 12                     # a 16-byte aligned stand-in address

# B, H, Tq, Tk, cus, flags -> kernel, tiles_192, tiles_128, whole_workgroups, split_tiles, workgroups, xcd_order
# (the launcher's rules before fa_form existed, evaluated by hand on the CPU)
TABLE = [
    (2, 32, 1280, 1280, 256, 0, MIX, 4, 4, 512, 0, 512, 1),
    (2, 32, 1280, 1024, 256, 0, MIX, 4, 4, 512, 0, 512, 1),
    (4, 32, 1280, 1280, 256, 0, MIX, 4, 4, 1024, 0, 1024, 1),
    (2, 32, 1296, 1296, 256, 0, MIX, 7, 0, 448, 0, 448, 1),
    (2, 32, 1536, 1280, 256, 0, MIX, 8, 0, 512, 0, 512, 1),
    (2, 32, 2560, 2560, 256, 0, MIX, 12, 2, 896, 0, 896, 1),
    (1, 32, 2560, 1024, 256, 0, MIX, 14, 0, 448, 0, 448, 1),
    (2, 32, 3328, 1024, 256, 0, MIX, 16, 2, 1152, 0, 1152, 1),
    (2, 32, 5184, 5184, 256, 0, MIX, 27, 0, 1728, 0, 1728, 1),
    (2, 32, 6656, 6656, 256, 0, MIX, 32, 4, 2304, 0, 2304, 1),
    (1, 32, 1280, 1280, 256, 0, K128, 0, 10, 128, 192, 512, 1),
    (1, 32, 1280, 1280, 256, NO_TAIL_SPLIT, K128, 0, 10, 320, 0, 320, 1),
    (2, 32, 1024, 1280, 256, 0, K128, 0, 8, 512, 0, 512, 1),
    (1, 32, 2048, 2048, 256, 0, K128, 0, 16, 512, 0, 512, 1),
    (2, 32, 640, 1024, 256, 0, K128, 0, 5, 128, 192, 512, 1),
    (2, 32, 320, 1024, 256, 0, K128, 0, 3, 0, 192, 384, 1),
    (1, 32, 640, 640, 256, 0, K128, 0, 5, 0, 160, 320, 1),
    (2, 32, 128, 1024, 256, 0, K128, 0, 1, 0, 64, 128, 1),
    (2, 32, 129, 1024, 256, 0, K128, 0, 2, 0, 128, 256, 1),
    (3, 5, 1290, 100, 256, 0, K128, 0, 11, 0, 165, 330, 0),
    (1, 3, 200, 70, 256, 0, K128, 0, 2, 0, 6, 12, 0),
    (1, 1, 128, 64, 256, 0, K128, 0, 1, 0, 1, 2, 0),
    (2, 32, 1280, 1280, 304, 0, K128, 0, 10, 608, 32, 672, 1),
    (1, 32, 1280, 1280, 64, 0, MIX, 4, 4, 256, 0, 256, 1),
    (2, 4, 400, 400, 8, 0, MIX, 1, 2, 24, 0, 24, 1),
    (1, 4, 400, 400, 8, 0, K128, 0, 4, 16, 0, 16, 0),
    (1, 8, 520, 130, 8, 0, MIX, 3, 0, 24, 0, 24, 1),
]

# the cases of tests/test_attn_forms_gpu.py at the MI355X's 256 CUs: (B, H, Tq, Tk, tail_split) -> the same seven fields
GPU_CASES = [
    (1, 3, 200, 70, True, K128, 0, 2, 0, 6, 12, 0),
    (1, 4, 200, 70, True, K128, 0, 2, 0, 8, 16, 0),
    (1, 32, 1280, 128, True, K128, 0, 10, 128, 192, 512, 1),
    (2, 32, 640, 128, True, K128, 0, 5, 128, 192, 512, 1),
    (1, 32, 1280, 128, False, K128, 0, 10, 320, 0, 320, 1),
    (2, 32, 1280, 128, True, MIX, 4, 4, 512, 0, 512, 1),
    (2, 32, 1296, 136, True, MIX, 7, 0, 448, 0, 448, 1),
]

SWEEP_BH = [1, 3, 8, 15, 32, 64, 128]
SWEEP_TQ = [1, 64, 127, 128, 129, 191, 192, 193, 320, 640, 1024, 1280, 1296, 1536, 2560, 3328]
SWEEP_TK = [64, 100, 1024, 1280]
SWEEP_CUS = [8, 64, 256, 304]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    from mlx_video_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    from mlx_video_amd import ops
    return ops


def fields(pl):
    return (pl.kernel, pl.tiles_192, pl.tiles_128, pl.whole_workgroups, pl.split_tiles, pl.workgroups, pl.xcd_order)


# ---- the launcher's rules as they were before fa_form, restated: the greedy goes CU by CU, one 128-row workgroup at a time ----
@functools.lru_cache(maxsize=None)
def ref_pick_mix(Tq, Tk, BH, cus):
    cus = min(cus, 1024)
    fixed = 8 * 128 * 128 // max(Tk, 128)
    ca, cb = 192 * 7 + fixed, 128 * 8 + fixed
    best = None
    for nb in range(7):
        rest = Tq - 128 * nb
        if rest <= -128:
            break
        na = (rest + 191) // 192 if rest > 0 else 0
        wa, wb = na * BH, nb * BH
        load = np.array([(wa // cus + (1 if c < wa % cus else 0)) * ca for c in range(cus)], dtype=np.int64)
        for _ in range(wb):
            load[int(np.argmin(load))] += cb            # the first least-loaded CU
        span = int(load.max())
        if best is None or span < best[0]:
            best = (span, na, nb)
    return best[1], best[2]


def ref_plan(BH, Tq, Tk, cus, flags):
    slots = 2 * cus
    QT = (Tq + 127) // 128
    xcd = 1 if BH % 8 == 0 else 0
    tiles = QT * BH
    n_full, rem = tiles, 0
    if not (flags & NO_TAIL_SPLIT) and tiles % slots != 0:
        r = tiles % slots
        rem = r if 2 * r <= slots else slots - r
        n_full = tiles - rem
    if Tq > 128 and 4 * tiles >= 5 * slots:
        qta, qtb = ref_pick_mix(Tq, Tk, BH, cus)
        return (MIX, qta, qtb, (qta + qtb) * BH, 0, (qta + qtb) * BH, xcd)
    return (K128, 0, QT, n_full, rem, n_full + 2 * rem, xcd)


def test_attn_plan_abi(ops):
    from mlx_video_amd import _lib
    lib = _lib.load()
    assert lib.ltxk_flash_attn_plan_sizeof() == ctypes.sizeof(_lib.AttnPlan) == 32
    assert lib.ltxk_version() >= 407
    assert (_lib.ATTN_KERNEL_128, _lib.ATTN_KERNEL_MIX) == (K128, MIX) and _lib.ATTN_NO_TAIL_SPLIT == NO_TAIL_SPLIT


@pytest.mark.parametrize("case", TABLE, ids=lambda c: "-".join(map(str, c[:6])))
def test_fixed_table(ops, case):
    B, H, Tq, Tk, cus, flags = case[:6]
    pl = ops.flash_attn_plan(B, H, Tq, Tk, cus=cus, tail_split=not flags)
    assert fields(pl) == case[6:], pl
    assert pl.mfma_k == 16
    assert ref_plan(B * H, Tq, Tk, cus, flags) == case[6:]           # the restatement below is swept against says the same
    assert ops.flash_attn_plan(B, H, Tq, Tk, cus=cus, tail_split=not flags, fused_q=H % 4 == 0) == pl


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "-".join(map(str, c[:5])))
def test_gpu_test_cases_at_256_cus(ops, case):
    """The forms tests/test_attn_forms_gpu.py expects, by the plan and by the restatement; short keys (Tk = 128, 136) take the
    (192-row, 128-row) mix of the square shapes 1280^2 and 1296^2."""
    B, H, Tq, Tk, ts = case[:5]
    assert fields(ops.flash_attn_plan(B, H, Tq, Tk, cus=256, tail_split=ts)) == case[5:]
    assert ref_plan(B * H, Tq, Tk, 256, 0 if ts else NO_TAIL_SPLIT) == case[5:]
    if case[5] == MIX:
        assert ref_pick_mix(Tq, Tk, B * H, 256) == ref_pick_mix(Tq, Tq, B * H, 256)


def test_sweep_against_restatement_and_invariants(ops):
    kinds = {K128: 0, MIX: 0}
    splits = 0
    for BH in SWEEP_BH:
        for Tq in SWEEP_TQ:
            for Tk in SWEEP_TK:
                for cus in SWEEP_CUS:
                    got = {}
                    for flags in (0, NO_TAIL_SPLIT):
                        pl = ops.flash_attn_plan(1, BH, Tq, Tk, cus=cus, tail_split=not flags)
                        where = f"BH={BH} Tq={Tq} Tk={Tk} cus={cus} flags={flags}: {pl}"
                        assert fields(pl) == ref_plan(BH, Tq, Tk, cus, flags), where
                        assert pl.mfma_k == 16, where
                        assert pl.workgroups == pl.whole_workgroups + 2 * pl.split_tiles, where
                        if pl.mix:
                            assert pl.split_tiles == 0 and 192 * pl.tiles_192 + 128 * pl.tiles_128 >= Tq, where
                            assert pl.whole_workgroups == (pl.tiles_192 + pl.tiles_128) * BH, where
                        else:
                            assert pl.tiles_192 == 0 and (pl.tiles_128 - 1) * 128 < Tq <= pl.tiles_128 * 128, where
                            assert pl.whole_workgroups + pl.split_tiles == pl.tiles_128 * BH, where
                        if flags:
                            assert pl.split_tiles == 0, where
                        got[flags] = pl
                        kinds[pl.kernel] += 1
                        splits += pl.split_tiles > 0
                    if got[0].mix or got[NO_TAIL_SPLIT].mix:
                        assert got[0] == got[NO_TAIL_SPLIT], (BH, Tq, Tk, cus)
    assert kinds[MIX] > 300 and kinds[K128] > 300 and splits > 300, (kinds, splits)      # the sweep reaches every form


def _args(_lib, B=1, H=4, Tq=200, Tk=70):
    a = _lib.AttnArgs()
    a.q = a.k = a.vt = a.out = A
    a.ldq = a.ldk = a.ldo = H * 128
    a.ldvt = (Tk + 63) // 64 * 64
    a.B, a.H, a.Tq, a.Tk, a.scale = B, H, Tq, Tk, 0.125
    return a


def test_plan_refuses_what_the_launch_refuses(ops):
    """Every refusal carries LTXK_EINVAL and the launch's own message.  The launch runs the same checks before it touches the
    device, so on a machine without one it refuses the same arguments with the same words."""
    from mlx_video_amd import _lib
    from mlx_video_amd._lib import LtxkError
    lib = _lib.load()

    def refused(a, cus=256):
        pl = _lib.AttnPlan()
        rc = lib.ltxk_flash_attn_plan(ctypes.byref(a) if a is not None else None, cus, ctypes.byref(pl))
        msg = lib.ltxk_last_error().decode()
        assert rc == -1, (rc, msg)
        if cus > 0:                                       # the launch takes its CU count from the device
            assert lib.ltxk_flash_attn(ctypes.byref(a) if a is not None else None, None) == -1
            assert lib.ltxk_last_error().decode() == msg
        return msg

    assert refused(None) == "ltxk_flash_attn: null args"
    a = _args(_lib); a.vt = None
    assert refused(a) == "ltxk_flash_attn_bf16: null pointer"
    a = _args(_lib); a.out = A + 8
    assert refused(a) == "ltxk_flash_attn_bf16: misaligned pointer"
    a = _args(_lib, Tk=70); a.ldvt = 120
    assert refused(a) == "ltxk_flash_attn_bf16: ldvt=120 must be >= 128 (Tk rounded up to 64) and a multiple of 8"
    a = _args(_lib); a.ldk = 4 * 128 + 4
    assert refused(a) == "ltxk_flash_attn_bf16: row strides must be multiples of 8"
    a = _args(_lib); a.ldq = 4 * 128 - 8
    assert refused(a) == "ltxk_flash_attn_bf16: row strides < H*128"
    a = _args(_lib); a.Tq = 0
    assert refused(a) == "ltxk_flash_attn_bf16: bad dims"
    a = _args(_lib); a.q_sumsq, a.q_sumsq_ld, a.q_sumsq_n = A, 8, 8
    assert refused(a) == "ltxk_flash_attn: q_sumsq needs q_norm_weight"
    a.q_norm_weight, a.q_sumsq_n = A, 4
    assert "q_sumsq_n=4 must equal H*128/64" in refused(a)
    a.q_sumsq_n, a.cos = 8, A
    assert "cos and sin must both be set" in refused(a)
    assert "cus=0 must be positive" in refused(_args(_lib), cus=0)
    assert "cus=-3 must be positive" in refused(_args(_lib), cus=-3)
    pl = _lib.AttnPlan()
    assert lib.ltxk_flash_attn_plan(ctypes.byref(_args(_lib)), 256, None) == -1
    assert lib.ltxk_flash_attn_plan(ctypes.byref(_args(_lib)), 256, ctypes.byref(pl)) == 0      # ... and the untouched args pass
    with pytest.raises(LtxkError, match="bad dims"):
        ops.flash_attn_plan(1, 4, 0, 64, cus=256)
    with pytest.raises(LtxkError, match="cus=0"):
        ops.flash_attn_plan(1, 4, 128, 64, cus=0)


def test_attn_bound_cases_at_256_cus(ops, monkeypatch):
    """The forms tests/test_attn_bound_gpu.py aims its cases at, by the plan and by the restatement, and the plans its
    measurement-build switches produce (each switch must change the plan of the shape it is tried at)."""
    import test_attn_bound_gpu as G
    from mlx_video_amd import _lib

    def want_of(pl, want):
        return {k: getattr(pl, k) for k in want}

    checked = [(shape, ts, want, False) for _, shape, _, variants in G.CASES for ts, want in variants]
    checked += [(shape, ts, want, True) for _, shape, ts, want in G.FUSED_CASES]
    for shape, ts, want, fused in checked:
        B, H, Tq, Tk = shape
        pl = ops.flash_attn_plan(B, H, Tq, Tk, cus=256, tail_split=ts, fused_q=fused)
        assert want_of(pl, want) == want, (shape, ts, pl)
        assert fields(pl) == ref_plan(B * H, Tq, Tk, 256, 0 if ts else NO_TAIL_SPLIT), (shape, ts, pl)
    for var in ("LTXK_FA_MFMA", "LTXK_FA_QB", "LTXK_FA_XCD", "LTXK_FA_FILL"):
        monkeypatch.delenv(var, raising=False)
    if not os.path.exists(_lib.AB_LIB_PATH):
        pytest.skip("no measurement build")
    with _lib.use_library(_lib.AB_LIB_PATH):
        for var, val, shape, want in G.AB_CASES:
            base = ops.flash_attn_plan(*shape, cus=256)
            assert want_of(base, G.AB_DEFAULT.get(shape, {})) == G.AB_DEFAULT.get(shape, {}), (shape, base)
            monkeypatch.setenv(var, val)
            pl = ops.flash_attn_plan(*shape, cus=256)
            monkeypatch.delenv(var)
            assert want_of(pl, want) == want and pl != base, (var, val, shape, pl, base)
