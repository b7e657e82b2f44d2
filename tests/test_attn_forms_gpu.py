"""Flash attention in each of its launch forms, at the smallest shape that takes the form on an MI355X (256 CUs): each case
asserts its plan (ops.flash_attn_plan at the device's own CU count - the function the launch itself decides by; the rules are
pinned in tests/test_attn_plan_cpu.py), then holds the launch to test_kernels_gpu.py::test_flash_attn's two tolerances against
the oracle, and the fused query preparation to the two-launch form as test_attention_with_fused_query_prep does."""
import math

import parity
import pytest
import torch

from oracle import dit as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
K128, MIX = 0, 1

# form, (B, H, Tq, Tk), tail_split, expected plan fields
CASES = [
    ("split_all_tail", (1, 3, 200, 70), True, dict(kernel=K128, whole_workgroups=0, split_tiles=6, workgroups=12)),
    # (the fused query preparation needs H % 4 == 0: the same form at the next head count that has one)
    ("split_all_tail_h4", (1, 4, 200, 70), True, dict(kernel=K128, whole_workgroups=0, split_tiles=8, workgroups=16)),
    ("fill_rule_tail", (1, 32, 1280, 128), True, dict(kernel=K128, whole_workgroups=128, split_tiles=192, workgroups=512)),
    ("whole_rounds_plus_tail", (2, 32, 640, 128), True, dict(kernel=K128, whole_workgroups=128, split_tiles=192, workgroups=512)),
    ("no_split_by_flag", (1, 32, 1280, 128), False, dict(kernel=K128, whole_workgroups=320, split_tiles=0, workgroups=320)),
    ("mixed_grid", (2, 32, 1280, 128), True, dict(kernel=MIX, tiles_192=4, tiles_128=4, split_tiles=0, workgroups=512)),
    ("mixed_grid_ragged_tq", (2, 32, 1296, 136), True, dict(kernel=MIX, tiles_192=7, tiles_128=0, split_tiles=0, workgroups=448)),
]


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("form,shape,tail_split,want", CASES, ids=[c[0] for c in CASES])
def test_attention_launch_form(dev, form, shape, tail_split, want):
    from mlx_video_amd import ops
    from mlx_video_amd._lib import LtxkError
    B, H, Tq, Tk = shape
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if cus != 256:
        pytest.skip(f"the expected plans are those of a 256-CU device; this one has {cus}")
    fused_ok = H % 4 == 0
    pl = ops.flash_attn_plan(B, H, Tq, Tk, cus=cus, tail_split=tail_split)
    assert {k: getattr(pl, k) for k in want} == want, pl
    assert pl.mfma_k == 16
    if fused_ok:
        assert ops.flash_attn_plan(B, H, Tq, Tk, cus=cus, tail_split=tail_split, fused_q=True) == pl

    D = H * 128
    sc = 1.0 / math.sqrt(128)
    g = torch.Generator().manual_seed(B * 100 + Tq + Tk)
    q = torch.randn(B, Tq, D, generator=g).to(BF)
    k = torch.randn(B, Tk, D, generator=g).to(BF)
    v = torch.randn(B, Tk, D, generator=g).to(BF)
    w = (1 + 0.1 * torch.randn(1, D, generator=g)).to(BF)
    ang = torch.rand(H, Tq, 64, generator=g) * (2 * math.pi)
    vt = torch.zeros(B, D, (Tk + 63) // 64 * 64, dtype=BF)
    vt[:, :, :Tk] = v.transpose(1, 2)
    qd, kd, vtd = q.reshape(B * Tq, D).to(dev), k.reshape(B * Tk, D).to(dev), vt.to(dev)
    out = torch.full((B * Tq + 1, D), 7.0, dtype=BF, device=dev)
    ops.flash_attn(qd, kd, vtd, out[:B * Tq], B, H, Tq, Tk, sc, tail_split=tail_split)
    torch.cuda.synchronize()
    assert bool((out[B * Tq:] == 7.0).all()), "wrote past the last query row"
    got = out[:B * Tq].reshape(B, Tq, D)
    # test_flash_attn's tolerances: P rounded to bf16 before P.V against the oracle's fp32 P (1e-2), and against the "flash"
    # policy, which rounds P where the kernel does - fp32 summation order and final-rounding flips only (5e-4)
    parity.auto(rel_l2(got, O.sdpa(q.float(), k.float(), v.float(), H, O.BF16)), 1e-2)
    parity.auto(rel_l2(got, O.sdpa(q.float(), k.float(), v.float(), H, O.BF16_FLASH)), 5e-4, tag="vs_flash_policy")

    # fused query preparation (q_norm + SPLIT RoPE on the Q fragments) against qknorm_rope followed by the plain launch
    ss = (q.float() ** 2).reshape(B * Tq, D // 64, 64).sum(-1).to(dev)
    cd, sd = torch.cos(ang).contiguous().to(dev), torch.sin(ang).contiguous().to(dev)
    fused = torch.empty(B * Tq, D, dtype=BF, device=dev)
    kw = dict(q_sumsq=ss, q_norm_weight=w.to(dev), cos=cd, sin=sd, eps=1e-6, tail_split=tail_split)
    if not fused_ok:
        with pytest.raises(LtxkError, match="q_sumsq_n"):
            ops.flash_attn(qd, kd, vtd, fused, B, H, Tq, Tk, sc, **kw)
        return
    ops.flash_attn(qd, kd, vtd, fused, B, H, Tq, Tk, sc, **kw)
    qn = qd.clone()
    ops.qknorm_rope(qn, 1, D, w.to(dev), cd, sd, Tq, H, 1e-6)
    two = torch.empty(B * Tq, D, dtype=BF, device=dev)
    ops.flash_attn(qn, kd, vtd, two, B, H, Tq, Tk, sc, tail_split=tail_split)
    torch.cuda.synchronize()
    # same op order and rounding points; only the fp32 order of the row's sum of squares differs (1-ulp flips of rstd)
    assert rel_l2(fused, two) < 2e-3, rel_l2(fused, two)
