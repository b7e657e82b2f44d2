"""The step cache's kernels on the device (csrc/step_cache.hip): ltxk_step_cache_probe against the numpy float32 emulation of
its documented summation order (tests/ref_step_cache.py) - bit for bit - and against the float64 sums inside
gamma_(depth + 1) * sum |t_i|; ltxk_residual_store / ltxk_residual_apply against (a.float() -/+ b.float()).bfloat16(), bit
for bit.  Every buffer the kernels write lies between NaN sentinel rows that must stay intact.

Shapes (rows, D), one chunk = 8192 elements: below one chunk (1 x 512), exactly one chunk (2 x 4096, 16 x 512), one chunk plus
one 8-element vector (1025 x 8), three chunks with a ragged last one (5 x 4096, 10 x 2048), 130 x 512 = 8.125 chunks, and the
rest of D in {512, 2048, 4096} x rows in {1, 5, 130}."""
import numpy as np
import pytest
import torch

import ref_step_cache as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = [(1, 512), (2, 4096), (16, 512), (1025, 8), (5, 4096), (10, 2048), (130, 512), (1, 2048), (1, 4096), (5, 512), (5, 2048),
          (130, 2048), (130, 4096)]
NAN_BF16 = 0x7FC1                    # a quiet NaN with a payload, as int16
NAN_F32 = 0x7FC00123


def _values(kind, rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    spread = lambda: (torch.randn(rows, D, generator=g) * torch.exp2(torch.randint(-12, 9, (rows, D), generator=g).float())).to(BF)
    cur, prev = spread(), spread()
    if kind == "equal":
        prev = cur.clone()
    elif kind == "prev_zero":
        prev = torch.zeros_like(cur)
    elif kind == "negative_zeros":
        prev = torch.where(torch.rand(rows, D, generator=g) < 0.5, torch.full_like(cur, -0.0), prev)
        cur = torch.where(torch.rand(rows, D, generator=g) < 0.5, torch.full_like(cur, -0.0), cur)
    return cur, prev


class _Guarded:
    """A device buffer of ``n`` elements between two sentinel rows of NaNs with a payload."""

    def __init__(self, n, dtype, dev, pad=64):
        self.pad, self.n = pad, n
        self.int_dtype, self.nan = (torch.int16, NAN_BF16) if dtype == BF else (torch.int32, NAN_F32)
        self.buf = torch.full((n + 2 * pad,), self.nan, dtype=self.int_dtype, device=dev).view(dtype)

    @property
    def body(self):
        return self.buf[self.pad:self.pad + self.n]

    def intact(self):
        raw = self.buf.view(self.int_dtype)
        return bool((raw[:self.pad] == self.nan).all()) and bool((raw[self.pad + self.n:] == self.nan).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _probe(dev, cur, prev, init=False):
    from mlx_video_amd import ops
    rows, D = cur.shape
    gp = _Guarded(rows * D, BF, dev)            # 64 bf16 of padding = 128 bytes: the body stays 16-byte aligned
    gs = _Guarded(2, torch.float32, dev)
    gw = _Guarded(ops.step_cache_workspace_bytes(rows, D) // 4, torch.float32, dev)
    assert gp.body.data_ptr() % 16 == 0
    gp.body.copy_(prev.reshape(-1))
    pv = gp.body.view(rows, D)
    ops.step_cache_probe(cur.to(dev), pv, gs.body, gw.body, init=init)
    torch.cuda.synchronize()
    assert gp.intact() and gs.intact() and gw.intact(), "a sentinel row was overwritten"
    return pv.cpu(), gs.body.cpu(), gw


@pytest.mark.parametrize("rows,D", SHAPES, ids=[f"{r}x{d}" for r, d in SHAPES])
@pytest.mark.parametrize("kind", ["spread", "equal", "prev_zero", "negative_zeros"])
def test_probe_sums_have_the_documented_order(dev, rows, D, kind):
    from mlx_video_amd import _lib, ops
    lib = _lib.load()
    assert ops.step_cache_workspace_bytes(rows, D) == 8 * R.chunks(rows * D) == lib.ltxk_step_cache_workspace_bytes(rows, D)
    assert ops.step_cache_depth(rows, D) == R.depth(rows, D) == lib.ltxk_step_cache_depth(rows, D)
    cur, prev = _values(kind, rows, D, seed=rows * 131 + D)
    (e_d, e_p), (d64, p64), (b_d, b_p) = R.probe_emulation(cur, prev)
    new_prev, sums, _ = _probe(dev, cur, prev)
    got_d, got_p = (np.float32(x) for x in sums.tolist())
    print(f"{rows}x{D} {kind}: S_d {got_d!r} (float64 {d64!r}, bound {b_d:.3e}), S_p {got_p!r} (float64 {p64!r}, bound {b_p:.3e})")
    assert torch.equal(_bits(new_prev), _bits(cur)), "prev is not a copy of cur"
    assert got_d.tobytes() == e_d.tobytes() and got_p.tobytes() == e_p.tobytes(), "the sums are not the emulation's bits"
    assert abs(float(got_d) - d64) <= b_d and abs(float(got_p) - p64) <= b_p
    if kind == "equal":
        assert float(got_d) == 0.0
    if kind == "prev_zero":
        assert float(got_p) == 0.0
    again = _probe(dev, cur, prev)
    assert torch.equal(_bits(again[1]), _bits(sums)) and torch.equal(_bits(again[0]), _bits(new_prev)), "two runs differ"


def test_probe_init_copies_and_leaves_the_sums_alone(dev):
    from mlx_video_amd import ops
    rows, D = 5, 4096
    cur, prev = _values("spread", rows, D, seed=3)
    new_prev, sums, gw = _probe(dev, cur, prev, init=True)
    assert torch.equal(_bits(new_prev), _bits(cur))
    assert bool((_bits(sums) == NAN_F32).all()) and bool((gw.body.view(torch.int32) == NAN_F32).all()), "INIT touched sums or the workspace"
    p2 = prev.to(dev)
    ops.step_cache_probe(cur.to(dev), p2, None, None, init=True)          # neither is needed
    torch.cuda.synchronize()
    assert torch.equal(_bits(p2.cpu()), _bits(cur))


def test_probe_carries_a_nan_into_the_sums(dev):
    """A NaN in the measure reaches the host as a sum that is not finite: the policy then computes the step."""
    cur, prev = _values("spread", 5, 512, seed=5)
    prev[3, 17] = float("nan")
    _, sums, _ = _probe(dev, cur, prev)
    assert not np.isfinite(sums.numpy()).any()


def test_overlapping_buffers_are_refused_before_any_launch(dev):
    """The kernels take their two buffers as __restrict__: the library refuses buffers that share a byte, not only equal ones."""
    from mlx_video_amd import _lib, ops
    buf = torch.ones((6, 512), dtype=BF, device=dev)
    sums, ws = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    with pytest.raises(_lib.LtxkError, match="overlapping"):
        ops.step_cache_probe(buf[:5], buf[1:], sums, ws)
    for fn in (ops.residual_store, ops.residual_apply):
        with pytest.raises(_lib.LtxkError, match="overlapping"):
            fn(buf[:5], buf[1:])
        with pytest.raises(ValueError, match="two buffers"):
            fn(buf, buf)
    torch.cuda.synchronize()
    assert bool((buf == 1).all()) and not bool(sums.any())


COUNTS = [8, 8 * 257, 5 * 512, 2048 + 8, 3 * 2048 + 1032]       # one workgroup takes 256 vectors = 2048 elements


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("op", ["store", "apply"])
def test_residual_arithmetic_bit_for_bit(dev, n, op):
    from mlx_video_amd import ops
    g = torch.Generator().manual_seed(n)
    spread = lambda: (torch.randn(n, generator=g) * torch.exp2(torch.randint(-10, 6, (n,), generator=g).float())).to(BF)
    a, b = spread(), spread()
    b[::7] = a[::7]                                  # exact cancellation under store
    a[3], b[5] = -0.0, -0.0
    gx, gr = _Guarded(n, BF, dev), _Guarded(n, BF, dev)
    gx.body.copy_(a)
    gr.body.copy_(b)
    if op == "store":
        ops.residual_store(gx.body, gr.body)
        want_x, want_r = a, (a.float() - b.float()).to(BF)
    else:
        ops.residual_apply(gx.body, gr.body)
        want_x, want_r = (a.float() + b.float()).to(BF), b
    torch.cuda.synchronize()
    assert gx.intact() and gr.intact(), "a sentinel row was overwritten"
    assert torch.equal(_bits(gx.body.cpu()), _bits(want_x)) and torch.equal(_bits(gr.body.cpu()), _bits(want_r))
