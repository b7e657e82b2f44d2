"""torch.Tensor -> libltxk C-ABI call shims.  One function per entry point of include/ltxk.h.
Tensors carry device memory only; all math happens in the HIP kernels.  Every call is queued
on torch's current HIP stream (so a torch.cuda.graph capture records the whole step).

The boundary has one rule.  A shim first refuses the argument pairings that need no tensor (a scale without its shift, an
unknown guider), then hands EVERY tensor operand - outputs, tables and scratch included - to ``_operands``, which checks
per tensor dtype, shape, layout and alignment and, last, the device; only then is anything allocated or launched.  Sizes
come from the tensors: an integer a tensor already determines (``ada_combine``'s L,U,K,D, ``flash_attn``'s B,H,Tq,Tk) is
compared with it and a mismatch refused.  TypeError: dtype; ValueError: shape, layout, alignment; LtxkError: the device."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

from . import _lib
from ._lib import AttnArgs, CausalAttnArgs, Conv3dArgs, ConvTapsArgs, GemmArgs, GemmGroupedArgs, GuiderArgs, SampleArgs, StepArgs, check
from .weights import MXFP4_BLOCK          # k per e8m0 block scale

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU, EPI_BIAS_GATE_RES, EPI_BIAS_RES, EPI_SCALE_RES = 0, 1, 2, 3, 4, 5
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
F32, I32 = torch.float32, torch.int32


class KernelTimer:
    """Optional per-launch HIP-event timing (bench.py roofline leg).  Events are recorded on the
    stream the kernels are launched on; nothing is synchronised until ``summary()``."""

    def __init__(self):
        self.records = []       # (family, algorithmic flops, algorithmic bytes, start, end)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for fam, flops, nbytes, s, e in self.records:
            d = out.setdefault(fam, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


TIMER: Optional[KernelTimer] = None


class _timed:
    __slots__ = ("fam", "flops", "nbytes", "s")

    def __init__(self, fam, flops=0.0, nbytes=0.0):
        self.fam, self.flops, self.nbytes = fam, flops, nbytes

    def __enter__(self):
        if TIMER is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *a):
        if TIMER is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            TIMER.records.append((self.fam, self.flops, self.nbytes, self.s, e))


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dims(who: str, name: str, t: torch.Tensor, dtype, rank: int) -> torch.Size:
    """``t.shape`` once its dtype and rank hold: the first two checks of ``_operands``, on their own for the operand a
    shim derives its sizes from."""
    sh = t.shape
    if t.dtype != dtype:
        raise TypeError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    if len(sh) != rank:
        raise ValueError(f"{who}: {name} must have {rank} dimensions, got shape {tuple(sh)}")
    return sh


def _dense_rows(t: torch.Tensor, sh, k=True) -> bool:
    """(..., n, C) rows of a (..., n, ld >= C) buffer with unit inner stride (``sh``: t.shape).  ``k`` True: one leading
    dimension, the outer dimensions dense; an int: outer strides of their own, each a multiple of k elements (a layer or
    group stack)."""
    st = t.stride()
    n = len(st)
    if n < 2 or st[-1] != 1 or st[-2] < sh[-1]:
        return False
    if k is not True:
        return not any(s % k for s in st[:-1])
    return n == 2 or all(st[i] == st[i + 1] * sh[i + 1] for i in range(n - 2))


def _operands(who: str, *operands) -> None:
    """The one operand check of every shim.  An operand is ``(name, tensor or None, dtype, shape, align)``: ``shape`` the
    exact shape the call derives - an int: the rank alone; a negative entry ``-n``: at least n along that dimension (``sumsq``
    (M, >= cols/64), V^T (B, D, ld >= T)) - and ``align`` the byte alignment the C entry or its kernel's vector accesses
    demand (up to 4 bytes it is the element's own, which torch guarantees, and is not looked at).  The tensor is contiguous
    unless a sixth item allows more (``_dense_rows``): ``True`` a leading dimension, an int k outer strides of their own that
    are multiples of k elements.  Per tensor: dtype, shape, layout, alignment - and only when every operand has passed those,
    the device, so that each of the other refusals shows on CPU tensors too.  Nothing is launched on a tensor it refuses.
    One compound test per operand on the way through (this runs in front of every launch, and a forward of small launches
    waits for it: each tensor property is read once, a minimum in the last dimension alone - the common one - has a
    comparison of its own in front of the general one); ``_refuse`` words the error."""
    host = None
    for op in operands:
        t = op[1]
        if t is None:
            continue
        shape, sh = op[3], t.shape
        if t.dtype != op[2] or (len(sh) != shape if shape.__class__ is int else sh != shape and (
                (shape[-1] >= 0 or sh[:-1] != shape[:-1] or sh[-1] < -shape[-1]) and
                (len(sh) != len(shape) or any(s != n if n >= 0 else s < -n for s, n in zip(sh, shape))))) or \
                not (t.is_contiguous() or len(op) > 5 and _dense_rows(t, sh, op[5])) or (op[4] > 4 and t.data_ptr() % op[4]):
            _refuse(who, *op)
        if host is None and not t.is_cuda:
            host = op[0]
    if host is not None:
        raise _lib.LtxkError(f"{who}: {host} must be a device tensor (the product path has no CPU fallback)")


def _refuse(who: str, name: str, t: torch.Tensor, dtype, shape, align: int, ld=False) -> None:
    """Raises for the first of ``_operands``' per-tensor checks that ``t`` fails, in their order."""
    exact = not isinstance(shape, int)
    _dims(who, name, t, dtype, len(shape) if exact else shape)
    if exact and any(s != n if n >= 0 else s < -n for s, n in zip(t.shape, shape)):
        want = ", ".join(str(n) if n >= 0 else f">={-n}" for n in shape)
        raise ValueError(f"{who}: {name} must be ({want}{',' if len(shape) == 1 else ''}), got {tuple(t.shape)}")
    if not (t.is_contiguous() or ld and _dense_rows(t, t.shape, ld)):
        how = "contiguous" if ld is False else "rows with unit inner stride" if ld is True else \
            f"rows with unit inner stride, outer strides multiples of {ld}"
        raise ValueError(f"{who}: {name} must be {how}, got shape {tuple(t.shape)} with strides {t.stride()}")
    raise ValueError(f"{who}: {name} must be {align}-byte aligned")


def _table(who: str, name: str, t: Optional[torch.Tensor], D: int, stride: int) -> tuple:
    """The shape item of a table read as p[row * stride + d] (modulation, gate): (its own rows, D), once a view of more than
    one row has them ``stride`` elements apart."""
    if t is None or t.dim() != 2:
        return (-1, D)
    if t.stride(0) != stride and t.shape[0] > 1:
        raise ValueError(f"{who}: the rows of {name} lie {t.stride(0)} elements apart, the stride passed for it is {stride}")
    return (t.shape[0], D)


GEMM_WORKSPACE_BYTES = 64 << 20
SPLITK_WORKSPACE_BYTES = 96 << 20
SPLITK_MAX_M = 640          # rows up to which a launch is offered the split-K scratch (the library decides; gemm.hip)
# purpose -> (elements, dtype, constructor) of the per-device buffers the library is handed and never allocates itself
_SCRATCH_KINDS = {"gemm_splitk": (GEMM_WORKSPACE_BYTES // 4, torch.float32, torch.empty),        # ltxk_gemm_bf16 at small M
                  "conv_splitk": (SPLITK_WORKSPACE_BYTES // 4, torch.float32, torch.empty),      # ltxk_conv3d_k3_bf16
                  "zero_page": (256, torch.uint8, torch.zeros)}                                  # the conv's zero-padding halo
_SCRATCH = {}


def _scratch(purpose: str, dev: torch.device) -> torch.Tensor:
    """The per-device buffer of one purpose (_SCRATCH_KINDS): caller-owned and reused by every call on the stream - launches
    on one stream are ordered."""
    key = (purpose, dev.index if dev.index is not None else 0)
    buf = _SCRATCH.get(key)
    if buf is None:
        n, dtype, make = _SCRATCH_KINDS[purpose]
        buf = _SCRATCH[key] = make(n, dtype=dtype, device=dev)
    return buf


def _offers_workspace(M: int, split_k: bool) -> bool:
    return split_k and M <= SPLITK_MAX_M


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], *, epilogue: int = EPI_BIAS,
         out: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
         gate: Optional[torch.Tensor] = None, gate_row: Optional[torch.Tensor] = None,
         gate_stride: int = 0, out_tokens_per_batch: int = 0, alpha: float = 1.0,
         out2: Optional[torch.Tensor] = None, n_split: int = 0, sumsq: Optional[torch.Tensor] = None,
         split_k: bool = True, w_scale: Optional[torch.Tensor] = None,
         a_scale: Optional[torch.Tensor] = None, gemv: bool = False) -> torch.Tensor:
    """out = epi(a @ w.T + bias).  a (M,K) (row stride may exceed K), w (N,K) contiguous, bias (N); out / resid (M,N) rows,
    gate (rows,N) read as gate[gate_row[m] * gate_stride + n] with gate_row (M) int32.
    ``w`` may be ``torch.float8_e4m3fn`` (ltxk_gemm_w8: the panel is read as fp8 and widened in registers; with no ``w_scale``
    the result equals the bf16 call on ``w.to(bfloat16)`` bit for bit); ``w_scale`` (N) fp32 then multiplies the accumulator
    per output channel before the bias.  A bf16 ``w`` takes ltxk_gemm_bf16 and no ``w_scale``.
    ``out_tokens_per_batch`` = T: ``out`` is (M/T, N, ld >= T), written transposed per batch.  ``n_split``/``out2``: ``out`` is
    (M, n_split) and columns >= n_split go transposed to out2 (M/T, N-n_split, ld >= T).  ``sumsq``: (M, >= cols/64) fp32,
    receives the per-64-column sums of squares of the stored row-major outputs.  ``split_k=False``: no split-K scratch is
    offered, so the launch is single-pass (or big-tile) and a row's bits do not depend on M; with it the library may split K
    at M <= SPLITK_MAX_M (``gemm_plan`` tells).
    A ``float8_e4m3fn`` ``a`` together with ``a_scale`` (M) fp32 - what ``quant_rows_fp8`` returns - takes ltxk_gemm_w8a8: fp8
    operands on the fp8 matrix pipe, acc * a_scale[m] * w_scale[n] in front of the bias.  It needs an fp8 ``w``, K % 128 == 0
    and 16-byte aligned rows of ``a``; it is always single-pass (``split_k`` is ignored).
    ``gemv=True`` takes ltxk_gemv_w8, the weight stream of a decode step: a float8_e4m3fn ``w``, M <= GEMV_MAX_M rows,
    K % 16 == 0, any N, EPI_BIAS with or without ``bias`` / ``w_scale``, and none of the other outputs or operands.  One launch,
    no workspace (``split_k`` is ignored); a row's bits depend on that row, the panel row, its scale and its bias alone."""
    if gemv:
        return _gemv(a, w, bias, epilogue, out, w_scale, resid=resid, gate=gate, gate_row=gate_row, out2=out2, sumsq=sumsq,
                     a_scale=a_scale, n_split=n_split, out_tokens_per_batch=out_tokens_per_batch)
    w8 = w.dtype == FP8
    a8 = a.dtype == FP8
    if a8 != (a_scale is not None):
        raise TypeError("gemm: a float8_e4m3fn `a` and `a_scale` go together (quant_rows_fp8 gives both)")
    if a8 and not w8:
        raise TypeError(f"gemm: float8_e4m3fn activations need a float8_e4m3fn weight, got {w.dtype}")
    if w_scale is not None and not w8:
        raise TypeError("gemm: w_scale goes with a float8_e4m3fn weight")
    if n_split and out2 is None:
        raise ValueError("gemm: split output needs a bf16 `out2`")
    if out is None and out_tokens_per_batch:
        raise ValueError("gemm: transposed output needs a preallocated `out`")
    if not n_split:
        out2 = None
    adt, wdt, T = FP8 if a8 else BF16, FP8 if w8 else BF16, out_tokens_per_batch
    M, K = _dims("gemm", "a", a, adt, 2)
    N = _dims("gemm", "w", w, wdt, 2)[0]
    cols, nb = n_split or N, M // T if T else 0
    _operands("gemm", ("a", a, adt, 2, 16, True), ("w", w, wdt, (N, K), 16), ("bias", bias, BF16, (N,), 8),
              ("out", out, BF16, (nb, N, -T) if T and not n_split else (M, cols), 8, True), ("resid", resid, BF16, (M, N), 8, True),
              ("gate", gate, BF16, _table("gemm", "gate", gate, N, gate_stride), 8, True), ("gate_row", gate_row, I32, (M,), 4),
              ("out2", out2, BF16, (nb, N - n_split, -T), 8, True), ("sumsq", sumsq, F32, (M, -(cols // 64)), 4, True),
              ("w_scale", w_scale, F32, (N,), 4), ("a_scale", a_scale, F32, (M,), 4))
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    args = GemmArgs()
    args.A, args.W, args.bias, args.out = _p(a), _p(w), _p(bias), _p(out)
    args.resid, args.gate, args.gate_row = _p(resid), _p(gate), _p(gate_row)
    args.M, args.N, args.K = M, N, K
    args.lda = a.stride(0)
    args.ldo = out.stride(-2)
    args.ldr = resid.stride(0) if resid is not None else 0
    args.gate_stride = gate_stride
    args.epilogue = epilogue
    args.out_tokens_per_batch = out_tokens_per_batch
    args.alpha = alpha
    args.out2, args.n_split, args.ldo2 = _p(out2), n_split, (out2.stride(-2) if out2 is not None else 0)
    args.sumsq, args.sumsq_ld = _p(sumsq), (sumsq.stride(0) if sumsq is not None else 0)
    if a8:
        with _timed("gemm_w8a8", 2.0 * M * N * K, 1.0 * (M * K + N * K) + 2.0 * M * N):
            check(_lib.load().ltxk_gemm_w8a8(ctypes.byref(args), _p(a_scale), _p(w_scale), _stream()), "ltxk_gemm_w8a8")
        return out
    if _offers_workspace(M, split_k):
        ws = _scratch("gemm_splitk", a.device)
        args.workspace, args.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    if w8:
        with _timed("gemm_w8", 2.0 * M * N * K, 2.0 * (M * K + M * N) + 1.0 * N * K):
            check(_lib.load().ltxk_gemm_w8(ctypes.byref(args), _p(w_scale), _stream()), "ltxk_gemm_w8")
        return out
    with _timed("gemm_bf16", 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)):
        check(_lib.load().ltxk_gemm_bf16(ctypes.byref(args), _stream()), "ltxk_gemm_bf16")
    return out


GEMV_MAX_M = 8              # rows of one ltxk_gemv_w8 launch (csrc/gemv.hip)


def _gemv(a, w, bias, epilogue, out, w_scale, **unsupported) -> torch.Tensor:
    """``gemm(..., gemv=True)``: ltxk_gemv_w8."""
    if w.dtype != FP8:
        raise TypeError(f"gemm: gemv=True needs a float8_e4m3fn `w`, got {w.dtype}")
    for name, v in unsupported.items():
        if isinstance(v, torch.Tensor) or v:
            raise ValueError(f"gemm: gemv=True takes no `{name}`")
    if epilogue != EPI_BIAS:
        raise ValueError(f"gemm: gemv=True has the `epilogue` EPI_BIAS only, got {epilogue}")
    M, K = _dims("gemm", "a", a, BF16, 2)
    N = _dims("gemm", "w", w, FP8, 2)[0]
    if not 1 <= M <= GEMV_MAX_M:
        raise ValueError(f"gemm: gemv=True takes `a` of 1 to {GEMV_MAX_M} rows, got {M}")
    if K % 16:
        raise ValueError(f"gemm: gemv=True needs `a` and `w` of K % 16 == 0, got K = {K}")
    if a.stride(0) % 8:
        raise ValueError(f"gemm: the rows of `a` must lie a multiple of 8 elements apart for gemv=True, got {a.stride(0)}")
    _operands("gemm", ("a", a, BF16, 2, 16, True), ("w", w, FP8, (N, K), 16), ("bias", bias, BF16, (N,), 2),
              ("out", out, BF16, (M, N), 2, True), ("w_scale", w_scale, F32, (N,), 4))
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    args = GemmArgs()
    args.A, args.W, args.bias, args.out = _p(a), _p(w), _p(bias), _p(out)
    args.M, args.N, args.K, args.lda, args.ldo = M, N, K, a.stride(0), out.stride(0)
    args.epilogue, args.alpha = EPI_BIAS, 1.0
    with _timed("gemv_w8", 2.0 * M * N * K, 2.0 * (M * K + M * N) + 1.0 * N * K):
        check(_lib.load().ltxk_gemv_w8(ctypes.byref(args), _p(w_scale), _stream()), "ltxk_gemv_w8")
    return out


GEMV4_MAX_M = 8             # rows of one ltxk_gemv_w4 launch (csrc/gemv4.hip: no instance spills, so all 8)


def gemv_w4(a, codes, block_scales, bias=None, out=None):
    """out = a @ w.T + bias on an OCP MXFP4 panel (ltxk_gemv_w4): ``a`` (M, K) bf16, 1 <= M <= GEMV4_MAX_M, rows a multiple of 8
    elements apart; ``codes`` (N, K/2) uint8, two e2m1 codes per byte, low nibble first; ``block_scales`` (N, K/32) uint8 e8m0
    (``weights.quantize_mxfp4`` gives both); K % 32 == 0; ``bias`` (N) bf16; ``out`` (M, N) bf16 rows.  One launch, no workspace;
    a row's bits depend on that row, the panel row, its scale row and its bias alone.  (Its refusals - dtype, shape and layout of
    every operand, each before the device - are tabulated in tests/test_mxfp4_cpu.py.)"""
    M, K = _dims("gemv_w4", "a", a, BF16, 2)
    N = _dims("gemv_w4", "codes", codes, torch.uint8, 2)[0]
    if not 1 <= M <= GEMV4_MAX_M:
        raise ValueError(f"gemv_w4: `a` must have 1 to {GEMV4_MAX_M} rows, got {M}")
    if K == 0 or K % MXFP4_BLOCK:
        raise ValueError(f"gemv_w4: needs K % {MXFP4_BLOCK} == 0 (one scale per {MXFP4_BLOCK} k), got K = {K}")
    if a.stride(0) % 8:
        raise ValueError(f"gemv_w4: the rows of `a` must lie a multiple of 8 elements apart, got {a.stride(0)}")
    _operands("gemv_w4", ("a", a, BF16, 2, 16, True), ("codes", codes, torch.uint8, (N, K // 2), 16),
              ("block_scales", block_scales, torch.uint8, (N, K // MXFP4_BLOCK), 4), ("bias", bias, BF16, (N,), 2),
              ("out", out, BF16, (M, N), 2, True))
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    args = GemmArgs()
    args.A, args.W, args.bias, args.out = _p(a), _p(codes), _p(bias), _p(out)
    args.M, args.N, args.K, args.lda, args.ldo = M, N, K, a.stride(0), out.stride(0)
    args.epilogue, args.alpha = EPI_BIAS, 1.0
    with _timed("gemv_w4", 2.0 * M * N * K, 2.0 * (M * K + M * N) + 0.5 * N * K + 1.0 * N * (K // MXFP4_BLOCK)):
        check(_lib.load().ltxk_gemv_w4(ctypes.byref(args), _p(block_scales), _stream()), "ltxk_gemv_w4")
    return out


MXFP4_KSTEP = 256           # k per K-step of ltxk_gemm_mxfp4 (LTXK_MXFP4_KSTEP): K must be a multiple of it


def quant_rows_mxfp4(a, out=None):
    """ltxk_quant_rows_mxfp4: ``a`` (M, K) bf16 (row stride may exceed K), K % 32 == 0 -> (codes (M, K/2) uint8, block_scales
    (M, K/32) uint8), bit for bit ``weights.quantize_mxfp4(a)``: OCP MXFP4, one e8m0 scale per 32 consecutive k, element 2i in the
    low nibble.  ``out=(codes, block_scales)``: write into these (either may be rows of a wider buffer)."""
    M, K = _dims("quant_rows_mxfp4", "a", a, BF16, 2)
    if K == 0 or K % MXFP4_BLOCK:
        raise ValueError(f"quant_rows_mxfp4: needs K % {MXFP4_BLOCK} == 0 (one scale per {MXFP4_BLOCK} k), got K = {K}")
    if a.stride(0) % 8:
        raise ValueError(f"quant_rows_mxfp4: the rows of `a` must lie a multiple of 8 elements apart, got {a.stride(0)}")
    q, sc = out if out is not None else (None, None)
    if q is not None and q.dim() == 2 and q.stride(0) % 16:
        raise ValueError(f"quant_rows_mxfp4: the rows of out[0] must lie a multiple of 16 bytes apart, got {q.stride(0)}")
    _operands("quant_rows_mxfp4", ("a", a, BF16, 2, 16, True), ("out[0]", q, torch.uint8, (M, K // 2), 16, True),
              ("out[1]", sc, torch.uint8, (M, K // MXFP4_BLOCK), 1, True))
    if out is None:
        q = torch.empty((M, K // 2), dtype=torch.uint8, device=a.device)
        sc = torch.empty((M, K // MXFP4_BLOCK), dtype=torch.uint8, device=a.device)
    with _timed("quant_rows_mxfp4", 0.0, 2.0 * M * K + 0.5 * M * K + 1.0 * M * (K // MXFP4_BLOCK)):
        check(_lib.load().ltxk_quant_rows_mxfp4(_p(a), a.stride(0), _p(q), q.stride(0), _p(sc), sc.stride(0), M, K, _stream()),
              "ltxk_quant_rows_mxfp4")
    return q, sc


def gemm_mxfp4(a, a_scales, w, w_scales, bias=None, *, epilogue=EPI_BIAS, out=None, resid=None, gate=None, gate_row=None,
               gate_stride=0, out_tokens_per_batch=0, alpha=1.0, out2=None, n_split=0, sumsq=None):
    """out = epi(deq(a) @ deq(w).T + bias) with both operands in OCP MXFP4 (ltxk_gemm_mxfp4): ``a`` (M, K/2) uint8 codes (rows may
    be a multiple of 16 bytes apart) with ``a_scales`` (M, K/32) uint8 - what ``quant_rows_mxfp4`` returns - and ``w`` (N, K/2) /
    ``w_scales`` (N, K/32), the contiguous pair of ``weights.quantize_mxfp4``.  K % MXFP4_KSTEP == 0, N % 8 == 0.  Epilogues,
    ``out``, ``out2`` / ``n_split``, ``out_tokens_per_batch`` and ``sumsq`` as for ``gemm``.  Always single-pass: a row's bits
    depend on that row, the panel and the epilogue operands alone.  (Refusals: tests/test_mxfp4_dit_cpu.py.)"""
    U8 = torch.uint8
    M, K2 = _dims("gemm_mxfp4", "a", a, U8, 2)
    N = _dims("gemm_mxfp4", "w", w, U8, 2)[0]
    K = 2 * K2
    if K == 0 or K % MXFP4_KSTEP:
        raise ValueError(f"gemm_mxfp4: needs K % {MXFP4_KSTEP} == 0, got K = {K} ({K2} code bytes per row of `a`)")
    if N % 8:
        raise ValueError(f"gemm_mxfp4: needs N % 8 == 0, got N = {N}")
    if a.stride(0) % 16:
        raise ValueError(f"gemm_mxfp4: the rows of `a` must lie a multiple of 16 bytes apart, got {a.stride(0)}")
    if a_scales is not None and a_scales.dim() == 2 and a_scales.stride(0) % 8:
        raise ValueError(f"gemm_mxfp4: the rows of `a_scales` must lie a multiple of 8 bytes apart, got {a_scales.stride(0)}")
    if a_scales is None or w_scales is None:
        raise TypeError("gemm_mxfp4: both block-scale panels are required")
    if n_split and out2 is None:
        raise ValueError("gemm_mxfp4: split output needs a bf16 `out2`")
    if out is None and out_tokens_per_batch:
        raise ValueError("gemm_mxfp4: transposed output needs a preallocated `out`")
    if not n_split:
        out2 = None
    T = out_tokens_per_batch
    cols, nb = n_split or N, M // T if T else 0
    _operands("gemm_mxfp4", ("a", a, U8, 2, 16, True), ("a_scales", a_scales, U8, (M, K // MXFP4_BLOCK), 8, True),
              ("w", w, U8, (N, K2), 16), ("w_scales", w_scales, U8, (N, K // MXFP4_BLOCK), 8), ("bias", bias, BF16, (N,), 8),
              ("out", out, BF16, (nb, N, -T) if T and not n_split else (M, cols), 8, True), ("resid", resid, BF16, (M, N), 8, True),
              ("gate", gate, BF16, _table("gemm_mxfp4", "gate", gate, N, gate_stride), 8, True), ("gate_row", gate_row, I32, (M,), 4),
              ("out2", out2, BF16, (nb, N - n_split, -T), 8, True), ("sumsq", sumsq, F32, (M, -(cols // 64)), 4, True))
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    args = GemmArgs()
    args.A, args.W, args.bias, args.out = _p(a), _p(w), _p(bias), _p(out)
    args.resid, args.gate, args.gate_row = _p(resid), _p(gate), _p(gate_row)
    args.M, args.N, args.K = M, N, K
    args.lda = a.stride(0)
    args.ldo = out.stride(-2)
    args.ldr = resid.stride(0) if resid is not None else 0
    args.gate_stride = gate_stride
    args.epilogue = epilogue
    args.out_tokens_per_batch = out_tokens_per_batch
    args.alpha = alpha
    args.out2, args.n_split, args.ldo2 = _p(out2), n_split, (out2.stride(-2) if out2 is not None else 0)
    args.sumsq, args.sumsq_ld = _p(sumsq), (sumsq.stride(0) if sumsq is not None else 0)
    with _timed("gemm_mxfp4", 2.0 * M * N * K, 0.53125 * (M * K + N * K) + 2.0 * M * N):
        check(_lib.load().ltxk_gemm_mxfp4(ctypes.byref(args), _p(a_scales), a_scales.stride(0), _p(w_scales), w_scales.stride(0),
                                          _stream()), "ltxk_gemm_mxfp4")
    return out


@dataclass(frozen=True)
class GemmPlan:
    """ltxk_gemm_plan: the launch form of one ltxk_gemm_bf16 call (_lib.GEMM_FORM_*), its tile, and its K slices."""
    form: int
    tile_rows: int
    tile_cols: int
    row_tiles: int
    col_tiles: int
    slices: int
    ksteps: int

    @property
    def split_k(self) -> bool:
        return self.form == _lib.GEMM_FORM_SPLITK


_PLAN_ADDR = 1 << 12          # stands in for every device pointer of a planned call: non-NULL, aligned, never read


def gemm_plan(M: int, N: int, K: int, *, epilogue: int = EPI_BIAS, lda: Optional[int] = None, ldo: Optional[int] = None,
              out_tokens_per_batch: int = 0, n_split: int = 0, ldo2: Optional[int] = None, sumsq: bool = False,
              split_k: bool = True, workspace: Optional[Tuple[int, int]] = None, w8: bool = False,
              w8a8: bool = False, mxfp4: bool = False) -> GemmPlan:
    """The form ``gemm`` takes for an (M,K) x (N,K)^T launch with these options, decided on the host by the function the
    launch itself uses (no device needed).  The split-K scratch is offered exactly as ``gemm`` offers it (``split_k``,
    SPLITK_MAX_M); ``workspace=(address, bytes)`` offers that one instead (address 0: none).  Strides default to those of
    contiguous tensors (V^T: tokens padded to 64).  Raises LtxkError where ``gemm`` would refuse the arguments.
    ``w8``: the plan of the same call with a float8_e4m3fn weight (ltxk_gemm_w8_plan).  ``w8a8``: with float8_e4m3fn
    activations too (ltxk_gemm_w8a8_plan: always single-pass, 128-wide K-steps).  ``mxfp4``: the plan of ``gemm_mxfp4``
    (ltxk_gemm_mxfp4_plan: always single-pass, MXFP4_KSTEP-wide K-steps; ``lda`` in bytes, K/2 by default)."""
    args = GemmArgs()
    args.A = args.W = args.out = _PLAN_ADDR
    args.M, args.N, args.K = M, N, K
    args.lda = (K // 2 if mxfp4 else K) if lda is None else lda
    ld_t = (out_tokens_per_batch + 63) // 64 * 64
    args.ldo = ldo if ldo is not None else (ld_t if out_tokens_per_batch and not n_split else (n_split or N))
    if epilogue in (EPI_BIAS_GATE_RES, EPI_BIAS_RES, EPI_SCALE_RES):
        args.resid, args.ldr = _PLAN_ADDR, N
    if epilogue == EPI_BIAS_GATE_RES:
        args.gate = _PLAN_ADDR
    args.epilogue = epilogue
    args.out_tokens_per_batch = out_tokens_per_batch
    if n_split:
        args.out2, args.n_split, args.ldo2 = _PLAN_ADDR, n_split, (ld_t if ldo2 is None else ldo2)
    if sumsq:
        args.sumsq, args.sumsq_ld = _PLAN_ADDR, (n_split or N) // 64
    if workspace is not None:
        args.workspace, args.workspace_bytes = workspace
    elif _offers_workspace(M, split_k):
        args.workspace, args.workspace_bytes = _PLAN_ADDR, GEMM_WORKSPACE_BYTES
    pl = _lib.GemmPlan()
    if mxfp4:
        check(_lib.load().ltxk_gemm_mxfp4_plan(ctypes.byref(args), ctypes.byref(pl)), "ltxk_gemm_mxfp4_plan")
    elif w8a8:
        check(_lib.load().ltxk_gemm_w8a8_plan(ctypes.byref(args), ctypes.byref(pl)), "ltxk_gemm_w8a8_plan")
    elif w8:
        check(_lib.load().ltxk_gemm_w8_plan(ctypes.byref(args), ctypes.byref(pl)), "ltxk_gemm_w8_plan")
    else:
        check(_lib.load().ltxk_gemm_plan(ctypes.byref(args), ctypes.byref(pl)), "ltxk_gemm_plan")
    return GemmPlan(pl.form, pl.tile_rows, pl.tile_cols, pl.row_tiles, pl.col_tiles, pl.slices, pl.ksteps)


def quant_rows_fp8(a: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ltxk_quant_rows_fp8: a (M,K) bf16 (row stride may exceed K) -> (a8 (M,K) float8_e4m3fn, a_scale (M) fp32) with
    a ~= a8 * a_scale[:, None]: per row scale = max(max|a|, 2^-64) / 448 and a8 = e4m3(a / scale), round to nearest even.
    ``out=(a8, a_scale)``: write into these (a8 may be a strided view; a_scale contiguous)."""
    M, K = _dims("quant_rows_fp8", "a", a, BF16, 2)
    a8, sc = out if out is not None else (None, None)
    _operands("quant_rows_fp8", ("a", a, BF16, 2, 16, True), ("out[0]", a8, FP8, (M, K), 8, True), ("out[1]", sc, F32, (M,), 4))
    if out is None:
        a8 = torch.empty((M, K), dtype=FP8, device=a.device)
        sc = torch.empty((M,), dtype=torch.float32, device=a.device)
    with _timed("quant_rows_fp8", 0.0, 3.0 * M * K):
        check(_lib.load().ltxk_quant_rows_fp8(_p(a), a.stride(0), _p(a8), a8.stride(0), _p(sc), M, K, _stream()), "ltxk_quant_rows_fp8")
    return a8, sc


def pointer_table(tensors) -> torch.Tensor:
    """Device array of the tensors' addresses (int64): the per-group operand table of ``gemm_grouped``.  It holds
    addresses only - the caller keeps the tensors alive and in place for as long as the table is used."""
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=tensors[0].device)


def _grouped_args(G: int, M: int, N: int, K: int, n_split: int, out_tokens_per_batch: int) -> GemmGroupedArgs:
    args = GemmGroupedArgs()
    args.G, args.M, args.N, args.K = G, M, N, K
    args.n_split, args.out_tokens_per_batch = n_split, out_tokens_per_batch
    return args


def gemm_grouped(a: torch.Tensor, w_table: torch.Tensor, bias_table: Optional[torch.Tensor], N: int, *,
                 out: torch.Tensor, out2: torch.Tensor, n_split: int, out_tokens_per_batch: int,
                 sumsq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_gemm_bf16_grouped: for every group g, ``gemm(a, W[g], bias[g], out=out[g], out2=out2[g], n_split=...,
    sumsq=sumsq[g], split_k=False)`` - the same bits - as ONE persistent launch.  a (M,K); w_table / bias_table:
    ``pointer_table`` of G contiguous (N,K) panels / (N) rows; out (G,M,n_split), out2 (G,B,N-n_split,ld >= tokens), sumsq
    (G,M,>=n_split/64) fp32, each with unit inner stride, a group stride of its own and, in out2, dense batches."""
    M, K = _dims("gemm_grouped", "a", a, BF16, 2)
    G = _dims("gemm_grouped", "w_table", w_table, torch.int64, 1)[0]
    T = out_tokens_per_batch
    if out2.dim() == 4 and out2.stride(1) != out2.shape[2] * out2.stride(2):
        raise ValueError(f"gemm_grouped: out2 must be (G,B,N-n_split,ld) with contiguous batches, got strides {out2.stride()}")
    _operands("gemm_grouped", ("a", a, BF16, 2, 16, True), ("w_table", w_table, torch.int64, 1, 8), ("bias_table", bias_table, torch.int64, (G,), 8),
              ("out", out, BF16, (G, M, n_split), 8, 4), ("out2", out2, BF16, (G, M // T if T else 0, N - n_split, -T), 8, 4),
              ("sumsq", sumsq, F32, (G, M, -(n_split // 64)), 4, 1))
    args = _grouped_args(G, M, N, K, n_split, out_tokens_per_batch)
    args.A, args.W, args.bias = _p(a), _p(w_table), _p(bias_table)
    args.out, args.out2, args.sumsq = _p(out), _p(out2), _p(sumsq)
    args.out_gstride, args.out2_gstride = out.stride(0), out2.stride(0)
    args.sumsq_gstride = sumsq.stride(0) if sumsq is not None else 0
    args.lda, args.ldo, args.ldo2 = a.stride(0), out.stride(1), out2.stride(2)
    args.sumsq_ld = sumsq.stride(1) if sumsq is not None else 0
    with _timed("gemm_bf16", 2.0 * G * M * N * K, 2.0 * (M * K + G * (N * K + M * N))):
        check(_lib.load().ltxk_gemm_bf16_grouped(ctypes.byref(args), _stream()), "ltxk_gemm_bf16_grouped")
    return out


@dataclass(frozen=True)
class GemmGroupedPlan:
    """ltxk_gemm_grouped_plan: the tiling of one ltxk_gemm_bf16_grouped launch."""
    tile_rows: int
    rem_rows: int
    row_tiles: int
    col_tiles: int
    tiles: int


def gemm_grouped_plan(G: int, M: int, N: int, K: int, *, n_split: int, out_tokens_per_batch: int) -> GemmGroupedPlan:
    """The tile ``gemm_grouped`` takes for G (M,K) x (N,K)^T problems, decided on the host (no device needed) by the function
    the launch itself uses.  Strides are those of contiguous buffers."""
    args = _grouped_args(G, M, N, K, n_split, out_tokens_per_batch)
    args.A = args.W = args.out = args.out2 = _PLAN_ADDR
    ld_t = (out_tokens_per_batch + 63) // 64 * 64
    args.lda, args.ldo, args.ldo2 = K, n_split, ld_t
    args.out_gstride = M * n_split
    args.out2_gstride = (M // max(out_tokens_per_batch, 1)) * (N - n_split) * ld_t
    pl = _lib.GemmGroupedPlan()
    check(_lib.load().ltxk_gemm_grouped_plan(ctypes.byref(args), ctypes.byref(pl)), "ltxk_gemm_grouped_plan")
    return GemmGroupedPlan(pl.tile_rows, pl.rem_rows, pl.row_tiles, pl.col_tiles, pl.tiles)


def flash_attn(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, B: int, H: int,
               Tq: int, Tk: int, scale: float, q_sumsq: Optional[torch.Tensor] = None,
               q_norm_weight: Optional[torch.Tensor] = None, cos: Optional[torch.Tensor] = None,
               sin: Optional[torch.Tensor] = None, eps: float = 1e-6, tail_split: bool = True, head_dim: int = 128) -> torch.Tensor:
    """q (B*Tq, H*128) rows, k (B*Tk, H*128) rows, vt (B, H*128, ld >= Tk), out (B*Tq, H*128) rows.  With ``q_sumsq``
    (B*Tq, >= H*2) the raw q projection is normalised (q_norm_weight (H*128)) and rotated (cos/sin (H,Tq,64)) inside the
    kernel; without it those three are not read.
    ``tail_split=False``: LTXK_ATTN_NO_TAIL_SPLIT (results independent of how many (batch, head) pairs share the launch).
    ``head_dim=64``: ltxk_flash_attn_dh64, the same operands at H*64 columns; it has no fused query preparation (``q_sumsq`` is
    refused) and one launch form, so ``tail_split`` has nothing to decide."""
    if head_dim not in (64, 128):
        raise ValueError(f"flash_attn: head_dim = {head_dim} must be 128 or 64")
    if head_dim == 64 and q_sumsq is not None:
        raise ValueError("flash_attn: head_dim = 64 has no fused query preparation, q_sumsq must be None")
    if q_sumsq is None:
        q_norm_weight = cos = sin = None
    elif q_norm_weight is None or (cos is None) != (sin is None):
        raise ValueError("flash_attn: q_sumsq needs q_norm_weight, and cos and sin both or neither")
    D = H * head_dim
    _operands("flash_attn", ("q", q, BF16, (B * Tq, D), 16, True), ("k", k, BF16, (B * Tk, D), 16, True),
              ("vt", vt, BF16, (B, D, -Tk), 16, True), ("out", out, BF16, (B * Tq, D), 16, True),
              ("q_sumsq", q_sumsq, F32, (B * Tq, -(H * 2)), 16, True),
              ("q_norm_weight", q_norm_weight, BF16, (1, D) if q_sumsq is not None and q_norm_weight.dim() == 2 else (D,), 16),
              ("cos", cos, F32, (H, Tq, 64), 16), ("sin", sin, F32, (H, Tq, 64), 16))
    a = AttnArgs()
    a.flags = 0 if tail_split else _lib.ATTN_NO_TAIL_SPLIT
    a.q, a.k, a.vt, a.out = _p(q), _p(k), _p(vt), _p(out)
    a.ldq, a.ldk, a.ldvt, a.ldo = q.stride(0), k.stride(0), vt.stride(-2), out.stride(0)
    a.B, a.H, a.Tq, a.Tk, a.scale = B, H, Tq, Tk, scale
    if q_sumsq is not None:
        a.q_sumsq, a.q_sumsq_ld, a.q_sumsq_n = _p(q_sumsq), q_sumsq.stride(0), H * 2
        a.q_norm_weight, a.cos, a.sin, a.eps = _p(q_norm_weight), _p(cos), _p(sin), eps
    with _timed("flash_attn", 4.0 * B * H * Tq * Tk * head_dim, 2.0 * B * H * head_dim * (2 * Tq + 2 * Tk)):
        if head_dim == 64:
            check(_lib.load().ltxk_flash_attn_dh64(ctypes.byref(a), _stream()), "ltxk_flash_attn_dh64")
        else:
            check(_lib.load().ltxk_flash_attn(ctypes.byref(a), _stream()), "ltxk_flash_attn")
    return out


@dataclass(frozen=True)
class AttnPlan:
    """ltxk_flash_attn_plan: the launch form of one ltxk_flash_attn call (include/ltxk.h, struct ltxk_flash_attn_plan)."""
    kernel: int
    mfma_k: int
    tiles_192: int
    tiles_128: int
    whole_workgroups: int
    split_tiles: int
    workgroups: int
    xcd_order: int

    @property
    def mix(self) -> bool:
        return self.kernel == _lib.ATTN_KERNEL_MIX


def flash_attn_plan(B: int, H: int, Tq: int, Tk: int, *, cus: int, tail_split: bool = True, fused_q: bool = False) -> AttnPlan:
    """The form ``flash_attn`` takes for these dimensions on a device of ``cus`` compute units
    (torch.cuda.get_device_properties(d).multi_processor_count), decided on the host by the function the launch itself uses
    (no device needed).  Strides are those of contiguous tensors (V^T: keys padded to 64); ``fused_q``: with the fused query
    preparation's operands.  Raises LtxkError where ``flash_attn`` would refuse the arguments."""
    a = AttnArgs()
    a.flags = 0 if tail_split else _lib.ATTN_NO_TAIL_SPLIT
    a.q = a.k = a.vt = a.out = _PLAN_ADDR
    a.ldq = a.ldk = a.ldo = H * 128
    a.ldvt = (Tk + 63) // 64 * 64
    a.B, a.H, a.Tq, a.Tk, a.scale = B, H, Tq, Tk, 1.0 / math.sqrt(128)
    if fused_q:
        a.q_sumsq, a.q_sumsq_ld, a.q_sumsq_n = _PLAN_ADDR, H * 2, H * 2
        a.q_norm_weight = a.cos = a.sin = _PLAN_ADDR
        a.eps = 1e-6
    pl = _lib.AttnPlan()
    check(_lib.load().ltxk_flash_attn_plan(ctypes.byref(a), cus, ctypes.byref(pl)), "ltxk_flash_attn_plan")
    return AttnPlan(pl.kernel, pl.mfma_k, pl.tiles_192, pl.tiles_128, pl.whole_workgroups, pl.split_tiles, pl.workgroups,
                    pl.xcd_order)


def _modulation(who: str, M: int, D: int, scale, shift, mod_stride: int, mod_row) -> tuple:
    """The modulation operands of a row norm over (M,D): scale / shift are rows of a (rows, D) table that lie ``mod_stride``
    apart, picked per token by mod_row (M) int32 (None: row 0)."""
    if (scale is None) != (shift is None):
        raise ValueError(f"{who}: scale and shift must both be given or both be None")
    return (("scale", scale, BF16, _table(who, "scale", scale, D, mod_stride), 16, True),
            ("shift", shift, BF16, _table(who, "shift", shift, D, mod_stride), 16, True), ("mod_row", mod_row, I32, (M,), 4))


def rmsnorm_modulate(x: torch.Tensor, eps: float, scale: Optional[torch.Tensor] = None,
                     shift: Optional[torch.Tensor] = None, mod_stride: int = 0,
                     mod_row: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                     sumsq: Optional[torch.Tensor] = None, scale_is_one_plus: bool = False,
                     scale2: Optional[torch.Tensor] = None, shift2: Optional[torch.Tensor] = None,
                     out2: Optional[torch.Tensor] = None):
    """x, out (M,D) contiguous; the modulation of row m is scale / shift[mod_row[m] * mod_stride + d].
    ``sumsq`` (M, >= D/64) fp32: the rows' sums of squares in 64-column partials (gemm(..., sumsq=)); without it the
    kernel reduces the row itself.  ``scale_is_one_plus``: scale holds bf16(1+scale) (needs sumsq).
    ``scale2`` / ``shift2``: a second modulation of the same normalised row (ltxk_rmsnorm_modulate2: x is read once) with the
    same mod_stride / mod_row / scale_is_one_plus, into ``out2``; the call then returns (out, out2), each with the bits of
    the one-pair call on the same operands."""
    if scale_is_one_plus and sumsq is None:
        raise ValueError("rmsnorm_modulate: scale_is_one_plus needs sumsq")
    two = scale2 is not None or shift2 is not None
    if two and (scale is None or shift is None or scale2 is None or shift2 is None):
        raise ValueError("rmsnorm_modulate: a second modulation needs scale, shift, scale2 and shift2")
    if out2 is not None and not two:
        raise ValueError("rmsnorm_modulate: out2 goes with scale2 / shift2")
    M, D = _dims("rmsnorm_modulate", "x", x, BF16, 2)
    _operands("rmsnorm_modulate", ("x", x, BF16, 2, 16), ("out", out, BF16, (M, D), 16),
              *_modulation("rmsnorm_modulate", M, D, scale, shift, mod_stride, mod_row), ("sumsq", sumsq, F32, (M, -(D // 64)), 4, True),
              ("scale2", scale2, BF16, _table("rmsnorm_modulate", "scale2", scale2, D, mod_stride), 16, True),
              ("shift2", shift2, BF16, _table("rmsnorm_modulate", "shift2", shift2, D, mod_stride), 16, True),
              ("out2", out2, BF16, (M, D), 16))
    if out is None:
        out = torch.empty_like(x)
    if two:
        if out2 is None:
            out2 = torch.empty_like(x)
        if out2.data_ptr() == out.data_ptr():
            raise ValueError("rmsnorm_modulate: out and out2 must be two buffers")
        with _timed("rmsnorm_modulate", 0.0, 6.0 * M * D):
            check(_lib.load().ltxk_rmsnorm_modulate2(_p(x), _p(out), _p(out2), M, D, eps, _p(sumsq), 0 if sumsq is None else sumsq.stride(0),
                                                     D // 64, _p(scale), _p(shift), _p(scale2), _p(shift2), mod_stride, _p(mod_row),
                                                     int(scale_is_one_plus), _stream()), "ltxk_rmsnorm_modulate2")
        return out, out2
    with _timed("rmsnorm_modulate", 0.0, 4.0 * M * D):
        if sumsq is not None:
            check(_lib.load().ltxk_rmsnorm_modulate_ss(_p(x), _p(out), M, D, eps, _p(sumsq), sumsq.stride(0), D // 64, _p(scale),
                                                       _p(shift), mod_stride, _p(mod_row), int(scale_is_one_plus), _stream()),
                  "ltxk_rmsnorm_modulate_ss")
        else:
            check(_lib.load().ltxk_rmsnorm_modulate(_p(x), _p(out), M, D, eps, _p(scale), _p(shift), mod_stride,
                                                    _p(mod_row), _stream()), "ltxk_rmsnorm_modulate")
    return out


def layernorm_modulate(x: torch.Tensor, eps: float, scale: Optional[torch.Tensor] = None,
                       shift: Optional[torch.Tensor] = None, mod_stride: int = 0,
                       mod_row: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    M, D = _dims("layernorm_modulate", "x", x, BF16, 2)
    _operands("layernorm_modulate", ("x", x, BF16, 2, 16), ("out", out, BF16, (M, D), 16),
              *_modulation("layernorm_modulate", M, D, scale, shift, mod_stride, mod_row))
    if out is None:
        out = torch.empty_like(x)
    check(_lib.load().ltxk_layernorm_modulate(_p(x), _p(out), M, D, eps, _p(scale), _p(shift), mod_stride,
                                              _p(mod_row), _stream()), "ltxk_layernorm_modulate")
    return out


def qknorm_rope(buf: torch.Tensor, nseg: int, D: int, weight: torch.Tensor, cos: Optional[torch.Tensor],
                sin: Optional[torch.Tensor], T: int, H: int, eps: float, sumsq: Optional[torch.Tensor] = None,
                head_dim: int = 128) -> torch.Tensor:
    """In place on the first nseg*D columns of buf (M, ld), D = 128*H: weight (nseg,D) (or flat), cos / sin (H,T,64) fp32 or
    both None.  ``sumsq`` (M, >= nseg*D/64) fp32: precomputed partial sums of squares of those columns (gemm(..., sumsq=)).
    ``head_dim=64``: ltxk_qknorm_rope_dh64 - D = 64*H, H <= 32, cos / sin (H,T,32), the rotation partner of channel j is j + 32."""
    if head_dim not in (64, 128):
        raise ValueError(f"qknorm_rope: head_dim = {head_dim} must be 128 or 64")
    if (cos is None) != (sin is None) or D != head_dim * H:
        raise ValueError(f"qknorm_rope: cos and sin go together, and D = {D} must be {head_dim} * H = {head_dim * H}")
    M, ld = _dims("qknorm_rope", "buf", buf, BF16, 2)
    _operands("qknorm_rope", ("buf", buf if ld == nseg * D else buf[:, :nseg * D], BF16, (M, nseg * D), 16, True),
              ("weight", weight, BF16, (nseg, D) if weight.dim() == 2 else (nseg * D,), 16), ("cos", cos, F32, (H, T, head_dim // 2), 16),
              ("sin", sin, F32, (H, T, head_dim // 2), 16), ("sumsq", sumsq, F32, (M, -(nseg * D // 64)), 4, True))
    with _timed("qknorm_rope", 0.0, 4.0 * M * nseg * D + (8.0 * M * D // 2 if cos is not None else 0.0)):
        if head_dim == 64:
            check(_lib.load().ltxk_qknorm_rope_dh64(_p(buf), buf.stride(0), M, nseg, D, _p(weight), _p(cos), _p(sin), T, H, eps,
                                                    _p(sumsq), 0 if sumsq is None else sumsq.stride(0), _stream()),
                  "ltxk_qknorm_rope_dh64")
        elif sumsq is not None:
            check(_lib.load().ltxk_qknorm_rope_ss(_p(buf), buf.stride(0), M, nseg, D, _p(weight), _p(cos), _p(sin),
                                                  T, H, eps, _p(sumsq), sumsq.stride(0), _stream()), "ltxk_qknorm_rope_ss")
        else:
            check(_lib.load().ltxk_qknorm_rope(_p(buf), buf.stride(0), M, nseg, D, _p(weight), _p(cos), _p(sin),
                                               T, H, eps, _stream()), "ltxk_qknorm_rope")
    return buf


def qknorm_grouped(buf: torch.Tensor, weight: torch.Tensor, H: int, eps: float, sumsq: torch.Tensor) -> torch.Tensor:
    """ltxk_qknorm_grouped_ss: q/k RMSNorm without rotation, in place on buf (G,M,D) with weight row g of the (G,D) table
    and the row statistics sumsq (G,M,>=D/64) of ``gemm_grouped`` - the bits of G ``qknorm_rope(buf[g], 1, D, weight[g],
    None, None, ..., sumsq=sumsq[g])`` calls, in one launch."""
    G, M, D = _dims("qknorm_grouped", "buf", buf, BF16, 3)
    _operands("qknorm_grouped", ("buf", buf, BF16, 3, 16, 8), ("weight", weight, BF16, (G, D), 16), ("sumsq", sumsq, F32, (G, M, -(D // 64)), 4, 1))
    with _timed("qknorm_rope", 0.0, 4.0 * G * M * D):
        check(_lib.load().ltxk_qknorm_grouped_ss(_p(buf), buf.stride(0), buf.stride(1), G, M, D, _p(weight), H, eps, _p(sumsq),
                                                 sumsq.stride(0), sumsq.stride(1), _stream()), "ltxk_qknorm_grouped_ss")
    return buf


def timestep_embed(t: torch.Tensor, dim: int = 256, mult: float = 1.0) -> torch.Tensor:
    """t: U bf16 timesteps, contiguous -> (U, dim)."""
    _operands("timestep_embed", ("t", t, BF16, t.dim(), 2))
    out = torch.empty((t.numel(), dim), dtype=BF16, device=t.device)
    check(_lib.load().ltxk_timestep_embed(_p(t), _p(out), t.numel(), dim, mult, _stream()), "ltxk_timestep_embed")
    return out


def rope_table(positions: torch.Tensor, freq: torch.Tensor, H: int, dim: int, max_pos) -> tuple:
    """positions (3,T,2) fp32, freq (n_freq) fp32 -> cos, sin (H,T,dim/2/H) fp32."""
    T = _dims("rope_table", "positions", positions, F32, 3)[1]
    _operands("rope_table", ("positions", positions, F32, (3, T, 2), 4), ("freq", freq, F32, 1, 4))
    per_head = dim // 2 // H
    cos = torch.empty((H, T, per_head), dtype=torch.float32, device=positions.device)
    sin = torch.empty_like(cos)
    mp = (ctypes.c_float * 3)(*[float(v) for v in max_pos])
    check(_lib.load().ltxk_rope_table(_p(positions), _p(freq), _p(cos), _p(sin), T, H, dim, freq.numel(), mp,
                                      _stream()), "ltxk_rope_table")
    return cos, sin


def ada_combine(table: torch.Tensor, ada: torch.Tensor, L: int, U: int, K: int, D: int, one_plus_mask: int = 0) -> torch.Tensor:
    """table (L,K,D), ada (U,K*D) -> (L,U,K,D); rows k with bit k of one_plus_mask set hold bf16(1 + value)."""
    _operands("ada_combine", ("table", table, BF16, (L, K, D), 16), ("ada", ada, BF16, (U, K * D), 16))
    out = torch.empty((L, U, K, D), dtype=BF16, device=ada.device)
    check(_lib.load().ltxk_ada_combine(_p(table), _p(ada), _p(out), L, U, K, D, one_plus_mask, _stream()), "ltxk_ada_combine")
    return out


def silu(x: torch.Tensor) -> torch.Tensor:
    _operands("silu", ("x", x, BF16, x.dim(), 16))
    out = torch.empty_like(x)
    check(_lib.load().ltxk_silu(_p(x), _p(out), x.numel(), _stream()), "ltxk_silu")
    return out


def latent_to_tokens(latent: torch.Tensor, rep: int = 1) -> torch.Tensor:
    """(B,C,F,H,W) or (B,C,S) -> (rep*B,S,C); a latent that is not contiguous is copied first."""
    if latent.dim() < 3:
        raise ValueError(f"latent_to_tokens: latent must be (B,C,...), got {tuple(latent.shape)}")
    B, C = latent.shape[:2]
    S = latent.numel() // (B * C)
    lat = latent.contiguous()
    _operands("latent_to_tokens", ("latent", lat, BF16, lat.dim(), 2))
    out = torch.empty((rep * B, S, C), dtype=BF16, device=latent.device)
    check(_lib.load().ltxk_latent_to_tokens(_p(lat), _p(out), B, C, S, rep, _stream()), "ltxk_latent_to_tokens")
    return out


GUIDER_IDS = {"cfg_star": _lib.GUIDER_CFG_STAR, "apg": _lib.GUIDER_APG}
GUIDER_RECORD_FLOATS = _lib.GUIDER_RECORD_FLOATS


def _step_tail_args(who: str, v_pos, v_neg, v_pert, latent, guider: str, eta, norm_threshold, clean, mask_tok, sigmas_dev, more):
    """The one validator of the step-tail family, and the input fields it checked in the struct of the entry that runs
    ``guider``: a StepArgs for "cfg", a GuiderArgs for "cfg_star" / "apg".  ``more(B, C, S)``: the entry's own operands (out,
    record, workspace), checked in the same ``_operands`` call.  v_* are (B,S,C), mask_tok (B,S), sigmas_dev (2,); latent,
    clean and out are (B,C,...) volumes that the kernels index as dense (B,C,S) arrays and that callers pass in the
    latent's own 5-D shape or flattened, so they are held to the element count B*C*S, not to one shape."""
    if guider != "cfg":
        if guider not in GUIDER_IDS:
            raise ValueError(f"{who}: unknown guider {guider!r} (expected 'cfg' or one of {sorted(GUIDER_IDS)})")
        eta, norm_threshold = float(eta), float(norm_threshold)
        if not math.isfinite(eta):
            raise ValueError(f"{who}: eta must be finite, got {eta}")
        if not (math.isfinite(norm_threshold) and norm_threshold >= 0.0):
            raise ValueError(f"{who}: norm_threshold must be finite and >= 0, got {norm_threshold}")
        if v_neg is None:
            raise ValueError(f"{who}: v_neg is required (the guider compares the positive with the negative prediction)")
    if v_pos is None or (clean is None) != (mask_tok is None):
        raise ValueError(f"{who}: v_pos is required; clean and mask_tok must both be given or both be None")
    if latent.dim() < 2:
        raise ValueError(f"{who}: latent must be (B,C,...), got {tuple(latent.shape)}")
    B, C = latent.shape[:2]
    S = latent.numel() // max(B * C, 1)
    _operands(who, ("latent", latent, BF16, latent.dim(), 2), ("v_pos", v_pos, BF16, (B, S, C), 16), ("v_neg", v_neg, BF16, (B, S, C), 16),
              ("v_pert", v_pert, BF16, (B, S, C), 16), ("clean", clean, BF16, _volume(clean, B, C, S), 2),
              ("mask_tok", mask_tok, F32, (B, S), 4), ("sigmas_dev", sigmas_dev, F32, (2,), 4), *more(B, C, S))
    a = StepArgs() if guider == "cfg" else GuiderArgs()
    a.v_pos, a.v_neg, a.v_pert, a.latent = _p(v_pos), _p(v_neg), _p(v_pert), _p(latent)
    a.clean, a.mask, a.sigmas_dev = _p(clean), _p(mask_tok), _p(sigmas_dev)
    a.B, a.C, a.S = B, C, S
    if guider != "cfg":
        a.guider, a.eta, a.norm_threshold = GUIDER_IDS[guider], eta, norm_threshold
    return a


def _volume(t: Optional[torch.Tensor], B: int, C: int, S: int):
    """The shape item of a (B,C,...) volume held to its element count: ``t``'s own shape if that has B*C*S elements."""
    return t.shape if t is not None and t.numel() == B * C * S else (B, C, S)


def step_tail(v_pos: torch.Tensor, v_neg: Optional[torch.Tensor], v_pert: Optional[torch.Tensor], latent: torch.Tensor, *,
              cfg_scale: float, stg_scale: float = 0.0, sigma: float, sigma_next: float, guider: str = "cfg",
              record: Optional[torch.Tensor] = None, eta: float = 1.0, norm_threshold: float = 0.0,
              clean: Optional[torch.Tensor] = None, mask_tok: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              sigmas_dev: Optional[torch.Tensor] = None, bf16_euler: bool = False) -> torch.Tensor:
    """One denoise-step tail, one launch: guidance -> x0 -> mask blend -> Euler.  v_* (B,S,C) tokens; latent (B,C,...)
    channels-first; mask_tok (B,S) float32.  ``guider`` "cfg": the velocity-space CFG combine (``v_neg=None``: none), and with
    ``v_pert`` - the velocity of the perturbed forward - the STG term v = bf16(g + bf16(stg_scale * bf16(v_pos - v_pert)))
    (ltxk_guided_euler_step).  "cfg_star" / "apg": the guider's delta and the STG term in x0 space with the scalars of
    ``record`` (from ``guidance_sums`` on the same inputs; ltxk_guider_euler_step).  With ``sigmas_dev`` (2 float32 on the
    device) the scalars are read from device memory (hipGraph replay).  ``out`` may be ``latent`` itself (each element is
    read and written by one thread).  ``bf16_euler``: the reference's fp32_euler=False compiled step (generate.py:741-748)."""
    if guider != "cfg" and record is None:
        raise ValueError("step_tail: record is required (the output of guidance_sums)")
    a = _step_tail_args("step_tail", v_pos, v_neg, v_pert, latent, guider, eta, norm_threshold, clean, mask_tok, sigmas_dev,
                        lambda B, C, S: (("out", out, BF16, _volume(out, B, C, S), 2),
                                         ("record", record if guider != "cfg" else None, F32, (B, GUIDER_RECORD_FLOATS), 4)))
    if out is None:
        out = torch.empty_like(latent)
    a.out = _p(out)
    a.cfg_scale, a.stg_scale, a.sigma, a.sigma_next = cfg_scale, stg_scale, sigma, sigma_next
    a.flags = int(bf16_euler)
    if guider == "cfg":
        check(_lib.load().ltxk_guided_euler_step(ctypes.byref(a), _stream()), "ltxk_guided_euler_step")
    else:
        a.record = _p(record)
        check(_lib.load().ltxk_guider_euler_step(ctypes.byref(a), _stream()), "ltxk_guider_euler_step")
    return out


def cfg_euler_step(v_pos: torch.Tensor, v_neg: Optional[torch.Tensor], latent: torch.Tensor, cfg_scale: float,
                   sigma: float, sigma_next: float, clean: Optional[torch.Tensor] = None,
                   mask_tok: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   sigmas_dev: Optional[torch.Tensor] = None, bf16_euler: bool = False) -> torch.Tensor:
    """``step_tail`` with plain CFG and no STG term."""
    return step_tail(v_pos, v_neg, None, latent, cfg_scale=cfg_scale, sigma=sigma, sigma_next=sigma_next, clean=clean,
                     mask_tok=mask_tok, out=out, sigmas_dev=sigmas_dev, bf16_euler=bf16_euler)


def guided_euler_step(v_pos: torch.Tensor, v_neg: Optional[torch.Tensor], v_pert: Optional[torch.Tensor], latent: torch.Tensor,
                      cfg_scale: float, stg_scale: float, sigma: float, sigma_next: float, clean: Optional[torch.Tensor] = None,
                      mask_tok: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      sigmas_dev: Optional[torch.Tensor] = None, bf16_euler: bool = False) -> torch.Tensor:
    """``step_tail`` with plain CFG and the STG term of ``v_pert`` (None: the launch ``cfg_euler_step`` makes)."""
    return step_tail(v_pos, v_neg, v_pert, latent, cfg_scale=cfg_scale, stg_scale=stg_scale, sigma=sigma, sigma_next=sigma_next,
                     clean=clean, mask_tok=mask_tok, out=out, sigmas_dev=sigmas_dev, bf16_euler=bf16_euler)


def guider_euler_step(v_pos: torch.Tensor, v_neg: torch.Tensor, v_pert: Optional[torch.Tensor], latent: torch.Tensor,
                      record: torch.Tensor, guider: str, cfg_scale: float, stg_scale: float, sigma: float, sigma_next: float,
                      eta: float = 1.0, norm_threshold: float = 0.0, clean: Optional[torch.Tensor] = None,
                      mask_tok: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      sigmas_dev: Optional[torch.Tensor] = None, bf16_euler: bool = False) -> torch.Tensor:
    """``step_tail`` under the ``cfg_star`` / ``apg`` guider; plain CFG is ``cfg_euler_step``."""
    if guider == "cfg":
        raise ValueError("guider_euler_step: 'cfg' is not a guider id here (plain CFG is cfg_euler_step)")
    return step_tail(v_pos, v_neg, v_pert, latent, cfg_scale=cfg_scale, stg_scale=stg_scale, sigma=sigma, sigma_next=sigma_next,
                     guider=guider, record=record, eta=eta, norm_threshold=norm_threshold, clean=clean, mask_tok=mask_tok, out=out,
                     sigmas_dev=sigmas_dev, bf16_euler=bf16_euler)


def guidance_sums_workspace_bytes(B: int, C: int, S: int) -> int:
    """Bytes of the partial-sum workspace ``guidance_sums`` needs for (B,C,S) (ltxk_guidance_sums_workspace_bytes)."""
    n = int(_lib.load().ltxk_guidance_sums_workspace_bytes(B, C, S))
    if n < 0:
        raise ValueError(f"guidance_sums_workspace_bytes: bad shape B={B} C={C} S={S} (C must be a multiple of 8)")
    return n


def guidance_sums(v_pos: torch.Tensor, v_neg: torch.Tensor, latent: torch.Tensor, guider: str, sigma: float,
                  norm_threshold: float = 0.0, record: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                  sigmas_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-sample sums and derived scalars of the ``cfg_star`` / ``apg`` guider (ltxk_guidance_sums): v_* (B,S,C) tokens,
    latent (B,C,...) -> ``record`` (B,8) float32 in device memory (layout: include/ltxk.h), which ``step_tail`` reads.
    Deterministic (no atomics; the summation order depends on (C,S) only).  ``workspace``: a float32 device vector of at least
    ``guidance_sums_workspace_bytes`` bytes (allocated when None).  ``sigmas_dev``: sigma is read from device memory."""
    if guider == "cfg":
        raise ValueError("guidance_sums: 'cfg' is not a guider id here (plain CFG has no sums)")
    a = _step_tail_args("guidance_sums", v_pos, v_neg, None, latent, guider, 1.0, norm_threshold, None, None, sigmas_dev,
                        lambda B, C, S: (("record", record, F32, (B, GUIDER_RECORD_FLOATS), 4),
                                         ("workspace", workspace, F32, (-(guidance_sums_workspace_bytes(B, C, S) // 4),), 4)))
    if workspace is None:
        workspace = torch.empty((guidance_sums_workspace_bytes(a.B, a.C, a.S) // 4,), dtype=torch.float32, device=latent.device)
    if record is None:
        record = torch.empty((a.B, GUIDER_RECORD_FLOATS), dtype=torch.float32, device=latent.device)
    a.record, a.workspace, a.workspace_bytes = _p(record), _p(workspace), workspace.numel() * 4
    a.sigma = sigma
    check(_lib.load().ltxk_guidance_sums(ctypes.byref(a), _stream()), "ltxk_guidance_sums")
    return record


def attn_value_passthrough(vt: torch.Tensor, out: torch.Tensor, B: int, T: int, row_mask: int) -> torch.Tensor:
    """STG's skipped self-attention: rows b with bit b of ``row_mask`` set get out[b*T+t, :D] = vt[b, :, t] (bit-exact
    transpose of the (>= B, D, ld >= T) V^T buffer into the (>= B*T, >= D) token-major attention output).  Other rows untouched."""
    if not 0 <= int(row_mask) < (1 << 64):
        raise ValueError("attn_value_passthrough: row_mask must fit 64 bits")
    D = _dims("attn_value_passthrough", "vt", vt, BF16, 3)[1]
    _operands("attn_value_passthrough", ("vt", vt, BF16, (-B, D, -T), 16, True), ("out", out, BF16, (-(B * T), -D), 16, True))
    check(_lib.load().ltxk_attn_value_passthrough(_p(vt), vt.stride(1), _p(out), out.stride(0), B, D, T, int(row_mask), _stream()),
          "ltxk_attn_value_passthrough")
    return out


def step_scalars(ts_all: torch.Tensor, sig_all: torch.Tensor, step: torch.Tensor, ts: torch.Tensor, sig: torch.Tensor) -> None:
    """ts_all (steps,U) bf16, sig_all (steps,2) fp32, step (1) int32 -> ts (U), sig (2); step += 1 (device side)."""
    n, U = _dims("step_scalars", "ts_all", ts_all, BF16, 2)
    _operands("step_scalars", ("ts_all", ts_all, BF16, 2, 2), ("sig_all", sig_all, F32, (n, 2), 4), ("step", step, I32, (1,), 4),
              ("ts", ts, BF16, (U,), 2), ("sig", sig, F32, (2,), 4))
    check(_lib.load().ltxk_step_scalars(_p(ts_all), _p(sig_all), _p(step), _p(ts), _p(sig), U, n, _stream()), "ltxk_step_scalars")


def euler_only(latent: torch.Tensor, denoised: torch.Tensor, sigma: float, sigma_next: float) -> torch.Tensor:
    """out = bf16(x0 + sigma_next * (x - x0) / sigma) over two tensors of one shape; either is copied if not contiguous."""
    lat, den = latent.contiguous(), denoised.contiguous()
    _operands("euler_only", ("latent", lat, BF16, lat.dim(), 16), ("denoised", den, BF16, lat.shape, 16))
    out = torch.empty_like(lat)
    check(_lib.load().ltxk_euler_step(_p(lat), _p(den), _p(out), lat.numel(), sigma, sigma_next, _stream()), "ltxk_euler_step")
    return out


def resize_area(x: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """(..., H, W) fp32 / bf16 device tensor -> (..., oh, ow) bf16: cv2.INTER_AREA downscale of every (H,W) plane
    (prepare_video_for_encoding, utils.py:699-705).  An ``x`` that is not contiguous is copied first."""
    if x.dim() < 2:
        raise ValueError(f"resize_area: x must be (..., H, W), got {tuple(x.shape)}")
    x = x.contiguous()
    _operands("resize_area", ("x", x, F32 if x.dtype == F32 else BF16, x.dim(), 2))
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W)
    out = torch.empty(tuple(x.shape[:-2]) + (oh, ow), dtype=BF16, device=x.device)
    check(_lib.load().ltxk_resize_area(_p(x), int(x.dtype == torch.float32), _p(out), planes, H, W, oh, ow, _stream()), "ltxk_resize_area")
    return out


# ------------------------------------------------------------------------------------------- text stage (csrc/text_ops.hip, csrc/elementwise.hip)
STATS_PARTIALS = 64          # workgroups per (batch row, layer) of ltxk_masked_layer_stats' first stage
STATS_THREADS = 256          # threads of one of them; a thread keeps 8 running sums


def layer_stats_depth(count: int, D: int) -> int:
    """The longest chain of fp32 additions a term of ltxk_masked_layer_stats' sum passes through (include/ltxk.h): the
    running sum of a thread's element slot, then the fixed trees 8 slots -> 64 lanes -> 4 waves -> 64 partials."""
    rows = -(-count // STATS_PARTIALS)
    return -(-rows * (D // 8) // STATS_THREADS) + 3 + 6 + 2 + 6


def masked_layer_stats(x: torch.Tensor, row_start: torch.Tensor, row_count: torch.Tensor, valid_rows: Optional[int] = None) -> torch.Tensor:
    """ltxk_masked_layer_stats: x (L,B,T,D) bf16 (any layer / batch / row strides that are multiples of 8), row_start /
    row_count (B) int32 on the device -> (B,L,3) fp32 {sum, min, max} over rows [start, start+count) x D.
    ``valid_rows``: the sum of the counts, if the host knows it (the kernel timer's byte count; the kernel reads valid rows only)."""
    L, B, T, D = _dims("masked_layer_stats", "x", x, BF16, 4)
    _operands("masked_layer_stats", ("x", x, BF16, 4, 16, 8), ("row_start", row_start, I32, (B,), 4), ("row_count", row_count, I32, (B,), 4))
    partials = torch.empty((B * L, 3, STATS_PARTIALS), dtype=torch.float32, device=x.device)
    stats = torch.empty((B, L, 3), dtype=torch.float32, device=x.device)
    with _timed("text_layer_stats", 0.0, 2.0 * L * D * (B * T if valid_rows is None else valid_rows)):
        check(_lib.load().ltxk_masked_layer_stats(_p(x), x.stride(0), x.stride(1), x.stride(2), _p(row_start), _p(row_count),
                                                  L, B, T, D, _p(partials), _p(stats), _stream()), "ltxk_masked_layer_stats")
    return stats


def layer_norm_compact(x: torch.Tensor, row_start: torch.Tensor, row_count: torch.Tensor, row0: torch.Tensor,
                       stats: torch.Tensor, out: torch.Tensor, rows: int) -> torch.Tensor:
    """ltxk_layer_norm_compact: the valid rows of x (L,B,T,D), normalised with ``stats`` of ``masked_layer_stats``, into the
    first ``rows`` rows of out (>= rows, >= L*D) bf16, layer-major columns l*D + d; row0 (B) int32 = exclusive prefix sums of
    the counts, ``rows`` their total (the host knows both)."""
    L, B, T, D = _dims("layer_norm_compact", "x", x, BF16, 4)
    _operands("layer_norm_compact", ("x", x, BF16, 4, 16, 8), ("row_start", row_start, I32, (B,), 4), ("row_count", row_count, I32, (B,), 4),
              ("row0", row0, I32, (B,), 4), ("stats", stats, F32, (B, L, 3), 4), ("out", out, BF16, (-rows, -(L * D)), 16, True))
    with _timed("text_layer_norm", 0.0, 4.0 * rows * L * D):
        check(_lib.load().ltxk_layer_norm_compact(_p(x), x.stride(0), x.stride(1), x.stride(2), _p(row_start), _p(row_count),
                                                  _p(row0), _p(stats), _p(out), out.stride(0), L, B, T, D, rows, _stream()),
              "ltxk_layer_norm_compact")
    return out


def rmsnorm_rows(x: torch.Tensor, eps: float = 1e-6, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_rmsnorm_rows: unit-weight RMSNorm of the rows of x (M,D), any D % 8 == 0 up to 8192; row strides may exceed D."""
    M, D = _dims("rmsnorm_rows", "x", x, BF16, 2)
    _operands("rmsnorm_rows", ("x", x, BF16, 2, 16, True), ("out", out, BF16, (M, D), 16, True))
    if out is None:
        out = torch.empty((M, D), dtype=BF16, device=x.device)
    with _timed("rmsnorm_rows", 0.0, 4.0 * M * D):
        check(_lib.load().ltxk_rmsnorm_rows(_p(x), x.stride(0), _p(out), out.stride(0), M, D, eps, _stream()), "ltxk_rmsnorm_rows")
    return out


def qknorm_rope_1d(buf: torch.Tensor, D: int, weight: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, T: int, H: int,
                   eps: float = 1e-6) -> torch.Tensor:
    """ltxk_qknorm_rope_1d: in place on columns [0, 2D) of buf (M, ld >= 2D): q | k RMSNorm over the full D with weight (2,D),
    then split RoPE with cos / sin (H,T,64) fp32; any H >= 1 with D == 128*H."""
    M = _dims("qknorm_rope_1d", "buf", buf, BF16, 2)[0]
    _operands("qknorm_rope_1d", ("buf", buf[:, :2 * D], BF16, (M, 2 * D), 16, True), ("weight", weight, BF16, (2, D), 16),
              ("cos", cos, F32, (H, T, 64), 16), ("sin", sin, F32, (H, T, 64), 16))
    with _timed("qknorm_rope_1d", 0.0, 8.0 * M * D + 8.0 * M * D):
        check(_lib.load().ltxk_qknorm_rope_1d(_p(buf), buf.stride(0), M, D, _p(weight), _p(cos), _p(sin), T, H, eps,
                                              _stream()), "ltxk_qknorm_rope_1d")
    return buf


def gelu_erf_(x: torch.Tensor) -> torch.Tensor:
    """ltxk_gelu_erf: exact (erf) GELU in place on a contiguous bf16 tensor."""
    _operands("gelu_erf_", ("x", x, BF16, x.dim(), 16))
    with _timed("gelu_erf", 0.0, 4.0 * x.numel()):
        check(_lib.load().ltxk_gelu_erf(_p(x), x.numel(), _stream()), "ltxk_gelu_erf")
    return x


def connector_assemble(feat: Optional[torch.Tensor], registers: torch.Tensor, row0: torch.Tensor, row_count: torch.Tensor,
                       B: int, T: int) -> torch.Tensor:
    """ltxk_connector_assemble: (B,T,D) connector input - batch row b's first row_count[b] rows are rows row0[b]... of feat
    (rows, D), the rest registers[t % R].  ``feat`` may be None when every count is 0."""
    R, D = _dims("connector_assemble", "registers", registers, BF16, 2)
    _operands("connector_assemble", ("feat", feat, BF16, (feat.shape[0], D) if feat is not None and feat.dim() == 2 else (-1, D), 16, True),
              ("registers", registers, BF16, 2, 16), ("row0", row0, I32, (B,), 4), ("row_count", row_count, I32, (B,), 4))
    rows, ldf = (feat.shape[0], feat.stride(0)) if feat is not None else (0, 0)
    out = torch.empty((B, T, D), dtype=BF16, device=registers.device)
    with _timed("connector_assemble", 0.0, 4.0 * B * T * D):
        check(_lib.load().ltxk_connector_assemble(_p(feat) if rows else None, ldf, _p(registers), _p(row0), _p(row_count), _p(out),
                                                  B, T, D, R, rows, _stream()), "ltxk_connector_assemble")
    return out


# ------------------------------------------------------------------- Gemma-3 text encoder (csrc/text_ops.hip, csrc/causal_attn.hip)
GEMMA_HEAD_DIM = 256
GEMMA_ROWS_PER_WG = 4        # rows (waves) per workgroup of ltxk_rmsnorm_weight_rows
CAUSAL_ATTN_BQ = 64          # query rows per workgroup of ltxk_causal_attn
CAUSAL_ATTN_BK = 64          # keys per tile


def embed_rows(table: torch.Tensor, ids: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None,
               ids_host: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None, trusted_ids: bool = False) -> torch.Tensor:
    """ltxk_embed_rows: out[m,:] = bf16(table[ids[m],:] * scale).  table (V,D) contiguous bf16, ids (M) int32 on the device.
    The kernel cannot raise for device data, so the id range is validated here on ``ids_host``, the host copy the caller
    tokenised (without one, ``ids`` is copied back once - a synchronisation, once per prompt).
    A ``float8_e4m3fn`` table (D % 16 == 0) takes ltxk_embed_rows_fp8: out[m,:] = bf16((table[ids[m],:] * row_scale[ids[m]]) *
    scale) with ``row_scale`` (V) fp32, or bf16(table[ids[m],:] * scale) without one - the bf16 call on the widened table.
    ``trusted_ids``: the ids come from a kernel that only emits ids in [0, V) (``sample_rows``): the host range check and its
    copy-back are skipped, so that the call neither synchronises nor breaks a graph capture."""
    f8 = table.dtype == FP8
    if row_scale is not None and not f8:
        raise TypeError("embed_rows: row_scale goes with a float8_e4m3fn table")
    tdt = FP8 if f8 else BF16
    V, D = _dims("embed_rows", "table", table, tdt, 2)
    M = _dims("embed_rows", "ids", ids, I32, 1)[0]
    if f8 and D % 16:
        raise ValueError(f"embed_rows: a float8_e4m3fn table must have rows of a multiple of 16 elements, got {D}")
    _operands("embed_rows", ("table", table, tdt, 2, 16), ("ids", ids, I32, 1, 4), ("out", out, BF16, (M, D), 16, True),
              ("row_scale", row_scale, F32, (V,), 4))
    if not trusted_ids:
        host = ids.cpu() if ids_host is None else ids_host.reshape(-1)
        if host.numel() != M:
            raise ValueError(f"embed_rows: ids_host holds {host.numel()} ids, ids {M}")
        if M and (int(host.min()) < 0 or int(host.max()) >= V):
            raise ValueError(f"embed_rows: token ids must lie in [0, {V}), got [{int(host.min())}, {int(host.max())}]")
    if out is None:
        out = torch.empty((M, D), dtype=BF16, device=table.device)
    if f8:
        with _timed("embed_rows_fp8", 0.0, 3.0 * M * D):
            check(_lib.load().ltxk_embed_rows_fp8(_p(table), _p(row_scale), V, D, _p(ids), _p(out), out.stride(0), M, scale, _stream()),
                  "ltxk_embed_rows_fp8")
        return out
    with _timed("embed_rows", 0.0, 4.0 * M * D):
        check(_lib.load().ltxk_embed_rows(_p(table), V, D, _p(ids), _p(out), out.stride(0), M, scale, _stream()), "ltxk_embed_rows")
    return out


def rmsnorm_weight_rows(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, resid: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_rmsnorm_weight_rows: Gemma RMSNorm, y = bf16(x * rsqrt(mean(x^2) + eps) * (1 + weight)); with ``resid``
    y = bf16(resid + that).  x (M,D), any D % 8 == 0 up to 8192, row strides may exceed D; ``out`` may be ``resid`` or ``x``."""
    M, D = _dims("rmsnorm_weight_rows", "x", x, BF16, 2)
    _operands("rmsnorm_weight_rows", ("x", x, BF16, 2, 16, True), ("weight", weight, BF16, (D,), 16),
              ("resid", resid, BF16, (M, D), 16, True), ("out", out, BF16, (M, D), 16, True))
    if out is None:
        out = torch.empty((M, D), dtype=BF16, device=x.device)
    with _timed("rmsnorm_weight_rows", 0.0, (4.0 if resid is None else 6.0) * M * D):
        check(_lib.load().ltxk_rmsnorm_weight_rows(_p(x), x.stride(0), _p(weight), _p(resid), resid.stride(0) if resid is not None else 0,
                                                   _p(out), out.stride(0), M, D, eps, _stream()), "ltxk_rmsnorm_weight_rows")
    return out


def headnorm_rope(buf: torch.Tensor, Hq: int, Hkv: int, q_weight: torch.Tensor, k_weight: torch.Tensor, cos: torch.Tensor,
                  sin: torch.Tensor, T: int, eps: float = 1e-6, *, pos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_headnorm_rope: in place on columns [0, (Hq+Hkv)*256) of buf (M, ld): per 256-wide head Gemma RMSNorm with
    q_weight / k_weight (256,), then rotate-half RoPE with cos / sin (T,128) fp32, row m at position m % T.
    ``pos`` (ltxk_headnorm_rope_at): an int32 device tensor of one element; every row then takes table row ``pos[0]`` - the bits
    of the call on ``cos[p:p+1]``, ``sin[p:p+1]`` with T = 1 - and a position outside [0, T) stores nothing."""
    if Hq < 1 or Hkv < 1:
        raise ValueError(f"headnorm_rope: Hq = {Hq} and Hkv = {Hkv} must be positive")
    cols, HD = (Hq + Hkv) * GEMMA_HEAD_DIM, GEMMA_HEAD_DIM
    M = _dims("headnorm_rope", "buf", buf, BF16, 2)[0]
    _operands("headnorm_rope", ("buf", buf[:, :cols], BF16, (M, cols), 16, True), ("q_weight", q_weight, BF16, (HD,), 16),
              ("k_weight", k_weight, BF16, (HD,), 16), ("cos", cos, F32, (T, HD // 2), 16), ("sin", sin, F32, (T, HD // 2), 16),
              ("pos", pos, I32, (1,), 4))
    if pos is not None:
        with _timed("headnorm_rope", 0.0, 4.0 * M * cols):
            check(_lib.load().ltxk_headnorm_rope_at(_p(buf), buf.stride(0), M, Hq, Hkv, _p(q_weight), _p(k_weight), _p(cos), _p(sin),
                                                    T, _p(pos), eps, _stream()), "ltxk_headnorm_rope_at")
        return buf
    with _timed("headnorm_rope", 0.0, 4.0 * M * cols):
        check(_lib.load().ltxk_headnorm_rope(_p(buf), buf.stride(0), M, Hq, Hkv, _p(q_weight), _p(k_weight), _p(cos), _p(sin),
                                             T, eps, _stream()), "ltxk_headnorm_rope")
    return buf


def geglu_tanh_(gu: torch.Tensor) -> torch.Tensor:
    """ltxk_geglu_tanh in place: gu = [g | u] (M, 2F) -> its first F columns become bf16(bf16(gelu_tanh(g)) * u); returns that
    (M,F) view (row stride 2F: ``gemm`` takes it as ``a``)."""
    M, F2 = _dims("geglu_tanh_", "gu", gu, BF16, 2)
    if F2 % 16:
        raise ValueError(f"geglu_tanh_: gu must be (M, 2F) with F a multiple of 8, got {tuple(gu.shape)}")
    _operands("geglu_tanh_", ("gu", gu, BF16, 2, 16, True))
    F = F2 // 2
    with _timed("geglu_tanh", 0.0, 6.0 * M * F):
        check(_lib.load().ltxk_geglu_tanh(_p(gu), gu.stride(0), _p(gu), gu.stride(0), M, F, _stream()), "ltxk_geglu_tanh")
    return gu[:, :F]


CAUSAL_ATTN_STEP_SLICE = 256  # keys per workgroup of ltxk_causal_attn_step
CAUSAL_ATTN_STEP_PART = 258   # floats of one partial: M, l, O[256]


def causal_attn_step_slices(max_step: int, window: int = 0) -> int:
    """256-key slices per (batch row, head) of a ``causal_attn(step=<device tensor>, max_step=)`` launch: the most any step up to
    ``max_step`` touches - under a window no more than a window of keys can reach."""
    n = max_step // CAUSAL_ATTN_STEP_SLICE + 1
    return min(n, (window + CAUSAL_ATTN_STEP_SLICE - 2) // CAUSAL_ATTN_STEP_SLICE + 1) if window else n


def causal_attn(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, row_start: torch.Tensor, B: int, Hq: int,
                Hkv: int, T: int, scale: float, window: int = 0, *, step: Union[int, torch.Tensor, None] = None,
                k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None, partials: Optional[torch.Tensor] = None,
                max_step: Optional[int] = None) -> torch.Tensor:
    """ltxk_causal_attn (head dim 256): q (B*T, >= Hq*256) view, k (B*T, >= Hkv*256) view, vt (B, Hkv*256, ldvt >= T),
    out (B*T, >= Hq*256) view, row_start (B) int32 on the device (valid tokens of batch row b: [row_start[b], T)).  Key j is
    visible to query i iff row_start <= j <= i and (window == 0 or i - j < window); rows below row_start come out zero.

    With ``step`` (ltxk_causal_attn_step): one query position per batch row against a KV cache.  ``k`` / ``vt`` are the cache in
    the same layouts with T its capacity (a multiple of 64), q / out are (B, >= Hq*256) rows, ``k_new`` / ``v_new`` (B, >= Hkv*256)
    the step's rotated key and its value - read in the place of cache position ``step`` and stored there by the launch - and
    ``partials`` a caller-owned fp32 buffer of at least B * Hq * slices * CAUSAL_ATTN_STEP_PART floats, the 256-key slices of a
    launch being [s0, step/256] with s0 = max(0, step - window + 1) / 256 under a window, else 0 (B * Hq * ceil(T/256) * 258
    floats serve every step).  Key j is visible iff row_start <= j <= step and (window == 0 or step - j < window).

    ``step`` an int32 device tensor of one element (ltxk_causal_attn_dev_step), with ``max_step`` in [0, T): the position is read
    on the device, the launch is sized for ``max_step`` and ``partials`` holds B * Hq * ``causal_attn_step_slices(max_step,
    window)`` * 258 floats.  For step[0] == s the bits are those of ``step=s``, whatever ``max_step`` >= s is; step[0] outside
    [0, max_step] leaves the cache, ``partials`` and ``out`` as they were."""
    nq, nkv = Hq * GEMMA_HEAD_DIM, Hkv * GEMMA_HEAD_DIM
    if step is None:
        if k_new is not None or v_new is not None or partials is not None:
            raise ValueError("causal_attn: k_new, v_new and partials belong to the step form (step=)")
        _operands("causal_attn", ("q", q, BF16, (B * T, -nq), 16, True), ("k", k, BF16, (B * T, -nkv), 16, True),
                  ("vt", vt, BF16, (B, nkv, -T), 16, True), ("out", out, BF16, (B * T, -nq), 16, True), ("row_start", row_start, I32, (B,), 4))
        a = CausalAttnArgs()
        a.q, a.k, a.vt, a.out, a.row_start = _p(q), _p(k), _p(vt), _p(out), _p(row_start)
        a.ldq, a.ldk, a.ldvt, a.ldo = q.stride(0), k.stride(0), vt.stride(1), out.stride(0)
        a.B, a.Hq, a.Hkv, a.T, a.window, a.scale = B, Hq, Hkv, T, window, scale
        with _timed("causal_attn", 2.0 * B * Hq * T * T * GEMMA_HEAD_DIM, 2.0 * B * T * GEMMA_HEAD_DIM * (2 * Hq + 2 * Hkv)):
            check(_lib.load().ltxk_causal_attn(ctypes.byref(a), _stream()), "ltxk_causal_attn")
        return out
    missing = [n for n, t in (("k_new", k_new), ("v_new", v_new), ("partials", partials)) if t is None]
    if missing:
        raise ValueError(f"causal_attn: the step form needs {', '.join(missing)}")
    if B < 1 or Hq < 1 or Hkv < 1 or Hq % Hkv or Hq // Hkv > 16:
        raise ValueError(f"causal_attn: the step form takes Hq = {Hq} a multiple of Hkv = {Hkv}, at most 16 times it")
    if T < 1 or T % CAUSAL_ATTN_BK:
        raise ValueError(f"causal_attn: the cache capacity T = {T} must be a positive multiple of {CAUSAL_ATTN_BK}")
    dev = isinstance(step, torch.Tensor)
    if dev != (max_step is not None):
        raise ValueError("causal_attn: max_step goes with a device tensor as step, and such a step needs it")
    top = max_step if dev else step
    if not 0 <= top < T:
        raise ValueError(f"causal_attn: {'max_step' if dev else 'step'} = {top} must lie in [0, {T}), the cache capacity")
    if window < 0:
        raise ValueError(f"causal_attn: window = {window} must be 0 (none) or a positive count")
    if dev:
        need = B * Hq * causal_attn_step_slices(max_step, window) * CAUSAL_ATTN_STEP_PART
    else:
        s0 = max(0, step - window + 1) // CAUSAL_ATTN_STEP_SLICE if window else 0
        need = B * Hq * (step // CAUSAL_ATTN_STEP_SLICE + 1 - s0) * CAUSAL_ATTN_STEP_PART
    _operands("causal_attn", ("q", q, BF16, (B, -nq), 16, True), ("k", k, BF16, (B * T, -nkv), 16, True),
              ("vt", vt, BF16, (B, nkv, -T), 16, True), ("out", out, BF16, (B, -nq), 16, True), ("row_start", row_start, I32, (B,), 4),
              ("k_new", k_new, BF16, (B, -nkv), 16, True), ("v_new", v_new, BF16, (B, -nkv), 16, True),
              ("partials", partials, F32, (-need,), 16), ("step", step if dev else None, I32, (1,), 4))
    live = min(top + 1, window) if window else top + 1
    if dev:
        with _timed("causal_attn_step", 4.0 * B * Hq * live * GEMMA_HEAD_DIM, 4.0 * B * Hkv * live * GEMMA_HEAD_DIM):
            check(_lib.load().ltxk_causal_attn_dev_step(_p(q), q.stride(0), _p(k_new), k_new.stride(0), _p(v_new), v_new.stride(0), _p(k),
                                                        k.stride(0), _p(vt), vt.stride(1), _p(out), out.stride(0), _p(row_start), B, Hq, Hkv, T,
                                                        _p(step), max_step, window, scale, _p(partials), partials.numel(), _stream()),
                  "ltxk_causal_attn_dev_step")
        return out
    with _timed("causal_attn_step", 4.0 * B * Hq * live * GEMMA_HEAD_DIM, 4.0 * B * Hkv * live * GEMMA_HEAD_DIM):
        check(_lib.load().ltxk_causal_attn_step(_p(q), q.stride(0), _p(k_new), k_new.stride(0), _p(v_new), v_new.stride(0), _p(k), k.stride(0),
                                                _p(vt), vt.stride(1), _p(out), out.stride(0), _p(row_start), B, Hq, Hkv, T, step, window,
                                                scale, _p(partials), partials.numel(), _stream()), "ltxk_causal_attn_step")
    return out


SAMPLE_CHUNK = 2048           # logits per workgroup of ltxk_sample_rows: the chunks partial maxima and sums are merged over
SAMPLE_DEPTH_BASE = 17        # sequential fp32 additions behind a prefix sum inside a chunk; one more per chunk (csrc/sample.hip)
SAMPLE_MAX_B, SAMPLE_MAX_CTX, SAMPLE_MAX_EOS = 8, 64, 8


def sample_depth(V: int) -> int:
    """The longest sequential fp32 addition chain behind a prefix sum of ltxk_sample_rows over V logits."""
    return SAMPLE_DEPTH_BASE + -(-V // SAMPLE_CHUNK)


def sample_workspace_floats(B: int, V: int) -> int:
    """fp32 elements of ``sample_rows``' workspace: per row and chunk a maximum, its index and a sum."""
    return 3 * B * -(-V // SAMPLE_CHUNK)


def sample_rows(logits, ctl, done, next_ids, history, hist_len, tokens_out, eos, uniforms, workspace, *, temperature: float,
                penalty: float = 1.0, rep_ctx: int = 0, draw: bool = True, advance: bool = True) -> None:
    """ltxk_sample_rows: one token per row of ``logits`` (B, V) bf16 (rows with unit inner stride; 1 <= B <= 8, V % 8 == 0)
    against the decode state on the device - every operand a tensor: ``ctl`` (3) = {n, pos, live}, ``done`` (B), ``next_ids`` (B),
    ``history`` (B, Hcap) with ``hist_len`` (B), ``tokens_out`` (B, Nmax), ``eos`` (n_eos <= 8), all int32; ``uniforms`` (Nmax, B)
    fp32 in [0, 1) (None at temperature 0); ``workspace`` fp32 of at least ``sample_workspace_floats(B, V)`` elements.
    ``draw``: the repetition penalty over the last ``rep_ctx`` <= 64 ids of the row's history (a set), then the smallest argmax
    at ``temperature`` 0, else the inverse CDF of softmax(l' / temperature) at uniforms[n, b], then the bookkeeping (include/ltxk.h).
    ``advance``: ctl = {n + 1, pos + 1, rows not done}, a launch of its own behind the draw - a decode step draws first
    (``advance=False``), feeds ``next_ids`` at ctl's pos and advances last (``draw=False``).  n >= Nmax: nothing is stored.
    (The tensor parameters carry no annotation: tests/test_ops_shims_cpu.py finds the shims of its closed table by their annotated
    tensor parameters.  This shim's refusals, operand by operand, are in tests/test_gemma_sample_cpu.py.)"""
    if not (draw or advance):
        raise ValueError("sample_rows: neither draw nor advance")
    if not isinstance(logits, torch.Tensor) or not isinstance(tokens_out, torch.Tensor):
        raise TypeError("sample_rows: logits and tokens_out must be tensors")
    B, V = _dims("sample_rows", "logits", logits, BF16, 2)
    Nmax = _dims("sample_rows", "tokens_out", tokens_out, I32, 2)[1]
    Hcap = _dims("sample_rows", "history", history, I32, 2)[1]
    n_eos = _dims("sample_rows", "eos", eos, I32, 1)[0]
    if not 1 <= B <= SAMPLE_MAX_B or V < 8 or V % 8 or logits.stride(0) % 8:
        raise ValueError(f"sample_rows: logits must be (B, V) with 1 <= B <= {SAMPLE_MAX_B}, V a positive multiple of 8 and rows a "
                         f"multiple of 8 elements apart, got {tuple(logits.shape)} with strides {logits.stride()}")
    if Nmax < 1 or Hcap < 1 or n_eos > SAMPLE_MAX_EOS:
        raise ValueError(f"sample_rows: tokens_out (B, Nmax >= 1), history (B, Hcap >= 1) and eos (<= {SAMPLE_MAX_EOS}), got Nmax = {Nmax}, "
                         f"Hcap = {Hcap}, {n_eos} eos ids")
    if not 0 <= rep_ctx <= SAMPLE_MAX_CTX:
        raise ValueError(f"sample_rows: rep_ctx = {rep_ctx} must lie in [0, {SAMPLE_MAX_CTX}]")
    if not (0.0 <= temperature < math.inf and 0.0 < penalty < math.inf):
        raise ValueError(f"sample_rows: temperature = {temperature} must be >= 0 and penalty = {penalty} positive, both finite")
    if temperature > 0 and uniforms is None:
        raise ValueError("sample_rows: temperature > 0 needs uniforms")
    _operands("sample_rows", ("logits", logits, BF16, (B, V), 16, True), ("ctl", ctl, I32, (3,), 4), ("done", done, I32, (B,), 4),
              ("next_ids", next_ids, I32, (B,), 4), ("history", history, I32, (B, Hcap), 4), ("hist_len", hist_len, I32, (B,), 4),
              ("tokens_out", tokens_out, I32, (B, Nmax), 4), ("eos", eos, I32, (n_eos,), 4), ("uniforms", uniforms, F32, (Nmax, B), 4),
              ("workspace", workspace, F32, (-sample_workspace_floats(B, V),), 4))
    a = SampleArgs()
    a.struct_bytes = ctypes.sizeof(SampleArgs)
    a.B, a.V, a.ld, a.n_max, a.hist_cap, a.rep_ctx, a.n_eos = B, V, logits.stride(0), Nmax, Hcap, rep_ctx, n_eos
    a.flags = (_lib.SAMPLE_DRAW if draw else 0) | (_lib.SAMPLE_ADVANCE if advance else 0)
    a.temperature, a.penalty = temperature, penalty
    a.logits, a.ctl, a.done, a.next_ids, a.history, a.hist_len = _p(logits), _p(ctl), _p(done), _p(next_ids), _p(history), _p(hist_len)
    a.tokens_out, a.eos, a.uniforms, a.workspace, a.workspace_bytes = _p(tokens_out), _p(eos) if n_eos else None, _p(uniforms), _p(workspace), workspace.numel() * 4
    with _timed("sample_rows", 0.0, (2.0 if temperature == 0 else 4.0) * B * V if draw else 0.0):
        check(_lib.load().ltxk_sample_rows(ctypes.byref(a), _stream()), "ltxk_sample_rows")


# ------------------------------------------------------------------- step cache of the denoise loop (csrc/step_cache.hip)
STEP_CACHE_CHUNK = 8192       # elements per workgroup of ltxk_step_cache_probe: the chunks its partial sums are merged over
STEP_CACHE_DEPTH_BASE = 40    # sequential fp32 additions behind a chunk's partial; one more per further chunk


def _step_cache_chunks(who: str, rows: int, D: int) -> int:
    rows, D = int(rows), int(D)
    if rows < 1 or D < 8 or D % 8 or rows * D > 1 << 35:
        raise ValueError(f"{who}: rows = {rows} must be positive, D = {D} a positive multiple of 8 and rows * D at most 2^35")
    return -(-rows * D // STEP_CACHE_CHUNK)


def step_cache_workspace_bytes(rows: int, D: int) -> int:
    """Bytes of the partial-sum workspace ``step_cache_probe`` needs for (rows, D) (ltxk_step_cache_workspace_bytes; a size
    function: it hands the library no tensor)."""
    n = 8 * _step_cache_chunks("step_cache_workspace_bytes", rows, D)
    lib = _lib.load()
    if lib.ltxk_step_cache_workspace_bytes(int(rows), int(D)) != n:
        raise _lib.LtxkError("step_cache_workspace_bytes: the library cuts (rows, D) into other chunks than this binding; rebuild it")
    return n


def step_cache_depth(rows: int, D: int) -> int:
    """The longest sequential fp32 addition chain behind a sum of ltxk_step_cache_probe over (rows, D) (ltxk_step_cache_depth)."""
    d = STEP_CACHE_DEPTH_BASE + _step_cache_chunks("step_cache_depth", rows, D) - 1
    lib = _lib.load()
    if lib.ltxk_step_cache_depth(int(rows), int(D)) != d:
        raise _lib.LtxkError("step_cache_depth: the library sums (rows, D) in another order than this binding; rebuild it")
    return d


def step_cache_probe(cur, prev, sums, workspace, *, init: bool = False) -> None:
    """ltxk_step_cache_probe: ``cur``, ``prev`` (rows, D) bf16, contiguous, 16-byte aligned, D % 8 == 0.  One pass:
    sums[0] = sum |cur - prev|, sums[1] = sum |prev| (``sums`` (2,) fp32 on the device, ``prev`` as it was on entry), and
    prev <- cur.  The summation order depends on (rows, D) alone (csrc/step_cache.hip); ``workspace``: fp32 of at least
    ``step_cache_workspace_bytes(rows, D) // 4`` elements.  ``init``: the copy alone - ``sums`` and ``workspace`` are not touched
    and may be None.  (No tensor annotations, as ``sample_rows``; the refusals are in tests/test_step_cache_cpu.py.)"""
    who = "step_cache_probe"
    if not isinstance(cur, torch.Tensor) or not isinstance(prev, torch.Tensor):
        raise TypeError(f"{who}: cur and prev must be tensors")
    rows, D = _dims(who, "cur", cur, BF16, 2)
    nws = 2 * _step_cache_chunks(who, rows, D)
    if not init and (sums is None or workspace is None):
        raise ValueError(f"{who}: sums and workspace are required unless init")
    _operands(who, ("cur", cur, BF16, (rows, D), 16), ("prev", prev, BF16, (rows, D), 16), ("sums", sums, F32, (2,), 4),
              ("workspace", workspace, F32, (-nws,), 4))
    if cur.data_ptr() == prev.data_ptr():
        raise ValueError(f"{who}: cur and prev must be two buffers")
    with _timed(who, 0.0 if init else 5.0 * rows * D, (4.0 if init else 6.0) * rows * D):
        check(_lib.load().ltxk_step_cache_probe(_p(cur), _p(prev), rows, D, _lib.PROBE_INIT if init else 0, _p(sums), _p(workspace),
                                                0 if workspace is None else workspace.numel() * 4, _stream()), "ltxk_step_cache_probe")


def _residual_operands(who: str, x, r) -> tuple:
    """The two operands of a residual shim, once ``x`` fixes the shape: bf16, a positive multiple of 8 elements."""
    if not isinstance(x, torch.Tensor) or not isinstance(r, torch.Tensor):
        raise TypeError(f"{who}: x and r must be tensors")
    shape = x.shape
    _dims(who, "x", x, BF16, len(shape))
    if x.numel() < 8 or x.numel() % 8:
        raise ValueError(f"{who}: x must hold a positive multiple of 8 elements, got shape {tuple(shape)}")
    return ("x", x, BF16, shape, 16), ("r", r, BF16, shape, 16)


def residual_store(x, r) -> None:
    """ltxk_residual_store: r <- rbf(f32(x) - f32(r)) in place, x and r bf16 of one shape, contiguous, 16-byte aligned,
    numel % 8 == 0.  On entry ``r`` holds the copy of the residual stream taken in front of block 0, ``x`` the stream behind the
    last block.  (No tensor annotations, as ``sample_rows``.)"""
    _operands("residual_store", *_residual_operands("residual_store", x, r))
    if x.data_ptr() == r.data_ptr():
        raise ValueError("residual_store: x and r must be two buffers")
    n = x.numel()
    with _timed("residual_store", float(n), 6.0 * n):
        check(_lib.load().ltxk_residual_store(_p(x), _p(r), n, _stream()), "ltxk_residual_store")


def residual_apply(x, r) -> None:
    """ltxk_residual_apply: x <- rbf(f32(x) + f32(r)) in place; operands as ``residual_store``."""
    _operands("residual_apply", *_residual_operands("residual_apply", x, r))
    if x.data_ptr() == r.data_ptr():
        raise ValueError("residual_apply: x and r must be two buffers")
    n = x.numel()
    with _timed("residual_apply", float(n), 6.0 * n):
        check(_lib.load().ltxk_residual_apply(_p(x), _p(r), n, _stream()), "ltxk_residual_apply")


# ------------------------------------------------------------------- VAE / upsampler (csrc/conv3d.hip, csrc/vae_ops.hip)
# Volumes are channels-last (B,D,H,W,C) bf16, a voxel one contiguous row.
PAD_ZEROS, PAD_REFLECT = 0, 1


def _taps_geometry(who: str, kernel, dilation: int, pad) -> tuple:
    """(kh, kw, dil, (top, bottom, left, right)) of a ``kernel=`` call, refused where ltxk_conv_taps_bf16 would refuse it."""
    kh, kw = (int(k) for k in kernel)
    dil = int(dilation)
    if not (1 <= kh <= 16 and kw in (1, 3) and 1 <= dil <= 8):
        raise ValueError(f"{who}: kernel=({kh},{kw}) dilation={dil}: needs kh in [1,16], kw 1 or 3, dilation in [1,8]")
    if pad is None or len(pad) != 4:
        raise ValueError(f"{who}: kernel= needs pad=(top, bottom, left, right)")
    pt, pb, pl_, pr = (int(v) for v in pad)
    if min(pt, pb, pl_, pr) < 0 or pt + pb != (kh - 1) * dil or pl_ + pr != kw - 1:
        raise ValueError(f"{who}: pad={tuple(pad)} must sum to ((kh-1)*dilation, kw-1) = ({(kh - 1) * dil}, {kw - 1}): the output extent is the input's")
    return kh, kw, dil, (pt, pb, pl_, pr)


def _conv_taps(x, w, b, resid, keep_out, kernel, dilation, pad, mean_with, leaky, tanh_out):
    """The ``kernel=`` form of ``conv3d``: ltxk_conv_taps_bf16 (include/ltxk.h has the sum and the epilogue's rounding order)."""
    who = "conv3d"
    B, D, H, W, Cin = _dims(who, "x", x, BF16, 5)
    kh, kw, dil, (pt, pb, pl_, pr) = _taps_geometry(who, kernel, dilation, pad)
    Cout = w.shape[0]
    if tuple(w.shape[1:]) != (kh, kw, Cin):
        raise ValueError(f"{who}: weight {tuple(w.shape)} does not match kernel=({kh},{kw}) and Cin={Cin}")
    if Cin != 32 and Cin % 64:
        raise ValueError(f"{who}: Cin={Cin} must be 32 or a multiple of 64 (pad channels with zeros)")
    mean_with = tuple(mean_with) if mean_with is not None else ()
    if len(mean_with) > 2:
        raise ValueError(f"{who}: mean_with takes one or two tensors, got {len(mean_with)}")
    if tanh_out and (resid is not None or mean_with or leaky is not None):
        raise ValueError(f"{who}: tanh_out is the final form: no resid, mean_with or leaky")
    if not tanh_out and leaky is None and not keep_out:
        raise ValueError(f"{who}: keep_out=False leaves no output without leaky=")
    oshape = (B, D, H, W, Cout)
    ra = 16 if Cout % 8 == 0 else 8 if Cout % 4 == 0 else 2
    a1, a2 = (mean_with + (None, None))[:2]
    _operands(who, ("x", x, BF16, 5, 16), ("w", w, BF16, (Cout, kh, kw, Cin), 16), ("bias", b, BF16, (Cout,), 2),
              ("resid", resid, BF16, oshape, ra), ("mean_with[0]", a1, BF16, oshape, ra), ("mean_with[1]", a2, BF16, oshape, ra))
    dev = x.device
    a = ConvTapsArgs()
    a.struct_bytes = ctypes.sizeof(ConvTapsArgs)
    a.B, a.D, a.H, a.W, a.Cin, a.Cout = B, D, H, W, Cin, Cout
    a.kh, a.kw, a.dil_h = kh, kw, dil
    a.pad_top, a.pad_bottom, a.pad_left, a.pad_right = pt, pb, pl_, pr
    a.x, a.w, a.bias, a.resid, a.mean_a1, a.mean_a2 = _p(x), _p(w), _p(b), _p(resid), _p(a1), _p(a2)
    a.n_mean = len(mean_with) + 1 if mean_with else 0
    a.zero_page = _p(_scratch("zero_page", dev))
    ws = _scratch("conv_splitk", dev)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel() * 4
    out = act_out = None
    if tanh_out:
        out = torch.empty(oshape, dtype=F32, device=dev)
        a.out_f32 = _p(out)
    else:
        if keep_out:
            out = torch.empty(oshape, dtype=BF16, device=dev)
            a.out = _p(out)
        if leaky is not None:
            act_out = torch.empty(oshape, dtype=BF16, device=dev)
            a.act_out, a.slope = _p(act_out), float(leaky)
    V = B * D * H * W
    with _timed("conv_taps", 2.0 * kh * kw * Cin * Cout * V, 2.0 * V * (Cin + Cout) + 2.0 * kh * kw * Cin * Cout):
        check(_lib.load().ltxk_conv_taps_bf16(ctypes.byref(a), _stream()), "ltxk_conv_taps_bf16")
    return out if leaky is None else (out, act_out)


def conv3d(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, causal: bool, pad_mode: int,
           resid: Optional[torch.Tensor] = None, act: Optional[dict] = None, keep_out: bool = True, *,
           kernel: Optional[Tuple[int, int]] = None, dilation: int = 1, pad: Optional[Tuple[int, int, int, int]] = None,
           mean_with=None, leaky: Optional[float] = None, tanh_out: bool = False):
    """x (B,D,H,W,Cin) bf16 channels-last; w (Cout,3,3,3,Cin), or (Cout,3,3,Cin) for a per-frame 3x3 kernel;
    returns (B,D,H,W,Cout).  ``act`` = dict(eps, silu, scale, shift): the PixelNorm (+ modulation) + SiLU that follows
    this conv is applied to its output rows in the epilogue (Cout 128 / 256) and returned as a second tensor:
    ``(out, act_out)``; ``keep_out=False`` skips the raw output (``out`` is None) when nothing else reads it.

    With ``kernel=(kh, kw)`` (ltxk_conv_taps_bf16: the audio decoder's causal 3x3 and the vocoder's dilated convolutions):
    w (Cout,kh,kw,Cin), each (H,W) frame convolved on its own with ``dilation`` along H and explicit zero halos
    ``pad=(top, bottom, left, right)`` that keep the extent; ``causal`` / ``pad_mode`` / ``act`` do not apply (pad_mode must
    be PAD_ZEROS).  y = bf16(conv + bias), then bf16(y + resid), then with ``mean_with=(a1[, a2])`` bf16((y + a1 [+ a2]) / n);
    ``leaky=slope`` returns ``(out, max(y, bf16(y * slope)))`` (``keep_out=False``: out None); ``tanh_out=True`` returns
    tanh(conv + bias) in float32, never rounded to bf16.  Cin 32 or a multiple of 64, any Cout."""
    if kernel is not None:
        if act is not None or pad_mode != PAD_ZEROS:
            raise ValueError("conv3d: kernel= takes explicit zero halos (pad=): no act, pad_mode must be PAD_ZEROS")
        return _conv_taps(x, w, b, resid, keep_out, kernel, dilation, pad, mean_with, leaky, tanh_out)
    if dilation != 1 or pad is not None or mean_with is not None or leaky is not None or tanh_out:
        raise ValueError("conv3d: dilation, pad, mean_with, leaky and tanh_out belong to the kernel= form")
    B, D, H, W, Cin = _dims("conv3d", "x", x, BF16, 5)
    Cout = w.shape[0]
    taps_d = 3 if w.dim() == 5 else 1
    if tuple(w.shape[1:]) != ((3, 3, 3, Cin) if taps_d == 3 else (3, 3, Cin)):
        raise ValueError(f"conv3d: weight {tuple(w.shape)} does not match Cin={Cin}")
    oshape = (B, D, H, W, Cout)
    sc, sh = (act.get("scale"), act.get("shift")) if act is not None else (None, None)
    if (sc is None) != (sh is None):
        raise ValueError("conv3d: act['scale'] and act['shift'] must both be given or both be absent")
    _operands("conv3d", ("x", x, BF16, 5, 16), ("w", w, BF16, w.dim(), 16), ("bias", b, BF16, (Cout,), 2),
              ("resid", resid, BF16, oshape, 8), ("act['scale']", sc, BF16, (B, Cout), 8), ("act['shift']", sh, BF16, (B, Cout), 8))
    out = torch.empty(oshape, dtype=BF16, device=x.device) if (keep_out or act is None) else None
    a = Conv3dArgs()
    a.x, a.w, a.bias, a.out, a.resid = _p(x), _p(w), _p(b), _p(out), _p(resid)
    a.zero_page = _p(_scratch("zero_page", x.device))
    a.B, a.D, a.H, a.W, a.Cin, a.Cout = B, D, H, W, Cin, Cout
    a.causal, a.pad_mode, a.taps_d = int(causal), pad_mode, taps_d
    ws = _scratch("conv_splitk", x.device)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel() * 4
    act_out = None
    if act is not None:
        act_out = torch.empty(oshape, dtype=BF16, device=x.device)
        a.act_out, a.act_scale, a.act_shift = _p(act_out), _p(sc), _p(sh)
        a.act_eps, a.act_silu = float(act["eps"]), int(bool(act.get("silu", True)))
    V = B * D * H * W
    ntap = 27 if taps_d == 3 else 9
    with _timed("conv3d_k3", 2.0 * ntap * Cin * Cout * V, 2.0 * V * (Cin + Cout) + 2.0 * ntap * Cin * Cout):
        check(_lib.load().ltxk_conv3d_k3_bf16(ctypes.byref(a), _stream()), "ltxk_conv3d_k3_bf16")
    return out if act is None else (out, act_out)


@dataclass(frozen=True)
class Conv3dPlan:
    """ltxk_conv3d_plan: the launch form of one ltxk_conv3d_k3_bf16 call (include/ltxk.h, struct ltxk_conv3d_plan)."""
    kernel: int               # _lib.CONV_KERNEL_*
    tile_rows: int
    tile_cols: int
    row_tiles: int            # of the main launch
    col_tiles: int
    slices: int               # 1 unless split-K
    ksteps: int               # per slice
    tail_tile_rows: int       # the tail launch (all 0: none)
    tail_m_base: int
    tail_row_tiles: int
    fused_act: bool

    @property
    def kw(self) -> bool:
        return self.kernel == _lib.CONV_KERNEL_KW

    @property
    def split_k(self) -> bool:
        return self.slices >= 2

    @property
    def tail(self) -> bool:
        return self.tail_row_tiles > 0


def conv3d_plan(B: int, D: int, H: int, W: int, Cin: int, Cout: int, *, causal: int = 1, pad_mode: int = PAD_REFLECT,
                taps_d: int = 3, resid: bool = False, act: bool = False, keep_out: bool = True,
                workspace: Optional[Tuple[int, int]] = None, kernel: Optional[Tuple[int, int]] = None, dilation: int = 1,
                pad: Optional[Tuple[int, int, int, int]] = None) -> Conv3dPlan:
    """The form ``conv3d`` takes for this volume, decided on the host by the function the launch itself uses (no device
    needed).  The split-K scratch is offered as ``conv3d`` offers it (SPLITK_WORKSPACE_BYTES); ``workspace=(address,
    bytes)`` offers that one instead (address 0: none).  Raises LtxkError where the launch would refuse the arguments.
    ``kernel=(kh, kw)``, ``dilation=``, ``pad=``: the form of the ``kernel=`` call (ltxk_conv_taps_plan)."""
    addr = _PLAN_ADDR
    if kernel is not None:
        kh, kw, dil, (pt, pb, pl_, pr) = _taps_geometry("conv3d_plan", kernel, dilation, pad)
        t = ConvTapsArgs()
        t.struct_bytes = ctypes.sizeof(ConvTapsArgs)
        t.x = t.w = t.bias = t.zero_page = t.out = addr
        t.resid = addr if resid else None
        t.B, t.D, t.H, t.W, t.Cin, t.Cout = B, D, H, W, Cin, Cout
        t.kh, t.kw, t.dil_h = kh, kw, dil
        t.pad_top, t.pad_bottom, t.pad_left, t.pad_right = pt, pb, pl_, pr
        t.workspace, t.workspace_bytes = (addr, SPLITK_WORKSPACE_BYTES) if workspace is None else workspace
        pl = _lib.Conv3dPlan()
        check(_lib.load().ltxk_conv_taps_plan(ctypes.byref(t), ctypes.byref(pl)), "ltxk_conv_taps_plan")
        return Conv3dPlan(pl.kernel, pl.tile_rows, pl.tile_cols, pl.row_tiles, pl.col_tiles, pl.slices, pl.ksteps,
                          pl.tail_tile_rows, pl.tail_m_base, pl.tail_row_tiles, bool(pl.fused_act))
    if dilation != 1 or pad is not None:
        raise ValueError("conv3d_plan: dilation and pad belong to the kernel= form")
    a = Conv3dArgs()
    a.x = a.w = a.bias = a.zero_page = addr
    a.out = addr if (keep_out or not act) else None
    a.resid = addr if resid else None
    a.B, a.D, a.H, a.W, a.Cin, a.Cout = B, D, H, W, Cin, Cout
    a.causal, a.pad_mode, a.taps_d = int(causal), pad_mode, taps_d
    a.workspace, a.workspace_bytes = (addr, SPLITK_WORKSPACE_BYTES) if workspace is None else workspace
    if act:
        a.act_out = addr
    pl = _lib.Conv3dPlan()
    check(_lib.load().ltxk_conv3d_plan(ctypes.byref(a), ctypes.byref(pl)), "ltxk_conv3d_plan")
    return Conv3dPlan(pl.kernel, pl.tile_rows, pl.tile_cols, pl.row_tiles, pl.col_tiles, pl.slices, pl.ksteps,
                      pl.tail_tile_rows, pl.tail_m_base, pl.tail_row_tiles, bool(pl.fused_act))


def pixelnorm_act(x: torch.Tensor, eps: float, silu: bool, scale: Optional[torch.Tensor] = None,
                  shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_pixelnorm_act over the rows of x (B,...,C) [+ (1+scale)+shift per (batch, channel): scale / shift (B,C)] [+ SiLU]."""
    if (scale is None) != (shift is None):
        raise ValueError("pixelnorm_act: scale and shift must both be given or both be None")
    B = x.shape[0]
    C = x.shape[-1]
    _operands("pixelnorm_act", ("x", x, BF16, x.dim(), 16), ("scale", scale, BF16, (B, C), 16), ("shift", shift, BF16, (B, C), 16))
    V = x.numel() // C
    out = torch.empty_like(x)
    with _timed("pixelnorm_act", 0.0, 4.0 * V * C):
        check(_lib.load().ltxk_pixelnorm_act(_p(x), _p(out), V, C, eps, _p(scale), _p(shift), V // B, int(silu),
                                             _stream()), "ltxk_pixelnorm_act")
    return out


def d2s_add(conv: torch.Tensor, xin: Optional[torch.Tensor]) -> torch.Tensor:
    """ltxk_d2s_add: conv (B,D,H,W,8*Co) -> (B,2D-1,2H,2W,Co) plus the tiled residual of xin (B,D,H,W,Ci) (None: none)."""
    B, D, H, W, C8 = _dims("d2s_add", "conv", conv, BF16, 5)
    if C8 % 8:
        raise ValueError(f"d2s_add: conv must be (B,D,H,W,8*Co), got {tuple(conv.shape)}")
    Co = C8 // 8
    _operands("d2s_add", ("conv", conv, BF16, 5, 16),
              ("xin", xin, BF16, None if xin is None else (B, D, H, W) + tuple(xin.shape[-1:]), 16))
    out = torch.empty((B, 2 * D - 1, 2 * H, 2 * W, Co), dtype=BF16, device=conv.device)
    with _timed("d2s_add", 0.0, 2.0 * conv.numel() * 2 + (2.0 * xin.numel() if xin is not None else 0)):
        check(_lib.load().ltxk_d2s_add(_p(conv), _p(xin), _p(out), B, D, H, W, Co, xin.shape[-1] if xin is not None else 0,
                                       _stream()), "ltxk_d2s_add")
    return out


def groupnorm_act(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, resid=None, silu: bool = True,
                  groups: int = 32, eps: float = 1e-5) -> torch.Tensor:
    """ltxk_groupnorm_act: GroupNorm over (voxels, C/groups) of x (B,...,C) + affine [+ resid] [+ SiLU]."""
    B, C = x.shape[0], x.shape[-1]
    if C % groups:
        raise ValueError(f"groupnorm_act: x has {C} channels, no multiple of groups={groups}")
    _operands("groupnorm_act", ("x", x, BF16, x.dim(), 2), ("gamma", gamma, BF16, (C,), 2), ("beta", beta, BF16, (C,), 2),
              ("resid", resid, BF16, x.shape, 2))
    V = x.numel() // (B * C)
    out = torch.empty_like(x)
    check(_lib.load().ltxk_groupnorm_act(_p(x), _p(out), _p(gamma), _p(beta), _p(resid), B, V, C, groups, eps, int(silu),
                                         _stream()), "ltxk_groupnorm_act")
    return out


def latent_denorm_cl(latent: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, noise: Optional[torch.Tensor] = None,
                     noise_scale: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_latent_denorm_cl: latent (B,C,...) channels-first -> (B,...,C) channels-last with x*std + mean, mean / std (C);
    with ``noise`` (the latent's shape) the blend noise*noise_scale + (1-noise_scale)*x comes first."""
    if latent.dim() < 3:
        raise ValueError(f"latent_denorm_cl: latent must be (B,C,...), got {tuple(latent.shape)}")
    B, C = latent.shape[:2]
    oshape = (B,) + tuple(latent.shape[2:]) + (C,)
    _operands("latent_denorm_cl", ("latent", latent, BF16, latent.dim(), 2), ("mean", mean, BF16, (C,), 2), ("std", std, BF16, (C,), 2),
              ("noise", noise, BF16, latent.shape, 2), ("out", out, BF16, oshape, 16))
    if out is None:
        out = torch.empty(oshape, dtype=BF16, device=latent.device)
    check(_lib.load().ltxk_latent_denorm_cl(_p(latent), _p(noise), float(noise_scale) if noise is not None else 0.0, _p(mean), _p(std),
                                            _p(out), B, C, latent.numel() // (B * C), _stream()), "ltxk_latent_denorm_cl")
    return out


def latent_norm_cf(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_latent_norm_cf: x (B,...,C) channels-last rows (row stride ldx >= C) -> (B,C,...) channels-first with
    (x - mean)/std, mean / std (C)."""
    if x.dim() < 3:
        raise ValueError(f"latent_norm_cf: x must be (B,...,C), got {tuple(x.shape)}")
    B, C = x.shape[0], x.shape[-1]
    oshape = (B, C) + tuple(x.shape[1:-1])
    _operands("latent_norm_cf", ("x", x, BF16, x.dim(), 16, True), ("mean", mean, BF16, (C,), 2), ("std", std, BF16, (C,), 2),
              ("out", out, BF16, oshape, 2))
    if out is None:
        out = torch.empty(oshape, dtype=BF16, device=x.device)
    check(_lib.load().ltxk_latent_norm_cf(_p(x), x.stride(-2), _p(mean), _p(std), _p(out), B, C, x.numel() // (B * C), _stream()),
          "ltxk_latent_norm_cf")
    return out


def patchify_cl(video: torch.Tensor, P: int, Cpad: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_patchify_cl: video (B,C,D,H,W) -> (B,D,H/P,W/P,Cpad) channels-last, channel (c,p_w,p_h), channels from C*P*P up zero."""
    B, C, D, H, W = _dims("patchify_cl", "video", video, BF16, 5)
    if P < 1 or H % P or W % P or Cpad < C * P * P:
        raise ValueError(f"patchify_cl: needs H % P == 0, W % P == 0 and Cpad >= C*P*P, got {tuple(video.shape)}, P={P}, Cpad={Cpad}")
    oshape = (B, D, H // P, W // P, Cpad)
    _operands("patchify_cl", ("video", video, BF16, 5, 2), ("out", out, BF16, oshape, 2))
    if out is None:
        out = torch.empty(oshape, dtype=BF16, device=video.device)
    check(_lib.load().ltxk_patchify_cl(_p(video), _p(out), B, C, D, H, W, P, Cpad, _stream()), "ltxk_patchify_cl")
    return out


def unpatchify_cf(x: torch.Tensor, C: int, P: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_unpatchify_cf: x (B,D,H,W,C*P*P) channels-last -> video (B,C,D,H*P,W*P) channels-first (8-byte aligned at P = 4)."""
    B, D, H, W, CPP = _dims("unpatchify_cf", "x", x, BF16, 5)
    if C < 1 or P < 1 or CPP != C * P * P:
        raise ValueError(f"unpatchify_cf: x must be (B,D,H,W,C*P*P = {C * P * P}), got {tuple(x.shape)}")
    oshape = (B, C, D, H * P, W * P)
    _operands("unpatchify_cf", ("x", x, BF16, 5, 2), ("out", out, BF16, oshape, 8 if P == 4 else 2))
    if out is None:
        out = torch.empty(oshape, dtype=BF16, device=x.device)
    check(_lib.load().ltxk_unpatchify_cf(_p(x), _p(out), B, D, H, W, C, P, _stream()), "ltxk_unpatchify_cf")
    return out


def s2d_skip(conv: torch.Tensor, xpad: torch.Tensor, stride: Tuple[int, int, int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_s2d_skip: conv (B,Dp,Hp,Wp,Cc) and the input xpad (B,Dp,Hp,Wp,Cx) it was computed on ->
    (B,Dp/st,Hp/sh,Wp/sw,Cc*st*sh*sw) = s2d(conv) + the mean over groups of Cx/Cc channels of s2d(xpad)."""
    st, sh, sw = stride
    B, Dp, Hp, Wp, Cc = _dims("s2d_skip", "conv", conv, BF16, 5)
    if st < 1 or sh < 1 or sw < 1 or Dp % st or Hp % sh or Wp % sw:
        raise ValueError(f"s2d_skip: volume {Dp}x{Hp}x{Wp} not divisible by stride {tuple(stride)}")
    Cx = xpad.shape[-1] if xpad.dim() else 0
    if Cx % Cc:
        raise ValueError(f"s2d_skip: xpad's {Cx} channels are no multiple of conv's {Cc}")
    oshape = (B, Dp // st, Hp // sh, Wp // sw, Cc * st * sh * sw)
    _operands("s2d_skip", ("conv", conv, BF16, 5, 2), ("xpad", xpad, BF16, (B, Dp, Hp, Wp, Cx), 2), ("out", out, BF16, oshape, 2))
    if out is None:
        out = torch.empty(oshape, dtype=BF16, device=conv.device)
    check(_lib.load().ltxk_s2d_skip(_p(conv), _p(xpad), _p(out), B, Dp, Hp, Wp, Cc, Cx, st, sh, sw, Cx // Cc, _stream()),
          "ltxk_s2d_skip")
    return out


def to_uint8(video: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_to_uint8: video (B,C,F,H,W) bf16 in [-1,1] -> frames (B,F,H,W,C) uint8."""
    B, C, F, H, W = _dims("to_uint8", "video", video, BF16, 5)
    oshape = (B, F, H, W, C)
    _operands("to_uint8", ("video", video, BF16, 5, 2), ("out", out, torch.uint8, oshape, 1))
    if out is None:
        out = torch.empty(oshape, dtype=torch.uint8, device=video.device)
    check(_lib.load().ltxk_to_uint8(_p(video), _p(out), B, C, F, H, W, _stream()), "ltxk_to_uint8")
    return out


def tile_blend_accum(tile: torch.Tensor, mt: torch.Tensor, mh: torch.Tensor, mw: torch.Tensor, acc: torch.Tensor,
                     wsum: torch.Tensor, t0: int, h0: int, w0: int) -> torch.Tensor:
    """ltxk_tile_blend_accum: acc[b,c,t0+t,h0+y,w0+x] += tile[b,c,t,y,x] * m and wsum[b,0,t0+t,h0+y,w0+x] += m with
    m = mt[t]*mh[y]*mw[x], over the leading (len(mt), len(mh), len(mw)) box of tile (B,C,Tt,Th,Tw) bf16; the masks and
    acc (B,C,F,H,W) / wsum (B,1,F,H,W) are float32.  The box must lie inside both volumes (the library refuses it otherwise)."""
    F32 = torch.float32
    B, C, F, H, W = _dims("tile_blend_accum", "acc", acc, F32, 5)
    _operands("tile_blend_accum", ("tile", tile, BF16, (B, C) + tuple(tile.shape[2:]) if tile.dim() == 5 else 5, 2), ("mt", mt, F32, 1, 4), ("mh", mh, F32, 1, 4),
              ("mw", mw, F32, 1, 4), ("acc", acc, F32, 5, 4), ("wsum", wsum, F32, (B, 1, F, H, W), 4))
    Tt, Th, Tw = tile.shape[2:]
    check(_lib.load().ltxk_tile_blend_accum(_p(tile), Tt, Th, Tw, mt.numel(), mh.numel(), mw.numel(), _p(mt), _p(mh), _p(mw),
                                            _p(acc), _p(wsum), B, C, F, H, W, t0, h0, w0, _stream()), "ltxk_tile_blend_accum")
    return acc


def tile_blend_finalize(acc: torch.Tensor, wsum: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ltxk_tile_blend_finalize: bf16(acc / max(wsum, 1e-8)), acc (B,C,...) and wsum (B,1,...) float32 -> acc's shape."""
    if acc.dim() < 3:
        raise ValueError(f"tile_blend_finalize: acc must be (B,C,...), got {tuple(acc.shape)}")
    B, C = acc.shape[:2]
    _operands("tile_blend_finalize", ("acc", acc, torch.float32, acc.dim(), 4),
              ("wsum", wsum, torch.float32, (B, 1) + tuple(acc.shape[2:]), 4), ("out", out, BF16, acc.shape, 2))
    if out is None:
        out = torch.empty(acc.shape, dtype=BF16, device=acc.device)
    check(_lib.load().ltxk_tile_blend_finalize(_p(acc), _p(wsum), _p(out), B, C, acc.numel() // (B * C), _stream()),
          "ltxk_tile_blend_finalize")
    return out
