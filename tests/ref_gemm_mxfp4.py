"""Float64 emulation of the MXFP4 x MXFP4 GEMM (ltxk_gemm_mxfp4), next to tests/ref_gemm.py whose bound it feeds.

An operand is a pair (codes (R, K/2) uint8, block_scales (R, K/32) uint8): OCP MXFP4, element 2i in the low nibble of byte i,
value = e2m1(code) * 2^(E - 127) with one E per 32 consecutive k.  ``dequant`` restates that without the product's own
``weights.dequantize_mxfp4``; every value is exact in float64 (and, for bytes 1..254, in fp32).  ``product`` gives
s = deq(a) @ deq(w)^T and mag = |deq(a)| @ |deq(w)|^T on the operands' device: what ``ref_gemm.bound`` takes.
tests/test_mxfp4_dit_cpu.py checks it against a 2 x 2 x 32 case computed by hand."""
import torch

F64 = torch.float64
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # magnitude by 3-bit index; bit 3 is the sign
BLOCK = 32


def dequant(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and codes.dim() == 2
    R, K = codes.shape[0], codes.shape[1] * 2
    assert tuple(scales.shape) == (R, K // BLOCK) and K % BLOCK == 0
    c = codes.to(torch.int64)
    nib = torch.stack([c & 15, c >> 4], dim=2).reshape(R, K)
    mag = torch.tensor(E2M1, dtype=F64, device=codes.device)[nib & 7]
    val = torch.where((nib & 8) != 0, -mag, mag)
    sc = torch.exp2(scales.to(F64) - 127.0)
    return (val.reshape(R, K // BLOCK, BLOCK) * sc[..., None]).reshape(R, K)


def product(a_codes, a_scales, w_codes, w_scales):
    a, w = dequant(a_codes, a_scales), dequant(w_codes, w_scales)
    return a @ w.t(), a.abs() @ w.abs().t()


def random_pair(R: int, K: int, g: torch.Generator, scale_bytes):
    """Codes uniform over all 256 byte values (so all 16 nibbles, -0 included) and scale bytes drawn independently per
    (row, block) from ``scale_bytes`` (a sequence of byte values).  CPU tensors, from the CPU generator ``g``."""
    codes = torch.randint(0, 256, (R, K // 2), generator=g, dtype=torch.int64).to(torch.uint8)
    pool = torch.tensor(list(scale_bytes), dtype=torch.int64)
    scales = pool[torch.randint(0, len(pool), (R, K // BLOCK), generator=g)].to(torch.uint8)
    return codes, scales
