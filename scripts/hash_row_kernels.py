"""SHA-256 of what the norm + RoPE entry points write, on seeded inputs: the row kernels that call csrc/rows.h
(qknorm_rope with and without carried statistics and tables, qknorm_grouped, qknorm_rope_1d, headnorm_rope), the two
RMSNorm entry points of csrc/text_ops.hip, and flash_attn with the fused query preparation in each launch form.  Inputs
are drawn on the host, so two builds of the library fed to this script (LTXK_LIB=/path/to/libltxk.so; the -DLTXK_AB build
is taken from the same directory for the 32x32x16 attention form) must print identical lines: profiles/rows_refactor_bits.txt.
usage: [LTXK_LIB=...] python scripts/hash_row_kernels.py   -> one `name shape sha256` line per case"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlx_video_amd import _lib, ops                                                        # noqa: E402
from mlx_video_amd.text_connector import rope_table_1d                                     # noqa: E402

BF = torch.bfloat16
dev = torch.device("cuda:0")


def emit(name, shape, t):
    torch.cuda.synchronize()
    h = hashlib.sha256(t.contiguous().cpu().view(torch.int16).numpy().tobytes()).hexdigest()
    print(f"{name} {shape} {h}", flush=True)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rows(M, D, g, spread=True):
    x = torch.randn(M, D, generator=g)
    return ((x * torch.logspace(-2, 2, M).reshape(M, 1)) if spread else x).to(BF).to(dev)


def sumsq(x, segs):
    """(M, segs * D/64) fp32 partial sums of squares, the layout gemm(..., sumsq=) writes."""
    return (x.float() ** 2).reshape(x.shape[0], -1, 64).sum(-1).contiguous()


def rmsnorm_cases():
    for M, D in ((5, 8), (5, 264), (3, 3840), (2, 8192), (2048, 3840)):
        g = gen(M + D)
        x = rows(M, D, g)
        w = (torch.randn(D, generator=g) * 0.3).to(BF).to(dev)
        r = torch.randn(M, D, generator=g).to(BF).to(dev)
        emit("rmsnorm_rows", f"M={M},D={D}", ops.rmsnorm_rows(x, 1e-6))
        emit("rmsnorm_weight_rows.plain", f"M={M},D={D}", ops.rmsnorm_weight_rows(x, w, 1e-6))
        emit("rmsnorm_weight_rows.resid", f"M={M},D={D}", ops.rmsnorm_weight_rows(x, w, 1e-6, resid=r))
        ra = r.clone()
        emit("rmsnorm_weight_rows.resid_aliased", f"M={M},D={D}", ops.rmsnorm_weight_rows(x, w, 1e-6, resid=ra, out=ra))


def qknorm_1d_cases():
    for D, H, M, T in ((3840, 30, 70, 32), (384, 3, 37, 32), (4224, 33, 5, 32), (8192, 64, 3, 32), (512, 4, 5, 3), (1536, 12, 5, 3),
                       (4096, 32, 5, 3), (3840, 30, 2048, 1024)):
        g = gen(D + M)
        buf = rows(M, 2 * D, g)
        w = (1.0 + 0.2 * torch.randn(2, D, generator=g)).to(BF).to(dev)
        cos, sin = (t.to(dev) for t in rope_table_1d(T, H))
        emit("qknorm_rope_1d", f"M={M},D={D},H={H},T={T}", ops.qknorm_rope_1d(buf, D, w, cos, sin, T, H, 1e-6))


def qknorm_cases():
    for M, D, H, T in ((5, 512, 4, 3), (5, 4096, 32, 3), (2560, 4096, 32, 1280)):
        g = gen(M + D + H)
        x = rows(M, 2 * D, g)
        w = (1.0 + 0.2 * torch.randn(2, D, generator=g)).to(BF).to(dev)
        cos = torch.randn(H, T, 64, generator=g).to(dev)
        sin = torch.randn(H, T, 64, generator=g).to(dev)
        ss = sumsq(x, 2)
        shape = f"M={M},D={D},H={H},T={T}"
        for tables in (True, False):
            c, s = (cos, sin) if tables else (None, None)
            tag = "rope" if tables else "norm_only"
            emit(f"qknorm_rope.{tag}", shape, ops.qknorm_rope(x.clone(), 2, D, w, c, s, T, H, 1e-6))
            emit(f"qknorm_rope.sumsq.{tag}", shape, ops.qknorm_rope(x.clone(), 2, D, w, c, s, T, H, 1e-6, sumsq=ss))
        G = 2
        gb = x.reshape(M, G, D).permute(1, 0, 2).contiguous()
        gs = ss.reshape(M, G, D // 64).permute(1, 0, 2).contiguous()
        emit("qknorm_grouped", f"G={G}," + shape, ops.qknorm_grouped(gb, w, H, 1e-6, gs))


def headnorm_cases():
    for M, Hq, Hkv, T in ((5, 4, 2, 3), (2048, 16, 8, 1024)):
        g = gen(M + Hq)
        buf = rows(M, (Hq + 2 * Hkv) * 256, g, spread=False)
        qw = (torch.randn(256, generator=g) * 0.3).to(BF).to(dev)
        kw = (torch.randn(256, generator=g) * 0.3).to(BF).to(dev)
        cos = torch.randn(T, 128, generator=g).to(BF).float().to(dev)
        sin = torch.randn(T, 128, generator=g).to(BF).float().to(dev)
        emit("headnorm_rope", f"M={M},Hq={Hq},Hkv={Hkv},T={T}", ops.headnorm_rope(buf, Hq, Hkv, qw, kw, cos, sin, T, 1e-6))


def attn_case(B, H, Tq, Tk, rope, tag=""):
    D = H * 128
    g = gen(B + H + Tq + Tk)
    q = torch.randn(B * Tq, D, generator=g).to(BF).to(dev)
    k = torch.randn(B * Tk, D, generator=g).to(BF).to(dev)
    ldvt = (Tk + 63) // 64 * 64
    vt = torch.zeros(B, D, ldvt, dtype=BF)
    vt[:, :, :Tk] = torch.randn(B, D, Tk, generator=g).to(BF)
    vt = vt.to(dev)
    w = (1.0 + 0.2 * torch.randn(D, generator=g)).to(BF).to(dev)
    cos = torch.randn(H, Tq, 64, generator=g).to(dev) if rope else None
    sin = torch.randn(H, Tq, 64, generator=g).to(dev) if rope else None
    out = torch.empty(B * Tq, D, dtype=BF, device=dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    pl = ops.flash_attn_plan(B, H, Tq, Tk, cus=cus, fused_q=True)
    form = f"kernel={pl.kernel},mfma_k={pl.mfma_k},t192={pl.tiles_192},t128={pl.tiles_128},split={pl.split_tiles}"
    ops.flash_attn(q, k, vt, out, B, H, Tq, Tk, 128 ** -0.5, q_sumsq=sumsq(q, 1), q_norm_weight=w, cos=cos, sin=sin, eps=1e-6)
    emit(f"flash_attn.fused_q{tag}.{'rope' if rope else 'norm_only'}", f"B={B},H={H},Tq={Tq},Tk={Tk},{form}", out)


def attn_cases():
    shapes = ((1, 4, 200, 333), (1, 32, 1280, 1280), (2, 32, 1280, 1280))      # key-split 128-row tiles; the same, whole rounds; mixed grid
    for B, H, Tq, Tk in shapes:
        for rope in (True, False):
            attn_case(B, H, Tq, Tk, rope)
    ab = os.path.join(os.path.dirname(_lib.LIB_PATH), "libltxk_ab.so")
    os.environ["LTXK_FA_MFMA"] = "32"
    with _lib.use_library(ab):
        for B, H, Tq, Tk in shapes[:2]:
            for rope in (True, False):
                attn_case(B, H, Tq, Tk, rope, tag=".ab_mfma32")
    del os.environ["LTXK_FA_MFMA"]


if __name__ == "__main__":
    rmsnorm_cases()
    qknorm_1d_cases()
    qknorm_cases()
    headnorm_cases()
    attn_cases()
