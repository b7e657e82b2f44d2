"""ltxk_gemm_bf16_grouped and ltxk_qknorm_grouped_ss against the per-group calls they stand for, BIT FOR BIT: k row-major,
V^T (with its zero-padded columns where S is not a multiple of 64) and the 64-column sums of squares of the GEMM; the
normalised k of the norm.  G in {1, 3, 48}; M in {2048, 1024, 1000, 154}: a 128-row remainder body, whole 256-row tiles, a
ragged remainder, and one short body with S = 77; at the model's full width (N=8192, K=4096) and at a reduced one."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = {2048: (2, 1024), 1024: (1, 1024), 1000: (2, 500), 154: (2, 77)}        # M -> (batches, tokens per batch)
WIDTHS = {"full": (8192, 4096), "reduced": (1024, 512)}                            # N (k | v packed), K


@pytest.fixture(scope="module")
def bank(dev):
    """48 weight panels / bias rows per width (3.2 GB at full width), generated once."""
    g = torch.Generator(device=dev).manual_seed(5)
    out = {}
    for name, (N, K) in WIDTHS.items():
        w = [(torch.randn((N, K), generator=g, device=dev) * 0.02).to(BF) for _ in range(48)]
        b = [(torch.randn((N,), generator=g, device=dev) * 0.01).to(BF) for _ in range(48)]
        out[name] = (w, b)
    return out


def _buffers(G, B, S, n_split, dev, fill):
    sp = (S + 63) // 64 * 64
    k = torch.full((G, B * S, n_split), fill, dtype=BF, device=dev)
    vt = torch.zeros((G, B, n_split, sp), dtype=BF, device=dev)
    ss = torch.full((G, B * S, n_split // 64), fill, dtype=torch.float32, device=dev)
    return k, vt, ss


@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("M", sorted(SHAPES))
@pytest.mark.parametrize("G", [1, 3, 48])
def test_grouped_gemm_equals_separate_calls(dev, bank, G, M, width):
    from mlx_video_amd import ops
    N, K = WIDTHS[width]
    B, S = SHAPES[M]
    D = N // 2
    w, b = bank[width]
    # (not the first G panels every time: a table that is not a prefix of the bank)
    pick = [(7 * i + G) % 48 for i in range(G)]
    g = torch.Generator(device=dev).manual_seed(1000 + M + G)
    a = torch.randn((M, K), generator=g, device=dev).to(BF)
    k, vt, ss = _buffers(G, B, S, D, dev, 7.0)
    ops.gemm_grouped(a, ops.pointer_table([w[i] for i in pick]), ops.pointer_table([b[i] for i in pick]), N,
                     out=k, out2=vt, n_split=D, out_tokens_per_batch=S, sumsq=ss)
    rk, rvt, rss = _buffers(1, B, S, D, dev, -3.0)
    for j, i in enumerate(pick):
        rvt.zero_()
        ops.gemm(a, w[i], b[i], out=rk[0], out2=rvt[0], n_split=D, out_tokens_per_batch=S, sumsq=rss[0], split_k=False)
        assert torch.equal(k[j], rk[0]), f"group {j}: k differs"
        assert torch.equal(vt[j], rvt[0]), f"group {j}: V^T differs"
        assert torch.equal(ss[j], rss[0]), f"group {j}: sumsq differs"
    if S % 64:
        assert float(vt[..., S:].abs().max()) == 0.0          # the pad columns stay zero
    assert bool(torch.isfinite(k.float()).all()) and float(k.float().abs().max()) > 0.0


def test_grouped_gemm_without_bias_and_statistics(dev, bank):
    from mlx_video_amd import ops
    N, K = WIDTHS["reduced"]
    D = N // 2
    w, _ = bank["reduced"]
    a = torch.randn((640, K), generator=torch.Generator(device=dev).manual_seed(3), device=dev).to(BF)
    k, vt, _ = _buffers(5, 2, 320, D, dev, 1.0)
    ops.gemm_grouped(a, ops.pointer_table(w[:5]), None, N, out=k, out2=vt, n_split=D, out_tokens_per_batch=320)
    for j in range(5):
        rk, rvt, _ = _buffers(1, 2, 320, D, dev, 2.0)
        ops.gemm(a, w[j], None, out=rk[0], out2=rvt[0], n_split=D, out_tokens_per_batch=320, split_k=False)
        assert torch.equal(k[j], rk[0]) and torch.equal(vt[j], rvt[0])


@pytest.mark.parametrize("G,M,H", [(48, 2048, 32), (3, 154, 32), (1, 1000, 4), (5, 64, 12)])
def test_grouped_knorm_equals_separate_calls(dev, G, M, H):
    from mlx_video_amd import ops
    D = H * 128
    g = torch.Generator(device=dev).manual_seed(G * 31 + M)
    x = torch.randn((G, M, D), generator=g, device=dev).to(BF)
    wn = (1.0 + 0.1 * torch.randn((G, D), generator=g, device=dev)).to(BF)
    ss = (x.float() ** 2).reshape(G, M, D // 64, 64).sum(-1)
    ref = x.clone()
    for j in range(G):
        ops.qknorm_rope(ref[j], 1, D, wn[j], None, None, M, H, 1e-6, sumsq=ss[j])
    got = x.clone()
    ops.qknorm_grouped(got, wn, H, 1e-6, ss)
    assert torch.equal(got, ref)
    assert not torch.equal(got, x)
