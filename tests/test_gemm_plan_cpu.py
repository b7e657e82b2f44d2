"""The GEMM launch plan on the host (ltxk_gemm_plan through ops.gemm_plan; no GPU): the split-K form's invariants over small
M, where the workspace decides it, and which launches of a DiT forward take it.  ltxk_gemm_bf16 decides its form by the same
host function, so these plans are the launches' forms.  The GPU tests test_gemm_splitk_gpu.py and
test_batch_invariance_gpu.py check their plans before they rely on them; when this heuristic moves, re-aim them."""
import os

import pytest

from dit_launches import dit_launches

D = 4096
MODEL_NK = [(3 * D, D), (2 * D, D), (D, D), (4 * D, D), (D, 4 * D), (6 * D, D), (D, 3840), (D, 256), (D, 128), (128, D)]
AWKWARD_NK = [(1000, 64 * 67), (4104, 64 * 67), (2056, 64 * 40), (8, 64 * 512), (520, 64 * 97), (12288, 64 * 9)]
SWEEP_M = sorted(set(range(1, 41)) | {47, 63, 64, 65, 96, 127, 128, 129, 159, 160, 161, 191, 192, 255, 256, 257, 319, 320, 321,
                                      383, 447, 448, 511, 512, 513, 575, 639, 640, 641})


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    from mlx_video_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    from mlx_video_amd import ops
    return ops


def _check_split_plan(ops, pl, M, N, K, ws_bytes):
    nk = K // 64
    where = f"M={M} N={N} K={K}: {pl}"
    assert pl.slices >= 2 and pl.ksteps >= 8, where                             # at least 8 K-steps per slice
    assert (pl.slices - 1) * pl.ksteps < nk <= pl.slices * pl.ksteps, where      # every K-step in a slice, no empty slice
    assert pl.slices * M * N * 4 <= ws_bytes, where                              # the slice tiles fit the scratch
    assert pl.tile_cols == 128 and pl.col_tiles * 128 >= N > (pl.col_tiles - 1) * 128, where
    assert pl.row_tiles * pl.tile_rows >= M > (pl.row_tiles - 1) * pl.tile_rows, where


def test_split_k_plan_invariants(ops):
    """Over M <= 641 x the model's (N, K) and awkward ones: a split-K plan never leaves a slice empty, fits its slices into
    the scratch ops.gemm offers and gives each at least 8 K-steps; the tiles cover the output exactly."""
    splits = 0
    for N, K in MODEL_NK + AWKWARD_NK:
        for M in SWEEP_M:
            for kw in ({}, dict(epilogue=ops.EPI_BIAS_GATE_RES, sumsq=N % 64 == 0)):
                pl = ops.gemm_plan(M, N, K, **kw)
                if pl.split_k:
                    splits += 1
                    _check_split_plan(ops, pl, M, N, K, ops.GEMM_WORKSPACE_BYTES)
                else:
                    assert pl.slices == 1 and pl.ksteps == K // 64, pl
                if M > ops.SPLITK_MAX_M:
                    assert not pl.split_k, (M, N, K, pl)             # ops.gemm offers no scratch above SPLITK_MAX_M
    assert splits > 400, f"only {splits} split-K plans in the sweep: the sweep no longer reaches the form"


@pytest.mark.parametrize("M,N,K", [(1, 4096, 4096), (33, 1000, 64 * 67), (160, 4096, 4096), (320, 4104, 64 * 67),
                                   (640, 4096, 16384)])
def test_split_k_needs_a_usable_workspace(ops, M, N, K):
    """No scratch, one too small for two slices, or a misaligned one: single-pass.  A smaller scratch caps the slices.
    M = 641 is single-pass even with a scratch."""
    A = 1 << 16
    full = ops.gemm_plan(M, N, K, workspace=(A, 1 << 30))
    assert full.split_k, full
    _check_split_plan(ops, full, M, N, K, 1 << 30)
    assert ops.gemm_plan(M, N, K) == full                                    # ops.gemm's 64 MB suffice here
    assert not ops.gemm_plan(M, N, K, workspace=(0, 1 << 30)).split_k
    assert not ops.gemm_plan(M, N, K, workspace=(A, 2 * M * N * 4 - 1)).split_k
    assert not ops.gemm_plan(M, N, K, workspace=(A + 8, 1 << 30)).split_k
    assert not ops.gemm_plan(M, N, K, split_k=False).split_k
    if full.slices > 2:
        small = ops.gemm_plan(M, N, K, workspace=(A, (full.slices - 1) * M * N * 4))
        assert small.split_k and small.slices < full.slices, small
        _check_split_plan(ops, small, M, N, K, (full.slices - 1) * M * N * 4)
    assert not ops.gemm_plan(641, N, K, workspace=(A, 1 << 30)).split_k


def test_plan_refuses_what_the_launch_refuses(ops):
    from mlx_video_amd._lib import LtxkError
    with pytest.raises(LtxkError, match="multiple of 64"):
        ops.gemm_plan(64, 4096, 100)
    with pytest.raises(LtxkError, match="multiple of 8"):
        ops.gemm_plan(64, 4100, 4096)
    with pytest.raises(LtxkError, match="unknown epilogue"):
        ops.gemm_plan(64, 4096, 4096, epilogue=9)
    with pytest.raises(LtxkError, match="n_split"):
        ops.gemm_plan(64, 4096, 4096, n_split=300, out_tokens_per_batch=32)


@pytest.mark.parametrize("T", [32, 128, 160, 320, 640, 1280])
@pytest.mark.parametrize("B", [1, 2])
def test_split_k_false_never_splits(ops, B, T):
    """ops.gemm(split_k=False), as LTXModel.batch_invariant runs every GEMM of a forward: never the split-K form."""
    for name, M, N, K, kw in dit_launches(ops, B, T):
        pl = ops.gemm_plan(M, N, K, split_k=False, **kw)
        assert not pl.split_k, (name, B, T, pl)


def test_default_plan_known_answer(ops):
    """The row the batch-invariance test relies on: at T=128 the out-projection is split-K for B=1 and single-pass for
    B=2.  If the heuristic stops splitting here, re-aim test_batch_invariance_gpu.py / test_gemm_splitk_gpu.py."""
    one = {n: ops.gemm_plan(M, N, K, **kw) for n, M, N, K, kw in dit_launches(ops, 1, 128)}
    two = {n: ops.gemm_plan(M, N, K, **kw) for n, M, N, K, kw in dit_launches(ops, 2, 128)}
    assert one["out"].split_k and one["out"].slices == 8, one["out"]
    assert not two["out"].split_k, two["out"]
    # the same for FF2 at T=320: four slices for B=1, two for B=2
    one = {n: ops.gemm_plan(M, N, K, **kw) for n, M, N, K, kw in dit_launches(ops, 1, 320)}
    two = {n: ops.gemm_plan(M, N, K, **kw) for n, M, N, K, kw in dit_launches(ops, 2, 320)}
    assert (one["ff2"].slices, two["ff2"].slices) == (4, 2), (one["ff2"], two["ff2"])
