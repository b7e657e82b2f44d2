"""The grouped GEMM on the host (no GPU): the binding's struct layout against the library's, and the tile
ltxk_gemm_bf16_grouped takes (ltxk_gemm_grouped_plan - the host function the launch itself uses) at the text k|v shapes."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    from mlx_video_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    from mlx_video_amd import ops
    return ops


def test_grouped_args_layout_matches_the_library(ops):
    from mlx_video_amd import _lib
    lib = _lib.load()
    assert lib.ltxk_gemm_grouped_args_sizeof() == ctypes.sizeof(_lib.GemmGroupedArgs) == 112
    assert _lib.GemmGroupedArgs.out_gstride.offset == 48 and _lib.GemmGroupedArgs.G.offset == 72
    assert lib.ltxk_abi_sizeof(5) == -1          # the index list stays closed: the new struct reports through its own entry
    for name in ("ltxk_gemm_bf16_grouped", "ltxk_gemm_grouped_plan", "ltxk_qknorm_grouped_ss"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_grouped_tile_choice(ops):
    D = 4096
    # M=2048 (B=2, S=1024): six whole 320-row tiles and the 128 rows left on a 128-row body; 48 x 7 x 32 tiles = 42 rounds of 256
    p = ops.gemm_grouped_plan(48, 2048, 2 * D, D, n_split=D, out_tokens_per_batch=1024)
    assert (p.tile_rows, p.rem_rows, p.row_tiles, p.col_tiles, p.tiles) == (320, 128, 7, 32, 48 * 224)
    # M=1024 (B=1): whole 256-row tiles beat 3 x 320 + a 128-row body for 64 rows
    p = ops.gemm_grouped_plan(48, 1024, 2 * D, D, n_split=D, out_tokens_per_batch=1024)
    assert (p.tile_rows, p.rem_rows, p.row_tiles) == (256, 0, 4)
    # ragged M: 3 x 320 + 40 rows; a short context: one 256-row body for 154 rows
    p = ops.gemm_grouped_plan(3, 1000, 2 * D, D, n_split=D, out_tokens_per_batch=500)
    assert (p.tile_rows, p.rem_rows, p.row_tiles) == (320, 128, 4)
    p = ops.gemm_grouped_plan(3, 154, 2 * D, D, n_split=D, out_tokens_per_batch=77)
    assert (p.tile_rows, p.rem_rows, p.row_tiles) == (320, 256, 1)
    p = ops.gemm_grouped_plan(1, 640, 1024, 512, n_split=512, out_tokens_per_batch=320)
    assert (p.tile_rows, p.rem_rows, p.row_tiles, p.col_tiles, p.tiles) == (320, 0, 2, 4, 8)


def test_grouped_refuses_bad_arguments(ops):
    from mlx_video_amd._lib import LtxkError
    with pytest.raises(LtxkError, match="n_split"):
        ops.gemm_grouped_plan(2, 256, 1024, 512, n_split=0, out_tokens_per_batch=128)
    with pytest.raises(LtxkError, match="multiple of 256"):
        ops.gemm_grouped_plan(2, 256, 1024 + 64, 512, n_split=512, out_tokens_per_batch=128)
    with pytest.raises(LtxkError, match="out_tokens_per_batch"):
        ops.gemm_grouped_plan(2, 250, 1024, 512, n_split=512, out_tokens_per_batch=128)
