"""The convolution launch plan on the host (ltxk_conv3d_plan through ops.conv3d_plan; no GPU): which kernel, which
tile, the split-K slices and the tail launch.  ltxk_conv3d_k3_bf16 decides its form by the same host function, so these
plans are the launches' forms.  tests/test_conv3d_bound_gpu.py asserts the plan of every case before it relies on it; when
a rule here moves, re-aim those cases."""
import ctypes
import os

import pytest

A = 1 << 16                     # a 16-byte aligned stand-in address
NO_WS = (0, 0)
BIG = (A, 1 << 30)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    from mlx_video_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    from mlx_video_amd import ops
    return ops


def test_conv3d_plan_abi(ops):
    from mlx_video_amd import _lib
    lib = _lib.load()
    assert lib.ltxk_conv3d_plan_sizeof() == ctypes.sizeof(_lib.Conv3dPlan) == 44
    assert lib.ltxk_version() >= 406
    assert lib.ltxk_abi_sizeof(1) == ctypes.sizeof(_lib.Conv3dArgs)           # ltxk_conv3d_args is unchanged


def _covers(pl, M, Cout):
    """The main launch plus the tail launch cover every row exactly once and every column."""
    assert (pl.col_tiles - 1) * pl.tile_cols < Cout <= pl.col_tiles * pl.tile_cols, pl
    if pl.tail:
        assert pl.tail_m_base == pl.row_tiles * pl.tile_rows < M, pl
        assert (pl.tail_row_tiles - 1) * pl.tail_tile_rows < M - pl.tail_m_base <= pl.tail_row_tiles * pl.tail_tile_rows, pl
    else:
        assert (pl.tail_tile_rows, pl.tail_m_base, pl.tail_row_tiles) == (0, 0, 0), pl
        assert (pl.row_tiles - 1) * pl.tile_rows < M <= pl.row_tiles * pl.tile_rows, pl


def test_tile_by_cout_and_ksteps(ops):
    for Cout, tile in [(8, (256, 128)), (128, (256, 128)), (136, (160, 256)), (256, (160, 256)), (264, (160, 256))]:
        for taps_d, Cin in [(3, 64), (1, 64), (3, 192)]:
            pl = ops.conv3d_plan(2, 3, 7, 9, Cin, Cout, taps_d=taps_d, workspace=NO_WS)
            assert not pl.kw and not pl.split_k and not pl.tail and not pl.fused_act, pl
            assert (pl.tile_rows, pl.tile_cols) == tile, pl
            assert pl.slices == 1 and pl.ksteps == (27 if taps_d == 3 else 9) * Cin // 64, pl
            _covers(pl, 378, Cout)


def test_split_k_slice_count(ops):
    """S = min(256 / tiles, nk / 16, what the workspace holds, 16) slices of ceil(nk / S) K-steps, empty trailing slices
    dropped; needs tiles <= 128 and at least two slices."""
    # (volume, Cin, Cout, taps_d) -> (slices, ksteps)
    for vol, Cin, Cout, taps_d, want in [((1, 2, 4, 4), 128, 128, 3, (3, 18)), ((2, 3, 7, 9), 128, 264, 3, (3, 18)),
                                         ((1, 2, 4, 4), 192, 128, 3, (5, 17)),      # 81 K-steps: the last slice has 13
                                         ((2, 3, 7, 9), 256, 128, 1, (2, 18)),
                                         ((1, 2, 4, 4), 1024, 1024, 3, (16, 27)),   # capped at 16 slices
                                         ((1, 5, 16, 16), 512, 512, 3, (13, 17))]:  # 216 K-steps / 16 = 13 slices
        M = vol[0] * vol[1] * vol[2] * vol[3]
        pl = ops.conv3d_plan(*vol, Cin, Cout, taps_d=taps_d, workspace=BIG)
        nk = (27 if taps_d == 3 else 9) * Cin // 64
        assert pl.split_k and not pl.kw and not pl.tail, pl
        assert (pl.slices - 1) * pl.ksteps < nk <= pl.slices * pl.ksteps, pl          # no empty slice
        assert pl.ksteps >= 16 and pl.slices <= 16, pl
        assert (pl.slices, pl.ksteps) == want, pl
        _covers(pl, M, Cout)
        assert ops.conv3d_plan(*vol, Cin, Cout, taps_d=taps_d) == pl                   # conv3d's own scratch suffices here
        # no workspace, a misaligned one is refused, one too small for two slabs: single pass
        assert not ops.conv3d_plan(*vol, Cin, Cout, taps_d=taps_d, workspace=NO_WS).split_k
        per = M * Cout * 4
        one = ops.conv3d_plan(*vol, Cin, Cout, taps_d=taps_d, workspace=(A, 2 * per - 1))
        assert not one.split_k and one.slices == 1 and one.ksteps == nk, one
        assert not ops.conv3d_plan(*vol, Cin, Cout, taps_d=taps_d, workspace=(A, per)).split_k
        two = ops.conv3d_plan(*vol, Cin, Cout, taps_d=taps_d, workspace=(A, 2 * per))
        assert two.split_k and two.slices == 2, two
    # nk < 32: never two slices of 16 K-steps
    for Cin, taps_d in [(64, 3), (192, 1)]:
        pl = ops.conv3d_plan(2, 3, 7, 9, Cin, 128, taps_d=taps_d, workspace=BIG)
        assert pl.ksteps < 32 and not pl.split_k, pl
    assert ops.conv3d_plan(2, 3, 7, 9, 256, 128, taps_d=1, workspace=BIG).ksteps == 18      # 36 K-steps: two slices
    # more than 128 tiles: the grid fills the chip on its own
    assert ops.conv3d_plan(1, 8, 64, 60, 128, 128, workspace=BIG).split_k                   # 120 tiles
    assert not ops.conv3d_plan(1, 9, 64, 60, 128, 128, workspace=BIG).split_k               # 135 tiles


def test_act_out_drops_split_k(ops):
    for Cout in (128, 256):
        base = ops.conv3d_plan(2, 3, 7, 9, 128, Cout, workspace=BIG)
        assert base.split_k and not base.fused_act, base
        for keep in (True, False):
            pl = ops.conv3d_plan(2, 3, 7, 9, 128, Cout, workspace=BIG, act=True, keep_out=keep)
            assert pl.fused_act and not pl.split_k and not pl.kw, pl
            assert (pl.tile_cols, pl.col_tiles) == (Cout, 1), pl                          # the tile holds whole rows
    # and the kw kernel has no fused epilogue
    assert ops.conv3d_plan(1, 3, 128, 128, 64, 128).kw
    assert not ops.conv3d_plan(1, 3, 128, 128, 64, 128, act=True).kw


def test_kw_conditions(ops):
    """kw-reuse: 27 taps, W >= 64, Cout <= 128, a raw output, no fused activation, and either no workspace or more than
    128 tiles of 256 rows (below that, a call with a workspace belongs to split-K)."""
    kw = ops.conv3d_plan(1, 1, 2, 64, 64, 8, workspace=NO_WS)
    assert kw.kw and (kw.tile_rows, kw.tile_cols, kw.row_tiles, kw.col_tiles) == (256, 128, 1, 1), kw
    assert kw.slices == 1 and kw.ksteps == 9 * 64 // 32 and not kw.tail, kw
    assert not ops.conv3d_plan(1, 1, 2, 63, 64, 8, workspace=NO_WS).kw                      # W < 64
    assert not ops.conv3d_plan(1, 1, 2, 64, 64, 8, taps_d=1, workspace=NO_WS).kw            # 9 taps
    assert not ops.conv3d_plan(1, 1, 2, 64, 64, 136, workspace=NO_WS).kw                    # two column tiles
    assert ops.conv3d_plan(1, 1, 2, 64, 64, 128, workspace=NO_WS).kw
    assert not ops.conv3d_plan(1, 1, 2, 64, 64, 128, workspace=NO_WS, act=True).kw
    # with a workspace: only above 128 tiles (129 x 256 rows = 33024 voxels)
    assert not ops.conv3d_plan(1, 4, 64, 128, 128, 128, workspace=BIG).kw                   # 32768 rows = 128 tiles
    assert ops.conv3d_plan(1, 4, 64, 128, 128, 128, workspace=BIG).split_k
    pl = ops.conv3d_plan(1, 4, 64, 129, 128, 128, workspace=BIG)                            # 33024 rows = 129 tiles
    assert pl.kw and not pl.split_k, pl
    for W in (64, 65, 131, 257, 300):
        pl = ops.conv3d_plan(2, 3, 3, W, 192, 48, workspace=NO_WS)
        assert pl.kw and pl.ksteps == 54, pl
        _covers(pl, 18 * W, 48)


def test_tail_conditions(ops):
    """A tail launch of lower tiles takes the rows past the last whole round of 256 workgroups: more than one round, a
    short last round of whole row tiles, and at most 256 tail tiles."""
    # kw: 66306 rows = 260 tiles of 256: 256 main tiles, 770 rows in 7 tail tiles of 128
    pl = ops.conv3d_plan(1, 2, 129, 257, 64, 128, workspace=NO_WS)
    assert pl.kw and (pl.row_tiles, pl.tail_tile_rows, pl.tail_m_base, pl.tail_row_tiles) == (256, 128, 65536, 7), pl
    _covers(pl, 66306, 128)
    assert ops.conv3d_plan(1, 2, 129, 257, 64, 128) == pl                                   # with conv3d's workspace too
    # per-tap 256-row tile: 65880 rows = 258 tiles; per-tap 160-row tile: 41040 rows = 257 tiles
    pl = ops.conv3d_plan(1, 3, 366, 60, 64, 128, workspace=NO_WS)
    assert not pl.kw and (pl.tile_rows, pl.row_tiles, pl.tail_tile_rows, pl.tail_m_base, pl.tail_row_tiles) == (256, 256, 128, 65536, 3), pl
    _covers(pl, 65880, 128)
    pl = ops.conv3d_plan(1, 2, 342, 60, 64, 256, workspace=NO_WS)
    assert (pl.tile_rows, pl.row_tiles, pl.tail_tile_rows, pl.tail_m_base, pl.tail_row_tiles) == (160, 256, 96, 40960, 1), pl
    _covers(pl, 41040, 256)
    # exactly one round, or a last round that is whole: no tail
    assert not ops.conv3d_plan(1, 4, 256, 64, 64, 128, workspace=NO_WS).tail                # 65536 rows = 256 tiles
    assert not ops.conv3d_plan(1, 8, 256, 64, 64, 128, workspace=NO_WS).tail                # 512 tiles
    assert not ops.conv3d_plan(1, 1, 200, 60, 64, 128, workspace=NO_WS).tail                # 47 tiles: under one round
    # a last round too long to fit 256 tail tiles: 256 + 129 row tiles -> 258 tail tiles of 128 rows
    pl = ops.conv3d_plan(1, 1, 385 * 4, 64, 64, 128, workspace=NO_WS)
    assert pl.row_tiles == 385 and not pl.tail, pl
    pl = ops.conv3d_plan(1, 1, 384 * 4, 64, 64, 128, workspace=NO_WS)                       # 128 row tiles -> 256 tail tiles
    assert (pl.row_tiles, pl.tail_row_tiles) == (256, 256) and pl.tail, pl
    # two column tiles: 300 row tiles x 2 = 600 tiles, 88 past the second round = 44 row tiles -> 74 tail row tiles of 96
    pl = ops.conv3d_plan(1, 1, 800, 60, 64, 512, workspace=NO_WS)
    assert (pl.tile_rows, pl.col_tiles, pl.row_tiles, pl.tail_m_base, pl.tail_row_tiles) == (160, 2, 256, 40960, 74), pl
    _covers(pl, 48000, 512)


def test_plan_refuses_what_the_launch_refuses(ops):
    from mlx_video_amd._lib import LtxkError
    with pytest.raises(LtxkError, match="multiple of 64"):
        ops.conv3d_plan(1, 1, 4, 4, 96, 128)
    with pytest.raises(LtxkError, match="multiple of 8"):
        ops.conv3d_plan(1, 1, 4, 4, 64, 100)
    with pytest.raises(LtxkError, match="bad volume"):
        ops.conv3d_plan(1, 1, 1, 4, 64, 128)
    with pytest.raises(LtxkError, match="taps_d"):
        ops.conv3d_plan(1, 1, 4, 4, 64, 128, taps_d=2)
    with pytest.raises(LtxkError, match="Cout == 128 or 256"):
        ops.conv3d_plan(1, 1, 4, 4, 64, 64, act=True)
    with pytest.raises(LtxkError, match="16-byte aligned"):
        ops.conv3d_plan(1, 1, 4, 4, 64, 128, workspace=(A + 8, 1 << 20))
    with pytest.raises(LtxkError, match="4 GiB"):
        ops.conv3d_plan(1, 64, 1024, 1024, 64, 128)
