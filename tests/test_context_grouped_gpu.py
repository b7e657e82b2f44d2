"""LTXModel with the text K / V^T of all blocks from one grouped launch (grouped_context_kv, the default) against the
per-block launches, BIT FOR BIT: forward_tokens at full width (D=4096), L=4, B=1 and B=2, with and without
batch_invariant; a captured graph replayed against the eager forward; prepare_context + ctx_kv= against the recompute path."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GEOM = (5, 4, 8)          # 160 video tokens


@pytest.fixture(scope="module")
def model(dev):
    from mlx_video_amd.ltx_model import LTXModel, LTXModelConfig
    return LTXModel.random_init(LTXModelConfig(num_layers=4), dev, seed=33)


def _inputs(dev, B, S, seed):
    from mlx_video_amd.ltx_model import TimestepPlan, precompute_freqs_cis
    from mlx_video_amd.schedulers import create_position_grid
    T = GEOM[0] * GEOM[1] * GEOM[2]
    g = torch.Generator(device=dev).manual_seed(seed)
    tok = torch.randn((B, T, 128), generator=g, device=dev).to(BF)
    ctx = torch.randn((B, S, 3840), generator=g, device=dev).to(BF)
    pe = precompute_freqs_cis(create_position_grid(1, *GEOM).to(dev), 4096)
    plan = TimestepPlan(torch.tensor([0.625], dtype=BF, device=dev), torch.zeros(B * T, dtype=torch.int32, device=dev))
    return tok, plan, ctx, pe


def _forward(model, grouped, *args, **kw):
    model.grouped_context_kv = grouped
    try:
        return model.forward_tokens(*args, **kw)
    finally:
        model.grouped_context_kv = True


# (S = 77 in batch_invariant mode only: at M = 154 text rows the default mode's per-block launches split K, so the forward keeps
# them there - test_default_mode_keeps_per_block_launches_where_they_split_k)
@pytest.mark.parametrize("B,S,invariant", [(1, 1024, False), (2, 1024, False), (1, 1024, True), (2, 1024, True), (2, 77, True)])
def test_forward_grouped_equals_per_block(dev, model, B, S, invariant):
    args = _inputs(dev, B, S, 10 * B + S)
    model.batch_invariant = invariant
    try:
        assert model._grouped_context_ok(B, S), "the grouped path is not taken at this shape: the comparison would be empty"
        got = _forward(model, True, *args)
        ref = _forward(model, False, *args)
    finally:
        model.batch_invariant = False
    assert torch.equal(got, ref)
    assert bool(torch.isfinite(got.float()).all())


def test_default_mode_keeps_per_block_launches_where_they_split_k(dev, model):
    from mlx_video_amd import ops
    assert ops.gemm_plan(154, 8192, 4096, n_split=4096, out_tokens_per_batch=77, sumsq=True).split_k
    assert not model._grouped_context_ok(2, 77)
    model.batch_invariant = True
    try:
        assert model._grouped_context_ok(2, 77)
    finally:
        model.batch_invariant = False


def test_graph_replay_equals_eager(dev, model):
    args = _inputs(dev, 2, 1024, 77)
    eager = _forward(model, True, *args)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.forward_tokens(*args)                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.forward_tokens(*args)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_prepared_context_equals_recompute(dev, model):
    tok, plan, ctx, pe = _inputs(dev, 2, 1024, 5)
    kv = model.prepare_context(ctx)
    assert kv.stacked is not None and kv.kv[3][0].data_ptr() == kv.stacked[0][3].data_ptr()
    ref = model.forward_tokens(tok, plan, ctx, pe)
    assert torch.equal(model.forward_tokens(tok, plan, ctx, pe, ctx_kv=kv), ref)
    # refreshed in place for a new prompt: same buffers, new contents; and equal to the per-block preparation
    ctx2 = torch.randn(ctx.shape, generator=torch.Generator(device=dev).manual_seed(6), device=dev).to(BF)
    ptr = kv.stacked[0].data_ptr()
    model.prepare_context(ctx2, out=kv)
    assert kv.stacked[0].data_ptr() == ptr
    model.grouped_context_kv = False
    try:
        per_block = model.prepare_context(ctx2)
    finally:
        model.grouped_context_kv = True
    for a, b in zip(kv.kv, per_block.kv):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
