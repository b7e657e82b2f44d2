"""The ops.gemm launches of one LTXModel.forward_tokens as a table (no test in here: a helper of test_gemm_plan_cpu.py,
test_batch_invariance_gpu.py and test_dit_launch_trace_gpu.py, which holds the forward itself to this table)."""

D = 4096


def dit_launches(ops, B, T, S=64, D=D, caption=3840, U=1):
    """(name, M, N, K, gemm options) of every ops.gemm of one LTXModel.forward_tokens (fuse=15, U distinct timestep rows) with B
    batch rows of T video tokens and S text tokens; "qk" / "v" are the two launches of fuse without bit 1 (or with bit 8)."""
    M, Mc = B * T, B * S
    return [("patchify", M, D, 128, dict(sumsq=True)),
            ("caption1", Mc, D, caption, dict(epilogue=ops.EPI_BIAS_GELU)),
            ("caption2", Mc, D, D, {}),
            ("text_kv", Mc, 2 * D, D, dict(n_split=D, out_tokens_per_batch=S, sumsq=True)),
            ("text_k", Mc, D, D, dict(sumsq=True)),
            ("text_v", Mc, D, D, dict(out_tokens_per_batch=S)),
            ("timestep1", U, D, 256, dict(epilogue=ops.EPI_BIAS_SILU)),
            ("timestep2", U, D, D, {}),
            ("adaln", U, 6 * D, D, {}),
            ("qkv", M, 3 * D, D, dict(n_split=2 * D, out_tokens_per_batch=T, sumsq=True)),
            ("qk", M, 2 * D, D, dict(sumsq=True)),
            ("v", M, D, D, dict(out_tokens_per_batch=T)),
            ("out", M, D, D, dict(epilogue=ops.EPI_BIAS_GATE_RES, sumsq=True)),
            ("q2", M, D, D, dict(sumsq=True)),
            ("o2", M, D, D, dict(epilogue=ops.EPI_BIAS_RES, sumsq=True)),
            ("ff1", M, 4 * D, D, dict(epilogue=ops.EPI_BIAS_GELU)),
            ("ff2", M, D, 4 * D, dict(epilogue=ops.EPI_BIAS_GATE_RES, sumsq=True)),
            ("proj_out", M, 128, D, {})]
