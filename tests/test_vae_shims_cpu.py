"""The VAE / upsampler rows of the refusal table of tests/test_ops_shims_cpu.py (one table, one generator: the rows of the
other shims run there), and the model constructors' bf16 normalisation of their weights."""
import pytest

import test_ops_shims_cpu as table
from test_ops_shims_cpu import BF, F32, nc, z

VAE_CASES = [c for c in table.CASES if c[1] in table.VAE_SHIMS]


@pytest.mark.parametrize("shim", sorted(table.VAE_SHIMS))
def test_well_formed_cpu_operands_are_refused_for_the_device_only(shim):
    table.test_well_formed_cpu_operands_are_refused_for_the_device_only(shim)


@pytest.mark.parametrize("shim,args,kw,exc,operand", [c[1:] for c in VAE_CASES], ids=[c[0] for c in VAE_CASES])
def test_shims_refuse_bad_operands_before_any_launch(shim, args, kw, exc, operand):
    table.test_shims_refuse_bad_operands_before_any_launch(shim, args, kw, exc, operand)


# ------------------------------------------------------------------------------------------------- constructors
def _decoder_weights(dtype):
    return {"conv_in.conv.weight": z(8, 3, 3, 3, 8, dtype=dtype), "conv_out.conv.weight": z(8, 3, 3, 3, 8, dtype=dtype),
            "up_blocks.1.conv.weight": z(8, 3, 3, 3, 8, dtype=dtype), "latents_mean": z(128, dtype=dtype), "latents_std": z(128, dtype=dtype)}


def _encoder_weights(dtype):
    return {"conv_in.weight": z(8, 3, 3, 3, 64, dtype=dtype), "conv_out.weight": z(129, 3, 3, 3, 8, dtype=dtype),
            "conv_out.bias": z(129, dtype=dtype), "per_channel_statistics.mean": z(128, dtype=dtype),
            "per_channel_statistics.std": z(128, dtype=dtype)}


def _upsampler_weights(dtype):
    return {"initial_conv.weight": z(8, 3, 3, 3, 8, dtype=dtype), "upsampler.conv.weight": z(32, 3, 3, 8, dtype=dtype),
            "initial_norm.weight": z(8, dtype=dtype)}


@pytest.mark.parametrize("which", ["decoder", "encoder", "upsampler"])
def test_constructors_keep_bf16_weights_and_convert_the_rest(which):
    from mlx_video_amd.upsampler import LatentUpsampler
    from mlx_video_amd.video_vae import LTX2VideoDecoder, VideoEncoder
    cls, make = {"decoder": (LTX2VideoDecoder, _decoder_weights), "encoder": (VideoEncoder, _encoder_weights),
                 "upsampler": (LatentUpsampler, _upsampler_weights)}[which]
    w32 = make(F32)
    m = cls(w32)
    assert all(m.W[k].dtype == BF and m.W[k].is_contiguous() for k in w32)
    wbf = make(BF)
    m = cls(wbf)
    assert all(m.W[k] is wbf[k] for k in wbf)                                  # no copy, no launch
    strided = {k: nc(v) for k, v in make(BF).items()}
    m = cls(strided)
    assert all(m.W[k].is_contiguous() and m.W[k].dtype == BF for k in strided)
