"""Joint audio-video denoising, the parts that need no device: the AudioVideo restatement (ref_av_dit) against oracle.dit in the
degenerate case, the cross positional tables, planted faults against the yardstick of the GPU tests, the three-way key split of
a joint checkpoint, and the surface's parser and refusals."""
import pytest
import torch

import ref_av_dit as RA
from oracle import dit as O

BF = torch.bfloat16
SIGMA = 0.725
# the tiny model of tests/test_av_dit_gpu.py
CFG_V = O.DiTConfig(num_layers=2, heads=8, d_head=128, caption_channels=256)
CFG_A = O.DiTConfig(num_layers=2, heads=8, d_head=64, caption_channels=256, max_pos=(20,))


def _rel(a, b) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm())


def tiny_case(Ta: int, seed: int, B: int = 2, S: int = 70, grid=(3, 5, 5)):
    """Inputs of one forward at the GPU test's tiny shape: N = 75 video tokens, Ta audio frames."""
    from mlx_video_amd.schedulers import create_audio_position_grid
    g = torch.Generator().manual_seed(seed)
    N = grid[0] * grid[1] * grid[2]
    c = dict(vlat=torch.randn(B, N, 128, generator=g).to(BF), alat=torch.randn(B, Ta, 128, generator=g).to(BF),
             vctx=torch.randn(B, S, 256, generator=g).to(BF), actx=torch.randn(B, S, 256, generator=g).to(BF),
             vpos=torch.from_numpy(O.create_position_grid(B, *grid)), apos=create_audio_position_grid(B, Ta),
             vts=torch.full((B, N), O.bf16_round_scalar(SIGMA)), ats=torch.full((B, Ta), O.bf16_round_scalar(SIGMA)))
    c["vpe"] = O.precompute_freqs_cis(c["vpos"], CFG_V.dim, CFG_V.theta, CFG_V.max_pos, CFG_V.heads)
    c["ape"] = O.precompute_freqs_cis(c["apos"], CFG_A.dim, CFG_A.theta, CFG_A.max_pos, CFG_A.heads)
    c["vcpe"] = RA.cross_freqs_cis(c["vpos"], CFG_V, CFG_A, CFG_V.heads)
    c["acpe"] = RA.cross_freqs_cis(c["apos"], CFG_V, CFG_A, CFG_A.heads)
    return c


def forward(c, W, p, **kw):
    Wv, Wa, Wc = W
    return RA.av_forward(c["vlat"], c["vts"], c["vctx"], c["vpe"], c["vcpe"], c["alat"], c["ats"], c["actx"], c["ape"], c["acpe"],
                         Wv, Wa, Wc, CFG_V, CFG_A, p, **kw)


@pytest.fixture(scope="module")
def weights():
    return RA.make_av_weights(CFG_V, CFG_A, seed=7)


@pytest.fixture(scope="module")
def case():
    return tiny_case(21, 32)


@pytest.mark.parametrize("p", [O.F64, O.BF16_FLASH], ids=["f64", "bf16_flash"])
def test_zeroed_cross_out_is_two_independent_forwards(weights, case, p):
    Wv, Wa, Wc = weights
    v, a, hv, ha = forward(case, (Wv, Wa, RA.zero_cross_out(Wc)), p, return_hidden=True)
    v1, hv1 = O.ltx_forward(case["vlat"], case["vts"], case["vctx"], case["vpe"], Wv, CFG_V, p, return_hidden=True)
    a1, ha1 = O.ltx_forward(case["alat"], case["ats"], case["actx"], case["ape"], Wa, CFG_A, p, return_hidden=True)
    assert torch.equal(v, v1) and torch.equal(a, a1)
    assert all(torch.equal(x, y) for x, y in zip(hv + ha, hv1 + ha1))
    # and with the cross weights live the streams do see each other
    v2, a2 = forward(case, weights, p)
    assert not torch.equal(v2, v1) and not torch.equal(a2, a1)


def test_cross_tables_are_the_one_axis_table_of_the_time_axis(case):
    from mlx_video_amd.av_model import LTXAVModel
    for pos, heads, T in ((case["vpos"], CFG_V.heads, 75), (case["apos"], CFG_A.heads, 21)):
        ref = O.precompute_freqs_cis(pos[:, 0:1], CFG_A.dim, CFG_A.theta, (20,), heads)
        got = RA.cross_freqs_cis(pos, CFG_V, CFG_A, heads)
        assert all(torch.equal(x, y) for x, y in zip(got, ref)) and tuple(got[0].shape) == (2, heads, T, 32)
        # the package's host table: the same fp32 angles, cos / sin evaluations within 2 ulp (test_audio_dit_cpu's argument)
        host = LTXAVModel.cross_freqs_cis(_Shim(), pos, heads)
        for x, y in zip(host, ref):
            ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(x.abs(), y.abs()).clamp_min(2.0 ** -126))) - 23)
            assert tuple(x.shape) == tuple(y.shape) and float(((x - y).abs() / ulp).max()) <= 2.0


class _Shim:
    """What LTXAVModel.cross_freqs_cis reads of the model."""
    class audio:
        inner_dim = CFG_A.dim

    class video:
        positional_embedding_theta = CFG_V.theta
    cross_pe_max_pos = 20.0


@pytest.mark.parametrize("fault", ["v2a_post_a2v", "swap_scale_shift", "k_pe_is_pe"])
def test_planted_faults_move_the_velocity_by_more_than_ten_policy_errors(weights, fault):
    """The GPU tests ask device error <= 1.25 * e_ref with e_ref the BF16_FLASH policy's own error against F64.  Each planted
    fault moves a float64 velocity by more than 10 * e_ref at the tiny shape, so that rule sees it."""
    c = tiny_case(70, 33)
    v64, a64 = forward(c, weights, O.F64)
    vp, ap = forward(c, weights, O.BF16_FLASH)
    vf, af = forward(c, weights, O.F64, fault=fault)
    e = {"video": (_rel(vp, v64), _rel(vf, v64)), "audio": (_rel(ap, a64), _rel(af, a64))}
    for k, (e_ref, moved) in e.items():
        print(f"{fault} {k}: e_ref {e_ref:.3e}  moved {moved:.3e}  ratio {moved / e_ref:.1f}")
    assert any(moved > 10 * e_ref for e_ref, moved in e.values())


def test_restated_loop_runs_and_cfg_one_is_the_positive_forward(weights):
    """The loop of ref_av_dit at cfg_scale 1 over one step to sigma 0 is x - sigma * velocity of one forward."""
    c = tiny_case(21, 34, B=1)
    g = torch.Generator().manual_seed(35)
    vlat, alat = torch.randn(1, 128, 3, 5, 5, generator=g).to(BF), torch.randn(1, 8, 21, 16, generator=g).to(BF)
    p, s = O.F64, 0.5
    xv, xa = RA.denoise_dev_av(vlat, alat, c["vpos"], c["apos"], c["vctx"], None, c["actx"], None, *weights, CFG_V, CFG_A, [s, 0.0], p,
                               cfg_scale=1.0)
    vv, va = RA.av_forward(O.latent_to_tokens(p.r(vlat)), torch.full((1, 75), s), c["vctx"], c["vpe"], c["vcpe"], RA.audio_tokens(p.r(alat)),
                           torch.full((1, 21), s), c["actx"], c["ape"], c["acpe"], *weights, CFG_V, CFG_A, p)
    assert torch.equal(xv, p.r(vlat) - s * O.tokens_to_latent(vv, vlat.shape))
    assert torch.equal(xa, p.r(alat) - s * va.reshape(1, 21, 8, 16).permute(0, 2, 1, 3))


# ------------------------------------------------------------------------------------------------ weights
def _joint_keys():
    audio = ["audio_patchify_proj.weight", "audio_adaln_single.linear.bias", "audio_scale_shift_table", "audio_proj_out.weight",
             "transformer_blocks.3.audio_attn1.to_q.weight", "transformer_blocks.3.audio_attn2.to_out.0.bias",
             "transformer_blocks.3.audio_ff.net.0.proj.weight", "transformer_blocks.3.audio_scale_shift_table"]
    video = ["patchify_proj.weight", "scale_shift_table", "transformer_blocks.3.attn1.to_q.weight", "transformer_blocks.3.ff.net.2.bias",
             "transformer_blocks.3.scale_shift_table"]
    cross = ["transformer_blocks.3.audio_to_video_attn.to_q.weight", "transformer_blocks.3.audio_to_video_attn.to_out.0.bias",
             "transformer_blocks.3.video_to_audio_attn.k_norm.weight", "transformer_blocks.3.scale_shift_table_a2v_ca_audio",
             "transformer_blocks.3.scale_shift_table_a2v_ca_video", "av_ca_video_scale_shift_adaln_single.emb.timestep_embedder.linear_1.weight",
             "av_ca_audio_scale_shift_adaln_single.linear.bias", "av_ca_a2v_gate_adaln_single.linear.weight",
             "av_ca_v2a_gate_adaln_single.emb.timestep_embedder.linear_2.bias"]
    other = ["audio_embeddings_connector.learnable_registers", "video_embeddings_connector.transformer_1d_blocks.0.attn1.to_q.weight"]
    return video, audio, cross, other


def test_av_key_split_is_three_disjoint_sets_and_loses_nothing():
    from mlx_video_amd.weights import av_transformer_weights
    video, audio, cross, other = _joint_keys()
    p = "model.diffusion_model."
    raw = {p + k: torch.full((2, 2), float(i)) for i, k in enumerate(video + audio + cross + other)}
    raw["vae.decoder.conv_in.weight"] = torch.zeros(2, 2)
    Wv, Wa, Wc = av_transformer_weights(raw, "cpu", strict=False)
    assert len(Wv) == len(video) and len(Wa) == len(audio) and len(Wc) == len(cross)
    assert set(Wc) == {"transformer_blocks.3.audio_to_video_attn.to_q.weight", "transformer_blocks.3.audio_to_video_attn.to_out.bias",
                       "transformer_blocks.3.video_to_audio_attn.k_norm.weight", "transformer_blocks.3.scale_shift_table_a2v_ca_audio",
                       "transformer_blocks.3.scale_shift_table_a2v_ca_video", "av_ca_video_scale_shift_adaln_single.emb.timestep_embedder.linear1.weight",
                       "av_ca_audio_scale_shift_adaln_single.linear.bias", "av_ca_a2v_gate_adaln_single.linear.weight",
                       "av_ca_v2a_gate_adaln_single.emb.timestep_embedder.linear2.bias"}
    assert "transformer_blocks.3.attn1.to_q.weight" in Wv and "transformer_blocks.3.attn1.to_q.weight" in Wa      # audio under the video names
    # every transformer tensor lands in exactly one set (by value: each raw tensor carries its index), the connectors in none
    vals = sorted(float(t.flatten()[0]) for W in (Wv, Wa, Wc) for t in W.values())
    assert vals == [float(i) for i in range(len(video + audio + cross))]
    assert all(t.dtype == BF for W in (Wv, Wa, Wc) for t in W.values())


def test_av_key_split_names_the_missing_cross_tensors():
    from mlx_video_amd.av_model import LTXAVModel
    from mlx_video_amd.ltx_model import LTXModelConfig
    from mlx_video_amd.weights import av_transformer_weights
    cv = LTXModelConfig(num_attention_heads=8, num_layers=1, caption_channels=256, cross_attention_dim=1024)
    ca = LTXModelConfig.audio(num_attention_heads=8, num_layers=1, caption_channels=256, cross_attention_dim=512)
    Wv, Wa, Wc = RA.make_av_weights(O.DiTConfig(num_layers=1, heads=8, caption_channels=256),
                                    O.DiTConfig(num_layers=1, heads=8, d_head=64, caption_channels=256, max_pos=(20,)), seed=3)
    assert set(Wc) == set(LTXAVModel.expected_cross_keys(cv, ca))
    back = {"audio_attn1.": "attn1.", "audio_attn2.": "attn2.", "audio_ff.": "ff."}

    def audio_raw(k):                  # module key of the audio set -> its name in the joint checkpoint
        if k.startswith("transformer_blocks."):
            head, idx, rest = k.split(".", 2)
            if rest == "scale_shift_table":
                return f"{head}.{idx}.audio_scale_shift_table"
            for old, new in back.items():
                if rest.startswith(new):
                    return f"{head}.{idx}.{old}{rest[len(new):]}"
        return "audio_" + k

    raw = {**Wv, **{audio_raw(k): v for k, v in Wa.items()}, **Wc}
    assert len(raw) == len(Wv) + len(Wa) + len(Wc)
    got = av_transformer_weights(raw, "cpu")
    assert [set(x) for x in got] == [set(Wv), set(Wa), set(Wc)]
    gone = ["transformer_blocks.0.video_to_audio_attn.to_k.weight", "av_ca_v2a_gate_adaln_single.linear.bias"]
    with pytest.raises(ValueError, match="(?s)2 cross-modal.*av_ca_v2a_gate_adaln_single.linear.bias.*video_to_audio_attn.to_k.weight"):
        av_transformer_weights({k: v for k, v in raw.items() if k not in gone}, "cpu")


# ------------------------------------------------------------------------------------------------ surface
def test_joint_parses_and_refuses_what_it_does_not_do():
    from mlx_video_amd import generate as G
    from mlx_video_amd.pipelines import PipelineType
    a = G.build_parser().parse_args(["--audio", "--audio-mode", "joint"])
    assert (a.audio, a.audio_mode) == (True, "joint")
    with pytest.raises(ValueError, match="(?s)joint.*distilled"):
        G.generate_video(audio=True, audio_mode="joint", av_transformer=object(), pipeline=PipelineType.DISTILLED)
    with pytest.raises(ValueError, match="(?s)joint.*stage2_dev"):
        G.generate_video(audio=True, audio_mode="joint", av_transformer=object(), pipeline=PipelineType.DEV, stage2_dev=True)
    with pytest.raises(ValueError, match="(?s)joint.*fp8"):
        G.generate_video(audio=True, audio_mode="joint", av_transformer=object(), pipeline=PipelineType.DEV, enable_fp8=True)
    # "auto" still resolves to separate: an audio transformer gets it past the audio refusals, to the first thing that is missing
    with pytest.raises(FileNotFoundError, match="no transformer"):
        G.generate_video(audio=True, audio_mode="auto", audio_transformer=object())


def test_joint_loop_refuses_stg_and_guiders():
    from mlx_video_amd.denoise import denoise_dev_av
    z = torch.zeros(1)
    for kw, word in ((dict(stg_scale=1.0), "STG"), (dict(guider="apg"), "apg"), (dict(guider="cfg_star"), "cfg_star"),
                     (dict(cache_context=True), "cache_context")):
        with pytest.raises(ValueError, match=f"(?s)joint.*{word}"):
            denoise_dev_av(z, z, z, z, z, z, z, z, None, [1.0, 0.0], **kw)
