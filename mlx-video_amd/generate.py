"""Pipeline driver with the surface of ``mlx_video.generate`` (generate.py:2035-4197, main() 4200-4758):
``generate_video(...)`` for the distilled / dev / keyframe / ic_lora pipelines and a CLI.

What is kept: argument names and meaning, dimension padding (/64 distilled-style, /32 dev) with crop
back, frames -> 1+8k round-up, sigma schedules and subsampling, conditioning semantics (replace /
guide, per-pipeline forcing), two-stage flow (half-res stage 1 -> latent upsample -> re-noise ->
stage 2, optional stage-2 LoRA transformer), tiling policy, the `_PhaseTimer` phase names
(`stage1_denoise`, `upsample`, `stage2_denoise`, `dev_denoise`, `vae_decode`, `to_uint8_numpy`) and
the `--profile-json` payload.

What is injected instead of loaded (nothing exists offline and they are out of scope, SURVEY.md §2a
#17/#21): text embeddings (the Gemma-3 text encoder's output tensor is an INPUT of this path), model
weights (`weights=` dicts or ready modules; `model_repo` may point at a local directory of
safetensors read by ``weights.py``), random draws (`noise_fn`: MLX's threefry stream is not
reproducible, so seeds are not cross-compatible), audio (`audio=True`: separate generation by an audio-only transformer after the
video, `audio_mode="joint"`: audio and video denoised together by the AudioVideo transformer, or finished `audio_latents=`; either
way decoded to a waveform by ``audio_vae``).  Frames are returned as the reference returns them (uint8 (F,H,W,3));
`output_path` accepts `.npy`, or a video file written through an ffmpeg child process when an ffmpeg binary
is installed (media.write_video_ffmpeg); a decoded waveform goes to a `.wav` sidecar and is muxed into that file the same way.
"""
from __future__ import annotations

import argparse
import json
import math
import time
from contextlib import contextmanager
from enum import Enum
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .conditioning import (LatentState, VideoConditionByKeyframeIndex, VideoConditionByLatentIndex, apply_conditioning,
                           noise_blend)
from . import ops
from .denoise import denoise_dev, denoise_distilled
from .ltx_model import LTXModel, LTXModelConfig
from .schedulers import (STAGE_1_SIGMAS, STAGE_2_SIGMAS, _subsample_refinement_sigmas, _subsample_sigmas,
                         create_position_grid, ltx2_scheduler)
from .video_vae import LTX2VideoDecoder, TilingConfig, VideoEncoder, to_uint8_frames

BF16 = torch.bfloat16
DEFAULT_NEGATIVE_PROMPT = ""


class PipelineType(Enum):
    """generate.py:299-304."""
    DISTILLED = "distilled"
    DEV = "dev"
    KEYFRAME = "keyframe"
    IC_LORA = "ic_lora"


class _PhaseTimer:
    """generate.py:64-94 (phases are closed with a device sync so they mean GPU time)."""

    def __init__(self, enabled: bool):
        self.enabled = enabled
        self.times_s: Dict[str, float] = {}

    @contextmanager
    def phase(self, name: str):
        if not self.enabled:
            yield
            return
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            yield
        finally:
            torch.cuda.synchronize()
            self.times_s[name] = self.times_s.get(name, 0.0) + (time.perf_counter() - t0)

    def render(self, elapsed_s: float) -> str:
        if not self.times_s:
            return ""
        total = sum(self.times_s.values())
        denom = total if total > 0 else (elapsed_s if elapsed_s > 0 else 1.0)
        lines = [f"{n:>18}: {dt:6.2f}s ({100.0 * dt / denom:5.1f}%)"
                 for n, dt in sorted(self.times_s.items(), key=lambda kv: kv[1], reverse=True)]
        lines += [f"{'total(phases)':>18}: {total:6.2f}s", f"{'elapsed(wall)':>18}: {elapsed_s:6.2f}s"]
        return "\n".join(lines)


def _default_noise_fn(seed: int, device) -> Callable[[Tuple[int, ...]], torch.Tensor]:
    g = torch.Generator(device=device).manual_seed(int(seed))
    return lambda shape: torch.randn(shape, generator=g, device=device, dtype=torch.float32).to(BF16)


def _pad_dims(height: int, width: int, divisor: int):
    """generate.py:2238-2259: pad to a multiple of `divisor`, remember the crop."""
    if height % divisor == 0 and width % divisor == 0:
        return height, width, None
    ph, pw = (-height) % divisor, (-width) % divisor
    top, left = ph // 2, pw // 2
    return height + ph, width + pw, (top, left, height, width)


def _round_frames(num_frames: int) -> int:
    """generate.py:2261-2266: round UP to 1 + 8k."""
    return num_frames if num_frames % 8 == 1 else ((num_frames - 1 + 7) // 8) * 8 + 1


def _resolve_frame_idx(frame_idx: int, num_frames: int, latent_frames: int) -> int:
    """generate.py:2612-2619."""
    if frame_idx < latent_frames:
        return frame_idx
    if num_frames <= 1 or latent_frames <= 1:
        return 0
    return int(max(0, min(latent_frames - 1, int((frame_idx / (num_frames - 1) * (latent_frames - 1)) + 0.5))))


def _cond_pixels(src, height: int, width: int, is_video: bool, num_frames: int, device=None) -> torch.Tensor:
    """One conditioning source at one stage's resolution -> (1,3,F,height,width) in [-1,1].
    Paths go through media.load_image / load_frames on the host (utils.py:529-613: LANCZOS for images, an area filter on
    the decoded uint8 frames for video, frame_cap=num_frames).  Pixel tensors (1,3,F,H,W) in [-1,1] of another size are
    resized the way prepare_image_for_encoding / prepare_video_for_encoding do (utils.py:643-715): images through uint8 +
    LANCZOS on the host (one frame); VIDEO frames with cv2.INTER_AREA on the float frames - here the HIP kernel
    ltxk_resize_area on the device (65 frames of 768x768 cost 1.0 s as a host loop, config 5), bf16 out."""
    from . import media
    if isinstance(src, (str, Path)):
        if is_video:
            return media.frames_to_conditioning(media.load_frames(src, height, width, frame_cap=num_frames))
        return media.image_to_conditioning(media.load_image(src, height=height, width=width))
    if isinstance(src, np.ndarray):
        src = torch.from_numpy(src)
    if not torch.is_tensor(src) or src.dim() != 5 or src.shape[1] != 3:
        raise ValueError("conditioning source must be a path, or a (1,3,F,H,W) pixel tensor in [-1,1]")
    t = src.detach()
    if is_video:
        t = t[:, :, :num_frames]
        t = t[:, :, : 1 + ((t.shape[2] - 1) // 8) * 8]            # the encoder takes 1+8k frames (video_vae.py:332-337)
    if tuple(t.shape[-2:]) == (height, width):
        return t
    if is_video and height <= t.shape[-2] and width <= t.shape[-1] and device is not None:
        td = t.to(device)
        return ops.resize_area(td if td.dtype in (torch.float32, BF16) else td.float(), height, width)
    t = t.to("cpu", torch.float32)
    frames01 = ((t[0].permute(1, 2, 3, 0) + 1.0) / 2.0).clamp(0, 1).numpy()        # (F,H,W,3) in [0,1]
    return media.resize_conditioning(frames01, height, width, is_video)


def _encode_conditionings(items, encoder: Optional[VideoEncoder], height: int, width: int, num_frames: int,
                          latent_frames: int, guide: bool, device, is_video: bool = False):
    """items: (path | pixels (1,3,F,H,W) in [-1,1] | latent (1,128,f,h,w), frame_idx, strength).  Pixels are
    brought to the stage's resolution and encoded with the VAE encoder (generate.py:3064-3113)."""
    out = []
    for src, frame_idx, strength in items:
        if torch.is_tensor(src) and src.dim() == 5 and src.shape[1] == 128:
            t = src.to(device).to(BF16)                                             # already a latent
        else:
            if encoder is None:
                raise ValueError("pixel conditioning needs a VAE encoder (pass vae_encoder= or a model_repo with VAE encoder weights)")
            t = encoder(_cond_pixels(src, height, width, is_video, num_frames, device).to(device).to(BF16))
        idx = _resolve_frame_idx(int(frame_idx), num_frames, latent_frames)
        out.append(VideoConditionByKeyframeIndex(t, idx, float(strength)) if guide
                   else VideoConditionByLatentIndex(t, idx, float(strength)))
    return out


def _layer_stack(hs) -> torch.Tensor:
    """(L,B,T,D) from a stack, a list of (B,T,D) layers, or the batchless (L,T,D) a file holds."""
    x = torch.stack(list(hs), 0) if isinstance(hs, (list, tuple)) else hs
    if x.dim() == 3:
        x = x[:, None]
    if x.dim() != 4:
        raise ValueError(f"gemma hidden states must be (L,B,T,D), (L,T,D) or a list of L (B,T,D) tensors, got {tuple(x.shape)}")
    return x


def _connect_gemma(hs, mask, neg_hs, neg_mask, text_connector, model_repo, dev, want_audio: bool = False):
    """(prompt_embeds, negative_prompt_embeds or None) from Gemma hidden states: one TextConnector call, B = 2 with a negative.
    ``want_audio``: a third item, the positive prompt's AUDIO context from the audio embeddings connector over the same
    features (``TextConnector.both``) - None when the connector that was passed in has no audio set."""
    if mask is None or (neg_hs is not None and neg_mask is None):
        raise ValueError("gemma_hidden_states need their gemma_attention_mask (and the negative pair its own)")
    if text_connector is None:
        if model_repo is None:
            raise ValueError("gemma_hidden_states were given without a text connector: pass text_connector= (a TextConnector) or a "
                             "model_repo whose checkpoint holds the connector weights")
        from .text_connector import TextConnector
        from .weights import text_connector_weights
        root = Path(model_repo)
        files = [f for f in sorted(root.glob("*.safetensors")) if "upscaler" not in f.name and "upsampler" not in f.name]
        files = files + sorted((root / "connectors").glob("*.safetensors"))
        text_connector = TextConnector(text_connector_weights(files, dev),
                                       text_connector_weights(files, dev, which="audio") if want_audio else None)
    x, m = _layer_stack(hs).to(dev), mask.reshape(-1, mask.shape[-1]).to(dev)
    if want_audio:
        both = text_connector.audio_blocks is not None
        run = text_connector.both if both else (lambda a, b: (text_connector(a, b), None))
        if neg_hs is not None:
            nx, nm = _layer_stack(neg_hs).to(dev), neg_mask.reshape(-1, neg_mask.shape[-1]).to(dev)
            if nx.shape != x.shape or x.shape[1] != 1:
                raise ValueError(f"positive and negative gemma hidden states must both be (L,1,T,D) of one shape, got {tuple(x.shape)} and {tuple(nx.shape)}")
            x, m = torch.cat([x, nx], 1), torch.cat([m, nm], 0)
        video, aud = run(x, m)
        # (a fourth item: the NEGATIVE prompt's audio context, which joint denoising's CFG takes)
        return (video[0:1], (video[1:2] if neg_hs is not None else None), (aud[0:1] if aud is not None else None),
                (aud[1:2] if aud is not None and neg_hs is not None else None))
    if neg_hs is None:
        return text_connector(x, m), None
    nx, nm = _layer_stack(neg_hs).to(dev), neg_mask.reshape(-1, neg_mask.shape[-1]).to(dev)
    if nx.shape != x.shape or x.shape[1] != 1:
        raise ValueError(f"positive and negative gemma hidden states must both be (L,1,T,D) of one shape, got {tuple(x.shape)} and {tuple(nx.shape)}")
    out = text_connector(torch.cat([x, nx], 1), torch.cat([m, nm], 0))
    return out[0:1], out[1:2]


def _as_tokens(tokens, what: str):
    """(input_ids, attention_mask) as (1,T) tensors from a pair of tensors / arrays / lists."""
    if not isinstance(tokens, (tuple, list)) or len(tokens) != 2:
        raise ValueError(f"{what} must be an (input_ids, attention_mask) pair")
    ids, mask = (torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t) for t in tokens)
    ids, mask = ids.reshape(-1, ids.shape[-1]), mask.reshape(-1, mask.shape[-1])
    if ids.shape != mask.shape or ids.shape[0] != 1:
        raise ValueError(f"{what}: input_ids and attention_mask must both be (T,) or (1,T), got {tuple(ids.shape)} and {tuple(mask.shape)}")
    return ids, mask


def _encode_gemma(gemma, gemma_repo, tokenizer_path, prompt, negative_prompt, prompt_tokens, negative_prompt_tokens, dev, fp8=None):
    """(hidden states (L+1,2,T,D), mask (2,T)) of the positive and the negative prompt: tokens -> GemmaEncoder as ONE B = 2 call.
    Tokens are taken as given, or made from the prompt strings with the tokenizer.json of ``tokenizer_path`` / ``gemma_repo``."""
    from .gemma import GemmaConfig, GemmaEncoder, load_tokenizer, tokenize
    if gemma is None:
        from .weights import gemma_weights
        gemma = GemmaEncoder(gemma_weights(gemma_repo, dev, fp8=fp8), GemmaConfig.from_json(gemma_repo), fp8=fp8)
    if prompt_tokens is None or negative_prompt_tokens is None:
        where = tokenizer_path or gemma_repo
        if where is None:
            raise ValueError("a Gemma encoder was given without tokens: pass prompt_tokens= and negative_prompt_tokens= "
                             "((input_ids, attention_mask) pairs), or tokenizer_path= / gemma_repo= a local directory with a tokenizer.json")
        tok = load_tokenizer(where)
    pos = _as_tokens(prompt_tokens, "prompt_tokens") if prompt_tokens is not None else tokenize(tok, [prompt])
    neg = _as_tokens(negative_prompt_tokens, "negative_prompt_tokens") if negative_prompt_tokens is not None else tokenize(tok, [negative_prompt])
    if pos[0].shape != neg[0].shape:
        raise ValueError(f"positive and negative prompt tokens must have one length, got {tuple(pos[0].shape)} and {tuple(neg[0].shape)}")
    ids, mask = torch.cat([pos[0], neg[0]], 0), torch.cat([pos[1], neg[1]], 0)
    return gemma(ids, mask), mask


def _check_enhance(gemma, gemma_repo, text_encoder_repo, tokenizer_path, prompt_tokens, prompt_embeds, gemma_hidden_states, text_encoder):
    """enhance_prompt's preconditions, before anything is loaded: a Gemma-3 model, a tokenizer, and a prompt read as a string."""
    if gemma_repo is None and text_encoder_repo and Path(text_encoder_repo).is_dir():
        gemma_repo = text_encoder_repo
    missing = []
    if gemma is None and gemma_repo is None:
        missing.append("a Gemma-3 model: gemma= (a GemmaEncoder) or gemma_repo= (a local Gemma-3 directory, --gemma-repo)")
    if tokenizer_path is None and gemma_repo is None:
        missing.append("a tokenizer: tokenizer_path= (--tokenizer) or gemma_repo= a local directory with a tokenizer.json")
    if missing:
        raise ValueError("enhance_prompt (--enhance-prompt) needs " + " and ".join(missing))
    given = [n for n, v in (("prompt_tokens", prompt_tokens), ("prompt_embeds", prompt_embeds), ("gemma_hidden_states", gemma_hidden_states),
                            ("text_encoder", text_encoder)) if v is not None]
    if given:
        raise ValueError(f"enhance_prompt (--enhance-prompt) rewrites the prompt string, which {', '.join(given)} replaces: drop one of the two")


def _enhance_prompt(gemma, gemma_repo, tokenizer_path, prompt, system_prompt, max_tokens, temperature, seed, dev, verbose, fp8=None,
                    device_loop=False, mxfp4=False):
    """(the GemmaEncoder, the enhanced prompt): the encoder is built here when only ``gemma_repo`` was given, and handed on so that
    the text encode that follows reuses its panels."""
    from .gemma import GemmaConfig, GemmaEncoder, GemmaGenerator, enhance_prompt, load_tokenizer
    if gemma is None:
        from .weights import gemma_weights
        gemma = GemmaEncoder(gemma_weights(gemma_repo, dev, fp8=fp8), GemmaConfig.from_json(gemma_repo), fp8=fp8)
    tok = load_tokenizer(tokenizer_path or gemma_repo)
    generator = GemmaGenerator(gemma, **({"decode_panels": "mxfp4"} if mxfp4 else {}))
    enhanced = enhance_prompt(generator, tok, prompt, system_prompt, max_tokens=max_tokens, temperature=temperature, seed=seed,
                              **({"device_loop": True} if device_loop else {}),          # (off adds no keyword: today's call)
                              **({"mxfp4": True} if mxfp4 else {}))
    if verbose:
        print(f"enhanced prompt: {enhanced}")
    return gemma, enhanced


def generate_video(model_repo: Optional[str] = None, text_encoder_repo: Optional[str] = None, prompt: str = "",
                   pipeline: PipelineType = PipelineType.DISTILLED, negative_prompt: str = DEFAULT_NEGATIVE_PROMPT,
                   height: int = 512, width: int = 512, num_frames: int = 33, num_inference_steps: int = 40,
                   cfg_scale: float = 4.0, seed: int = 42, fps: float = 24.0, output_path: Optional[str] = None,
                   save_frames: bool = False, verbose: bool = False, profile: bool = False,
                   profile_json_path: Optional[str] = None, image=None, image_strength: float = 1.0,
                   image_frame_idx: int = 0, images: Optional[list] = None, video_conditionings: Optional[list] = None,
                   distilled_loras: Optional[list] = None, conditioning_mode: str = "replace", tiling: str = "auto",
                   stream: bool = False, audio: bool = False, eval_interval: int = 1, compile_step: bool = False,
                   compile_shapeless: bool = False, cfg_batch: bool = False, fp32_euler: bool = True,
                   loras: Optional[list] = None, stage2_dev: bool = False, stage1_steps: int = 8, stage2_steps: int = 3,
                   sigma_subsample: str = "farthest",
                   # ---- injected in place of what the reference downloads / samples ----
                   transformer: Optional[LTXModel] = None, stage2_transformer: Optional[LTXModel] = None,
                   transformer_weights: Optional[Dict[str, torch.Tensor]] = None, transformer_config: Optional[LTXModelConfig] = None,
                   vae_decoder: Optional[LTX2VideoDecoder] = None, vae_encoder: Optional[VideoEncoder] = None,
                   upsampler=None, prompt_embeds: Optional[torch.Tensor] = None,
                   negative_prompt_embeds: Optional[torch.Tensor] = None, text_encoder: Optional[Callable] = None,
                   noise_fn: Optional[Callable] = None, device=None, on_frames_ready: Optional[Callable] = None,
                   return_latents: bool = False, lora_in_place: Optional[bool] = None,
                   hoist_context: bool = False, stg_scale: Optional[float] = None, stg_blocks: Optional[list] = None,
                   stg_mode: Optional[str] = None, enable_fp8: bool = False, fp8_scaling: str = "channel",
                   fp8_activations: bool = False, gemma_hidden_states=None, gemma_attention_mask: Optional[torch.Tensor] = None,
                   negative_gemma_hidden_states=None, negative_gemma_attention_mask: Optional[torch.Tensor] = None,
                   text_connector=None, guider: Optional[str] = None, apg_eta: float = 1.0,
                   apg_norm_threshold: float = 0.0, gemma=None, gemma_repo: Optional[str] = None,
                   tokenizer_path: Optional[str] = None, prompt_tokens=None, negative_prompt_tokens=None,
                   enhance_prompt: bool = False, max_tokens: int = 512, temperature: float = 0.7,
                   enhance_system_prompt: Optional[str] = None, audio_latents: Optional[torch.Tensor] = None,
                   audio_decoder=None, vocoder=None, output_audio: Optional[str] = None, audio_mode: str = "auto",
                   audio_model_repo: Optional[str] = None, audio_steps: int = 8, audio_transformer: Optional[LTXModel] = None,
                   audio_prompt_embeds: Optional[torch.Tensor] = None, av_transformer=None,
                   audio_negative_prompt_embeds: Optional[torch.Tensor] = None, fp8_text_encoder: bool = False,
                   enhance_device_loop: bool = False, enhance_mxfp4: bool = False,
                   step_cache_threshold: Optional[float] = None,
                   step_cache_coefficients: Optional[Sequence[float]] = None, enable_mxfp4: bool = False) -> np.ndarray:
    """See the module docstring.  Returns uint8 frames (F,H,W,3) (generate.py:4195-4197).
    ``hoist_context`` (not in the reference, off by default): the part of the forward that depends on the text context only -
    caption projection and the 48 cross-attention K / V^T projections, 3.37 TFLOP that the reference recomputes in every forward
    (ltx.py:77-89, attention.py:123-126) - is computed once per denoise call and reused by every step: the same kernels on the
    same inputs, hence the same latents bit for bit, 8-10 % less work per dev step at 512x512x33.
    ``stg_scale`` / ``stg_blocks`` / ``stg_mode`` (--stg-scale / --stg-blocks / --stg-mode; the reference parses and ignores
    them): spatio-temporal guidance in every guided (denoise_dev) stage - the dev pipeline, and stage 2 with ``stage2_dev``.
    A non-zero ``stg_scale`` on a run without a guided stage is a ValueError.  None / 0: off.
    ``enable_fp8`` (--enable-fp8; the reference parses and ignores it): every transformer this call builds keeps its Linear
    matrices as FP8 e4m3 panels, calculations still in bf16 (ltxk_gemm_w8) - half the weight bytes in memory and per forward.
    ``fp8_scaling``: "channel" (per-output-channel scale, amax -> 448) or "none" (the upstream plain cast).  LoRAs are merged in
    bf16 and the merged weights quantised (never merged into fp8 panels), so a LoRA-merged stage-2 transformer is a fresh fp8
    model.  A ``transformer=`` / ``stage2_transformer=`` passed in is used as it is.
    ``fp8_activations`` (--fp8-activations; needs ``enable_fp8``, a ValueError without it): the transformers this call builds also
    quantise the inputs of their in-block Linear layers to e4m3 per row and multiply fp8 x fp8 (ltxk_gemm_w8a8).
    ``enable_mxfp4`` (--enable-mxfp4; opt-in): every video transformer this call builds - the LoRA-merged stage-2 one
    included - keeps the matrices of its in-block Linear layers as OCP MXFP4 (4.25 bits per weight) and multiplies them with
    activations quantised to MXFP4 per row and 32 k, on the fp4 block-scaled MFMA (ltxk_gemm_mxfp4); everything else stays bf16.
    LoRAs are merged in bf16 and the result quantised, as for fp8.  Not together with ``enable_fp8`` / ``fp8_activations``, nor with
    ``audio_mode="joint"``: a ValueError.  A ``transformer=`` / ``stage2_transformer=`` passed in is used as it is.
    ``fp8_text_encoder`` (--fp8-text-encoder): the Gemma-3 encoder this call builds from ``gemma_repo`` keeps its projections and
    its embedding table as e4m3 panels (``GemmaEncoder(fp8=fp8_scaling)``) - half the resident bytes, and half the
    bytes a decoded token of ``enhance_prompt`` streams; the one encoder serves the text encode and the enhancement.  It needs
    ``gemma_repo``; with a passed ``gemma=`` that holds bf16 panels it is a ValueError (drop one of the two; an fp8 ``gemma=`` is
    taken as it is).  ``enable_fp8`` alone keeps meaning the transformer only.
    ``gemma_hidden_states`` / ``gemma_attention_mask`` (and the ``negative_`` pair): the text route that starts behind Gemma -
    the L hidden states of a Gemma-3 forward ((L,1,T,D) stack or list of L (1,T,D)) and its left-padded 0/1 mask (1,T); the
    feature extractor and the video embeddings connector run here (``text_connector=`` a ``TextConnector``, or loaded from
    ``model_repo``), positive and negative prompt as one B = 2 call.  ``prompt_embeds`` wins when both are given.
    ``gemma`` (a ``gemma.GemmaEncoder``) or ``gemma_repo`` (a local Gemma-3 directory, --gemma-repo / --text-encoder-repo; a
    ``text_encoder_repo`` that is an existing local directory counts as one): the text
    route that starts at the prompt - tokens -> GemmaEncoder -> ``text_connector`` -> context, positive and negative prompt as one
    B = 2 call.  Tokens are ``prompt_tokens`` / ``negative_prompt_tokens`` ((input_ids, attention_mask) pairs, left-padded), or made
    from ``prompt`` / ``negative_prompt`` with the tokenizer.json of ``tokenizer_path`` or ``gemma_repo`` (truncated and left-padded to
    1024; nothing is fetched).  ``prompt_embeds``, ``gemma_hidden_states`` and ``text_encoder`` keep their precedence over it, in that order.
    ``guider`` / ``apg_eta`` / ``apg_norm_threshold`` (--guider / --apg-eta / --apg-norm-threshold; not in the reference CLI, the
    guiders are ltx_core/components/guiders.py): what the CFG slot of every guided (denoise_dev) stage runs - "cfg" (None: the
    same), "cfg_star" or "apg" (DESIGN.md 5j).  A non-default guider on a run without a guided stage is a ValueError, as for STG.
    ``enhance_prompt`` / ``max_tokens`` / ``temperature`` (--enhance-prompt / --max-tokens / --temperature, the reference's names
    and defaults) and ``enhance_system_prompt`` (the system text; --enhance-system-prompt FILE; None: the package's default): the
    positive ``prompt`` is first rewritten by Gemma-3 itself (``gemma.enhance_prompt``: KV-cached decoding on the encoder's panels,
    sampled with ``seed``) and the rewritten string takes the text route above.  It needs ``gemma`` or ``gemma_repo``
    and a tokenizer.json (``tokenizer_path`` or ``gemma_repo``), a ValueError that names what is missing otherwise, and a prompt
    that the text route reads as a string (no ``prompt_tokens`` / ``prompt_embeds`` / ``gemma_hidden_states`` in its place).  Off, the
    default, nothing of it runs.
    ``enhance_device_loop`` (--enhance-device-loop; not in the reference CLI): the enhancement's token loop on the device - sampling
    by ``ops.sample_rows``, the decode step recorded once as a graph and replayed.  Off, the default, the host loop
    runs.  At ``temperature`` 0 both give the same prompt; above it the device loop consumes ``seed`` differently from the host
    loop's ``torch.multinomial``, so the same seed gives another rewrite.  A ValueError without ``enhance_prompt``.
    ``enhance_mxfp4`` (--enhance-mxfp4; not in the reference CLI; opt-in): the enhancement decodes on an OCP MXFP4 copy of the
    encoder's panels (``GemmaGenerator(decode_panels="mxfp4")``, ltxk_gemv_w4: 4.25 bits per weight streamed per token; DESIGN.md
    5r).  The rewrite is a 4-bit model's; the text encoding that conditions the DiT stays on the encoder's own bf16 / fp8 panels
    and is not affected.  It composes with ``fp8_text_encoder`` and ``enhance_device_loop``.  A ValueError without ``enhance_prompt``.
    ``audio_latents`` (--audio-latents FILE): finished audio latents (B, 8, T, 16) - the reference's own layout - decoded after the
    VAE decode under an ``audio_decode`` phase by ``audio_decoder`` / ``vocoder`` (``audio_vae.AudioDecoder`` / ``Vocoder``; loaded
    from ``model_repo`` when not given) into a stereo 24 kHz waveform.  It is written to ``output_audio`` (--output-audio PATH; by
    default the ``.wav`` beside ``output_path``) and, where ``output_path`` is a video file and an ffmpeg binary exists, muxed into
    it (generate.py:4049-4127).
    ``audio=True`` (--audio): SEPARATE audio generation (generate.py:3930-4047, the reference's ``audio_mode="separate"``): after the
    video an audio-only transformer (``audio_transformer=``, an ``LTXModel`` of ``LTXModelConfig.audio()``; else loaded from the
    ``audio_*`` tensors of ``audio_model_repo``'s or ``model_repo``'s checkpoint, ``weights.load_audio_transformer``) denoises
    (1, 8, T, 16) latents, T = ``compute_audio_frames(num_frames, fps)``, from noise seeded with ``seed`` alone, over
    ``_subsample_sigmas(STAGE_1_SIGMAS, audio_steps)`` (``audio_steps`` 1..8, --audio-steps) without CFG
    (``denoise.denoise_audio_only``), under an ``audio_generate`` phase; the latents then take the decode / ``.wav`` / mux path
    above.  Its context is ``audio_prompt_embeds`` (1,S,3840), or the audio embeddings connector's output where the text
    route runs the connector here.  ``audio_mode``: "auto" and "separate" are this.  With nothing to take an audio transformer
    from, ``audio=True`` raises as before; ``audio_latents`` given, they win and nothing is generated.  The audio transformer stays
    bf16 under ``enable_fp8``.
    ``audio_mode="joint"`` (--audio-mode joint; dev pipeline only): audio and video are denoised TOGETHER by the AudioVideo
    transformer, whose blocks exchange information through the a2v / v2a cross-modal attentions (``denoise.denoise_dev_av``,
    generate.py:1330-1680) - ``av_transformer=`` (an ``av_model.LTXAVModel``; its ``.video`` is the video transformer), else built
    from ``model_repo``'s joint checkpoint (``weights.load_av_transformer``).  The audio latents (1, 8, T, 16) come from ``seed`` as
    above; both modalities share the video schedule and CFG, each with its own context pair: ``audio_prompt_embeds`` /
    ``audio_negative_prompt_embeds`` (zeros when absent, like the video negative), or the audio connector's outputs for prompt and
    negative prompt where the text route runs here.  It runs under the ``dev_denoise`` phase (no ``audio_generate``), the
    profile reports ``audio_mode``, and the result takes the same decode / ``.wav`` / mux path.  The reference's "auto" picks joint
    for the dev pipeline; here joint is asked for by name.  Refused with it: every other pipeline and ``stage2_dev``, ``enable_fp8``
    / ``fp8_activations``, STG and the cfg_star / apg guiders, ``hoist_context``, and ``audio_transformer=``.
    ``step_cache_threshold`` / ``step_cache_coefficients`` (--step-cache-threshold X / --step-cache-coefficients C ...; not in the
    reference, off by default): a timestep-aware step cache (TeaCache, ``denoise.StepCache``) in every video denoise
    call - a step whose input to block 0 has moved little since the step before skips the 48 blocks and reuses the last
    computed step's residual.  The threshold is >= 0 (0 never skips; the latents are then today's, bit for bit); the
    coefficients are a polynomial applied to the relative distance, highest degree first - the default (1, 0) is the identity,
    NOT a calibrated fit, and no trained checkpoint has been run: which threshold gives which skip rate at which quality is
    open.  It implies ``hoist_context`` (same bits).  Each stage of a two-stage pipeline has a cache of its own; the profile
    JSON gains ``step_cache`` with the computed / skipped steps per denoise call.  Coefficients without a threshold, a negative
    or NaN threshold, and ``audio_mode="joint"`` with a step cache are ValueErrors."""
    t_start = time.perf_counter()
    if isinstance(pipeline, str):
        pipeline = PipelineType(pipeline)
    if audio_mode not in ("auto", "separate", "joint"):
        raise ValueError(f"Unknown audio_mode: {audio_mode!r} (expected 'auto', 'separate' or 'joint')")
    gen_audio = bool(audio) and audio_latents is None
    joint = gen_audio and audio_mode == "joint"         # "auto" stays separate: joint is asked for by name
    if joint:
        if audio_transformer is not None:
            raise ValueError("audio_mode='joint': audio_transformer= is the separate route's audio-only model and is not supported "
                             "with it; pass av_transformer= (an av_model.LTXAVModel) or a model_repo with the cross-modal tensors")
        if pipeline != PipelineType.DEV or stage2_dev:
            raise ValueError(f"audio_mode='joint' runs in the dev pipeline's denoise loop only, not in the {pipeline.value} pipeline"
                             f"{' with stage2_dev' if stage2_dev else ''} (the joint branch of the distilled loop and the audio "
                             "re-noising between stages are not implemented)")
        if enable_fp8 or fp8_activations or enable_mxfp4:
            raise ValueError("audio_mode='joint' runs on bf16 weights: enable_fp8 / fp8_activations / enable_mxfp4 are not supported with it")
        if float(stg_scale or 0.0) != 0.0 or (guider or "cfg") != "cfg" or hoist_context:
            raise ValueError("audio_mode='joint': the joint loop does plain CFG - no STG (stg_scale), no cfg_star / apg guider, no "
                             "hoist_context")
        if av_transformer is None and audio_model_repo is None and model_repo is None:
            raise ValueError("audio_mode='joint' is not supported without the joint transformer: pass av_transformer= (an "
                             "av_model.LTXAVModel) or model_repo= a local checkpoint directory with the cross-modal tensors")
        if transformer is None and av_transformer is not None:
            transformer = av_transformer.video
    elif gen_audio:
        if audio_transformer is None and audio_model_repo is None and model_repo is None:
            raise ValueError("audio generation is not supported without an audio transformer: pass audio_transformer= (an LTXModel of "
                             "LTXModelConfig.audio()), or audio_model_repo= / model_repo= a local checkpoint directory with the audio_* tensors")
        if audio_steps < 1 or audio_steps > (len(STAGE_1_SIGMAS) - 1):
            raise ValueError("--audio-steps must be between 1 and 8.")
    if step_cache_threshold is None and step_cache_coefficients is not None:
        raise ValueError("step_cache_coefficients (--step-cache-coefficients) shape the step cache's decision: they need "
                         "step_cache_threshold (--step-cache-threshold)")
    step_caches = []                  # one StepCache per video denoise call: each stage has a cache lifetime of its own
    if step_cache_threshold is not None:
        from .denoise import StepCache
        if joint:
            raise ValueError("audio_mode='joint': the joint loop does not take a step cache (step_cache_threshold)")
        if step_cache_coefficients is None:
            step_cache_coefficients = (1.0, 0.0)
        StepCache(step_cache_threshold, step_cache_coefficients)       # refuses a bad threshold or polynomial here

    def step_cache_kw() -> dict:
        """The keyword of one denoise call: nothing when the cache is off (today's call), else a fresh StepCache."""
        if step_cache_threshold is None:
            return {}
        step_caches.append(StepCache(step_cache_threshold, step_cache_coefficients))
        return {"step_cache": step_caches[-1]}

    if enhance_device_loop and not enhance_prompt:
        raise ValueError("enhance_device_loop (--enhance-device-loop) is a mode of enhance_prompt (--enhance-prompt), which is off")
    if enhance_mxfp4 and not enhance_prompt:
        raise ValueError("enhance_mxfp4 (--enhance-mxfp4) is a mode of enhance_prompt (--enhance-prompt), which is off")
    if enhance_prompt:
        _check_enhance(gemma, gemma_repo, text_encoder_repo, tokenizer_path, prompt_tokens, prompt_embeds, gemma_hidden_states, text_encoder)
    images_list = list(images or [])
    if image is not None:
        images_list.append((image, image_frame_idx, image_strength))
    video_conditionings = list(video_conditionings or [])
    if conditioning_mode not in ("replace", "guide"):
        raise ValueError(f"Unknown conditioning_mode: {conditioning_mode}")
    if pipeline == PipelineType.KEYFRAME:                         # generate.py:2223-2225
        conditioning_mode = "guide"
    if pipeline == PipelineType.IC_LORA:                          # generate.py:2226-2229
        if not video_conditionings:
            raise ValueError("IC-LoRA pipeline requires --video-conditioning PATH [FRAME_IDX] STRENGTH")
        conditioning_mode = "replace"
    is_distilled = pipeline in (PipelineType.DISTILLED, PipelineType.KEYFRAME, PipelineType.IC_LORA)
    if pipeline == PipelineType.DEV and video_conditionings:     # generate.py:2234-2235
        raise ValueError("Video conditioning is only supported in ic_lora/distilled pipelines.")
    if sigma_subsample not in ("uniform", "farthest"):
        raise ValueError(f"Unknown sigma subsample method: {sigma_subsample}")
    stg = {"stg_scale": float(stg_scale or 0.0), "stg_blocks": stg_blocks, "stg_mode": stg_mode or "stg_v"}
    if stg["stg_scale"] != 0.0 and is_distilled and not stage2_dev:
        raise ValueError(f"STG (stg_scale={stg_scale}) needs a guided denoise stage: the {pipeline.value} pipeline has none "
                         "without stage2_dev (--stage2-dev)")
    if stg["stg_mode"] not in ("stg_v", "stg_av"):
        raise ValueError(f"Unknown stg_mode: {stg_mode!r}")
    from .guidance import GuiderConfig
    gcfg = GuiderConfig(guider or "cfg", apg_eta, apg_norm_threshold)
    if not gcfg.is_default and is_distilled and not stage2_dev:
        raise ValueError(f"guider={gcfg.kind!r} needs a guided denoise stage: the {pipeline.value} pipeline has none "
                         "without stage2_dev (--stage2-dev)")
    if not gcfg.is_default:           # the default adds no keyword: today's calls
        stg.update(guider=gcfg.kind, apg_eta=gcfg.eta, apg_norm_threshold=gcfg.norm_threshold)
    from .weights import FP8_SCALINGS
    if fp8_scaling not in FP8_SCALINGS:
        raise ValueError(f"Unknown fp8_scaling: {fp8_scaling!r} (expected one of {FP8_SCALINGS})")
    if enable_mxfp4 and (enable_fp8 or fp8_activations):
        raise ValueError("enable_mxfp4 (--enable-mxfp4) and enable_fp8 / fp8_activations (--enable-fp8 / --fp8-activations) are two formats "
                         "of the same matrices: choose one")
    if fp8_activations and not enable_fp8:
        raise ValueError("fp8_activations (--fp8-activations) needs enable_fp8 (--enable-fp8): fp8 activations multiply fp8 weight panels")
    if fp8_text_encoder:
        if gemma is not None and gemma.weight_dtype == BF16:
            raise ValueError("fp8_text_encoder (--fp8-text-encoder) with a gemma= encoder that holds bf16 panels: drop fp8_text_encoder to "
                             "run that encoder, or drop gemma= and pass gemma_repo= to have an fp8 one built "
                             "(or build it yourself: GemmaEncoder(weights, config, fp8=...))")
        if gemma is None and gemma_repo is None and not (text_encoder_repo and Path(text_encoder_repo).is_dir()):
            raise ValueError("fp8_text_encoder (--fp8-text-encoder) needs a Gemma-3 model to build: gemma_repo= (a local Gemma-3 "
                             "directory, --gemma-repo)")
    gemma_fp8 = {"fp8": fp8_scaling} if fp8_text_encoder else {}          # (off adds no keyword: today's calls)

    def _build(cfg_, weights_) -> LTXModel:
        """A transformer from a module-key weight dict; under enable_fp8 from its quantised twin (an fp8 dict is kept as it is)."""
        if enable_fp8:
            from .weights import quantize_transformer_weights
            weights_ = quantize_transformer_weights(weights_, fp8_scaling)
        if enable_mxfp4:              # (an MXFP4 dict is kept as it is; the model recognises it)
            from .weights import quantize_transformer_weights_mxfp4
            return LTXModel(cfg_, quantize_transformer_weights_mxfp4(weights_))
        return LTXModel(cfg_, weights_, fp8_activations=fp8_activations)

    out_h, out_w = height, width
    height, width, crop = _pad_dims(height, width, 64 if is_distilled else 32)
    num_frames = _round_frames(num_frames)
    latent_frames = 1 + (num_frames - 1) // 8

    if is_distilled:                                               # generate.py:3054-3057
        if stage1_steps < 1 or stage1_steps > (len(STAGE_1_SIGMAS) - 1):
            raise ValueError("--stage1-steps must be between 1 and 8.")
        if stage2_steps not in (1, 2, 3):
            raise ValueError("--stage2-steps must be 1, 2, or 3.")
    if stage2_transformer is not None and distilled_loras:          # generate.py:3210-3211
        raise ValueError("--stage2-model-repo cannot be combined with --distilled-lora (stage-2 LoRA).")

    def _with_loras(lora_list, what: str) -> LTXModel:
        """generate.py:2957-3031 (_load_transformer_with_loras), merge mode: base weights + the listed LoRAs."""
        if transformer_weights is None:
            raise ValueError(f"{what} were given but the base transformer weights are not reachable: pass "
                             "transformer_weights= (the dict the transformer was built from) or a model_repo")
        from .lora import LoraSpec, apply_lora_to_weights
        merged = apply_lora_to_weights(transformer_weights, [LoraSpec(Path(pth), float(st)) for pth, st in lora_list], verbose=verbose)
        return _build(transformer_config or (transformer.config if transformer is not None else LTXModelConfig()), merged)

    # LoRAs may be merged INTO the model when nobody needs its un-merged weights again (`loras` alone: one merged model serves every
    # stage; `distilled_loras` alone: the stage-1 model is dead when stage 2 starts): by default only when the weights are loaded
    # here (this call owns them); a caller that passes its own model opts in explicitly
    if lora_in_place is None:
        lora_in_place = transformer is None and transformer_weights is None
    if (enable_fp8 or enable_mxfp4) and (transformer is None or transformer.weight_dtype != BF16):
        # fp8 panels take no in-place merge: merge-then-quantise builds the merged model afresh, and an fp8 replica is no
        # larger than what the in-place merge was saving
        lora_in_place = False
    if transformer is None and transformer_weights is None:
        if model_repo is None:
            raise FileNotFoundError("no transformer: pass transformer= or a local model_repo directory with LTX-2 safetensors")
        from .weights import load_pipeline_modules
        mods = load_pipeline_modules(model_repo, device or torch.device("cuda:0"), need_encoder=bool(images_list or video_conditionings),
                                     need_upsampler=is_distilled, build_transformer=False,
                                     # with LoRAs to merge the base dict stays bf16 (they are merged in bf16, then quantised)
                                     fp8=enable_fp8 and not (loras or distilled_loras), fp8_scaling=fp8_scaling,
                                     **({"mxfp4": True} if enable_mxfp4 and not (loras or distilled_loras) else {}))
        transformer_weights, transformer_config = mods["transformer_weights"], mods["transformer_config"]
        vae_decoder = vae_decoder or mods["vae_decoder"]
        vae_encoder, upsampler = vae_encoder or mods.get("vae_encoder"), upsampler or mods.get("upsampler")
    if loras:
        if lora_in_place and not distilled_loras:
            # nobody needs the un-merged weights again (stage 2 of a two-stage pipeline runs the same merged model): merge into the
            # model's own panels instead of building a second 21-GB copy (0.5 s of first-touch allocation, 17 GB of HBM)
            if transformer_weights is None:
                raise ValueError("loras were given but the base transformer weights are not reachable: pass transformer_weights= "
                                 "(the dict the transformer was built from) or a model_repo")
            from .lora import LoraSpec, apply_lora_to_weights
            if transformer is None:
                transformer = _build(transformer_config or LTXModelConfig(), transformer_weights)
            apply_lora_to_weights(transformer.weight_views(), [LoraSpec(Path(pth), float(st)) for pth, st in loras], verbose=verbose, in_place=True)
        else:
            transformer = _with_loras(loras, "loras")              # stage 1 / dev: base + loras
    elif transformer is None:
        transformer = _build(transformer_config or LTXModelConfig(), transformer_weights)
    if vae_decoder is None:
        raise FileNotFoundError("no VAE decoder: pass vae_decoder= or a model_repo containing VAE weights")
    dev = device or transformer.tables.device
    if joint and av_transformer is None:
        from .weights import load_av_transformer
        av_transformer = load_av_transformer(audio_model_repo or model_repo, dev, video=transformer)
    if noise_fn is None:
        noise_fn = _default_noise_fn(seed, dev)

    if prompt_embeds is None and gemma_hidden_states is not None:
        want = gen_audio and audio_prompt_embeds is None
        got = _connect_gemma(gemma_hidden_states, gemma_attention_mask, negative_gemma_hidden_states,
                             negative_gemma_attention_mask, text_connector, model_repo, dev, **({"want_audio": True} if want else {}))
        prompt_embeds, negative_prompt_embeds = got[0], got[1]
        if want:
            audio_prompt_embeds = got[2]
            if joint and audio_negative_prompt_embeds is None and len(got) > 3:
                audio_negative_prompt_embeds = got[3]
    if gemma_repo is None and text_encoder_repo and Path(text_encoder_repo).is_dir():
        gemma_repo = text_encoder_repo          # the reference's name for it; a repo NAME is not resolved (nothing is fetched)
    timer = _PhaseTimer(profile or bool(profile_json_path))
    if enhance_prompt:
        with timer.phase("prompt_enhance"):
            gemma, prompt = _enhance_prompt(gemma, gemma_repo, tokenizer_path, prompt, enhance_system_prompt, max_tokens, temperature,
                                            seed, dev, verbose, **({"device_loop": True} if enhance_device_loop else {}),
                                            **({"mxfp4": True} if enhance_mxfp4 else {}), **gemma_fp8)
    if prompt_embeds is None and text_encoder is None and (gemma is not None or gemma_repo is not None):
        hs, m = _encode_gemma(gemma, gemma_repo, tokenizer_path, prompt, negative_prompt, prompt_tokens, negative_prompt_tokens, dev,
                              **gemma_fp8)
        want = gen_audio and audio_prompt_embeds is None
        got = _connect_gemma(hs[:, 0:1], m[0:1], hs[:, 1:2], m[1:2], text_connector, model_repo, dev, **({"want_audio": True} if want else {}))
        prompt_embeds, negative_prompt_embeds = got[0], got[1]
        if want:
            audio_prompt_embeds = got[2]
            if joint and audio_negative_prompt_embeds is None and len(got) > 3:
                audio_negative_prompt_embeds = got[3]
    if prompt_embeds is None:
        if text_encoder is None:
            raise ValueError("prompt_embeds is required: pass prompt_embeds=(1,1024,3840) or text_encoder=callable, the hidden states "
                             "of a Gemma-3 forward as gemma_hidden_states= / gemma_attention_mask=, or run Gemma-3 here: gemma= (a "
                             "GemmaEncoder) or gemma_repo= (a local Gemma-3 directory, --gemma-repo) with prompt_tokens= / "
                             "negative_prompt_tokens= or a tokenizer.json (tokenizer_path=, --tokenizer)")
        prompt_embeds = text_encoder(prompt)
        negative_prompt_embeds = text_encoder(negative_prompt)
    if gen_audio and audio_prompt_embeds is None:
        raise ValueError("audio=True needs the audio context: pass audio_prompt_embeds= (1,S,3840), or take a text route that runs the "
                         "connector here (gemma_hidden_states= / gemma= / gemma_repo=) with the audio embeddings connector's weights")
    ctx_pos = prompt_embeds.to(dev).to(BF16)
    ctx_neg = (negative_prompt_embeds if negative_prompt_embeds is not None else torch.zeros_like(prompt_embeds)).to(dev).to(BF16)

    guide = conditioning_mode == "guide"

    def init_state(shape, conds, sigma0):
        """generate.py:3139-3160 / 3430-3449: zeros -> apply_conditioning -> masked noise blend."""
        st = LatentState(torch.zeros(shape, dtype=BF16, device=dev), torch.zeros(shape, dtype=BF16, device=dev),
                         torch.ones((1, 1, shape[2], 1, 1), dtype=BF16, device=dev))
        st = apply_conditioning(st, conds)
        return noise_blend(st, noise_fn(shape), float(sigma0))

    if is_distilled:
        if upsampler is None:
            raise FileNotFoundError("the two-stage pipelines need the latent upsampler (pass upsampler=)")
        s1h, s1w, s2h, s2w = height // 2 // 32, width // 2 // 32, height // 32, width // 32
        sig1 = _subsample_sigmas(list(STAGE_1_SIGMAS), stage1_steps, sigma_subsample)
        sig2 = _subsample_refinement_sigmas(list(STAGE_2_SIGMAS), stage2_steps, sigma_subsample)
        conds1, conds2 = [], []
        if images_list or video_conditionings:
            with timer.phase("cond_encode"):
                # every image is encoded twice, at the half- and the full-resolution stage, with the chosen mode;
                # a video conditioning (IC-LoRA) guides stage 1 only, always as keyframes (generate.py:3073-3110)
                conds1 = _encode_conditionings(images_list, vae_encoder, height // 2, width // 2, num_frames, latent_frames, guide, dev)
                conds2 = _encode_conditionings(images_list, vae_encoder, height, width, num_frames, latent_frames, guide, dev)
                conds1 += _encode_conditionings(video_conditionings, vae_encoder, height // 2, width // 2, num_frames, latent_frames,
                                                True, dev, is_video=True)
        shape1 = (1, 128, latent_frames, s1h, s1w)
        pos1 = create_position_grid(1, latent_frames, s1h, s1w, fps=fps).to(dev)
        state1 = init_state(shape1, conds1, sig1[0]) if conds1 else None
        latents = state1.latent if state1 is not None else noise_fn(shape1)
        with timer.phase("stage1_denoise"):
            latents, _ = denoise_distilled(latents, pos1, ctx_pos, transformer, sig1, state=state1,
                                           compile_step=compile_step, fp32_euler=fp32_euler, use_graph=compile_step, cache_context=hoist_context,
                                           **step_cache_kw())
        with timer.phase("upsample"):
            from .upsampler import upsample_latents
            latents = upsample_latents(latents, upsampler, vae_decoder.latents_mean, vae_decoder.latents_std)
        tr2 = stage2_transformer or transformer
        if distilled_loras:                                          # generate.py:3229-3237: base + distilled LoRAs only
            with timer.phase("stage2_transformer_load"):
                if lora_in_place and not loras:
                    # the stage-1 model IS the base model and is not used again: merge into its own panels (same EPI_SCALE_RES
                    # launches with the output aliasing the residual, same bits) instead of building a second 21-GB replica
                    from .lora import LoraSpec, apply_lora_to_weights
                    apply_lora_to_weights(transformer.weight_views(), [LoraSpec(Path(pth), float(st)) for pth, st in distilled_loras],
                                          verbose=verbose, in_place=True)
                    tr2 = transformer
                else:
                    tr2 = _with_loras(distilled_loras, "distilled_loras")
        pos2 = create_position_grid(1, latent_frames, s2h, s2w, fps=fps).to(dev)
        state2 = None
        if conds2:                                                  # generate.py:3290-3311
            st = LatentState(latents, torch.zeros_like(latents), torch.ones((1, 1, latent_frames, 1, 1), dtype=BF16, device=dev))
            state2 = noise_blend(apply_conditioning(st, conds2), noise_fn(tuple(latents.shape)), float(sig2[0]))
            latents = state2.latent
        else:                                                       # generate.py:3317-3321
            s0 = torch.tensor(sig2[0], dtype=BF16, device=dev)
            latents = (noise_fn(tuple(latents.shape)) * s0 + latents * torch.tensor(1.0 - sig2[0], dtype=BF16, device=dev)).to(BF16)
        with timer.phase("stage2_denoise"):
            if stage2_dev:
                latents = denoise_dev(latents, pos2, ctx_pos, ctx_neg, tr2, torch.tensor(sig2), cfg_scale=cfg_scale,
                                      state=state2, compile_step=compile_step, cfg_batch=cfg_batch, use_graph=compile_step, cache_context=hoist_context,
                                      **stg, **step_cache_kw())
            else:
                latents, _ = denoise_distilled(latents, pos2, ctx_pos, tr2, sig2, state=state2, compile_step=compile_step,
                                               fp32_euler=fp32_euler, use_graph=compile_step, cache_context=hoist_context,
                                               **step_cache_kw())
    else:
        lh, lw = height // 32, width // 32
        n_tok = latent_frames * lh * lw
        sigmas = ltx2_scheduler(num_inference_steps, n_tok)          # generate.py:3410-3411
        pos = create_position_grid(1, latent_frames, lh, lw, fps=fps).to(dev)
        shape = (1, 128, latent_frames, lh, lw)
        conds = []
        if images_list:
            with timer.phase("cond_encode"):
                conds = _encode_conditionings(images_list, vae_encoder, height, width, num_frames, latent_frames, guide, dev)
        state = init_state(shape, conds, float(sigmas[0])) if conds else None
        latents = state.latent if state is not None else noise_fn(shape)
        if joint:                                                    # audio and video together: generate.py:1330-1680
            from .denoise import denoise_dev_av
            from .schedulers import AUDIO_LATENT_CHANNELS, AUDIO_MEL_BINS, compute_audio_frames, create_audio_position_grid
            if av_transformer.video is not transformer:
                raise ValueError("audio_mode='joint': transformer= must be av_transformer.video (or left out)")
            audio_frames = compute_audio_frames(num_frames, fps)
            # seeded from `seed` alone, as the separate route draws them
            a_noise = _default_noise_fn(seed, dev)((1, AUDIO_LATENT_CHANNELS, audio_frames, AUDIO_MEL_BINS))
            a_pos = audio_prompt_embeds.to(dev).to(BF16)
            a_neg = (audio_negative_prompt_embeds if audio_negative_prompt_embeds is not None else torch.zeros_like(a_pos)).to(dev).to(BF16)
            with timer.phase("dev_denoise"):
                latents, audio_latents = denoise_dev_av(latents, a_noise, pos, create_audio_position_grid(1, audio_frames).to(dev),
                                                        ctx_pos, ctx_neg, a_pos, a_neg, av_transformer, sigmas, cfg_scale=cfg_scale,
                                                        video_state=state, compile_step=compile_step, cfg_batch=cfg_batch,
                                                        use_graph=compile_step)
            gen_audio = False                                        # the latents exist: the separate pass below has nothing to do
        else:
            with timer.phase("dev_denoise"):
                latents = denoise_dev(latents, pos, ctx_pos, ctx_neg, transformer, sigmas, cfg_scale=cfg_scale, state=state,
                                      compile_step=compile_step, cfg_batch=cfg_batch, use_graph=compile_step,
                                      cache_context=hoist_context, **stg, **step_cache_kw())

    if return_latents:
        return latents
    # ---- VAE decode (generate.py:3794-3830) ----
    tcfg = None
    if tiling == "auto":
        tcfg = TilingConfig.auto(height, width, num_frames)
    elif tiling not in ("none", None):
        tcfg = {"default": TilingConfig.default, "aggressive": TilingConfig.aggressive,
                "conservative": TilingConfig.conservative, "spatial": TilingConfig.spatial_only,
                "temporal": TilingConfig.temporal_only}[tiling]()
    # a timestep-conditioned decoder draws fresh noise per decode call, i.e. per tile (decoder.py:381-385)
    dec_noise_fn = noise_fn if vae_decoder.timestep_conditioning else None
    with timer.phase("vae_decode"):
        if tcfg is not None and (tiling != "auto" or stream):
            video = vae_decoder.decode_tiled(latents, tiling_config=tcfg, tiling_mode=tiling, on_frames_ready=on_frames_ready,
                                             noise_fn=dec_noise_fn)
        else:
            # "auto": the reference first tries the non-tiled decode and only falls back on an OOM-looking
            # exception (generate.py:3798-3818); 288 GB of HBM never takes that fallback at these sizes.
            video = vae_decoder(latents, noise_fn=dec_noise_fn)
    with timer.phase("to_uint8_numpy"):
        frames = to_uint8_frames(video)[0]
        video_np = frames.cpu().numpy()
        if crop is not None:
            top, left, oh, ow = crop
            video_np = video_np[:, top:top + oh, left:left + ow, :]
    waveform = None
    if gen_audio:                                                      # generate.py:3930-4047
        from .denoise import denoise_audio_only
        from .schedulers import AUDIO_LATENT_CHANNELS, AUDIO_MEL_BINS, compute_audio_frames, create_audio_position_grid
        with timer.phase("audio_generate"):
            if audio_transformer is None:
                from .weights import load_audio_transformer
                audio_transformer = load_audio_transformer(audio_model_repo or model_repo, dev)
            audio_frames = compute_audio_frames(num_frames, fps)
            # seeded from `seed` alone: the audio does not depend on how much noise the video stages drew (generate.py:4025-4028)
            a_noise = _default_noise_fn(seed, dev)((1, AUDIO_LATENT_CHANNELS, audio_frames, AUDIO_MEL_BINS))
            a_sig = _subsample_sigmas(list(STAGE_1_SIGMAS), audio_steps, sigma_subsample)
            audio_latents = denoise_audio_only(a_noise, create_audio_position_grid(1, audio_frames).to(dev),
                                               audio_prompt_embeds.to(dev).to(BF16), audio_transformer, a_sig,
                                               fp32_euler=fp32_euler, cache_context=hoist_context)
    if audio_latents is not None:                                     # generate.py:4049-4127
        from .audio_vae import decode_audio
        if audio_decoder is None or vocoder is None:
            from .weights import load_audio_decoder, load_vocoder
            audio_decoder = audio_decoder or load_audio_decoder(model_repo, dev)
            vocoder = vocoder or load_vocoder(model_repo, dev)
        with timer.phase("audio_decode"):
            waveform = decode_audio(audio_latents.to(dev), audio_decoder, vocoder)
            waveform = (waveform[0] if waveform.dim() == 3 else waveform).cpu()
    elapsed = time.perf_counter() - t_start
    if output_path:
        p = Path(output_path)
        p.parent.mkdir(parents=True, exist_ok=True)
        if p.suffix == ".npy":
            np.save(p, video_np)
        else:                                                          # generate.py:3900-3913 (ffmpeg encoder)
            from .media import write_video_ffmpeg
            write_video_ffmpeg(video_np, p, fps)
    if waveform is not None and (output_audio or output_path):
        from .media import mux_video_audio, save_audio
        wav_path = Path(output_audio) if output_audio else Path(output_path).with_suffix(".wav")
        wav_path.parent.mkdir(parents=True, exist_ok=True)
        save_audio(waveform, wav_path, vocoder.output_sample_rate)
        if output_path and Path(output_path).suffix != ".npy":
            vp = Path(output_path)
            tmp = vp.with_name(vp.stem + ".video_only" + vp.suffix)
            vp.replace(tmp)
            if mux_video_audio(tmp, wav_path, vp, audio_sample_rate=vocoder.output_sample_rate):
                tmp.unlink()
            else:
                tmp.replace(vp)                                        # no ffmpeg: the silent video and the sidecar stay
    if profile and verbose:
        print(timer.render(elapsed))
    if profile_json_path and timer.times_s:                          # generate.py:4158-4189 (same keys)
        outp = Path(output_path).with_suffix(".profile.json") if profile_json_path == "auto" and output_path else Path(profile_json_path)
        payload = {"elapsed_s": float(elapsed), "num_frames": int(num_frames), "fps": float(fps), "pipeline": pipeline.value,
                   "stage1_steps": int(stage1_steps) if is_distilled else None,
                   "stage2_steps": int(stage2_steps) if is_distilled else None, "eval_interval": int(eval_interval),
                   "compile_step": bool(compile_step), "compile_shapeless": bool(compile_shapeless),
                   "fp32_euler": bool(fp32_euler), "audio": waveform is not None,
                   **({"audio_mode": "joint" if joint else "separate"} if audio else {}), "phases_s": {k: float(v) for k, v in timer.times_s.items()},
                   "peak_memory_gb": float(torch.cuda.max_memory_allocated() / (1024 ** 3))}
        if enable_mxfp4:              # off: today's keys
            payload["weight_format"] = "mxfp4"
        if step_caches:               # off: today's keys
            payload["step_cache"] = {"threshold": step_caches[0].threshold, "coefficients": list(step_caches[0].coefficients),
                                     "calls": [c.counts for c in step_caches]}
        outp.parent.mkdir(parents=True, exist_ok=True)
        outp.write_text(json.dumps(payload, indent=2, sort_keys=True), encoding="utf-8")
    return video_np


class _ImageConditionAction(argparse.Action):
    """generate.py:4201-4215: --image PATH [FRAME_IDX STRENGTH], repeatable."""

    def __call__(self, parser, namespace, values, option_string=None):
        if len(values) not in (1, 3):
            raise argparse.ArgumentError(self, f"{option_string} accepts 1 or 3 args (PATH [FRAME_IDX STRENGTH]), got {len(values)}")
        item = (values[0], int(values[1]), float(values[2])) if len(values) == 3 else (values[0], None, None)
        setattr(namespace, self.dest, (getattr(namespace, self.dest) or []) + [item])


class _VideoConditionAction(argparse.Action):
    """generate.py:4217-4231: --video-conditioning PATH STRENGTH | PATH FRAME_IDX STRENGTH, repeatable."""

    def __call__(self, parser, namespace, values, option_string=None):
        if len(values) not in (2, 3):
            raise argparse.ArgumentError(self, f"{option_string} accepts PATH STRENGTH or PATH FRAME_IDX STRENGTH")
        item = (values[0], 0, float(values[1])) if len(values) == 2 else (values[0], int(values[1]), float(values[2]))
        setattr(namespace, self.dest, (getattr(namespace, self.dest) or []) + [item])


class _LoraAction(argparse.Action):
    """generate.py:4233-4242: --lora PATH [STRENGTH], repeatable."""

    def __call__(self, parser, namespace, values, option_string=None):
        if len(values) not in (1, 2):
            raise argparse.ArgumentError(self, f"{option_string} accepts PATH or PATH STRENGTH, got {len(values)}")
        item = (values[0], float(values[1]) if len(values) == 2 else 1.0)
        setattr(namespace, self.dest, (getattr(namespace, self.dest) or []) + [item])


def _finite_float(text: str) -> float:
    v = float(text)
    if not math.isfinite(v):
        raise argparse.ArgumentTypeError(f"expected a finite number, got {text!r}")
    return v


def _step_cache_threshold(text: str) -> float:
    v = float(text)
    if not v >= 0:                        # inf is a threshold (skip all but the ends); NaN and negatives are not
        raise argparse.ArgumentTypeError(f"expected a threshold >= 0, got {text!r}")
    return v


def _nonneg_float(text: str) -> float:
    v = _finite_float(text)
    if v < 0:
        raise argparse.ArgumentTypeError(f"expected a number >= 0, got {text!r}")
    return v


def build_parser() -> argparse.ArgumentParser:
    """The subset of generate.py:4244-4525 that drives this path."""
    ap = argparse.ArgumentParser(description="LTX-2 video generation on MI355X (libltxk)")
    ap.add_argument("--image", "-i", action=_ImageConditionAction, nargs="+", metavar="PATH", default=[],
                    help="Image conditioning: --image path.jpg or --image path.jpg FRAME_IDX STRENGTH (repeatable)")
    ap.add_argument("--condition-image", type=str, default=None, help="Alias for --image (frame 0, strength 1.0)")
    ap.add_argument("--image-strength", type=float, default=1.0)
    ap.add_argument("--image-frame-idx", type=int, default=0)
    ap.add_argument("--video-conditioning", action=_VideoConditionAction, nargs="+", metavar="ARG", default=[],
                    help="Video conditioning for IC-LoRA: PATH [FRAME_IDX] STRENGTH (a directory of frames or an .npy array here)")
    ap.add_argument("--reference-video", type=str, default=None, help="Alias for --video-conditioning (frame 0, strength 1.0)")
    ap.add_argument("--lora", "--lora-path", dest="lora", action=_LoraAction, nargs="+", metavar="ARG", default=[],
                    help="LoRA weights to merge (repeatable): --lora path 0.8")
    ap.add_argument("--distilled-lora", action=_LoraAction, nargs="+", metavar="ARG", default=[],
                    help="LoRA(s) for stage-2 refinement (distilled pipelines only)")
    ap.add_argument("--conditioning-mode", choices=["replace", "guide"], default="replace")
    ap.add_argument("--stream", action="store_true", help="Decode tiled and hand frames over as they are finished")
    ap.add_argument("--stage2-dev", action="store_true")
    ap.add_argument("--no-fp32-euler", dest="fp32_euler", action="store_false",
                    default=__import__("os").getenv("LTX_FP32_EULER", "").lower() not in ("0", "false", "no"))
    ap.add_argument("--prompt", type=str, default="")
    ap.add_argument("--negative-prompt", type=str, default=DEFAULT_NEGATIVE_PROMPT)
    ap.add_argument("--pipeline", choices=[p.value for p in PipelineType], default="distilled")
    ap.add_argument("--model-repo", type=str, default=None)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--num-frames", type=int, default=33)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--cfg-scale", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--fps", type=float, default=24.0)
    ap.add_argument("--output-path", type=str, default="output.npy")
    ap.add_argument("--audio-latents", type=str, default=None, metavar="FILE",
                    help="Finished audio latents (B,8,T,16) as .npy or a torch file: decoded to a 24 kHz stereo waveform after the VAE decode")
    ap.add_argument("--output-audio", type=str, default=None, metavar="PATH",
                    help="Where the decoded waveform goes (.wav); default: beside --output-path")
    ap.add_argument("--audio", action="store_true", default=False,
                    help="Generate audio separately after the video (an audio-only transformer pass over the checkpoint's audio_* "
                         "weights), decode it to a 24 kHz stereo waveform and mux it")
    ap.add_argument("--audio-mode", choices=["auto", "separate", "joint"], default="auto",
                    help="auto = separate (audio-only transformer pass after the video); joint = audio and video denoised together "
                         "through the cross-modal attentions (dev pipeline, a checkpoint with the cross-modal tensors)")
    ap.add_argument("--audio-model-repo", type=str, default=None, metavar="DIR",
                    help="Local checkpoint directory the audio transformer is read from (default: --model-repo)")
    ap.add_argument("--audio-steps", type=int, default=8, help="Denoise steps of the separate audio pass (1..8)")
    ap.add_argument("--audio-prompt-embeds", type=str, default=None, metavar="FILE",
                    help="The audio context (1,S,3840) as .npy or a torch file, where the text route does not run the connector here")
    ap.add_argument("--tiling", type=str, default="auto")
    ap.add_argument("--stage1-steps", type=int, default=None)
    ap.add_argument("--stage2-steps", type=int, default=None)
    ap.add_argument("--sigma-subsample", choices=["uniform", "farthest"], default=__import__("os").getenv("LTX_SIGMA_SUBSAMPLE", "farthest"))
    ap.add_argument("--eval-interval", type=int, default=None, help="Host sync cadence of the denoise loop (default: auto)")
    ap.add_argument("--compile", dest="compile_step", action="store_true", default=False,
                    help="Captured step (the reference's mx.compile'd step: bf16-rounded sigmas in x0 and Euler)")
    ap.add_argument("--no-compile", action="store_true", help="Disable the compiled step even if LTX_COMPILE enables it")
    ap.add_argument("--cfg-batch", action="store_true", default=False, help="CFG pair as one B=2 forward")
    ap.add_argument("--no-cfg-batch", action="store_true", help="Two sequential forwards even if LTX_CFG_BATCH enables batching")
    ap.add_argument("--hoist-context", action="store_true",
                    help="(not in the reference CLI) compute the text-only part of the forward once per denoise call instead of in every step; same latents")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-json", type=str, default=None)
    ap.add_argument("--prompt-embeds", type=str, default=None, help=".pt/.npy file with (1,1024,3840) text embeddings")
    ap.add_argument("--negative-prompt-embeds", type=str, default=None)
    ap.add_argument("--gemma-hidden-states", type=str, default=None,
                    help="(not in the reference CLI) .pt/.safetensors file with `hidden_states` (L,T,D) or (L,1,T,D) - the hidden states of a "
                         "Gemma-3 forward - and `attention_mask` (T), left-padded; the feature extractor and the connector of --model-repo run here")
    ap.add_argument("--negative-gemma-hidden-states", type=str, default=None, help="the same for the negative prompt")
    ap.add_argument("--gemma-repo", "--text-encoder-repo", dest="gemma_repo", type=str, default=None,
                    help="local Gemma-3 directory (config.json + safetensors, optionally tokenizer.json): the text encoder runs here; "
                         "--text-encoder-repo is the reference's spelling")
    ap.add_argument("--tokenizer", type=str, default=None, help="(not in the reference CLI) local directory with a tokenizer.json (default: --gemma-repo)")
    ap.add_argument("--prompt-tokens", type=str, default=None,
                    help="(not in the reference CLI) .npz with `input_ids` and `attention_mask`, left-padded: the tokenised --prompt")
    ap.add_argument("--negative-prompt-tokens", type=str, default=None, help="the same for the negative prompt")
    ap.add_argument("--enhance-prompt", action="store_true", help="Enhance the prompt using Gemma (needs --gemma-repo and a tokenizer.json)")
    ap.add_argument("--max-tokens", type=int, default=512, help="Max tokens for prompt enhancement")
    ap.add_argument("--temperature", type=float, default=0.7, help="Temperature for prompt enhancement")
    ap.add_argument("--enhance-device-loop", action="store_true",
                    help="(not in the reference CLI) run --enhance-prompt's token loop on the device: sampling in a HIP kernel, the decode "
                         "step replayed as one graph; at --temperature > 0 the same --seed gives other tokens than the host loop")
    ap.add_argument("--enhance-mxfp4", action="store_true",
                    help="(not in the reference CLI) decode --enhance-prompt on 4-bit (OCP MXFP4) panels built from the Gemma weights: "
                         "opt-in, about half the bytes per token of --fp8-text-encoder; the text encoding is unaffected")
    ap.add_argument("--enhance-system-prompt", type=str, default=None, metavar="FILE",
                    help="(not in the reference CLI) text file with the system prompt of --enhance-prompt (default: the package's own)")
    ap.add_argument("--synthetic", action="store_true", help="random-init weights + random text embeddings (no checkpoints offline)")
    ap.add_argument("--layers", type=int, default=48)
    # spatio-temporal guidance (the reference's spellings and defaults; it ignores them, this port runs them)
    ap.add_argument("--stg-scale", type=float, default=None, help="STG scale (0 / unset: off); dev pipeline or --stage2-dev")
    ap.add_argument("--stg-blocks", type=int, nargs="*", default=None, help="Blocks whose video self-attention the STG pass skips (default: all)")
    ap.add_argument("--stg-mode", type=str, choices=["stg_av", "stg_v"], default=None,
                    help="stg_av acts as stg_v: the model has no audio branch")
    # the guider of the CFG slot (not in the reference CLI; ltx_core/components/guiders.py)
    ap.add_argument("--guider", type=str, choices=["cfg", "cfg_star", "apg"], default="cfg",
                    help="cfg: classifier-free guidance; cfg_star: CFG with the negative prediction projected onto the positive one; "
                         "apg: adaptive projected guidance.  dev pipeline or --stage2-dev")
    ap.add_argument("--apg-eta", type=_finite_float, default=1.0, help="--guider apg: weight of the guidance component parallel to the prediction")
    ap.add_argument("--apg-norm-threshold", type=_nonneg_float, default=0.0, help="--guider apg: clamp the guidance norm to this (0: off)")
    # timestep-aware step cache (not in the reference; denoise.StepCache)
    ap.add_argument("--step-cache-threshold", type=_step_cache_threshold, default=None, metavar="X",
                    help="(not in the reference CLI) skip the transformer blocks of a step while the accumulated relative change of "
                         "block 0's input stays below X >= 0 (0: never skip; inf: every step but the first and last); unset: off")
    ap.add_argument("--step-cache-coefficients", type=_finite_float, nargs="+", default=None, metavar="C",
                    help="polynomial applied to the relative change before it is accumulated, highest degree first "
                         "(default 1 0: the identity, not a calibrated fit); needs --step-cache-threshold")
    # the reference's flag (it parses and ignores it): keep the model in lower precision, calculations still in bfloat16
    ap.add_argument("--enable-fp8", action="store_true", default=False,
                    help="Keep the transformer's Linear weights as FP8 (e4m3) panels; calculations still in bfloat16")
    ap.add_argument("--fp8-scaling", type=str, choices=["channel", "none"], default="channel",
                    help="(not in the reference CLI) channel: per-output-channel scale; none: the plain cast")
    ap.add_argument("--fp8-activations", action="store_true", default=False,
                    help="(not in the reference CLI; needs --enable-fp8) quantise the in-block Linear inputs to FP8 per row and "
                         "multiply on the fp8 matrix pipe")
    ap.add_argument("--enable-mxfp4", action="store_true", default=False,
                    help="(not in the reference CLI; opt-in) keep the in-block Linear matrices of the video transformer as OCP MXFP4 and "
                         "multiply them with MXFP4-quantised activations on the fp4 block-scaled MFMA; not with --enable-fp8")
    ap.add_argument("--fp8-text-encoder", action="store_true", default=False,
                    help="(not in the reference CLI; needs --gemma-repo) keep Gemma-3's projections and embedding table as FP8 (e4m3) "
                         "panels, scaled as --fp8-scaling says: the text encode and --enhance-prompt run on them")
    return ap


def resolve_cli_heuristics(args, env=None):
    """The auto rules of generate.py:4545-4560 and 4629-4644 that pick the hot path's flavour: step counts, the host sync
    cadence, compiled-vs-eager step (they differ in the sigma the Euler update sees, generate.py:1170-1174 vs 1293-1301)
    and batched-vs-sequential CFG.  Pure function of the parsed args and the environment (LTX_COMPILE, LTX_CFG_BATCH,
    LTX_EVAL_INTERVAL); mutates and returns ``args``."""
    env = __import__("os").environ if env is None else env
    truthy = lambda name: str(env.get(name, "")).lower() in ("1", "true", "yes")
    is_dev = args.pipeline == "dev"
    if args.stage1_steps is None:
        args.stage1_steps = 5 if args.pipeline == "distilled" else 8
    if args.stage2_steps is None:
        args.stage2_steps = 1 if args.pipeline == "distilled" else 3
    if args.eval_interval is None:
        ev = env.get("LTX_EVAL_INTERVAL")
        args.eval_interval = int(ev) if ev is not None else (2 if is_dev else 4)
    if args.eval_interval < 1:
        args.eval_interval = 1
    repo_l = str(getattr(args, "model_repo", None) or "").lower()
    is_quant_repo = any(tag in repo_l for tag in ("4bit", "8bit", "q4", "q8", "int4", "int8"))
    if getattr(args, "no_compile", False):
        args.compile_step = False
    elif truthy("LTX_COMPILE"):
        args.compile_step = True
    elif not args.compile_step:
        if is_dev and args.steps >= 8:
            args.compile_step = True
        elif (not is_dev) and args.num_frames >= 97 and (args.stage1_steps + args.stage2_steps) >= 5:
            args.compile_step = True
    if getattr(args, "no_cfg_batch", False):
        args.cfg_batch = False
    elif truthy("LTX_CFG_BATCH"):
        args.cfg_batch = True
    elif not args.cfg_batch and is_dev and args.cfg_scale > 1.0 and not is_quant_repo:
        args.cfg_batch = True
    return args


def load_gemma_hidden_states(path: str):
    """--gemma-hidden-states FILE: a .pt (torch.save of a dict, read with weights_only=True) or .safetensors file with
    `hidden_states` (L,T,D) or (L,1,T,D) and `attention_mask` (T) or (1,T) -> ((L,1,T,D), (1,T))."""
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        d = load_file(str(path))
    else:
        d = torch.load(path, weights_only=True)
    if not isinstance(d, dict) or "hidden_states" not in d or "attention_mask" not in d:
        raise ValueError(f"{path}: expected `hidden_states` and `attention_mask` tensors")
    hs, mask = d["hidden_states"], d["attention_mask"]
    if hs.dim() == 3:
        hs = hs[:, None]
    if hs.dim() != 4 or hs.shape[1] != 1:
        raise ValueError(f"{path}: hidden_states must be (L,T,D) or (L,1,T,D), got {tuple(hs.shape)}")
    mask = mask.reshape(1, -1)
    if mask.shape[1] != hs.shape[2]:
        raise ValueError(f"{path}: attention_mask has {mask.shape[1]} positions, hidden_states {hs.shape[2]}")
    return hs, mask


def load_prompt_tokens(path: str):
    """--prompt-tokens FILE: an .npz with `input_ids` and `attention_mask` ((T,) or (1,T)) -> ((1,T), (1,T)) int64 tensors."""
    with np.load(path) as d:
        if "input_ids" not in d or "attention_mask" not in d:
            raise ValueError(f"{path}: expected `input_ids` and `attention_mask` arrays")
        return _as_tokens((d["input_ids"].astype(np.int64), d["attention_mask"].astype(np.int64)), path)


def main(argv: Optional[Sequence[str]] = None) -> None:
    args = resolve_cli_heuristics(build_parser().parse_args(argv))
    if args.enable_mxfp4 and (args.enable_fp8 or args.fp8_activations):
        raise ValueError("--enable-mxfp4 and --enable-fp8 / --fp8-activations are two formats of the same matrices: choose one")
    if args.fp8_activations and not args.enable_fp8:
        raise ValueError("--fp8-activations needs --enable-fp8: fp8 activations multiply fp8 weight panels")
    if args.fp8_text_encoder and not args.gemma_repo:
        raise ValueError("--fp8-text-encoder needs --gemma-repo: it is the Gemma-3 model built from that directory that keeps fp8 panels")
    if args.enhance_mxfp4 and not args.enhance_prompt:
        raise ValueError("--enhance-mxfp4 is a mode of --enhance-prompt, which is off")
    if args.step_cache_coefficients is not None and args.step_cache_threshold is None:
        raise ValueError("--step-cache-coefficients needs --step-cache-threshold")
    is_dev = args.pipeline == "dev"
    dev = torch.device("cuda:0")
    kw = {}
    if args.step_cache_threshold is not None:
        kw.update(step_cache_threshold=args.step_cache_threshold, step_cache_coefficients=args.step_cache_coefficients)
    # generate.py:4667-4694: --image items without an explicit index/strength take --image-frame-idx / --image-strength
    images = [(pth, args.image_frame_idx if fi is None else fi, args.image_strength if st is None else st) for pth, fi, st in args.image]
    if args.condition_image:
        images.append((args.condition_image, 0, 1.0))
    videos = list(args.video_conditioning)
    if args.reference_video:
        videos.append((args.reference_video, 0, 1.0))
    if args.synthetic:
        from .video_vae import random_decoder_weights
        if args.enable_fp8 or args.enable_mxfp4:       # the weight dict instead of the model: generate_video quantises what it builds
            kw["transformer_config"] = LTXModelConfig(num_layers=args.layers)
            kw["transformer_weights"] = LTXModel.random_weights(kw["transformer_config"], dev)
        else:
            kw["transformer"] = LTXModel.random_init(LTXModelConfig(num_layers=args.layers), dev)
        kw["vae_decoder"] = LTX2VideoDecoder(random_decoder_weights(dev))
        g = torch.Generator(device=dev).manual_seed(43)
        if args.gemma_repo:       # the text route runs for real; only the connector's weights are random (Gemma width, its L + 1 states)
            from .gemma import GemmaConfig
            from .text_connector import TextConnector, random_connector_weights
            gc = GemmaConfig.from_json(args.gemma_repo)
            kw["text_connector"] = TextConnector(random_connector_weights(dev, D=gc.hidden_size, L=gc.num_hidden_layers + 1, layers=1,
                                                                          generator_device=dev))
        else:
            kw["prompt_embeds"] = torch.randn((1, 1024, 3840), generator=g, device=dev).to(BF16)
            kw["negative_prompt_embeds"] = torch.randn((1, 1024, 3840), generator=g, device=dev).to(BF16)
        if not is_dev:
            from .upsampler import LatentUpsampler
            from .weights import random_upsampler_weights
            kw["upsampler"] = LatentUpsampler(random_upsampler_weights(dev))
        if images or videos:
            from .video_vae import random_encoder_weights
            kw["vae_encoder"] = VideoEncoder(random_encoder_weights(dev))
    else:
        def _load(path):
            return torch.from_numpy(np.load(path)) if path.endswith(".npy") else torch.load(path, weights_only=True)
        if args.prompt_embeds:
            kw["prompt_embeds"] = _load(args.prompt_embeds)
        if args.negative_prompt_embeds:
            kw["negative_prompt_embeds"] = _load(args.negative_prompt_embeds)
        if args.gemma_hidden_states:
            kw["gemma_hidden_states"], kw["gemma_attention_mask"] = load_gemma_hidden_states(args.gemma_hidden_states)
        if args.negative_gemma_hidden_states:
            kw["negative_gemma_hidden_states"], kw["negative_gemma_attention_mask"] = load_gemma_hidden_states(args.negative_gemma_hidden_states)
    if args.audio_latents:
        kw["audio_latents"] = torch.from_numpy(np.load(args.audio_latents)) if args.audio_latents.endswith(".npy") else \
            torch.load(args.audio_latents, weights_only=True)
        kw["output_audio"] = args.output_audio
    elif args.audio:
        kw["output_audio"] = args.output_audio
    elif args.output_audio:
        raise ValueError("--output-audio needs --audio-latents (finished latents) or --audio (generate them)")
    if args.audio:
        kw.update(audio=True, audio_mode=args.audio_mode, audio_model_repo=args.audio_model_repo, audio_steps=args.audio_steps)
        if args.audio_prompt_embeds:
            f = args.audio_prompt_embeds
            kw["audio_prompt_embeds"] = torch.from_numpy(np.load(f)) if f.endswith(".npy") else torch.load(f, weights_only=True)
    if args.gemma_repo:
        kw["gemma_repo"], kw["tokenizer_path"] = args.gemma_repo, args.tokenizer
    if args.prompt_tokens:
        kw["prompt_tokens"] = load_prompt_tokens(args.prompt_tokens)
    if args.negative_prompt_tokens:
        kw["negative_prompt_tokens"] = load_prompt_tokens(args.negative_prompt_tokens)
    if args.enhance_prompt:
        kw.update(enhance_prompt=True, max_tokens=args.max_tokens, temperature=args.temperature)
        if args.enhance_device_loop:
            kw["enhance_device_loop"] = True
        if args.enhance_mxfp4:
            kw["enhance_mxfp4"] = True
        if args.enhance_system_prompt:
            kw["enhance_system_prompt"] = Path(args.enhance_system_prompt).read_text(encoding="utf-8")
    generate_video(model_repo=args.model_repo, prompt=args.prompt, pipeline=PipelineType(args.pipeline),
                   negative_prompt=args.negative_prompt, height=args.height, width=args.width, num_frames=args.num_frames,
                   num_inference_steps=args.steps, cfg_scale=args.cfg_scale, seed=args.seed, fps=args.fps,
                   output_path=args.output_path, tiling=args.tiling, compile_step=args.compile_step, cfg_batch=args.cfg_batch, hoist_context=args.hoist_context,
                   eval_interval=args.eval_interval,
                   profile=args.profile, profile_json_path=args.profile_json, stage1_steps=args.stage1_steps,
                   stage2_steps=args.stage2_steps, sigma_subsample=args.sigma_subsample, verbose=True, device=dev,
                   images=images, video_conditionings=videos, loras=args.lora, distilled_loras=args.distilled_lora,
                   conditioning_mode=args.conditioning_mode, stream=args.stream, stage2_dev=args.stage2_dev,
                   fp32_euler=args.fp32_euler, stg_scale=args.stg_scale, stg_blocks=args.stg_blocks, stg_mode=args.stg_mode,
                   enable_fp8=args.enable_fp8, fp8_scaling=args.fp8_scaling, fp8_activations=args.fp8_activations,
                   guider=args.guider, apg_eta=args.apg_eta, apg_norm_threshold=args.apg_norm_threshold,
                   **({"fp8_text_encoder": True} if args.fp8_text_encoder else {}),
                   **({"enable_mxfp4": True} if args.enable_mxfp4 else {}), **kw)


if __name__ == "__main__":
    main()
