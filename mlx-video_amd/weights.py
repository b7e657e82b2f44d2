"""Checkpoint ingestion: safetensors -> bf16 device tensors with the reference's key
maps (ltx.py:508-533 transformer; decoder.py:544-591,675-721 VAE decoder; encoder.py:135-179 VAE encoder;
upsampler.py:319-373), PyTorch conv layouts (O,I,D,H,W) transposed to the MLX layout (O,D,H,W,I) the
kernels consume, and VAE `timestep_conditioning` sniffed from the safetensors metadata
(decoder.py:621-635).  Files are read with safetensors only (nothing is unpickled)."""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Dict, Iterable, List, Optional

import torch

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0                     # largest finite e4m3fn value
FP8_SCALINGS = ("channel", "none")
SCALE_SUFFIX = "_scale"             # "<name>.weight" (e4m3fn) is accompanied by "<name>.weight_scale" ((N) fp32) when it has one


def _to_dev(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=BF16).contiguous()


def _conv_to_mlx(key: str, v: torch.Tensor) -> torch.Tensor:
    if v.ndim == 5 and "weight" in key:
        return v.permute(0, 2, 3, 4, 1).contiguous()      # (O,I,D,H,W) -> (O,D,H,W,I)
    if v.ndim == 4 and "weight" in key:
        return v.permute(0, 2, 3, 1).contiguous()         # (O,I,H,W)   -> (O,H,W,I)
    return v


def scan_header(path: Path) -> Dict[str, dict]:
    """safetensors header parsed directly (8-byte length + JSON), no tensor is materialised: the key / shape scan of
    ltx.py:563-586.  Returns {key: {"dtype", "shape", "data_offsets"}}; "__metadata__" is kept under that name."""
    import struct
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        return json.loads(f.read(n))


def iter_safetensors(paths: Iterable[Path], want=None):
    """Yield (key, host tensor) one tensor at a time (each is dropped by the caller after its device copy, so the
    host never holds the checkpoint: a 26 GB transformer streams through a few hundred MB)."""
    from safetensors import safe_open
    for p in paths:
        with safe_open(str(p), framework="pt", device="cpu") as f:
            for k in f.keys():
                if want is None or want(k):
                    yield k, f.get_tensor(k)


def read_safetensors(paths: Iterable[Path]) -> Dict[str, torch.Tensor]:
    return dict(iter_safetensors(paths))


def read_metadata(path: Path) -> dict:
    return dict(scan_header(path).get("__metadata__") or {})


def quantize_fp8(w: torch.Tensor, scaling: str = "channel"):
    """(N,K) matrix -> (e4m3fn matrix, per-output-channel fp32 scale or None), so that w ~ w8 * scale[:, None].
    "none": the plain cast of the upstream --enable-fp8 path (w.to(float8_e4m3fn)), no scale.
    "channel": scale_n = amax_n / 448 - the row's largest magnitude lands on +-448 exactly and the row uses the whole e4m3
    range; |w - dequantize| <= amax_n * 2^-4 (half an ulp of the 3-bit mantissa in the top binade).  A zero row gets scale 1."""
    if scaling not in FP8_SCALINGS:
        raise ValueError(f"fp8 scaling {scaling!r}: expected one of {FP8_SCALINGS}")
    if w.ndim != 2:
        raise ValueError(f"quantize_fp8: expected a matrix, got shape {tuple(w.shape)}")
    wf = w.float()
    if scaling == "none":
        return w.to(FP8), None
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX)
    # the row's extreme element is +-448 by construction (x / (x / 448) may round one ulp off it)
    q = torch.where(wf.abs() == amax[:, None], torch.copysign(torch.full_like(q, FP8_MAX), wf), q)
    q = torch.where(wf == 0, torch.zeros_like(q), q)
    return q.to(FP8), scale.contiguous()


def dequantize_fp8(w8: torch.Tensor, scale: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """The matrix an e4m3fn panel (and its per-output-channel scale) stands for, in ``dtype``."""
    w = w8.float()
    if scale is not None:
        w = w * scale.float()[:, None]
    return w.to(dtype)


MXFP4_BLOCK = 32                    # OCP MXFP4: e2m1 elements, one e8m0 scale per 32 consecutive k
# the e2m1 magnitudes by their 3-bit index (1 exponent-ish bit pair, 1 mantissa bit); code = sign << 3 | index
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# midpoints between neighbouring magnitudes, and whether a tie at that midpoint goes UP (to the even index)
_E2M1_MID = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def quantize_mxfp4(w: torch.Tensor):
    """(N,K) float matrix, K % 32 == 0 -> (codes (N, K/2) uint8, block_scales (N, K/32) uint8): OCP MXFP4.  fp32 arithmetic on
    the matrix's device.  Per row and block of 32 consecutive k: amax = max |w|; scale byte E = clamp(floor(log2 amax) - 2,
    -127, 127) + 127 (the OCP rule, e2m1's emax = 2; floor(log2) read from the exponent field by ``frexp``), a zero block 127;
    byte 255 (NaN) is never written.  Per element x = w / 2^(E-127) (a power of two: exact), code = the nearest of +-{0, 0.5, 1,
    1.5, 2, 3, 4, 6}, ties to the even 3-bit magnitude index, |x| > 6 saturating to +-6, the sign bit kept (-0 stays -0).
    Element 2i sits in the low nibble of byte i, 2i+1 in the high one (``torch.float4_e2m1fn_x2``'s order).
    |w - dequantize_mxfp4| <= amax_block / 4, the worst case being the clamp at 6 (amax just below 8 x 2^(E-127))."""
    if w.ndim != 2 or w.shape[1] == 0 or w.shape[1] % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4: expected an (N, K) matrix with K a positive multiple of {MXFP4_BLOCK}, got shape {tuple(w.shape)}")
    if not w.dtype.is_floating_point:
        raise ValueError(f"quantize_mxfp4: expected a floating-point matrix, got {w.dtype}")
    wf = w.to(torch.float32)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_mxfp4: the matrix holds NaN or Inf")
    N, K = wf.shape
    blk = wf.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = blk.abs().amax(dim=2)
    # frexp: amax = m * 2^ex with m in [0.5, 1), so floor(log2 amax) = ex - 1 (subnormals included)
    ex = torch.frexp(amax)[1].to(torch.int32)
    e = torch.where(amax > 0, (ex - 1 - 2).clamp(-127, 127), torch.zeros_like(ex))
    # x = w * 2^-e in two exact steps (2^-e itself can be beyond fp32 at e = -127; a product that underflows is below every midpoint)
    half = torch.div(e, 2, rounding_mode="floor")
    x = blk * torch.exp2(-half.to(torch.float32))[..., None] * torch.exp2(-(e - half).to(torch.float32))[..., None]
    ax = x.abs()
    idx = torch.zeros_like(ax, dtype=torch.int32)
    for i, mid in enumerate(_E2M1_MID):          # index = number of midpoints passed; a tie passes it when the upper index is even
        idx += ((ax >= mid) if (i + 1) % 2 == 0 else (ax > mid)).to(torch.int32)
    code = (idx | (torch.signbit(blk).to(torch.int32) << 3)).to(torch.uint8).view(N, K)
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    return codes, (e + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4(codes: torch.Tensor, block_scales: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """The (N,K) matrix an MXFP4 pair stands for: e2m1(code) * 2^(E-127), computed in float64 and exact in fp32 for scale
    bytes 1 .. 254 (byte 255 gives NaN, the format's meaning).  ``codes`` uint8 (or a ``torch.float4_e2m1fn_x2`` view of them)."""
    if codes.dtype != torch.uint8:
        codes = codes.view(torch.uint8)
    if block_scales.dtype != torch.uint8:
        raise TypeError(f"dequantize_mxfp4: block_scales must be uint8, got {block_scales.dtype}")
    if codes.ndim != 2 or block_scales.ndim != 2 or (codes.shape[1] * 2) % MXFP4_BLOCK or \
            tuple(block_scales.shape) != (codes.shape[0], codes.shape[1] * 2 // MXFP4_BLOCK):
        raise ValueError(f"dequantize_mxfp4: codes {tuple(codes.shape)} and block_scales {tuple(block_scales.shape)} are not an "
                         f"(N, K/2) / (N, K/{MXFP4_BLOCK}) pair")
    N, K = codes.shape[0], codes.shape[1] * 2
    nib = torch.stack([codes & 0xF, codes >> 4], dim=2).view(N, K).to(torch.int64)
    mag = torch.tensor(_E2M1, dtype=torch.float64, device=codes.device)[nib & 7]
    val = torch.where((nib & 8) != 0, -mag, mag)
    sc = torch.exp2(block_scales.to(torch.float64) - 127.0)
    sc = torch.where(block_scales == 255, torch.full_like(sc, math.nan), sc)
    return (val.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * sc[..., None]).view(N, K).to(dtype)


def is_fp8_matrix_key(key: str, t: torch.Tensor) -> bool:
    """The tensors --enable-fp8 keeps in e4m3: the (out,in) matrices of the Linear layers (every one of them is a GEMM panel
    of LTXModel._pack); biases, norm weights and the scale-shift tables stay bf16."""
    return key.endswith(".weight") and t.ndim == 2


MXSCALE_SUFFIX = "_mxscale"         # "<name>.weight" (uint8 MXFP4 codes) is accompanied by "<name>.weight_mxscale" ((N, K/32) uint8)
_MXFP4_LINEARS = tuple(f".{a}.{n}.weight" for a in ("attn1", "attn2") for n in ("to_q", "to_k", "to_v", "to_out")) + \
    (".ff.proj_in.weight", ".ff.proj_out.weight")


def is_mxfp4_matrix_key(key: str, t: torch.Tensor) -> bool:
    """The tensors --enable-mxfp4 keeps in MXFP4: the matrices of the IN-BLOCK Linear layers (attn1 / attn2 to_q, to_k, to_v,
    to_out, ff.proj_in, ff.proj_out).  Patchify, the timestep and AdaLN Linears, the caption projection, proj_out, biases, norm
    weights and tables stay bf16."""
    return key.startswith("transformer_blocks.") and key.endswith(_MXFP4_LINEARS) and t.ndim == 2


def _put_transformer_tensor(out: Dict[str, torch.Tensor], key: str, v: torch.Tensor, device, fp8: bool, fp8_scaling: str,
                            mxfp4: bool = False) -> None:
    """One checkpoint tensor under its module key.  fp8: Linear matrices go to e4m3fn - an F8_E4M3 tensor of the checkpoint as
    it is (no upcast, no scale), anything else quantised here, one tensor at a time, on the device it will live on.  mxfp4: the
    in-block Linear matrices go to MXFP4 codes + "<key>_mxscale" block scales the same way; everything else is bf16."""
    if mxfp4 and is_mxfp4_matrix_key(key, v):
        out[key], out[key + MXSCALE_SUFFIX] = quantize_mxfp4(v.to(device=device))
        return
    if fp8 and is_fp8_matrix_key(key, v):
        if v.dtype == FP8:
            out[key] = v.to(device=device).contiguous()
            return
        w8, scale = quantize_fp8(v.to(device=device), fp8_scaling)
        out[key] = w8.contiguous()
        if scale is not None:
            out[key + SCALE_SUFFIX] = scale
        return
    out[key] = _to_dev(v, device)


_TR_PREFIXES = ("transformer_blocks.", "patchify_proj.", "adaln_single.", "caption_projection.", "proj_out.", "scale_shift_table")


def _transformer_key(raw_key: str) -> Optional[str]:
    """Checkpoint key -> module key of the VIDEO transformer, or None (ltx.py:508-533 plus the converted-MLX layout
    where keys are already sanitised, optionally under "transformer.")."""
    from .ltx_model import LTXModel
    k = raw_key
    if k.startswith("model.diffusion_model."):
        m = LTXModel.sanitize({k: None})
        if not m:
            return None
        k = next(iter(m))
    elif k.startswith("transformer."):
        k = k[len("transformer."):]
    if not k.startswith(_TR_PREFIXES):
        return None
    if k.startswith(("audio_", "av_ca_")) or ".audio_" in k or "audio_to_video" in k or "video_to_audio" in k or "a2v_ca" in k:
        return None
    return k


def transformer_weights(raw: Dict[str, torch.Tensor], device, fp8: bool = False, fp8_scaling: str = "channel",
                        mxfp4: bool = False) -> Dict[str, torch.Tensor]:
    """Module-key dict of the video transformer.  ``fp8``: the Linear matrices as e4m3fn panels (plus "<key>_scale" vectors
    under ``fp8_scaling="channel"``) for LTXModel's weight-fp8 GEMMs; off, every tensor is bf16 (an fp8 checkpoint is upcast).
    ``mxfp4``: the in-block Linear matrices as MXFP4 codes plus "<key>_mxscale" block scales (``is_mxfp4_matrix_key``) for
    ltxk_gemm_mxfp4, the rest bf16; not together with ``fp8``."""
    if fp8 and mxfp4:
        raise ValueError("transformer_weights: fp8 and mxfp4 are two weight formats of the same matrices; choose one")
    if fp8 and fp8_scaling not in FP8_SCALINGS:
        raise ValueError(f"fp8 scaling {fp8_scaling!r}: expected one of {FP8_SCALINGS}")
    out = {}
    for k, v in raw.items():
        kk = _transformer_key(k)
        if kk is not None:
            _put_transformer_tensor(out, kk, v, device, fp8, fp8_scaling, mxfp4)
    return out


# top-level / per-block audio names of the joint checkpoint -> the names the one model class reads (ltx.py AudioOnly)
_AUDIO_TOP = (("audio_patchify_proj.", "patchify_proj."), ("audio_adaln_single.", "adaln_single."),
              ("audio_caption_projection.", "caption_projection."), ("audio_proj_out.", "proj_out."))
_AUDIO_BLOCK = (("audio_attn1.", "attn1."), ("audio_attn2.", "attn2."), ("audio_ff.", "ff."))


def _audio_transformer_key(raw_key: str) -> Optional[str]:
    """Checkpoint key -> module key of the AUDIO-ONLY transformer, or None: the ``audio_*`` tensors of the joint checkpoint under
    the video names.  The cross-modal tensors are not part of it - ``audio_to_video_attn`` (which also starts with ``audio_``),
    ``video_to_audio_attn``, ``scale_shift_table_a2v_ca_*``, ``av_ca_*`` - nor is ``audio_embeddings_connector``."""
    from .ltx_model import LTXModel
    k = raw_key
    if k.startswith("model.diffusion_model."):
        m = LTXModel.sanitize({k: None})
        if not m:
            return None
        k = next(iter(m))
    elif k.startswith("transformer."):
        k = k[len("transformer."):]
    if "audio_to_video" in k or "video_to_audio" in k or "a2v_ca" in k or "av_ca_" in k or "embeddings_connector" in k:
        return None
    if k == "audio_scale_shift_table":
        return "scale_shift_table"
    for old, new in _AUDIO_TOP:
        if k.startswith(old):
            return new + k[len(old):]
    if k.startswith("transformer_blocks."):
        head, idx, rest = k.split(".", 2)
        if rest == "audio_scale_shift_table":
            return f"{head}.{idx}.scale_shift_table"
        for old, new in _AUDIO_BLOCK:
            if rest.startswith(old):
                return f"{head}.{idx}.{new}{rest[len(old):]}"
    return None


def audio_transformer_weights(raw: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """Module-key dict of the audio-only transformer (``LTXModel(LTXModelConfig.audio(), ...)``) from the same checkpoint the
    video transformer is read from: ``_audio_transformer_key``.  bf16 (an fp8 checkpoint is upcast)."""
    out = {}
    for k, v in raw.items():
        kk = _audio_transformer_key(k)
        if kk is not None:
            out[kk] = _to_dev(v, device)
    return out


def infer_audio_transformer_config(shapes: Dict[str, Iterable[int]]):
    """``LTXModelConfig.audio()`` with depth, widths and head count from the shapes of an ``audio_transformer_weights`` dict
    (head dim 64: the audio transformer's, config.py audio_attention_head_dim)."""
    from .ltx_model import LTXModelConfig
    layers = 1 + max((int(k.split(".")[1]) for k in shapes if k.startswith("transformer_blocks.")), default=-1)
    if layers <= 0 or "patchify_proj.weight" not in shapes:
        raise ValueError("no audio transformer in this checkpoint: no transformer_blocks.*.audio_* / audio_patchify_proj.weight")
    inner, in_ch = (int(x) for x in shapes["patchify_proj.weight"])
    if inner % 64:
        raise ValueError(f"audio inner dim {inner} is not a multiple of the head dim 64")
    return LTXModelConfig.audio(num_attention_heads=inner // 64, in_channels=in_ch, out_channels=int(list(shapes["proj_out.weight"])[0]),
                                num_layers=layers, cross_attention_dim=inner,
                                caption_channels=int(list(shapes["caption_projection.linear1.weight"])[1]))


def load_audio_transformer(model_repo, device):
    """The audio-only ``LTXModel`` of a local checkpoint directory (generate.py:3969-4015): the ``audio_*`` tensors of its
    LTX-2 safetensors, streamed one by one; strict (every expected key must be there).  FileNotFoundError / ValueError when the
    directory or the audio tensors are missing."""
    from .ltx_model import LTXModel
    root = Path(model_repo)
    if not root.is_dir():
        raise FileNotFoundError(f"model_repo {str(model_repo)!r} is not a local directory; nothing is fetched")
    main = [f for f in sorted(root.glob("*.safetensors")) if "upscaler" not in f.name and "upsampler" not in f.name]
    W = {_audio_transformer_key(k): _to_dev(v, device)
         for k, v in iter_safetensors(main, want=lambda k: _audio_transformer_key(k) is not None)}
    cfg = infer_audio_transformer_config({k: tuple(v.shape) for k, v in W.items()})
    return LTXModel(cfg, W)


_CROSS_MARKS = ("audio_to_video_attn.", "video_to_audio_attn.", "scale_shift_table_a2v_ca_")
_CROSS_ADALN = ("av_ca_video_scale_shift_adaln_single", "av_ca_audio_scale_shift_adaln_single", "av_ca_a2v_gate_adaln_single",
                "av_ca_v2a_gate_adaln_single")


def _cross_transformer_key(raw_key: str) -> Optional[str]:
    """Checkpoint key -> module key of the CROSS-MODAL tensors of the joint transformer, or None: ``audio_to_video_attn.*``,
    ``video_to_audio_attn.*`` and ``scale_shift_table_a2v_ca_*`` of every block and the four ``av_ca_*`` AdaLN-singles - what
    ``_transformer_key`` and ``_audio_transformer_key`` both leave out."""
    from .ltx_model import LTXModel
    k = raw_key
    if k.startswith("model.diffusion_model."):
        m = LTXModel.sanitize({k: None})
        if not m:
            return None
        k = next(iter(m))
    elif k.startswith("transformer."):
        k = k[len("transformer."):]
    if k.startswith("transformer_blocks."):
        return k if any(m in k for m in _CROSS_MARKS) else None
    return k if k.startswith(tuple(m + "." for m in _CROSS_ADALN)) else None


def _missing_cross_keys(video_keys: Iterable[str], cross_keys: Iterable[str]) -> list:
    """The cross tensors a joint transformer of the video set's depth needs and ``cross_keys`` lacks."""
    from .av_model import LTXAVModel
    from .ltx_model import LTXModelConfig
    layers = 1 + max((int(k.split(".")[1]) for k in video_keys if k.startswith("transformer_blocks.")), default=-1)
    want = LTXAVModel.expected_cross_keys(LTXModelConfig(num_layers=layers), None)
    have = set(cross_keys)
    return [k for k in want if k not in have]


def av_transformer_weights(raw: Dict[str, torch.Tensor], device, strict: bool = True):
    """The three module-key dicts of a joint checkpoint, (video, audio, cross): what ``_transformer_key`` keeps, what
    ``_audio_transformer_key`` keeps (under the video names), and the cross-modal tensors (``_cross_transformer_key``).  The sets
    are disjoint by construction - each raw key goes to the first map that takes it - and the embeddings connectors go to none.
    bf16.  ``strict``: ValueError listing the cross tensors that a joint transformer of the video set's depth needs and the
    checkpoint lacks."""
    out = ({}, {}, {})
    for k, v in raw.items():
        for dst, key_of in zip(out, (_transformer_key, _audio_transformer_key, _cross_transformer_key)):
            kk = key_of(k)
            if kk is not None:
                dst[kk] = _to_dev(v, device)
                break
    if strict:
        missing = _missing_cross_keys(out[0], out[2])
        if missing:
            raise ValueError(f"the checkpoint lacks {len(missing)} cross-modal tensors of the joint transformer: {missing}")
    return out


def load_av_transformer(model_repo, device, video=None):
    """The ``LTXAVModel`` of a local joint checkpoint directory: video, audio and cross tensors of its LTX-2 safetensors,
    streamed one by one; strict.  ``video``: the video ``LTXModel`` already built from this checkpoint - only the audio and the
    cross tensors are then read.  FileNotFoundError / ValueError when the directory or a tensor is missing."""
    from .av_model import LTXAVModel
    from .ltx_model import LTXModel
    root = Path(model_repo)
    if not root.is_dir():
        raise FileNotFoundError(f"model_repo {str(model_repo)!r} is not a local directory; nothing is fetched")
    main = [f for f in sorted(root.glob("*.safetensors")) if "upscaler" not in f.name and "upsampler" not in f.name]
    maps = ((lambda k: None) if video is not None else _transformer_key, _audio_transformer_key, _cross_transformer_key)
    sets = ({}, {}, {})
    for k, v in iter_safetensors(main, want=lambda k: any(m(k) is not None for m in maps)):
        for dst, key_of in zip(sets, maps):
            kk = key_of(k)
            if kk is not None:
                dst[kk] = _to_dev(v, device)
                break
    Wv, Wa, Wc = sets
    missing = _missing_cross_keys(Wv if video is None else [f"transformer_blocks.{len(video.blocks) - 1}."], Wc)
    if missing:
        raise ValueError(f"{root} lacks {len(missing)} cross-modal tensors of the joint transformer (audio_mode='joint' needs a joint "
                         f"checkpoint): {missing[:8]}{' ...' if len(missing) > 8 else ''}")
    if video is None:
        video = LTXModel(infer_transformer_config({k: tuple(v.shape) for k, v in Wv.items()}), Wv)
    audio = LTXModel(infer_audio_transformer_config({k: tuple(v.shape) for k, v in Wa.items()}), Wa)
    return LTXAVModel(video, audio, Wc)


def quantize_transformer_weights(W: Dict[str, torch.Tensor], fp8_scaling: str = "channel") -> Dict[str, torch.Tensor]:
    """A bf16 module-key dict (e.g. after a LoRA merge) -> the dict ``transformer_weights(fp8=True)`` gives; the input is kept."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in W.items():
        if k.endswith(SCALE_SUFFIX) or v.dtype == FP8:            # already quantised (an fp8 dict passes through unchanged)
            out[k] = v
        else:
            _put_transformer_tensor(out, k, v, v.device, True, fp8_scaling)
    return out


def quantize_transformer_weights_mxfp4(W: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A bf16 module-key dict (e.g. after a LoRA merge) -> the dict ``transformer_weights(mxfp4=True)`` gives: the in-block Linear
    matrices as ``quantize_mxfp4`` codes under their keys and block scales under "<key>_mxscale", tensor by tensor on the device
    each lives on; every other tensor is the same object.  The input is kept; an already quantised dict passes through unchanged."""
    if any(k.endswith(MXSCALE_SUFFIX) for k in W):
        return dict(W)
    out: Dict[str, torch.Tensor] = {}
    for k, v in W.items():
        if is_mxfp4_matrix_key(k, v):
            out[k], out[k + MXSCALE_SUFFIX] = quantize_mxfp4(v)
        else:
            out[k] = v
    return out


def infer_transformer_config(shapes: Dict[str, Iterable[int]]):
    """LTXModelConfig from the tensor shapes of a (sanitised) checkpoint: depth from the block indices, inner dim
    from patchify_proj, caption width from caption_projection.linear1, head count = inner_dim / 128 (the head dim is
    fixed by the RoPE / attention kernels, config.py:93-129)."""
    from .ltx_model import LTXModelConfig
    layers = 1 + max((int(k.split(".")[1]) for k in shapes if k.startswith("transformer_blocks.")), default=-1)
    if layers <= 0 or "patchify_proj.weight" not in shapes:
        raise ValueError("not an LTX-2 transformer checkpoint: no transformer_blocks.* / patchify_proj.weight")
    inner, in_ch = (int(x) for x in shapes["patchify_proj.weight"])
    if inner % 128:
        raise ValueError(f"inner dim {inner} is not a multiple of the head dim 128")
    cap = int(list(shapes["caption_projection.linear1.weight"])[1])
    out_ch = int(list(shapes["proj_out.weight"])[0])
    return LTXModelConfig(num_attention_heads=inner // 128, attention_head_dim=128, in_channels=in_ch, out_channels=out_ch,
                          num_layers=layers, cross_attention_dim=inner, caption_channels=cap)


def vae_decoder_weights(raw: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """decoder.py:675-721: strip `vae.decoder.` / `decoder.`, remap diffusers names, transpose convs,
    per-channel statistics -> latents_mean / latents_std."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in raw.items():
        kk = _vae_decoder_key(k)
        if kk is not None:
            out[kk] = _to_dev(_conv_to_mlx(kk, v), device)
    _alias_stats(out)
    return out


# Per-channel statistics tensors the reference loads, by exact name (decoder.py:667-690, encoder.py:141-157).  A PyTorch
# LTX-2 checkpoint also carries `channel`, `mean-of-stds`, `mean-of-stds_over_std-of-means` (convert.py:277-286 skips them)
# and an `audio_vae.per_channel_statistics.*` pair of the same shape: none of those may land on the video VAE's mean / std.
_STATS_PREFIXES = ("vae.per_channel_statistics.", "per_channel_statistics.")
_STATS_NAMES = {"mean-of-means": "mean", "mean": "mean", "std-of-means": "std", "std": "std"}


def _stats_kind(k: str) -> Optional[str]:
    """'mean' / 'std' for the video VAE's statistics tensors, None for every other key."""
    for pre in _STATS_PREFIXES:
        if k.startswith(pre):
            return _STATS_NAMES.get(k[len(pre):])
    return None


def _vae_decoder_key(k: str) -> Optional[str]:
    from .video_vae import LTX2VideoDecoder
    kk = k
    for pre in ("vae.decoder.", "vae_decoder.", "decoder."):
        if kk.startswith(pre):
            kk = kk[len(pre):]
            break
    else:
        if k in ("latents_mean", "latents_std"):
            return k
        kind = _stats_kind(k)
        if kind is None:
            return None
        # keep the checkpoint's own name so that _alias_stats applies the reference's precedence
        # (per_channel_statistics.mean / .std override *-of-means, decoder.py:676-689)
        return "per_channel_statistics." + k.rsplit(".", 1)[-1]
    return LTX2VideoDecoder.remap_decoder_key(kk)


def _alias_stats(out: Dict[str, torch.Tensor]) -> None:
    """The chain of `if key in weights` assignments of decoder.py:676-695: *-of-means first, plain per_channel_statistics
    .mean / .std override them, explicit latents_mean / latents_std override both."""
    explicit = {d: out[d] for d in ("latents_mean", "latents_std") if d in out}
    for src, dst in (("per_channel_statistics.mean-of-means", "latents_mean"), ("per_channel_statistics.std-of-means", "latents_std"),
                     ("per_channel_statistics.mean", "latents_mean"), ("per_channel_statistics.std", "latents_std")):
        if src in out:
            out[dst] = out[src]
    out.update(explicit)


def _resolve_encoder_stats(out: Dict[str, torch.Tensor]) -> None:
    """encoder.py:141-157: plain `mean` / `std` override the *-of-means tensors, whatever the order in the file."""
    for kind in ("mean", "std"):
        of = out.pop(f"per_channel_statistics.{kind}#of-means", None)
        if of is not None and f"per_channel_statistics.{kind}" not in out:
            out[f"per_channel_statistics.{kind}"] = of


def _vae_encoder_key(k: str) -> Optional[str]:
    kk = None
    for pre in ("vae.encoder.", "vae_encoder.", "encoder."):
        if k.startswith(pre):
            kk = k[len(pre):]
    if kk is None:
        kind = _stats_kind(k)
        if kind is None:
            return None
        # "-of-means" names first, plain "mean"/"std" override them (encoder.py:141-157): see vae_encoder_weights
        return "per_channel_statistics." + kind + ("" if k.rsplit(".", 1)[-1] in ("mean", "std") else "#of-means")
    kk = kk.replace(".conv.conv.", ".conv.").replace("conv_in.conv.", "conv_in.").replace("conv_out.conv.", "conv_out.")
    return kk.replace(".conv1.conv.", ".conv1.").replace(".conv2.conv.", ".conv2.")


def vae_encoder_weights(raw: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """encoder.py:135-179: strip `vae.encoder.` / `encoder.`, drop the `.conv.` wrapper level, transpose convs."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in raw.items():
        kk = _vae_encoder_key(k)
        if kk is not None:
            out[kk] = _to_dev(_conv_to_mlx(kk, v), device)
    _resolve_encoder_stats(out)
    return out


def upsampler_weights(raw: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """upsampler.py:345-367."""
    return {k: _to_dev(_conv_to_mlx(k, v) if "conv" in k else v, device) for k, v in raw.items()}


def sniff_timestep_conditioning(path: Path) -> bool:
    """decoder.py:621-635."""
    try:
        cfg = json.loads(read_metadata(path).get("config", "{}"))
        return bool(cfg.get("vae", {}).get("timestep_conditioning", False))
    except Exception:
        return False


# ------------------------------------------------------------------------------------------- text connector
def aggregate_k_to_layer_major(w: torch.Tensor, D: int) -> torch.Tensor:
    """aggregate_embed.weight (N, D*L) with the checkpoint's K order d*L + l (text_encoder.py:598,633: the hidden states are
    stacked on the last axis and flattened) -> K order l*D + d, the column order of ltxk_layer_norm_compact's output."""
    N, K = w.shape
    if K % D:
        raise ValueError(f"aggregate_embed.weight has K = {K}, not a multiple of the hidden width {D}")
    return w.reshape(N, D, K // D).transpose(1, 2).reshape(N, K).contiguous()


def aggregate_k_from_layer_major(w: torch.Tensor, D: int) -> torch.Tensor:
    """The inverse of ``aggregate_k_to_layer_major``."""
    N, K = w.shape
    return w.reshape(N, K // D, D).transpose(1, 2).reshape(N, K).contiguous()


# (aggregate_embed key, connector prefix) of the three layouts the reference reads (text_encoder.py:756-836), in its order of
# precedence: the LTX-2 checkpoint itself, a converted `connector.*` file, a diffusers `connectors/` file
_CONNECTOR_FAMILIES = (("text_embedding_projection.aggregate_embed.weight", "model.diffusion_model.video_embeddings_connector."),
                       ("text_embedding_projection.aggregate_embed.weight", "connector.video_embeddings_connector."),
                       ("text_proj_in.weight", "video_connector."))


def _connector_key(k: str) -> str:
    """text_encoder.py:820-828."""
    return k.replace(".ff.net.0.proj.", ".ff.proj_in.").replace(".ff.net.2.", ".ff.proj_out.").replace(".to_out.0.", ".to_out.")


def text_connector_weights(files: Iterable[Path], device, which: str = "video") -> Dict[str, torch.Tensor]:
    """The feature extractor + video embeddings connector of ``text_connector.TextConnector`` from safetensors files, under
    module keys: ``aggregate_embed.weight_layer_major`` (K axis permuted, ``aggregate_k_to_layer_major``),
    ``learnable_registers``, ``transformer_1d_blocks.*``.  Three key families are read (text_encoder.py:756-836):
    `text_embedding_projection.aggregate_embed.weight` + `model.diffusion_model.video_embeddings_connector.*`;
    `connector.video_embeddings_connector.*`; `text_proj_in.weight` + `video_connector.*` (a diffusers
    connectors/diffusion_pytorch_model.safetensors).  The first family that has connector tensors wins, as in the reference;
    `audio_embeddings_connector.*` / `audio_connector.*` are ignored.
    ``which="audio"``: the audio embeddings connector instead (text_encoder.py:838-871) - the same three families with
    `audio_` in place of `video_` in the prefix, the same aggregate_embed (the feature extractor is shared); the video
    connector's tensors are then the ignored ones."""
    if which not in ("video", "audio"):
        raise ValueError(f"text_connector_weights: which must be 'video' or 'audio', got {which!r}")
    families = _CONNECTOR_FAMILIES if which == "video" else \
        tuple((agg, pre.replace("video_", "audio_")) for agg, pre in _CONNECTOR_FAMILIES)
    files = [Path(f) for f in files]
    found = []
    for f in files:
        keys = [k for k in scan_header(f) if k != "__metadata__"]
        for fam, (agg_key, prefix) in enumerate(families):
            if any(k.startswith(prefix) for k in keys):
                found.append((fam, f))
    if not found:
        raise ValueError("no text connector in " + ", ".join(str(f) for f in files) + f": expected {which}_embeddings_connector.* "
                         f"(LTX-2 checkpoint) or {which}_connector.* (connectors/diffusion_pytorch_model.safetensors) tensors")
    fam = min(fam for fam, _ in found)
    agg_key, prefix = families[fam]
    out: Dict[str, torch.Tensor] = {}
    agg = None
    for k, v in iter_safetensors(files, want=lambda k: k == agg_key or k.startswith(prefix)):
        if k == agg_key:
            agg = v
        else:
            out[_connector_key(k[len(prefix):])] = _to_dev(v, device)
    if agg is None:
        raise ValueError(f"the connector tensors ({prefix}*) come without {agg_key}")
    if "learnable_registers" not in out:
        raise ValueError(f"{prefix}learnable_registers is missing")
    D = int(out["learnable_registers"].shape[1])
    out["aggregate_embed.weight_layer_major"] = aggregate_k_to_layer_major(agg.to(device=device, dtype=BF16), D)
    return out


# ------------------------------------------------------------------------------------------------ Gemma-3 text encoder
_GEMMA_PREFIXES = ("model.language_model.", "language_model.model.", "language_model.")     # longest match first
_GEMMA_SKIP = ("vision_tower.", "vision_model.", "multi_modal_projector.", "model.vision_tower.", "model.multi_modal_projector.")


def gemma_shard_files(root: Path) -> list:
    """The one shard set of a local Gemma-3 directory the reference would read (text_encoder.py:200-216): an indexed
    diffusion_pytorch_model-* set, else an indexed model-* set, else the single file of either name, else every *.safetensors."""
    root = Path(root)
    if (root / "diffusion_pytorch_model.safetensors.index.json").exists():
        files = sorted(root.glob("diffusion_pytorch_model-*.safetensors"))
    elif (root / "model.safetensors.index.json").exists():
        files = sorted(root.glob("model-*.safetensors"))
    elif (root / "diffusion_pytorch_model.safetensors").exists():
        files = [root / "diffusion_pytorch_model.safetensors"]
    elif (root / "model.safetensors").exists():
        files = [root / "model.safetensors"]
    else:
        files = sorted(root.glob("*.safetensors"))
    return files or sorted(root.glob("*.safetensors"))


def gemma_key(raw_key: str) -> Optional[str]:
    """The language model's own key (``embed_tokens.weight``, ``layers.{i}...``, ``norm.weight``) of a checkpoint key, None for
    what the encoder does not use (vision tower, projector, lm_head)."""
    k = raw_key
    if any(k.startswith(p) or ("." + p) in k for p in _GEMMA_SKIP):
        return None
    for p in _GEMMA_PREFIXES:
        if k.startswith(p):
            k = k[len(p):]
            break
    if k.startswith("model."):
        k = k[len("model."):]
    if k.startswith(("embed_tokens.", "layers.", "norm.")):
        return k
    return None


def gemma_weights(root, device, fp8: Optional[str] = None, fp8_scaling: str = "channel") -> Dict[str, torch.Tensor]:
    """The Gemma-3 language model of a local directory as device bf16 tensors under its own keys, for ``gemma.GemmaEncoder``.
    Streams the shards of ``gemma_shard_files`` one tensor at a time; fp32 tensors are cast to bf16 (text_encoder.py:154-163),
    vision-tower keys skipped.  A pre-quantised checkpoint (.scales / .biases) raises, as the DiT loader does.
    ``fp8`` (one of FP8_SCALINGS, or True for ``fp8_scaling``): the matrices - the projections and the embedding table - come
    back as e4m3fn with ``key + SCALE_SUFFIX`` scales under "channel", each quantised as it streams (``_put_transformer_tensor``:
    no bf16 copy of the model is ever resident); an F8_E4M3 tensor of the checkpoint is kept as it is, unscaled.  Norm weights
    stay bf16."""
    if fp8 is True:
        fp8 = fp8_scaling
    if fp8 is not None and fp8 is not False and fp8 not in FP8_SCALINGS:
        raise ValueError(f"fp8 scaling {fp8!r}: expected one of {FP8_SCALINGS}")
    root = Path(root)
    if not root.is_dir():
        raise FileNotFoundError(f"{root} is not a local directory (repo names are not resolved and nothing is fetched)")
    files = gemma_shard_files(root)
    if not files:
        raise FileNotFoundError(f"no *.safetensors in {root}")
    for f in files:
        if any(k.endswith((".scales", ".biases")) for k in scan_header(f)):
            raise ValueError(f"{f.name}: pre-quantised MLX checkpoints (.scales/.biases) are not supported: MLX affine quantisation is "
                             "out of scope; use the bf16 Gemma-3 weights")
    out: Dict[str, torch.Tensor] = {}
    for k, v in iter_safetensors(files, want=lambda k: gemma_key(k) is not None):
        if not v.dtype.is_floating_point:
            raise ValueError(f"{k}: expected a floating-point tensor, got {v.dtype}")
        if fp8:
            _put_transformer_tensor(out, gemma_key(k), v, device, True, fp8)
        else:
            out[gemma_key(k)] = _to_dev(v, device)
    if "embed_tokens.weight" not in out:
        raise ValueError(f"no language-model tensors (…embed_tokens.weight) in {', '.join(f.name for f in files)}")
    return out


def infer_encoder_blocks(keys: Iterable[str]):
    """Encoder block list from the checkpoint's key set: `down_blocks.i.res_blocks.j.*` => ("res_x", n); a bare
    `down_blocks.i.conv.*` is a compress block whose stride follows the default schedule of encoder.py:95-105."""
    from .video_vae import ENC_BLOCKS
    res: Dict[int, int] = {}
    comp = set()
    for k in keys:
        p = k.split(".")
        if len(p) >= 3 and p[0] == "down_blocks" and p[1].isdigit():
            i = int(p[1])
            if p[2] == "res_blocks" and len(p) > 3 and p[3].isdigit():
                res[i] = max(res.get(i, 0), int(p[3]) + 1)
            elif p[2] == "conv":
                comp.add(i)
    n = 1 + max(list(res) + list(comp), default=-1)
    if n != len(ENC_BLOCKS):
        return None
    blocks = []
    for i in range(n):
        kind, arg = ENC_BLOCKS[i]
        if i in res:
            if kind != "res_x":
                return None
            blocks.append(("res_x", res[i]))
        elif i in comp and kind != "res_x":
            blocks.append((kind, arg))
        else:
            return None
    return blocks


def load_pipeline_modules(model_repo: str, device, need_encoder: bool = False, need_upsampler: bool = False,
                          loras: Optional[list] = None, build_transformer: bool = True, fp8: bool = False,
                          fp8_scaling: str = "channel", need_text_connector: bool = False, mxfp4: bool = False) -> dict:
    """Local-directory loader (no network: repo *names* are not resolved, utils.py:78-374 is out of scope).
    Headers are scanned first (keys, shapes, `timestep_conditioning` metadata), the architecture is inferred from the
    shapes, then tensors stream one by one straight into device memory under their module keys (ltx.py:548-826,
    decoder.py:594-740, encoder.py:108-187).  Returns the modules plus ``transformer_weights`` / ``transformer_config``
    (the base dict stays reachable so LoRA-merged twins can be built, generate.py:2957-3031,3229-3237).
    ``need_text_connector``: also ``mods["text_connector"]``, a ``TextConnector`` built from the directory's files and its
    ``connectors/`` sub-directory (``text_connector_weights``).
    ``mxfp4``: the transformer's in-block Linear matrices as MXFP4 (``transformer_weights(mxfp4=True)``), each quantised as it
    streams; with ``loras`` the merge runs on the bf16 dict and the result is quantised.  Not together with ``fp8``."""
    from .ltx_model import LTXModel
    from .video_vae import LTX2VideoDecoder, VideoEncoder
    if fp8 and mxfp4:
        raise ValueError("load_pipeline_modules: fp8 and mxfp4 are two weight formats of the same matrices; choose one")
    root = Path(model_repo)
    if not root.exists():
        raise FileNotFoundError(f"model_repo {model_repo!r} is not a local directory; HF downloads are not available offline")
    files = sorted(root.glob("*.safetensors"))
    if not files:
        raise FileNotFoundError(f"no .safetensors under {root}")
    main = [f for f in files if "upscaler" not in f.name and "upsampler" not in f.name]
    ups = [f for f in files if "upscaler" in f.name or "upsampler" in f.name]
    # ---- pass 1: headers only ----
    tshapes: Dict[str, list] = {}
    enc_keys = []
    has_quant = False
    for f in main:
        for k, meta in scan_header(f).items():
            if k == "__metadata__":
                continue
            has_quant = has_quant or k.endswith((".scales", ".biases"))
            tk = _transformer_key(k)
            if tk is not None:
                tshapes[tk] = meta["shape"]
            ek = _vae_encoder_key(k)
            if ek is not None:
                enc_keys.append(ek.replace("#of-means", ""))
    if has_quant:
        raise ValueError("pre-quantised MLX checkpoints (.scales/.biases) are not supported: MLX affine quantisation is out of scope "
                         "(SURVEY.md §2a); use bf16 weights")
    tcfg = infer_transformer_config(tshapes)
    missing = [k for k in LTXModel.expected_keys(tcfg) if k not in tshapes]
    if missing:   # strict load (ltx.py:874-881)
        raise ValueError(f"Missing {len(missing)} parameters in checkpoint, e.g. {missing[:4]}")
    # ---- pass 2: stream tensors to the device ----
    tw: Dict[str, torch.Tensor] = {}
    dw: Dict[str, torch.Tensor] = {}
    ew: Dict[str, torch.Tensor] = {}
    for k, v in iter_safetensors(main):
        tk = _transformer_key(k)
        if tk is not None:
            # (a LoRA is merged into bf16 matrices and the merged dict quantised: merge-then-quantise)
            _put_transformer_tensor(tw, tk, v, device, fp8 and not loras, fp8_scaling, mxfp4 and not loras)
            continue
        dk = _vae_decoder_key(k)
        if dk is not None:
            dw[dk] = _to_dev(_conv_to_mlx(dk, v), device)
        if need_encoder:
            ek = _vae_encoder_key(k)
            if ek is not None:
                ew[ek] = _to_dev(_conv_to_mlx(ek, v), device)
    _alias_stats(dw)
    _resolve_encoder_stats(ew)
    mods = {"transformer_weights": tw, "transformer_config": tcfg}
    if build_transformer:
        w = tw
        if loras:
            from .lora import LoraSpec, apply_lora_to_weights
            w = apply_lora_to_weights(tw, [LoraSpec(Path(p), float(s)) for p, s in loras])
            if fp8:
                w = quantize_transformer_weights(w, fp8_scaling)
            if mxfp4:
                w = quantize_transformer_weights_mxfp4(w)
        mods["transformer"] = LTXModel(tcfg, w)
    nres = 1 + max((int(k.split(".")[3]) for k in dw if k.startswith("up_blocks.0.res_blocks.")), default=4)
    mods["vae_decoder"] = LTX2VideoDecoder(dw, timestep_conditioning=any(sniff_timestep_conditioning(f) for f in main),
                                           num_layers_per_block=nres)
    if need_encoder:
        mods["vae_encoder"] = VideoEncoder(ew, encoder_blocks=infer_encoder_blocks(ew.keys()))
    if need_upsampler and ups:
        from .upsampler import LatentUpsampler
        uw = {k: _to_dev(_conv_to_mlx(k, v) if "conv" in k else v, device) for k, v in iter_safetensors(ups[:1])}
        nb = 1 + max((int(k.split(".")[1]) for k in uw if k.startswith("res_blocks.")), default=3)
        mods["upsampler"] = LatentUpsampler(uw, num_blocks_per_stage=nb)
    if need_text_connector:
        from .text_connector import TextConnector
        mods["text_connector"] = TextConnector(text_connector_weights(main + sorted((root / "connectors").glob("*.safetensors")), device))
    return mods


# ---- audio VAE decoder and vocoder (convert.py:376-471 as key maps) --------------------------------------------------------
# Three sources: the tensors of a unified (already converted) checkpoint under `audio_vae.` / `vocoder.` - MLX layouts, the
# reference loads them as they are -; `audio_vae/` and `vocoder/` `diffusion_pytorch_model.safetensors`; and the full PyTorch
# checkpoint.  The latter two carry PyTorch layouts: Conv2d (O,I,H,W) -> (O,H,W,I), Conv1d (O,I,k) -> (O,k,I), ConvTranspose1d
# (I,O,k) -> (O,k,I).  Everything is cast to bf16 like every other module.
_AUDIO_STATS = {"mean-of-means": "_mean_of_means", "std-of-means": "_std_of_means", "_mean_of_means": "_mean_of_means",
                "_std_of_means": "_std_of_means"}


def _audio_decoder_key(k: str) -> Optional[str]:
    """The decoder's own name of a checkpoint key, `per_channel_statistics._mean_of_means` / `._std_of_means` for either
    spelling of the statistics, None for every other tensor (the encoder's included)."""
    if k in ("latents_mean", "latents_std"):                    # audio_vae/diffusion_pytorch_model.safetensors
        return "per_channel_statistics." + ("_mean_of_means" if k.endswith("mean") else "_std_of_means")
    if k.startswith("audio_vae."):
        k = k[len("audio_vae."):]
    if k.startswith("decoder."):
        return k[len("decoder."):]
    if k.startswith("per_channel_statistics."):
        name = _AUDIO_STATS.get(k[len("per_channel_statistics."):])
        return None if name is None else "per_channel_statistics." + name
    return None


def audio_decoder_weights(raw: Dict[str, torch.Tensor], device, layout: str = "pytorch") -> Dict[str, torch.Tensor]:
    """sanitize_audio_vae_weights (convert.py:376-419) for the decoder: keys by ``_audio_decoder_key``; ``layout`` "pytorch"
    transposes 4-D conv weights to (O,H,W,I), "mlx" (a unified checkpoint) takes them as they are."""
    if layout not in ("pytorch", "mlx"):
        raise ValueError(f"audio_decoder_weights: layout must be 'pytorch' or 'mlx', got {layout!r}")
    out: Dict[str, torch.Tensor] = {}
    for k, v in raw.items():
        kk = _audio_decoder_key(k)
        if kk is None:
            continue
        if layout == "pytorch" and v.ndim == 4 and "conv" in kk.lower() and "weight" in kk:
            v = v.permute(0, 2, 3, 1)
        out[kk] = _to_dev(v, device)
    return out


_VOCODER_RENAMES = (("upsamplers.", "ups."), ("resnets.", "resblocks."), ("conv_in.", "conv_pre."), ("conv_out.", "conv_post."))


def _vocoder_key(k: str, has_prefix: bool) -> Optional[str]:
    if has_prefix:
        if not k.startswith("vocoder."):
            return None
        k = k[len("vocoder."):]
    for old, new in _VOCODER_RENAMES:
        if k.startswith(old):
            return new + k[len(old):]
    return k if k.startswith(("ups.", "resblocks.", "conv_pre.", "conv_post.")) else None


def vocoder_weights(raw: Dict[str, torch.Tensor], device, layout: str = "pytorch") -> Dict[str, torch.Tensor]:
    """sanitize_vocoder_weights (convert.py:422-471): only `vocoder.` keys where any key has that prefix, the upstream
    names (upsamplers / resnets / conv_in / conv_out) mapped to ups / resblocks / conv_pre / conv_post; ``layout`` "pytorch"
    transposes Conv1d (O,I,k) and ConvTranspose1d (I,O,k) weights to (O,k,I)."""
    if layout not in ("pytorch", "mlx"):
        raise ValueError(f"vocoder_weights: layout must be 'pytorch' or 'mlx', got {layout!r}")
    has_prefix = any(k.startswith("vocoder.") for k in raw)
    out: Dict[str, torch.Tensor] = {}
    for k, v in raw.items():
        kk = _vocoder_key(k, has_prefix)
        if kk is None:
            continue
        if layout == "pytorch" and v.ndim == 3 and "weight" in kk:
            v = v.permute(1, 2, 0) if kk.startswith("ups.") else v.permute(0, 2, 1)
        out[kk] = _to_dev(v, device)
    return out


def _audio_source(model_repo, sub: str, prefix: str, unified: Optional[Dict[str, torch.Tensor]]):
    """(raw tensors, layout) from the first source that has them (generate.py:1725-1760): the unified dict's `prefix` keys,
    `<repo>/<sub>/diffusion_pytorch_model.safetensors`, the repo's full checkpoint."""
    if unified is not None:
        picked = {k: v for k, v in unified.items() if k.startswith(prefix)}
        if picked:
            return picked, "mlx"
    root = Path(model_repo) if model_repo is not None else None
    if root is not None:
        f = root / sub / "diffusion_pytorch_model.safetensors"
        if f.exists():
            return read_safetensors([f]), "pytorch"
        main = [p for p in sorted(root.glob("*.safetensors")) if "upscaler" not in p.name and "upsampler" not in p.name]
        raw = dict(iter_safetensors(main, want=lambda k: k.startswith(prefix)))
        if raw:
            return raw, "pytorch"
    raise FileNotFoundError(f"{prefix}* weights not found: no unified tensors, no {sub}/diffusion_pytorch_model.safetensors and no "
                            f"checkpoint with them under {model_repo!r}")


def load_audio_decoder(model_repo, device, unified_weights: Optional[Dict[str, torch.Tensor]] = None):
    """The ``AudioDecoder`` of ``model_repo`` (a local directory) or of ``unified_weights`` (generate.py:1706-1763)."""
    from .audio_vae import AudioDecoder
    raw, layout = _audio_source(model_repo, "audio_vae", "audio_vae.", unified_weights)
    W = audio_decoder_weights(raw, device, layout)
    # width and depth from the shapes, as the other loaders infer theirs: conv_out reads ch channels, level 0 has num_res_blocks + 1 blocks
    nres = max((int(k.split(".")[3]) for k in W if k.startswith("up.0.block.")), default=2)
    return AudioDecoder(W, ch=W["conv_out.conv.weight"].shape[-1], num_res_blocks=nres)


def load_vocoder(model_repo, device, unified_weights: Optional[Dict[str, torch.Tensor]] = None):
    """The ``Vocoder`` of ``model_repo`` or of ``unified_weights`` (generate.py:1766-1812)."""
    from .audio_vae import Vocoder
    raw, layout = _audio_source(model_repo, "vocoder", "vocoder.", unified_weights)
    W = vocoder_weights(raw, device, layout)
    return Vocoder(W, upsample_initial_channel=W["conv_pre.weight"].shape[0])


def random_upsampler_weights(device, mid: int = 1024, seed: int = 99, nb: int = 4) -> Dict[str, torch.Tensor]:
    g = torch.Generator(device=device).manual_seed(seed)
    W: Dict[str, torch.Tensor] = {}

    def rn(*shape, std=1.0, mean=0.0):
        return (torch.randn(shape, generator=g, device=device) * std + mean).to(BF16)

    def conv(name, o, i):
        W[f"{name}.weight"], W[f"{name}.bias"] = rn(o, 3, 3, 3, i, std=1.0 / math.sqrt(27 * i)), rn(o, std=0.01)

    def norm(name, c):
        W[f"{name}.weight"], W[f"{name}.bias"] = rn(c, std=0.1, mean=1.0), rn(c, std=0.1)

    conv("initial_conv", mid, 128); norm("initial_norm", mid)
    for stage in ("res_blocks", "post_upsample_res_blocks"):
        for i in range(nb):
            conv(f"{stage}.{i}.conv1", mid, mid); norm(f"{stage}.{i}.norm1", mid)
            conv(f"{stage}.{i}.conv2", mid, mid); norm(f"{stage}.{i}.norm2", mid)
    W["upsampler.conv.weight"], W["upsampler.conv.bias"] = rn(4 * mid, 3, 3, mid, std=1.0 / math.sqrt(9 * mid)), rn(4 * mid, std=0.01)
    conv("final_conv", 128, mid)
    return W
