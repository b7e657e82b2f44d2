"""Guidance configs.  ``GuiderConfig``: which x0-space guider of ltx_core/components/guiders.py the guided denoise loop
runs in the CFG slot.  The rest: perturbation configs of spatio-temporal guidance (STG), ltx_core/guidance/perturbations.py
with torch in place of mx.

A ``BatchedPerturbationConfig`` holds one ``PerturbationConfig`` per batch row of a forward.  ``mask(type, block)`` is 1 for
a row that runs the perturbable operation of ``block`` as usual and 0 for a row in which it is perturbed.  The only type this
video-only model acts on is ``SKIP_VIDEO_SELF_ATTN``: in such a row the self-attention of the block returns its value
projection instead of softmax(q k^T) v (``LTXModel.forward_tokens``, DESIGN.md "Spatio-temporal guidance").  The audio
types are accepted and have no effect."""
from __future__ import annotations

import math
from dataclasses import dataclass
from enum import Enum
from typing import List, Optional

import torch


GUIDER_KINDS = ("cfg", "cfg_star", "apg")


@dataclass(frozen=True)
class GuiderConfig:
    """The guider of the CFG slot: ``cfg`` (CFGGuider, the fused velocity-space step tail), ``cfg_star``
    (CFGStarRescalingGuider) or ``apg`` (LtxAPGGuider with ``eta`` and ``norm_threshold``; 0 = no norm clamp).  The scale is
    the loop's ``cfg_scale``; at cfg_scale == 1 every kind is disabled, as the reference's ``enabled()``.  ``eta`` and
    ``norm_threshold`` are validated for every kind and used by ``apg`` only."""
    kind: str = "cfg"
    eta: float = 1.0
    norm_threshold: float = 0.0

    def __post_init__(self):
        if self.kind not in GUIDER_KINDS:
            raise ValueError(f"Unknown guider: {self.kind!r} (expected one of {GUIDER_KINDS})")
        try:
            eta, thr = float(self.eta), float(self.norm_threshold)
        except (TypeError, ValueError):
            raise ValueError(f"apg_eta / apg_norm_threshold must be numbers, got {self.eta!r} / {self.norm_threshold!r}") from None
        if not math.isfinite(eta):
            raise ValueError(f"apg_eta must be finite, got {self.eta!r}")
        if not (math.isfinite(thr) and thr >= 0.0):
            raise ValueError(f"apg_norm_threshold must be finite and >= 0, got {self.norm_threshold!r}")
        object.__setattr__(self, "eta", eta)
        object.__setattr__(self, "norm_threshold", thr)

    @property
    def is_default(self) -> bool:
        return self.kind == "cfg"

    @property
    def key(self) -> tuple:
        """What distinguishes two captured step graphs."""
        return (self.kind, self.eta, self.norm_threshold)

    def component(self, scale: float):
        """The host-side guider of ``components`` this config stands for at ``scale``."""
        from . import components as C
        if self.kind == "cfg":
            return C.CFGGuider(scale)
        if self.kind == "cfg_star":
            return C.CFGStarRescalingGuider(scale)
        return C.LtxAPGGuider(scale, self.eta, self.norm_threshold)


class PerturbationType(Enum):
    """Types of attention perturbations for STG (Spatio-Temporal Guidance)."""

    SKIP_A2V_CROSS_ATTN = "skip_a2v_cross_attn"
    SKIP_V2A_CROSS_ATTN = "skip_v2a_cross_attn"
    SKIP_VIDEO_SELF_ATTN = "skip_video_self_attn"
    SKIP_AUDIO_SELF_ATTN = "skip_audio_self_attn"


@dataclass(frozen=True)
class Perturbation:
    type: PerturbationType
    blocks: Optional[List[int]]          # None: every block

    def is_perturbed(self, perturbation_type: PerturbationType, block: int) -> bool:
        if self.type != perturbation_type:
            return False
        if self.blocks is None:
            return True
        return block in self.blocks


@dataclass(frozen=True)
class PerturbationConfig:
    perturbations: Optional[List[Perturbation]]

    def is_perturbed(self, perturbation_type: PerturbationType, block: int) -> bool:
        if self.perturbations is None:
            return False
        return any(p.is_perturbed(perturbation_type, block) for p in self.perturbations)

    @staticmethod
    def empty() -> "PerturbationConfig":
        return PerturbationConfig([])


@dataclass(frozen=True)
class BatchedPerturbationConfig:
    perturbations: List[PerturbationConfig]

    def mask(self, perturbation_type: PerturbationType, block: int, device=None,
             dtype: torch.dtype = torch.float32) -> torch.Tensor:
        m = torch.ones((len(self.perturbations),), dtype=dtype, device=device)
        for i, p in enumerate(self.perturbations):
            if p.is_perturbed(perturbation_type, block):
                m[i] = 0
        return m

    def mask_like(self, perturbation_type: PerturbationType, block: int, values: torch.Tensor) -> torch.Tensor:
        m = self.mask(perturbation_type, block, values.device, values.dtype)
        return m.reshape((m.shape[0],) + (1,) * (values.dim() - 1))

    def any_in_batch(self, perturbation_type: PerturbationType, block: int) -> bool:
        return any(p.is_perturbed(perturbation_type, block) for p in self.perturbations)

    def all_in_batch(self, perturbation_type: PerturbationType, block: int) -> bool:
        return all(p.is_perturbed(perturbation_type, block) for p in self.perturbations)

    def rows(self, perturbation_type: PerturbationType, block: int) -> List[int]:
        """The batch rows perturbed in ``block`` (the zeros of ``mask``), as host ints."""
        return [i for i, p in enumerate(self.perturbations) if p.is_perturbed(perturbation_type, block)]

    @staticmethod
    def empty(batch_size: int) -> "BatchedPerturbationConfig":
        return BatchedPerturbationConfig([PerturbationConfig.empty() for _ in range(batch_size)])


def stg_perturbation(stg_blocks: Optional[List[int]], stg_mode: str, num_layers: int) -> PerturbationConfig:
    """The perturbation of the STG row for ``--stg-blocks`` / ``--stg-mode``.  ``stg_blocks=None``: every block.  ``stg_av``
    perturbs the video and the audio self-attention upstream; this model has no audio branch, so it acts as ``stg_v``."""
    if stg_mode not in ("stg_v", "stg_av"):
        raise ValueError(f"Unknown stg_mode: {stg_mode!r} (expected 'stg_v' or 'stg_av')")
    if stg_blocks is not None:
        stg_blocks = [int(b) for b in stg_blocks]
        if not stg_blocks:
            raise ValueError("stg_blocks is empty: name at least one block, or pass None for every block")
        bad = [b for b in stg_blocks if not 0 <= b < num_layers]
        if bad:
            raise ValueError(f"stg_blocks {bad} are outside [0, {num_layers})")
    types = [PerturbationType.SKIP_VIDEO_SELF_ATTN]
    if stg_mode == "stg_av":
        types.append(PerturbationType.SKIP_AUDIO_SELF_ATTN)
    return PerturbationConfig([Perturbation(t, stg_blocks) for t in types])
