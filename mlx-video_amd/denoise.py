"""Denoise loops: ``denoise_dev`` (CFG) and ``denoise_distilled`` (mlx_video/generate.py:1060-1327,
564-881), video branch, ``denoise_audio_only`` (888-1053), the loop of separate audio
generation, and ``denoise_dev_av`` (1330-1680), the dev loop of joint audio-video denoising over
``av_model.LTXAVModel``.  The step body is: tokens <- latent transpose, DiT forward(s), then one
fused kernel for guidance + x0 + mask blend + Euler (ops.step_tail).

Sigma handling follows the reference exactly (SURVEY.md §7 "bf16-quantised timesteps"):
timesteps = bf16(sigma)*mask always (generate.py:1084,1237); with ``compile_step`` x0 and Euler
use the bf16-rounded sigma (1160-1174), without it x0 uses bf16(sigma) and Euler the Python
float (1288,1293-1301).  ``fp32_euler=False`` (LTX_FP32_EULER=0) only changes the compiled
distilled step (generate.py:741-748): the Euler update then runs op by op in bf16."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .conditioning import LatentState
from .guidance import BatchedPerturbationConfig, GuiderConfig, PerturbationConfig, stg_perturbation
from .ltx_model import ContextKV, LTXModel, TimestepPlan, precompute_freqs_cis

BF16 = torch.bfloat16
GRAPH_MAX_STEPS = 256        # rows of the per-step scalar tables a captured step graph reads


def _bf16_round(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32).to(BF16).to(torch.float32))


class _StepPlan:
    """Per-call constants: the U distinct values of the (per-frame) denoise mask, the token -> row map,
    and the per-step scalar tables {timestep values, sigma, sigma_next}."""

    def __init__(self, latents: torch.Tensor, state: Optional[LatentState], batch_rep: int, sig: Sequence[float]):
        b, c, f, h, w = latents.shape
        n = f * h * w
        dev = latents.device
        if state is not None:
            m = state.denoise_mask.reshape(b, 1, f, 1, 1).to(BF16)
            mask_tok = m.expand(b, 1, f, h, w).reshape(b, n)
        else:
            mask_tok = torch.ones((b, n), dtype=BF16, device=dev)
        vals, inv = torch.unique(mask_tok.reshape(-1), sorted=True, return_inverse=True)
        self.mask_vals = vals.to(torch.float32).cpu().tolist()        # U distinct mask values (host)
        self.U = len(self.mask_vals)
        self.tok2row = inv.to(torch.int32).repeat(batch_rep).contiguous()
        self.mask_tok_f32 = mask_tok.to(torch.float32).contiguous() if state is not None else None
        self.clean = state.clean_latent.to(BF16).contiguous() if state is not None else None
        self.dev = dev
        # timesteps = bf16(sigma) * mask as a bf16 multiply (generate.py:1084,1237): one value per distinct mask entry
        nst = len(sig) - 1
        self.sig_bf = [_bf16_round(s) for s in sig]
        ts = torch.tensor([[self.sig_bf[i] * mv for mv in self.mask_vals] for i in range(nst)], dtype=torch.float32).to(BF16)
        self.ts_host = ts.reshape(nst, self.U)
        self.sig_host = torch.tensor([[self.sig_bf[i], self.sig_bf[i + 1]] for i in range(nst)], dtype=torch.float32).reshape(nst, 2)
        self._ts_dev: Optional[torch.Tensor] = None

    def timestep_plan(self, i: int) -> TimestepPlan:
        if self._ts_dev is None:
            self._ts_dev = self.ts_host.to(self.dev)              # one upload per call; rows are views
        return TimestepPlan(self._ts_dev[i], self.tok2row)


class _Guidance:
    """What one step evaluates: the positive forward, the negative one (CFG, cfg_scale != 1) and the perturbed one (STG,
    stg_scale != 0), either as separate forwards or - ``batched`` (cfg_batch) - as one forward over the rows
    [pos | neg | pos+], each block of ``b`` rows.  ``guider``: the x0-space guider of the CFG slot when it is not plain CFG
    (``cfg_star`` / ``apg``; None otherwise, and at cfg_scale == 1, where every guider is disabled)."""

    def __init__(self, b: int, cfg_scale: float, cfg_batch: bool, stg_scale: float, pert: Optional[PerturbationConfig],
                 guider: Optional[GuiderConfig] = None):
        self.b = b
        self.use_cfg = cfg_scale != 1.0
        self.guider = guider if (guider is not None and not guider.is_default and self.use_cfg) else None
        self.use_stg = pert is not None
        self.cfg_scale, self.stg_scale = float(cfg_scale), float(stg_scale)
        self.batched = bool(cfg_batch) and (self.use_cfg or self.use_stg)
        self.reps = (1 + self.use_cfg + self.use_stg) if self.batched else 1
        # the batched forward perturbs its last b rows; the separate perturbed forward all of its b rows
        self.pert_batched = BatchedPerturbationConfig([PerturbationConfig.empty()] * ((self.reps - 1) * b) + [pert] * b) \
            if self.use_stg and self.batched else None
        self.pert_alone = BatchedPerturbationConfig([pert] * b) if self.use_stg and not self.batched else None

    def context_rows(self, ctx_pos, ctx_neg):
        """The contexts of the batched forward's rows, in row order."""
        return [ctx_pos] + ([ctx_neg] if self.use_cfg else []) + ([ctx_pos] if self.use_stg else [])

    def velocities(self, tr: LTXModel, lat, tp, pe, ctx_rows, kv_rows, ctx_pos, kv_pos, ctx_neg, kv_neg):
        """(v_pos, v_neg | None, v_pert | None) of one step.  ``ctx_rows``/``kv_rows``: the batched forward's context (and its
        ContextKV or None); ``ctx_pos``/``kv_pos``, ``ctx_neg``/``kv_neg``: those of the separate forwards."""
        b = self.b
        if self.batched:
            v = tr.forward_tokens(ops.latent_to_tokens(lat, rep=self.reps), tp, ctx_rows, pe, kv_rows,
                                  perturbations=self.pert_batched)
            v_neg = v[b:2 * b] if self.use_cfg else None
            v_pert = v[(self.reps - 1) * b:] if self.use_stg else None
            return v[:b], v_neg, v_pert
        tok = ops.latent_to_tokens(lat, rep=1)
        v_pos = tr.forward_tokens(tok, tp, ctx_pos, pe, kv_pos)
        v_neg = tr.forward_tokens(tok, tp, ctx_neg, pe, kv_neg) if self.use_cfg else None
        v_pert = tr.forward_tokens(tok, tp, ctx_pos, pe, kv_pos, perturbations=self.pert_alone) if self.use_stg else None
        return v_pos, v_neg, v_pert

    def tail(self, v_pos, v_neg, v_pert, latents, s, s_next, clean, mask_tok, out=None, sigmas_dev=None, bf16_euler=False,
             record=None, workspace=None):
        kw = {}
        g = self.guider
        if g is not None:             # cfg_star / apg: the reduction launch(es) into the device record the tail reads
            record = ops.guidance_sums(v_pos, v_neg, latents, g.kind, s, g.norm_threshold, record=record, workspace=workspace,
                                       sigmas_dev=sigmas_dev)
            kw = dict(guider=g.kind, record=record, eta=g.eta, norm_threshold=g.norm_threshold)
        return ops.step_tail(v_pos, v_neg, v_pert, latents, cfg_scale=self.cfg_scale, stg_scale=self.stg_scale, sigma=s,
                             sigma_next=s_next, clean=clean, mask_tok=mask_tok, out=out, sigmas_dev=sigmas_dev,
                             bf16_euler=bf16_euler, **kw)


class StepCache:
    """A timestep-aware step cache (TeaCache) for ``denoise_dev`` / ``denoise_distilled``: a step whose input to block 0 has
    barely moved since the step before skips the transformer blocks and adds the residual (x behind the last block minus x in
    front of block 0) of the last computed step instead.  Opt-in, not in the reference.

    One object serves one denoise call at a time; a call resets it and leaves ``report``.  The measure is m_i, block 0's
    modulated self-attention input of the positive rows at step i; the device returns S_d = sum |m_i - m_(i-1)| and
    S_p = sum |m_(i-1)| (ops.step_cache_probe), the host decides (``decide``).  A step has ONE decision, shared by its
    forwards; with b > 1 samples it is joint over them (the sums run over all b positive rows), so a sample's result then
    depends on its batch - with b = 1 it is the sample's own.  Each forward (pos, neg, pos+; or the one batched forward) keeps
    a residual of its own.  ``threshold`` tau >= 0: 0 never skips, inf skips every step but the first and the last.
    ``coefficients``: the polynomial applied to rel = S_d / S_p before it is accumulated, highest degree first
    (numpy.poly1d); the default (1, 0) is the identity, not a calibrated fit.  ``schedule``: a list of booleans, True =
    compute, one per step, that overrides the policy (the probe still runs and reports); its first entry must be True.
    ``report``: per step {"rel", "acc", "computed", "s_d", "s_p"}; step 0 has no distance (None); "acc" is the accumulator the
    decision compared with tau, before its reset."""

    def __init__(self, threshold: float, coefficients: Sequence[float] = (1.0, 0.0), schedule: Optional[Sequence[bool]] = None):
        threshold = float(threshold)
        if not threshold >= 0.0:
            raise ValueError(f"StepCache: threshold = {threshold} must be >= 0")
        coefficients = tuple(float(c) for c in coefficients)
        if not coefficients or not all(math.isfinite(c) for c in coefficients):
            raise ValueError(f"StepCache: coefficients = {coefficients} must be one or more finite numbers, highest degree first")
        if schedule is not None:
            schedule = [bool(s) for s in schedule]
            if not schedule or not schedule[0]:
                raise ValueError("StepCache: schedule must start with a computed step (there is no residual before it)")
        self.threshold, self.coefficients, self.schedule = threshold, coefficients, schedule
        self.report: List[dict] = []
        self._acc = 0.0
        self._n = 0

    @staticmethod
    def decide(i: int, n: int, s_d: Optional[float], s_p: Optional[float], acc: float, threshold: float,
               coefficients: Sequence[float] = (1.0, 0.0)) -> Tuple[bool, float, Optional[float]]:
        """The policy, a pure host function in Python floats: (compute, acc compared with the threshold, rel) of step ``i`` of
        ``n`` given the two sums and the accumulator ``acc`` carried into the step (0 after a computed step).  Step 0 and step
        n - 1 are computed.  Otherwise rel = s_d / s_p, acc += poly(rel) by Horner, compute = not (acc < threshold).
        s_p == 0 or a sum that is not finite: compute."""
        if i == 0:
            return True, 0.0, None
        if s_d is None or s_p is None or not (math.isfinite(s_d) and math.isfinite(s_p)) or s_p == 0.0:
            return True, 0.0, None
        rel = s_d / s_p
        if i == n - 1:
            return True, 0.0, rel
        p = 0.0
        for c in coefficients:
            p = p * rel + c
        acc = acc + p
        return (not acc < threshold), acc, rel

    def reset(self, n: int) -> None:
        if self.schedule is not None and len(self.schedule) != n:
            raise ValueError(f"StepCache: schedule has {len(self.schedule)} entries, the call {n} steps")
        self.report, self._acc, self._n = [], 0.0, n

    def step(self, i: int, s_d: Optional[float], s_p: Optional[float]) -> bool:
        """Record step ``i`` with its sums (None at step 0) and return whether it is computed."""
        compute, acc, rel = self.decide(i, self._n, s_d, s_p, self._acc, self.threshold, self.coefficients)
        if self.schedule is not None:
            compute = self.schedule[i]
        self.report.append({"rel": rel, "acc": acc, "computed": compute, "s_d": s_d, "s_p": s_p})
        self._acc = 0.0 if compute else acc
        return compute

    @property
    def counts(self) -> Dict[str, int]:
        c = sum(1 for r in self.report if r["computed"])
        return {"steps": len(self.report), "computed": c, "skipped": len(self.report) - c}


class _CachedForwards:
    """The forwards of one step under a step cache, cut in three: ``prepare`` (every forward's part in front of block 0),
    ``probe`` (m_i of the first forward's positive rows, the two sums, prev <- m_i) and ``finish`` (per forward the blocks
    and the residual store, or the residual apply; then the head).  Owns what outlives a step: prev, the probe's buffers
    and one residual per forward."""

    def __init__(self, gd: _Guidance, tr: LTXModel, b: int, n_tok: int, dev):
        self.gd, self.tr = gd, tr
        D = tr.inner_dim
        self.rows = b * n_tok
        nf = 1 if gd.batched else 1 + gd.use_cfg + gd.use_stg
        self.resid = [torch.empty((gd.reps * self.rows, D), dtype=BF16, device=dev) for _ in range(nf)]
        self.m = torch.empty((self.rows, D), dtype=BF16, device=dev)
        self.prev = torch.zeros_like(self.m)
        self.sums = torch.zeros((2,), dtype=torch.float32, device=dev)
        self.ws = torch.empty((ops.step_cache_workspace_bytes(self.rows, D) // 4,), dtype=torch.float32, device=dev)

    def prepare(self, lat, tp, pe, ctx_rows, kv_rows, ctx_pos, kv_pos, ctx_neg, kv_neg) -> list:
        gd, tr = self.gd, self.tr
        if gd.batched:
            return [tr._fwd_prepare(ops.latent_to_tokens(lat, rep=gd.reps), tp, ctx_rows, pe, kv_rows, gd.pert_batched)]
        tok = ops.latent_to_tokens(lat, rep=1)
        sts = [tr._fwd_prepare(tok, tp, ctx_pos, pe, kv_pos, None)]
        if gd.use_cfg:
            sts.append(tr._fwd_prepare(tok, tp, ctx_neg, pe, kv_neg, None))
        if gd.use_stg:
            sts.append(tr._fwd_prepare(tok, tp, ctx_pos, pe, kv_pos, gd.pert_alone))
        return sts

    def probe(self, sts: list, init: bool) -> None:
        self.tr.step_cache_input(sts[0], self.rows, self.m)
        ops.step_cache_probe(self.m, self.prev, self.sums, self.ws, init=init)

    def finish(self, sts: list, compute: bool):
        gd, b = self.gd, self.gd.b
        vs = [self.tr.forward_cached(st, r, compute) for st, r in zip(sts, self.resid)]
        if gd.batched:
            v = vs[0]
            return v[:b], (v[b:2 * b] if gd.use_cfg else None), (v[(gd.reps - 1) * b:] if gd.use_stg else None)
        return vs[0], (vs[1] if gd.use_cfg else None), (vs[-1] if gd.use_stg else None)


def _refuse_step_cache(step_cache, who: str) -> None:
    if step_cache is not None:
        raise ValueError(f"{who} does not take a step cache (step_cache): it is part of denoise_dev and denoise_distilled only")


def _denoise(latents: torch.Tensor, positions: torch.Tensor, ctx_pos_in: torch.Tensor, ctx_neg_in: Optional[torch.Tensor],
             transformer: LTXModel, sig: List[float], cfg_scale: float, state: Optional[LatentState], compile_step: bool,
             cfg_batch: bool, use_graph: bool, graph_cache: Optional[dict], cache_context: bool, bf16_euler: bool,
             stg_scale: float = 0.0, stg_pert: Optional[PerturbationConfig] = None, stg_key: tuple = (),
             guider: Optional[GuiderConfig] = None, step_cache: Optional[StepCache] = None) -> torch.Tensor:
    if step_cache is not None and not isinstance(step_cache, StepCache):
        raise TypeError(f"step_cache must be a StepCache or None, got {type(step_cache).__name__}")
    if state is not None:
        latents = state.latent
    latents = latents.to(BF16).contiguous()
    use_cfg = cfg_scale != 1.0
    bf16_euler = bf16_euler and compile_step          # the eager body always updates in fp32 (generate.py:835-849)
    if step_cache is not None:
        step_cache.reset(max(len(sig) - 1, 0))
        # a skipped step must not pay for the text K | V^T of blocks it never runs: the text-only part is prepared once per
        # call - the same bits, it is a function of the context alone
        cache_context = True
    if len(sig) < 2:
        return latents
    b = latents.shape[0]
    gd = _Guidance(b, cfg_scale, cfg_batch, stg_scale, stg_pert, guider)
    pe = precompute_freqs_cis(positions[:1].contiguous(), transformer.inner_dim, transformer.positional_embedding_theta,
                              transformer.positional_embedding_max_pos, transformer.num_attention_heads)
    plan = _StepPlan(latents, state, gd.reps, sig)
    ctx_pos = ctx_pos_in.to(BF16).contiguous()
    ctx_neg = ctx_neg_in.to(BF16).contiguous() if use_cfg else None
    if use_graph and compile_step and len(sig) - 1 <= GRAPH_MAX_STEPS:
        key = (tuple(latents.shape), bool(gd.batched), bool(use_cfg), float(cfg_scale), tuple(ctx_pos.shape), id(transformer),
               state is not None, plan.U, bool(bf16_euler), bool(cache_context))
        if gd.use_stg:                # STG off: today's key
            key = key + stg_key
        if gd.guider is not None:     # plain CFG: today's key
            key = key + ("guider",) + gd.guider.key
        if step_cache is not None:    # no step cache: today's key.  (The policy runs on the host: one capture serves every
            key = key + ("step_cache",)                               # threshold, polynomial and schedule)
        cache = graph_cache if graph_cache is not None else {}
        ent = cache.get(key)
        if ent is None:
            ent = _StepGraph(latents, plan, transformer, ctx_pos, gd, bf16_euler, cache_context, cached=step_cache is not None)
            cache[key] = ent
        return ent.run(latents, plan, ctx_pos, ctx_neg, pe, step_cache)
    ctx_cat = torch.cat(gd.context_rows(ctx_pos, ctx_neg), 0).contiguous() if gd.batched else None
    kv_pos = kv_neg = kv_cat = None
    if cache_context:
        if gd.batched:
            kv_cat = transformer.prepare_context(ctx_cat)
        else:
            kv_pos = transformer.prepare_context(ctx_pos)
            kv_neg = transformer.prepare_context(ctx_neg) if use_cfg else None
    cf = None
    if step_cache is not None:
        cf = _CachedForwards(gd, transformer, b, latents.numel() // (b * latents.shape[1]), latents.device)
    for i in range(len(sig) - 1):
        s_bf, sn_bf = plan.sig_bf[i], plan.sig_bf[i + 1]
        tp = plan.timestep_plan(i)
        if cf is None:
            v_pos, v_neg, v_pert = gd.velocities(transformer, latents, tp, pe, ctx_cat, kv_cat, ctx_pos, kv_pos, ctx_neg, kv_neg)
        else:       # one prepare per forward, the probe, one host read of the two sums, then either branch
            sts = cf.prepare(latents, tp, pe, ctx_cat, kv_cat, ctx_pos, kv_pos, ctx_neg, kv_neg)
            cf.probe(sts, init=i == 0)
            v_pos, v_neg, v_pert = cf.finish(sts, step_cache.step(i, *(cf.sums.tolist() if i else (None, None))))
        # x0 uses the bf16 sigma in both paths; Euler: bf16 sigmas if compiled else Python floats.
        # The fused kernel takes one sigma for x0 and the ratio terms; when they differ (eager path)
        # x0 and Euler run as two launches.
        if compile_step or (s_bf == sig[i] and sn_bf == sig[i + 1]):
            latents = gd.tail(v_pos, v_neg, v_pert, latents, s_bf, sn_bf, plan.clean, plan.mask_tok_f32, bf16_euler=bf16_euler)
        else:
            latents = _eager_tail(gd, v_pos, v_neg, v_pert, latents, s_bf, sig[i], sig[i + 1], plan)
    return latents


def denoise_dev(latents: torch.Tensor, positions: torch.Tensor, text_embeddings_pos: torch.Tensor,
                text_embeddings_neg: torch.Tensor, transformer: LTXModel, sigmas: torch.Tensor,
                cfg_scale: float = 4.0, verbose: bool = False, state: Optional[LatentState] = None,
                eval_interval: int = 1, compile_step: bool = False, compile_shapeless: bool = False,
                cfg_batch: bool = False, ui_phase: str = "denoise", use_graph: bool = False,
                graph_cache: Optional[dict] = None, cache_context: bool = False, stg_scale: float = 0.0,
                stg_blocks: Optional[Sequence[int]] = None, stg_mode: str = "stg_v", guider: str = "cfg",
                apg_eta: float = 1.0, apg_norm_threshold: float = 0.0, step_cache: Optional[StepCache] = None) -> torch.Tensor:
    """generate.py:1060-1327.  latents (B,128,F,H,W) bf16 on the GPU; returns the same shape.
    ``use_graph``: capture the whole step (forward(s) + fused tail, ~1000 launches) once as a hipGraph and
    replay it per step — the analogue of the reference's mx.compile'd step_fn (generate.py:1109-1177);
    requires compile_step semantics (bf16 sigmas) and gives bit-identical results to the eager path.
    ``graph_cache`` (a dict owned by the caller) keeps the captured graph across calls of the same geometry,
    like a compiled function that is traced once: the graph owns persistent copies of every per-call input
    (latents, contexts, clean latent, mask, token->row map, RoPE table) and each call REFRESHES them, so a new
    prompt / mask / conditioning never sees stale data whatever addresses the new tensors happen to get.
    ``cache_context``: compute the text-only part of the forward (caption projection, cross-attention K/V)
    once per call instead of every step — an algorithmic change relative to the reference.
    ``stg_scale`` != 0 turns on spatio-temporal guidance (STG, upstream LTX-2's STGGuider): every step also evaluates the
    positive prompt with the video self-attention of ``stg_blocks`` skipped (each returns its value projection; None = every
    block) and pushes the guided velocity away from that prediction by ``stg_scale`` (ltxk_guided_euler_step; DESIGN.md
    "Spatio-temporal guidance").  With ``cfg_batch`` the three predictions are one B=3 forward [pos, neg, pos+] ([pos, pos+]
    when cfg_scale == 1); without it a third forward.  ``stg_mode``: "stg_v" or "stg_av"; the latter also perturbs the
    audio self-attention upstream, and as this model has no audio branch it acts as "stg_v".  ``stg_blocks`` that is
    empty or names a block outside [0, num_layers) is a ValueError.  stg_scale == 0: no STG, today's loop bit for bit.
    ``guider``: what the CFG slot runs - "cfg" (default: today's fused velocity-space tail, launch for launch), "cfg_star"
    (CFGStarRescalingGuider) or "apg" (LtxAPGGuider with ``apg_eta`` and ``apg_norm_threshold``, 0 = no clamp); the latter two act
    in x0 space on per-sample dot products that stay on the device (ltxk_guidance_sums + ltxk_guider_euler_step, DESIGN.md
    §5j), compose with STG, and are disabled at cfg_scale == 1 like CFG itself.
    ``step_cache``: a ``StepCache`` - steps whose input to block 0 has barely moved skip the transformer blocks and reuse the
    last computed step's residual; it implies ``cache_context`` (same bits: the text side is a function of the
    context alone).  None: today's loop, branch for branch."""
    gcfg = GuiderConfig(guider, apg_eta, apg_norm_threshold)
    stg_scale = float(stg_scale or 0.0)
    pert = stg_perturbation(stg_blocks, stg_mode, transformer.config.num_layers) if stg_scale != 0.0 else None
    stg_key = (stg_scale, None if stg_blocks is None else tuple(int(x) for x in stg_blocks), stg_mode)
    sig = [float(s) for s in (sigmas.tolist() if torch.is_tensor(sigmas) else sigmas)]
    return _denoise(latents, positions, text_embeddings_pos, text_embeddings_neg, transformer, sig, cfg_scale, state,
                    compile_step, cfg_batch, use_graph, graph_cache, cache_context, False, stg_scale, pert, stg_key, gcfg,
                    step_cache)


class _StepInputs:
    """The persistent per-call inputs of a captured step: the buffers the captured kernels read (latents, clean latent, mask,
    token -> row map, RoPE table, the per-step scalar tables and the device-side step counter), refreshed by ``load``."""

    def __init__(self, latents, plan: _StepPlan):
        dev = latents.device
        self.lat_buf = torch.empty_like(latents)
        self.clean = torch.empty_like(plan.clean) if plan.clean is not None else None
        self.mask_tok = torch.empty_like(plan.mask_tok_f32) if plan.mask_tok_f32 is not None else None
        self.tok2row = torch.empty_like(plan.tok2row)
        self.pe: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self.ts_all = torch.zeros((GRAPH_MAX_STEPS, plan.U), dtype=BF16, device=dev)
        self.sig_all = torch.zeros((GRAPH_MAX_STEPS, 2), dtype=torch.float32, device=dev)
        self.step = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.ts_buf = torch.zeros((plan.U,), dtype=BF16, device=dev)
        self.sig_buf = torch.zeros((2,), dtype=torch.float32, device=dev)

    def load(self, latents, plan: _StepPlan, pe) -> None:
        """Refresh every buffer from this call's inputs and rewind the step counter."""
        self.lat_buf.copy_(latents)
        if self.clean is not None:
            self.clean.copy_(plan.clean)
            self.mask_tok.copy_(plan.mask_tok_f32)
        self.tok2row.copy_(plan.tok2row)
        cos, sin = pe
        if self.pe is None:
            self.pe = (cos.clone(), sin.clone())
        else:
            self.pe[0].copy_(cos)
            self.pe[1].copy_(sin)
        nst = plan.ts_host.shape[0]
        self.ts_all[:nst].copy_(plan.ts_host)
        self.sig_all[:nst].copy_(plan.sig_host)
        self.step.zero_()

    def next_step(self) -> TimestepPlan:
        """The ltxk_step_scalars node: this step's timestep values -> ``ts_buf``, {sigma, sigma_next} -> ``sig_buf``, and the
        device-side step counter advances."""
        ops.step_scalars(self.ts_all, self.sig_all, self.step, self.ts_buf, self.sig_buf)
        return TimestepPlan(self.ts_buf, self.tok2row)


class _StepGraph:
    """One denoise step as a hipGraph.  First node: ltxk_step_scalars, which reads this step's {timestep values,
    sigma, sigma_next} from device tables and advances a device-side step counter — so the schedule runs as bare
    graph replays with no host->device traffic in between; the fused tail updates the latents in place.  The
    first step of the first run executes eagerly (it doubles as the warm-up torch requires before capture:
    allocator, lazy hipFuncSetAttribute calls), then the step is captured and every later step is a replay."""

    def __init__(self, latents, plan: _StepPlan, transformer: LTXModel, ctx_pos, gd: _Guidance, bf16_euler, cache_context,
                 cached: bool = False):
        dev = latents.device
        # step cache: the step is three graphs - probe, full body, skip body - and the host picks a body per step (_run_cached)
        bb, cc = latents.shape[:2]
        self.cf = _CachedForwards(gd, transformer, bb, latents.numel() // (bb * cc), dev) if cached else None
        self.sts: Optional[list] = None
        self.g_probe = self.g_full = self.g_skip = None
        self.tr = transformer                       # strong reference: id(transformer) in the cache key stays unique
        self.gd, self.bf16_euler = gd, bf16_euler
        self.inp = _StepInputs(latents, plan)
        # the batched forward's rows pos (| neg) (| pos+); unbatched: pos, and neg for CFG
        self.ctx_a = torch.empty((gd.reps * ctx_pos.shape[0],) + tuple(ctx_pos.shape[1:]), dtype=BF16, device=dev)
        self.ctx_b = torch.empty_like(ctx_pos) if (gd.use_cfg and not gd.batched) else None
        self.kv_a: Optional[ContextKV] = None
        self.kv_b: Optional[ContextKV] = None
        self.cache_context = cache_context
        # cfg_star / apg: the sums record and the partials workspace, persistent so that the captured launches keep their addresses
        self.g_rec = self.g_ws = None
        if gd.guider is not None:
            bb, cc = latents.shape[:2]
            self.g_rec = torch.zeros((bb, ops.GUIDER_RECORD_FLOATS), dtype=torch.float32, device=dev)
            self.g_ws = torch.zeros((ops.guidance_sums_workspace_bytes(bb, cc, latents.numel() // (bb * cc)) // 4,),
                                    dtype=torch.float32, device=dev)
        self.graph = None

    def _load(self, latents, plan: _StepPlan, ctx_pos, ctx_neg, pe) -> None:
        """Refresh every per-call input in the buffers the captured kernels read."""
        self.inp.load(latents, plan, pe)
        if self.gd.batched:
            n = ctx_pos.shape[0]
            for r, c in enumerate(self.gd.context_rows(ctx_pos, ctx_neg)):
                self.ctx_a[r * n:(r + 1) * n].copy_(c)
        else:
            self.ctx_a.copy_(ctx_pos)
            if self.ctx_b is not None:
                self.ctx_b.copy_(ctx_neg)
        if self.cache_context:
            self.kv_a = self.tr.prepare_context(self.ctx_a, out=self.kv_a)
            if self.ctx_b is not None:
                self.kv_b = self.tr.prepare_context(self.ctx_b, out=self.kv_b)

    def _step(self):
        gd, inp = self.gd, self.inp
        tp = inp.next_step()
        if gd.batched:
            v_pos, v_neg, v_pert = gd.velocities(self.tr, inp.lat_buf, tp, inp.pe, self.ctx_a, self.kv_a, None, None, None, None)
        else:
            v_pos, v_neg, v_pert = gd.velocities(self.tr, inp.lat_buf, tp, inp.pe, None, None, self.ctx_a, self.kv_a,
                                                 self.ctx_b, self.kv_b)
        gd.tail(v_pos, v_neg, v_pert, inp.lat_buf, 1.0, 0.0, inp.clean, inp.mask_tok, out=inp.lat_buf, sigmas_dev=inp.sig_buf,
                bf16_euler=self.bf16_euler, record=self.g_rec, workspace=self.g_ws)

    # --- step cache: probe | full | skip.  What crosses from one graph to another - the forwards' _Fwd states (self.sts), prev,
    # the residuals, the sums - is either allocated before the captures (self.cf) or referenced from here across all three
    # captures of one shared pool, so no later capture is handed its memory.  One stream, no parallel branches.
    def _prepare_probe(self, init: bool) -> list:
        gd, inp, cf = self.gd, self.inp, self.cf
        tp = inp.next_step()
        if gd.batched:
            sts = cf.prepare(inp.lat_buf, tp, inp.pe, self.ctx_a, self.kv_a, None, None, None, None)
        else:
            sts = cf.prepare(inp.lat_buf, tp, inp.pe, None, None, self.ctx_a, self.kv_a, self.ctx_b, self.kv_b)
        cf.probe(sts, init)
        return sts

    def _body(self, sts: list, compute: bool) -> None:
        gd, inp = self.gd, self.inp
        v_pos, v_neg, v_pert = self.cf.finish(sts, compute)
        gd.tail(v_pos, v_neg, v_pert, inp.lat_buf, 1.0, 0.0, inp.clean, inp.mask_tok, out=inp.lat_buf, sigmas_dev=inp.sig_buf,
                bf16_euler=self.bf16_euler, record=self.g_rec, workspace=self.g_ws)

    def _run_cached(self, nst: int, sc: StepCache) -> torch.Tensor:
        cf, start = self.cf, 0
        if self.g_probe is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._body(self._prepare_probe(init=True), True)     # real step 0, eager: prev <- m_0, the first residuals
                # the launches the captures would otherwise see first: the skip body's add and the probe's merge, on scratch
                scratch = torch.zeros((2, 1, 8), dtype=BF16, device=self.inp.lat_buf.device)
                ops.residual_apply(scratch[0], scratch[1])
                ops.step_cache_probe(scratch[0], scratch[1], torch.zeros_like(cf.sums), torch.zeros_like(cf.sums))
            torch.cuda.current_stream().wait_stream(side)
            sc.step(0, None, None)
            pool = torch.cuda.graph_pool_handle()
            self.g_probe, self.g_full, self.g_skip = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_probe, pool=pool, capture_error_mode="thread_local"):
                self.sts = self._prepare_probe(init=False)
            with torch.cuda.graph(self.g_full, pool=pool, capture_error_mode="thread_local"):
                self._body(self.sts, True)
            with torch.cuda.graph(self.g_skip, pool=pool, capture_error_mode="thread_local"):
                self._body(self.sts, False)
            start = 1
        for i in range(start, nst):
            self.g_probe.replay()
            # step 0 of a later call: the replayed probe has compared m_0 with the last call's prev; its sums are not read
            compute = sc.step(i, *(cf.sums.tolist() if i else (None, None)))
            (self.g_full if compute else self.g_skip).replay()
        return self.inp.lat_buf.clone()

    def run(self, latents, plan: _StepPlan, ctx_pos, ctx_neg, pe, step_cache: Optional[StepCache] = None) -> torch.Tensor:
        self._load(latents, plan, ctx_pos, ctx_neg, pe)
        nst = plan.ts_host.shape[0]
        if self.cf is not None:       # (the host's cache state was rewound by StepCache.reset; prev is rewritten by step 0)
            return self._run_cached(nst, step_cache)
        start = 0
        if self.graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._step()                              # real step 0, eager (device step counter 0 -> 1)
            torch.cuda.current_stream().wait_stream(side)
            # thread_local: a process-group watchdog thread (RCCL, N > 1) polling its events must not invalidate the capture
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self._step()
            start = 1
        for _ in range(start, nst):
            self.graph.replay()
        return self.inp.lat_buf.clone()


def _eager_tail(gd: _Guidance, v_pos, v_neg, v_pert, latents, s_bf, s, s_next, plan):
    """generate.py:1283-1301: x0 = x - bf16(sigma)*v (rounded to bf16), then fp32 Euler with the
    un-rounded Python-float sigmas."""
    x0 = gd.tail(v_pos, v_neg, v_pert, latents, s_bf, 0.0, plan.clean, plan.mask_tok_f32)
    if s_next <= 0:
        return x0
    return ops.euler_only(latents, x0, s, s_next)


def denoise_distilled(latents: torch.Tensor, positions: torch.Tensor, text_embeddings: torch.Tensor,
                      transformer: LTXModel, sigmas: Sequence[float], verbose: bool = False,
                      state: Optional[LatentState] = None, audio_latents=None, audio_positions=None,
                      audio_embeddings=None, eval_interval: int = 1, compile_step: bool = False,
                      compile_shapeless: bool = False, fp32_euler: bool = True,
                      ui_phase: str = "denoise", use_graph: bool = False, graph_cache: Optional[dict] = None,
                      cache_context: bool = False, step_cache: Optional[StepCache] = None) -> Tuple[torch.Tensor, None]:
    """generate.py:564-881, video branch (no CFG).  ``fp32_euler=False`` selects the bf16 Euler update of the
    compiled step (generate.py:741-748); the un-compiled loop body always updates in fp32 (835-849).
    ``step_cache``: a ``StepCache``, as in ``denoise_dev`` (implies ``cache_context``); None: today's loop."""
    if audio_latents is not None:
        raise ValueError("audio latents are not supported: the audio branch is out of scope (SURVEY.md §2a #3)")
    sig = [float(s) for s in (sigmas.tolist() if torch.is_tensor(sigmas) else sigmas)]
    out = _denoise(latents, positions, text_embeddings, None, transformer, sig, 1.0, state, compile_step, False,
                   use_graph, graph_cache, cache_context, not fp32_euler, step_cache=step_cache)
    return out, None


def audio_latent_to_volume(audio_latents: torch.Tensor) -> torch.Tensor:
    """(B,8,T,16) audio latents as the (B,128,T,1,1) volume the video loop takes, channel c*16 + f: its token view
    (ops.latent_to_tokens) is then the reference's transpose(0,2,1,3).reshape(B,T,128) (generate.py:936-937)."""
    b, c, t, f = audio_latents.shape
    return audio_latents.permute(0, 1, 3, 2).reshape(b, c * f, t, 1, 1).contiguous()


def audio_volume_to_latent(volume: torch.Tensor, channels: int = 8) -> torch.Tensor:
    """The inverse of ``audio_latent_to_volume``: (B,128,T,1,1) -> (B,8,T,16)."""
    b, cf, t = volume.shape[:3]
    return volume.reshape(b, channels, cf // channels, t).permute(0, 1, 3, 2).contiguous()


class _AVStep:
    """One joint step over persistent or per-call operands: the AudioVideo forward(s) - one B = 2 forward under ``batched``, else
    the positive and (CFG) the negative one - and the two fused tails, video then audio."""

    def __init__(self, tr, gd: _Guidance):
        self.tr, self.gd = tr, gd

    def velocities(self, lat_v, vol_a, tp_v, tp_a, ctx_v, ctx_a, tables):
        """((video v_pos, v_neg | None), (audio v_pos, v_neg | None)).  ``ctx_v`` / ``ctx_a``: [batched rows] or [pos, neg]."""
        gd, b = self.gd, self.gd.b
        pe_v, cpe_v, pe_a, cpe_a = tables
        tok_v, tok_a = ops.latent_to_tokens(lat_v, rep=gd.reps), ops.latent_to_tokens(vol_a, rep=gd.reps)
        if gd.batched:
            vv, va = self.tr.forward_tokens(tok_v, tp_v, ctx_v[0], pe_v, cpe_v, tok_a, tp_a, ctx_a[0], pe_a, cpe_a)
            return (vv[:b], vv[b:2 * b]), (va[:b], va[b:2 * b])
        vp, ap = self.tr.forward_tokens(tok_v, tp_v, ctx_v[0], pe_v, cpe_v, tok_a, tp_a, ctx_a[0], pe_a, cpe_a)
        vn = an = None
        if gd.use_cfg:
            vn, an = self.tr.forward_tokens(tok_v, tp_v, ctx_v[1], pe_v, cpe_v, tok_a, tp_a, ctx_a[1], pe_a, cpe_a)
        return (vp, vn), (ap, an)


class _AVStepGraph:
    """The joint step as a hipGraph on one stream, ``_StepGraph``'s scheme: both modalities' persistent inputs (``_StepInputs``
    each, with its own ltxk_step_scalars node and device-side step counter), the contexts and the cross tables, refreshed by
    every call; step 0 of the first run is eager, then the step is captured once and replayed."""

    def __init__(self, lat_v, vol_a, plan_v: _StepPlan, plan_a: _StepPlan, transformer, ctx_v, ctx_a, gd: _Guidance):
        self.tr = transformer                       # strong reference: id(transformer) in the cache key stays unique
        self.step = _AVStep(transformer, gd)
        self.inp_v, self.inp_a = _StepInputs(lat_v, plan_v), _StepInputs(vol_a, plan_a)
        self.ctx_v = [torch.empty_like(c) for c in ctx_v]
        self.ctx_a = [torch.empty_like(c) for c in ctx_a]
        self.cross: Optional[list] = None
        self.graph = None

    def _load(self, lat_v, vol_a, plan_v, plan_a, ctx_v, ctx_a, tables) -> None:
        pe_v, cpe_v, pe_a, cpe_a = tables
        self.inp_v.load(lat_v, plan_v, pe_v)
        self.inp_a.load(vol_a, plan_a, pe_a)
        for dst, src in zip(self.ctx_v + self.ctx_a, list(ctx_v) + list(ctx_a)):
            dst.copy_(src)
        if self.cross is None:
            self.cross = [t.clone() for t in (*cpe_v, *cpe_a)]
        else:
            for dst, src in zip(self.cross, (*cpe_v, *cpe_a)):
                dst.copy_(src)

    def _step(self) -> None:
        iv, ia, gd = self.inp_v, self.inp_a, self.step.gd
        tables = (iv.pe, tuple(self.cross[:2]), ia.pe, tuple(self.cross[2:]))
        (vp, vn), (ap, an) = self.step.velocities(iv.lat_buf, ia.lat_buf, iv.next_step(), ia.next_step(), self.ctx_v, self.ctx_a, tables)
        gd.tail(vp, vn, None, iv.lat_buf, 1.0, 0.0, iv.clean, iv.mask_tok, out=iv.lat_buf, sigmas_dev=iv.sig_buf)
        gd.tail(ap, an, None, ia.lat_buf, 1.0, 0.0, None, None, out=ia.lat_buf, sigmas_dev=ia.sig_buf)

    def run(self, lat_v, vol_a, plan_v, plan_a, ctx_v, ctx_a, tables):
        self._load(lat_v, vol_a, plan_v, plan_a, ctx_v, ctx_a, tables)
        nst, start = plan_v.ts_host.shape[0], 0
        if self.graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._step()                              # real step 0, eager (device step counters 0 -> 1)
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self._step()
            start = 1
        for _ in range(start, nst):
            self.graph.replay()
        return self.inp_v.lat_buf.clone(), self.inp_a.lat_buf.clone()


def denoise_dev_av(video_latents: torch.Tensor, audio_latents: torch.Tensor, video_positions: torch.Tensor,
                   audio_positions: torch.Tensor, video_embeddings_pos: torch.Tensor, video_embeddings_neg: torch.Tensor,
                   audio_embeddings_pos: torch.Tensor, audio_embeddings_neg: torch.Tensor, transformer, sigmas,
                   cfg_scale: float = 4.0, verbose: bool = False, video_state: Optional[LatentState] = None,
                   eval_interval: int = 1, compile_step: bool = False, compile_shapeless: bool = False, cfg_batch: bool = False,
                   ui_phase: str = "denoise", use_graph: bool = False, graph_cache: Optional[dict] = None,
                   cache_context: bool = False, stg_scale: float = 0.0, stg_blocks: Optional[Sequence[int]] = None,
                   guider: str = "cfg", step_cache=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """generate.py:1330-1680: the dev loop of joint audio-video denoising over an ``av_model.LTXAVModel``.  video_latents
    (B,128,F,H,W), audio_latents (B,8,T,16), video_positions (B,3,N,2), audio_positions (B,1,T,2) seconds, one context pair per
    modality; returns (video latents, audio latents) in the shapes given.  Both modalities share sigma; the audio timestep mask
    is all ones; CFG combines each modality's velocities with its own context pair (``cfg_batch``: one B = 2 forward); x0 uses
    the bf16 sigma, Euler the Python floats, or the bf16 sigmas under ``compile_step`` - ``denoise_dev``'s rules, through the same
    fused tail: the audio latents travel as the (B,128,T,1,1) volume.  The video conditioning mask goes through ``video_state``.
    ``use_graph`` (with ``compile_step``): the whole joint step - forward(s) plus the two tails - captured once on one stream and
    replayed; ``graph_cache`` keeps it across calls, every per-call input refreshed.  STG, the cfg_star / apg guiders and
    ``cache_context`` and a step cache (``step_cache``) are not part of the joint loop: ValueError."""
    _refuse_step_cache(step_cache, "the joint audio-video loop (denoise_dev_av)")
    if float(stg_scale or 0.0) != 0.0 or stg_blocks is not None:
        raise ValueError("the joint audio-video loop does not do STG (stg_scale / stg_blocks); use denoise_dev for it")
    if guider != "cfg":
        raise ValueError(f"the joint audio-video loop does plain CFG only, not the {guider!r} guider (cfg_star / apg: denoise_dev)")
    if cache_context:
        raise ValueError("the joint audio-video loop recomputes the text side every step: cache_context is not part of it")
    sig = [float(s) for s in (sigmas.tolist() if torch.is_tensor(sigmas) else sigmas)]
    if video_state is not None:
        video_latents = video_state.latent
    if audio_latents.dim() != 4 or video_latents.dim() != 5 or audio_latents.shape[0] != video_latents.shape[0]:
        raise ValueError(f"video_latents must be (B,C,F,H,W) and audio_latents (B,C,T,F) of one batch, got {tuple(video_latents.shape)} "
                         f"and {tuple(audio_latents.shape)}")
    lat_v = video_latents.to(BF16).contiguous()
    ac = audio_latents.shape[1]
    vol_a = audio_latent_to_volume(audio_latents.to(BF16))
    if len(sig) < 2:
        return lat_v, audio_latents.to(BF16)
    b = lat_v.shape[0]
    V, A = transformer.video, transformer.audio
    use_cfg = cfg_scale != 1.0
    gd = _Guidance(b, cfg_scale, cfg_batch, 0.0, None, None)
    plan_v, plan_a = _StepPlan(lat_v, video_state, gd.reps, sig), _StepPlan(vol_a, None, gd.reps, sig)
    dev = lat_v.device
    vpos, apos = video_positions[:1].to(dev).contiguous(), audio_positions[:1].to(dev).contiguous()
    tables = (precompute_freqs_cis(vpos, V.inner_dim, V.positional_embedding_theta, V.positional_embedding_max_pos, V.num_attention_heads),
              transformer.cross_freqs_cis(vpos, V.num_attention_heads),
              precompute_freqs_cis(apos, A.inner_dim, A.positional_embedding_theta, A.positional_embedding_max_pos, A.num_attention_heads),
              transformer.cross_freqs_cis(apos, A.num_attention_heads))

    def contexts(pos, neg):
        pos = pos.to(BF16).contiguous()
        if not use_cfg:
            return [pos]
        neg = neg.to(BF16).contiguous()
        return [torch.cat([pos, neg], 0).contiguous()] if gd.batched else [pos, neg]

    ctx_v, ctx_a = contexts(video_embeddings_pos, video_embeddings_neg), contexts(audio_embeddings_pos, audio_embeddings_neg)
    if use_graph and compile_step and len(sig) - 1 <= GRAPH_MAX_STEPS:
        key = ("av", tuple(lat_v.shape), tuple(vol_a.shape), bool(gd.batched), bool(use_cfg), float(cfg_scale), tuple(ctx_v[0].shape),
               tuple(ctx_a[0].shape), id(transformer), video_state is not None, plan_v.U)
        cache = graph_cache if graph_cache is not None else {}
        ent = cache.get(key)
        if ent is None:
            ent = cache[key] = _AVStepGraph(lat_v, vol_a, plan_v, plan_a, transformer, ctx_v, ctx_a, gd)
        out_v, out_a = ent.run(lat_v, vol_a, plan_v, plan_a, ctx_v, ctx_a, tables)
        return out_v, audio_volume_to_latent(out_a, ac)
    step = _AVStep(transformer, gd)
    for i in range(len(sig) - 1):
        s_bf, sn_bf = plan_v.sig_bf[i], plan_v.sig_bf[i + 1]
        (vp, vn), (ap, an) = step.velocities(lat_v, vol_a, plan_v.timestep_plan(i), plan_a.timestep_plan(i), ctx_v, ctx_a, tables)
        if compile_step or (s_bf == sig[i] and sn_bf == sig[i + 1]):
            lat_v = gd.tail(vp, vn, None, lat_v, s_bf, sn_bf, plan_v.clean, plan_v.mask_tok_f32)
            vol_a = gd.tail(ap, an, None, vol_a, s_bf, sn_bf, None, None)
        else:
            lat_v = _eager_tail(gd, vp, vn, None, lat_v, s_bf, sig[i], sig[i + 1], plan_v)
            vol_a = _eager_tail(gd, ap, an, None, vol_a, s_bf, sig[i], sig[i + 1], plan_a)
    return lat_v, audio_volume_to_latent(vol_a, ac)


def denoise_audio_only(audio_latents: torch.Tensor, audio_positions: torch.Tensor, audio_embeddings: torch.Tensor,
                       transformer: LTXModel, sigmas: Sequence[float], verbose: bool = False, eval_interval: int = 1,
                       compile_step: bool = False, compile_shapeless: bool = False, fp32_euler: bool = True,
                       ui_phase: str = "audio_denoise", use_graph: bool = False, graph_cache: Optional[dict] = None,
                       cache_context: bool = False, step_cache=None) -> torch.Tensor:
    """generate.py:888-1053: the distilled-style loop of separate audio generation over an audio-only transformer
    (``LTXModelConfig.audio()``), no CFG.  audio_latents (B,8,T,16), audio_positions (B,1,T,2) seconds
    (``schedulers.create_audio_position_grid``), audio_embeddings (B,S,caption_channels); returns (B,8,T,16) bf16.
    The latents run through the video loop as a (B,128,T,1,1) volume - converted once on entry and once on exit, where the
    reference transposes in every step - so the step tail, the sigma handling (x0 with bf16(sigma), Euler in fp32 with the
    Python floats; bf16 sigmas under ``compile_step``), ``use_graph`` and ``cache_context`` are ``denoise_distilled``'s.  A step cache (``step_cache``) is not part of this loop: ValueError."""
    _refuse_step_cache(step_cache, "the audio-only loop (denoise_audio_only)")
    if audio_latents.dim() != 4:
        raise ValueError(f"audio_latents must be (B,C,T,F), got {tuple(audio_latents.shape)}")
    b, c, t, f = audio_latents.shape
    if c * f != transformer.config.in_channels:
        raise ValueError(f"audio_latents (B,{c},T,{f}) carry {c * f} values per frame, the transformer takes {transformer.config.in_channels}")
    if tuple(audio_positions.shape) != (b, 1, t, 2):
        raise ValueError(f"audio_positions must be ({b},1,{t},2), got {tuple(audio_positions.shape)}")
    if len(transformer.positional_embedding_max_pos) != 1:
        raise ValueError("denoise_audio_only needs an audio-only transformer (one position axis, LTXModelConfig.audio())")
    sig = [float(s) for s in (sigmas.tolist() if torch.is_tensor(sigmas) else sigmas)]
    out = _denoise(audio_latent_to_volume(audio_latents.to(BF16)), audio_positions.to(audio_latents.device), audio_embeddings, None, transformer, sig, 1.0,
                   None, compile_step, False, use_graph, graph_cache, cache_context, not fp32_euler)
    return audio_volume_to_latent(out, c)
