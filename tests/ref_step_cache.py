"""References of the step cache (csrc/step_cache.hip, denoise.StepCache), shared by the CPU and the GPU tests:

* ``probe_emulation``: the probe's two sums in numpy float32, in the summation order the kernel's header documents, next to the
  float64 sums and the bound gamma_(depth + 1) * sum |t_i| they are held to;
* ``cached_loop``: the cached CFG denoise loop restated out of ``oracle.dit``'s pieces, in float64 or under a bf16 policy,
  teacher-forced with a list of decisions or deciding by ``StepCache.decide`` itself, with the algorithm faults the CPU
  tests plant."""
import numpy as np
import torch

from oracle import dit as O

CHUNK, THREADS, VECS, DEPTH_BASE = 8192, 256, 4, 40
U = 2.0 ** -24


def chunks(n):
    return -(-n // CHUNK)


def depth(rows, D):
    return DEPTH_BASE + chunks(rows * D) - 1


def gamma(k):
    return k * U / (1 - k * U)


def bf16_as_f32(t):
    """A bf16 torch tensor as a flat numpy float32 array (exact; NaN payloads and signed zeros kept)."""
    bits = t.detach().cpu().contiguous().view(torch.int16).numpy().reshape(-1).astype(np.uint16).astype(np.uint32) << 16
    return bits.view(np.float32)


def ordered_sum(terms, drop_chunk=None, reverse_merge=False):
    """float32 sum of the non-negative float32 ``terms`` in the kernel's order.  Planted faults: ``drop_chunk`` leaves a
    chunk out of the merge, ``reverse_merge`` merges in descending chunk order."""
    n = terms.size
    nc = chunks(n)
    t = np.zeros(nc * CHUNK, dtype=np.float32)
    t[:n] = terms
    t = t.reshape(nc, VECS, THREADS, 8)                     # element 8 * (1024 c + 256 k + thread) + j
    acc = np.zeros((nc, THREADS), dtype=np.float32)
    for k in range(VECS):                                   # the thread's chain: k ascending, j ascending, from 0
        for j in range(8):
            acc = acc + t[:, k, :, j]
    w = acc.reshape(nc, THREADS // 64, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):                        # the wave butterfly
        w = w + w[:, :, lane ^ off]
    w = w[:, :, 0]
    part = w[:, 0]
    for i in range(1, THREADS // 64):                       # the wave totals, ascending
        part = part + w[:, i]
    assert part.dtype == np.float32
    order = [c for c in range(nc) if c != drop_chunk]
    if reverse_merge:
        order.reverse()
    s = np.float32(0.0)
    for c in order:                                         # the merge, ascending chunks
        s = np.float32(s + part[c])
    return s


def probe_terms(cur, prev):
    """The float32 terms of S_d and S_p: |cur - prev| rounds once, to float32 - and that rounded term is what the sums add;
    |prev| is exact."""
    a, b = bf16_as_f32(cur), bf16_as_f32(prev)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs((a - b).astype(np.float32)), np.abs(b)


def probe_emulation(cur, prev, **fault):
    """((S_d, S_p) float32 in the kernel's order, (S_d, S_p) float64 of the same terms, (bound_d, bound_p)) with
    |float32 - float64| <= bound = gamma_(depth + 1) * sum |t_i|."""
    td, tp = probe_terms(cur, prev)
    s32 = (ordered_sum(td, **fault), ordered_sum(tp, **fault))
    s64 = (float(td.astype(np.float64).sum()), float(tp.astype(np.float64).sum()))
    g = gamma(DEPTH_BASE + chunks(td.size) - 1 + 1)
    return s32, s64, (g * s64[0], g * s64[1])


# ------------------------------------------------------------------------------------------------- the cached loop, restated
LIVELY = dict(blk=3.0, txt=6.0, ada=2.0, emb=8.0, head=0.5, gate=1.0)      # the timestep moves block 0's input from step to step
QUIET = dict(blk=16.0, txt=16.0, ada=0.25, emb=1.0, head=0.5, gate=12.0)   # the latents' drift does, and the blocks dominate x


def make_weights(cfg, seed=7, blk=3.0, txt=6.0, ada=2.0, emb=8.0, head=0.5, gate=1.0):
    """``oracle.dit.make_weights`` with the blocks given a trained model's weight in the result: at N(0, 0.02^2) throughout, the
    gates are ~0.02, the blocks add a few percent to the residual stream and neither the text nor the timestep moves much - a
    wrong residual or a wrong decision then moves the latents by less than one bf16 evaluation's own error, which no test
    could see.  The blocks' modulation tables become N(0, 0.5^2) with the gate rows around ``gate``; the self-attention and
    feed-forward value / output projections are scaled by ``blk``, the text attention's by ``txt``; the timestep path by ``ada``
    (adaln_single.linear) and ``emb`` (the embedder's second layer); the head's table is N(0, head^2).  LIVELY and QUIET are
    the two settings the tests use."""
    W = O.make_weights(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    D, bf = cfg.dim, torch.bfloat16

    def scale(name, k):
        W[name] = (W[name].float() * k).to(bf)

    for i in range(cfg.num_layers):
        pre = f"transformer_blocks.{i}"
        tab = torch.randn(6, D, generator=g) * 0.5
        tab[2] += gate
        tab[5] += gate
        W[f"{pre}.scale_shift_table"] = tab.to(bf)
        for name in (f"{pre}.attn1.to_out", f"{pre}.ff.proj_out", f"{pre}.attn1.to_v"):
            scale(f"{name}.weight", blk)
        for name in (f"{pre}.attn2.to_out", f"{pre}.attn2.to_v"):
            scale(f"{name}.weight", txt)
    scale("adaln_single.linear.weight", ada)
    scale("adaln_single.emb.timestep_embedder.linear2.weight", emb)
    W["scale_shift_table"] = (torch.randn(2, D, generator=g) * head).to(bf)
    return W


def fwd_prepare(tok, ts, context, pe, W, cfg, p):
    """``oracle.dit.ltx_forward`` in front of its blocks, statement for statement."""
    latent, context = p.r(tok), p.r(context)
    b, n, _ = latent.shape
    x = O.linear(latent, W["patchify_proj.weight"], W["patchify_proj.bias"], p)
    t = p.r(p.r(ts) * cfg.timestep_scale_multiplier)
    ss, emb = O.adaln_single(t.reshape(-1), W, "adaln_single", p)
    ctx = O.linear(context, W["caption_projection.linear1.weight"], W["caption_projection.linear1.bias"], p)
    ctx = O.gelu_tanh(ctx, p)
    ctx = O.linear(ctx, W["caption_projection.linear2.weight"], W["caption_projection.linear2.bias"], p)
    cos, sin = pe
    if cos.shape[0] != b:
        cos, sin = cos.expand(b, *cos.shape[1:]), sin.expand(b, *sin.shape[1:])
    return dict(x=x, ts=ss.reshape(b, n, -1), emb=emb.reshape(b, n, -1), ctx=ctx.reshape(b, -1, x.shape[-1]), pe=(cos, sin))


def block0_input(st, W, cfg, p):
    """Block 0's modulated self-attention input (``oracle.dit.transformer_block``'s first ``nx``)."""
    shift, scale, _ = O.ada_values(W["transformer_blocks.0.scale_shift_table"], st["ts"], 0, 3, p)
    return O.modulate(O.rms_norm(st["x"], p, cfg.norm_eps), scale, shift, p)


def fwd_blocks(st, W, cfg, p):
    x = st["x"]
    for i in range(cfg.num_layers):
        x = O.transformer_block(x, st["ts"], st["ctx"], st["pe"], W, i, cfg, p)
    return x


def fwd_head(st, x, W, cfg, p):
    """``oracle.dit.ltx_forward`` behind its blocks."""
    tab = W["scale_shift_table"].to(p.dtype)
    shift = p.r(tab[0][None, None, :] + st["emb"])
    scale = p.r(tab[1][None, None, :] + st["emb"])
    x = O.modulate(O.layer_norm_noaffine(x, p, cfg.norm_eps), scale, shift, p)
    return O.linear(x, W["proj_out.weight"], W["proj_out.bias"], p)


FAULTS = ("prev_on_computed", "acc_no_reset", "cache_behind_head", "shared_residual")


def cached_loop(lat, positions, ctx_pos, ctx_neg, W, cfg, sigmas, p, cfg_scale, decisions=None, decide=None, threshold=None,
                coefficients=(1.0, 0.0), fault=None):
    """``oracle.dit.denoise_dev`` (compiled step, no mask) with a step cache.  ``decisions``: a teacher-forced list of booleans;
    else ``decide`` (StepCache.decide) with ``threshold`` / ``coefficients`` decides from the restated sums.  Returns
    (latents, report), report[i] = {"rel", "computed", "s_d", "s_p"}.  ``fault``, the planted algorithm faults:
    "prev_on_computed" prev is updated on computed steps only; "acc_no_reset" the accumulator is not reset on compute;
    "cache_behind_head" the residual is taken over the blocks AND the head - the cache then holds what leaves the head, and a
    skipped step reuses the last computed velocity; "shared_residual" the pos and neg forwards share one residual (pos's)."""
    assert fault is None or fault in FAULTS
    n = len(sigmas) - 1
    pe = O.precompute_freqs_cis(torch.from_numpy(positions), cfg.dim, cfg.theta, cfg.max_pos, cfg.heads)
    x = p.r(lat)
    b, ntok = x.shape[0], x.shape[2] * x.shape[3] * x.shape[4]
    prev, acc, resid, report = None, 0.0, {}, []
    for i in range(n):
        s, s_next = float(sigmas[i]), float(sigmas[i + 1])
        s_m = O.bf16_round_scalar(s) if p.emulate_bf16 else s
        sn_m = O.bf16_round_scalar(s_next) if p.emulate_bf16 else s_next
        tok = O.latent_to_tokens(x)
        ts = p.r(s_m * torch.ones(b, ntok))
        sts = {"pos": fwd_prepare(tok, ts, ctx_pos, pe, W, cfg, p), "neg": fwd_prepare(tok, ts, ctx_neg, pe, W, cfg, p)}
        m = block0_input(sts["pos"], W, cfg, p).double()
        s_d = s_p = None
        if prev is not None:
            s_d, s_p = float((m - prev).abs().sum()), float(prev.abs().sum())
        if decisions is not None:
            compute, rel = bool(decisions[i]), (s_d / s_p if s_p else None)
        else:
            compute, acc_new, rel = decide(i, n, s_d, s_p, acc, threshold, coefficients)
            acc = acc_new if (not compute or fault == "acc_no_reset") else 0.0
        if prev is None or compute or fault != "prev_on_computed":
            prev = m
        report.append({"rel": rel, "computed": compute, "s_d": s_d, "s_p": s_p})
        v = {}
        for k, st in sts.items():
            rk = "pos" if fault == "shared_residual" else k
            if compute:
                x_out = fwd_blocks(st, W, cfg, p)
                v[k] = fwd_head(st, x_out, W, cfg, p)
                if rk == k:
                    resid[rk] = v[k] if fault == "cache_behind_head" else p.r(x_out - st["x"])
            elif fault == "cache_behind_head":
                v[k] = resid[rk]
            else:
                v[k] = fwd_head(st, p.r(st["x"] + resid[rk]), W, cfg, p)
        vel = O.tokens_to_latent(O.cfg_combine(v["pos"], v["neg"], cfg_scale, p), x.shape)
        x0 = O.to_denoised(x, vel, s_m, p)
        x = p.r(x0 + sn_m * (x - x0) / s_m)
    return x, report
