"""Test-side restatement of the CFG* and APG guiders of the guided step (include/ltxk.h "CFG* and APG"; DESIGN.md 5j;
ltx_core/components/guiders.py:14-43, 57-76), in torch on the CPU.

Two forms.  ``*_f64``: float64 without any rounding - the guiders' mathematics, compared with ``components`` in
test_guiders_cpu.py.  The rest: float32 with the explicit bf16 rounding points the kernels state (``r`` = round to bf16; every
array-valued op of the reference materialises a bf16 array), tokens (B,S,C) and latents (B,C,S) as the kernels take them.
Sums are per batch sample over all C*S elements; each summand is the bf16-rounded product; a sum is used as r(sum).

The device record has 8 fp32 per sample (ltxk.h): cfg_star [0] S r(p*n) [1] S r(n*n) [5] a; apg [0] S r(g*g) (g before the
clamp) [1] S r(g*p) (g after it) [2] S r(p*p) [3] nrm [4] f [5] c; f = 1 and [0] = [3] = 0 without the clamp."""
import torch

BF = torch.bfloat16
EPS = 1e-8
REC = 8


def r(t):
    return t.to(BF).float()


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def per_sample(t, like):
    """(B,) scalars -> broadcastable against (B,C,S)."""
    return t.reshape(-1, *([1] * (like.dim() - 1))).to(like.dtype)


# ------------------------------------------------------------------------------------------------- float64, no rounding
def cfg_star_x0_f64(p, n, a, scale):
    """CFG* with a given projection coefficient: p + (scale-1) * (p - a*n)."""
    return p + (scale - 1.0) * (p - a * n)


def guided_x0_f64(p, n, kind, scale, eta=1.0, norm_threshold=0.0):
    """p + delta(p, n) in the dtype of p (float64 in the tests), sums per sample over every other axis."""
    b = p.shape[0]
    dot = lambda u, v: per_sample((u.reshape(b, -1) * v.reshape(b, -1)).sum(1), p)
    k = scale - 1.0
    if kind == "cfg":
        return p + k * (p - n)
    if kind == "cfg_star":
        return cfg_star_x0_f64(p, n, dot(p, n) / (dot(n, n) + EPS), scale)
    assert kind == "apg"
    g = p - n
    if norm_threshold > 0:
        nrm = torch.sqrt(dot(g, g) + EPS)
        g = g * torch.minimum(torch.ones_like(nrm), norm_threshold / nrm)
    c = dot(g, p) / (dot(p, p) + EPS)
    par = c * p
    return p + k * (par * eta + (g - par))


# ----------------------------------------------------------------------------------------- float32 with bf16 rounding
def denoised(v_tok, x, sigma):
    """r(x - sigma*v): v (B,S,C) tokens, x (B,C,S) -> (B,C,S) float32 holding bf16 values."""
    return r(x.float() - sigma * v_tok.float().transpose(1, 2))


def apg_guidance(p, n, clamp, f):
    g = r(p - n)
    if clamp:
        g = r(g * per_sample(f, g))
    return g


def sums_f64(p, n, kind, norm_threshold=0.0, f=None):
    """The float64 sums of the bf16-rounded products, and the sums of their absolute values (the error bound's scale):
    {name: (sum (B,), abs sum (B,))}.  ``f`` (B,): the clamp factor the rescaled g of S r(g*p) is built with."""
    b = p.shape[0]

    def s(u, v):
        t = r(u * v).double().reshape(b, -1)
        return t.sum(1), t.abs().sum(1)
    if kind == "cfg_star":
        return {"pn": s(p, n), "nn": s(n, n)}
    clamp = norm_threshold > 0
    out = {"pp": s(p, p)}
    if clamp:
        g0 = apg_guidance(p, n, False, None)
        out["gg"] = s(g0, g0)
    g = apg_guidance(p, n, clamp, f)
    out["gp"] = s(g, p)
    return out


def coef(num, den):
    """r(r(num) / r(r(den) + 1e-8)) from sums of any float dtype."""
    return r(r(num) / r(r(den) + f32(EPS)))


def clamp_scalars(gg, norm_threshold):
    nrm = r(torch.sqrt(r(r(gg) + f32(EPS))))
    return nrm, torch.minimum(torch.ones_like(nrm), r(f32(norm_threshold) / nrm))


def record(v_pos, v_neg, x, sigma, kind, norm_threshold=0.0):
    """The whole record (B,8) float32 from float64 sums: what ltxk_guidance_sums writes, up to the rounding of its sums."""
    p, n = denoised(v_pos, x, sigma), denoised(v_neg, x, sigma)
    rec = torch.zeros(p.shape[0], REC)
    rec[:, 4] = 1.0
    if kind == "cfg_star":
        sm = sums_f64(p, n, kind)
        rec[:, 0], rec[:, 1] = sm["pn"][0].float(), sm["nn"][0].float()
        rec[:, 5] = coef(sm["pn"][0], sm["nn"][0])
        return rec
    f = None
    if norm_threshold > 0:
        g0 = apg_guidance(p, n, False, None)
        gg = r(g0 * g0).double().reshape(p.shape[0], -1).sum(1)
        rec[:, 0] = gg.float()
        rec[:, 3], rec[:, 4] = clamp_scalars(gg, norm_threshold)
        f = rec[:, 4]
    sm = sums_f64(p, n, kind, norm_threshold, f)
    rec[:, 1], rec[:, 2] = sm["gp"][0].float(), sm["pp"][0].float()
    rec[:, 5] = coef(sm["gp"][0], sm["pp"][0])
    return rec


def tail(v_pos, v_neg, v_pert, x, rec, kind, cfg_scale, stg_scale, sigma, sigma_next, eta=1.0, norm_threshold=0.0, clean=None,
         mask=None, bf16_euler=False):
    """ltxk_guider_euler_step: the guided x0 with the scalars of ``rec`` (B,8), the STG term, mask blend and Euler -> bf16."""
    xf = x.float()
    p, n = denoised(v_pos, x, sigma), denoised(v_neg, x, sigma)
    k = f32(cfg_scale) - 1.0
    c = per_sample(rec[:, 5].float(), p)
    if kind == "cfg_star":
        d = r(k * r(p - r(c * n)))
    else:
        g = apg_guidance(p, n, norm_threshold > 0, rec[:, 4].float())
        par = r(c * p)
        d = r(k * r(r(par * f32(eta)) + r(g - par)))
    x0 = r(p + d)
    if v_pert is not None:
        x0 = r(x0 + r(f32(stg_scale) * r(p - denoised(v_pert, x, sigma))))
    if mask is not None:
        m = mask[:, None, :].float()
        x0 = r(r(x0 * m) + r(clean.float() * r(1.0 - m)))
    if bf16_euler:
        o = x0 + r(r(sigma_next * r(xf - x0)) / sigma)
    elif sigma_next > 0:
        o = x0 + (sigma_next * (xf - x0)) / sigma
    else:
        o = x0
    return o.to(BF)
