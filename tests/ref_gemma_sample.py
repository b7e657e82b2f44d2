"""What ``ops.sample_rows`` (csrc/sample.hip) may return, stated in float64, and an fp32 numpy emulation of the kernel's own
order of operations.

``admissible`` is the reference.  The kernel draws by the inverse CDF on ONE uniform per (draw, row), so the tokens a correct
fp32 implementation may return are those whose float64 CDF interval lies within ``tol`` of u * S:

    tol = 2^-23 * sum_v p_v (|z_v - m| + 4)  +  depth * 2^-24 * S

First term: what fp32 arithmetic does to one p_v = exp(z_v - m).  z_v = l'_v / T carries half an ulp of its own, m another,
their difference a third - each at most 2^-24 |z| <= 2^-24 (|z - m| + |m|), and the exponential turns an absolute error of its
argument into a relative one of its value - plus the exponential's own rounding (2 ulp allowed); |m| enters only through
z - m, where the kernel and float64 subtract the same m, so the bound keeps |z - m| and spends the constant 4 on the half-ulps
and the exponential.  Second term: a prefix sum that went through ``depth`` sequential fp32 additions is off by at most
depth * 2^-24 times the largest partial sum, S.  ``depth`` is the kernel's longest chain: SAMPLE_DEPTH_BASE = 17 inside a
2048-element chunk (7 in the thread, 6 levels of the lane scan, 2 wave offsets, the thread's base, the element) plus one per
chunk for the ascending merge - ``sample_depth(V)``, the constants of mlx_video_amd/ops.py and of the kernel's header comment.
The penalty itself is exact fp32 arithmetic (one IEEE multiply or one correctly rounded divide), so ``admissible`` applies it in
fp32 and widens from there; temperature 0 has one admissible token, the smallest index of the maximum."""
import numpy as np

SAMPLE_CHUNK = 2048
SAMPLE_DEPTH_BASE = 17


def sample_depth(V: int) -> int:
    return SAMPLE_DEPTH_BASE + -(-V // SAMPLE_CHUNK)


def penalised(logits, ctx, penalty, twice=False):
    """fp32 l': the ids of ``ctx`` (a set: once per id) multiplied by ``penalty`` when negative, else divided by it.  ``twice``
    (a planted fault): once per OCCURRENCE."""
    l = np.asarray(logits, dtype=np.float32).copy()
    pen = np.float32(penalty)
    if pen != np.float32(1.0):
        ids = [int(t) for t in ctx] if twice else sorted(set(int(t) for t in ctx))
        for v in ids:
            if 0 <= v < l.size:
                l[v] = l[v] * pen if l[v] < 0 else l[v] / pen
    return l


def cdf64(logits, ctx, penalty, temperature):
    """(p, lo, cum, S, tol) in float64 of softmax(l' / temperature): token t owns [lo[t], cum[t])."""
    z = penalised(logits, ctx, penalty).astype(np.float64) / float(np.float32(temperature))
    m = z.max()
    p = np.exp(z - m)
    cum = np.cumsum(p)
    S = float(cum[-1])
    tol = 2.0 ** -23 * float((p * (np.abs(z - m) + 4.0)).sum()) + sample_depth(z.size) * 2.0 ** -24 * S
    return p, np.concatenate([[0.0], cum[:-1]]), cum, S, tol


def admissible(logits, ctx, penalty, temperature, u, cdf=None):
    """The set of tokens a correct fp32 sampler may return for the uniform ``u`` (see the module docstring): t with p_t > 0
    and lo[t] - tol <= u * S <= cum[t] + tol.  ``cdf``: a ``cdf64`` result to reuse over many uniforms."""
    if temperature == 0:
        l = penalised(logits, ctx, penalty)
        return {int(np.flatnonzero(l == l.max())[0])}
    p, lo, cum, S, tol = cdf or cdf64(logits, ctx, penalty, temperature)
    x = float(np.float32(u)) * S
    first = int(np.searchsorted(cum, x - tol, side="left"))           # cum[t] + tol >= x   (cum and lo ascend)
    end = int(np.searchsorted(lo, x + tol, side="right"))             # lo[t] - tol <= x
    return set(t for t in range(first, end) if p[t] > 0)


class Emulation:
    """The kernel's arithmetic in fp32 numpy, in its order: per chunk of 2048 the 8-element running sums of a thread, the
    inclusive scan of the 64 thread totals of a wave (x[i] += x[i - d], d = 1 .. 32), the waves' totals added in ascending
    order, prefix = (wave offset + lanes before) + running sum; the chunk's sum is the prefix of its last element, the chunks
    are merged by one ascending chain, target = u * S, the first chunk whose cumulative sum exceeds it, then the smallest v
    there with p_v > 0 and cum[c - 1] + prefix(v) > target, else the largest v with p_v > 0.
    ``fault``: "no_temperature", "no_penalty", "penalty_twice" alter the distribution; "next" / "prev" the returned token."""

    def __init__(self, logits, ctx, penalty, temperature, fault=None):
        self.fault, self.V = fault, len(logits)
        f32 = np.float32
        l = penalised(logits, ctx, 1.0 if fault == "no_penalty" else penalty, twice=fault == "penalty_twice")
        self.l = l
        if temperature == 0:
            return
        T = f32(1.0) if fault == "no_temperature" else f32(temperature)
        z = (l / T).astype(f32)
        m = f32(l.max()) / T
        p = np.exp((z - m).astype(f32)).astype(f32)
        nch = -(-self.V // SAMPLE_CHUNK)
        pp = np.zeros(nch * SAMPLE_CHUNK, dtype=f32)
        pp[:self.V] = p
        loc = np.cumsum(pp.reshape(nch, 4, 64, 8), axis=3, dtype=f32)          # sequential, fp32
        x = loc[..., 7].copy()
        for d in (1, 2, 4, 8, 16, 32):
            y = x.copy()
            y[..., d:] = x[..., d:] + x[..., :-d]
            x = y
        before = np.concatenate([np.zeros_like(x[..., :1]), x[..., :-1]], axis=2)
        wtot = x[..., 63]                                                      # (nch, 4)
        off = np.zeros_like(wtot)
        for w in range(1, 4):
            off[:, w] = off[:, w - 1] + wtot[:, w - 1]
        base = (off[..., None] + before).astype(f32)
        self.incl = (base[..., None] + loc).astype(f32).reshape(nch, SAMPLE_CHUNK)
        self.p = pp.reshape(nch, SAMPLE_CHUNK)
        self.sums = self.incl[:, -1].copy()
        self.cum = np.cumsum(self.sums, dtype=f32)
        self.S = self.cum[-1]

    def token(self, u) -> int:
        t = self._token(u)
        return {"next": min(t + 1, self.V - 1), "prev": max(t - 1, 0)}.get(self.fault, t)

    def _token(self, u) -> int:
        if not hasattr(self, "cum"):
            return int(np.flatnonzero(self.l == self.l.max())[0])
        f32 = np.float32
        target = f32(u) * self.S
        over = np.flatnonzero(self.cum > target)
        if over.size:
            c = int(over[0])
            below = self.cum[c - 1] if c else f32(0.0)
            hit = np.flatnonzero((self.p[c] > 0) & ((below + self.incl[c]).astype(f32) > target))
            if hit.size:
                return c * SAMPLE_CHUNK + int(hit[0])
        else:
            c = int(np.flatnonzero(self.sums > 0)[-1])
        return c * SAMPLE_CHUNK + int(np.flatnonzero(self.p[c] > 0)[-1])


def bf16_round(x):
    """float array rounded to bfloat16 (nearest even), as float32."""
    import torch
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def dominant_logits(V: int, at: int = 2, values=(4.0, 3.0, 3.5), floor: float = -24.0):
    """V logits with three dominant neighbours at ``at`` .. ``at + 2`` over a floor whose whole mass is below e^-27 each: the
    inputs of the planted-fault and single-token-set checks (every value a bf16 number)."""
    l = np.full(V, floor, dtype=np.float32)
    l[at:at + 3] = values
    return l
