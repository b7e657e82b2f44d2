"""Every single-pass form of ltxk_gemm_bf16 - the 160-row family (TT = 1..5 x the 128- and 256-column tile), the 320 x 256 and
256 x 256 big tiles, what the product library's own dispatch takes - and the grouped persistent launch, held element by
element to tests/ref_gemm.py's float64 bound (tests/test_ref_gemm_cpu.py shows what that bound accepts and rejects).  ZERO
elements may lie beyond it.

Every case asserts its plan first (ops.gemm_plan / ops.gemm_grouped_plan: form, tile_rows, tile_cols, rem_rows), launches
through ops.gemm on strided views inside NaN frames that must survive (A with lda = K + 8 and the residual with ldr = N + 4
carry NaN pads, the gate is columns [N, 2N) of a 2N-wide table), runs twice and requires equal bits, and records the worst
d / bound with parity.auto(worst, 1.0, tag=...).  The shapes are the smallest that reach each path:

  M   1 | 32 TT + 1 | 64 TT + 17: one row, one row into the second tile, a ragged third (big tiles: 1 | tile + 1 | 2 tile + 17)
  N   8 | 136 | 264 | 1000: one 8-column group; 8 columns past a 128- and a 256-column tile; no multiple of 64
  K   64 | 128 | 192 | 256 | 64 * 67: 1, 2, 3 (= the ring's stages), 4 K-steps and a long odd count - all of them at one (M, N)
      per tile, K = 192 elsewhere
  out ldo = N + 8 on a 16-byte aligned base (the staged 16-byte stores, p.wide) and ldo = N + 4 on a base 8 bytes off (direct)
  V^T T = M for an odd M (element stores, one batch) | T = M / 2, T % 4 == 0 (vector stores) | T % 4 == 2 (a batch boundary
      inside a group of 4 tokens), ldo2 > T with NaN pad columns; the split k | V^T output at N = 264 + 256
  row statistics at N = 64 and 320 with sumsq_ld == N / 64 exactly and a canary behind

ref_gemm.inputs plants edge columns (bias 3e38, +-300, +-12, +-0 on a zero W row) in every N that has room: the BIAS output
there must be the bias itself, GELU of -300 the -0 of the formula."""
import pytest
import torch

import parity
import ref_gemm as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NS = 256                      # split output: k = columns [0, 256), V^T the rest


@pytest.fixture(scope="module")
def bank(dev):
    """(M, N, K) -> (inputs, s, mag): operands and float64 product, computed once and shared by epilogues and forms."""
    cache = {}

    def get(M, N, K):
        key = (M, N, K)
        if key not in cache:
            inp = R.inputs(M, N, K, M * 7 + N * 3 + K, dev)
            s, mag = R.product(inp.a, inp.w)
            R.premises(inp, s, mag)
            cache[key] = (inp, s, mag)
        return cache[key]
    yield get
    cache.clear()


def _bits(t):
    return t.view(torch.int16)


class Runner:
    """The launches of one test: every launch is planned and asserted first, run twice into fresh frames (equal bits), its
    frames checked, its output held to the bound; ``worst`` collects d / bound per tag."""

    def __init__(self, ops, dev, want):
        self.ops, self.dev, self.want, self.worst, self.launches = ops, dev, want, {}, 0

    def plan(self, inp, **kw):
        pl = self.ops.gemm_plan(inp.M, inp.N, inp.K, lda=inp.K + 8, **kw)
        self.want(pl, kw)
        return pl

    def note(self, tag, w):
        self.worst[tag] = max(self.worst.get(tag, 0.0), w)

    def twice(self, make, launch):
        """frames = make(); launch(frames) - twice; equal bits over the whole buffers, frames intact.  Returns the first."""
        runs = []
        for _ in range(2):
            frames = make()
            launch(*frames)
            runs.append(frames)
        torch.cuda.synchronize()
        self.launches += 1
        for f0, f1 in zip(*runs):
            assert torch.equal(_bits(f0.buf), _bits(f1.buf)), "two runs differ"
            assert f0.intact(), "wrote outside the output view"
        return runs[0]

    def rows(self, tag, inp, s, mag, epi, bias_on, row_on=True, direct=False, sumsq=False):
        """One row-major launch.  direct: ldo = N + 4 on a base 8 bytes off 16-byte alignment; else ldo = N + 8, aligned."""
        ops, dev, M, N = self.ops, self.dev, inp.M, inp.N
        ldo, lead = (N + 4, 4) if direct else (N + 8, 8)
        pl = self.plan(inp, epilogue=epi, ldo=ldo, sumsq=sumsq)
        kw = dict(epilogue=epi)
        if epi >= 3:
            kw["resid"] = inp.res
        if epi == R.EPI_BIAS_GATE_RES:
            kw.update(gate=inp.gate, gate_row=inp.grow if row_on else None, gate_stride=inp.gate_stride)
        if epi == R.EPI_SCALE_RES:
            kw["alpha"] = inp.alpha
        P = N // 64

        def make():
            out = R.rows_frame(M, N, ldo, dev, lead=lead)
            return (out, R.Frame((M, P), (P, 1), dev, dtype=torch.float32, lead=0, sentinel=-7.0)) if sumsq else (out,)

        def launch(out, ss=None):
            ops.gemm(inp.a, inp.w, inp.b if bias_on else None, out=out.view, sumsq=None if ss is None else ss.view, **kw)
        got = self.twice(make, launch)
        out = got[0].view
        name = f"{tag} {M}x{N}x{inp.K} epi{epi} bias={bias_on} gate_row={row_on} {'direct' if direct else 'wide'}"
        d, b = R.bound(epi, out, s, mag, inp.K, inp.b if bias_on else None, inp.res if epi >= 3 else None,
                       R.gate_of(inp, row_on) if epi == R.EPI_BIAS_GATE_RES else None, inp.alpha)
        self.note(tag, R.check(name, d, b, tile=(pl.tile_rows, pl.tile_cols)))
        if sumsq:
            self.note(tag + ".sumsq", R.check(name + " sumsq", *R.sumsq_bound(got[1].view, out)))
        cols = [c for c, _ in inp.edge]
        if cols and epi == R.EPI_BIAS:                   # y IS the bias (or 0) there: no rounding at all
            want = inp.b[cols] if bias_on else torch.zeros(len(cols), dtype=BF, device=dev)
            assert bool((out[:, cols] == want).all()), name + ": an edge column is not its bias"
        if cols and epi == R.EPI_BIAS_GELU and bias_on:
            c = [c for c, v in inp.edge if v == -300.0]
            assert bool((out[:, c] == 0).all()) and bool(torch.signbit(out[:, c]).all()), name + ": gelu(-300) is not -0"

    def transposed(self, tag, inp, s, mag, T, bias_on, split, sumsq=False):
        """V^T (split False) or the split k | V^T launch: T tokens per batch, ldo2 > T with NaN pad columns."""
        ops, dev, M, N = self.ops, self.dev, inp.M, inp.N
        nb, ld = M // T, (T + 3) // 4 * 4 + 4
        bias = inp.b if bias_on else None
        name = f"{tag} {M}x{N}x{inp.K} T={T} bias={bias_on}"
        if not split:
            pl = self.plan(inp, out_tokens_per_batch=T, ldo=ld)
            (vt,) = self.twice(lambda: (R.vt_frame(nb, N, T, ld, dev),),
                               lambda vt: ops.gemm(inp.a, inp.w, bias, out=vt.view, out_tokens_per_batch=T))
            self.note(tag, R.check(name, *R.bound(0, R.vt_rows(vt.view, T), s, mag, inp.K, bias), tile=(pl.tile_rows, pl.tile_cols)))
            return
        pl = self.plan(inp, n_split=NS, out_tokens_per_batch=T, ldo=NS + 8, ldo2=ld, sumsq=sumsq)
        P = NS // 64

        def make():
            f = (R.rows_frame(M, NS, NS + 8, dev), R.vt_frame(nb, N - NS, T, ld, dev, lead=4))
            return f + ((R.Frame((M, P), (P, 1), dev, dtype=torch.float32, lead=0, sentinel=-7.0),) if sumsq else ())

        def launch(k, v, ss=None):
            ops.gemm(inp.a, inp.w, bias, out=k.view, out2=v.view, n_split=NS, out_tokens_per_batch=T, sumsq=None if ss is None else ss.view)
        got = self.twice(make, launch)
        tile = (pl.tile_rows, pl.tile_cols)
        self.note(tag + ".k", R.check(name + " k", *R.bound(0, got[0].view, s[:, :NS], mag[:, :NS], inp.K, None if bias is None else bias[:NS]), tile=tile))
        self.note(tag + ".vt", R.check(name + " vt", *R.bound(0, R.vt_rows(got[1].view, T), s[:, NS:], mag[:, NS:], inp.K,
                                                              None if bias is None else bias[NS:]), tile=tile))
        if sumsq:
            self.note(tag + ".sumsq", R.check(name + " sumsq", *R.sumsq_bound(got[2].view, got[0].view)))

    def record(self):
        for tag, w in sorted(self.worst.items()):
            print(f"{tag}: worst d / bound = {w:.3f}")
            parity.auto(w, 1.0, tag=tag)
        print(f"{self.launches} launches, each twice")


def _t_kinds(base):
    """(M, T) of the three transposed kinds: T = M odd (element stores, one batch); T = M / 2 with T % 4 == 0 (vector
    stores); T % 4 == 2 (a batch boundary inside a group of 4 tokens)."""
    kinds = [(base + 17, base + 17), (base + 24, (base + 24) // 2), (base + 20, (base + 20) // 2)]
    assert kinds[0][0] % 2 == 1 and kinds[1][1] % 4 == 0 and kinds[2][1] % 4 == 2
    return kinds


def _forced_single(tt, nt):
    from mlx_video_amd import _lib

    def want(pl, kw):
        assert (pl.form, pl.tile_rows, pl.tile_cols) == (_lib.GEMM_FORM_SINGLE, 32 * tt, 64 * nt), (kw, pl)
    return want


def _force_160(monkeypatch, tt, nt):
    monkeypatch.setenv("LTXK_GEMM_KSPLIT", "-1")
    monkeypatch.setenv("LTXK_GEMM_BIG", "0")
    monkeypatch.setenv("LTXK_GEMM_TT", str(tt))
    monkeypatch.setenv("LTXK_GEMM_NT", str(nt))


@pytest.mark.parametrize("nt", [2, 4], ids=["128col", "256col"])
@pytest.mark.parametrize("tt", [1, 2, 3, 4, 5])
def test_160_row_family_epilogues(dev, bank, tt, nt, monkeypatch, ab_lib):
    """Six epilogues, with and without bias (the gate epilogue also without gate_row), both store paths: the M x N cross at
    K = 192, every K at (64 TT + 17, 264)."""
    from mlx_video_amd import ops
    _force_160(monkeypatch, tt, nt)
    run = Runner(ops, dev, _forced_single(tt, nt))
    Ms, Ns = (1, 32 * tt + 1, 64 * tt + 17), (8, 136, 264, 1000)
    cases = [("rows", M, N, 192) for M in Ms for N in Ns] + [("ksteps", Ms[2], 264, K) for K in (64, 128, 256, 64 * 67)]
    for tag, M, N, K in cases:
        inp, s, mag = bank(M, N, K)
        for epi in range(6):
            for bias_on in (True, False):
                for direct in (False, True):
                    run.rows(tag, inp, s, mag, epi, bias_on, direct=direct)
        run.rows(tag, inp, s, mag, R.EPI_BIAS_GATE_RES, True, row_on=False)
    run.record()


@pytest.mark.parametrize("nt", [2, 4], ids=["128col", "256col"])
@pytest.mark.parametrize("tt", [1, 2, 3, 4, 5])
def test_160_row_family_statistics_and_transposed(dev, bank, tt, nt, monkeypatch, ab_lib):
    """Row statistics (the epilogues that have them) at N = 64 and 320 with sumsq_ld == N / 64 and a canary behind; V^T at
    N = 264 and the split k | V^T output at N = 264 + 256 (and, with its statistics, 320 + 256) in the three T kinds."""
    from mlx_video_amd import ops
    _force_160(monkeypatch, tt, nt)
    run = Runner(ops, dev, _forced_single(tt, nt))
    for M in (1, 32 * tt + 1, 64 * tt + 17):
        for N in (64, 320):
            inp, s, mag = bank(M, N, 192)
            for epi in (R.EPI_BIAS, R.EPI_BIAS_GATE_RES, R.EPI_BIAS_RES):
                run.rows("stats", inp, s, mag, epi, True, sumsq=True)
            run.rows("stats", inp, s, mag, R.EPI_BIAS, False, direct=True, sumsq=True)
    for M, T in _t_kinds(64 * tt):
        for bias_on in (True, False):
            run.transposed("vt", *bank(M, 264, 192), T, bias_on, split=False)
            run.transposed("split", *bank(M, 264 + NS, 192), T, bias_on, split=True)
            run.transposed("split", *bank(M, 320 + NS, 192), T, bias_on, split=True, sumsq=True)      # (statistics need N % 64 == 0)
    run.transposed("vt", *bank(1, 264, 192), 1, True, split=False)
    run.record()


@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("big,tile", [(2, 320), (3, 256)], ids=["320row", "256row"])
def test_big_tiles(dev, bank, big, tile, N, monkeypatch, ab_lib):
    """The 320 x 256 and 256 x 256 tiles, forced: epilogues 0, 1, 2 with and without bias on both store paths at every (M, K);
    row statistics; V^T and (N = 768) the split output in the three T kinds."""
    from mlx_video_amd import _lib, ops
    monkeypatch.setenv("LTXK_GEMM_BIG", str(big))
    monkeypatch.setenv("LTXK_GEMM_KSPLIT", "-1")

    def want(pl, kw):
        assert (pl.form, pl.tile_rows, pl.tile_cols) == (_lib.GEMM_FORM_BIG, tile, 256), (kw, pl)
    run = Runner(ops, dev, want)
    for M in (1, tile + 1, 2 * tile + 17):
        for K in (64, 128, 192, 576):
            inp, s, mag = bank(M, N, K)
            for epi in (R.EPI_BIAS, R.EPI_BIAS_GELU, R.EPI_BIAS_SILU):
                for bias_on in (True, False):
                    for direct in (False, True):
                        run.rows("rows", inp, s, mag, epi, bias_on, direct=direct)
            run.rows("stats", inp, s, mag, R.EPI_BIAS, True, sumsq=True)
            run.rows("stats", inp, s, mag, R.EPI_BIAS, False, direct=True, sumsq=True)
    for M, T in _t_kinds(2 * tile):
        for K in (64, 128, 192, 576):
            for bias_on in (True, False):
                run.transposed("vt", *bank(M, N, K), T, bias_on, split=False)
                if N > NS:
                    run.transposed("split", *bank(M, N, K), T, bias_on, split=True, sumsq=bias_on)
    run.record()


# what the product library takes by itself (no environment, no measurement build): M, N -> form, tile rows, tile columns of
# the epilogues the big tiles have (0, 1, 2); the others stay on the 160-row family there
DEFAULT = {(2560, 4096): ("single", 160, 256), (1280, 4096): ("single", 160, 128), (2560, 8192): ("big", 320, 256),
           (2048, 8192): ("big", 256, 256)}


@pytest.mark.parametrize("M,N", sorted(DEFAULT))
def test_default_dispatch(dev, bank, M, N):
    """The product library's own choice at K = 128, asserted and not forced: the 256- and the 128-column single-pass tile
    (M = 1280, N = 4096 is the model's), the 320-row tile, the 256-row tile.  All six epilogues."""
    from mlx_video_amd import _lib, ops
    form, rows, cols = DEFAULT[(M, N)]

    def want(pl, kw):
        if form == "big" and kw.get("epilogue", 0) <= R.EPI_BIAS_SILU:
            assert (pl.form, pl.tile_rows, pl.tile_cols) == (_lib.GEMM_FORM_BIG, rows, cols), (kw, pl)
        elif form == "big":
            assert pl.form == _lib.GEMM_FORM_SINGLE and pl.tile_rows <= 160, (kw, pl)
        else:
            assert (pl.form, pl.tile_rows, pl.tile_cols) == (_lib.GEMM_FORM_SINGLE, rows, cols), (kw, pl)
    run = Runner(ops, dev, want)
    inp, s, mag = bank(M, N, 128)
    for epi in range(6):
        run.rows(f"epi{epi}", inp, s, mag, epi, True, direct=epi == R.EPI_BIAS_GELU)
    run.rows("epi0", inp, s, mag, R.EPI_BIAS, False, direct=True)
    run.rows("epi0", inp, s, mag, R.EPI_BIAS, True, sumsq=True)
    run.record()


GROUPED = {640: (320, 0), 321: (320, 128), 450: (320, 256), 577: (320, 320), 512: (256, 0)}       # M -> tile_rows, rem_rows


@pytest.mark.parametrize("M", sorted(GROUPED))
def test_grouped_launch(dev, bank, M):
    """ops.gemm_grouped against the float64 product itself, per group: G = 3, N = 512, n_split = 256, K in {64, 192}, with
    and without the bias table and the statistics; M picks the body (no remainder, the 128-row, 256-row and full-height
    remainder bodies, the 256-row tile).  Group strides exceed a group's output; NaN (statistics: canary) in between."""
    from mlx_video_amd import ops
    G, N = 3, 2 * NS
    T = M if M % 2 else M // 2
    nb, ld2, ldo, P = M // T, (T + 3) // 4 * 4 + 4, NS + 4, NS // 64
    worst = {}
    for K in (64, 192):
        pl = ops.gemm_grouped_plan(G, M, N, K, n_split=NS, out_tokens_per_batch=T)
        assert (pl.tile_rows, pl.rem_rows) == GROUPED[M] and pl.col_tiles == N // 256, pl
        groups = []
        a = bank(M, N, K)[0].a
        for g in range(G):                               # one A, G panels: group g's W and bias come from another seed
            inp = R.inputs(M, N, K, M * 7 + N * 3 + K + 1000 * (g + 1), dev)
            s, mag = R.product(a, inp.w)
            inp.a = a
            R.premises(inp, s, mag)
            groups.append((inp, s, mag))
        w_tab = ops.pointer_table([inp.w for inp, _, _ in groups])
        b_tab = ops.pointer_table([inp.b for inp, _, _ in groups])
        for with_bias, with_ss in ((True, True), (False, False), (True, False), (False, True)):
            runs = []
            for _ in range(2):
                k = R.Frame((G, M, NS), (M * ldo + 12, ldo, 1), dev)
                v = R.Frame((G, nb, NS, T), (nb * NS * ld2 + 8, NS * ld2, ld2, 1), dev, lead=4)
                ss = R.Frame((G, M, P), (M * (P + 1) + 7, P + 1, 1), dev, dtype=torch.float32, lead=0, sentinel=-7.0)
                ops.gemm_grouped(a, w_tab, b_tab if with_bias else None, N, out=k.view, out2=v.view, n_split=NS, out_tokens_per_batch=T,
                                 sumsq=ss.view if with_ss else None)
                runs.append((k, v, ss))
            torch.cuda.synchronize()
            for f0, f1 in zip(*runs):
                assert torch.equal(_bits(f0.buf), _bits(f1.buf)), "two runs differ"
                assert f0.intact(), "wrote outside a group's output"
            k, v, ss = runs[0]
            if not with_ss:
                assert bool((ss.buf == -7.0).all())
            for g, (inp, s, mag) in enumerate(groups):
                name = f"grouped M={M} K={K} bias={with_bias} group {g}"
                bias = inp.b if with_bias else None
                tile = (pl.tile_rows, 256)
                wk = R.check(name + " k", *R.bound(0, k.view[g], s[:, :NS], mag[:, :NS], K, None if bias is None else bias[:NS]), tile=tile)
                wv = R.check(name + " vt", *R.bound(0, R.vt_rows(v.view[g], T), s[:, NS:], mag[:, NS:], K, None if bias is None else bias[NS:]), tile=tile)
                worst["k"], worst["vt"] = max(worst.get("k", 0.0), wk), max(worst.get("vt", 0.0), wv)
                if with_ss:
                    worst["sumsq"] = max(worst.get("sumsq", 0.0), R.check(name + " sumsq", *R.sumsq_bound(ss.view[g], k.view[g])))
    for tag, w in sorted(worst.items()):
        print(f"grouped M={M} {tag}: worst d / bound = {w:.3f}")
        parity.auto(w, 1.0, tag=tag)
