"""``ops.sample_rows`` (csrc/sample.hip) alone on the device: temperature 0 equal to ``gemma.sample_tokens`` exactly, every
draw at temperature 0.7 and 1.5 inside ``ref_gemma_sample.admissible`` (no draw exempt), the decode state's bookkeeping, the
no-op past the last draw, and the token's independence of the batch.

Shapes: V = 8 (one thread of one chunk), 264 (33 threads), 4104 (three chunks, the last one 8 elements) and the model's 262208
(129 chunks, the last one 64 elements), with B = 1, 3 and 8 rows."""
import numpy as np
import pytest
import torch

import ref_gemma_sample as S

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
VS, BS = (8, 264, 4104, 262208), (1, 3, 8)
PATTERN = -77


class State:
    """The sampler's operands on the device, from host values: logits (B,V) fp32 holding bf16 numbers, a history per row."""

    def __init__(self, dev, logits, history, n_max=4, n=0, pos=10, done=None, eos=(), uniforms=None, hist_cap=None, ld=None):
        from mlx_video_amd import ops
        B, V = logits.shape
        self.B, self.V, self.n_max = B, V, n_max
        buf = torch.full((B, ld or V), 9.0, dtype=BF)
        buf[:, :V] = torch.as_tensor(logits).to(BF)
        self.logits = buf.to(dev)[:, :V]
        hist_cap = hist_cap or max(len(h) for h in history) + n_max + 1
        hist = torch.full((B, hist_cap), PATTERN, dtype=torch.int32)
        for b, h in enumerate(history):
            hist[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
        i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).to(dev)          # noqa: E731
        self.ctl, self.done = i32([n, pos, B]), i32(done if done is not None else [0] * B)
        self.next_ids, self.history, self.hist_len = i32([PATTERN] * B), hist.to(dev), i32([len(h) for h in history])
        self.tokens_out = torch.full((B, n_max), PATTERN, dtype=torch.int32, device=dev)
        self.eos = i32(list(eos))
        self.uniforms = None if uniforms is None else torch.as_tensor(uniforms, dtype=torch.float32).to(dev)
        self.workspace = torch.full((ops.sample_workspace_floats(B, V),), float(PATTERN), dtype=torch.float32, device=dev)

    def run(self, temperature, penalty=1.0, rep_ctx=0, **kw):
        from mlx_video_amd import ops
        ops.sample_rows(self.logits, self.ctl, self.done, self.next_ids, self.history, self.hist_len, self.tokens_out, self.eos,
                        self.uniforms, self.workspace, temperature=temperature, penalty=penalty, rep_ctx=rep_ctx, **kw)
        torch.cuda.synchronize()
        return self.tokens_out.cpu()

    def host(self):
        return {k: getattr(self, k).cpu().clone() for k in ("ctl", "done", "next_ids", "history", "hist_len", "tokens_out", "workspace")}


def _greedy_rows(V, seed):
    """The five rows of the greedy cases: plain, maximum at index 0, at V - 1, an exact three-way tie, all negative."""
    g = np.random.default_rng(seed)
    base = S.bf16_round(g.standard_normal(V) * 3)
    rows = [base, base.copy(), base.copy(), base.copy(), S.bf16_round(-np.abs(base) - 1)]
    rows[1][0], rows[2][V - 1] = 50.0, 50.0
    rows[3][[1, V // 2, V - 2]] = 40.0
    return rows


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_greedy_equals_sample_tokens(dev, V, B):
    """Temperature 0 against ``sample_tokens`` on the widened logits, exactly: the maximum at index 0 and at V - 1, a tie (the
    lowest index wins), all-negative logits (the penalty multiplies), with an empty context and with the last 64 of a 70-id
    history that holds the row's top ids several times, at penalty 1, 1.3 and 100.  The rows rotate through the batch, so each of
    the five meets each (context, penalty); the logits sit in a wider buffer (ld = V + 8)."""
    from mlx_video_amd.gemma import sample_tokens
    rows = _greedy_rows(V, seed=V + B)
    g = np.random.default_rng(V)
    hist = []
    for r in rows:
        top = [int(t) for t in np.argsort(r)[-3:]]
        hist.append([int(t) for t in g.integers(0, V, 6)] + (top * 22)[:61] + [1, V // 2, V - 2])          # 70 ids, the last 64 count
    for shift in range(5 if B < 5 else 1):
        pick = [(b + shift) % 5 for b in range(B)]
        lg = np.stack([rows[i] for i in pick])
        for history, rep_ctx in (([[] for _ in pick], 20), ([hist[i] for i in pick], 64)):
            for pen in (1.0, 1.3, 100.0):
                st = State(dev, lg, history, ld=V + 8)
                got = st.run(0.0, pen, rep_ctx)[:, 0]
                want = sample_tokens(torch.from_numpy(lg), [h[-rep_ctx:] for h in history], 0.0, pen, None)
                assert got.tolist() == want.tolist(), (V, B, shift, rep_ctx, pen, got.tolist(), want.tolist())
                assert st.next_ids.cpu().tolist() == want.tolist()


N_DRAWS = 12


def _check_draws(dev, lg, history, temperature, pen, rep_ctx, seed, single=False):
    """N_DRAWS draws of every row with the advance in between - the history, and so the context, grows by the drawn token - each
    token held to admissible(...) of that draw's context and uniform.  Returns the largest admissible set met."""
    B, V = lg.shape
    us = torch.rand((N_DRAWS, B), generator=torch.Generator().manual_seed(seed))
    st = State(dev, lg, history, n_max=N_DRAWS, uniforms=us)
    for _ in range(N_DRAWS):
        toks = st.run(temperature, pen, rep_ctx)
    assert st.ctl.cpu().tolist() == [N_DRAWS, 10 + N_DRAWS, B]
    largest = 0
    for b in range(B):
        h = list(history[b])
        for n in range(N_DRAWS):
            ctx = h[-rep_ctx:] if rep_ctx else []
            ok = S.admissible(lg[b], ctx, pen, temperature, float(us[n, b]))
            t = int(toks[b, n])
            assert t in ok, (V, B, b, n, t, sorted(ok)[:5], float(us[n, b]))
            if single:
                assert len(ok) == 1, (V, b, n, sorted(ok))
            largest = max(largest, len(ok))
            h.append(t)
        assert st.history.cpu()[b, :len(h)].tolist() == h and int(st.hist_len.cpu()[b]) == len(h)
    return largest


@pytest.mark.parametrize("temperature", [0.7, 1.5])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("V", VS)
def test_every_draw_is_admissible(dev, V, B, temperature):
    """Normal logits of std 3 rounded to bf16, penalty 1.3 over the last 20 ids of a history that starts with the row's top
    tokens: every draw of every row lies in the float64 admissible set; where the set holds several tokens any of them passes."""
    g = np.random.default_rng(V * 10 + B)
    lg = S.bf16_round(g.standard_normal((B, V)) * 3)
    history = [[int(t) for t in np.argsort(lg[b])[-5:]] * 2 for b in range(B)]
    largest = _check_draws(dev, lg, history, temperature, 1.3, 20, seed=V + B)
    print(f"V {V} B {B} T {temperature}: largest admissible set {largest}")


@pytest.mark.parametrize("temperature", [0.7, 1.5])
@pytest.mark.parametrize("V,at", [(8, 2), (264, 130)])
def test_dominant_tokens_give_single_sets(dev, V, at, temperature):
    """Three dominant neighbours over a floor of no mass: the admissible set is one token except within tol of an edge - a
    2 V tol / S share of the uniforms, below 1e-3 here - and the seeds used give single-token sets at every draw (asserted), so
    the kernel is held to the exact token.  The middle token is penalised, twice over in the history."""
    p, _, _, Ssum, tol = S.cdf64(S.dominant_logits(V, at), [at + 1], 1.3, temperature)
    assert 2 * V * tol / Ssum < 1e-3
    for B in BS:
        lg = np.stack([S.dominant_logits(V, at if b % 2 == 0 else at - 1, values=(4.0, 3.0, 3.5) if b % 3 else (3.5, 4.0, 3.0)) for b in range(B)])
        history = [[at + 1, 0, at + 1] for _ in range(B)]
        assert _check_draws(dev, lg, history, temperature, 1.3, 20, seed=100 + V + B, single=True) == 1


def test_bookkeeping(dev):
    """n selects the uniform row and the output column; a done row writes -1 and keeps next_ids / history; an EOS sets done; the
    advance counts the rows not finished; nothing else is touched."""
    V, B, at = 264, 3, 130
    lg = np.stack([S.dominant_logits(V, at)] * B)
    us = torch.tensor([[0.05] * B, [0.99] * B, [0.65, 0.65, 0.97], [0.05] * B])          # the tokens of logit 4.0 / 3.5 / 3.0, 3.0, 3.5 / 4.0
    want = {n: [next(iter(S.admissible(lg[b], [], 1.0, 0.7, float(us[n, b])))) for b in range(B)] for n in range(4)}
    assert want[0] == [at] * 3 and want[1] == [at + 2] * 3 and want[2] == [at + 1, at + 1, at + 2]
    st = State(dev, lg, [[7, 8], [9], [5, 6, 7]], n_max=4, n=2, pos=40, done=[0, 1, 0], eos=(at + 1, 3), uniforms=us)
    before = st.host()
    toks = st.run(0.7)
    after = st.host()
    assert toks[:, 2].tolist() == [at + 1, -1, at + 2] and bool((toks[:, [0, 1, 3]] == PATTERN).all())
    assert after["next_ids"].tolist() == [at + 1, PATTERN, at + 2]
    assert after["hist_len"].tolist() == [3, 1, 4] and after["history"][0, :4].tolist() == [7, 8, at + 1, PATTERN]
    assert torch.equal(after["history"][1], before["history"][1]) and after["history"][2, :5].tolist() == [5, 6, 7, at + 2, PATTERN]
    assert after["done"].tolist() == [1, 1, 0] and after["ctl"].tolist() == [3, 41, 1]
    # draw without the advance, then the advance alone: the same state
    st2 = State(dev, lg, [[7, 8], [9], [5, 6, 7]], n_max=4, n=2, pos=40, done=[0, 1, 0], eos=(at + 1, 3), uniforms=us)
    st2.run(0.7, advance=False)
    assert st2.ctl.cpu().tolist() == [2, 40, 3] and st2.tokens_out.cpu()[:, 2].tolist() == [at + 1, -1, at + 2]
    st2.run(0.7, draw=False)
    mid = st2.host()
    assert all(torch.equal(mid[k], after[k]) for k in ("ctl", "done", "next_ids", "history", "hist_len", "tokens_out"))
    # the next draw takes uniform row 3 and column 3; row 0 is done now
    toks = st.run(0.7)
    assert toks[:, 3].tolist() == [-1, -1, at] and st.ctl.cpu().tolist() == [4, 42, 1] and st.done.cpu().tolist() == [1, 1, 0]


@pytest.mark.parametrize("temperature", [0.0, 0.7])
@pytest.mark.parametrize("V", [264, 262208])
def test_past_the_last_draw_nothing_is_stored(dev, V, temperature):
    """n == Nmax (and a negative n): every buffer, pre-filled with a pattern, stays bit for bit - the workspace included."""
    B = 3
    lg = S.bf16_round(np.random.default_rng(1).standard_normal((B, V)))
    for n in (4, 5, -1):
        st = State(dev, lg, [[1, 2, 3]] * B, n_max=4, n=n, uniforms=torch.full((4, B), 0.5), eos=(1,))
        before = st.host()
        st.run(temperature, 1.3, 20)
        after = st.host()
        for k in before:
            assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), (n, k)


@pytest.mark.parametrize("V", [4104, 262208])
def test_a_row_alone_gives_its_batch_token(dev, V):
    """The token is a function of the row alone: each row of a batch of 8 run as a batch of one (its own uniform, context and
    history) gives the same token, at temperature 0.7 and 0; two runs of the batch agree."""
    B = 8
    g = np.random.default_rng(V + 1)
    lg = S.bf16_round(g.standard_normal((B, V)) * 3)
    history = [[int(t) for t in g.integers(0, V, 10 + b)] for b in range(B)]
    us = torch.rand((2, B), generator=torch.Generator().manual_seed(V))
    for temperature in (0.7, 0.0):
        runs = []
        for _ in range(2):
            st = State(dev, lg, history, n_max=2, n=1, uniforms=us)
            runs.append(st.run(temperature, 1.3, 20)[:, 1].tolist())
        assert runs[0] == runs[1]
        for b in range(B):
            st = State(dev, lg[b:b + 1], history[b:b + 1], n_max=2, n=1, uniforms=us[:, b:b + 1])
            assert st.run(temperature, 1.3, 20)[0, 1].item() == runs[0][b], (V, temperature, b)
