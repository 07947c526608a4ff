"""Scoring on the GPU (``-m gpu``): the two kernels, token_logprobs, continuation_logprobs and rank_continuations.

The oracle is always float64 ``log_softmax`` on the CPU of the SAME bf16 logits, and the bound is derived, not measured:

    |got - want| <= 2**-13 * max(1, |want|)

Each thread sums at most 64 terms, a tree of 64 lanes and 16 waves follows: the relative error of the sum stays below ~90 * 2**-24
(with 256 threads it would be ~260 * 2**-24 = 1.6e-5); expf and logf add a few ulp each, the final subtraction 2**-24 * |x - lse|.
The sum of these is below 2**-13 with a factor of about 5 to spare: a case that exceeds it means the kernel is wrong.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import lit_parrot_amd as L  # noqa: E402
import retrieval_model as rm  # noqa: E402
from lit_parrot_amd import ops  # noqa: E402
from lit_parrot_amd.config import Config, name_to_config  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import is_linear_key, synthetic_prompt, synthetic_state_dict  # noqa: E402
from oracle import int4 as o4  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
MODEL_SEED = 4321
S_GEN, RETURNED = 96, 90  # with ATTN_SPLIT_KEYS = 32: three splits of 32 slots
BOUND = 2.0 ** -13


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture
def engine_off():
    gb.ENGINE_DEFAULT = False
    yield
    gb.ENGINE_DEFAULT = "auto"


@pytest.fixture
def split_keys_32():
    ops.ATTN_SPLIT_KEYS = 32
    yield
    ops.ATTN_SPLIT_KEYS = 1024


@pytest.fixture
def share_switch():
    default = ops.CANDIDATES_SHARE_LOADS
    yield ops
    ops.CANDIDATES_SHARE_LOADS = default


# ---- the oracle
def oracle_logprobs(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """float64 log_softmax on the CPU of bf16 ``logits`` (M, V) at ``targets`` (M,); NaN for a target outside [0, V)."""
    lp = torch.log_softmax(logits.detach().cpu().double(), dim=-1)
    t = targets.cpu().long()
    inside = (t >= 0) & (t < logits.shape[-1])
    out = lp.gather(1, t.clamp(0, logits.shape[-1] - 1).view(-1, 1)).view(-1)
    return torch.where(inside, out, torch.full_like(out, float("nan")))


def lowest_argmax(logits: torch.Tensor) -> torch.Tensor:
    """The arg-max of every row as argmax_advance takes it: a NaN counts as -inf, the lowest index wins a tie."""
    x = logits.detach().cpu().float()
    x = torch.where(x != x, torch.full_like(x, -math.inf), x)
    first = (x == x.max(dim=-1, keepdim=True).values).int().argmax(dim=-1)  # (the first 1 of a 0/1 row)
    for m in range(x.shape[0]):
        assert int(first[m]) == int((x[m] == x[m].max()).nonzero()[0]), "the oracle's own tie rule"
    return first


def assert_close(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    got, want = got.detach().cpu().double().view(-1), want.double().view(-1)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} entries, expected {tuple(want.shape)}"
    nan = want != want
    assert torch.equal(got != got, nan), f"{what}: NaN entries at {(got != got).nonzero().view(-1).tolist()}, expected at {nan.nonzero().view(-1).tolist()}"
    err = ((got - want).abs() / want.abs().clamp_min(1.0))[~nan]
    worst = float(err.max()) if err.numel() else 0.0
    print(f"{what}: max |got - want| / max(1, |want|) = {worst:.3e} (bound {BOUND:.3e})")
    assert worst <= BOUND, f"{what}: {worst:.3e} exceeds 2**-13"


# ---- 1. token_logprob_rows
SHAPES_V = [8, 264, 1000, 32000, 65024]  # two chunks per thread at most, ragged last chunk round, 4 and 8 chunks per thread
SHAPES_M = [1, 3, 130]


@functools.lru_cache(maxsize=None)
def random_case(V, M):
    """N(0, 4) logits rounded to bf16, random targets (row 0's is its arg-max), and the oracle's answer: computed once per shape."""
    g = gen(1000 * M + V)
    logits = (torch.randn((M, V), generator=g) * 2.0).to(BF)
    targets = torch.randint(0, V, (M,), generator=g, dtype=torch.int64)
    best = lowest_argmax(logits)
    targets[0] = best[0]
    return logits, targets, oracle_logprobs(logits, targets), (best == targets)


def padded(logits: torch.Tensor, ldl: int) -> torch.Tensor:
    """``logits`` on the device as the first V columns of rows ``ldl`` long; the padding holds NaN: reading it would show."""
    M, V = logits.shape
    buf = torch.full((M, ldl), float("nan"), dtype=BF, device=DEV)
    buf[:, :V] = logits.to(DEV)
    return buf[:, :V]


def run_rows(logits_dev: torch.Tensor, targets: torch.Tensor, with_greedy: bool = True):
    M = logits_dev.shape[0]
    lp = torch.full((M + 1,), -7.0, dtype=torch.float32, device=DEV)
    gr = torch.full((M + 1,), -7, dtype=torch.int32, device=DEV) if with_greedy else None
    ops.token_logprob_rows(logits_dev, targets.to(DEV), lp[:M], gr[:M] if with_greedy else None)
    assert float(lp[M]) == -7.0 and (gr is None or int(gr[M]) == -7), "wrote past the last row"
    return lp[:M], (gr[:M] if with_greedy else None)


@pytest.mark.parametrize("V", SHAPES_V)
@pytest.mark.parametrize("M", SHAPES_M)
@pytest.mark.parametrize("pad", [0, 24, 1], ids=["ldl=V", "ldl=V+24", "ldl=V+1"])
def test_token_logprob_rows_random_logits(V, M, pad):
    """ldl = V + 1 gives rows with 2-byte alignment: the element-by-element path (with M = 1 the one row stays aligned)."""
    logits, targets, want, want_greedy = random_case(V, M)
    lp, gr = run_rows(padded(logits, V + pad), targets)
    assert_close(lp, want, f"V={V} M={M} ldl=V+{pad}")
    assert torch.equal(gr.cpu().bool(), want_greedy), "is_greedy"
    lp2, _ = run_rows(padded(logits, V + pad), targets, with_greedy=False)  # is_greedy may be null
    assert torch.equal(lp2, lp)


@pytest.mark.parametrize("V", SHAPES_V)
@pytest.mark.parametrize("pad", [0, 24, 1], ids=["ldl=V", "ldl=V+24", "ldl=V+1"])
def test_token_logprob_rows_special_rows(V, pad):
    g = gen(77 + V)
    base = (torch.randn((V,), generator=g) * 2.0).to(BF)
    spike, lo, hi, nan_at = V // 2, 1, V - 1, 2
    rows, targets, what = [], [], []

    def add(row, t, name):
        rows.append(row), targets.append(t), what.append(name)

    add(torch.full((V,), 1.5, dtype=BF), 0, "equal values, the first index")           # -log V, greedy
    add(torch.full((V,), 1.5, dtype=BF), V - 1, "equal values, the last index")        # -log V, not greedy
    s = torch.full((V,), -80.0, dtype=BF)
    s[spike] = 80.0
    add(s, spike, "on the spike"), add(s, spike - 1, "off the spike")
    two = base.clone()
    two[lo] = two[hi] = 30.0
    add(two, lo, "the lower of two maxima"), add(two, hi, "the higher of two maxima")
    n = base.clone()
    n[nan_at] = float("nan")
    add(n, int(lowest_argmax(n[None])[0]), "a NaN in the row")
    add(base, -1, "target -1"), add(base, V, "target V"), add(base, int(lowest_argmax(base[None])[0]), "a plain row")
    logits, t = torch.stack(rows), torch.tensor(targets, dtype=torch.int64)
    want = oracle_logprobs(logits, t)
    want_greedy = (lowest_argmax(logits) == t)
    lp, gr = run_rows(padded(logits, V + pad), t)
    got = dict(zip(what, zip(lp.tolist(), gr.tolist())))
    assert_close(lp, want, f"V={V} ldl=V+{pad} special rows")
    assert torch.equal(gr.cpu().bool(), want_greedy), got
    for name in ("equal values, the first index", "equal values, the last index"):
        assert abs(got[name][0] + math.log(V)) <= BOUND * max(1.0, math.log(V)), got
    assert got["equal values, the first index"][1] == 1 and got["equal values, the last index"][1] == 0
    assert got["on the spike"] == (0.0, 1) and got["off the spike"] == (-160.0, 0), got
    assert got["the lower of two maxima"][1] == 1 and got["the higher of two maxima"][1] == 0, got
    assert got["the lower of two maxima"][0] == got["the higher of two maxima"][0]
    assert math.isnan(got["a NaN in the row"][0]) and got["a NaN in the row"][1] == 1, got  # (the arg-max skips the NaN)
    for name in ("target -1", "target V"):
        assert math.isnan(got[name][0]) and got[name][1] == 0, got
    assert got["a plain row"][1] == 1 and not math.isnan(got["a plain row"][0])


# ---- 2. logprob_advance_rows
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V,pad", [(1000, 0), (1000, 1), (264, 24), (65024, 0)])
def test_logprob_advance_rows(B, V, pad):
    """Rows at their end (and one past it) are frozen: sentinel outputs and pos untouched; live rows write column pos + 1 only and
    advance by one; tokens are never written.  Two calls: rows that reach their end in the first are frozen in the second."""
    g = gen(5 * B + V)
    Lt = 12
    logits = (torch.randn((B, V), generator=g) * 2.0).to(BF)
    tokens = torch.randint(0, V, (B, Lt), generator=g, dtype=torch.int64)
    pos_l = [(3 * b + 1) % (Lt - 2) for b in range(B)]
    ahead = (2,) if B == 1 else (1, 2, 3, 0)  # frozen: p + 1 >= end, rows 0 and 3 (mod 4); the one row of B = 1 is live once
    end_l = [p + ahead[b % len(ahead)] for b, p in enumerate(pos_l)]
    tokens[0, pos_l[0] + 1] = lowest_argmax(logits)[0]               # (B > 1: row 0 is frozen; its greedy token must not show)
    if B > 1:
        tokens[1, pos_l[1] + 1] = lowest_argmax(logits)[1]           # a live row that scores its arg-max
    dev_logits = padded(logits, V + pad)
    tok_d, pos, end = tokens.to(DEV), torch.tensor(pos_l, dtype=torch.int32, device=DEV), torch.tensor(end_l, dtype=torch.int32, device=DEV)
    lp = torch.full((B, Lt + 3), -7.0, dtype=torch.float32, device=DEV)  # (ldo != ldt)
    gr = torch.full((B, Lt + 3), -7, dtype=torch.int32, device=DEV)
    want_lp, want_gr, want_pos = lp.cpu().clone(), gr.cpu().clone(), list(pos_l)
    best = lowest_argmax(logits)
    for call in range(2):
        live = [b for b in range(B) if want_pos[b] + 1 < end_l[b]]
        assert (0 < len(live) < B) if B > 1 else len(live) == 1 - call, "the case needs live and frozen rows"
        for b in live:
            p1 = want_pos[b] + 1
            t = tokens[b, p1]
            want_lp[b, p1] = float(oracle_logprobs(logits[b:b + 1], t.view(1))[0])
            want_gr[b, p1] = int(best[b] == t)
            want_pos[b] = p1
        ops.logprob_advance_rows(dev_logits, tok_d, pos, end, lp, gr)
        assert pos.tolist() == want_pos, f"call {call}: pos"
        assert torch.equal(tok_d.cpu(), tokens), "tokens were written"
        got_lp, got_gr = lp.cpu(), gr.cpu()
        untouched = want_gr == -7
        assert torch.equal(got_gr, want_gr), f"call {call}: is_greedy (or a column other than pos + 1 was written)"
        assert bool((got_lp[untouched] == -7.0).all()), f"call {call}: a column other than pos + 1 was written"
        assert_close(got_lp[~untouched], want_lp[~untouched], f"B={B} V={V} ldl=V+{pad} call {call}")
    assert int(gr[min(1, B - 1), pos_l[min(1, B - 1)] + 1]) == 1


# ---- 3. token_logprobs
_models = {}


def tiny_model(name, mode, copy=0):
    """The tiny models of tests/test_candidates_gpu.py with positions up to 256 (T = 200 takes the MFMA prompt attention), built
    once per session; ``copy``: a second instance for the batched forward, whose caches are n rows wide."""
    key = (name, mode, copy)
    if key in _models:
        return _models[key]
    if mode == "bnb.nf4":
        from lit_parrot_amd.checkpoint import stream_load

        cfg = Config(**{**name_to_config[name], "intermediate_size": 384, "block_size": 256})
        sd = synthetic_state_dict(cfg, seed=7, dtype=BF)
        with torch.device("cuda"), L.quantization(mode):
            model = L.GPT(cfg)
        model = model.to(BF).eval()
        assert stream_load(model, sd) == []
    else:
        cfg = Config.from_name(name, block_size=256)
        sd = {k: v.to(BF) for k, v in synthetic_state_dict(cfg, MODEL_SEED, perturb=True).items()}
        if mode is not None and mode.startswith("gptq"):
            sd = o4.quantize_state_dict(sd, 128, is_linear_key)
        with L.quantization(mode):
            model = L.GPT(cfg)
        model.load_state_dict(sd, strict=mode is None or mode.startswith("gptq"))  # (LLM.int8 quantises on arrival)
        model = model.to(BF).to(DEV).eval()
    _models[key] = model
    return model


def prompt_of(cfg, T):
    return synthetic_prompt(cfg, T, 9 + T).to(DEV)


SCORED_MODELS = [("tiny-llama", None), ("tiny-neox", None), ("tiny-falcon-mqa", None), ("tiny-llama", "gptq.int4-g128"),
                 ("tiny-llama-hs128", "bnb.nf4"), ("tiny-llama", "bnb.int8")]


@pytest.mark.parametrize("name,mode", SCORED_MODELS)
@pytest.mark.parametrize("T", [2, 33, 200])
def test_token_logprobs_are_the_log_softmax_of_forward(name, mode, T):
    model = tiny_model(name, mode)
    idx = prompt_of(model.config, T)
    with torch.no_grad():
        logits = model(idx[None])[0]  # (T, V) bf16
    lp, greedy = L.token_logprobs(model, idx, return_greedy=True)
    assert lp.dtype == torch.float32 and greedy.dtype == torch.bool and lp.shape == greedy.shape == (T - 1,) and lp.device == idx.device
    assert_close(lp, oracle_logprobs(logits[:-1], idx[1:]), f"{name} {mode} T={T}")
    assert torch.equal(greedy.cpu(), lowest_argmax(logits[:-1]) == idx[1:].cpu())
    unique = (logits[:-1].float().cpu() == logits[:-1].float().cpu().max(-1, keepdim=True).values).sum(-1) == 1  # (torch pins no tie rule)
    assert torch.equal(greedy.cpu()[unique], (logits[:-1].argmax(-1) == idx[1:]).cpu()[unique])
    assert torch.equal(L.token_logprobs(model, idx), lp)
    # a sequence that follows the arg-max is greedy everywhere
    follow = idx.clone()
    follow[1] = lowest_argmax(logits[:1])[0]
    _, g2 = L.token_logprobs(model, follow, return_greedy=True)
    assert bool(g2[0])


def test_perplexity_scores_every_token_but_the_first_once():
    model = tiny_model("tiny-llama", None)
    tokens = prompt_of(model.config, 300)  # longer than block_size = 256
    want = torch.cat([L.token_logprobs(model, tokens[:256]), L.token_logprobs(model, tokens[128:300])[127:]]).double()
    ppl, nll, n = L.perplexity(model, tokens)  # window 256, stride 128: passes [0, 256) and [128, 300)
    assert n == 299 and nll == pytest.approx(-float(want.sum()), rel=1e-12) and ppl == pytest.approx(math.exp(nll / n), rel=1e-12)
    one = L.token_logprobs(model, tokens[:100]).double()
    ppl, nll, n = L.perplexity(model, tokens[:100], window=100, stride=50)  # one pass
    assert n == 99 and nll == pytest.approx(-float(one.sum()), rel=1e-12)
    _, nll2, n2 = L.perplexity(model, tokens[:100], window=40, stride=40)
    assert n2 == 99 and math.isfinite(nll2) and abs(nll2 - nll) < 0.05 * nll  # (less context: another number, the same size)


# ---- 4. continuation_logprobs
def score_sessions(model):
    return [s for k, s in model._decode_sessions.items() if k[0] == "score"]


def forced_forward(model, prompt, rows, S, free_from=None):
    """Teacher forcing through the public batched GPT.forward with a KV cache: the prompt prefilled into B slices, then (B, 1) tokens.
    ``rows``: (B, n) tokens behind the prompt.  Returns the logits that score them, (B, n, V) on the CPU: entry 0 from the prompt's
    last row, entry i from the step that fed token i - 1.  ``free_from`` = k: from entry k on, a row is fed its own arg-max (the lowest
    index on ties) instead of the given token; the tokens fed or chosen are returned as well."""
    B, n = rows.shape
    T = prompt.numel()
    rows = rows.clone().to(DEV)
    model.reset_cache()
    out = []
    with torch.no_grad():
        logits = model(prompt.to(DEV)[None].expand(B, -1).contiguous(), S, torch.arange(T, device=DEV))[:, -1]
        for i in range(n):
            out.append(logits.cpu())
            if free_from is not None and i >= free_from:
                rows[:, i] = lowest_argmax(logits).to(DEV)
            if i + 1 < n:
                logits = model(rows[:, i:i + 1].contiguous(), S, torch.tensor([T + i], device=DEV))[:, 0]
    model.reset_cache()
    return torch.stack(out, dim=1), rows.cpu()


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("share", [True, False])
def test_greedy_rows_are_greedy_and_one_replaced_token_shows_alone(engine_off, split_keys_32, share_switch, n, share):
    """(a) The rows of generate_candidates(top_k=1) score greedy everywhere.  One token replaced in the middle of one row - the row
    behind it continued greedily from the replaced token, through the batched forward, whose rows are the shared-prefix rows bit for
    bit - makes exactly that position not greedy in that row and leaves the other rows bit-identical."""
    cand, batch = tiny_model("tiny-llama", None), tiny_model("tiny-llama", None, copy=1)
    ops.CANDIDATES_SHARE_LOADS = share
    T = 70
    p = prompt_of(cand.config, T)
    rows = L.generate_candidates(cand, p, n, RETURNED, S_GEN, top_k=1)
    conts = [r[T:] for r in rows]
    lp, gr = L.continuation_logprobs(cand, p, conts, S_GEN, return_greedy=True)
    assert len(lp) == len(gr) == n
    for b in range(n):
        assert lp[b].shape == gr[b].shape == (RETURNED - T,) and lp[b].dtype == torch.float32 and gr[b].dtype == torch.bool
        assert bool(gr[b].all()), f"row {b}: not greedy at {(~gr[b]).nonzero().view(-1).tolist()}"
        assert bool((lp[b] <= 0).all()) and torch.equal(lp[b], lp[0])  # (greedy rows of one prompt are one row)
    r, k = n // 2, (RETURNED - T) // 2
    changed = conts[r].clone()
    changed[k] = (changed[k] + 1) % cand.config.vocab_size
    two = torch.stack([changed, changed]).cpu()  # (two rows: the batched pass of GPT.forward)
    _, freed = forced_forward(batch, p, two, S_GEN, free_from=k + 1)
    assert torch.equal(freed[0], freed[1]) and torch.equal(freed[0, :k + 1], changed[:k + 1].cpu())
    changed = freed[0].to(DEV)
    conts2 = [changed if b == r else c for b, c in enumerate(conts)]
    lp2, gr2 = L.continuation_logprobs(cand, p, conts2, S_GEN, return_greedy=True)
    want = torch.ones(RETURNED - T, dtype=torch.bool)
    want[k] = False
    assert torch.equal(gr2[r].cpu(), want), f"row {r}: not greedy at {(~gr2[r]).nonzero().view(-1).tolist()}, expected at [{k}]"
    assert torch.equal(lp2[r][:k], lp[r][:k]) and float(lp2[r][k]) <= float(lp[r][k])
    for b in range(n):
        if b != r:
            assert torch.equal(lp2[b], lp[b]) and torch.equal(gr2[b], gr[b]), f"row {b} changed with row {r}"


@pytest.mark.parametrize("name,mode", [("tiny-llama", None), ("tiny-falcon-mqa", None), ("tiny-llama", "gptq.int4-g128")])
@pytest.mark.parametrize("share", [True, False])
def test_continuation_values_against_the_batched_forward(engine_off, split_keys_32, share_switch, name, mode, share):
    """(b) Three continuations of 5 tokens behind a 40-token prompt against teacher forcing through GPT.forward: only the kernel's
    error is in play."""
    cand, batch = tiny_model(name, mode), tiny_model(name, mode, copy=1)
    ops.CANDIDATES_SHARE_LOADS = share
    cfg = cand.config
    p = prompt_of(cfg, 40)
    conts = torch.stack([synthetic_prompt(cfg, 5, 300 + b) for b in range(3)])
    logits, _ = forced_forward(batch, p, conts, 64)
    lp, gr = L.continuation_logprobs(cand, p, list(conts.to(DEV)), 64, return_greedy=True)
    for b in range(3):
        assert_close(lp[b], oracle_logprobs(logits[b], conts[b]), f"{name} {mode} share={share} row {b}")
        assert torch.equal(gr[b].cpu(), lowest_argmax(logits[b]) == conts[b])
    order, totals = L.rank_continuations(cand, p, list(conts.to(DEV)), 64)
    assert torch.equal(totals, torch.stack([x.sum() for x in lp])) and order == sorted(range(3), key=lambda b: -float(totals[b]))
    order, means = L.rank_continuations(cand, p, list(conts.to(DEV)), 64, length_normalize=True)
    assert torch.equal(means, torch.stack([x.mean() for x in lp]))


@pytest.mark.parametrize("share", [True, False])
def test_ragged_continuations(engine_off, split_keys_32, share_switch, share):
    """(c) Lengths 1, 4 and 9: a row's first k entries are the entries of the call with every row cut to k."""
    model = tiny_model("tiny-llama", None)
    ops.CANDIDATES_SHARE_LOADS = share
    cfg = model.config
    p = prompt_of(cfg, 70)
    conts = [synthetic_prompt(cfg, n, 500 + n).to(DEV) for n in (1, 4, 9)]
    lp, gr = L.continuation_logprobs(model, p, conts, S_GEN, return_greedy=True)
    assert [x.numel() for x in lp] == [1, 4, 9] == [x.numel() for x in gr]
    assert all(bool(torch.isfinite(x).all()) and bool((x < 0).all()) for x in lp)
    for k in (1, 4):
        cut_lp, cut_gr = L.continuation_logprobs(model, p, [c[:k] for c in conts], S_GEN, return_greedy=True)
        for b, c in enumerate(conts):
            m = min(k, c.numel())
            assert cut_lp[b].numel() == m
            assert torch.equal(cut_lp[b], lp[b][:m]) and torch.equal(cut_gr[b], gr[b][:m]), f"k={k} row {b}"
    # a row alone is the row among others
    alone = L.continuation_logprobs(model, p, [conts[2]], S_GEN)
    assert torch.equal(alone[0], lp[2])
    # and the concatenation through token_logprobs agrees within the two paths' bf16 logits (a loose check of the plumbing)
    whole = L.token_logprobs(model, torch.cat([p, conts[2]]))[-9:]
    assert float((whole - lp[2]).abs().max()) < 0.1


def test_a_second_call_reuses_the_captured_session(engine_off, split_keys_32):
    """(d)"""
    model = tiny_model("tiny-llama", None)
    model.__dict__.pop("_decode_sessions", None)
    cfg = model.config
    conts = [synthetic_prompt(cfg, 6, 600 + b).to(DEV) for b in range(3)]
    first = L.continuation_logprobs(model, prompt_of(cfg, 70), conts, S_GEN)
    (sess,) = score_sessions(model)
    graph = sess.graph
    assert graph is not None and sess.S_tail == 64 and isinstance(sess, gb.ScoringSession)
    L.continuation_logprobs(model, prompt_of(cfg, 40), [c[:3] for c in conts], S_GEN)  # another prompt and other lengths: the same step
    again = L.continuation_logprobs(model, prompt_of(cfg, 70), conts, S_GEN)
    assert score_sessions(model) == [sess] and sess.graph is graph, "the session was rebuilt"
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    L.generate_candidates(model, prompt_of(cfg, 70), 3, RETURNED, S_GEN, top_k=1)  # the candidates keep their own key
    assert score_sessions(model) == [sess] and len(model._decode_sessions) == 2
    # captured replay == eager launches
    model._decode_sessions.clear()
    orig = gb.ScoringSession.__init__
    try:
        gb.ScoringSession.__init__ = lambda self, *a, **k: orig(self, *a, **{**k, "use_graph": False})
        eager = L.continuation_logprobs(model, prompt_of(cfg, 70), conts, S_GEN)
        assert score_sessions(model)[0].graph is None
    finally:
        gb.ScoringSession.__init__ = orig
        model._decode_sessions.clear()
    assert all(torch.equal(a, b) for a, b in zip(first, eager)), "hipGraph replay and eager launches disagree"


def test_capture_restores_what_the_scoring_step_writes():
    """After an 8-token prompt in a window of 32: capture() leaves tokens, pos, end, the tails, the shared cache and both outputs bit
    for bit as they were, a second capture() keeps the graph, and a step then advances the live rows and scores one column."""
    cfg = Config.from_name("tiny-llama")
    model = L.GPT(cfg)
    model.load_state_dict({k: v.to(BF) for k, v in synthetic_state_dict(cfg, MODEL_SEED, perturb=True).items()}, strict=True)
    model = model.to(BF).to(DEV).eval()
    sess = gb.ScoringSession(model, 2, 32, gb.candidate_tail_slots(32, 8))
    with torch.no_grad():
        sess.logprob.fill_(-7.0), sess.is_greedy.fill_(-7)
        sess.prefill(prompt_of(cfg, 8), [synthetic_prompt(cfg, 5, 3).to(DEV), synthetic_prompt(cfg, 1, 4).to(DEV)])

        def snapshot():
            named = {n: getattr(sess, n) for n in ("tokens", "pos", "end", "logprob", "is_greedy", "prefix_len")}
            for i, (k, v) in enumerate(sess.caches + sess.tails):
                named[f"k{i}"], named[f"v{i}"] = k, v
            return {n: t.clone() for n, t in named.items()}

        before = snapshot()
        assert before["pos"].tolist() == [7, 7] and before["end"].tolist() == [13, 9] and bool(before["k0"].any())
        sess.capture()
        after = snapshot()
        for n in before:
            assert torch.equal(before[n], after[n]), f"capture() changed {n}"
        graph = sess.graph
        assert graph is not None
        sess.capture()
        assert sess.graph is graph, "captured twice"
        sess.score_first()
        assert sess.pos.tolist() == [8, 8] and bool((sess.logprob[:, 8] != -7.0).all()) and int((sess.logprob != -7.0).sum()) == 2
        sess.step()
        assert sess.pos.tolist() == [9, 8], "row 1 is at its end"
        assert int((sess.logprob != -7.0).sum()) == 3 and float(sess.logprob[0, 9]) != -7.0
        assert torch.equal(sess.tokens, before["tokens"]), "the step wrote tokens"


# ---- 5. the scored rows read the shared cache
@pytest.mark.parametrize("share", [True, False])
def test_ranking_follows_the_needle_in_the_shared_cache(engine_off, split_keys_32, share_switch, share):
    """tests/retrieval_model.py: behind a prompt that holds a needle and ends in its class's query, the automaton's continuation
    ranks first among 8 that differ from it in the answer token; with the needle removed, the NONE continuation does."""
    ops.CANDIDATES_SHARE_LOADS = share
    cfg, sd, ids = rm.retrieval_model("tiny-llama")
    model = L.GPT(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(BF).to(DEV).eval()
    T, S, b, a = 70, 96, 1, 5
    assert ids.A >= 8
    prompt = [ids.fill[(3 * i) % len(ids.fill)] for i in range(T)]
    prompt[T - 1] = ids.Q[b]
    with_needle = list(prompt)
    with_needle[10] = ids.N[b][a]  # in the first split of 32 slots: a shared split when the switch is on
    for toks, answer in ((with_needle, ids.N[b][a]), (prompt, ids.NONE[b])):
        tail = rm.automaton(ids, toks, T + 6, S)[T:]
        assert tail[0] == answer
        others = [x for x in ids.N[b] if x != answer][:7]
        conts = [torch.tensor(tail)] + [torch.tensor([x] + tail[1:]) for x in others]
        for place in (0, 3, 7):  # wherever the right one stands
            order = list(range(1, 8))
            order.insert(place, 0)
            ranked, totals = L.rank_continuations(model, torch.tensor(toks), [conts[i] for i in order], S)
            assert ranked[0] == place, f"needle {'present' if toks is with_needle else 'absent'}: ranked {ranked}, totals {totals.tolist()}"
            _, gr = L.continuation_logprobs(model, torch.tensor(toks), [conts[i] for i in order], S, return_greedy=True)
            assert bool(gr[place].all()) and not any(bool(g[0]) for i, g in enumerate(gr) if i != place)
