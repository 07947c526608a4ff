"""A hand-built model whose TOKENS are its attention's answer (plain functions, shared by test_retrieval_*.py).

With N(0, 0.02) weights the softmax over a few hundred keys is nearly flat and the logits barely depend on which keys
were read (testing section).  Here layer 0 is wired so that after a query token ``Q[b]`` the next token is
decided by ONE key slot: the most recent "needle" ``N[b, a]`` of class ``b`` inside the window - the model emits that
needle, or ``NONE[b]`` when the window holds none.  After a needle or a NONE token it emits the next class's query, so
greedy generation is a closed-form automaton over the token list (``expected_next`` / ``automaton``), and a lost, extra
or misplaced key flips a token.

Residual subspaces (disjoint index ranges of n_embd): class 8 | query 8 | answer B*A | constant 1 | not-found 8 | filler.
Every token embeds as exactly two entries of 1.0, so the input norm scales all tokens alike:
    N[b, a]: class b, answer b*A + a        Q[b]: query b, constant        NONE[b]: not-found b, a filler dim
    fillers: two filler dims
Layer 0: class b lives on query head b % n_head, in head dimension d(b); that head's Q row d(b) reads query dim b and the K
row d(b) of the head's K/V group reads class dim b (gain GAIN each; the other groups' rows stay zero, so a key or value read
from the wrong group finds nothing): a needle of the class scores GAIN^2 n_embd / (2 sqrt(hs)) >= 24
behind the 1 / sqrt(hs) scale, every other key ~0.  d(b), distinct among the classes of one K/V group, is an unrotated
dimension under a partial rotary width, else the first element of one of the slowest rotary pairs (angle ~1.3e-4 rad per position: a match 1200 positions back keeps > 0.9
of its score).  The group's V rows copy the answer dims of its classes into head dims b*A + a and proj writes head h's dims back to the answer
subspace (gain PROJ_GAIN) for the classes head h serves ONLY - the flat attention of the other heads then leaks nothing.
All MLP weights and all later layers are zero (identity; they still run the step's whole op table); norm weights are 1.
lm_head: N[b, a] reads answer b*A + a and query b; NONE[b] reads the constant and query b; Q[(b+1) % B] reads class b and
not-found b with weight 3.
"""
import math
import random
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

N_CLASS_DIMS = 8  # widths of the class, query and not-found subspaces: at most 8 classes
GAIN = math.sqrt(3.0)
PROJ_GAIN = 0.25
Q_HEAD_WEIGHT = 3.0


def default_classes(cfg) -> Tuple[int, int]:
    """(B, A) that probe every query head of ``cfg``: B >= n_head classes, B * A <= head_size answers."""
    B = max(4, cfg.n_head)
    assert B <= N_CLASS_DIMS, f"{cfg.name}: {cfg.n_head} heads need more than {N_CLASS_DIMS} classes"
    return B, min(16, cfg.head_size // B)


def class_group(cfg, b: int) -> int:
    """The K/V group of the query head (b % n_head) that serves class ``b``."""
    return (b % cfg.n_head) // (cfg.n_head // cfg.n_query_groups)


def class_head_dim(cfg, b: int) -> int:
    """d(b): the head dimension class ``b`` is matched in - distinct among the classes whose heads share a K/V group (they
    share the K rows), numbered from the slowest rotary pair."""
    j = sum(1 for o in range(b) if class_group(cfg, o) == class_group(cfg, b))
    n_elem = cfg.rope_n_elem
    if n_elem < cfg.head_size:
        return n_elem + j  # never rotated
    return n_elem // 2 - 1 - j  # first element of the j-th slowest pair (its partner: n_elem - 1 - j)


def retrieval_state_dict(cfg, B: int = 4, A: int = 16, n_fill: int = 100):
    """fp32 state dict of ``cfg`` (the reference's keys, in ``synthetic_state_dict``'s order) and the token-id layout."""
    c = cfg
    hs, d = c.head_size, c.n_embd
    assert B <= N_CLASS_DIMS and B * A <= hs, (B, A, hs)
    o_class, o_query, o_answer = 0, N_CLASS_DIMS, 2 * N_CLASS_DIMS
    o_const = o_answer + B * A
    o_none = o_const + 1
    o_fill = o_none + N_CLASS_DIMS
    n_fdims = d - o_fill
    assert n_fdims >= 2 and n_fdims * (n_fdims - 1) // 2 >= n_fill, f"n_embd={d} leaves {n_fdims} filler dims"
    n_vocab = n_fill + B * A + 2 * B
    assert n_vocab <= c.vocab_size

    ids = SimpleNamespace(B=B, A=A, fill=list(range(n_fill)),
                          N=[[n_fill + b * A + a for a in range(A)] for b in range(B)],
                          Q=[n_fill + B * A + b for b in range(B)],
                          NONE=[n_fill + B * A + B + b for b in range(B)], n_vocab=n_vocab)
    ids.kind = {}  # token id -> ("fill",) | ("N", b, a) | ("Q", b) | ("NONE", b)
    for t in ids.fill:
        ids.kind[t] = ("fill",)
    for b in range(B):
        ids.kind[ids.Q[b]] = ("Q", b)
        ids.kind[ids.NONE[b]] = ("NONE", b)
        for a in range(A):
            ids.kind[ids.N[b][a]] = ("N", b, a)

    V = c.padded_vocab_size
    wte = torch.zeros(V, d)
    lm = torch.zeros(V, d)
    pairs = [(i, j) for i in range(n_fdims) for j in range(i + 1, n_fdims)]
    step = max(1, len(pairs) // n_fill)
    for n, t in enumerate(ids.fill):
        i, j = pairs[n * step]
        wte[t, o_fill + i] = wte[t, o_fill + j] = 1.0
    for b in range(B):
        wte[ids.Q[b], o_query + b] = wte[ids.Q[b], o_const] = 1.0
        wte[ids.NONE[b], o_none + b] = wte[ids.NONE[b], o_fill + b % n_fdims] = 1.0
        lm[ids.NONE[b], o_const] = lm[ids.NONE[b], o_query + b] = 1.0
        nxt = ids.Q[(b + 1) % B]
        lm[nxt, o_class + b] = lm[nxt, o_none + b] = Q_HEAD_WEIGHT
        for a in range(A):
            t = ids.N[b][a]
            wte[t, o_class + b] = wte[t, o_answer + b * A + a] = 1.0
            lm[t, o_answer + b * A + a] = lm[t, o_query + b] = 1.0

    # layer 0: rows of the fused QKV Linear are [q_per_kv query heads, K, V] per group (model.py:208-211)
    qkv = torch.zeros(c.qkv_size, d)
    proj = torch.zeros(d, d)
    q_per_kv = c.n_head // c.n_query_groups

    def row(g: int, slot: int, dim: int) -> int:
        return (g * (q_per_kv + 2) + slot) * hs + dim

    for b in range(B):
        h = b % c.n_head
        db = class_head_dim(c, b)
        g = class_group(c, b)
        qkv[row(g, h % q_per_kv, db), o_query + b] = GAIN
        qkv[row(g, q_per_kv, db), o_class + b] = GAIN
        for a in range(A):
            i = b * A + a
            qkv[row(g, q_per_kv + 1, i), o_answer + i] = 1.0
            proj[o_answer + i, h * hs + i] = PROJ_GAIN

    sd: Dict[str, torch.Tensor] = {}

    def norm(prefix: str) -> None:
        sd[prefix + ".weight"] = torch.ones(d)
        if c._norm_class == "LayerNorm":
            sd[prefix + ".bias"] = torch.zeros(d)

    def linear(prefix: str, w: torch.Tensor) -> None:
        sd[prefix + ".weight"] = w
        if c.bias:
            sd[prefix + ".bias"] = torch.zeros(w.shape[0])

    sd["lm_head.weight"] = lm
    sd["transformer.wte.weight"] = wte
    for i in range(c.n_layer):
        p = f"transformer.h.{i}"
        norm(f"{p}.norm_1")
        linear(f"{p}.attn.attn", qkv if i == 0 else torch.zeros(c.qkv_size, d))
        linear(f"{p}.attn.proj", proj if i == 0 else torch.zeros(d, d))
        if not c.shared_attention_norm:
            norm(f"{p}.norm_2")
        if c._mlp_class == "LLaMAMLP":
            linear(f"{p}.mlp.fc_1", torch.zeros(c.intermediate_size, d))
            linear(f"{p}.mlp.fc_2", torch.zeros(c.intermediate_size, d))
        else:
            linear(f"{p}.mlp.fc", torch.zeros(c.intermediate_size, d))
        linear(f"{p}.mlp.proj", torch.zeros(d, c.intermediate_size))
    norm("transformer.ln_f")
    return sd, ids


# ------------------------------------------------------------------------------------------------ the rule
def expected_next(ids, tokens: Sequence[int], S: int) -> Optional[int]:
    """The token the model must emit after ``tokens`` (the last one is the row being decoded) with a window of the last
    ``S`` positions; None after a filler, where every logit is ~0 and nothing is decided."""
    kind = ids.kind[int(tokens[-1])]
    if kind[0] == "fill":
        return None
    if kind[0] in ("N", "NONE"):
        return ids.Q[(kind[1] + 1) % ids.B]
    b = kind[1]
    window = tokens[max(0, len(tokens) - S):]
    found = [ids.kind[int(t)][2] for t in window if ids.kind[int(t)][0] == "N" and ids.kind[int(t)][1] == b]
    assert len(set(found)) <= 1, f"the window holds different answers {sorted(set(found))} of class {b}"
    return ids.N[b][found[-1]] if found else ids.NONE[b]


def automaton(ids, prompt_tokens: Sequence[int], n: int, S: int) -> List[int]:
    """``prompt_tokens`` continued greedily to ``n`` tokens in all."""
    out = [int(t) for t in prompt_tokens]
    while len(out) < n:
        t = expected_next(ids, out, S)
        assert t is not None, "a free-running prompt must end in a query, a needle or a not-found token"
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------ scenarios
class Scenario(SimpleNamespace):
    """tokens: the whole forced sequence; T: prompt length; S: window.  Row p (T-1 <= p < len(tokens)) decodes tokens[p];
    ``expect(p)`` is the token it must emit (None: unchecked)."""

    def expect(self, ids, p: int) -> Optional[int]:
        return expected_next(ids, self.tokens[: p + 1], self.S)

    @property
    def rows(self) -> range:
        return range(self.T - 1, len(self.tokens))


def _fillers(ids, n: int, rng: random.Random) -> List[int]:
    return [rng.choice(ids.fill) for _ in range(n)]


def _query_walk(ids, first: int, n: int) -> List[int]:
    return [ids.Q[(first + i) % ids.B] for i in range(n)]


def edge_scenarios(ids, T: int, S: int, slots: Sequence[int], seed: int = 0) -> List[Scenario]:
    """One needle per class per scenario at ``slots`` (each < T), B - 1 slots per scenario; the prompt ends in a query (or in the
    needle when slot T-1 is asked for), then every class is queried in turn by forced tokens, one class absent per scenario
    in rotation so that NONE answers are checked behind the same windows."""
    rng = random.Random(seed)
    slots = sorted(set(int(s) for s in slots))
    assert all(0 <= s < T for s in slots)
    out = []
    per = ids.B - 1  # one class has no needle
    for n, i in enumerate(range(0, len(slots), per)):
        chunk = slots[i:i + per]
        absent = n % ids.B
        classes = [b for b in range(ids.B) if b != absent]
        rng.shuffle(classes)
        toks = _fillers(ids, T, rng)
        for s, b in zip(chunk, classes):
            toks[s] = ids.N[b][rng.randrange(ids.A)]
        if T - 1 not in chunk:
            toks[T - 1] = ids.Q[rng.randrange(ids.B)]
        toks += _query_walk(ids, rng.randrange(ids.B), ids.B + 1)
        out.append(Scenario(tokens=toks, T=T, S=S))
    return out


def engine_split_per(n_valid: int, hs: int, max_splits: int = 8, keys_per_split: int = 32) -> Tuple[int, int]:
    """(splits in use, keys per split) of the stream engine's attention op at a row that sees ``n_valid`` keys, restated from the
    comment on eng_keys (csrc/engine.hip): one CU per 32 keys, doubled up to the 8 CUs reserved per (virtual) group; the keys
    are dealt in ranges of ceil(n_valid / splits) rounded up to whole 1-KiB pieces of 512 / hs keys; split s holds
    [s * per, (s + 1) * per)."""
    ns = 1
    while ns < max_splits and ns * keys_per_split < n_valid:
        ns *= 2
    kpp = 512 // hs
    per = -(-n_valid // ns)
    return ns, -(-per // kpp) * kpp


def edge_slots(T: int, S: int, hs: int, n_rows: int) -> List[int]:
    """Needle slots of the long-window scenarios: block and power-of-two edges, the prompt's last two slots, both sides of
    every engine split edge at the rows asked (positions T-1 .. T-1+n_rows) and of the multi-launch step's split edges
    (ceil(S / 1024) splits of ceil(S / splits) slots, ops.attn_nsplit)."""
    slots = {0, 1, 31, 32, 33, 63, 64, 127, 128, 255, 256, 511, 512, 513, T - 2, T - 1}
    for p in range(T - 1, T + n_rows):
        ns, per = engine_split_per(min(p + 1, S), hs)
        for s in range(1, ns):
            slots.update((s * per - 1, s * per))
    nsplit = -(-S // 1024)
    per = -(-S // nsplit)
    for s in range(1, nsplit):
        slots.update((s * per - 1, s * per))
    return sorted(x for x in slots if 0 <= x < T)


def growing_scenarios(ids, T: int, S: int, crossings: Sequence[int], k: int = 3, seed: int = 0) -> List[Scenario]:
    """Forced walks from a ``T``-token prompt, two per n in ``crossings``: class 0's needle sits in slot 1 (the first split),
    class 1's is planted at position n - 2, and row n - 1 - the row that sees n keys - asks for the one in the last split
    (the newest key but one) or for the one in the first split, row n for the other; both are asked again ``k`` rows later,
    then a class that has no needle at all."""
    rng = random.Random(seed)
    assert ids.B >= 3
    out = []
    for n in crossings:
        for first in (1, 0):
            p = n - 1
            assert p - 1 >= T and p + k + 2 < S
            plan = {p - 1: ids.N[1][rng.randrange(ids.A)], p: ids.Q[first], p + 1: ids.Q[1 - first],
                    p + k: ids.Q[1], p + k + 1: ids.Q[0], p + k + 2: ids.Q[2]}
            toks = _fillers(ids, T, rng)
            toks[1] = ids.N[0][rng.randrange(ids.A)]
            toks[T - 1] = ids.Q[0]
            toks += [plan.get(q, rng.choice(ids.fill)) for q in range(T, p + k + 3)]
            out.append(Scenario(tokens=toks, T=T, S=S))
    return out


def ring_scenario(ids, T: int, S: int, n_steps: int, seed: int = 0) -> Scenario:
    """Forced tokens through a ring of ``S`` slots: class b's needle is planted every ``S + 1`` positions (the ring slot it lands
    in moves on by one each time; the classes start S / B slots apart), with a fresh answer each time, and queried when it is
    the newest key but one (one step later), when it is the oldest key of the window (S - 1 later: found) and one step after
    that (S later: NONE).  ``ring_coverage`` lists the slots a run covers."""
    rng = random.Random(seed)
    total = T + n_steps
    toks: List[Optional[int]] = [None] * total
    used = set()
    for b in range(ids.B):
        period = S + 1  # > S: never two needles of one class in a window
        p = 1 + b * max(2, S // ids.B)
        while p < total:
            want = [q for q in (p, p + 1, p + S - 1, p + S) if q < total]
            if not any(q in used for q in want):
                a = rng.randrange(ids.A)
                toks[p] = ids.N[b][a]
                for q in want[1:]:
                    toks[q] = ids.Q[b]
                used.update(want)
                p += period
            else:
                p += 1
    toks = [t if t is not None else rng.choice(ids.fill) for t in toks]
    if ids.kind[toks[T - 1]][0] == "fill":
        toks[T - 1] = ids.Q[ids.B - 1]
    return Scenario(tokens=toks, T=T, S=S)


def ring_coverage(ids, sc: Scenario) -> Tuple[set, set]:
    """Ring slots (position % S) whose needle was asked for by a checked row as the OLDEST key of the window, and by the row
    right behind it (the newest key but the query itself)."""
    oldest, newest = set(), set()
    for p in sc.rows:
        kind = ids.kind[sc.tokens[p]]
        if kind[0] != "Q":
            continue
        for q, into in ((p - sc.S + 1, oldest), (p - 1, newest)):
            if q >= 0 and ids.kind[sc.tokens[q]][:2] == ("N", kind[1]):
                into.add(q % sc.S)
    return oldest, newest


def prefill_scenario(ids, T: int, S: int, slots: Sequence[int], seed: int = 0) -> Scenario:
    """A prompt of ``T`` tokens ending in a query whose needle is at ``slots[0]``; the other slots hold needles of the other
    classes, queried by forced tokens afterwards."""
    rng = random.Random(seed)
    slots = [int(s) for s in slots]
    assert len(slots) <= ids.B and all(0 <= s < T - 1 for s in slots)
    toks = _fillers(ids, T, rng)
    first = rng.randrange(ids.B)
    for i, s in enumerate(slots):
        toks[s] = ids.N[(first + i) % ids.B][rng.randrange(ids.A)]
    toks[T - 1] = ids.Q[first]
    toks += _query_walk(ids, first + 1, ids.B)
    return Scenario(tokens=toks, T=T, S=S)


def free_prompt(ids, T: int, seed: int = 0, classes: Optional[Sequence[int]] = None) -> List[int]:
    """A prompt for free-running generation: fillers, one needle of each class in ``classes`` (default: all but the last, so
    the walk also meets NONE) at random slots, ending in a query."""
    rng = random.Random(seed)
    classes = list(range(ids.B - 1)) if classes is None else list(classes)
    toks = _fillers(ids, T, rng)
    for b, s in zip(classes, rng.sample(range(T - 1), len(classes))):
        toks[s] = ids.N[b][rng.randrange(ids.A)]
    toks[T - 1] = ids.Q[0]
    return toks


def all_rows_prompt(ids, T: int, seed: int = 0) -> List[int]:
    """A prompt whose EVERY row is checked (logits of all T rows): needles, queries and not-found tokens at random, a class's
    answer fixed for the whole prompt, so rows ask for keys at every distance behind them, and for classes not planted yet.
    The first 16 tokens are fillers: a needle row's flat attention reads its own value row with weight 1 / (keys in the window),
    which in a window of two or three keys is no longer small next to its embedding."""
    rng = random.Random(seed)
    ans = [rng.randrange(ids.A) for _ in range(ids.B)]
    toks = _fillers(ids, 16, rng)
    for _ in range(16, T):
        r, b = rng.random(), rng.randrange(ids.B)
        toks.append(ids.N[b][ans[b]] if r < 0.08 else ids.Q[b] if r < 0.55 else rng.choice(ids.fill))
    toks[T - 1] = ids.Q[0]
    return toks


def batch_scenarios(ids, n_rows: int, S: int, n_steps: int, seed: int = 0) -> List[Scenario]:
    """One scenario per row of a batched step: its own prompt length (40 .. 600), its own needle slots and, for every class, an
    answer no other row has ((row + class) % A: a row that reads another row's cache or position emits that row's answer)."""
    rng = random.Random(seed)
    assert n_rows <= ids.A
    lengths = [40, 600] + [rng.randrange(41, 600) for _ in range(n_rows - 2)]
    out = []
    for r in range(n_rows):
        T = lengths[r]
        toks = _fillers(ids, T, rng)
        classes = [b for b in range(ids.B) if b != r % ids.B]  # one class absent per row: NONE
        slots = [0, T - 2] + rng.sample(range(1, T - 2), len(classes) - 2)
        for b, s in zip(classes, slots):
            toks[s] = ids.N[b][(r + b) % ids.A]
        toks[T - 1] = ids.Q[r % ids.B]
        toks += _query_walk(ids, r + 1, n_steps)
        out.append(Scenario(tokens=toks, T=T, S=S))
    return out


def candidate_scenarios(ids, n_rows: int, T: int, S: int, slots: Sequence[int], seed: int = 0) -> List[List[Scenario]]:
    """Scenario groups for the candidates step: the ``n_rows`` scenarios of a group share their prompt (needles at ``slots``, B - 1
    per group; slot T is the first slot of the rows' own tails) and differ behind it: every row plants its OWN answer of the class
    the prompt lacks at position T (or, when slot T is not asked for, one row later), then asks for every class in turn."""
    rng = random.Random(seed)
    assert n_rows <= ids.A
    shared = sorted(set(int(s) for s in slots if s < T))
    per = ids.B - 1
    out = []
    for n, i in enumerate(range(0, len(shared), per)):
        chunk = shared[i:i + per]
        absent = n % ids.B
        classes = [b for b in range(ids.B) if b != absent]
        rng.shuffle(classes)
        prompt = _fillers(ids, T, rng)
        for s, b in zip(chunk, classes):
            prompt[s] = ids.N[b][rng.randrange(ids.A)]
        if T - 1 not in chunk:
            prompt[T - 1] = ids.Q[classes[0]]
        a0, delay = rng.randrange(ids.A), n % 2  # the rows' own needle at slot T or T + 1
        group = []
        for r in range(n_rows):
            tail = _fillers(ids, delay, rng) + [ids.N[absent][(a0 + r) % ids.A]] + _query_walk(ids, absent, ids.B + 1)
            group.append(Scenario(tokens=prompt + tail, T=T, S=S))
        out.append(group)
    return out


# ------------------------------------------------------------------------------------------------ the oracle's side
def oracle_rows(oracle, sc: Scenario, memo: Optional[dict] = None):
    """float32 logits (len(sc.rows), V) of oracle/model.py's OracleGPT for the forced tokens of ``sc``: the prompt in one call,
    then row by row.  ``memo``: a dict that keeps the prompt pass (last row's logits, kv caches) for scenarios sharing a prompt."""
    toks = torch.tensor(sc.tokens)
    key = (sc.S, tuple(sc.tokens[: sc.T]))
    with torch.no_grad():
        if memo is not None and key in memo:
            first, caches = memo[key]
            oracle.kv_caches = [(k.clone(), v.clone()) for k, v in caches]
        else:
            oracle.reset_cache()
            first = oracle(toks[: sc.T].view(1, -1), sc.S, torch.arange(sc.T))[0, -1].float()
            if memo is not None:
                memo.clear()  # (scenarios of one prompt follow each other: one entry is enough)
                memo[key] = (first, [(k.clone(), v.clone()) for k, v in oracle.kv_caches])
        out = [first]
        for p in range(sc.T, len(sc.tokens)):
            out.append(oracle(toks[p].view(1, 1), sc.S, torch.tensor([p]))[0, -1].float())
    return torch.stack(out)


def check_rows(ids, sc: Scenario, logits: torch.Tensor, what: str = "") -> Tuple[int, float, float]:
    """Every decided row of ``sc`` emits ``expected_next`` in ``logits`` (len(sc.rows), V).  Returns (rows checked, smallest
    top-1 - top-2 gap, largest |logit|) over them."""
    n, margin, largest = 0, float("inf"), 0.0
    for i, p in enumerate(sc.rows):
        want = sc.expect(ids, p)
        if want is None:
            continue
        row = logits[i].float()
        got = int(row.argmax())
        assert got == want, (f"{what}: row {p} (T={sc.T}, S={sc.S}) after {ids.kind[sc.tokens[p]]} emitted "
                             f"{ids.kind.get(got, got)}, expected {ids.kind[want]}")
        top = row.topk(2).values
        n, margin, largest = n + 1, min(margin, float(top[0] - top[1])), max(largest, float(row.abs().max()))
    return n, margin, largest


# ------------------------------------------------------------------------------------------------ what the tests run
EDGE_T, EDGE_S = 1100, 1200
CAND_T, CAND_S = 600, 704
CAND_SPLIT_KEYS = {4: 128, 8: 64}  # ops.ATTN_SPLIT_KEYS of the candidates tests: 6 splits of 118 slots, 11 of 64
BATCH_S, BATCH_STEPS = 640, 12
PREFILL_LENGTHS = (32, 100, 257, 512)
GROW_CROSSINGS = (32, 33, 64, 65, 128, 129)


def retrieval_model(name: str, dtype: torch.dtype = torch.bfloat16):
    """(config, state dict in ``dtype``, ids) of the retrieval model of family ``name``: two layers, positions up to 2048."""
    from lit_parrot_amd.config import Config

    cfg = Config.from_name(name, block_size=2048, n_layer=2)
    sd, ids = retrieval_state_dict(cfg, *default_classes(cfg))
    return cfg, {k: v.to(dtype) for k, v in sd.items()}, ids


def candidate_slots(n_rows: int) -> List[int]:
    """Both sides of every edge of the splits the candidates share (generate/base.py::shared_splits, restated: split j of
    ceil(S / nsplit) slots is shared when it ends inside the prompt), and the seam: the prompt's last slot and the tails' first."""
    nsplit = -(-CAND_S // CAND_SPLIT_KEYS[n_rows])
    per = -(-CAND_S // nsplit)
    slots = {CAND_T - 1, CAND_T}
    for j in range(nsplit - 1):
        if (j + 1) * per <= CAND_T:
            slots.update(((j + 1) * per - 1, (j + 1) * per))
    return sorted(slots)


def prefill_slots(T: int) -> List[int]:
    """Key-block edges of the prompt kernels (16 / 32 / 64 keys and their multiples) and row T - 2."""
    return sorted({s for s in (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 383, 384, T - 2) if s < T - 1})


def forced_scenarios(cfg, ids) -> Dict[str, List[Scenario]]:
    """Every forced-token scenario of tests/test_retrieval_gpu.py, by test (the rows of the batched and candidates tests as
    single-sequence scenarios: that is what each row must compute)."""
    hs = cfg.head_size
    out = {
        "edges": edge_scenarios(ids, EDGE_T, EDGE_S, edge_slots(EDGE_T, EDGE_S, hs, ids.B + 1), seed=1),
        "growing": growing_scenarios(ids, 20, 200, GROW_CROSSINGS, seed=2),
        "ring48": [ring_scenario(ids, 8, 48, 660, seed=3)],
        "ring160": [ring_scenario(ids, 8, 160, 340, seed=4)],
        "prefill": [prefill_scenario(ids, T, T + 2 * ids.B, [s], seed=5 + s) for T in PREFILL_LENGTHS for s in prefill_slots(T)],
        "batch3": batch_scenarios(ids, 3, BATCH_S, BATCH_STEPS, seed=6),
        "batch8": batch_scenarios(ids, 8, BATCH_S, BATCH_STEPS, seed=7),
    }
    for n in (4, 8):
        groups = candidate_scenarios(ids, n, CAND_T, CAND_S, candidate_slots(n), seed=8 + n)
        out[f"candidates{n}"] = [sc for group in groups for sc in group]
    return out
