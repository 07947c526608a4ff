"""Prompt-lookup speculative decoding (generate_speculative's two captured steps) on a synthetic model of a bench.py workload:
a 128-token prompt, 256 new tokens, greedy, timed with device events after 16 warm-up steps; every leg runs ``--rounds`` times,
the legs alternating inside the one call, and the median is reported.

    python tools/spec_bench.py [--workload llama2-7b-int4] [--rows 2,4,8] [--new 256] [--warmup 16] [--rounds 3] [--out FILE]

Legs:
  generate_multilaunch / generate_default   generate()'s captured one-row step on the multi-launch executor / the default one
  rows[M][acceptance]     the M-row step with the draft hook forcing 0 %, 50 % (every other step right) and 100 % of the drafts to
                          be accepted: ms per step (host read and hook included, as the loop pays them), tokens/s, launches per step
  break_even              accepted drafts per step at which the M-row step pays for itself: t_M / t_1 - 1 (t_1: generate()'s
                          multi-launch step), and that number as a share of the K drafts
  lookup[K]               the free-running loop (generate_speculative, the prompt included) against generate(): acceptance seen,
                          tokens/s of both, and whether the tokens are equal.  Synthetic weights decode into loops, which the
                          lookup predicts well: this leg shows the mechanism at full size, it is NOT a user workload.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import lit_parrot_amd as L  # noqa: E402
from bench import WORKLOADS  # noqa: E402
from lit_parrot_amd import _hip, ops  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import build_synthetic_model, synthetic_prompt  # noqa: E402

T_PROMPT = 128


def _launches(sess, step) -> dict:
    """Kernel launches of one uncaptured step, the loop state restored afterwards."""
    saved = (sess.tokens.clone(), sess.pos.clone(), [(k.clone(), v.clone()) for k, v in sess.caches])
    _hip.prof_begin()
    step()
    prof = _hip.prof_end()
    sess.tokens.copy_(saved[0])
    sess.pos.copy_(saved[1])
    for (k, v), (k0, v0) in zip(sess.caches, saved[2]):
        k.copy_(k0)
        v.copy_(v0)
    return {name: n for name, (_, n) in sorted(prof.items())}


def run_generate_step(model, prompt, new: int, warmup: int, engine) -> dict:
    """generate()'s captured one-row step (as tools/batch_bench.py::run_single)."""
    total = T_PROMPT + warmup + new + 2
    with torch.no_grad():
        model.reset_cache()
        model.__dict__.pop("_decode_sessions", None)
        sess = gb.DecodeSession(model, total, total, greedy=True, engine=engine)
        logits = sess.prefill(prompt)
        ops.argmax_advance(logits, sess.tokens, sess.pos)
        launches = _launches(sess, sess._step) if sess.eng is None else {"eng_token": 1}
        sess.capture()
        for _ in range(warmup):
            sess.step()
        torch.cuda.synchronize(prompt.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(new):
            sess.step()
        e1.record()
        torch.cuda.synchronize(prompt.device)
        ms = e0.elapsed_time(e1)
        sess.check_error()
    return {"ms_per_step": ms / new, "tok_s": 1000.0 * new / ms, "launches_per_step": sum(launches.values()),
            "executor": "engine" if sess.eng is not None else "multi-launch"}


def run_rows(model, prompt, truth, M: int, rate: float, new: int, warmup: int) -> dict:
    """The M-row step with forced acceptance: the hook writes the true continuation (``truth``: generate()'s tokens) or wrong
    tokens behind pos; verification keeps the sequence on ``truth`` either way."""
    K, dev = M - 1, prompt.device
    total = truth.numel() - M
    wrong = (truth + 1) % model.config.vocab_size
    with torch.no_grad():
        model.reset_cache()
        model.__dict__.pop("_decode_sessions", None)
        sess = gb.SpeculativeSession(model, total, total, draft_len=K, draft_hook=lambda s: K)
        logits = sess.prefill(prompt, total)
        sess.capture(rows=True)
        ops.argmax_advance(logits, sess.tokens, sess.pos)
        launches = _launches(sess, sess._step_rows)
        p, n_step = T_PROMPT, 0

        def step():
            nonlocal p, n_step
            right = rate >= 1.0 or (rate > 0.0 and n_step % 2 == 0)
            sess.tokens[p + 1:p + 1 + K].copy_((truth if right else wrong)[p + 1:p + 1 + K])
            sess.step(True)
            n_step += 1
            p = int(sess.pos)  # the loop's one host read per step

        for _ in range(warmup):
            step()
        torch.cuda.synchronize(dev)
        p0, s0 = p, n_step
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        while p - p0 < new and p + M <= total:
            step()
        e1.record()
        torch.cuda.synchronize(dev)
        ms, steps, toks = e0.elapsed_time(e1), n_step - s0, p - p0
        assert torch.equal(sess.tokens[:p + 1], truth[:p + 1]), "the verified tokens left generate()'s"
    return {"M": M, "forced_acceptance": rate, "ms_per_step": ms / steps, "tok_s": 1000.0 * toks / ms, "steps": steps, "tokens": toks,
            "accepted_per_step": toks / steps - 1, "launches_per_step": sum(launches.values()), "launches": launches}


def run_lookup(model, prompt, K: int, new: int) -> dict:
    total = T_PROMPT + new
    dev = prompt.device
    out = {}
    with torch.no_grad():
        for name, fn in (("generate", lambda: (L.generate(model, prompt, total, total, top_k=1), None)),
                         ("speculative", lambda: L.generate_speculative(model, prompt, total, total, draft_len=K, return_stats=True))):
            fn()  # builds and captures the session
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            y, stats = fn()
            torch.cuda.synchronize(dev)
            out[name] = {"tok_s": new / (time.perf_counter() - t0), "tokens": y, "stats": stats}
    st = out["speculative"]["stats"]
    return {"draft_len": K, "generate_tok_s": out["generate"]["tok_s"], "speculative_tok_s": out["speculative"]["tok_s"],
            "speedup": out["speculative"]["tok_s"] / out["generate"]["tok_s"], **st,
            "accepted_share_of_tokens": st["accepted"] / max(1, new - 1),
            "tokens_equal_generate": bool(torch.equal(out["generate"]["tokens"], out["speculative"]["tokens"])),
            "note": "prompt included in both timings; synthetic weights decode into loops: not a user workload"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="llama2-7b-int4", choices=["llama2-7b-int4", "stablelm-3b-bf16"])
    ap.add_argument("--rows", default="2,4,8")
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg_name, mode, _, dtype_label = WORKLOADS[args.workload]
    cfg = L.Config.from_name(cfg_name)
    t0 = time.perf_counter()
    model = build_synthetic_model(cfg, mode, seed=1234, device=dev)
    why = model.speculative_decode_unsupported()
    if why is not None:
        raise SystemExit(f"{args.workload}: {why}")
    prompt = synthetic_prompt(cfg, T_PROMPT, 1234).to(dev)
    Ms = [int(m) for m in args.rows.split(",")]
    gb.ENGINE_DEFAULT = False
    # the continuation the forced legs feed: generate()'s own tokens, long enough for the widest step at 0 % acceptance
    n_truth = T_PROMPT + (args.warmup + 2) * max(Ms) + args.new + 2 * max(Ms)
    n_truth = min(n_truth, cfg.block_size)
    with torch.no_grad():
        truth = torch.cat([L.generate(model, prompt, n_truth, n_truth, top_k=1), prompt.new_zeros(max(Ms))])
    gb.ENGINE_DEFAULT = "auto"
    legs = {"generate_multilaunch": lambda: run_generate_step(model, prompt, args.new, args.warmup, False),
            "generate_default": lambda: run_generate_step(model, prompt, args.new, args.warmup, None)}
    for M in Ms:
        for rate in (0.0, 0.5, 1.0):
            legs[f"rows{M}_{int(rate * 100)}"] = (lambda M=M, rate=rate: run_rows(model, prompt, truth[:n_truth - max(Ms) + M].contiguous(),
                                                                                 M, rate, args.new, args.warmup))
    runs = {k: [] for k in legs}
    for _ in range(args.rounds):  # the legs alternate: drift of the machine lands on all of them alike
        for k, fn in legs.items():
            runs[k].append(fn())

    def med(k):
        rs = sorted(runs[k], key=lambda r: r["ms_per_step"])
        r = dict(rs[len(rs) // 2])
        r["ms_per_step_runs"] = [x["ms_per_step"] for x in runs[k]]
        return r

    res = {"workload": args.workload, "model": cfg_name, "weights": dtype_label, "prompt": T_PROMPT, "new_tokens": args.new,
           "warmup": args.warmup, "rounds": args.rounds, "sampling": "greedy",
           "generate_multilaunch": med("generate_multilaunch"), "generate_default": med("generate_default"), "rows": {}, "break_even": {}}
    t1 = res["generate_multilaunch"]["ms_per_step"]
    for M in Ms:
        res["rows"][str(M)] = {str(int(r * 100)): med(f"rows{M}_{int(r * 100)}") for r in (0.0, 0.5, 1.0)}
        tM = statistics.median(res["rows"][str(M)][a]["ms_per_step"] for a in ("0", "50", "100"))
        res["break_even"][str(M)] = {"step_cost_vs_one_row": tM / t1, "accepted_per_step": tM / t1 - 1,
                                     "share_of_drafts": (tM / t1 - 1) / (M - 1)}
    gb.ENGINE_DEFAULT = False
    res["lookup"] = [run_lookup(model, prompt, K, args.new) for K in (1, 3, 7)]
    gb.ENGINE_DEFAULT = "auto"
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
