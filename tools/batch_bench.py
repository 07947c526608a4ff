"""Batched decode (generate_batch's captured step) at B = 1, 2, 4, 8 sequences on a synthetic model of a bench.py workload:
128-token prompts, 128 new tokens per sequence, greedy, captured step, timed with device events after warm-up.

    python tools/batch_bench.py [--workload llama2-7b-int4] [--batches 1,2,4,8] [--steps 128] [--warmup 16] [--out FILE]

Per B: aggregate tokens/s (B tokens per step), ms per step, and the kernel launches of one step counted through the library's
profiling sink (one uncaptured step).  The ``single`` entry is the single-sequence multi-launch step (DecodeSession,
engine=False) for reference: B = 1 of the batched step computes the same tokens with the same kernels but for the embedding /
attention / sampling launches.  For a kernel table run one B under ``rocprofv3 --kernel-trace --stats``.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import lit_parrot_amd as L  # noqa: E402
from bench import WORKLOADS  # noqa: E402
from lit_parrot_amd import _hip  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import build_synthetic_model, synthetic_prompt  # noqa: E402

T_PROMPT = 128


def _launches(sess) -> dict:
    """Kernel launches of one uncaptured step, the loop state restored afterwards."""
    saved = (sess.tokens.clone(), sess.pos.clone(), [(k.clone(), v.clone()) for k, v in sess.caches])
    _hip.prof_begin()
    sess._step()
    prof = _hip.prof_end()
    sess.tokens.copy_(saved[0])
    sess.pos.copy_(saved[1])
    for (k, v), (k0, v0) in zip(sess.caches, saved[2]):
        k.copy_(k0)
        v.copy_(v0)
    return {name: n for name, (_, n) in sorted(prof.items())}


def _time(sess, steps: int, warmup: int, dev) -> float:
    for _ in range(warmup):
        sess.step()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        sess.step()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def run_batch(model, prompts, steps: int, warmup: int) -> dict:
    B, dev = len(prompts), prompts[0].device
    total = T_PROMPT + warmup + steps + 2
    with torch.no_grad():
        model.reset_cache()
        model.__dict__.pop("_decode_sessions", None)
        sess = gb.BatchDecodeSession(model, B, total, total, greedy=True)
        sess.prefill(prompts, total)
        sess.sample(sess.first_logits, -1)
        launches = _launches(sess)
        sess.capture()
        ms = _time(sess, steps, warmup, dev)
        assert int(sess.pos.min()) == T_PROMPT + warmup + steps, "a row stopped early"
    return {"B": B, "ms_per_step": ms / steps, "tok_s": 1000.0 * B * steps / ms, "launches_per_step": sum(launches.values()),
            "launches": launches}


def run_single(model, prompt, steps: int, warmup: int) -> dict:
    total = T_PROMPT + warmup + steps + 2
    with torch.no_grad():
        model.reset_cache()
        model.__dict__.pop("_decode_sessions", None)
        sess = gb.DecodeSession(model, total, total, greedy=True, engine=False)
        logits = sess.prefill(prompt)
        L.ops.argmax_advance(logits, sess.tokens, sess.pos)
        launches = _launches(sess)
        sess.capture()
        ms = _time(sess, steps, warmup, prompt.device)
    return {"ms_per_step": ms / steps, "tok_s": 1000.0 * steps / ms, "launches_per_step": sum(launches.values()), "launches": launches}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="llama2-7b-int4", choices=["llama2-7b-int4", "stablelm-3b-bf16"])
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--no-single", action="store_true", help="skip the single-sequence reference leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg_name, mode, _, dtype_label = WORKLOADS[args.workload]
    cfg = L.Config.from_name(cfg_name)
    t0 = time.perf_counter()
    model = build_synthetic_model(cfg, mode, seed=1234, device=dev)
    prompts = [synthetic_prompt(cfg, T_PROMPT, 1234 + b).to(dev) for b in range(8)]
    res = {"workload": args.workload, "model": cfg_name, "weights": dtype_label, "prompt": T_PROMPT, "new_tokens": args.steps,
           "warmup": args.warmup, "sampling": "greedy", "executor": "multi-launch batched step, captured"}
    if not args.no_single:
        res["single"] = run_single(model, prompts[0], args.steps, args.warmup)
    res["batch"] = [run_batch(model, prompts[:B], args.steps, args.warmup) for B in (int(b) for b in args.batches.split(","))]
    by_b = {r["B"]: r for r in res["batch"]}
    if 1 in by_b:
        res["speedup_vs_b1"] = {str(B): r["tok_s"] / by_b[1]["tok_s"] for B, r in by_b.items()}
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
