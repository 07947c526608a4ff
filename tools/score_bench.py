"""Scoring (lit_parrot_amd.score) on a synthetic model of a bench.py workload, timed with device events after warm-up.

    python tools/score_bench.py [--workload llama2-7b-int4] [--tokens 512] [--continuations 8] [--length 32] [--reps 20] [--out FILE]

(a) ``token_logprobs`` on ``--tokens`` tokens against the torch-op route on the same tree,
    ``F.log_softmax(model(idx[None]).float(), -1).gather(...)`` - the same prompt pass, then a (T, V) fp32 copy and three torch
    launches in the place of one ``token_logprob_rows`` launch; the scoring launches alone are timed as well.
(b) ``continuation_logprobs`` for ``--continuations`` continuations of ``--length`` tokens behind a ``--tokens``-token prompt
    against one ``token_logprobs`` call per concatenation (the prompt prefilled once per continuation).
Both legs of a comparison alternate inside one timed loop; the outputs of the two routes are compared (max |difference|).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import lit_parrot_amd as L  # noqa: E402
from bench import WORKLOADS  # noqa: E402
from lit_parrot_amd import ops  # noqa: E402
from lit_parrot_amd.synth import build_synthetic_model, synthetic_prompt  # noqa: E402


def torch_route(model, idx):
    logits = model(idx[None])[0]
    return F.log_softmax(logits[:-1].float(), dim=-1).gather(1, idx[1:].view(-1, 1)).view(-1)


def alternate(legs: dict, reps: int, warmup: int, dev) -> dict:
    """ms per call of every leg: the legs take turns inside one loop, each call bracketed by its own pair of device events."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize(dev)
    events = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            events[name].append((e0, e1))
    torch.cuda.synchronize(dev)
    out = {}
    for name, evs in events.items():
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        out[name] = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="llama2-7b-int4", choices=sorted(WORKLOADS))
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--continuations", type=int, default=8)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    cfg_name, mode, _, dtype_label = WORKLOADS[args.workload]
    cfg = L.Config.from_name(cfg_name)
    t0 = time.perf_counter()
    model = build_synthetic_model(cfg, mode, seed=1234, device=dev)
    T, n, ln = args.tokens, args.continuations, args.length
    V = cfg.padded_vocab_size
    res = {"workload": args.workload, "model": cfg_name, "weights": dtype_label, "tokens": T, "continuations": n, "length": ln,
           "reps": args.reps, "warmup": args.warmup, "timing": "device events per call, legs alternating in one loop"}
    with torch.no_grad():
        # ---- (a)
        idx = synthetic_prompt(cfg, T, 1234).to(dev)
        logits = model(idx[None])[0].clone()
        lp = torch.empty((T - 1,), dtype=torch.float32, device=dev)
        legs = {
            "token_logprobs": lambda: L.token_logprobs(model, idx),
            "torch_route": lambda: torch_route(model, idx),
            "score_launch_only": lambda: ops.token_logprob_rows(logits[:-1], idx[1:], lp),
            "torch_ops_only": lambda: F.log_softmax(logits[:-1].float(), dim=-1).gather(1, idx[1:].view(-1, 1)),
        }
        a = alternate(legs, args.reps, args.warmup, dev)
        a["max_abs_difference"] = float((L.token_logprobs(model, idx) - torch_route(model, idx)).abs().max())
        a["fp32_copy_bytes_avoided"] = (T - 1) * V * 4
        a["speedup_end_to_end"] = a["torch_route"]["ms_median"] / a["token_logprobs"]["ms_median"]
        a["speedup_scoring_step"] = a["torch_ops_only"]["ms_median"] / a["score_launch_only"]["ms_median"]
        res["token_logprobs"] = a
        # ---- (b)
        S = T + ln
        prompt = idx
        conts = [synthetic_prompt(cfg, ln, 77 + b).to(dev) for b in range(n)]
        cats = [torch.cat([prompt, c]) for c in conts]
        legs = {
            "continuation_logprobs": lambda: L.continuation_logprobs(model, prompt, conts, S),
            "token_logprobs_per_continuation": lambda: [L.token_logprobs(model, c)[-ln:] for c in cats],
        }
        b = alternate(legs, max(3, args.reps // 4), args.warmup, dev)
        got, ref = legs["continuation_logprobs"](), legs["token_logprobs_per_continuation"]()
        b["max_abs_difference"] = max(float((x - y).abs().max()) for x, y in zip(got, ref))
        b["speedup"] = b["token_logprobs_per_continuation"]["ms_median"] / b["continuation_logprobs"]["ms_median"]
        res["continuation_logprobs"] = b
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
