"""n samples of one prompt: generate_batch([p] * n) against generate_candidates (one prefill, one shared prompt cache) on a
synthetic model of a bench.py workload.  Window 4096, prompts of 128 / 1024 / 3072 tokens, 128 new tokens, temperature 0.8,
top_k 200, no eos, n = 2, 4, 8; captured steps, timed with device events after warm-up.

    python tools/candidates_bench.py [--workload llama2-7b-int4] [--prompts 128,1024,3072] [--n 2,4,8] [--out FILE]

Three legs per point: ``batch`` (BatchDecodeSession: n prefills, n copies of the prompt K/V, unchanged code - the baseline of every
ratio), ``cand_noshare`` (CandidateSession with ops.CANDIDATES_SHARE_LOADS off: every row walks the shared cache itself) and
``cand_share`` (the shared-load workgroups).  Per leg: seconds until the first token of every row (prefill + first sample, warm),
ms per step, aggregate tokens/s and the bytes of K/V the session holds.  Nothing is reported after a HIP error or a row that did
not advance: the run ends with a non-zero status instead.
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
from bench import WORKLOADS, Watchdog  # noqa: E402
from lit_parrot_amd import ops  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import build_synthetic_model, synthetic_prompt  # noqa: E402

S = 4096
SAMPLER = (0.8, 200)


def _time_steps(sess, steps: int, warmup: int, dev) -> float:
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


def run_leg(model, leg: str, prompt: torch.Tensor, n: int, new_tokens: int, warmup: int) -> dict:
    dev, T = prompt.device, prompt.numel()
    total = T + new_tokens
    steps = new_tokens - 1 - warmup  # the first token comes from the prompt's logits
    model.reset_cache()
    model.__dict__.pop("_decode_sessions", None)
    ops.CANDIDATES_SHARE_LOADS = leg == "cand_share"
    if leg == "batch":
        sess = gb.BatchDecodeSession(model, n, S, total, False, SAMPLER)
        prefill = lambda: sess.prefill([prompt] * n, total)  # noqa: E731
        kv_bytes = sum(t.numel() * t.element_size() for pair in sess.caches for t in pair)
    else:
        sess = gb.CandidateSession(model, n, S, gb.candidate_tail_slots(total, T), False, SAMPLER)
        prefill = lambda: sess.prefill(prompt, total)  # noqa: E731
        kv_bytes = sess.kv_bytes()
    prefill()  # warm: lazy repacks, workspaces
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    prefill()
    sess.sample(sess.first_logits, -1)
    torch.cuda.synchronize(dev)
    first_s = time.perf_counter() - t0
    sess.capture()
    ms = _time_steps(sess, steps, warmup, dev)
    pos = sess.pos.cpu()
    if int(pos.min()) != T + warmup + steps or int(pos.max()) != T + warmup + steps:
        raise RuntimeError(f"{leg} n={n} T={T}: rows stand at {pos.tolist()}, expected {T + warmup + steps}")
    return {"leg": leg, "first_token_s": first_s, "ms_per_step": ms / steps, "tok_s": 1000.0 * n * steps / ms, "kv_bytes": kv_bytes}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="llama2-7b-int4", choices=["llama2-7b-int4", "stablelm-3b-bf16"])
    ap.add_argument("--prompts", default="128,1024,3072")
    ap.add_argument("--n", default="2,4,8")
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--watchdog", type=float, default=300.0, help="seconds without a phase change before the run exits with status 3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    wd = Watchdog(args.watchdog, tag="candidates_bench.py")
    dev = torch.device("cuda", 0)
    cfg_name, mode, _, dtype_label = WORKLOADS[args.workload]
    cfg = L.Config.from_name(cfg_name)
    t_start = time.perf_counter()
    wd.phase("building the synthetic model")
    model = build_synthetic_model(cfg, mode, seed=1234, device=dev)
    res = {"workload": args.workload, "model": cfg_name, "weights": dtype_label, "window": S, "new_tokens": args.new_tokens,
           "warmup": args.warmup, "sampling": {"temperature": SAMPLER[0], "top_k": SAMPLER[1]},
           "attn_nsplit": ops.attn_nsplit(cfg.n_query_groups, S, cfg.q_per_kv, 1), "points": []}
    share_default = ops.CANDIDATES_SHARE_LOADS
    try:
        with torch.no_grad():
            for T in (int(t) for t in args.prompts.split(",")):
                prompt = synthetic_prompt(cfg, T, 1234).to(dev)
                for n in (int(x) for x in args.n.split(",")):
                    point = {"prompt": T, "n": n, "legs": []}
                    for leg in ("batch", "cand_noshare", "cand_share"):
                        wd.phase(f"prompt {T}, n {n}: {leg}")
                        torch.manual_seed(1234)
                        point["legs"].append(run_leg(model, leg, prompt, n, args.new_tokens, args.warmup))
                    base = point["legs"][0]
                    for r in point["legs"][1:]:
                        r["step_speedup_vs_batch"] = base["ms_per_step"] / r["ms_per_step"]
                        r["first_token_speedup_vs_batch"] = base["first_token_s"] / r["first_token_s"]
                    res["points"].append(point)
            torch.cuda.synchronize(dev)
    except Exception as e:  # a HIP error, an engine error or a row that stopped: no figures
        print(f"candidates_bench.py: {type(e).__name__}: {e} - nothing is reported", file=sys.stderr, flush=True)
        wd.stop()
        return 2
    finally:
        ops.CANDIDATES_SHARE_LOADS = share_default
    wd.phase("summary")
    res["wall_s"] = time.perf_counter() - t_start
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    wd.stop()
    return 0


if __name__ == "__main__":
    sys.exit(main())
