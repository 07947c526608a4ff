"""Single-stream decode of a synthetic Llama-2-7B bf16 model with LLaMA-Adapter v2 (adapter_start_layer 2, aT 10) against the
same base model: 128-token prompt, 128 new tokens, greedy, captured step; timed with device events after warm-up.

    python tools/adapter_bench.py [--legs adapter,base,default] [--steps 128] [--warmup 16] [--out FILE]

Legs: ``adapter`` - the adapter-v2 model (the stream engine declines it: multi-launch step); ``base`` - the base model with
engine=False (the same executor); ``default`` - the base model on the library's default executor choice.  Every leg also
counts the kernel launches of one decode step through the library's profiling sink (one uncaptured step).  For an
independent count run one leg per process under ``rocprofv3 --kernel-trace --stats`` with --steps 0 and --steps N: the
difference of the dispatch totals over N is the launches per token.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import lit_parrot_amd as L  # noqa: E402
from lit_parrot_amd import _hip  # noqa: E402
from lit_parrot_amd import adapter as A  # noqa: E402
from lit_parrot_amd import adapter_v2 as V  # noqa: E402
from lit_parrot_amd.generate import base as gb  # noqa: E402
from lit_parrot_amd.synth import build_synthetic_model, synthetic_prompt  # noqa: E402

T_PROMPT = 128


def adapter_twin(base: torch.nn.Module, start: int, aT: int, seed: int) -> torch.nn.Module:
    """The adapter-v2 model on the base model's weights, with non-trivial adapter parameters."""
    cfg = A.Config(**{**base.config.to_dict(), "adapter_start_layer": start, "adapter_prompt_length": aT})
    dev = base.lm_head.weight.device
    with torch.device(dev):
        model = A.GPT(cfg)
    V.add_adapter_v2_parameters_to_linear_layers(model)
    model = model.to(torch.bfloat16)
    model.load_state_dict(base.state_dict(), strict=False)
    gen = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "adapter_scale" in name:
                p.copy_(1 + 0.05 * torch.randn(p.shape, generator=gen, device=dev))
            elif "adapter_bias" in name:
                p.copy_(0.01 * torch.randn(p.shape, generator=gen, device=dev))
            elif "adapter_wte" in name:
                p.copy_(0.02 * torch.randn(p.shape, generator=gen, device=dev))
            elif "gating_factor" in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=gen, device=dev))
    return model.eval()


def run_leg(model, prompt, steps: int, warmup: int, engine) -> dict:
    total = T_PROMPT + warmup + steps + 2
    dev = prompt.device
    with torch.no_grad():
        model.reset_cache()
        model.__dict__.pop("_decode_sessions", None)
        sess = gb.DecodeSession(model, total, total, greedy=True, engine=engine)
        logits = sess.prefill(prompt)
        L.ops.argmax_advance(logits, sess.tokens, sess.pos)
        # launches of one decode step (uncaptured, through the library's profiling sink), state restored afterwards
        saved = (sess.tokens.clone(), sess.pos.clone(), [(k.clone(), v.clone()) for k, v in sess.caches])
        _hip.prof_begin()
        sess._step()
        launches = sum(n for _, n in _hip.prof_end().values())
        sess.tokens.copy_(saved[0])
        sess.pos.copy_(saved[1])
        for (k, v), (k0, v0) in zip(sess.caches, saved[2]):
            k.copy_(k0)
            v.copy_(v0)
        sess.capture()
        for _ in range(warmup):
            sess.step()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            sess.step()
        e1.record()
        torch.cuda.synchronize(dev)
        sess.check_error()
    ms = e0.elapsed_time(e1) if steps else 0.0
    return {"engine": sess.eng is not None, "launches_per_step": launches, "steps": steps,
            "ms_per_token": ms / steps if steps else None, "tok_s": 1000.0 * steps / ms if steps else None}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="adapter,base,default")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--model", default="Llama-2-7b-hf")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = L.Config.from_name(args.model)
    t0 = time.perf_counter()
    base = build_synthetic_model(cfg, None, seed=1234, device=dev)
    prompt = synthetic_prompt(cfg, T_PROMPT, 1234).to(dev)
    legs = args.legs.split(",")
    res = {"model": args.model, "prompt": T_PROMPT, "new_tokens": args.steps, "warmup": args.warmup, "adapter_start_layer": 2,
           "adapter_prompt_length": 10}
    if "adapter" in legs:
        model = adapter_twin(base, 2, 10, 99)
        res["adapter"] = run_leg(model, prompt, args.steps, args.warmup, engine="auto")
        del model
        torch.cuda.empty_cache()
    if "base" in legs:
        res["base_multilaunch"] = run_leg(base, prompt, args.steps, args.warmup, engine=False)
    if "default" in legs:
        res["base_default"] = run_leg(base, prompt, args.steps, args.warmup, engine="auto")
    if "adapter" in res and "base_multilaunch" in res and args.steps:
        res["adapter_vs_base_multilaunch"] = res["adapter"]["tok_s"] / res["base_multilaunch"]["tok_s"]
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
