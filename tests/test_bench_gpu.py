"""bench.py end to end on the tiny workload: the plain line, --full, and --dump-outputs (what the last timed step computed)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "prefill_ms", "reference_definition_tokens_per_s", "sampled", "cpu_baseline")


def _bench(*args: str) -> dict:
    proc = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--workload", "tiny-llama-int4", "--watchdog", "120", *args],
                          cwd=REPO, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


def test_plain_and_full_lines_and_their_outputs(tmp_path):
    plain = _bench("--steps", "5", "--warmup", "3", "--dump-outputs", str(tmp_path / "plain"))
    for k in CONTRACT:
        assert k in plain, k
    assert plain["steps"] == 5 and plain["warmup"] == 3 and plain["higher_is_better"] is True
    assert plain["ms_per_step"] > 0 and abs(plain["value"] - 1e3 / plain["ms_per_step"]) < 1e-6 * plain["value"]
    assert not any(k in plain for k in FULL_ONLY), sorted(plain)

    full = _bench("--steps", "5", "--warmup", "3", "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    for k in CONTRACT + FULL_ONLY:
        assert k in full, k
    assert full["kernels"] and full["prefill_ms"] > 0 and full["sampled"]["steps"] == 5 and full["cpu_baseline"] is None

    logits, tokens = (np.load(tmp_path / "plain" / f"{n}.npy") for n in ("logits", "tokens"))
    assert logits.dtype == np.float32 and tokens.dtype == np.float64
    assert logits.shape == (512,) and np.isfinite(logits).all()  # tiny-llama: padded vocabulary of 512
    assert tokens.shape == (16 + 3 + 5 + 1,)  # prompt, the prefill's token, every warm-up and timed step's token
    assert tokens[-1] == logits.argmax()  # greedy: the last step chose the arg-max of the logits it returned
    # the same seeded inputs: --full (a second prefill, measurements after the clock) leaves the timed path's outputs alone
    for n in ("logits", "tokens"):
        assert np.array_equal(np.load(tmp_path / "plain" / f"{n}.npy"), np.load(tmp_path / "full" / f"{n}.npy")), n
