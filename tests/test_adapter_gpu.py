"""LLaMA-Adapter (v1) and Adapter-v2 models on the HIP path (MI355X box: ``-m gpu``).

Judges: tests/golden/adapter.npz - logits of the REFERENCE's lit_gpt.adapter / adapter_v2 models on the synthetic base weights
and the adapter parameters stored in the file (tests/golden/make_golden_adapter.py) - with the per-logit bounds of
test_model_gpu.py (restated below), and kernel-level equivalences: the fused decode prefix against the multi-row prefix
kernel, the fused adapter affine against the plain kernels followed by torch's bf16 ops in the reference's order.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import lit_parrot_amd as L  # noqa: E402
from lit_parrot_amd import _hip, ops  # noqa: E402
from lit_parrot_amd import adapter as A  # noqa: E402
from lit_parrot_amd import adapter_v2 as V  # noqa: E402
from lit_parrot_amd._hip import EPI_GELU, EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU, ParrotHipError  # noqa: E402
from lit_parrot_amd.config import Config  # noqa: E402
from lit_parrot_amd.model import build_rope_cache  # noqa: E402
from lit_parrot_amd.synth import is_linear_key, synthetic_state_dict  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
MODEL_SEED, T_NOCACHE, T_PROMPT, MAX_SEQ, N_DECODE = 4321, 12, 7, 16, 4
MAIN_CASES = ["llama_gqa", "falcon_mqa", "neox", "llama_hs128"]
CASES = MAIN_CASES + ["llama_gqa_s0", "neox_v1"]


# ---- the bounds of test_model_gpu.py (a) - (d), restated
def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -100))) - 7)


def check_bf16_logits(hip, ref_bf16, ref_f32, what, k_row):
    hip = hip.detach().float().cpu()
    assert torch.isfinite(hip).all(), what
    dist = (hip - ref_bf16).abs()
    if k_row == 0:
        assert float(dist.max()) == 0.0, f"{what}: {int((dist != 0).sum())} logits differ from the reference's (expected bit-identical)"
        return
    ulp_row = ulp_bf16(ref_bf16.abs().amax(dim=-1, keepdim=True))
    bad = dist > 1e-3 + k_row * ulp_row
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} logits further than 1e-3 + {k_row} row-ulp from the reference's "
                                 f"(worst {float((dist / ulp_row).max()):.2f} row-ulp, |d| {float(dist.max()):.4g})")
    big = ref_bf16.abs() >= 0.125
    bad = (dist > 1e-3 + 9 * ulp_bf16(ref_bf16)) & big
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} logits with |ref| >= 1/8 further than 1e-3 + 9 ulp(ref)"
    err_hip, err_ref = (hip - ref_f32).abs(), (ref_bf16 - ref_f32).abs()
    assert float(err_hip.max()) <= 1.25 * float(err_ref.max()) + 1e-3, f"{what}: max error {float(err_hip.max()):.4g} vs reference's {float(err_ref.max()):.4g}"
    assert float(err_hip.mean()) <= 1.25 * float(err_ref.mean()) + 1e-4, f"{what}: mean error {float(err_hip.mean()):.4g} vs reference's {float(err_ref.mean()):.4g}"
    same = float((dist == 0).float().mean())
    assert same >= 0.15, f"{what}: only {same:.3f} of the logits bit-identical"


def k_row_for(cfg, rsqrt_mode):
    if cfg.n_query_groups == 1 and cfg.n_head > 1:
        return 0
    if cfg._norm_class == "LayerNorm":
        return 1.5
    return 2.5 if rsqrt_mode else 3


# ---- golden access
@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir / "adapter.npz")


def from_bits(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(BF)


def ref_logits(g, case, what):
    b = from_bits(g[f"{case}/{what}_bf16"]).float()
    src = "nocache" if what == "prefill" else what
    if f"{case}/{src}_f32d" not in g.files:
        return b, None  # (the multi-query case: compared bit for bit)
    f = from_bits(g[f"{case}/{src}_bf16"]).float() + torch.from_numpy(g[f"{case}/{src}_f32d"].astype(np.float32))
    return b, (f[: b.shape[0]] if what == "prefill" else f)


def case_config(g, case):
    name, start, v2 = (str(x) for x in g[f"{case}/cfg"])
    return A.Config.from_name(name, adapter_start_layer=int(start)), v2 == "1"


def adapter_state(g, cfg, v2, scale_params=None):
    """Base weights (synthetic, seed MODEL_SEED) + the golden's adapter parameters for this model's keys."""
    shell = A.GPT(cfg)
    if v2:
        V.add_adapter_v2_parameters_to_linear_layers(shell)
    sd = {k: v.to(BF) for k, v in synthetic_state_dict(cfg, MODEL_SEED, perturb=True).items()}
    for k in shell.state_dict():
        if k not in sd:
            sd[k] = from_bits(g[f"params/{cfg.name}/{k}"]).view(shell.state_dict()[k].shape)
            if scale_params is not None:
                sd[k] = scale_params(k, sd[k])
    return sd


def adapter_model(cfg, v2, sd, **overrides):
    if overrides:
        cfg = A.Config(**{**cfg.to_dict(), **overrides})
    model = A.GPT(cfg)
    if v2:
        V.add_adapter_v2_parameters_to_linear_layers(model)
    model.load_state_dict(sd, strict=True)
    return model.to(BF).to(DEV).eval()


# ---- 1. logits against the reference
@pytest.fixture
def cpu_reference_modes():
    """The two parity switches of test_model_gpu.py: the CPU-run reference's RMSNorm rsqrt rounding, and its softmax (torch's CPU
    flash kernel rounds the probabilities to bf16 - the multi-query family runs torch's fp32 math path and keeps mode 0).  The
    adapter models add a second softmax per adapted layer (the prefix) and Linears scaled by adapter_scale; in the default
    arithmetic single logits land just past the base models' bounds (one logit past 9 ulp(ref) on tiny-llama-gqa / -hs128,
    2.0 row-ulp against 1.5 on tiny-neox)."""
    yield ops
    ops.RMSNORM_RSQRT_MODE, ops.ATTN_SOFTMAX_MODE = 0, 0


@pytest.mark.parametrize("case", CASES)
def test_adapter_logits_match_the_reference(g, golden_dir, case, cpu_reference_modes):
    cfg, v2 = case_config(g, case)
    model = adapter_model(cfg, v2, adapter_state(g, cfg, v2))
    ops.RMSNORM_RSQRT_MODE = 1
    ops.ATTN_SOFTMAX_MODE = 0 if (cfg.n_query_groups == 1 and cfg.n_head > 1) else 1
    # the base models' bound with the parity switches, except LayerNorm families with adapter-v2 Linears: measured 2.00 row-ulp
    # (tiny-neox decode, two logits of 2048), against 1.5 for the base models
    tight = k_row_for(cfg, 1)
    if tight and v2 and cfg._norm_class == "LayerNorm":
        tight = 2.0
    tokens = torch.from_numpy(g[f"{case}/tokens"]).to(DEV)
    with torch.no_grad():
        out = model(tokens[:T_NOCACHE].view(1, -1))
        assert out.shape == (1, T_NOCACHE, cfg.padded_vocab_size) and out.dtype == BF
        check_bf16_logits(out[0], *ref_logits(g, case, "nocache"), f"{case} no-cache", tight)
        model.reset_cache()
        pos = torch.arange(T_PROMPT, device=DEV)
        pre = model(tokens[:T_PROMPT].view(1, -1), MAX_SEQ, pos)[0]
        if f"{case}/prefill_bf16" in g.files:
            check_bf16_logits(pre, *ref_logits(g, case, "prefill"), f"{case} prefill", tight)
        assert len(model.adapter_kv_caches) == cfg.n_layer
        for i, kv in enumerate(model.adapter_kv_caches):
            assert (kv is None) == (i < cfg.adapter_start_layer)
            if kv is not None:
                assert kv[0].shape == (1, cfg.n_query_groups, cfg.adapter_prompt_length, cfg.head_size)
        rows = []
        for i in range(N_DECODE):
            pos = pos[-1:] + 1
            rows.append(model(tokens[T_PROMPT + i].view(1, 1), MAX_SEQ, pos)[0])
        check_bf16_logits(torch.cat(rows), *ref_logits(g, case, "decode"), f"{case} decode", tight)
    # the adapter is no no-op: its golden logits sit far from the base model's on the same tokens (>= 11 row-ulp measured)
    base = torch.from_numpy(np.load(golden_dir / f"model_{cfg.name}.npz")["nocache_bf16"])
    mine = from_bits(g[f"{case}/nocache_bf16"]).float()[: base.shape[0]]
    row_ulps = ((mine - base).abs() / ulp_bf16(base.abs().amax(-1, keepdim=True))).amax(-1)
    assert float(row_ulps.min()) > 8, f"{case}: the adapter moves a row by only {float(row_ulps.min()):.1f} row-ulp"


# ---- 2. the captured decode step against the reference's bf16 greedy run
def test_adapter_captured_greedy_against_the_reference_bf16_run(g):
    from lit_parrot_amd.generate import base as gb

    cfg, v2 = case_config(g, "llama_gqa")
    model = adapter_model(cfg, v2, adapter_state(g, cfg, v2))
    prompt = torch.from_numpy(g["gen/prompt"])
    ref_tokens = torch.from_numpy(g["gen/tokens"])
    top_v, top_i = torch.from_numpy(g["gen/top2_values"]), torch.from_numpy(g["gen/top2_indices"])
    T, total = prompt.numel(), ref_tokens.numel()
    N = total - T
    margin_ulps = (top_v[:, 0] - top_v[:, 1]) / ulp_bf16(top_v[:, 0])
    with torch.no_grad():
        # teacher-forced through the captured step
        sess = gb.DecodeSession(model, total, total, greedy=False, use_graph=True, engine=False)
        assert sess.eng is None
        sess.tokens[:total].copy_(ref_tokens.to(DEV))
        logits = sess.prefill(prompt.to(DEV)).float().view(-1).cpu()
        sess.capture()
        assert sess.graph is not None
        for i in range(N):
            tok = int(logits.argmax())
            if float(margin_ulps[i]) > 2:
                assert tok == int(ref_tokens[T + i]), f"step {i}: arg-max {tok}, the reference's {int(ref_tokens[T + i])}"
            else:
                assert tok in top_i[i].tolist(), f"step {i}: arg-max {tok} is neither of {top_i[i].tolist()}"
            if i + 1 < N:
                sess.pos.fill_(T + i)
                logits = sess.step().float().view(-1).cpu()
        # free-running generate(): the reference's tokens up to the first near-tied step
        model.reset_cache()
        y = L.generate(model, prompt.to(DEV), total, total, top_k=1).cpu()
    for i in range(N):
        if float(margin_ulps[i]) <= 2:
            break
        assert int(y[T + i]) == int(ref_tokens[T + i]), f"generate() step {i}: {y[T:].tolist()} vs {ref_tokens[T:].tolist()}"


# ---- 3 / 4. kernel equivalence, every exit
def _rand(shape, scale=1.0, seed=0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=gen) * scale).to(BF).to(DEV)


ATTN_CASES = [  # (n_groups, q_per_kv, hs, S, pos, aT, softmax_mode)
    (2, 2, 64, 16, 6, 10, 0),      # GQA q_per_kv 2
    (1, 8, 64, 16, 3, 10, 0),      # q_per_kv 8 (two workgroups of 4 heads per group)
    (1, 4, 64, 16, 9, 1, 0),       # MQA, aT 1
    (2, 1, 128, 16, 12, 64, 0),    # MHA hs 128, aT 64
    (2, 2, 128, 2048, 1500, 10, 0),  # nsplit > 1: the last arriver adds the prefix
    (1, 8, 64, 1100, 1099, 64, 0),   # nsplit > 1, 8 heads per group
    (2, 2, 64, 10, 23, 10, 0),     # ring wrap past the window
    (2, 2, 64, 16, 6, 10, 1),      # softmax_mode 1
    (1, 4, 128, 16, 5, 10, 1),     # softmax_mode 1, MQA hs 128
]


@pytest.mark.parametrize("n_groups,q_per_kv,hs,S,pos_v,aT,mode", ATTN_CASES)
def test_fused_decode_prefix_equals_the_multi_row_prefix_kernel(n_groups, q_per_kv, hs, S, pos_v, aT, mode):
    n_head = n_groups * q_per_kv
    n_elem = hs // 2
    qkv = _rand((1, n_groups * (q_per_kv + 2) * hs), 1.0, 1)
    kc0, vc0 = _rand((n_groups, S, hs), 1.0, 2), _rand((n_groups, S, hs), 1.0, 3)
    ak, av = _rand((n_groups, aT, hs), 1.0, 4), _rand((n_groups, aT, hs), 1.0, 5)
    gate = _rand((n_head,), 1.0, 6)
    cos, sin = build_rope_cache(max(S, pos_v + 1), n_elem, BF, DEV)
    pos = torch.tensor([pos_v], dtype=torch.int32, device=DEV)
    nsplit = ops.attn_nsplit(n_groups, S, q_per_kv, 1)
    if S > 1024:
        assert nsplit > 1
    prefix = ops.AdapterPrefix(ak, av, gate)
    saved = ops.ATTN_SOFTMAX_MODE
    ops.ATTN_SOFTMAX_MODE = mode
    try:
        def fused(with_prefix):
            kc, vc = kc0.clone(), vc0.clone()
            y = torch.zeros((1, n_head * hs), dtype=BF, device=DEV)
            ws = ops.attn_workspace(1, n_head, hs, nsplit, DEV)
            tickets = torch.zeros((n_head,), dtype=torch.int32, device=DEV)
            args = (qkv, cos, sin, n_elem, pos, kc, vc, n_groups, q_per_kv, hs, S, nsplit, ws, tickets, y)
            (ops.attn_fused_decode_adapter(*args, prefix) if with_prefix else ops.attn_fused_decode(*args))
            return y, kc, vc

        y1, kc1, vc1 = fused(True)
        y0, kc2, vc2 = fused(False)
        assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2)
        q = torch.empty((1, n_head * hs), dtype=BF, device=DEV)
        ops.rope_kvappend(qkv, cos, sin, n_elem, pos, n_groups, q_per_kv, hs, S, q, kc0.clone(), vc0.clone())
        base = y0.clone()
        ops.attn_adapter_prefix(q, n_groups, q_per_kv, hs, y0, prefix)
        torch.cuda.synchronize()
    finally:
        ops.ATTN_SOFTMAX_MODE = saved
    assert torch.equal(y1.view(torch.int16), y0.view(torch.int16)), f"{int((y1 != y0).sum())} outputs differ"
    if mode == 1:
        return  # (bf16 probabilities: the float64 comparison below is for the default mode)
    # and the term is the gated prefix attention (float64 on the host; the kernel rounds ay, gate * ay and the sum to bf16)
    qh = q.view(n_groups, q_per_kv, hs).double().cpu()
    s = torch.einsum("gqd,gtd->gqt", qh, ak.double().cpu()) / hs ** 0.5
    ay = torch.einsum("gqt,gtd->gqd", torch.softmax(s, -1), av.double().cpu()).reshape(n_head, hs)
    want = (base.view(n_head, hs).double().cpu() + (gate.double().cpu()[:, None] * ay.to(BF).double()).to(BF).double())
    d = (y1.view(n_head, hs).double().cpu() - want).abs()
    assert float((d / ulp_bf16(want.float()).double()).max()) <= 2.0 or float(d.max()) <= 1e-2


def _torch_affine(t, s, b):
    return (t + b) * s  # two bf16 tensor ops: rounded after the sum and after the product (adapter_v2.py:34-35)


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_RESIDUAL, EPI_GELU, EPI_SWIGLU])
@pytest.mark.parametrize("M", [1, 2, 5, 9, 64, 200])
def test_adapter_linear_equals_plain_linear_then_torch_ops(epi, M):
    """M <= 8: the affine fused into the GEMV epilogue; M > 8: the prompt GEMM with PARROT_EPI_NONE + the element-wise
    adapter epilogue.  Either equals the plain Linear followed by the reference's bf16 torch ops, bit for bit."""
    N, K = 352, 256
    W, W2 = _rand((N, K), 0.05, 10), _rand((N, K), 0.05, 11)
    x = _rand((M, K), 1.0, 12)
    bias = None if epi == EPI_SWIGLU else _rand((N,), 0.05, 13)
    s, b, s2, b2 = 1 + _rand((N,), 0.25, 14), _rand((N,), 0.05, 15), 1 + _rand((N,), 0.25, 16), _rand((N,), 0.05, 17)
    res = _rand((M, N), 1.0, 18) if epi == EPI_RESIDUAL else None
    ad = ops.Adapter(s, b, s2 if epi == EPI_SWIGLU else None, b2 if epi == EPI_SWIGLU else None)
    got = ops.bf16_linear(W, x, torch.empty((M, N), dtype=BF, device=DEV), bias=bias, epilogue=epi, residual=res,
                          weight2=W2 if epi == EPI_SWIGLU else None, adapter=ad)
    t = _torch_affine(ops.bf16_linear(W, x, torch.empty((M, N), dtype=BF, device=DEV), bias=bias), s, b)
    if epi == EPI_RESIDUAL:
        want = res + t
    elif epi == EPI_GELU:
        want = F.gelu(t)
    elif epi == EPI_SWIGLU:
        t2 = _torch_affine(ops.bf16_linear(W2, x, torch.empty((M, N), dtype=BF, device=DEV)), s2, b2)
        want = F.silu(t) * t2
    else:
        want = t
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} outputs differ"


# ---- 5. no stale prefix
def test_reset_cache_refills_the_prefix_from_new_weights(g):
    cfg, v2 = case_config(g, "llama_gqa")
    sd1 = adapter_state(g, cfg, v2)
    sd2 = adapter_state(g, cfg, v2, scale_params=lambda k, v: (-v if "gating_factor" in k else (v * 3 if "adapter_wte" in k else v)))
    prompt = torch.from_numpy(g["gen/prompt"]).to(DEV)
    model = adapter_model(cfg, v2, sd1)
    with torch.no_grad():
        y1 = L.generate(model, prompt, 20, 20, top_k=1)
        ak1 = model.adapter_kv_caches[1][0].clone()
        buf = model.adapter_kv_caches[1][0].data_ptr()
        model.load_state_dict(sd2, strict=True)
        model.reset_cache()
        y2 = L.generate(model, prompt, 20, 20, top_k=1)
        assert model.adapter_kv_caches[1][0].data_ptr() == buf, "the prefix buffer was reallocated"
        assert not torch.equal(model.adapter_kv_caches[1][0], ak1)
        fresh = adapter_model(cfg, v2, sd2)
        y3 = L.generate(fresh, prompt, 20, 20, top_k=1)
        model.reset_cache()
        fresh.reset_cache()
        l2 = model(prompt.view(1, -1), 20, torch.arange(prompt.numel(), device=DEV))
        l3 = fresh(prompt.view(1, -1), 20, torch.arange(prompt.numel(), device=DEV))
    assert torch.equal(y2, y3), f"{y2.tolist()} vs fresh {y3.tolist()}"
    assert torch.equal(l2, l3)


# ---- 6. the stream engine declines adapter models
def test_stream_engine_declines_adapter_models(g):
    from lit_parrot_amd.engine import StreamEngine
    from lit_parrot_amd.generate import base as gb

    cfg, v2 = case_config(g, "llama_gqa")
    for use_v2 in (True, False):
        sd = adapter_state(g, cfg, use_v2)
        model = adapter_model(cfg, use_v2, sd)
        assert "adapter" in StreamEngine.supported(model)
        sess = gb.DecodeSession(model, 24, 24, greedy=True, use_graph=False, engine=True)
        assert sess.eng is None
    base_cfg = Config.from_name(cfg.name)
    base = L.GPT(base_cfg)
    base.load_state_dict({k: v.to(BF) for k, v in synthetic_state_dict(base_cfg, MODEL_SEED, perturb=True).items()}, strict=True)
    base = base.to(BF).to(DEV).eval()
    reason = StreamEngine.supported(base)
    assert reason is None or "adapter" not in reason
    sess = gb.DecodeSession(base, 24, 24, greedy=True, use_graph=False, engine=True)
    assert (sess.eng is not None) == (reason is None)


# ---- 7. quantized Linears with adapter vectors are refused
def test_quantized_linear_with_adapter_parameters_is_refused(g):
    from oracle import int4 as o4

    cfg = A.Config.from_name("tiny-llama", adapter_start_layer=1)
    sd = {k: v.to(BF) for k, v in synthetic_state_dict(cfg, MODEL_SEED, perturb=True).items()}
    qsd = o4.quantize_state_dict(sd, 128, is_linear_key)
    with L.quantization("gptq.int4-g128"):
        model = A.GPT(cfg)
    model.load_state_dict(qsd, strict=False)
    for m in model.modules():
        if hasattr(m, "hip_linear"):
            m.adapter_scale = torch.nn.Parameter(torch.ones(m.out_features), requires_grad=False)
            m.adapter_bias = torch.nn.Parameter(torch.zeros(m.out_features), requires_grad=False)
    model = model.to(BF).to(DEV).eval()
    prompt = torch.arange(5, device=DEV).view(1, -1)
    with torch.no_grad(), pytest.raises(ParrotHipError, match="adapter"):
        model(prompt)


# ---- 8. base models unchanged
def test_base_paths_identical_through_the_adapter_entry_points():
    lib = _hip.load()
    N, K = 352, 256
    W, x = _rand((N, K), 0.05, 20), _rand((1, K), 1.0, 21)
    bias = _rand((N,), 0.05, 22)
    outs = []
    for entry in ("old", "null", "empty"):
        out = torch.empty((1, N), dtype=BF, device=DEV)
        args = (W.data_ptr(), None, x.data_ptr(), K, 1, bias.data_ptr(), None, 0, out.data_ptr(), N, N, K, EPI_NONE, None)
        if entry == "old":
            _hip.check(lib.parrot_bf16_gemv(*args, ops.stream()), "gemv")
        elif entry == "null":
            _hip.check(lib.parrot_bf16_gemv_adapter(*args, None, ops.stream()), "gemv_adapter")
        else:
            _hip.check(lib.parrot_bf16_gemv_adapter(*args, C.byref(_hip.ParrotAdapter(None, None, None, None)), ops.stream()), "gemv_adapter")
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert torch.equal(outs[0], outs[2])  # identity affine (scale 1, bias 0): the same values


def test_adapter_gpt_without_adapted_layers_is_the_base_model():
    cfg = A.Config.from_name("tiny-llama-gqa", adapter_start_layer=2)  # 2 layers: none adapted
    sd = {k: v.to(BF) for k, v in synthetic_state_dict(cfg, MODEL_SEED, perturb=True).items()}
    model = A.GPT(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(BF).to(DEV).eval()
    base = L.GPT(Config.from_name("tiny-llama-gqa"))
    base.load_state_dict(sd, strict=True)
    base = base.to(BF).to(DEV).eval()
    tokens = torch.arange(3, 12, device=DEV).view(1, -1)
    with torch.no_grad():
        assert torch.equal(model(tokens).view(torch.int16), base(tokens).view(torch.int16))
        pos = torch.arange(9, device=DEV)
        assert torch.equal(model(tokens, 16, pos).view(torch.int16), base(tokens, 16, pos).view(torch.int16))
        step = torch.tensor([9], device=DEV)
        assert torch.equal(model(tokens[:, :1], 16, step).view(torch.int16), base(tokens[:, :1], 16, step).view(torch.int16))
