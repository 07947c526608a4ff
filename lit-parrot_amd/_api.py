"""Public names of the package (what ``import lit_parrot_amd`` exposes)."""
from ._hip import ParrotHipError
from .config import Config, name_to_config
from .generate.base import generate, generate_batch, generate_candidates, generate_speculative
from .model import GPT, Block, CausalSelfAttention, GptNeoxMLP, LLaMAMLP, apply_rope, build_rope_cache
from .rmsnorm import RMSNorm
from .score import continuation_logprobs, perplexity, rank_continuations, score_windows, token_logprobs
from .utils import quantization
from .weights import weights_changed

__all__ = [
    "GPT", "Block", "CausalSelfAttention", "GptNeoxMLP", "LLaMAMLP", "RMSNorm", "Config", "name_to_config",
    "generate", "generate_batch", "generate_candidates", "generate_speculative", "quantization", "apply_rope", "build_rope_cache", "ParrotHipError",
    "token_logprobs", "continuation_logprobs", "rank_continuations", "perplexity", "score_windows",
    "weights_changed",
]
