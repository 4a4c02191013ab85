"""Token sampling: greedy, temperature, top-k/top-p — device-side torch ops
on [B, V] logits (the per-step cost is dwarfed by the lm_head GEMM). This
is the grouped path: unseeded requests, engine-wide generator. Requests that
carry a seed, and every eligible request under the engine's fused_sampler
option, sample through ops.sample_rows instead (one launch per step,
per-row parameters, RNG keyed by (seed, output position)).

Matches the reference generation knobs (bee2bee/hf.py:94-103: temperature,
top_p 0.95, repetition_penalty 1.15)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

# the fused sampler (ops.sample_rows) keeps at most this many candidates
from ..ops.reference import SAMPLE_MAX_K as FUSED_MAX_TOP_K


def sanitize_seed(seed) -> Optional[int]:
    """A request's `seed` -> an int in [0, 2^64), or None (unseeded).
    Integers (and floats with an integral value) are taken mod 2^64;
    anything else, bools and NaN/inf included, is None."""
    if isinstance(seed, bool):
        return None
    if isinstance(seed, float):
        if seed != seed or seed in (float("inf"), float("-inf")) \
                or seed != int(seed):
            return None
        seed = int(seed)
    if not isinstance(seed, int):
        return None
    return seed % (1 << 64)


@dataclass
class SamplingParams:
    temperature: float = 0.7
    top_p: float = 0.95
    top_k: int = 64
    repetition_penalty: float = 1.0
    greedy: bool = False
    # a seeded request samples through ops.sample_rows with a counter-based
    # RNG keyed by (seed, output position): the same tokens in any batch
    seed: Optional[int] = None

    def fused_eligible(self) -> bool:
        """Whether ops.sample_rows expresses these params exactly."""
        return self.greedy or 1 <= self.top_k <= FUSED_MAX_TOP_K

    def fused_row(self):
        """(temperature, top_k, top_p, penalty) as ops.sample_rows takes
        them: greedy is top_k 1 at temperature 1, and a top_k the kernel
        cannot hold (0 = off, or above 1024) is served with 1024."""
        if self.greedy:
            return 1.0, 1, 1.0, self.repetition_penalty
        k = self.top_k if 1 <= self.top_k <= FUSED_MAX_TOP_K \
            else FUSED_MAX_TOP_K
        return self.temperature, k, self.top_p, self.repetition_penalty

    @classmethod
    def from_request(
        cls,
        temperature: Optional[float],
        top_p: Optional[float] = None,
        top_k: Optional[int] = None,
        repetition_penalty: Optional[float] = None,
        seed=None,
    ) -> "SamplingParams":
        """Wire/API request knobs -> params, with the REFERENCE's generation
        defaults (bee2bee/hf.py:94-103): temperature 0.7, top_p 0.95,
        repetition_penalty 1.15. temperature <= 1e-4 selects greedy (the
        penalty still applies — matching do_sample=False + penalty in HF)."""
        import math

        t = 0.7 if temperature is None else float(temperature)
        if not math.isfinite(t):
            t = 0.7  # NaN/inf from hostile JSON: fall back to the default
        p = cls(temperature=max(t, 1e-4), greedy=t <= 1e-4)
        if top_p is not None and math.isfinite(float(top_p)):
            p.top_p = float(top_p)
        if top_k is not None:
            p.top_k = max(0, int(top_k))
        rp = (1.15 if repetition_penalty is None
              else float(repetition_penalty))
        p.repetition_penalty = rp if math.isfinite(rp) and rp > 0 else 1.15
        p.seed = sanitize_seed(seed)
        return p


def apply_repetition_penalty(
    logits: torch.Tensor, prev_ids: torch.Tensor, penalty: float
) -> torch.Tensor:
    """prev_ids [B, L] (pad with -1); penalize already-emitted tokens.

    Fully batched: one scatter builds a seen-token mask (pad indices land in
    a sacrificial extra column), one where applies the penalty — no host
    loop, so a large decode batch pays O(1) kernel launches."""
    if penalty == 1.0 or prev_ids.numel() == 0:
        return logits
    B, V = logits.shape
    valid = prev_ids >= 0
    idx = torch.where(valid, prev_ids, torch.full_like(prev_ids, V))
    seen = torch.zeros((B, V + 1), dtype=torch.bool, device=logits.device)
    seen.scatter_(1, idx.long(), True)
    seen = seen[:, :V]
    return torch.where(
        seen,
        torch.where(logits > 0, logits / penalty, logits * penalty),
        logits,
    )


def sample(
    logits: torch.Tensor,
    params: SamplingParams,
    generator: Optional[torch.Generator] = None,
) -> torch.Tensor:
    """logits [B, V] -> next token ids [B] (int64, on device)."""
    if params.greedy:
        return torch.argmax(logits, dim=-1)
    logits = logits.float() / max(params.temperature, 1e-5)
    if params.top_k > 0 and params.top_k < logits.shape[-1]:
        vals, idx = torch.topk(logits, params.top_k, dim=-1)
    else:
        vals, idx = torch.sort(logits, dim=-1, descending=True)
    probs = torch.softmax(vals, dim=-1)
    if 0.0 < params.top_p < 1.0:
        cum = torch.cumsum(probs, dim=-1)
        mask = cum - probs > params.top_p  # keep first token crossing top_p
        probs = probs.masked_fill(mask, 0.0)
        probs = probs / probs.sum(dim=-1, keepdim=True)
    choice = torch.multinomial(probs, 1, generator=generator)
    return idx.gather(-1, choice).squeeze(-1)
