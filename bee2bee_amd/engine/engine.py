"""InferenceEngine: continuous-batching serving front end over the Runner.

Replaces the reference's per-request `transformers.generate()` thread
(bee2bee/hf.py:84-108) with a single engine thread that owns the GPU:
requests are admitted into a running batch (batched varlen prefill), decoded
together one token per step (hipGraph-replayed on GPU), streamed out
per-request, and retired individually. Paged KV blocks are recycled on
retirement, so the 288 GB HBM pool is shared across the whole request mix.
"""
from __future__ import annotations

import json
import logging
import os
import queue
import random
import threading
import time
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Union

import torch

from ..models.spec import ModelSpec, resolve_spec
from ..models.tokenizer import load_tokenizer
from ..models.weights import ModelWeights
from ..utils import new_id, report_engine_throughput
from .graphs import DecodeGraphs, DecodeState
from .kv import PagedKV
from . import kv as kv_mod
from .runner import Runner
from .sampler import SamplingParams, sample

logger = logging.getLogger("bee2bee_amd.engine")

_STREAM_END = object()

# fp8 KV scales file: small JSON, one scale per (layer, kv head)
KV_SCALES_FORMAT = "bee2bee-kv-scales-v1"
# e4m3 finite maximum; calibration maps amax * margin onto it
E4M3_MAX = 448.0
# amax floor: an all-zero head still gets a finite positive scale
KV_AMAX_FLOOR = 1e-6


def load_kv_scales_file(path: str, spec: ModelSpec):
    """Read a KV scales file and validate it against the model spec.
    Returns (k_scale, v_scale) fp32 [n_layers, n_kv_heads]; raises
    ValueError on any mismatch."""
    with open(path, "r", encoding="utf-8") as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("format") != KV_SCALES_FORMAT:
        raise ValueError(
            f"{path}: not a KV scales file (format != {KV_SCALES_FORMAT!r})")
    for key, want in (("n_layers", spec.n_layers),
                      ("n_kv_heads", spec.n_kv_heads)):
        if doc.get(key) != want:
            raise ValueError(
                f"{path}: {key}={doc.get(key)!r} does not match model "
                f"{spec.name} ({key}={want})")
    out = []
    for key in ("k_scale", "v_scale"):
        try:
            t = torch.tensor(doc[key], dtype=torch.float32)
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f"{path}: bad or missing {key}: {e}") from None
        if tuple(t.shape) != (spec.n_layers, spec.n_kv_heads):
            raise ValueError(
                f"{path}: {key} has shape {tuple(t.shape)}, expected "
                f"({spec.n_layers}, {spec.n_kv_heads})")
        out.append(t)
    return out[0], out[1]


# start-up calibration set (serve --kv-scales calibrate): a few natural-
# language/code strings through the model's tokenizer plus a few synthetic
# uniform-random token sequences, so rare-token K/V outliers count too
_CALIBRATION_TEXTS = (
    "The quick brown fox jumps over the lazy dog. " * 8,
    "Q: What is the capital of France?\nA: The capital of France is Paris. "
    "Q: What is 12 times 12?\nA: 144.",
    "def fib(n):\n    a, b = 0, 1\n    for _ in range(n):\n"
    "        a, b = b, a + b\n    return a\n",
    "In 1969, Apollo 11 landed on the Moon; 3.14159 and 2.71828 are "
    "constants, and {\"key\": [1, 2, 3]} is JSON.",
)


def default_calibration_prompts(engine: "InferenceEngine",
                                n_synthetic: int = 4,
                                synthetic_len: int = 256) -> List[List[int]]:
    """The built-in calibration prompts as token-id lists."""
    prompts = [engine.tokenizer.encode(t) for t in _CALIBRATION_TEXTS]
    gen = torch.Generator().manual_seed(20240)
    n = min(synthetic_len, engine.max_seq_len - 1)
    lo = min(4, engine.spec.vocab_size - 1)
    for _ in range(n_synthetic):
        prompts.append(torch.randint(
            lo, engine.spec.vocab_size, (n,), generator=gen).tolist())
    return [p for p in prompts if p]


class TextStreamDecoder:
    """Incrementally turns a growing token list into text deltas: emits the
    first token at once (TTFT), then every `flush_every` tokens, holding
    back a possibly-incomplete multibyte char (at most 3 flushes)."""

    def __init__(self, tokenizer, flush_every: int = 4) -> None:
        self.tokenizer = tokenizer
        self.flush_every = flush_every
        self.decoded_upto = 0
        self.n_seen = 0
        # trailing-replacement hold-back state: a U+FFFD at the stream tail
        # is usually a multibyte char split across the boundary — commit the
        # valid prefix NOW, hold only the trailing replacements, and release
        # them only if the same boundary persists (genuinely invalid bytes)
        self._hold_pos = -1
        self._held_flushes = 0

    def delta(self, output_ids: List[int], final: bool = False) -> str:
        if not final:
            self.n_seen += 1
            if (self.flush_every > 1 and self.n_seen > 1
                    and self.n_seen % self.flush_every != 1):
                return ""
        text = self.tokenizer.decode(output_ids)
        d = text[self.decoded_upto:]
        if final:
            self.decoded_upto = len(text)
            return d
        if not d:
            return ""
        stripped = d.rstrip("\ufffd")
        if len(stripped) != len(d):
            cut = self.decoded_upto + len(stripped)
            if cut == self._hold_pos:
                self._held_flushes += 1
            else:
                self._hold_pos = cut
                self._held_flushes = 1
            # a real utf-8 char completes within 3 more ids, so a boundary
            # stuck longer than that is invalid data — emit it as-is
            if self._held_flushes > 3:
                stripped = d
        self.decoded_upto += len(stripped)
        return stripped


class StopStringFilter:
    """Incremental stop-string truncation for token streams.

    Emits EXACTLY the buffered truncation (cut at the EARLIEST occurrence
    of any stop) without un-saying text. Two hazards make this more than a
    tail hold-back: a stop can straddle chunk boundaries, and a LONGER
    stop completing later can start at an EARLIER position than a short
    stop already visible — so text is withheld from the earliest position
    where any stop is complete OR could still complete, and the cut is
    final only when no earlier candidate remains open. `done` flips when
    the cut is final (callers cancel generation — an improvement over the
    reference's generate-then-truncate, bee2bee/hf.py:111-136)."""

    __slots__ = ("stops", "buf", "n_emitted", "emitted", "done")

    def __init__(self, stops) -> None:
        self.stops = [s for s in (stops or []) if s]
        self.buf = ""
        self.n_emitted = 0
        self.emitted = ""
        self.done = False

    def _earliest_completed(self) -> Optional[int]:
        c = None
        for s in self.stops:
            i = self.buf.find(s, self.n_emitted)
            if i >= 0 and (c is None or i < c):
                c = i
        return c

    def _earliest_open(self) -> Optional[int]:
        """Start of the earliest tail that is a proper prefix of a stop
        (a stop that may still complete with future text)."""
        L = len(self.buf)
        p = None
        for s in self.stops:
            lo = max(self.n_emitted, L - len(s) + 1)
            for k in range(lo, L):
                if self.buf[k:] == s[: L - k]:
                    if p is None or k < p:
                        p = k
                    break
        return p

    def feed(self, delta: str) -> str:
        if self.done or not delta:
            return ""
        self.buf += delta
        c = self._earliest_completed()
        p = self._earliest_open()
        safe = len(self.buf)
        if c is not None:
            safe = min(safe, c)
        if p is not None:
            safe = min(safe, p)
        out = self.buf[self.n_emitted:safe]
        self.n_emitted = max(self.n_emitted, safe)
        self.emitted += out
        if c is not None and (p is None or p >= c):
            self.done = True
        return out

    def flush(self) -> str:
        """End of stream: open candidates are dead; finalize the cut."""
        if self.done:
            return ""
        c = self._earliest_completed()
        end = c if c is not None else len(self.buf)
        out = self.buf[self.n_emitted:end]
        self.n_emitted = end
        self.emitted += out
        if c is not None:
            self.done = True
        return out


@dataclass
class GenerationRequest:
    prompt_ids: List[int]
    max_new_tokens: int = 128
    sampling: SamplingParams = field(default_factory=SamplingParams)
    stop_token_ids: tuple = ()
    rid: str = field(default_factory=lambda: new_id("req"))
    # filled by the engine
    out_queue: "queue.Queue" = field(default_factory=queue.Queue)
    submit_ts: float = field(default_factory=time.time)
    admitted_ts: Optional[float] = None   # left the queue, prefill began
    first_token_ts: Optional[float] = None
    done_ts: Optional[float] = None
    error: Optional[str] = None
    cancelled: bool = False
    output_ids: List[int] = field(default_factory=list)
    # the seed this request's rows carry into ops.sample_rows: its own
    # sampling.seed, or one the engine drew at submit (fused_sampler);
    # None = the request samples on the grouped torch path
    sample_seed: Optional[int] = None
    # optional: called from the engine thread as on_emit(token_id, done);
    # when set, tokens are NOT pushed to out_queue (async consumers use this
    # to avoid one blocking thread per request)
    on_emit: Optional[Any] = None


def _penalize(logits: torch.Tensor, seen: torch.Tensor, p) -> torch.Tensor:
    """Repetition penalty over a seen-token mask: seen logits are divided
    by p when positive, multiplied when not. p: a float, or one per row
    as [rows, 1]."""
    return torch.where(
        seen, torch.where(logits > 0, logits / p, logits * p), logits)


class _Active:
    __slots__ = ("req", "seq_id", "length", "prefilled", "spec_index",
                 "pen_slot")

    def __init__(self, req: GenerationRequest, seq_id: int, length: int) -> None:
        self.req = req
        self.seq_id = seq_id
        self.length = length  # tokens currently in KV cache
        self.prefilled = 0  # prompt tokens prefetched so far (chunked prefill)
        self.spec_index = None  # lazy NGramIndex (speculative proposer)
        self.pen_slot = None    # repetition-penalty seen-mask pool row


class InferenceEngine:
    def __init__(
        self,
        model: str | ModelSpec,
        device: Optional[str] = None,
        dtype: torch.dtype = torch.bfloat16,
        model_path: Optional[str] = None,
        max_batch: int = 64,
        max_seq_len: Optional[int] = None,
        use_graphs: Optional[bool] = None,
        seed: int = 0,
        kv_margin_blocks: int = 8,
        max_prefill_tokens: int = 4096,
        spec_decode: bool = False,
        spec_k: int = 4,
        spec_ngram: int = 2,
        kv_dtype: str = "native",
        kv_scales: Optional[str] = None,
        sliding_window: Optional[int] = None,
        fused_sampler: bool = False,
    ) -> None:
        """fused_sampler: sample every eligible request (greedy, or top_k
        1..1024) through ops.sample_rows, one launch per step whatever the
        parameter mix; off, only requests that carry a seed take it. The
        environment's BEE2BEE_FUSED_SAMPLER=1 switches it on too.

        kv_scales (fp8 KV only): None keeps unit scales; a path loads a
        scales file written by save_kv_scales(); "checkpoint" uses the
        self_attn.k_scale / v_scale tensors of the HF checkpoint. Run
        calibrate_kv_scales() to measure them instead.

        sliding_window: None takes the model spec's value, 0 forces the
        window off. The effective window (self.sliding_window) is 0
        whenever it is >= max_seq_len: no servable context reaches it."""
        if sliding_window is not None and sliding_window < 0:
            raise ValueError("sliding_window must be >= 0 (0 = off)")
        if kv_scales is not None and kv_dtype != "fp8":
            raise ValueError(
                "kv_scales given but the KV cache is not fp8: per-head KV "
                "scales only apply with kv_dtype='fp8'")
        # cap on prompt tokens prefill-batched per step: bounds time-to-first
        # -token for requests behind a burst (they decode while later
        # arrivals prefill)
        self.max_prefill_tokens = max_prefill_tokens
        # speculative decoding (prompt-lookup / n-gram proposer + exact
        # greedy verification over the paged-history prefill path); output-
        # invariant: verified tokens equal plain greedy decode
        self.spec_decode = spec_decode
        self.spec_k = spec_k
        self.spec_ngram = spec_ngram
        self.spec_stats = {"steps": 0, "proposed": 0, "accepted": 0,
                           "delegated": 0}
        self.spec = model if isinstance(model, ModelSpec) else resolve_spec(model, model_path)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        on_gpu = self.device.type == "cuda"
        if not on_gpu and dtype is torch.bfloat16:
            dtype = torch.float32  # CPU reference path runs fp32
        self.dtype = dtype
        self.max_batch = max_batch
        self.max_seq_len = min(max_seq_len or 4096, self.spec.max_seq_len)
        # the decode combine kernel stages <=128 chunk (m,l) pairs in LDS
        # (attn_decode.hip ml_s): clamp at construction instead of raising
        # mid-step and tearing down every active request
        DECODE_MAX_CTX = 128 * 256
        if self.max_seq_len > DECODE_MAX_CTX:
            logger.warning(
                "max_seq_len %d exceeds the decode kernel's %d-token context"
                " limit; clamping", self.max_seq_len, DECODE_MAX_CTX)
            self.max_seq_len = DECODE_MAX_CTX
        # effective sliding window: a query at position i attends keys
        # (i - w, i]. Off (0) when it covers every servable context, so
        # those engines launch the same kernels and keep the same pages
        # as a windowless one
        win = (self.spec.sliding_window if sliding_window is None
               else sliding_window) or 0
        self.sliding_window = int(win) if 0 < win < self.max_seq_len else 0
        # set when release_below() handed pages back: the decode state's
        # block table is rebuilt on the next step
        self._window_released = False
        self.tokenizer = load_tokenizer(
            model_path, self.spec.vocab_size, self.spec.bos_token_id, self.spec.eos_token_id
        )

        if on_gpu:
            # fail loudly if the HIP extension is absent (no silent eager path)
            from .. import ops

            ops.require_hip()

        logger.info(
            "building %s (%.2fB params) on %s dtype=%s max_seq_len=%d "
            "sliding_window=%d",
            self.spec.name,
            self.spec.n_params() / 1e9,
            self.device,
            dtype,
            self.max_seq_len,
            self.sliding_window,
        )
        self.weights = ModelWeights(self.spec, self.device, dtype)
        if model_path:
            self.weights.load_hf(model_path)
        else:
            self.weights.random_init(seed=seed)

        blocks_per_seq = -(-self.max_seq_len // kv_mod.BLOCK_SIZE)
        n_blocks = max_batch * blocks_per_seq + kv_margin_blocks
        # "fp8": OCP e4m3 KV pool — half the decode-attention bytes, with
        # per-(layer, kv head) scales (unit until calibrated or loaded).
        # The speculative path is not fp8-enabled yet and is rejected up
        # front
        self.kv_dtype = kv_dtype
        if kv_dtype == "fp8" and spec_decode:
            raise ValueError("fp8 KV does not support spec_decode yet")
        self.kv = PagedKV(self.spec, self.device, dtype, n_blocks=n_blocks,
                          kv_dtype=kv_dtype)
        self.runner = Runner(self.spec, self.weights, self.kv, self.device,
                             dtype, window=self.sliding_window)
        if kv_scales == "checkpoint":
            ck = self.weights.kv_scales
            if ck is None:
                raise ValueError(
                    "kv_scales='checkpoint' but the checkpoint "
                    f"({model_path or 'random init'}) has no "
                    "self_attn.k_scale / v_scale tensors")
            self.kv.set_scales(ck["k_scale"], ck["v_scale"],
                               source="checkpoint")
        elif kv_scales is not None:
            ks, vs = load_kv_scales_file(kv_scales, self.spec)
            self.kv.set_scales(ks, vs, source="file")

        # MoE captures while every decode bucket takes a capture-safe path:
        # dense all-experts bmm, or the grouped-GEMM kernel (device-side
        # segment sizes, no host sync) — only the padded-bmm fallback above
        # the grouped range blocks capture.
        # spec mode keeps graphs: steps where NO sequence has a proposal
        # delegate to the captured decode path (neutral cost on workloads
        # with nothing to speculate on)
        graphs_ok = on_gpu and (
            not self.spec.is_moe
            or Runner.moe_graph_capturable(self.spec, max_batch)
        )
        self.use_graphs = graphs_ok if use_graphs is None else (use_graphs and graphs_ok)
        self.graphs: Optional[DecodeGraphs] = None
        if self.use_graphs:
            self.graphs = DecodeGraphs(self.runner, max_batch, blocks_per_seq)
        # scratch sequence backing pad rows of graph-bucket batches
        self._scratch_seq = -1
        self.kv.new_seq(self._scratch_seq)
        self.kv.extend_seq(self._scratch_seq, 1)
        # the decode inputs on the device, serving and benchmark alike
        self._decode = DecodeState(self.runner, self.graphs,
                                   self._scratch_seq)

        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed)
        # repetition-penalty seen-token masks: one pooled [slots, V] bool
        # buffer, maintained INCREMENTALLY (prompt scatter at admission, one
        # batched scatter of the sampled tokens per step) — the r2 parity
        # change made penalty 1.15 the wire default, and rebuilding a
        # [B, context] history tensor on the host every step cost ms-scale
        # GIL time on the serving path. Lazy: never allocated for
        # penalty-1.0-only workloads (bench).
        self._pen_pool: Optional[torch.Tensor] = None
        self._pen_free: List[int] = []
        self._pen_slot_cache: Optional[tuple] = None  # (slots, tensor)
        # fused sampler (ops.sample_rows): seeded requests always take it;
        # with fused_sampler on, every eligible request does, under a seed
        # drawn at submit from a HOST generator (the device generator stays
        # untouched, so the legacy path's draws do not move)
        self.fused_sampler = bool(fused_sampler) or (
            os.environ.get("BEE2BEE_FUSED_SAMPLER") == "1")
        self._seed_rng = random.Random(seed)
        self._seed_lock = threading.Lock()
        # per-row parameter tensors of the last fused call, cached against
        # the rows' signature; pos is advanced on the device
        self._fused_cache: Optional[dict] = None

        self._busy_s = 0.0       # engine-thread time inside working steps
        self._busy_steps = 0
        self._born = time.time()
        self._pending: "queue.Queue[GenerationRequest]" = queue.Queue()
        self._active: List[_Active] = []
        # admitted requests whose prompt is longer than one prefill budget:
        # they prefill one chunk per step (vs the paged history) while the
        # active set keeps decoding — chunked prefill
        self._prefilling: List[_Active] = []
        self._next_seq = 0
        self._stop = False
        self._wake = threading.Event()
        self._thread: Optional[threading.Thread] = None
        self._tok_window: List[tuple] = []  # (ts, n_tokens)
        self.total_tokens = 0

    # ------------------------------------------------------------ lifecycle

    def start(self) -> None:
        if self._thread is None:
            self._thread = threading.Thread(target=self._loop, daemon=True, name="engine")
            self._thread.start()

    def shutdown(self) -> None:
        self._stop = True
        self._wake.set()
        if self._thread is not None:
            self._thread.join(timeout=30)
            self._thread = None

    # ------------------------------------------------------- fp8 KV scales

    def _require_idle(self, what: str) -> None:
        if self._active or self._prefilling or not self._pending.empty():
            raise RuntimeError(f"{what} needs an idle engine (requests are "
                               "active or queued)")

    @torch.no_grad()
    def calibrate_kv_scales(
        self, prompts: Sequence[Union[str, Sequence[int]]],
        margin: float = 2.0,
    ) -> None:
        """Measure per-(layer, kv head) fp8 KV scales: run the prompts
        (token-id lists or strings) through the whole-prompt prefill with
        an observer that keeps the running amax of post-RoPE K and of V,
        then set scale = amax * margin / 448. margin=2.0 leaves one binade
        of headroom, which costs e4m3 (a floating format) no relative
        precision in its normal range — it only moves the subnormal floor.
        Not a hot path: torch reductions, one host read at the end."""
        if self.kv_dtype != "fp8":
            raise ValueError("calibrate_kv_scales needs kv_dtype='fp8'")
        if not margin > 0:
            raise ValueError("margin must be positive")
        self._require_idle("calibrate_kv_scales")
        self.kv.check_scales_mutable()
        if not prompts:
            raise ValueError("calibrate_kv_scales needs at least one prompt")
        s, dev = self.spec, self.device
        amax = torch.zeros(2, s.n_layers, s.n_kv_heads, dtype=torch.float32,
                           device=dev)

        def observe(layer_idx, k, v):
            for row, t in ((amax[0, layer_idx], k), (amax[1, layer_idx], v)):
                torch.maximum(row, t.abs().amax(dim=(0, 2)).float(), out=row)

        self.runner.kv_observer = observe
        try:
            for p in prompts:
                ids = self.tokenizer.encode(p) if isinstance(p, str) else list(p)
                ids = ids[: self.max_seq_len - 1] or [self.spec.bos_token_id]
                seq_id = self._next_seq
                self._next_seq += 1
                self.kv.new_seq(seq_id)
                try:
                    n = len(ids)
                    self.kv.extend_seq(seq_id, n)
                    slots = self.kv.slot_mapping(seq_id, range(n))
                    self.runner.forward_prefill(
                        torch.tensor(ids, dtype=torch.int64, device=dev),
                        torch.arange(n, dtype=torch.int32, device=dev),
                        torch.tensor(slots, dtype=torch.int32, device=dev),
                        torch.tensor([0, n], dtype=torch.int32, device=dev),
                        n,
                    )
                finally:
                    self.kv.free_seq(seq_id)
        finally:
            self.runner.kv_observer = None
        amax = amax.cpu()  # the one host read
        if not bool(torch.isfinite(amax).all()):
            raise RuntimeError("calibration saw non-finite K/V values")
        scale = amax.clamp_min(KV_AMAX_FLOOR) * (float(margin) / E4M3_MAX)
        self.kv.set_scales(scale[0], scale[1], source="calibrated")

    def save_kv_scales(self, path: str) -> None:
        """Write the current scales as a small JSON file that
        InferenceEngine(..., kv_scales=path) loads back bit-equal."""
        if self.kv_dtype != "fp8":
            raise ValueError("save_kv_scales needs kv_dtype='fp8'")
        doc = {
            "format": KV_SCALES_FORMAT,
            "model": self.spec.name,
            "n_layers": self.spec.n_layers,
            "n_kv_heads": self.spec.n_kv_heads,
            "k_scale": self.kv.k_scale.cpu().tolist(),
            "v_scale": self.kv.v_scale.cpu().tolist(),
        }
        with open(path, "w", encoding="utf-8") as f:
            json.dump(doc, f)

    # -------------------------------------------------------------- serving

    def submit(self, req: GenerationRequest) -> GenerationRequest:
        # empty prompts become [bos] at admission (engine loop); <1
        # max_new behaves as 1 (prefill completion always emits one token)
        req.max_new_tokens = max(1, int(req.max_new_tokens))
        sp = req.sampling
        if sp.seed is not None:
            req.sample_seed = sp.seed % (1 << 64)
        elif self.fused_sampler and sp.fused_eligible():
            with self._seed_lock:
                req.sample_seed = self._seed_rng.getrandbits(64)
        self.start()
        self._pending.put(req)
        self._wake.set()
        return req

    def generate(
        self,
        prompt_ids: List[int],
        max_new_tokens: int = 128,
        temperature: Optional[float] = 0.7,
        stop_token_ids: tuple = (),
        on_token=None,
        top_p: Optional[float] = None,
        top_k: Optional[int] = None,
        repetition_penalty: Optional[float] = None,
        seed: Optional[int] = None,
    ) -> GenerationRequest:
        """Blocking convenience wrapper: submit + drain the stream. With a
        seed the sampled tokens are a function of the request alone."""
        req = GenerationRequest(
            prompt_ids=list(prompt_ids),
            max_new_tokens=max_new_tokens,
            sampling=SamplingParams.from_request(
                temperature, top_p, top_k, repetition_penalty, seed),
            stop_token_ids=tuple(stop_token_ids),
        )
        self.submit(req)
        while True:
            item = req.out_queue.get()
            if item is _STREAM_END:
                break
            if on_token is not None:
                on_token(item)
        if req.error:
            raise RuntimeError(req.error)
        return req

    def generate_text(
        self,
        prompt: str,
        max_new_tokens: int = 128,
        temperature: Optional[float] = 0.7,
        on_text=None,
        stop: Optional[List[str]] = None,
        repetition_penalty: Optional[float] = None,
        top_p: Optional[float] = None,
        top_k: Optional[int] = None,
        cancel=None,
        seed: Optional[int] = None,
    ) -> Dict[str, Any]:
        """Text-level wrapper used by the mesh service. `stop` strings
        truncate the output at the first occurrence (reference stop-word
        scan, bee2bee/hf.py:111-136). `cancel` (a threading.Event) stops
        generation at the next emitted token — a disconnected client must
        not keep burning decode steps."""
        t0 = time.time()
        ids = self.tokenizer.encode(prompt)
        ids = ids[-(self.max_seq_len - max_new_tokens - 1) :]
        # emit the first token at once (TTFT), then flush every few tokens:
        # per-token queue/HTTP hops dominate the serving path at high
        # concurrency; split multibyte chars are held back by the decoder,
        # split stop strings by the stop filter (which also cancels
        # generation the moment a stop completes)
        decoder = TextStreamDecoder(self.tokenizer, flush_every=4)
        stop_filter = StopStringFilter(stop)

        def _on_token(tok: int) -> None:
            if on_text is None:
                return
            out = stop_filter.feed(decoder.delta(req.output_ids))
            if out:
                on_text(out)
            if stop_filter.done:
                req.cancelled = True

        stop_ids = ()
        eos = getattr(self.tokenizer, "eos_token_id", None)
        if eos is not None:
            stop_ids = (eos,)
        sp = SamplingParams.from_request(temperature, top_p, top_k,
                                         repetition_penalty, seed)
        req = GenerationRequest(
            prompt_ids=ids,
            max_new_tokens=max_new_tokens,
            sampling=sp,
            stop_token_ids=stop_ids,
        )
        self.submit(req)
        while True:
            item = req.out_queue.get()
            if item is _STREAM_END:
                break
            _on_token(item)
            if cancel is not None and cancel.is_set():
                req.cancelled = True  # engine stops at the next step
        if req.error:
            raise RuntimeError(req.error)
        text = self.tokenizer.decode(req.output_ids)
        if stop:
            cut = min(
                (text.find(w) for w in stop if w and text.find(w) >= 0),
                default=-1,
            )
            if cut >= 0:
                text = text[:cut]
        if on_text is not None:
            tail = stop_filter.feed(decoder.delta(req.output_ids, final=True))
            tail += stop_filter.flush()
            if tail:
                on_text(tail)
        now = time.time()
        ft = req.first_token_ts or now
        adm = req.admitted_ts or req.submit_ts
        return {
            "text": text,
            "tokens": len(req.output_ids),
            "latency_ms": int((now - t0) * 1000),
            "ttft_ms": int((ft - t0) * 1000),
            # per-stage request trace (the reference reports one opaque
            # latency_ms; SURVEY §5 calls for stage timestamps)
            "timing": {
                "queue_ms": int((adm - req.submit_ts) * 1000),
                "prefill_ms": int((ft - adm) * 1000),
                "decode_ms": int(((req.done_ts or now) - ft) * 1000),
            },
        }

    # ---------------------------------------------------------- engine loop

    def _loop(self) -> None:
        prof = None
        if os.environ.get("BEE2BEE_PROFILE_ENGINE") == "1":
            import cProfile

            prof = cProfile.Profile()
            prof.enable()
        while not self._stop:
            t0 = time.perf_counter()
            try:
                did_work = self._step()
            except Exception as e:  # engine errors fail all active requests
                logger.exception("engine step failed")
                for a in self._active + self._prefilling:
                    a.req.error = str(e)
                    if a.req.on_emit is not None:
                        try:
                            a.req.on_emit(None, True)
                        except Exception:
                            pass
                    else:
                        a.req.out_queue.put(_STREAM_END)
                    self.kv.free_seq(a.seq_id)
                    self._pen_release(a)
                self._active.clear()
                self._prefilling.clear()
                did_work = True
            if did_work:
                self._busy_s += time.perf_counter() - t0
                self._busy_steps += 1
            if not did_work:
                self._wake.wait(timeout=0.05)
                self._wake.clear()
        if prof is not None:
            import pstats

            prof.disable()
            os.makedirs("gpurun_out", exist_ok=True)
            with open("gpurun_out/engine_profile.txt", "w") as f:
                st = pstats.Stats(prof, stream=f)
                st.sort_stats("tottime").print_stats(40)
                st.sort_stats("cumulative").print_stats(40)

    def _step(self) -> bool:
        admitted = self._admit()
        worked = bool(admitted) or bool(self._prefilling)
        if worked:
            self._prefill(self._prefilling + admitted)
        if self._active:
            if self.spec_decode:
                self._decode_spec_once()
            else:
                self._decode_once()
            return True
        return worked

    def _release_window(self, a: "_Active") -> None:
        """Hand back the pages of `a` that lie wholly below the attention
        window of every query still to come: the next one sits at position
        a.length (committed length), so keys < a.length + 1 - window are
        dead. Call only with a.length at a COMMITTED length (after
        speculative acceptance, never on the speculative extension)."""
        if self.sliding_window and self.kv.release_below(
                a.seq_id, a.length + 1 - self.sliding_window):
            self._window_released = True

    def _need_blocks(self, prompt_len: int, max_new: int) -> int:
        need_len = min(prompt_len + max_new, self.max_seq_len)
        return -(-need_len // self.kv.block_size)

    def _admit(self) -> List[_Active]:
        admitted: List[_Active] = []
        admit_tokens = 0
        # blocks the current residents will still grow into: admission must
        # leave room for them or a later extend_seq blows the pool mid-step
        reserved = 0
        for a in self._active + self._prefilling:
            need = self._need_blocks(len(a.req.prompt_ids), a.req.max_new_tokens)
            reserved += max(0, need - self.kv.seq_n_blocks(a.seq_id))
        # count in-flight chunked prefills too: they join _active later and
        # must not push it past max_batch (graph buckets size to it)
        while (len(self._active) + len(self._prefilling) + len(admitted)
               < self.max_batch):
            if admitted and admit_tokens >= self.max_prefill_tokens:
                break
            try:
                req = self._pending.get_nowait()
            except queue.Empty:
                break
            blocks_needed = self._need_blocks(
                len(req.prompt_ids), req.max_new_tokens
            )
            if self.kv.free_blocks - reserved < blocks_needed:
                # out of KV memory: push back and wait for retirements
                self._pending.put(req)
                break
            reserved += blocks_needed
            seq_id = self._next_seq
            self._next_seq += 1
            self.kv.new_seq(seq_id)
            a_new = _Active(req, seq_id, 0)
            if req.sampling.repetition_penalty != 1.0:
                self._pen_assign(a_new)
            admitted.append(a_new)
            admit_tokens += len(req.prompt_ids)
        return admitted

    @torch.no_grad()
    def _prefill(self, queue_: List[_Active]) -> None:
        """Prefill up to max_prefill_tokens prompt tokens across the queued
        requests. Whole prompts take the packed varlen fast path; prompts
        longer than the budget prefill in chunks against their paged history
        (ops.attn_prefill_paged) across successive steps."""
        budget = self.max_prefill_tokens
        batch: List[tuple] = []  # (active, start, take)
        n_consumed = 0
        now_admit = time.time()
        for a in queue_:
            if budget <= 0:
                break
            if a.prefilled == 0:
                if a.req.admitted_ts is None:
                    a.req.admitted_ts = now_admit
                p = a.req.prompt_ids or [self.spec.bos_token_id]
                p = p[: self.max_seq_len - a.req.max_new_tokens - 1] or p[:1]
                a.req.prompt_ids = p
            take = min(len(a.req.prompt_ids) - a.prefilled, budget)
            batch.append((a, a.prefilled, take))
            budget -= take
            n_consumed += 1
        # keep EVERYTHING in _prefilling until this step succeeds, so a
        # mid-prefill failure reaches the error path (which fails + frees
        # _active and _prefilling) instead of orphaning admitted requests
        self._prefilling = list(queue_)

        whole = all(
            start == 0 and take == len(a.req.prompt_ids)
            for a, start, take in batch
        )
        hidden, cu = self._forward_packed(
            [(a, start, a.req.prompt_ids[start : start + take])
             for a, start, take in batch], paged=not whole)
        for a, start, take in batch:  # the chunk is committed
            a.prefilled = a.length = start + take
            self._release_window(a)
        self._prefilling = [
            a
            for a, start, take in batch
            if start + take < len(a.req.prompt_ids)
        ] + [t for t in queue_[n_consumed:]]
        # sample only for requests whose whole prompt is now in the cache
        done_idx = [
            i
            for i, (a, start, take) in enumerate(batch)
            if start + take == len(a.req.prompt_ids)
        ]
        if not done_idx:
            return
        completed = [batch[i][0] for i in done_idx]
        last_rows = self._dev([cu[i + 1] - 1 for i in done_idx], torch.int64)
        logits = self.runner.lm_head(hidden[last_rows])
        self._sample_and_emit(completed, logits)
        # a request can finish AT prefill (max_new=1 / instant stop token):
        # retire it here or its KV blocks leak until shutdown
        self._active.extend(self._retire(completed))

    def _dev(self, values: Sequence[int], dtype: torch.dtype) -> torch.Tensor:
        """Host list -> device tensor, without the synchronizing pageable
        copy of torch.tensor(..., device=cuda)."""
        return torch.tensor(values, dtype=dtype).to(self.device,
                                                    non_blocking=True)

    def _forward_packed(self, items: List[tuple], paged: bool):
        """Grow each sequence by its tokens and run them as one packed
        varlen batch. items: (active, start, tokens), the tokens sitting at
        positions start.. of the sequence. paged=True attends each
        sequence's paged history below `start` as well (chunked prefill,
        speculative verify). Returns (hidden [T, H], cu host list)."""
        ids_list, pos_list, slot_list, cu = [], [], [], [0]
        for a, start, toks in items:
            span = range(start, start + len(toks))
            self.kv.extend_seq(a.seq_id, span.stop)
            ids_list.extend(toks)
            pos_list.extend(span)
            slot_list.extend(self.kv.slot_mapping(a.seq_id, span))
            cu.append(cu[-1] + len(toks))
        qlens = [len(toks) for _, _, toks in items]
        args = (self._dev(ids_list, torch.int64),
                self._dev(pos_list, torch.int32),
                self._dev(slot_list, torch.int32),
                self._dev(cu, torch.int32), max(qlens))
        if not paged:
            return self.runner.forward_prefill(*args), cu
        bt = self.kv.block_table([a.seq_id for a, _, _ in items])
        seq_lens = torch.tensor(
            [start + q for (_, start, _), q in zip(items, qlens)],
            dtype=torch.int32, device=self.device)
        hidden = self.runner.forward_prefill(
            *args, block_table=bt, seq_lens=seq_lens,
            query_lens=self._dev(qlens, torch.int32))
        return hidden, cu

    def _retire(self, acts: List[_Active]) -> List[_Active]:
        """Free the KV pages and penalty rows of the finished requests in
        `acts`; returns the ones still running."""
        done = [a for a in acts if a.req.done_ts is not None]
        if not done:
            return acts
        for a in done:
            self.kv.free_seq(a.seq_id)
            self._pen_release(a)
        return [a for a in acts if a.req.done_ts is None]

    @torch.no_grad()
    def _decode_once(self) -> None:
        """One decode step over the active set.

        Host work is incremental: the decode state's device-side inputs
        persist across steps and are bumped in place; full rebuilds happen
        only when the active set changed membership or was stepped by
        another path (speculative verify), and block tables are re-read
        only when a sequence crosses a KV-block boundary (every block_size
        tokens) or releases a window page."""
        # pages released below the window since the last step: their table
        # entries now read 0
        blocks_changed = self._window_released
        self._window_released = False
        for a in self._active:
            nblk0 = (a.length + self.kv.block_size - 1) // self.kv.block_size
            self.kv.extend_seq(a.seq_id, a.length + 1)
            nblk1 = (a.length + self.kv.block_size) // self.kv.block_size
            blocks_changed |= nblk1 != nblk0

        seqs = [a.seq_id for a in self._active]
        st = self._decode
        next_ids = st.pending(seqs)
        if next_ids is not None:
            st.advance(next_ids, blocks_changed)
        else:
            st.load(seqs,
                    [(a.req.output_ids or a.req.prompt_ids)[-1]
                     for a in self._active],
                    [a.length for a in self._active])
        logits = st.logits()

        for a in self._active:
            a.length += 1
            self._release_window(a)
        # only this step hands ids to the decode state: ids sampled for any
        # other batch (prefill completions, speculative subsets) would feed
        # these sequences their neighbours' tokens
        st.hold(seqs, self._sample_and_emit(self._active, logits))
        self._active = self._retire(self._active)

    # ------------------------------------------------- speculative decoding

    def _propose(self, a: "_Active", ids: List[int], k: int) -> List[int]:
        """Longest-match-first prompt-lookup via an incremental per-sequence
        n-gram index (engine/spec.py) — covers prompt AND output history at
        O(1) maintenance per token instead of the O(context) rescan of the
        naive scan; n sizes tried {spec_ngram+2, spec_ngram+1, spec_ngram}."""
        if k <= 0:
            return []
        idx = a.spec_index
        if idx is None:
            from .spec import NGramIndex

            n = self.spec_ngram
            idx = NGramIndex(ids, ns=(n + 2, n + 1, n))
            a.spec_index = idx
        else:
            idx.sync(ids)
        return idx.propose(k)

    @torch.no_grad()
    def _decode_spec_once(self) -> None:
        """One speculative step: each greedy sequence verifies its pending
        token plus up to spec_k proposed tokens in ONE forward through the
        chunked-prefill (paged-history) path; the accepted prefix is exactly
        what plain greedy decode would emit (verification is exact)."""
        acts = self._active
        # propose first: when nothing is speculatable this step, take the
        # plain (hipGraph-captured) decode path instead of the slower
        # verify-forward — spec mode then costs ~nothing on workloads
        # without self-similarity
        props = self._spec_propose(acts)
        if not any(props):
            self.spec_stats["delegated"] += 1
            self._decode_once()
            return
        logits, cu = self._spec_verify(acts, props)
        self._spec_accept(acts, props, logits, cu)
        self.spec_stats["steps"] += 1
        # the sequences moved on without the decode state
        self._decode.forget()
        self._active = self._retire(acts)

    def _spec_propose(self, acts: List[_Active]) -> List[List[int]]:
        """Up to spec_k proposed tokens per sequence ([] = none)."""
        props: List[List[int]] = []
        for a in acts:
            r = a.req
            prop: List[int] = []
            # greedy with repetition penalty is ALSO speculatable: the
            # verify pass applies the penalty exactly (seen-mask + the
            # in-window proposal prefix) before each argmax
            if r.sampling.greedy and (
                    r.sampling.repetition_penalty == 1.0
                    or a.pen_slot is not None):
                room = self.max_seq_len - (a.length + 1) - 1
                rem = r.max_new_tokens - len(r.output_ids) - 1
                kcap = min(self.spec_k, room, rem)
                prop = self._propose(a, r.prompt_ids + r.output_ids, kcap)
            props.append(prop)
        return props

    def _spec_verify(self, acts: List[_Active], props: List[List[int]]):
        """One forward over every sequence's pending token plus its
        proposal, against the paged history: logits for all verify rows,
        and the host list of row offsets per sequence."""
        hidden, cu = self._forward_packed(
            [(a, a.length, [(a.req.output_ids or a.req.prompt_ids)[-1]] + prop)
             for a, prop in zip(acts, props)], paged=True)
        return self.runner.lm_head(hidden), cu

    def _spec_accept(self, acts: List[_Active], props: List[List[int]],
                     logits: torch.Tensor, cu: List[int]) -> None:
        """Emit, per sequence, the longest verified prefix of its proposal
        plus the one token the model gives after it."""
        greedy_idx = [i for i, a in enumerate(acts)
                      if a.req.sampling.greedy
                      and a.req.sampling.repetition_penalty == 1.0]
        pen_idx = [i for i, a in enumerate(acts)
                   if a.req.sampling.greedy
                   and a.req.sampling.repetition_penalty != 1.0
                   and a.pen_slot is not None]
        handled = set(greedy_idx) | set(pen_idx)
        nong = [a for i, a in enumerate(acts) if i not in handled]
        if greedy_idx:
            argmax = logits.argmax(dim=-1).cpu()
        pen_argmax = {}
        if pen_idx:
            # penalized argmax under the BASE seen mask for every verify
            # row in one batch + one sync; in-window corrections happen on
            # the host walk below
            row_ids, row_act, row_p = [], [], []
            for i in pen_idx:
                q = cu[i + 1] - cu[i]
                row_ids.extend(range(cu[i], cu[i] + q))
                row_act.extend([i] * q)
                row_p.extend([acts[i].req.sampling.repetition_penalty] * q)
            rid = self._dev(row_ids, torch.int64)
            slot_t = self._dev([acts[i].pen_slot for i in row_act],
                               torch.int64)
            p_t = self._dev(row_p, torch.float32).unsqueeze(1)
            pa = _penalize(logits[rid].float(), self._pen_pool[slot_t],
                           p_t).argmax(dim=-1).cpu()
            for k, row in enumerate(row_ids):
                pen_argmax[row] = int(pa[k])
        now = time.time()
        n_emitted = 0
        pen_new_slots: List[int] = []
        pen_new_toks: List[int] = []
        for i in greedy_idx + pen_idx:
            a, r, prop = acts[i], acts[i].req, props[i]
            self.spec_stats["proposed"] += len(prop)
            emitted: List[int] = []
            j = 0
            if a.req.sampling.repetition_penalty == 1.0:
                while True:
                    tok = int(argmax[cu[i] + j])
                    emitted.append(tok)
                    if (j < len(prop) and tok == prop[j]
                            and tok not in r.stop_token_ids):
                        j += 1
                        continue
                    break
            else:
                # exact penalized walk: row j's base-mask argmax is exact
                # unless it collides with a token proposed EARLIER in this
                # window (whose in-window penalty could demote it) — at a
                # collision, truncate acceptance (still exact: every
                # emitted token equals what plain penalized decode emits)
                window: set = set()
                while True:
                    tok = pen_argmax[cu[i] + j]
                    if j > 0 and tok in window:
                        break  # ambiguous under in-window penalty: stop
                    emitted.append(tok)
                    if (j < len(prop) and tok == prop[j]
                            and tok not in r.stop_token_ids):
                        window.add(tok)
                        j += 1
                        continue
                    break
            self.spec_stats["accepted"] += j
            # rewind the KV length past rejected proposals (their stored
            # keys get overwritten; attention never reads past seq_len)
            a.length += len(emitted)
            self.kv.extend_seq(a.seq_id, a.length)
            # release from the accepted length only; the roll-back above
            # never reaches below it
            self._release_window(a)
            for tok in emitted:
                if r.done_ts is not None:
                    break
                if a.pen_slot is not None:
                    pen_new_slots.append(a.pen_slot)
                    pen_new_toks.append(tok)
                n_emitted += 1
                self._emit(a, tok, now)
        if n_emitted:
            self._note_throughput(n_emitted, now)
        # mark penalized-greedy emissions seen (one batched scatter)
        if pen_new_slots:
            self._pen_pool[self._dev(pen_new_slots, torch.int64),
                           self._dev(pen_new_toks, torch.int64)] = True
        if nong:
            # non-greedy requests take the plain one-token path
            rows = self._dev([cu[i + 1] - 1 for i in range(len(acts))
                              if i not in handled], torch.int64)
            for a in nong:
                a.length += 1
                self._release_window(a)
            self._sample_and_emit(nong, logits[rows])

    def _pen_slots_t(self, slots: List[int]) -> torch.Tensor:
        """Device tensor of pen-pool slots, cached against the slot list
        (the active set changes far less often than it steps)."""
        key = tuple(slots)
        cached = self._pen_slot_cache
        if cached is not None and cached[0] == key:
            return cached[1]
        t = torch.tensor(slots, dtype=torch.int64, device=self.device)
        self._pen_slot_cache = (key, t)
        return t

    def _pen_assign(self, a: "_Active") -> None:
        """Give a penalized request a seen-mask row seeded with its prompt."""
        V = self.spec.vocab_size
        if self._pen_pool is None:
            n = self.max_batch + 8
            self._pen_pool = torch.zeros(n, V, dtype=torch.bool,
                                         device=self.device)
            self._pen_free = list(range(n))
        if not self._pen_free:
            return  # degrade: penalty falls back to the host rebuild below
        slot = self._pen_free.pop()
        a.pen_slot = slot
        row = self._pen_pool[slot]
        row.zero_()
        ids = torch.tensor(a.req.prompt_ids, dtype=torch.int64,
                           device=self.device)
        row[ids] = True

    def _pen_release(self, a: "_Active") -> None:
        if a.pen_slot is not None:
            self._pen_free.append(a.pen_slot)
            a.pen_slot = None

    def _emit(self, a: _Active, tok: int, now: float) -> bool:
        """Record one token of a request and hand it to its consumer;
        returns whether the request is done with it."""
        r = a.req
        if r.first_token_ts is None:
            r.first_token_ts = now
        r.output_ids.append(tok)
        done = (r.cancelled or tok in r.stop_token_ids
                or len(r.output_ids) >= r.max_new_tokens)
        if done:
            r.done_ts = now
        if r.on_emit is not None:
            try:
                r.on_emit(tok, done)
            except Exception:
                logger.exception("on_emit callback failed")
        else:
            r.out_queue.put(tok)
            if done:
                r.out_queue.put(_STREAM_END)
        return done

    def _sample_and_emit(self, acts: List[_Active],
                         logits: torch.Tensor) -> torch.Tensor:
        """Sample one token per row of logits [len(acts), V] and emit it;
        returns the sampled ids on the device."""
        fused = self._fused_rows(acts)
        if fused is None:
            next_dev = self._sample_grouped(acts, logits)
        else:
            # ONE launch for every fused row, whatever the parameter mix;
            # rows of the grouped path ride along as greedy and are
            # overwritten below, so the fused rows need no gather
            next_dev = self._sample_fused(acts, logits, fused)
            rest = [i for i, f in enumerate(fused) if not f]
            if rest:
                idx = self._dev(rest, torch.int64)
                next_dev[idx] = self._sample_grouped(
                    [acts[i] for i in rest], logits[idx])
        # mark the freshly sampled tokens seen (one batched device scatter)
        if self._pen_pool is not None:
            pen_idx = [i for i, a in enumerate(acts) if a.pen_slot is not None]
            if len(pen_idx) == len(acts):
                self._pen_pool[
                    self._pen_slots_t([a.pen_slot for a in acts]), next_dev
                ] = True
            elif pen_idx:
                slot_t = self._pen_slots_t([acts[i].pen_slot for i in pen_idx])
                idx_t = torch.tensor(pen_idx, dtype=torch.int64,
                                     device=logits.device)
                self._pen_pool[slot_t, next_dev[idx_t]] = True
        next_ids = next_dev.cpu()  # the one host sync per step (emission)
        now = time.time()
        for i, a in enumerate(acts):
            self._emit(a, int(next_ids[i]), now)
        self._note_throughput(len(acts), now)
        return next_dev

    def _fused_rows(self, acts: List[_Active]) -> Optional[List[bool]]:
        """Which rows sample through ops.sample_rows; None when none does.
        A row does when its request carries a sample seed (its own, or one
        drawn at submit under fused_sampler), unless it needs a penalty
        mask and the seen pool had no row left for it."""
        if not any(a.req.sample_seed is not None for a in acts):
            return None
        fused = [
            a.req.sample_seed is not None and (
                a.req.sampling.repetition_penalty == 1.0
                or a.pen_slot is not None)
            for a in acts
        ]
        return fused if any(fused) else None

    def _sample_fused(self, acts: List[_Active], logits: torch.Tensor,
                      fused: List[bool]) -> torch.Tensor:
        """One ops.sample_rows call over all rows of logits. The per-row
        parameter tensors are cached against the rows' signature; while it
        holds, only pos moves, on the device. No [rows, V] gather: the seen
        pool and the slot indices go straight in."""
        from .. import ops

        sig = tuple((a.seq_id, f) for a, f in zip(acts, fused))
        pos = [len(a.req.output_ids) if f else 0
               for a, f in zip(acts, fused)]
        c = self._fused_cache
        if c is not None and c["sig"] == sig and c["pos"] == pos:
            c["pos_t"].add_(c["step"])
        else:
            temp, topk, topp, pen, slot, seed, step = [], [], [], [], [], [], []
            for a, f in zip(acts, fused):
                t, k, p, rp = (a.req.sampling.fused_row() if f
                               else (1.0, 1, 1.0, 1.0))
                temp.append(t)
                topk.append(k)
                topp.append(p)
                pen.append(rp)
                slot.append(a.pen_slot if f and a.pen_slot is not None
                            and rp != 1.0 else -1)
                s = a.req.sample_seed if f else 0
                seed.append(s - (1 << 64) if s >= (1 << 63) else s)
                step.append(1 if f else 0)
            fl = self._dev([temp, topp, pen], torch.float32)
            it = self._dev([topk, slot, pos, step], torch.int32)
            c = self._fused_cache = {
                "sig": sig, "temp": fl[0], "topp": fl[1], "pen": fl[2],
                "topk": it[0], "slot": it[1], "pos_t": it[2], "step": it[3],
                "seed": self._dev(seed, torch.int64),
                "use_pool": any(s >= 0 for s in slot),
            }
        # where this call leaves the host's view of pos, if every fused row
        # emits its token
        c["pos"] = [p + 1 if f else 0 for p, f in zip(pos, fused)]
        return ops.sample_rows(
            logits, c["temp"], c["topk"], c["topp"], c["pen"],
            self._pen_pool if c["use_pool"] else None, c["slot"], c["seed"],
            c["pos_t"])

    def _sample_grouped(self, acts: List[_Active],
                        logits: torch.Tensor) -> torch.Tensor:
        """The grouped torch path: one sample() per distinct parameter set,
        every row drawing from the engine-wide device generator. Returns
        the sampled ids [len(acts)] on the device."""
        # group rows by sampling params so each group is one sample() call
        groups: Dict[tuple, List[int]] = {}
        for i, a in enumerate(acts):
            sp = a.req.sampling
            groups.setdefault(
                (sp.greedy, sp.temperature, sp.top_p, sp.top_k,
                 sp.repetition_penalty), []
            ).append(i)
        # CAUTION (measured): torch.tensor(..., device=cuda) on this path
        # is a pageable H2D copy that synchronizes with the busy stream —
        # profiled at ~0.8 ms per call, 68% of the engine thread under
        # load. The single-group case (uniform sampling params — the
        # common serving mix) therefore indexes nothing, and the penalty
        # slot tensors are cached against the active-set signature.
        single = len(groups) == 1
        next_dev = None if single else torch.empty(
            len(acts), dtype=torch.int64, device=logits.device
        )
        for key, rows in groups.items():
            sp = acts[rows[0]].req.sampling
            gen = self._gen if self.device.type == "cuda" else None
            if single:
                idx = None
                grp_logits = logits
            else:
                idx = torch.tensor(rows, dtype=torch.int64,
                                   device=logits.device)
                grp_logits = logits[idx]
            if sp.repetition_penalty != 1.0:
                slots = [acts[r].pen_slot for r in rows]
                if self._pen_pool is not None and all(
                        sl is not None for sl in slots):
                    grp_logits = _penalize(
                        grp_logits.float(),
                        self._pen_pool[self._pen_slots_t(slots)],
                        sp.repetition_penalty)
                else:
                    # pool exhausted fallback: host-rebuilt history
                    from .sampler import apply_repetition_penalty

                    width = max(
                        (len(acts[r].req.output_ids)
                         + len(acts[r].req.prompt_ids))
                        for r in rows
                    )
                    prev = torch.full((len(rows), width), -1,
                                      dtype=torch.int64)
                    for j, r in enumerate(rows):
                        ids = acts[r].req.prompt_ids + acts[r].req.output_ids
                        prev[j, : len(ids)] = torch.tensor(
                            ids, dtype=torch.int64)
                    grp_logits = apply_repetition_penalty(
                        grp_logits.float(), prev.to(grp_logits.device),
                        sp.repetition_penalty,
                    )
            toks = sample(grp_logits, sp, generator=gen)
            if single:
                next_dev = toks
            else:
                next_dev[idx] = toks
        return next_dev

    def stats(self) -> Dict[str, Any]:
        """Live engine observability (served at the API home endpoint)."""
        now = time.time()
        span = (now - self._tok_window[0][0]) if len(self._tok_window) > 1 else 1.0
        tps = sum(x[1] for x in self._tok_window) / max(span, 1e-3)
        out = {
            "model": self.spec.name,
            "device": str(self.device),
            "kv_dtype": self.kv_dtype,
            "kv_scales": self.kv.scales_source,
            "max_seq_len": self.max_seq_len,
            # effective sliding window (0 = full causal attention)
            "sliding_window": self.sliding_window,
            "active_requests": len(self._active),
            "prefilling_requests": len(self._prefilling),
            "queued_requests": self._pending.qsize(),
            "kv_free_blocks": self.kv.free_blocks,
            "kv_total_blocks": self.kv.n_blocks,
            "tokens_total": self.total_tokens,
            "tokens_per_sec_10s": round(tps, 1),
            "decode_graphs": self.graphs is not None,
            "engine_busy_s": round(self._busy_s, 2),
            "engine_steps": self._busy_steps,
            "engine_ms_per_step": round(
                1e3 * self._busy_s / max(self._busy_steps, 1), 2),
        }
        if self.spec_decode:
            out["spec_decode"] = dict(self.spec_stats)
        return out

    def _note_throughput(self, n: int, now: float) -> None:
        self.total_tokens += n
        self._tok_window.append((now, n))
        cutoff = now - 10.0
        while self._tok_window and self._tok_window[0][0] < cutoff:
            self._tok_window.pop(0)
        span = now - self._tok_window[0][0] if len(self._tok_window) > 1 else 1.0
        tps = sum(x[1] for x in self._tok_window) / max(span, 1e-3)
        report_engine_throughput(tps)

    # ------------------------------------------------ direct batch API (bench)

    @torch.no_grad()
    def bench_prefill(self, batch: int, prompt_len: int, seed: int = 1234,
                      max_new: Optional[int] = None,
                      distinct: Optional[int] = None) -> List[int]:
        """Fill the KV cache with synthetic prompts; returns seq_ids.
        max_new must leave room for the prompt under max_seq_len or the
        admission truncation rule will cut the prompts short (a 10**9
        sentinel used to truncate every bench prompt to one token).

        distinct=D < batch prefills only the first D prompts; sequence j >= D
        reuses prompt j % D and gets a COPY of its KV in blocks of its own,
        so a decode step still reads batch * prompt_len tokens of KV from
        distinct addresses while set-up costs D prompts of prefill."""
        if max_new is None:
            max_new = max(1, self.max_seq_len - prompt_len - 1)
        assert prompt_len + max_new < self.max_seq_len + 1, "prompt would truncate"
        gen = torch.Generator().manual_seed(seed)
        seq_ids = []
        for b in range(batch):
            seq_id = self._next_seq
            self._next_seq += 1
            self.kv.new_seq(seq_id)
            seq_ids.append(seq_id)
        ids = torch.randint(
            4, self.spec.vocab_size, (batch, prompt_len), generator=gen
        )
        n_src = batch if distinct is None else max(1, min(distinct, batch))
        acts = []
        for b, seq_id in enumerate(seq_ids):
            req = GenerationRequest(
                prompt_ids=ids[b % n_src].tolist(), max_new_tokens=max_new,
                sampling=SamplingParams(greedy=True),
            )
            acts.append(_Active(req, seq_id, 0))
        self._prefill_no_admit(acts[:n_src])
        # replicas: the state prefill left in their source, KV in own blocks
        for j in range(n_src, batch):
            a, src = acts[j], acts[j % n_src]
            self.kv.extend_seq(a.seq_id, src.length)
            a.prefilled = a.length = src.length
            a.req.output_ids.append(src.req.output_ids[-1])
        for lo in range(n_src, batch, n_src):
            grp = acts[lo:lo + n_src]
            dst = self.kv.block_table([a.seq_id for a in grp]).flatten().long()
            src_blk = self.kv.block_table(
                [a.seq_id for a in acts[:len(grp)]]).flatten().long()
            for cache in self.kv.k_cache + self.kv.v_cache:
                cache[dst] = cache[src_blk]
        self._bench_acts = acts
        for a in acts:
            assert a.prefilled == prompt_len, "bench prompt truncated"
        return seq_ids

    @torch.no_grad()
    def _prefill_no_admit(self, acts: List[_Active]) -> None:
        """_prefill for the bench path, without touching the serving active
        set — looping until EVERY prompt is fully in the cache (_prefill
        consumes at most max_prefill_tokens per call, which also bounds the
        transient activation memory to ~max_prefill_tokens rows)."""
        saved_active = self._active
        saved_prefilling = self._prefilling
        self._active = []
        self._prefilling = []
        self._prefill(list(acts))
        while self._prefilling:
            self._prefill(list(self._prefilling))
        self._active = saved_active
        self._prefilling = saved_prefilling

    @torch.no_grad()
    def bench_setup(self, batch: int, prompt_len: int, steps_budget: int,
                    seed: int = 1234, distinct: Optional[int] = None) -> None:
        """Prefill a synthetic batch and preallocate KV for the whole run so
        the timed loop is pure device work (graph replay + sampling + buffer
        bumps; zero host round-trips per step). distinct: see bench_prefill."""
        assert batch <= self.max_batch
        seq_ids = self.bench_prefill(batch, prompt_len, seed=seed,
                                     distinct=distinct)
        for sid in seq_ids:
            self.kv.extend_seq(sid, prompt_len + steps_budget + 1)
        self._decode.load(seq_ids,
                          [a.req.output_ids[-1] for a in self._bench_acts],
                          [prompt_len] * batch)
        if self.graphs is not None:
            # capture outside the timed region (the run only reads the
            # decode inputs, and rewrites the same KV slot at prompt_len)
            self._decode.logits()
        self._bench_state = (
            "graph" if self.graphs is not None else "eager", batch)

    @property
    def _bench_eager(self) -> Dict[str, torch.Tensor]:
        """What the benchmark's output dump reads on the eager backend."""
        return {"ids": self._decode.ids}

    @torch.no_grad()
    def bench_step(self) -> None:
        """One fully device-side greedy decode step over the bench batch."""
        st = self._decode
        st.advance(torch.argmax(st.logits(), dim=-1), False)
        self.total_tokens += self._bench_state[1]
