"""NativeEngineService — the MI355X HIP engine behind the mesh service
interface.

This is the row-for-row replacement of the reference's HFService
(bee2bee/services.py:27-116): same metadata/execute/execute_stream/load_sync
contract and JSON-lines streaming shape, but the compute is the in-process
InferenceEngine (CDNA4 kernels + hipGraph decode) instead of
transformers.generate(). Fixes reference quirk Q6: `tokens` counts NEW
tokens only (the reference re-encoded the full decoded text, prompt
included).
"""
from __future__ import annotations

import asyncio
import json
import os
import queue
import threading
import time
from typing import Any, AsyncIterator, Dict, Iterator, Optional

from .base import BaseService, ServiceError


class NativeEngineService(BaseService):
    def __init__(
        self,
        model_name: str,
        price_per_token: float = 0.0,
        max_new_tokens: int = 2048,
        model_path: Optional[str] = None,
        device: Optional[str] = None,
        max_batch: int = 16,
        max_seq_len: Optional[int] = None,
        wire_name: str = "hf",
    ) -> None:
        # wire_name defaults to "hf" so reference peers route to us unchanged
        super().__init__(wire_name)
        self.model_name = model_name
        self.price_per_token = price_per_token
        self.max_new_tokens = max_new_tokens
        self.model_path = model_path
        self.device = device
        self.max_batch = max_batch
        self.max_seq_len = max_seq_len
        self.engine = None

    def load_sync(self) -> None:
        try:
            from ..engine.engine import InferenceEngine

            kv_fp8 = os.environ.get("BEE2BEE_KV_FP8") == "1"
            # per-head fp8 KV scales: PATH | checkpoint | calibrate
            kv_scales = os.environ.get("BEE2BEE_KV_SCALES") or None
            if kv_scales and not kv_fp8:
                raise ValueError(
                    "BEE2BEE_KV_SCALES is set but the fp8 KV cache is off: "
                    "set BEE2BEE_KV_FP8=1 (--kv-fp8) as well")
            calibrate = kv_scales == "calibrate"
            # --max-seq-len / --sliding-window (0 forces the window off;
            # unset takes the checkpoint's / preset's value)
            msl = os.environ.get("BEE2BEE_MAX_SEQ_LEN")
            win = os.environ.get("BEE2BEE_SLIDING_WINDOW")
            self.engine = InferenceEngine(
                self.model_name,
                device=self.device,
                model_path=self.model_path,
                max_batch=self.max_batch,
                max_seq_len=int(msl) if msl else self.max_seq_len,
                sliding_window=int(win) if win else None,
                # speculative decoding (prompt-lookup + exact verification):
                # serving opt-in; greedy outputs are provably unchanged
                spec_decode=os.environ.get("BEE2BEE_SPEC_DECODE") == "1",
                # fp8 (OCP e4m3) KV pool: halves decode-attention bytes at a
                # small quantization cost; serving opt-in
                kv_dtype="fp8" if kv_fp8 else "native",
                kv_scales=None if calibrate else kv_scales,
                # fused batched sampler for every eligible request; off,
                # only requests that carry a seed take it
                fused_sampler=(
                    os.environ.get("BEE2BEE_FUSED_SAMPLER") == "1"),
            )
            if calibrate:
                from ..engine.engine import default_calibration_prompts

                self.engine.calibrate_kv_scales(
                    default_calibration_prompts(self.engine))
                out = os.environ.get("BEE2BEE_KV_SCALES_OUT")
                if out:
                    self.engine.save_kv_scales(out)
            self.engine.start()
        except Exception as e:
            raise ServiceError(f"failed to load model: {e}") from e

    def get_metadata(self) -> Dict[str, Any]:
        meta = {
            "models": [self.model_name],
            "price_per_token": self.price_per_token,
            "max_new_tokens": self.max_new_tokens,
            "backend": "bee2bee-amd-native",
        }
        if self.engine is not None:
            meta["arch"] = self.engine.spec.name
            meta["device"] = str(self.engine.device)
            meta["max_seq_len"] = self.engine.max_seq_len
            meta["sliding_window"] = self.engine.sliding_window
        return meta

    def _check(self, params: Dict[str, Any]):
        if self.engine is None:
            raise ServiceError("Model not loaded")
        # admission control: above this many queued requests, shed load with
        # a typed error instead of letting the queue (and every client's
        # latency) grow without bound
        max_queue = int(os.environ.get("BEE2BEE_MAX_QUEUE", "512"))
        if self.engine._pending.qsize() >= max_queue:
            raise ServiceError("server_overloaded")
        prompt = params.get("prompt")
        if not prompt:
            raise ServiceError("Missing prompt")
        max_new = int(params.get("max_new_tokens", self.max_new_tokens))
        max_new = max(1, min(max_new, self.max_new_tokens))
        temperature = float(params.get("temperature", 0.7))
        # None -> SamplingParams.from_request applies the reference's
        # generation defaults (top_p 0.95, repetition_penalty 1.15)
        rp = params.get("repetition_penalty")
        tp = params.get("top_p")
        tk = params.get("top_k")
        extra = {
            "stop": params.get("stop"),
            "repetition_penalty": None if rp is None else float(rp),
            "top_p": None if tp is None else float(tp),
            "top_k": None if tk is None else int(tk),
        }
        # an absent (or unusable) seed leaves the request unseeded
        from ..engine.sampler import sanitize_seed

        seed = sanitize_seed(params.get("seed"))
        if seed is not None:
            extra["seed"] = seed
        return prompt, max_new, temperature, extra

    def execute(self, params: Dict[str, Any]) -> Dict[str, Any]:
        prompt, max_new, temperature, extra = self._check(params)
        try:
            t0 = time.time()
            res = self.engine.generate_text(prompt, max_new, temperature, **extra)
            latency_ms = int((time.time() - t0) * 1000.0)
            tokens = res["tokens"]
            return {
                "text": res["text"],
                "tokens": tokens,
                "latency_ms": latency_ms,
                "ttft_ms": res.get("ttft_ms"),
                "timing": res.get("timing"),  # queue/prefill/decode stages
                "price_per_token": self.price_per_token,
                "cost": self.price_per_token * tokens,
                "backend": "bee2bee-amd-native",
            }
        except ServiceError:
            raise
        except Exception as e:
            raise ServiceError(str(e)) from e

    def execute_stream(self, params: Dict[str, Any]) -> Iterator[str]:
        prompt, max_new, temperature, extra = self._check(params)
        chunks: "queue.Queue" = queue.Queue()
        DONE = object()
        cancel = threading.Event()  # closing the generator stops the engine

        def _run() -> None:
            try:
                self.engine.generate_text(
                    prompt, max_new, temperature, on_text=chunks.put,
                    cancel=cancel, **extra
                )
                chunks.put(DONE)
            except Exception as e:  # noqa: BLE001
                chunks.put(e)

        t = threading.Thread(target=_run, daemon=True)
        t.start()
        try:
            while True:
                item = chunks.get()
                if item is DONE:
                    break
                if isinstance(item, Exception):
                    yield json.dumps(
                        {"status": "error", "message": f"Stream error: {item}"}
                    ) + "\n"
                    return
                yield json.dumps({"text": item}) + "\n"
            yield json.dumps({"done": True}) + "\n"
        finally:
            # GeneratorExit (consumer gone) or normal end: either way the
            # engine request must not keep burning decode steps
            cancel.set()

    async def execute_stream_async(
        self, params: Dict[str, Any]
    ) -> AsyncIterator[str]:
        """Zero-extra-threads streaming: the engine thread pushes tokens
        straight into an asyncio queue via call_soon_threadsafe. The HTTP
        gateway prefers this over the sync generator (which costs two
        threads per request — measurable GIL churn at high concurrency)."""
        from ..engine.engine import (GenerationRequest, StopStringFilter,
                                     TextStreamDecoder)
        from ..engine.sampler import SamplingParams

        prompt, max_new, temperature, extra = self._check(params)
        eng = self.engine
        ids = eng.tokenizer.encode(prompt)
        ids = ids[-(eng.max_seq_len - max_new - 1):]
        sp = SamplingParams.from_request(
            temperature, extra.get("top_p"), extra.get("top_k"),
            extra.get("repetition_penalty"), extra.get("seed"))
        stop_ids = ()
        eos = getattr(eng.tokenizer, "eos_token_id", None)
        if eos is not None:
            stop_ids = (eos,)
        req = GenerationRequest(
            prompt_ids=ids, max_new_tokens=max_new, sampling=sp,
            stop_token_ids=stop_ids,
        )
        loop = asyncio.get_running_loop()
        aq: asyncio.Queue = asyncio.Queue()
        decoder = TextStreamDecoder(eng.tokenizer)

        def on_emit(_tok, done) -> None:
            delta = decoder.delta(req.output_ids, final=done)
            if delta or done:
                loop.call_soon_threadsafe(aq.put_nowait, (delta, done))

        req.on_emit = on_emit
        eng.submit(req)
        # split stop strings across deltas are handled by the filter (the
        # streamed text equals the buffered truncation exactly)
        stop_filter = StopStringFilter(extra.get("stop"))
        try:
            while True:
                delta, done = await aq.get()
                out = stop_filter.feed(delta)
                if out:
                    yield json.dumps({"text": out}) + "\n"
                if stop_filter.done:
                    req.cancelled = True
                    break
                if done:
                    tail = stop_filter.flush()
                    if tail:
                        yield json.dumps({"text": tail}) + "\n"
                    break
            if req.error:
                yield json.dumps(
                    {"status": "error", "message": req.error}) + "\n"
                return
            yield json.dumps({"done": True}) + "\n"
        finally:
            # consumer disconnected (aclose/GeneratorExit) or finished:
            # make sure the engine request stops either way
            req.cancelled = True
