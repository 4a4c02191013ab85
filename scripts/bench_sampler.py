"""Time one sampling step: the engine's grouped torch path (one sample()
per distinct parameter set, as InferenceEngine._sample_grouped runs it)
against the fused kernel (ops.sample_rows, one launch), on bf16 logits.

Shapes [256, 128256], [1536, 128256], [768, 152064]; a uniform parameter
mix (T 0.7, k 64, p 0.95, penalty 1.15) and a 4-way mix. The two paths are
timed in alternating rounds between device events, each round ending in a
synchronise (the torch path's host copies are part of what it costs).
Prints one JSON line per (shape, mix): ms per step and logits bytes per
second, bytes = B * V * 2.

    python scripts/bench_sampler.py [--iters 200] [--rounds 5]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")

from bee2bee_amd import ops  # noqa: E402
from bee2bee_amd.engine.engine import _penalize  # noqa: E402
from bee2bee_amd.engine.sampler import SamplingParams, sample  # noqa: E402

SHAPES = [(256, 128256), (1536, 128256), (768, 152064)]
UNIFORM = [SamplingParams(0.7, 0.95, 64, 1.15)]
MIXED = [
    SamplingParams(0.7, 0.95, 64, 1.15),
    SamplingParams(1.0, 0.9, 256, 1.0),
    SamplingParams(1.0, 1.0, 1, 1.15, greedy=True),
    SamplingParams(1.2, 1.0, 8, 1.3),
]


def torch_step(logits, sets, pool, gen):
    """InferenceEngine._sample_grouped over rows whose parameters go round
    `sets`; every row has its own seen-pool slot (slot = row)."""
    B = logits.shape[0]
    dev = logits.device
    single = len(sets) == 1
    out = None if single else torch.empty(B, dtype=torch.int64, device=dev)
    for g, sp in enumerate(sets):
        if single:
            idx, grp = None, logits
            slots = torch.arange(B, device=dev)
        else:
            rows = list(range(g, B, len(sets)))
            idx = torch.tensor(rows, dtype=torch.int64, device=dev)
            grp = logits[idx]
            slots = torch.tensor(rows, dtype=torch.int64, device=dev)
        if sp.repetition_penalty != 1.0:
            grp = _penalize(grp.float(), pool[slots], sp.repetition_penalty)
        toks = sample(grp, sp, generator=gen)
        if single:
            out = toks
        else:
            out[idx] = toks
    return out


def kernel_args(logits, sets, pool):
    B = logits.shape[0]
    dev = logits.device
    rows = [sets[r % len(sets)].fused_row() for r in range(B)]
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    pen = [r[3] for r in rows]
    return (logits, torch.tensor([r[0] for r in rows], **f32),
            torch.tensor([r[1] for r in rows], **i32),
            torch.tensor([r[2] for r in rows], **f32),
            torch.tensor(pen, **f32), pool,
            torch.tensor([r if pen[r] != 1.0 else -1 for r in range(B)],
                         **i32),
            torch.arange(B, dtype=torch.int64, device=dev),
            torch.zeros(B, **i32))


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: timings are not taken on the CPU")
    ops.require_hip()
    dev = "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    for B, V in SHAPES:
        torch.manual_seed(B + V)
        logits = (torch.randn(B, V, device=dev) * 3.0).bfloat16()
        pool = torch.rand(B, V, device=dev) < 0.002   # ~300 seen tokens a row
        for mix, sets in (("uniform", UNIFORM), ("mixed4", MIXED)):
            kargs = kernel_args(logits, sets, pool)
            fns = {
                "torch": lambda: torch_step(logits, sets, pool, gen),
                "kernel": lambda: ops.sample_rows(*kargs),
            }
            for fn in fns.values():        # warm-up: code objects, allocator
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in fns}
            for _ in range(args.rounds):
                for name, fn in fns.items():
                    kargs[8].add_(1)       # a new draw per round
                    times[name].append(timed(fn, args.iters))
            nbytes = B * V * 2
            out = {"shape": [B, V], "mix": mix, "logits_bytes": nbytes,
                   "iters": args.iters, "rounds": args.rounds}
            for name, ts in times.items():
                med = statistics.median(ts)
                out[name] = {"ms_median": round(med, 4),
                             "ms_min": round(min(ts), 4),
                             "ms_max": round(max(ts), 4),
                             "logits_gbps_median": round(nbytes / med / 1e6,
                                                         1)}
            out["speedup_median"] = round(
                out["torch"]["ms_median"] / out["kernel"]["ms_median"], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
