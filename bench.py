"""Flagship benchmark: Llama-3-8B bf16 greedy decode throughput (output
tokens/sec) on N MI355X GPUs, one engine/peer per GPU (replica mesh — weak
scaling, matching BASELINE.json's "Llama-3-8B across 1/2/4/8 peers").

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
launched via torch.distributed.run with one rank per GPU over RCCL. Does W
untimed warmup steps, times exactly K steps bracketed by barrier +
torch.cuda.synchronize() on both sides, takes the MAX elapsed over ranks,
and rank 0 prints ONE JSON line.

A step = one decode iteration of a fixed per-GPU batch (default 1536 seqs at
prompt length 1024): full layer stack on the HIP kernels via hipGraph
replay + greedy sampling + paged-KV append. Weights are random-init of the
real architecture; prompts synthetic (no network for checkpoints).

A plain run does only what the headline needs: set up, warm up, time the K
steps, print the line. Its set-up prefills `--distinct-prompts` prompts
(default 256) and copies their KV into blocks of their own for the rest of
the batch: prefilling all 1536 takes ~22 s and the decode step does not
care. `--full` prefills every prompt and adds the hipBLASLt tuning sweep
before the timed steps. `--dump-outputs DIR` writes the last timed step's outputs as
.npy; weights, prompts and (without --full) GEMM dispatch are fixed by the
arguments, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

# --dump-outputs keeps the logits file under this size by storing a fixed,
# seeded sample of vocabulary columns (all batch rows) when the full
# [batch, vocab] float32 array would be larger.
DUMP_LOGITS_MAX_BYTES = 48 << 20
DUMP_SAMPLE_SEED = 20240607


def dump_outputs(engine, out_dir: str, suffix: str = "") -> None:
    """Write what the last bench_step() left for its caller as float32
    .npy files: `next_ids` [batch] (the greedy tokens fed to the following
    step) and, on the captured-graph path, `logits` [batch, n_cols] (the
    static logits buffer of the last replay; n_cols == vocab when it fits,
    else sorted columns drawn once with DUMP_SAMPLE_SEED). The eager path
    does not keep its logits, so it writes `next_ids` only."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    mode, B = engine._bench_state
    if mode == "graph":
        g = engine.graphs
        next_ids = g.input_ids[:B]
        logits = g.logits[g.bucket_for(B)][:B]
        V = logits.shape[1]
        n_cols = min(V, DUMP_LOGITS_MAX_BYTES // (4 * B))
        if n_cols < V:
            cols = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(
                V, size=n_cols, replace=False))
            logits = logits[:, torch.from_numpy(cols).to(logits.device)]
        np.save(os.path.join(out_dir, f"logits{suffix}.npy"),
                logits.float().cpu().numpy())
    else:
        next_ids = engine._bench_eager["ids"]
    # token ids are < 2**24: exact in float32
    np.save(os.path.join(out_dir, f"next_ids{suffix}.npy"),
            next_ids.to(torch.float32).cpu().numpy())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=1536)
    ap.add_argument("--kv-dtype", default="native", choices=["native", "fp8"],
                    help="fp8 = OCP e4m3 KV cache (reported separately from "
                         "the bf16 headline; never the default)")
    ap.add_argument("--prompt-len", type=int, default=1024)
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--no-tunableop", action="store_true",
                    help="skip hipBLASLt algorithm tuning (only runs with --full)")
    ap.add_argument("--distinct-prompts", type=int, default=256,
                    help="prefill this many distinct prompts and give the "
                         "rest of the batch copies of their KV in blocks of "
                         "their own (a decode step reads the same bytes; "
                         "set-up is ~batch/N times shorter)")
    ap.add_argument("--full", action="store_true",
                    help="also do the work a plain run leaves out: prefill "
                         "every prompt of the batch, and run the hipBLASLt "
                         "algorithm tuning sweep during set-up and warmup "
                         "(tens of seconds; tuned choices can differ from "
                         "run to run)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step computed as DIR/<name>.npy (float32)")
    ap.add_argument("--preflight", action="store_true",
                    help="run the scale-run preflight checks (RCCL self-"
                         "test, master endpoint, env, rank wiring) and exit")
    args = ap.parse_args()

    if args.preflight:
        from bee2bee_amd.parallel.preflight import run_preflight

        tune_dir = os.path.join(
            os.path.dirname(os.path.abspath(__file__)), "gpurun_out")
        report = run_preflight(args.gpus, tune_dir)
        print(json.dumps(report), flush=True)
        sys.exit(0 if report["preflight"] == "ok" else 1)

    from bee2bee_amd.models.spec import resolve_spec

    _spec_probe = resolve_spec(args.model)
    # --full: tune hipBLASLt GEMM algorithm selection during (untimed)
    # setup/warmup. A plain run keeps the library's default dispatch: the
    # sweep takes longer than the rest of the run, and its picks are not
    # reproducible, which --dump-outputs comparisons need. Off on CPU and
    # for MoE (tuning the batched expert GEMM shapes takes minutes).
    if (args.full and not args.no_tunableop and torch.cuda.is_available()
            and not _spec_probe.is_moe):
        tune_dir = os.path.join(
            os.path.dirname(os.path.abspath(__file__)), "gpurun_out"
        )
        try:
            os.makedirs(tune_dir, exist_ok=True)
            os.environ.setdefault(
                "PYTORCH_TUNABLEOP_FILENAME",
                os.path.join(tune_dir, "tunableop_%d.csv"),
            )
            os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
            os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "1")
            # multi-GPU runs: TunableOp keys files by device ordinal, but
            # the tuned algorithms are shape-keyed and identical across the
            # node's MI355Xs — seed ranks 1..7 from rank 0's table so the
            # scale run's warmup replays instead of re-tuning per GPU
            base = os.path.join(tune_dir, "tunableop_0.csv")
            if os.path.exists(base):
                import shutil

                for d in range(1, 8):
                    dst = os.path.join(tune_dir, f"tunableop_{d}.csv")
                    if not os.path.exists(dst):
                        try:
                            shutil.copyfile(base, dst)
                        except OSError:
                            pass
        except OSError:
            pass  # read-only checkout: run untuned

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = world_size if world_size > 1 else args.gpus

    on_gpu = torch.cuda.is_available()
    dist = None
    if world_size > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(
            backend="nccl" if on_gpu else "gloo",
            rank=rank,
            world_size=world_size,
        )
    if on_gpu:
        torch.cuda.set_device(local_rank)
        device = f"cuda:{local_rank}"
    else:
        device = "cpu"

    from bee2bee_amd.engine.engine import InferenceEngine

    budget = args.warmup + args.steps + 4
    # models with short contexts (gpt2 family: 1024) can't hold the default
    # 1024-token prompt plus the step budget — clamp instead of asserting
    max_prompt = _spec_probe.max_seq_len - budget - 2
    if args.prompt_len > max_prompt:
        print(f"# prompt-len {args.prompt_len} > {_spec_probe.name} context "
              f"budget; clamping to {max_prompt}", file=sys.stderr)
        args.prompt_len = max_prompt
    engine = InferenceEngine(
        args.model,
        device=device,
        max_batch=args.batch,
        max_seq_len=args.prompt_len + budget + 1,
        use_graphs=(not args.no_graphs) and on_gpu,
        seed=1234 + rank,
        kv_dtype=args.kv_dtype,
    )
    spec = engine.spec

    distinct = args.batch if args.full else max(
        1, min(args.distinct_prompts, args.batch))
    engine.bench_setup(args.batch, args.prompt_len, budget, distinct=distinct)

    def sync() -> None:
        if on_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        engine.bench_step()
    sync()

    if dist:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        engine.bench_step()
    sync()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if on_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs:
        # one set per rank (replica peers differ in their weights' seed)
        dump_outputs(engine, args.dump_outputs,
                     suffix=f"_rank{rank}" if world_size > 1 else "")

    ms_per_step = elapsed / args.steps * 1000.0
    total_tps = args.batch * args.steps * n_gpus / elapsed

    if rank == 0:
        result = {
            "metric": f"output tokens/sec ({spec.name} bf16 greedy decode, "
                      "replica peers)",
            "value": round(total_tps, 1),
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": ("bf16+fp8kv" if args.kv_dtype == "fp8" else "bf16") if on_gpu else "fp32-cpu-fallback",
            "data": "synthetic",
            "config": {
                "model": spec.name,
                "global_batch": args.batch * n_gpus,
                "seq_len": args.prompt_len,
                "parallelism": f"replica-dp{n_gpus}",
                "decode_graphs": bool(engine.graphs is not None),
                "distinct_prompts": distinct,
            },
        }
        print(json.dumps(result), flush=True)

    engine.shutdown()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
