"""Time ops.rope_kv_store against the two calls it replaces (rope_inplace,
then kv_cache_store) at a decode shape (default: Llama-3-8B, batch 1536,
256-token pages). Both leave the same bits in the qkv buffer and the caches.
The two are timed in alternating rounds, as graph replays between device
events. A graph's launches walk over `--buffers` qkv buffers and slot sets,
more bytes than the 256 MiB Infinity Cache holds, so a launch finds its
inputs in HBM as a decode step does, not in the cache where the previous
launch left them. Prints one JSON line.

    python scripts/bench_rope_kv_store.py [--tokens 1536] [--fp8] [--iters 192]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")

from bee2bee_amd import ops  # noqa: E402
from bee2bee_amd.ops import reference as R  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1536)
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--nkv", type=int, default=8)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--fp8", action="store_true",
                    help="fp8 cache with per-head scales, as the engine's")
    ap.add_argument("--buffers", type=int, default=16)
    ap.add_argument("--iters", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: timings are not taken on the CPU")
    ops.require_hip()
    dev = "cuda:0"
    T, nq, nkv, hd, bs = args.tokens, args.nq, args.nkv, args.hd, args.bs
    N = args.buffers
    torch.manual_seed(0)
    bufs = [torch.randn(T, (nq + 2 * nkv) * hd, device=dev).bfloat16()
            for _ in range(N)]
    cos, sin = R.rope_tables(4096, hd, 5e5, dev)
    pos = torch.randint(0, 4096, (T,), device=dev, dtype=torch.int32)
    # one page per token and buffer, written at a random offset: a decode
    # step's scatter, one row per sequence
    nb = N * T
    cdt = torch.uint8 if args.fp8 else torch.bfloat16
    kc = torch.zeros(nb, nkv, bs, hd, device=dev, dtype=cdt)
    vc = torch.zeros_like(kc)
    slots = [((torch.randperm(T, device=dev) + i * T) * bs
              + torch.randint(0, bs, (T,), device=dev)).to(torch.int32)
             for i in range(N)]
    kw = {}
    if args.fp8:
        kw = dict(k_inv_scale=torch.linspace(0.5, 2.0, nkv, device=dev),
                  v_inv_scale=torch.linspace(2.0, 0.5, nkv, device=dev))

    def views(i):
        q, k, v = bufs[i % N].split([nq * hd, nkv * hd, nkv * hd], dim=-1)
        return q.view(T, nq, hd), k.view(T, nkv, hd), v.view(T, nkv, hd)

    def fused(i):
        q, k, v = views(i)
        ops.rope_kv_store(q, k, v, pos, cos, sin, kc, vc, slots[i % N], **kw)

    def chain(i):
        q, k, v = views(i)
        ops.rope_inplace(q, k, pos, cos, sin)
        ops.kv_cache_store(k, v, kc, vc, slots[i % N], **kw)

    fns = {"rope_then_kv_store": chain, "rope_kv_store": fused}
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in fns.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up: code-object load
            for i in range(N):
                fn(i)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(args.iters):
                fn(i)
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, g in graphs.items():
            for b in bufs:
                b.normal_()
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            g.replay()
            end.record()
            torch.cuda.synchronize()
            times[name].append(start.elapsed_time(end) * 1e3 / args.iters)
    # one pass: q, k, v read; q, k written in place; K and V rows written
    csz = 1 if args.fp8 else 2
    floor_bytes = T * hd * ((nq + 2 * nkv) * 2 + (nq + nkv) * 2
                            + 2 * nkv * csz)
    out = {"shape": {"tokens": T, "nq": nq, "nkv": nkv, "hd": hd, "bs": bs,
                     "cache": "fp8s" if args.fp8 else "bf16"},
           "one_pass_bytes": floor_bytes,
           "one_pass_us_at_6.3TBps": round(floor_bytes / 6.3e6, 2),
           "buffers": N, "iters": args.iters, "rounds": args.rounds}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"us_median": round(med, 3), "us_min": round(min(ts), 3),
                     "us_max": round(max(ts), 3),
                     "one_pass_gbps_median": round(floor_bytes / med / 1e3, 1)}
    out["fused_slowest_beats_chain_fastest"] = (
        max(times["rope_kv_store"]) < min(times["rope_then_kv_store"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
