"""Time the fused QK-norm + RoPE kernel against plain RoPE at a decode
shape (default: qwen3-8b, batch 1536). Both run in place on the strided q/k
views of one fused qkv tensor and move the same bytes; the two are timed
in alternating rounds, as graph replays between device events. Prints one JSON line.

    python scripts/bench_qk_norm_rope.py [--tokens 1536] [--iters 200]
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: timings are not taken on the CPU")
    ops.require_hip()
    dev = "cuda:0"
    T, nq, nkv, hd = args.tokens, args.nq, args.nkv, args.hd
    torch.manual_seed(0)
    qkv = torch.randn(T, (nq + 2 * nkv) * hd, device=dev).bfloat16()
    q, k, _ = qkv.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
    q, k = q.view(T, nq, hd), k.view(T, nkv, hd)
    cos, sin = R.rope_tables(4096, hd, 1e6, dev)
    pos = torch.randint(0, 4096, (T,), device=dev, dtype=torch.int32)
    qw = (1 + 0.1 * torch.randn(hd, device=dev)).bfloat16()
    kw = (1 + 0.1 * torch.randn(hd, device=dev)).bfloat16()

    fns = {
        "rope_inplace": lambda: ops.rope_inplace(q, k, pos, cos, sin),
        "qk_norm_rope_inplace": lambda: ops.qk_norm_rope_inplace(
            q, k, pos, cos, sin, qw, kw, 1e-6),
    }
    # each op: `iters` launches captured into one graph, so the timed
    # window holds back-to-back kernels and not the host's enqueue rate
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in fns.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up: code-object load
            for _ in range(20):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.iters):
                fn()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, g in graphs.items():
            qkv.normal_()
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            g.replay()
            end.record()
            torch.cuda.synchronize()
            times[name].append(start.elapsed_time(end) * 1e3 / args.iters)
    # q and k read once and written once, bf16; tables and weights are small
    nbytes = T * (nq + nkv) * hd * 2 * 2
    out = {"shape": {"tokens": T, "nq": nq, "nkv": nkv, "hd": hd},
           "bytes": nbytes, "iters": args.iters, "rounds": args.rounds}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"us_median": round(med, 3), "us_min": round(min(ts), 3),
                     "us_max": round(max(ts), 3),
                     "gbps_median": round(nbytes / med / 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
