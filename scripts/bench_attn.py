"""Microbenchmark for the paged decode-attention kernel.

Usage: python scripts/bench_attn.py [--batch 64] [--len 1024] [--iters 50]
Prints achieved KV-read bandwidth (the kernel is memory-bound; the roofline
is ~6.3 TB/s achievable HBM on MI355X). With --window N (sliding-window
attention) the bandwidth is taken over the bytes the window leaves to read:
min(L, N) keys per sequence for decode.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--len", type=int, dest="seqlen", default=1024)
    ap.add_argument("--nkv", type=int, default=8)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--prefill", action="store_true",
                    help="bench the MFMA prefill kernel instead")
    ap.add_argument("--fp8", action="store_true",
                    help="fp8 (e4m3) KV cache variant of the decode bench")
    ap.add_argument("--fp8-scaled", action="store_true",
                    help="the --fp8 bench with non-unit per-kv-head scales "
                         "passed (scaled scores / PV kernels)")
    ap.add_argument("--window", type=int, default=0,
                    help="sliding-window attention over the last N keys "
                         "(0 = off), decode and --prefill")
    ap.add_argument("--path", choices=("auto", "split", "fused"),
                    default="auto",
                    help="decode kernels: the launcher's choice, the split "
                         "scores / PV kernels, or the fused kernel")
    args = ap.parse_args()
    wkw = {"window": args.window} if args.window > 0 else {}
    if args.fp8_scaled:
        args.fp8 = True

    from bee2bee_amd import ops

    dev = "cuda:0"
    torch.manual_seed(0)
    B, L, nkv, G, hd, bs = (
        args.batch, args.seqlen, args.nkv, args.group, args.hd, args.bs
    )
    nq = nkv * G

    if args.prefill:
        T = B * L
        q = torch.randn(T, nq, hd, device=dev).bfloat16()
        k = torch.randn(T, nkv, hd, device=dev).bfloat16()
        v = torch.randn(T, nkv, hd, device=dev).bfloat16()
        cu = torch.arange(0, T + 1, L, dtype=torch.int32, device=dev)
        scale = hd**-0.5
        for _ in range(3):
            out = ops.attn_prefill(q, k, v, cu, L, scale, True, **wkw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            out = ops.attn_prefill(q, k, v, cu, L, scale, True, **wkw)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.iters
        # causal flops: 4 * nq * hd per live (q, key) pair (QK^T + PV);
        # pairs = L^2/2, minus the (L - w)^2/2 a window w < L masks
        pairs = L * L / 2
        if 0 < args.window < L:
            pairs -= (L - args.window) ** 2 / 2
        flops = 4 * nq * hd * pairs * B
        wtag = f" w{args.window}" if args.window > 0 else ""
        print(f"prefill B{B} L{L} nq{nq} hd{hd}{wtag}: {dt * 1e3:.3f} ms  "
              f"{flops / dt / 1e12:.1f} TF/s")
        return

    W = (L + bs - 1) // bs
    nb = B * W + 1
    bt = torch.arange(1, B * W + 1, dtype=torch.int32).reshape(B, W).to(dev)
    if args.fp8:
        kc = torch.randint(0, 127, (nb, nkv, bs, hd), dtype=torch.uint8,
                           device=dev)
        vc = torch.randint(0, 127, (nb, nkv, bs, hd), dtype=torch.uint8,
                           device=dev)
    else:
        kc = torch.randn(nb, nkv, bs, hd, device=dev).bfloat16()
        vc = torch.randn(nb, nkv, bs, hd, device=dev).bfloat16()
    q = torch.randn(B, nq, hd, device=dev).bfloat16()
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    scale = hd**-0.5
    kw = {}
    if args.fp8_scaled:
        kw = {
            "k_scale": torch.linspace(0.02, 0.08, nkv, device=dev),
            "v_scale": torch.linspace(0.5, 2.0, nkv, device=dev),
        }

    kw.update(wkw)
    decode = ops.attn_decode
    if args.path != "auto":
        def decode(*a, **k):
            return ops.attn_decode_select(*a, path=args.path, **k)[0]
    for _ in range(5):
        out = decode(q, kc, vc, bt, lens, scale, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        out = decode(q, kc, vc, bt, lens, scale, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.iters
    live = min(L, args.window) if args.window > 0 else L  # keys read
    kv_bytes = B * live * 2 * nkv * hd * (1 if args.fp8 else 2)
    print(
        f"decode{' fp8' if args.fp8 else ''}"
        f"{'-scaled' if args.fp8_scaled else ''} "
        f"B{B} L{L} nkv{nkv} G{G} hd{hd}"
        f"{f' w{args.window}' if args.window > 0 else ''}"
        f"{f' path={args.path}' if args.path != 'auto' else ''}: "
        f"{dt * 1e6:.1f} us  "
        f"KV {kv_bytes / 1e6:.0f} MB  {kv_bytes / dt / 1e12:.2f} TB/s"
    )
    _ = out


_PROBE_ARGS = (["probe"], ["--probe"], ["paged"], ["--paged"])

if __name__ == "__main__" and sys.argv[1:2] not in _PROBE_ARGS:
    main()


def _time_probe(fn, n=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def probe():
    """Bandwidth ceiling of the decode kernels' two read patterns, with
    plain and with non-temporal (nt) loads side by side, on a 1 GiB pool
    (four times the Infinity Cache), head_dim 128:
    python scripts/bench_attn.py --probe
      row per lane:  a lane reads one key's 256-byte row in 16-byte pieces
                     (the K pattern), rows in order and through a shuffled
                     table of 64 KB pages (256 rows, a KV page at bs 256);
      row per instr: a wave reads one row per instruction, 4 bytes per lane
                     (the V pattern)."""
    from bee2bee_amd import ops

    hip = ops.require_hip()
    dev = "cuda:0"
    hd = 128
    pool = torch.randn(1 << 29, device=dev).bfloat16()  # 1 GiB
    nbytes = pool.numel() * 2
    lin = _time_probe(lambda: hip.bw_probe(pool, 0, hd, 0))
    print(f"{'linear dwordx4':34s} {nbytes / lin / 1e12:6.2f} TB/s")
    n_pages = pool.numel() // hd // 256
    table = torch.randperm(n_pages, device=dev).to(torch.int32)
    rows = (
        ("row-per-lane 16 B (serial)", lambda nt: hip.bw_probe(
            pool, 1 + 4 * nt, hd, 0)),
        ("row-per-lane 16 B (batch8)", lambda nt: hip.bw_probe(
            pool, 1 + 4 * nt, hd, 1)),
        ("row-per-lane 16 B, 64 KB pages", lambda nt: hip.bw_probe_paged(
            pool, table, hd, 256, nt)),
        ("row-per-instr 4 B rpw256", lambda nt: hip.bw_probe(
            pool, 2 + 4 * nt, hd, 256)),
        ("row-per-instr 4 B rpw1024", lambda nt: hip.bw_probe(
            pool, 2 + 4 * nt, hd, 1024)),
    )
    print(f"{'':34s} {'plain':>11s} {'nt':>11s}")
    for _round in range(3):  # alternating, three rounds
        for name, fn in rows:
            plain = _time_probe(lambda: fn(0))
            nt = _time_probe(lambda: fn(1))
            print(f"{name:34s} {nbytes / plain / 1e12:6.2f} TB/s "
                  f"{nbytes / nt / 1e12:6.2f} TB/s")


if __name__ == "__main__" and sys.argv[1:2] in (["probe"], ["--probe"]):
    probe()
    sys.exit(0)


def probe_paged():
    from bee2bee_amd import ops

    hip = ops.require_hip()
    dev = "cuda:0"
    hd = 128
    pool = torch.randn(1 << 29, device=dev).bfloat16()
    nbytes = pool.numel() * 2
    for rpp in (256, 64, 32, 16):
        n_pages = pool.numel() // hd // rpp
        for name, perm in (("seq", False), ("perm", True)):
            table = (
                torch.randperm(n_pages, device=dev)
                if perm else torch.arange(n_pages, device=dev)
            ).to(torch.int32)
            dts = [_time_probe(
                lambda: hip.bw_probe_paged(pool, table, hd, rpp, nt))
                for nt in (0, 1)]
            print(f"paged rows/page={rpp:4d} {name:5s}"
                  f" ({rpp * hd * 2 // 1024:3d} KB contig) "
                  f"{nbytes / dts[0] / 1e12:6.2f} TB/s plain "
                  f"{nbytes / dts[1] / 1e12:6.2f} TB/s nt")


if __name__ == "__main__" and sys.argv[1:2] in (["paged"], ["--paged"]):
    probe_paged()
    sys.exit(0)
