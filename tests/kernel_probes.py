"""Probe inputs for the kernel tests: cases where ONE key, row or element
carries a large share of the answer, a checker at the suite's existing
tolerances, and mutants (wrong references in plain torch) that prove the
cases can tell right from wrong.

With randn K/V an attention output is an average over hundreds of keys, of
the same order as the absolute tolerance: dropping one key moves it by
O(1/L). Here the query heads of a kv group are `base + 0.5 * noise` and the
key at a probe position is `c * base`, so that key takes most of the softmax
weight and an edge error costs O(1). The row reductions get one element of
magnitude sqrt(H), half the row's energy; the grouped GEMM gets one-hot
rows, whose output is a column of W bit for bit.

tests/test_kernel_probes.py (CPU) runs every case through a reference that
emulates the kernels' rounding, which must pass the checker, and through
every applicable mutant, which must fail it. tests/test_kernel_probes_gpu.py
runs the same cases through the HIP kernels.

Plain helper module: imports torch and bee2bee_amd.ops.reference only.
"""
import functools
import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from bee2bee_amd.ops import reference as R

NKV = 2
EPS = 1e-5
MIN_PROBE_WEIGHT = 0.25
LOUD_V = 8.0          # V rows of probe keys that some query must not see
# score of a probe key under an unscaled q at head_dim 128 with c = 1
TARGET_SCORE = math.sqrt(128.0)

# the suite's existing tolerances (tests/test_ops_gpu.py and friends)
TOL_DECODE = 2e-2      # bf16 decode
TOL_ELEMENTWISE = 2e-2
TOL_PREFILL = 3e-2
TOL_FP8 = 3e-2
TOL_GEMM = 3e-2


# ------------------------------------------------------------------ checker

def assert_close(a, b, atol=2e-2, rtol=2e-2, msg=""):
    """tests/test_attn_decode_fused_gpu.py's assert_close, finiteness
    checks included."""
    a = a.float().cpu()
    b = b.float().cpu()
    assert bool(torch.isfinite(b).all()), f"{msg}: reference is not finite"
    assert bool(torch.isfinite(a).all()), f"{msg}: non-finite output"
    diff = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = diff > tol
    assert not bool(bad.any()), (
        f"{msg}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; "
        f"max diff {float(diff.max()):.4f}"
    )


def assert_ml_close(ml, r_ml, msg=""):
    """The (m, l) bounds of test_ops_gpu.py::test_attn_decode_lse_merge."""
    ml = ml.float().cpu()
    r_ml = r_ml.float().cpu()
    assert bool(torch.isfinite(ml).all()), msg
    assert torch.allclose(ml[..., 0], r_ml[..., 0], atol=0.25, rtol=0.02), \
        (msg, (ml[..., 0] - r_ml[..., 0]).abs().max())
    assert torch.allclose(ml[..., 1] / r_ml[..., 1].clamp_min(1e-6),
                          torch.ones_like(r_ml[..., 1]), atol=0.1), \
        f"{msg}: sum-exp mismatch"


# ---------------------------------------------------------- attention cases

@dataclass
class Seq:
    """One sequence: L keys, the last QL of them are the query rows; `see`
    are probe keys some row must see, `hide` probe keys no row may see."""
    L: int
    QL: int
    see: Tuple[int, ...] = ()
    hide: Tuple[int, ...] = ()


@dataclass
class AttnCase:
    name: str
    kind: str                 # "decode" | "prefill" | "paged"
    seqs: List[Seq]
    G: int
    hd: int
    bs: int
    cache: str                # "bf16" | "fp8" | "fp8s" (per-head scales)
    window: int
    causal: bool
    q: torch.Tensor           # [T, nq, hd] bf16 (decode: T = B)
    k: Optional[torch.Tensor] = None   # packed prefill: [T, NKV, hd] bf16
    v: Optional[torch.Tensor] = None
    kc: Optional[torch.Tensor] = None  # [nb, NKV, bs, hd] bf16 | uint8
    vc: Optional[torch.Tensor] = None
    bt: Optional[torch.Tensor] = None  # [B, W] int32
    k_scale: Optional[torch.Tensor] = None
    v_scale: Optional[torch.Tensor] = None
    weights: list = field(default_factory=list)  # (seq, key, min weight)

    @property
    def nq(self):
        return NKV * self.G

    @property
    def scale(self):
        return self.hd ** -0.5

    @property
    def tol(self):
        if self.cache != "bf16":
            return TOL_FP8
        return TOL_DECODE if self.kind == "decode" else TOL_PREFILL

    @property
    def cu(self):
        out = [0]
        for s in self.seqs:
            out.append(out[-1] + s.QL)
        return out

    @property
    def lens(self):
        return [s.L for s in self.seqs]

    def rows(self, i):
        cu = self.cu
        return slice(cu[i], cu[i + 1])

    def scale_kw(self):
        if self.k_scale is None:
            return {}
        return {"k_scale": self.k_scale, "v_scale": self.v_scale}

    def kw(self):
        kw = self.scale_kw()
        if self.window:
            kw["window"] = self.window
        return kw


def visible(case, i, nk):
    """bool [QL, nk]: may query row r of sequence i see key j."""
    s = case.seqs[i]
    qpos = (s.L - s.QL + torch.arange(s.QL)).view(-1, 1)
    kpos = torch.arange(nk).view(1, -1)
    vis = (kpos < s.L).expand(s.QL, nk).clone()
    if case.causal:
        vis &= kpos <= qpos
    if case.window:
        vis &= kpos > qpos - case.window
    return vis


def _seq_kv(case, i, bt_shift=False):
    """fp32 keys, values [NKV, nk, hd] of sequence i as stored (no scale)."""
    if case.kind == "prefill":
        r = case.rows(i)
        return (case.k[r].float().permute(1, 0, 2),
                case.v[r].float().permute(1, 0, 2))
    cols = case.bt[i].long()
    if bt_shift:  # column j read from column j + 1
        cols = torch.roll(cols, -1)
    nk = cols.numel() * case.bs
    keys = R._kv_deq(case.kc[cols]).permute(1, 0, 2, 3).reshape(NKV, nk, -1)
    vals = R._kv_deq(case.vc[cols]).permute(1, 0, 2, 3).reshape(NKV, nk, -1)
    return keys, vals


def _e4m3_staged_q(qs, G, lift):
    """The fp8 MFMA decode kernels quantize the staged q [QL, nq, hd] to
    e4m3. With per-head scales, a kv head's [G, hd] block whose amax is
    below 2^-5 is first lifted by a power of two to amax in [128, 256),
    and the power is divided back out of the scores."""
    QL, nq, hd = qs.shape
    blk = qs.view(QL, nq // G, G * hd)
    mul = torch.ones(QL, nq // G, 1)
    if lift:
        amax = blk.abs().amax(-1, keepdim=True)
        _m, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1)
        small = (amax < 2.0 ** -5) & (amax > 0)
        mul = torch.where(small, torch.exp2(8.0 - ex.float()), mul)
    return ((blk * mul).to(torch.float8_e4m3fn).float() / mul).view_as(qs)


def attn_model(case, seqs=None, *, emulate=False, vis_edit=None,
               gqa_mod=False, bt_shift=False, swap_scales=False,
               want_probs=False):
    """Dense attention over `seqs` (default: all) of a case, the operation
    ops/reference.py defines, with the hooks the mutants need.

    emulate: the kernels' roundings. q * scale is rounded to the MFMA input
    type (e4m3 for fp8 decode, bf16 otherwise), p = exp(s - m) is stored as
    bf16 before PV (l sums the unrounded p), the output is stored as bf16.
    vis_edit(i, vis) -> vis edits the visibility mask; gqa_mod maps query
    head h to kv head h % NKV instead of h // G; bt_shift reads block-table
    column j + 1 for page j; swap_scales exchanges k_scale and v_scale.
    Rows with no visible key give zeros, as in the kernels.

    Returns (out [T, nq, hd] fp32, ml [T, nq, 2] fp32), zeros outside
    `seqs`; with want_probs a list of per-sequence [nq, QL, nk] weights.
    """
    nq, G = case.nq, case.G
    T = case.cu[-1]
    out = torch.zeros(T, nq, case.hd)
    ml = torch.zeros(T, nq, 2)
    probs = []
    hmap = torch.arange(nq) % NKV if gqa_mod else torch.arange(nq) // G
    ks, vs = case.k_scale, case.v_scale
    if swap_scales:
        ks, vs = vs, ks
    for i in (range(len(case.seqs)) if seqs is None else seqs):
        keys, vals = _seq_kv(case, i, bt_shift)
        nk = keys.shape[1]
        qs = case.q[case.rows(i)].float() * case.scale
        if emulate:
            qs = qs.bfloat16().float()
            if (case.cache != "bf16" and case.kind == "decode"
                    and case.hd in (64, 128)):
                qs = _e4m3_staged_q(qs, G, lift=case.cache == "fp8s")
        s = torch.einsum("qhd,hkd->hqk", qs, keys[hmap])
        if ks is not None:
            s = s * ks[hmap].view(-1, 1, 1)
        vis = visible(case, i, nk)
        if vis_edit is not None:
            vis = vis_edit(i, vis)
        s = s.masked_fill(~vis.unsqueeze(0), float("-inf"))
        m = s.amax(-1).clamp_min(-1e30)
        p = torch.exp(s - m.unsqueeze(-1))
        l = p.sum(-1)
        if want_probs:
            probs.append(p / l.unsqueeze(-1))
        if emulate:
            p = p.bfloat16().float()
        o = torch.einsum("hqk,hkd->hqd", p, vals[hmap])
        o = torch.where(l.unsqueeze(-1) > 0, o / l.unsqueeze(-1),
                        torch.zeros_like(o))
        if vs is not None:
            o = o * vs[hmap].view(-1, 1, 1)
        if emulate:
            o = o.bfloat16().float()
        out[case.rows(i)] = o.permute(1, 0, 2)
        ml[case.rows(i), :, 0] = m.t()
        ml[case.rows(i), :, 1] = l.t()
    if want_probs:
        return probs
    return out, ml


def attn_exact(case):
    """(out, ml) of ops/reference.py at fp32 on the case as stored (ml is
    None for the prefill kinds). Computed once per case."""
    if not hasattr(case, "_exact"):
        q = case.q.float()
        lens = torch.tensor(case.lens, dtype=torch.int32)
        if case.kind == "decode":
            case._exact = R.attn_decode_lse(q, case.kc, case.vc, case.bt,
                                            lens, case.scale, **case.kw())
        elif case.kind == "prefill":
            cu = torch.tensor(case.cu, dtype=torch.int32)
            ref = R.attn_prefill(q, case.k.float(), case.v.float(), cu,
                                 max(case.lens), case.scale, case.causal,
                                 window=case.window)
            case._exact = (ref, None)
        else:
            qlens = torch.tensor([s.QL for s in case.seqs],
                                 dtype=torch.int32)
            ref = R.attn_decode_with_history(q, case.kc, case.vc, case.bt,
                                             lens, qlens, case.scale,
                                             **case.kw())
            case._exact = (ref, None)
    return case._exact


def check_attn(case, out, ml=None, seqs=None, msg=""):
    """The checker: `out` (and decode's `ml`) against ops/reference.py at
    the case's existing tolerance, over `seqs` (default: all)."""
    r_out, r_ml = attn_exact(case)
    msg = f"{case.name} {msg}"
    for i in (range(len(case.seqs)) if seqs is None else seqs):
        r = case.rows(i)
        assert_close(out[r], r_out[r], atol=case.tol, rtol=case.tol,
                     msg=f"{msg} seq {i}")
        if case.kind == "decode":
            assert ml is not None
            assert_ml_close(ml[r], r_ml[r], msg=f"{msg} seq {i} (m, l)")


def _probe_c(hd, q_scale):
    """Probe key = c * base: c = 1 at head_dim 128 with an unscaled q,
    larger where sqrt(hd) or the q scale shrink the score."""
    return max(1.0, TARGET_SCORE / (q_scale * math.sqrt(hd)))


def build_attn(name, kind, seqs, *, G, hd, bs=32, cache="bf16", window=0,
               causal=True, seed=0):
    """One batch, one sequence per probe position, every sequence on its
    own pages behind a permuted block table whose page 0 is unused."""
    g = torch.Generator().manual_seed(seed)
    nq = NKV * G
    fp8 = cache != "bf16"
    if not fp8:
        q_scale, kv_scale = 1.0, 1.0
    elif kind == "decode":   # test_fp8_kv_attn_decode
        q_scale, kv_scale = 0.2, 0.7
    else:                    # test_fp8_kv_attn_prefill_paged
        q_scale, kv_scale = 0.4, 0.6
    c = _probe_c(hd, q_scale)
    base = torch.randn(NKV, hd, generator=g)
    base *= math.sqrt(hd) / base.norm(dim=-1, keepdim=True)
    assert float((c * base).abs().max()) < R.E4M3_MAX
    T = sum(s.QL for s in seqs)
    q = base.view(1, NKV, 1, hd) + 0.5 * torch.randn(T, NKV, G, hd,
                                                     generator=g)
    q = (q * q_scale).reshape(T, nq, hd)
    case = AttnCase(name, kind, list(seqs), G, hd, bs, cache, window, causal,
                    q=None)
    B = len(seqs)
    W = max(s.L // bs + 1 for s in seqs)  # a row for key L in every sequence
    Ks, Vs = [], []
    for i, s in enumerate(seqs):
        nk = s.L if kind == "prefill" else W * bs
        K = torch.randn(nk, NKV, hd, generator=g) * kv_scale
        V = torch.randn(nk, NKV, hd, generator=g) * kv_scale
        vis = visible(case, i, nk)
        for p in tuple(s.see) + tuple(s.hide):
            assert 0 <= p < nk, (name, i, p)
            K[p] = c * base
            if not bool(vis[:, p].all()):
                V[p] = LOUD_V * kv_scale * torch.randn(NKV, hd, generator=g)
        for p in s.see:
            assert bool(vis[:, p].any()), (name, i, p, "no row sees it")
        for p in s.hide:
            assert not bool(vis[:, p].any()), (name, i, p, "a row sees it")
        Ks.append(K)
        Vs.append(V)
    if cache == "fp8s":
        # kv head 0: K runs large and its q small (the fused test's case)
        for K in Ks:
            K[:, 0] *= 40.0 / 0.7
        q[:, :G] /= 40.0
    case.q = q.bfloat16()
    if kind == "prefill":
        case.k = torch.cat(Ks).bfloat16()
        case.v = torch.cat(Vs).bfloat16()
    else:
        nb = 1 + B * W
        bt = (torch.randperm(B * W, generator=g) + 1).reshape(B, W)
        ksrc = torch.randn(nb, NKV, bs, hd, generator=g) * kv_scale
        vsrc = torch.randn(nb, NKV, bs, hd, generator=g) * kv_scale
        for i in range(B):
            ksrc[bt[i]] = Ks[i].view(W, bs, NKV, hd).permute(0, 2, 1, 3)
            vsrc[bt[i]] = Vs[i].view(W, bs, NKV, hd).permute(0, 2, 1, 3)
        case.bt = bt.to(torch.int32)
        if not fp8:
            case.kc, case.vc = ksrc.bfloat16(), vsrc.bfloat16()
        else:
            kf = ksrc.permute(0, 2, 1, 3).reshape(nb * bs, NKV, hd)
            vf = vsrc.permute(0, 2, 1, 3).reshape(nb * bs, NKV, hd)
            skw = {}
            if cache == "fp8s":
                case.k_scale = kf.abs().amax(dim=(0, 2)) / R.E4M3_MAX
                case.v_scale = vf.abs().amax(dim=(0, 2)) / R.E4M3_MAX
                skw = {"k_inv_scale": 1.0 / case.k_scale,
                       "v_inv_scale": 1.0 / case.v_scale}
            case.kc = torch.zeros(nb, NKV, bs, hd, dtype=torch.uint8)
            case.vc = torch.zeros_like(case.kc)
            R.kv_cache_store(kf.bfloat16(), vf.bfloat16(), case.kc, case.vc,
                             torch.arange(nb * bs, dtype=torch.int32), **skw)
    # a condition on the inputs: every row that may see a must-see probe
    # gives it at least MIN_PROBE_WEIGHT, on the cache as actually stored
    probs = attn_model(case, want_probs=True)
    for i, s in enumerate(seqs):
        vis = visible(case, i, probs[i].shape[-1])
        for p in s.see:
            w = float(probs[i][:, vis[:, p], p].min())
            assert w >= MIN_PROBE_WEIGHT, (
                f"{name}: seq {i} probe key {p} has softmax weight {w:.3f}")
            case.weights.append((i, p, w))
    return case


# decode: the positions the issue lists, one sequence each

def decode_seqs(bs, window=0):
    if window:
        # lo = L - w mid-chunk, on a 256-key chunk edge, on a page edge that
        # is no chunk edge; and L <= w (lo = 0, nothing below the band)
        out = []
        for lo in (444 if window == 256 else 400, 512, 288):
            L = lo + window
            out.append(Seq(L, 1, see=(lo,), hide=(lo - 1, L)))
        out.append(Seq(window, 1, see=(0,), hide=(window,)))
        out.append(Seq(window - 44, 1, see=(window - 45,),
                       hide=(window - 44,)))
        return out
    if bs == 256:
        L = 1025
        return [Seq(L, 1, see=(p,), hide=(L,))
                for p in (0, 255, 256, 1023, 1024)]
    out = [Seq(600, 1, see=(p,), hide=(600,))
           for p in (0, 31, 32, 63, 64, 255, 256, 511, 512, 599)]
    out += [Seq(L, 1, see=(L - 1,), hide=(L,)) for L in (1, 256, 257)]
    return out


PREFILL_L = 200
PREFILL_PROBES = (0, 15, 16, 63, 64, 65, 127, 128)
PAGED_HIST = 100
PAGED_CHUNK = 100


def prefill_seqs(window=0):
    # with a window every probe p needs rows p + w - 1 and p + w: L > p + w
    L = PREFILL_L if not window else max(PREFILL_PROBES) + window + 2
    return [Seq(L, L, see=(p,)) for p in PREFILL_PROBES + (L - 1,)]


def paged_seqs(window=0):
    L = PAGED_HIST + PAGED_CHUNK
    keys = (PAGED_HIST - 1, PAGED_HIST, PAGED_HIST + 1) + PREFILL_PROBES + \
        (L - 1,)
    out = []
    for p in keys:
        # with a window, a key at or below hist - w is below every row's band
        if window and p <= PAGED_HIST - window:
            out.append(Seq(L, PAGED_CHUNK, hide=(p,)))
        else:
            out.append(Seq(L, PAGED_CHUNK, see=(p,)))
    return out


@functools.lru_cache(maxsize=None)
def decode_case(G=4, hd=128, bs=32, cache="bf16", window=0):
    name = f"decode G{G} hd{hd} bs{bs} {cache} w{window}"
    return build_attn(name, "decode", decode_seqs(bs, window), G=G, hd=hd,
                      bs=bs, cache=cache, window=window, seed=G + hd + window)


@functools.lru_cache(maxsize=None)
def prefill_case(G=4, hd=128, window=0, causal=True):
    name = f"prefill G{G} hd{hd} w{window} causal={causal}"
    seqs = prefill_seqs(window)
    return build_attn(name, "prefill", seqs, G=G, hd=hd, window=window,
                      causal=causal, seed=1 + G + hd + window)


@functools.lru_cache(maxsize=None)
def paged_case(G=4, hd=128, cache="bf16", window=0):
    name = f"paged G{G} hd{hd} {cache} w{window}"
    return build_attn(name, "paged", paged_seqs(window), G=G, hd=hd,
                      cache=cache, window=window, seed=2 + G + hd + window)


# the configurations both test files run: builder + keyword arguments
DECODE_CONFIGS = [
    dict(G=4, hd=128), dict(G=4, hd=64),
    dict(G=1, hd=128), dict(G=7, hd=128), dict(G=16, hd=128),
    dict(G=4, hd=128, bs=256),
    dict(G=4, hd=128, cache="fp8"), dict(G=4, hd=64, cache="fp8"),
    dict(G=7, hd=128, cache="fp8"),
    dict(G=4, hd=128, cache="fp8s"), dict(G=4, hd=64, cache="fp8s"),
    dict(G=16, hd=128, cache="fp8s"),
    dict(G=4, hd=128, window=256), dict(G=4, hd=128, window=300),
    dict(G=4, hd=64, window=300),
    dict(G=4, hd=128, cache="fp8", window=256),
    dict(G=4, hd=128, cache="fp8s", window=300),
]
DECODE_GENERIC_CONFIGS = [
    dict(G=2, hd=16), dict(G=4, hd=96),
    dict(G=2, hd=16, window=256), dict(G=4, hd=96, window=300),
    dict(G=4, hd=96, cache="fp8"), dict(G=2, hd=16, cache="fp8s"),
]
# prefill windows: 64 is the kernels' key tile, 100 is no multiple of it
PREFILL_CONFIGS = [
    dict(G=4, hd=128), dict(G=4, hd=64), dict(G=2, hd=16), dict(G=4, hd=96),
    dict(G=4, hd=128, window=64), dict(G=4, hd=128, window=100),
    dict(G=4, hd=64, window=100), dict(G=2, hd=16, window=64),
    dict(G=4, hd=96, window=100),
    dict(G=4, hd=128, causal=False),
]
PAGED_CONFIGS = [
    dict(G=4, hd=hd, cache=cache, window=w)
    for hd in (128, 64, 16)
    for cache in ("bf16", "fp8", "fp8s")
    for w in (0, 100)
]


def attn_mutants(case):
    """[(mutant name, sequence or None, attn_model keyword arguments)]:
    every wrong reference that applies to the case. A mutant of one probe
    changes one sequence and must be caught there."""
    out = []

    def edit(i, r, j, value):
        def f(k, vis):
            if k == i:
                vis = vis.clone()
                vis[r, j] = value
            return vis
        return f

    for i, s in enumerate(case.seqs):
        nk = s.L if case.kind == "prefill" else case.bt.shape[1] * case.bs
        vis = visible(case, i, nk)
        hist = s.L - s.QL
        for p in s.see:
            out.append((f"drop key {p}", i,
                        dict(vis_edit=edit(i, slice(None), p, False))))
            if not case.causal:
                continue
            r = p - 1 - hist  # the row just above the causal edge
            if 0 <= r < s.QL and not bool(vis[r, p]):
                out.append((f"causal: row {r} sees key {p}", i,
                            dict(vis_edit=edit(i, r, p, True))))
            r = p + case.window - hist  # first row whose band is past p
            if case.window and 0 <= r < s.QL:
                out.append((f"window: row {r} sees key {p}", i,
                            dict(vis_edit=edit(i, r, p, True))))
        for p in s.hide:
            out.append((f"include key {p}", i,
                        dict(vis_edit=edit(i, slice(None), p, True))))
    # bugs of the whole launch: run over the batch (sequence None). A
    # shifted table, say, leaves a sequence whose rows all see the probe
    # nearly unchanged; the sequences with an edge at the probe catch it.
    if case.G > 1:
        out.append(("GQA h % nkv", None, dict(gqa_mod=True)))
    if case.kind != "prefill":
        out.append(("block table + 1", None, dict(bt_shift=True)))
    if case.cache == "fp8s":
        out.append(("k/v scales swapped", None, dict(swap_scales=True)))
    return out


# ----------------------------------------------------- row-reduction spikes

NORM_H = (8, 64, 2056, 4096, 14336)
NORM_OPS = ("rmsnorm", "fused_add_rmsnorm", "layernorm", "fused_add_layernorm")
QKN_HD = (64, 128, 256)


def spike_positions(H, cand=None):
    if cand is None:
        cand = (0, 7, 8, 2047, 2048, H - 8, H - 1)
    return sorted({s for s in cand if 0 <= s < H})


@dataclass
class NormCase:
    name: str
    op: str
    H: int
    spikes: List[int]              # spike index of row t
    x: torch.Tensor                # [T, H] bf16
    resid: Optional[torch.Tensor]  # fused-add only
    w: torch.Tensor
    b: Optional[torch.Tensor]


@functools.lru_cache(maxsize=None)
def norm_case(op, H, spike_in="x"):
    """One row per spike index s: randn plus one element of magnitude
    sqrt(H) at s, about half the row's energy. The layernorm rows sit on a
    unit offset, so that the mean matters. Fused add: x and resid are randn
    / sqrt(2) each and the spike goes into `spike_in`."""
    g = torch.Generator().manual_seed(H + len(op))
    spikes = spike_positions(H)
    T = len(spikes)
    fused = op.startswith("fused")
    parts = {"x": torch.randn(T, H, generator=g)}
    if fused:
        parts["x"] /= math.sqrt(2.0)
        parts["resid"] = torch.randn(T, H, generator=g) / math.sqrt(2.0)
    if "layernorm" in op:
        parts["x"] += 1.0
    for t, s in enumerate(spikes):
        parts[spike_in][t, s] = math.sqrt(H) * (1 if t % 2 else -1)
    w = (1.0 + 0.5 * torch.randn(H, generator=g)).bfloat16()
    b = torch.randn(H, generator=g).bfloat16() if "layernorm" in op else None
    return NormCase(f"{op} H{H} spike in {spike_in}", op, H, spikes,
                    parts["x"].bfloat16(),
                    parts["resid"].bfloat16() if fused else None, w, b)


def norm_configs():
    out = []
    for op in NORM_OPS:
        for H in NORM_H:
            out.append((op, H, "x"))
            if op.startswith("fused"):
                out.append((op, H, "resid"))
    return out


def _reduce_masks(spikes, H, mutant):
    keep = torch.ones(len(spikes), H)
    if mutant == "omit 8 at spike":
        for t, s in enumerate(spikes):
            keep[t, s // 8 * 8: s // 8 * 8 + 8] = 0
    denom = float(H - 8) if mutant == "divide by H-8" else float(H)
    return keep, denom


def norm_model(case, mutant=None, emulate=False):
    """The norm at fp32 (emulate: output rounded to bf16), or a mutant of
    its row reduction. Returns y, or (y, new_residual) for the fused ops."""
    v = case.x.float()
    if case.resid is not None:
        v = v + case.resid.float()
    keep, denom = _reduce_masks(case.spikes, case.H, mutant)
    msq = (v * v * keep).sum(-1, keepdim=True) / denom
    if "rmsnorm" in case.op:
        y = v * torch.rsqrt(msq + EPS) * case.w.float()
    else:
        mean = (v * keep).sum(-1, keepdim=True) / denom
        if mutant == "no mean":
            mean = torch.zeros_like(mean)
        y = (v - mean) * torch.rsqrt(msq - mean * mean + EPS)
        y = y * case.w.float() + case.b.float()
    if emulate:
        y, v = y.bfloat16().float(), v.bfloat16().float()
    return (y, v) if case.resid is not None else y


def norm_exact(case):
    """ops/reference.py at fp32 (nothing rounded)."""
    x, w = case.x.float(), case.w.float()
    if case.op == "rmsnorm":
        return R.rmsnorm(x, w, EPS)
    if case.op == "fused_add_rmsnorm":
        return R.fused_add_rmsnorm(x, case.resid.float(), w, EPS)
    if case.op == "layernorm":
        return R.layernorm(x, w, case.b.float(), EPS)
    return R.fused_add_layernorm(x, case.resid.float(), w, case.b.float(),
                                 EPS)


def check_norm(case, got, msg=""):
    ref = norm_exact(case)
    if case.resid is None:
        got, ref = (got,), (ref,)
    for a, b, what in zip(got, ref, ("y", "residual")):
        assert_close(a, b, atol=TOL_ELEMENTWISE, rtol=TOL_ELEMENTWISE,
                     msg=f"{case.name} {msg} {what}")


def divide_mutant_applies(H):
    """Dividing by H - 8 scales every output by sqrt(H / (H - 8)): a purely
    relative error, which the existing rtol can resolve only where it is
    larger than rtol (H = 8 divides by zero)."""
    return H == 8 or math.sqrt(H / (H - 8.0)) - 1.0 > TOL_ELEMENTWISE


def norm_mutants(case):
    out = ["omit 8 at spike"]
    if divide_mutant_applies(case.H):
        out.append("divide by H-8")
    if "layernorm" in case.op:
        out.append("no mean")
    return out


@dataclass
class QKNormCase:
    name: str
    hd: int
    spikes: List[int]
    q: torch.Tensor    # [T, 4, hd] bf16
    k: torch.Tensor    # [T, 2, hd] bf16
    pos: torch.Tensor  # [T] int32
    cos: torch.Tensor
    sin: torch.Tensor
    qw: torch.Tensor
    kw: torch.Tensor


@functools.lru_cache(maxsize=None)
def qk_norm_case(hd):
    """One token per spike index: every q and k head of token t is randn
    with one element of magnitude sqrt(hd) at spikes[t]."""
    g = torch.Generator().manual_seed(hd)
    spikes = spike_positions(hd, (0, 63, 64, hd // 2 - 1, hd // 2, hd - 1))
    T = len(spikes)
    q = torch.randn(T, 4, hd, generator=g)
    k = torch.randn(T, 2, hd, generator=g)
    for t, s in enumerate(spikes):
        q[t, :, s] = math.sqrt(hd) * (1 if t % 2 else -1)
        k[t, :, s] = -math.sqrt(hd) * (1 if t % 2 else -1)
    cos, sin = R.rope_tables(64, hd, 10000.0, "cpu")
    pos = torch.randint(0, 64, (T,), generator=g).to(torch.int32)
    qw = (1.0 + 0.5 * torch.randn(hd, generator=g)).bfloat16()
    kw = (1.0 + 0.5 * torch.randn(hd, generator=g)).bfloat16()
    return QKNormCase(f"qk_norm_rope hd{hd}", hd, spikes, q.bfloat16(),
                      k.bfloat16(), pos, cos, sin, qw, kw)


def qk_norm_model(case, mutant=None, emulate=False):
    """(q, k) after per-head RMSNorm + RoPE at fp32, or a mutant of the
    per-head reduction."""
    hd = case.hd
    keep, denom = _reduce_masks(case.spikes, hd, mutant)
    c = case.cos[case.pos.long()].unsqueeze(1)
    s = case.sin[case.pos.long()].unsqueeze(1)
    outs = []
    for t, w in ((case.q, case.qw), (case.k, case.kw)):
        x = t.float()
        msq = (x * x * keep.unsqueeze(1)).sum(-1, keepdim=True) / denom
        x = x * torch.rsqrt(msq + EPS) * w.float()
        x1, x2 = x[..., : hd // 2], x[..., hd // 2:]
        y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
        outs.append(y.bfloat16().float() if emulate else y)
    return tuple(outs)


def qk_norm_exact(case):
    q, k = case.q.float(), case.k.float()
    R.qk_norm_rope_inplace(q, k, case.pos, case.cos, case.sin, case.qw,
                           case.kw, EPS)
    return q, k


def check_qk_norm(case, got, msg=""):
    for a, b, what in zip(got, qk_norm_exact(case), ("q", "k")):
        assert_close(a, b, atol=TOL_ELEMENTWISE, rtol=TOL_ELEMENTWISE,
                     msg=f"{case.name} {msg} {what}")


def qk_norm_mutants(case):
    out = ["omit 8 at spike"]
    if divide_mutant_applies(case.hd):
        out.append("divide by H-8")
    return out


# ------------------------------------------------------------- grouped GEMM

GEMM_KG = 64  # the kernel's K-group
GEMM_ONEHOT_K = (128, 256, 384, 512)
GEMM_SEGMENTS = (1, 16, 17, 127, 128, 129, 257)


@dataclass
class GemmCase:
    name: str
    x: torch.Tensor       # [S, K] bf16
    w: torch.Tensor       # [E, N, K] bf16
    offs: torch.Tensor    # [E + 1] int32
    hot: Optional[List[int]] = None  # one-hot cases: the k of row r


def onehot_positions(K):
    """The K positions of the issue, and the first and last element of every
    K-group, so that each group holds a probe."""
    ks = {0, 31, 32, 63, 64, 127, 128, K - 1}
    for g0 in range(0, K, GEMM_KG):
        ks |= {g0, g0 + GEMM_KG - 1}
    return sorted(k for k in ks if 0 <= k < K)


@functools.lru_cache(maxsize=None)
def gemm_onehot_case(K, E=3, N=128):
    """Every expert gets one one-hot row per probed k: out row == w[e, :, k]
    bit for bit iff each K position is consumed exactly once."""
    g = torch.Generator().manual_seed(K)
    ks = onehot_positions(K)
    hot = ks * E
    x = torch.zeros(len(hot), K)
    x[torch.arange(len(hot)), torch.tensor(hot)] = 1.0
    w = torch.randn(E, N, K, generator=g).bfloat16()
    assert bool((w != 0).all())
    offs = torch.arange(E + 1, dtype=torch.int32) * len(ks)
    return GemmCase(f"grouped_gemm one-hot K{K}", x.bfloat16(), w, offs, hot)


def gemm_onehot_expect(case):
    E = case.w.shape[0]
    n = len(case.hot) // E
    return torch.stack([case.w[r // n, :, k] for r, k in enumerate(case.hot)])


@functools.lru_cache(maxsize=None)
def gemm_segment_case(K=384, N=128):
    """Ragged segments with empty experts between them (and at both ends),
    randn inputs scaled as in test_grouped_gemm."""
    g = torch.Generator().manual_seed(11)
    counts = [0]
    for n in GEMM_SEGMENTS:
        counts += [n, 0]
    S = sum(counts)
    offs = torch.zeros(len(counts) + 1, dtype=torch.int32)
    offs[1:] = torch.tensor(counts).cumsum(0).to(torch.int32)
    x = (torch.randn(S, K, generator=g) * 0.3).bfloat16()
    w = (torch.randn(len(counts), N, K, generator=g) * 0.05).bfloat16()
    return GemmCase(f"grouped_gemm segments K{K}", x, w, offs)


def gemm_model(case, mutant=None, group=0, emulate=False):
    """Per-expert segment GEMM summed K-group by K-group at fp32.
    mutant "skip group" / "group twice" act on K-group `group`; "segment
    edge + 1" moves every inner segment boundary up by one row."""
    S, K = case.x.shape
    E, N, _ = case.w.shape
    offs = case.offs.long().clone()
    if mutant == "segment edge + 1":
        offs[1:-1] = (offs[1:-1] + 1).clamp_max(S)
    out = torch.zeros(S, N)
    for e in range(E):
        lo, hi = int(offs[e]), int(offs[e + 1])
        if hi <= lo:
            continue
        for g0 in range(0, K, GEMM_KG):
            coef = 1.0
            if g0 // GEMM_KG == group:
                coef = {"skip group": 0.0, "group twice": 2.0}.get(mutant, 1.0)
            out[lo:hi] += coef * (case.x[lo:hi, g0:g0 + GEMM_KG].float()
                                  @ case.w[e, :, g0:g0 + GEMM_KG].float().t())
    return out.bfloat16() if emulate else out


def gemm_mutants(case):
    ng = case.x.shape[1] // GEMM_KG
    out = [(m, g) for m in ("skip group", "group twice") for g in range(ng)]
    return out + [("segment edge + 1", 0)]


def check_gemm(case, got, msg=""):
    if case.hot is not None:
        expect = gemm_onehot_expect(case)
        assert torch.equal(got.cpu(), expect), (
            f"{case.name} {msg}: "
            f"{int((got.cpu() != expect).any(-1).sum())} rows differ from "
            f"their column of w")
        return
    ref = R.grouped_gemm(case.x.float(), case.w.float(), case.offs)
    assert_close(got, ref, atol=TOL_GEMM, rtol=TOL_GEMM,
                 msg=f"{case.name} {msg}")
