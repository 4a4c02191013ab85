"""Probe inputs for the KV write path: RoPE in place on the fused qkv buffer,
the paged store, and the fp8 (OCP e4m3) quantizer inside the store.

The readers of the cache are covered by tests/kernel_probes.py. The writers
are checked bit for bit here, because a write that lands one slot, one head
or one rounding step off still yields plausible attention outputs:

  * an e4m3 encoder in plain torch, written from the format's definition
    and independent of torch's fp8 cast, small enough to run on all 65 536
    bf16 patterns;
  * a plain-torch model of the scatter on sentinel-filled caches, compared
    over the WHOLE cache, so a stray write shows as well as a missing one;
  * a RoPE checker with a derived bound (half a bf16 ulp for the store plus
    the fp32 error of two products and a sum), and a check that everything
    outside the q and k views keeps its bits;
  * a model of the two calls chained as the runner chains them;
  * mutants (wrong models in plain torch) that prove each checker can tell
    right from wrong.

tests/test_write_path.py (CPU) runs the references through the checkers,
which must pass, and every mutant, which must fail.
tests/test_write_path_gpu.py runs the same cases through the HIP kernels.

Plain helper module: imports torch and bee2bee_amd.ops.reference only.
"""
import functools
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

from bee2bee_amd.ops import reference as R

E4M3_MAX = 448.0
# halfway between 448 and the 480 that code 0x7f would hold if it were a
# number: round-to-nearest sends (448, 464] to 448 and anything above to NaN
E4M3_OVERFLOW = 464.0
E4M3_NAN = 0x7F
SENTINEL16 = 0x5A5A
SENTINEL8 = 0x5A
# per-head reciprocal scales of the scaled store; every test uses these
INV_SCALES = (1.0, 8.0, 1 / 0.37, 300.0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _random_bits(shape, g):
    """Uniform 16-bit patterns as bf16: NaNs, infs and subnormals included."""
    raw = torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32)
    return raw.to(torch.int16).view(torch.bfloat16)


def bits(x):
    """The tensor's storage as integers: bf16 -> int16, fp8 bytes as is."""
    x = x.detach().cpu()
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16)
    assert x.dtype in (torch.int16, torch.uint8), x.dtype
    return x


# ------------------------------------------------------------ e4m3 encoder

@functools.lru_cache(maxsize=None)
def e4m3_values():
    """The 127 finite non-negative e4m3 values by code, in float64: code =
    eeee mmm, subnormal m * 2^-9 for e == 0, else (1 + m/8) * 2^(e - 7)."""
    code = torch.arange(127, dtype=torch.float64)
    e = torch.floor(code / 8)
    m = code - 8 * e
    return torch.where(e == 0, m * 2.0 ** -9,
                       (1 + m / 8) * torch.pow(2.0, e - 7))


def e4m3_encode(y, ties="even", flush_subnormals=False):
    """float tensor -> e4m3 bytes (uint8): the nearest finite code in
    float64, ties to the even code, sign bit carried over from the input;
    |y| > 464 and NaN give 0x7f, (448, 464] gives 0x7e.

    `ties` ("even" | "away" | "truncate") and `flush_subnormals` cut the
    mutants; the encoder proper is the default."""
    y = y.detach().cpu()
    a = y.double().abs()
    vals = e4m3_values()
    finite = a <= E4M3_OVERFLOW            # false for NaN and inf
    af = torch.where(finite, a, torch.zeros_like(a)).clamp(max=E4M3_MAX)
    hi = torch.searchsorted(vals, af).clamp(max=126)  # vals[hi] >= af
    lo = (hi - 1).clamp(min=0)
    if ties == "truncate":
        code = torch.where(af >= vals[hi], hi, lo)
    else:
        mid = (vals[lo] + vals[hi]) / 2    # exact: at most 5 significant bits
        tie = hi if ties == "away" else torch.where(lo % 2 == 0, lo, hi)
        code = torch.where(af > mid, hi, torch.where(af < mid, lo, tie))
    if flush_subnormals:
        code = torch.where(code < 8, torch.zeros_like(code), code)
    code = torch.where(finite, code, torch.full_like(code, E4M3_NAN))
    code = code + 128 * torch.signbit(y).long()
    return code.to(torch.uint8)


def quant_unscaled(x, **enc):
    """The unscaled store's bytes for bf16 x: the encoder, overflow to NaN."""
    return e4m3_encode(x.float(), **enc)


def quant_scaled(x, inv_scale, clamp="select", **enc):
    """The scaled store's bytes for x [T, n_kv, hd] and inv_scale [n_kv]:
    fp32 product, clamp to +-448 with NaN passing through, encoder.
    clamp="none" and clamp="minmax" (fminf / fmaxf semantics: a NaN operand
    is dropped, so NaN becomes -448) cut the mutants."""
    y = x.float() * inv_scale.float().view(1, -1, 1)
    if clamp == "minmax":
        y = torch.where(torch.isnan(y), torch.full_like(y, -E4M3_MAX), y)
    if clamp != "none":
        hi = torch.full_like(y, E4M3_MAX)
        y = torch.where(y > E4M3_MAX, hi, torch.where(y < -E4M3_MAX, -hi, y))
    return e4m3_encode(y, **enc)


def canon_bytes(b):
    """NaN bytes ((b & 0x7f) == 0x7f) all become 0x7f: the sign of a NaN
    byte is not compared."""
    b = b.detach().cpu()
    assert b.dtype == torch.uint8
    return torch.where((b & 0x7F) == 0x7F, torch.full_like(b, E4M3_NAN), b)


def assert_same_bits(got, want, msg=""):
    """Whole-tensor equality of storage; fp8 NaN bytes by NaN-ness."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, \
        f"{msg}: {tuple(g.shape)} {g.dtype} vs {tuple(w.shape)} {w.dtype}"
    if g.dtype == torch.uint8:
        g, w = canon_bytes(g), canon_bytes(w)
    bad = g != w
    if bool(bad.any()):
        at = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(
            f"{msg}: {int(bad.sum())}/{bad.numel()} elements differ; first "
            f"at {at}: got {int(g[at]) & 0xffff:#x}, want "
            f"{int(w[at]) & 0xffff:#x}")


@functools.lru_cache(maxsize=None)
def all_bf16():
    """Every bf16 pattern; pattern p at index p."""
    p = torch.arange(65536, dtype=torch.int32)
    return torch.where(p >= 32768, p - 65536, p).to(torch.int16).view(
        torch.bfloat16)


# ------------------------------------------------------------- the scatter

def _conv(cache_kind, inv_scale=None, **enc):
    """bf16 rows [T, n_kv, hd] -> rows in the cache's storage type."""
    if cache_kind == "bf16":
        return lambda x: bits(x)
    if cache_kind == "fp8":
        return lambda x: quant_unscaled(x, **enc)
    return lambda x: quant_scaled(x, inv_scale, **enc)


def sentinel_cache(nb, nkv, bs, hd, cache_kind, fill=None):
    """One cache as the ops take it (bf16 | uint8), every element holding
    the sentinel pattern (or `fill`)."""
    if cache_kind == "bf16":
        fill = SENTINEL16 if fill is None else fill
        return torch.full((nb, nkv, bs, hd), fill,
                          dtype=torch.int16).view(torch.bfloat16)
    fill = SENTINEL8 if fill is None else fill
    return torch.full((nb, nkv, bs, hd), fill, dtype=torch.uint8)


def scatter_model(k, v, kc, vc, slots, conv_k, conv_v, mutant=None):
    """The paged store on storage bits: kc / vc [nb, n_kv, bs, hd] (int16 or
    uint8) are written in place, row t of k / v to flat slot slots[t] =
    block * bs + offset. `mutant` names one of scatter_mutants()."""
    nb, nkv, bs, hd = kc.shape
    T = k.shape[0]
    if mutant == "v token stride taken from k":
        v = torch.as_strided(v, v.shape, (k.stride(0), hd, 1),
                             v.storage_offset())
    kr, vr = conv_k(k), conv_v(v)
    if mutant == "V written into the K cache":
        kr = vr
    if mutant == "d >= 128 not written":
        kr, vr = kr[..., :128], vr[..., :128]
    if mutant == "last token dropped":
        T -= 1
    width = kr.shape[-1]
    for t in range(T):
        s = int(slots[t])
        if mutant == "slot + 1":
            s = (s + 1) % (nb * bs)
        blk, off = divmod(s, bs)
        if mutant == "off = slot % (bs - 1)":
            off = s % (bs - 1)
        if mutant == "cache indexed [nb, bs, n_kv, hd]":
            kc.view(nb, bs, nkv, hd)[blk, off, :, :width] = kr[t]
            vc.view(nb, bs, nkv, hd)[blk, off, :, :width] = vr[t]
        else:
            kc[blk, :, off, :width] = kr[t]
            vc[blk, :, off, :width] = vr[t]
    if mutant == "zeros written to an untouched slot":
        used = set(int(s) for s in slots)
        blk, off = divmod(min(set(range(nb * bs)) - used), bs)
        kc[blk, :, off] = 0
    return kc, vc


SCATTER_SHAPES = [  # (T, n_kv, hd, bs, nb)
    (1, 1, 16, 16, 2),
    (7, 3, 96, 32, 3),     # 21 waves: partial workgroup, partial-lane trip
    (50, 8, 128, 32, 12),
    (9, 2, 256, 256, 2),   # second trip of the lane loop, 256-token pages
    (5, 1, 64, 16, 4),     # one kv head, as a TP shard has
]
SCATTER_LAYOUTS = ("fused", "separate")
CACHE_KINDS = ("bf16", "fp8", "fp8s")
SCATTER_CONFIGS = [
    dict(T=T, nkv=nkv, hd=hd, bs=bs, nb=nb, layout=layout, kind=kind)
    for (T, nkv, hd, bs, nb) in SCATTER_SHAPES
    for layout in SCATTER_LAYOUTS for kind in CACHE_KINDS]
PAD_K, PAD_V = 8, 24  # "separate": sk = n_kv*hd + 8, sv = n_kv*hd + 24


@dataclass
class ScatterCase:
    name: str
    T: int
    nkv: int
    hd: int
    bs: int
    nb: int
    layout: str               # "fused": k, v views of one qkv buffer
    kind: str                 # "bf16" | "fp8" | "fp8s" (per-head scales)
    bufs: Tuple[torch.Tensor, ...]   # the 2-D bf16 buffers behind k and v
    slots: torch.Tensor       # [T] int32, distinct
    k_inv: Optional[torch.Tensor] = None   # [n_kv] fp32, kind "fp8s"
    v_inv: Optional[torch.Tensor] = None

    def views(self, bufs):
        """(k, v) [T, n_kv, hd] as views of the given buffers (these, or
        copies of them on another device)."""
        T, n, hd = self.T, self.nkv, self.hd
        if self.layout == "fused":
            nq = 2 * n
            (buf,) = bufs
            return (buf[:, nq * hd:(nq + n) * hd].view(T, n, hd),
                    buf[:, (nq + n) * hd:(nq + 2 * n) * hd].view(T, n, hd))
        kb, vb = bufs
        return kb[:, :n * hd].view(T, n, hd), vb[:, :n * hd].view(T, n, hd)

    def scale_kw(self):
        if self.kind != "fp8s":
            return {}
        return dict(k_inv_scale=self.k_inv, v_inv_scale=self.v_inv)

    def caches(self, fill=None):
        """Fresh (k_cache, v_cache) as the ops take them."""
        return tuple(sentinel_cache(self.nb, self.nkv, self.bs, self.hd,
                                    self.kind, fill) for _ in range(2))

    def expected(self, mutant=None, fill=None):
        """Storage bits of both caches after the store."""
        k, v = self.views(self.bufs)
        kc, vc = (bits(c).clone() for c in self.caches(fill))
        return scatter_model(k, v, kc, vc, self.slots,
                             _conv(self.kind, self.k_inv),
                             _conv(self.kind, self.v_inv), mutant)


def probe_slots(T, bs, nb, g):
    """T distinct slots holding, as far as T allows and in this order of
    preference: the last slot of the pool, slot 0, a page's last offset and
    the following page's first. The rest are random; the order is shuffled."""
    must = [nb * bs - 1, 0, bs - 1, bs][:T]
    rest = [s for s in torch.randperm(nb * bs, generator=g).tolist()
            if s not in must][:T - len(must)]
    picked = must + rest
    order = torch.randperm(T, generator=g).tolist()
    return torch.tensor([picked[i] for i in order], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def scatter_case(T, nkv, hd, bs, nb, layout, kind):
    g = _gen(1000 * T + hd + bs + len(layout) + len(kind))
    if layout == "fused":
        shapes = [(T, 4 * nkv * hd)]
    else:
        shapes = [(T, nkv * hd + PAD_K), (T, nkv * hd + PAD_V)]
    if kind == "fp8s":   # finite inputs at randn scale; heads scaled apart
        bufs = tuple((torch.randn(s, generator=g) * 2).bfloat16()
                     for s in shapes)
        inv = torch.tensor([INV_SCALES[h % 4] for h in range(nkv)])
        k_inv, v_inv = inv, torch.tensor(
            [INV_SCALES[(h + 1) % 4] for h in range(nkv)])
    else:                # a bit copy / the full input domain of the cast
        bufs = tuple(_random_bits(s, g) for s in shapes)
        k_inv = v_inv = None
    case = ScatterCase(
        name=f"scatter T{T} kv{nkv} hd{hd} bs{bs} {layout} {kind}",
        T=T, nkv=nkv, hd=hd, bs=bs, nb=nb, layout=layout, kind=kind,
        bufs=bufs, slots=probe_slots(T, bs, nb, g), k_inv=k_inv, v_inv=v_inv)
    if layout == "separate" and T > 1:   # sk != sv, neither is n_kv * hd
        k, v = case.views(bufs)
        assert len({k.stride(0), v.stride(0), nkv * hd}) == 3
    return case


def scatter_mutants(case):
    """The mutants that change what this case's store writes."""
    out = ["slot + 1", "off = slot % (bs - 1)", "V written into the K cache",
           "last token dropped", "zeros written to an untouched slot"]
    if case.nkv > 1:
        out.append("cache indexed [nb, bs, n_kv, hd]")
    if case.layout == "separate" and case.T > 1:
        out.append("v token stride taken from k")
    if case.hd > 128:
        out.append("d >= 128 not written")
    return out


def check_scatter(case, kc, vc, msg=""):
    """Both whole caches against the model."""
    want_k, want_v = case.expected()
    assert_same_bits(kc, want_k, f"{case.name} {msg}: K cache")
    assert_same_bits(vc, want_v, f"{case.name} {msg}: V cache")


# The exhaustive quantizer case: every kv head sees all 65 536 bf16 patterns
# in one launch; the heads start at different (odd) offsets, so each pattern
# meets both lanes of the packed convert.
QUANT_T, QUANT_NKV, QUANT_HD, QUANT_BS, QUANT_NB = 512, 4, 128, 32, 16
QUANT_HEAD_OFFSETS = (0, 16411, 32821, 49157)


@functools.lru_cache(maxsize=None)
def quant_case(scaled):
    T, n, hd = QUANT_T, QUANT_NKV, QUANT_HD
    assert T * hd == 65536 and QUANT_NB * QUANT_BS == T
    idx = (torch.arange(65536).view(T, 1, hd)
           + torch.tensor(QUANT_HEAD_OFFSETS).view(1, n, 1)) % 65536
    k = bits(all_bf16())[idx].view(torch.bfloat16)        # [T, n, hd]
    v = k.roll(1, dims=0)                                 # K/V mix-ups show
    kb = torch.zeros(T, n * hd + PAD_K, dtype=torch.bfloat16)
    vb = torch.zeros(T, n * hd + PAD_V, dtype=torch.bfloat16)
    kb[:, :n * hd] = k.reshape(T, n * hd)
    vb[:, :n * hd] = v.reshape(T, n * hd)
    inv = torch.tensor(INV_SCALES)
    case = ScatterCase(
        name=f"all bf16 patterns, {'scaled' if scaled else 'unscaled'} fp8",
        T=T, nkv=n, hd=hd, bs=QUANT_BS, nb=QUANT_NB, layout="separate",
        kind="fp8s" if scaled else "fp8", bufs=(kb, vb),
        slots=torch.randperm(T, generator=_gen(7)).to(torch.int32),
        k_inv=inv if scaled else None,
        v_inv=inv.roll(1) if scaled else None)
    kk, vv = case.views(case.bufs)
    assert torch.equal(bits(kk), bits(k)) and torch.equal(bits(vv), bits(v))
    for h in range(n):   # every head sees every pattern
        assert bits(kk[:, h]).flatten().unique().numel() == 65536
    return case


# -------------------------------------------------------------------- RoPE

ROPE_MAX_LEN = 300
ROPE_THETA = 500000.0
ROPE_SHAPES = [  # (T, nq, n_kv, hd)
    (1, 1, 1, 16),
    (11, 5, 2, 96),    # 77 waves: partial last workgroup, partial-lane trip
    (9, 32, 8, 128),
    (5, 4, 2, 256),    # second trip of the lane loop
    (7, 2, 1, 64),
]
ROPE_CONFIGS = [dict(T=T, nq=nq, nkv=nkv, hd=hd, layout="fused")
                for (T, nq, nkv, hd) in ROPE_SHAPES]
ROPE_CONFIGS.append(dict(T=11, nq=5, nkv=2, hd=96, layout="separate"))
ROPE_PAD = 8
# 0 (the identity), the last table row, a repeated value; one token: the
# last table row
ROPE_POSITIONS = [0, 299, 7, 7, 150, 31, 0, 1, 298, 64, 100]
# the old check of test_ops_gpu.py::test_rope_strided
OLD_ROPE_TOL = 2e-2


@dataclass
class RopeCase:
    name: str
    T: int
    nq: int
    nkv: int
    hd: int
    layout: str               # "fused" | "separate"
    bufs: Tuple[torch.Tensor, ...]   # 2-D bf16 buffers behind q and k
    pos: torch.Tensor         # [T] int32
    cos: torch.Tensor         # [ROPE_MAX_LEN, hd/2] fp32
    sin: torch.Tensor

    def views(self, bufs):
        """(q, k) as views of the given buffers."""
        T, nq, n, hd = self.T, self.nq, self.nkv, self.hd
        if self.layout == "fused":
            (buf,) = bufs
            return (buf[:, :nq * hd].view(T, nq, hd),
                    buf[:, nq * hd:(nq + n) * hd].view(T, n, hd))
        qb, kb = bufs
        return qb[:, :nq * hd].view(T, nq, hd), kb[:, :n * hd].view(T, n, hd)


@functools.lru_cache(maxsize=None)
def rope_case(T, nq, nkv, hd, layout):
    g = _gen(100 * T + hd + len(layout))
    if layout == "fused":
        shapes = [(T, (nq + 2 * nkv) * hd + ROPE_PAD)]
    else:
        shapes = [(T, nq * hd + ROPE_PAD), (T, nkv * hd + 3 * ROPE_PAD)]
    # V and the padding: random bit patterns; q and k: finite values
    bufs = tuple(_random_bits(s, g) for s in shapes)
    cos, sin = R.rope_tables(ROPE_MAX_LEN, hd, ROPE_THETA, "cpu")
    pos = torch.tensor([299] if T == 1 else ROPE_POSITIONS[:T],
                       dtype=torch.int32)
    case = RopeCase(name=f"rope T{T} q{nq} kv{nkv} hd{hd} {layout}", T=T,
                    nq=nq, nkv=nkv, hd=hd, layout=layout, bufs=bufs, pos=pos,
                    cos=cos, sin=sin)
    for x in case.views(bufs):
        x.copy_((torch.randn(x.shape, generator=g) * 2).bfloat16())
    if layout == "separate":
        q, k = case.views(bufs)
        assert q.stride(0) != k.stride(0)
    return case


def _to_bf16(x, truncate):
    if not truncate:
        return x.bfloat16()
    return (x.contiguous().view(torch.int32) >> 16).to(torch.int16).view(
        torch.bfloat16)


def rope_model(case, mutant=None, fma=False):
    """The buffers after rotate-half RoPE in fp32 with one rounding to bf16,
    as the kernel computes it; fma=True contracts each product-and-sum as a
    compiler may. `mutant` names one of rope_mutants()."""
    bufs = tuple(b.clone() for b in case.bufs)
    half = case.hd // 2
    pos = case.pos.long()
    if mutant == "position + 1":
        pos = (pos + 1) % ROPE_MAX_LEN
    for x, is_k in zip(case.views(bufs), (False, True)):
        p = pos
        if is_k and mutant == "k rotated at the next token's position":
            p = pos.roll(-1)
        c = case.cos[p].unsqueeze(1)   # [T, 1, hd/2] fp32
        s = case.sin[p].unsqueeze(1)
        if mutant == "sin sign flipped":
            s = -s
        xf = x.float()
        if mutant == "interleaved (2i, 2i+1) pairs":
            x1, x2 = xf[..., 0::2], xf[..., 1::2]
        else:
            x1, x2 = xf[..., :half], xf[..., half:]
        if fma:
            o1 = (x1.double() * c.double() - (x2 * s).double()).float()
            o2 = (x2.double() * c.double() + (x1 * s).double()).float()
        else:
            o1, o2 = x1 * c - x2 * s, x2 * c + x1 * s
        if mutant == "pairs at d >= 64 not rotated":
            o1[..., 64:], o2[..., 64:] = x1[..., 64:], x2[..., 64:]
        trunc = mutant == "bf16 store by truncation"
        b1, b2 = _to_bf16(o1, trunc), _to_bf16(o2, trunc)
        if mutant == "interleaved (2i, 2i+1) pairs":
            x[..., 0::2], x[..., 1::2] = b1, b2
        else:
            x[..., :half], x[..., half:] = b1, b2
    return bufs


def rope_reference(case):
    """The buffers after ops/reference.py's rope_inplace."""
    bufs = tuple(b.clone() for b in case.bufs)
    q, k = case.views(bufs)
    R.rope_inplace(q, k, case.pos.long(), case.cos, case.sin)
    return bufs


def rope_mutants(case):
    out = ["sin sign flipped", "position + 1", "interleaved (2i, 2i+1) pairs",
           "bf16 store by truncation"]
    if case.T > 1:
        out.append("k rotated at the next token's position")
    if case.hd > 128:
        out.append("pairs at d >= 64 not rotated")
    return out


def check_rope(case, got_bufs, msg=""):
    """got_bufs: the case's buffers after the op.
      * outside the q and k views: bit-identical to the input;
      * tokens at position 0: bit-identical (cos = 1, sin = 0 exactly);
      * every other element: |got - exact| <= 2^-8 |exact| + 2^-22 (|x1| +
        |x2|), exact = the rotation in float64 on the fp32 table values,
        (x1, x2) the element's input pair. The first term is half a bf16
        ulp (a correctly rounded store), the second bounds the fp32 error
        of two products and a sum, contracted to fma or not.
    Returns the worst error / bound ratio."""
    name = f"{case.name} {msg}"
    got_bufs = tuple(b.detach().cpu() for b in got_bufs)
    for i, (got, orig) in enumerate(zip(got_bufs, case.bufs)):
        assert got.shape == orig.shape and got.dtype == orig.dtype
    marks = tuple(torch.zeros(b.shape, dtype=torch.bool) for b in case.bufs)
    for m in case.views(marks):
        m.fill_(True)
    for got, orig, m in zip(got_bufs, case.bufs, marks):
        changed = (bits(got) != bits(orig)) & ~m
        assert not bool(changed.any()), (
            f"{name}: {int(changed.sum())} elements outside the q and k "
            f"views changed; first at "
            f"{tuple(int(i) for i in changed.nonzero()[0])}")
    c = case.cos[case.pos.long()].double().unsqueeze(1)
    s = case.sin[case.pos.long()].double().unsqueeze(1)
    half = case.hd // 2
    still = case.pos == 0
    worst = 0.0
    for which, got, orig in zip("qk", case.views(got_bufs),
                                case.views(case.bufs)):
        same = bits(got[still]) == bits(orig[still])
        assert bool(same.all()), (
            f"{name}: {which} at position 0 is not bit-identical to its "
            f"input ({int((~same).sum())} elements)")
        x1, x2 = orig[..., :half].double(), orig[..., half:].double()
        exact = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
        mag = (x1.abs() + x2.abs()).repeat(1, 1, 2)
        bound = 2.0 ** -8 * exact.abs() + 2.0 ** -22 * mag
        g = got.double()
        assert bool(torch.isfinite(g).all()), f"{name}: non-finite {which}"
        err = (g - exact).abs()
        bad = err > bound
        assert not bool(bad.any()), (
            f"{name}: {int(bad.sum())}/{bad.numel()} elements of {which} "
            f"past the bound; worst error / bound "
            f"{float((err / bound)[bad].max()):.3f}")
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


def old_rope_check(case, got_bufs):
    """What test_ops_gpu.py::test_rope_strided asserts: the q and k views
    against the reference at atol = rtol = 2e-2."""
    for got, ref in zip(case.views(tuple(got_bufs)),
                        case.views(rope_reference(case))):
        diff = (got.float() - ref.float()).abs()
        assert bool((diff <= OLD_ROPE_TOL + OLD_ROPE_TOL * ref.float().abs())
                    .all())


# ---------------------------------------------- rope, then store: the chain

CHAIN_CONFIGS = [dict(hd=hd, kind=kind) for hd in (128, 64)
                 for kind in ("bf16", "fp8s")]
CHAIN_NQ, CHAIN_NKV, CHAIN_BS, CHAIN_PAGES = 4, 2, 16, 3


@dataclass
class ChainCase:
    name: str
    hd: int
    kind: str                 # "bf16" | "fp8s"
    qkv: torch.Tensor         # [B, (nq + 2 n_kv) * hd] bf16
    pos: torch.Tensor         # [B] int32: one decode token per sequence
    bt: torch.Tensor          # [B, CHAIN_PAGES] int32, a permutation
    cos: torch.Tensor
    sin: torch.Tensor
    k_inv: Optional[torch.Tensor] = None
    v_inv: Optional[torch.Tensor] = None
    nq: int = CHAIN_NQ
    nkv: int = CHAIN_NKV
    bs: int = CHAIN_BS

    @property
    def nb(self):
        return self.bt.numel() + 1   # page 0 is in no table

    def views(self, qkv):
        B, nq, n, hd = qkv.shape[0], self.nq, self.nkv, self.hd
        return (qkv[:, :nq * hd].view(B, nq, hd),
                qkv[:, nq * hd:(nq + n) * hd].view(B, n, hd),
                qkv[:, (nq + n) * hd:].view(B, n, hd))

    def caches(self):
        return tuple(sentinel_cache(self.nb, self.nkv, self.bs, self.hd,
                                    self.kind) for _ in range(2))

    def scale_kw(self):
        if self.kind != "fp8s":
            return {}
        return dict(k_inv_scale=self.k_inv, v_inv_scale=self.v_inv)

    def stored(self, k, v):
        """What the cache must hold for rows k, v: their storage bits."""
        return (_conv(self.kind, self.k_inv)(k.detach().cpu()),
                _conv(self.kind, self.v_inv)(v.detach().cpu()))


@functools.lru_cache(maxsize=None)
def chain_case(hd, kind):
    g = _gen(hd + len(kind))
    bs = CHAIN_BS
    # both sides of two page edges, the first slot of a sequence, mid-page
    pos = torch.tensor([bs - 1, bs, 2 * bs - 1, 2 * bs, 0, 2 * bs + 5],
                       dtype=torch.int32)
    B = pos.numel()
    bt = (torch.randperm(B * CHAIN_PAGES, generator=g) + 1).to(
        torch.int32).view(B, CHAIN_PAGES)
    qkv = (torch.randn(B, (CHAIN_NQ + 2 * CHAIN_NKV) * hd, generator=g)
           * 2).bfloat16()
    cos, sin = R.rope_tables(ROPE_MAX_LEN, hd, ROPE_THETA, "cpu")
    inv = torch.tensor(INV_SCALES[1:1 + CHAIN_NKV]) if kind == "fp8s" else None
    return ChainCase(name=f"chain hd{hd} {kind}", hd=hd, kind=kind, qkv=qkv,
                     pos=pos, bt=bt, cos=cos, sin=sin, k_inv=inv,
                     v_inv=None if inv is None else inv.flip(0))


def write_path_model(case, qkv, positions, slots,
                     rope: Callable = R.rope_inplace, mutant=None):
    """qkv, positions, slots -> (expected q [T, nq, hd] bf16, K cache bits,
    V cache bits): RoPE on the q and k views, then the store of the ROTATED
    k and of v into sentinel caches. A fused rope-and-append kernel has to
    produce exactly this up to the rounding check_rope allows on q and k;
    `rope` lets a test put the kernel's own rotation in."""
    qkv = qkv.detach().cpu().clone()
    q, k, v = case.views(qkv)
    k_before = k.clone()
    rope(q, k, positions.long().cpu(), case.cos, case.sin)
    kc, vc = (bits(c).clone() for c in case.caches())
    scatter_model(k_before if mutant == "store before rope" else k, v, kc, vc,
                  slots.cpu(), _conv(case.kind, case.k_inv),
                  _conv(case.kind, case.v_inv))
    return q, kc, vc


def gather_by_table(cache, bt, positions, bs):
    """The rows a reader finds for token b at positions[b] through block
    table row b: [B, n_kv, hd] storage bits."""
    cache = bits(cache)
    rows = []
    for b, p in enumerate(positions.tolist()):
        rows.append(cache[int(bt[b, p // bs]), :, p % bs, :])
    return torch.stack(rows)


def check_chain(case, qkv_after, kc, vc, msg=""):
    """Reading the cache through the block table at each token's position
    returns the post-RoPE K left in the buffer (through the encoder for an
    fp8 cache) and V bit for bit, and every other slot keeps the sentinel."""
    _q, k, v = case.views(qkv_after.detach().cpu())
    want_k, want_v = case.stored(k, v)
    name = f"{case.name} {msg}"
    assert_same_bits(gather_by_table(kc, case.bt, case.pos, case.bs), want_k,
                     f"{name}: K through the block table")
    assert_same_bits(gather_by_table(vc, case.bt, case.pos, case.bs), want_v,
                     f"{name}: V through the block table")
    # and nothing else was written: the whole cache, slot by slot
    for which, c, rows in (("K", kc, want_k), ("V", vc, want_v)):
        want = bits(sentinel_cache(case.nb, case.nkv, case.bs, case.hd,
                                   case.kind)).clone()
        for b, p in enumerate(case.pos.tolist()):
            want[int(case.bt[b, p // case.bs]), :, p % case.bs, :] = rows[b]
        assert_same_bits(c, want, f"{name}: whole {which} cache")
