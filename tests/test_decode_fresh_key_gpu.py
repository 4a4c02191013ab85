"""A decode step reads the key it has just written.

The decode kernels may read the KV stream with non-temporal loads (DEC_K_NT
/ DEC_V_NT in ops/csrc/attn_decode.hip). Such a read must still see the row
the previous launch on the same stream stored, at the slot where a stale row
stood before. So: the write path (ops.rope_kv_store, or the two ops), then
ops.attn_decode on the same stream, with a newest key built as in
tests/kernel_probes.py (k = c * base against q = base + noise, rotated at
the same position, which leaves their dot product alone), so that it carries
most of the softmax weight: an output computed from the stale row is far
outside the tolerance. The reference is ops/reference.py on the CPU, write
path included, at the suite's decode tolerances.

Then the same inside one captured graph, replayed three times with a
different newest key, value and query each time: the row a replay must read
is the one that same replay wrote over the previous replay's.
"""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.engine.graphs import decode_slot_mapping
from bee2bee_amd.ops import reference as R
from tests import kernel_probes as P
from tests import write_path_probes as W

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load

B, NKV, G = 3, 2, 4
NQ = NKV * G
CONFIGS = [dict(hd=hd, L=L, bs=bs, cache=cache)
           for hd, L, bs, cache in itertools.product(
               (64, 128), (255, 256, 257), (16, 256), ("bf16", "fp8"))]
IDS = ["-".join(f"{k}{v}" for k, v in c.items()) for c in CONFIGS]


class Stream:
    """B sequences of L - 1 cached keys each, on their own pages behind a
    permuted block table whose page 0 is unused; slot L - 1 of every
    sequence holds a stale row. step(i) is the i-th newest token: the qkv
    buffer before RoPE."""

    def __init__(self, hd, L, bs, cache):
        g = torch.Generator().manual_seed(hd + L + bs + len(cache))
        self.hd, self.L, self.bs, self.cache = hd, L, bs, cache
        self.fp8 = cache == "fp8"
        # kernel_probes.build_attn's scales for a decode case
        self.q_scale, self.kv_scale = (0.2, 0.7) if self.fp8 else (1.0, 1.0)
        self.c = P._probe_c(hd, self.q_scale)
        self.tol = P.TOL_FP8 if self.fp8 else P.TOL_DECODE
        Wp = L // bs + 1
        nb = 1 + B * Wp
        self.bt = (torch.randperm(B * Wp, generator=g) + 1).reshape(
            B, Wp).to(torch.int32)
        self.kc = self._as_cache(torch.randn(nb, NKV, bs, hd, generator=g))
        self.vc = self._as_cache(torch.randn(nb, NKV, bs, hd, generator=g))
        self.pos = torch.full((B,), L - 1, dtype=torch.int32)
        self.lens = torch.full((B,), L, dtype=torch.int32)
        self.slots = decode_slot_mapping(self.bt, self.pos, bs)
        self.cos, self.sin = R.rope_tables(W.ROPE_MAX_LEN, hd, W.ROPE_THETA,
                                           "cpu")
        assert L <= W.ROPE_MAX_LEN
        self.g = g

    def _as_cache(self, x):
        x = x * self.kv_scale
        if self.fp8:
            return x.to(torch.float8_e4m3fn).view(torch.uint8)
        return x.bfloat16()

    def step(self, i):
        g = torch.Generator().manual_seed(1000 * i + self.hd + self.L)
        hd = self.hd
        base = torch.randn(B, NKV, hd, generator=g)
        base *= math.sqrt(hd) / base.norm(dim=-1, keepdim=True)
        assert float((self.c * base).abs().max()) < R.E4M3_MAX
        q = base.view(B, NKV, 1, hd) + 0.5 * torch.randn(B, NKV, G, hd,
                                                         generator=g)
        q = (q * self.q_scale).reshape(B, NQ * hd)
        k = (self.c * base).reshape(B, NKV * hd)
        v = (torch.randn(B, NKV * hd, generator=g) * self.kv_scale)
        return torch.cat([q, k, v], dim=-1).bfloat16()

    def views(self, qkv):
        hd = self.hd
        return (qkv[:, :NQ * hd].view(B, NQ, hd),
                qkv[:, NQ * hd:(NQ + NKV) * hd].view(B, NKV, hd),
                qkv[:, (NQ + NKV) * hd:].view(B, NKV, hd))

    def reference(self, qkv):
        """ops/reference.py on the CPU: write path, then decode. Also the
        newest key's least softmax weight over all (sequence, head)."""
        qkv = qkv.clone()
        q, k, v = self.views(qkv)
        kc, vc = self.kc.clone(), self.vc.clone()
        R.rope_kv_store(q, k, v, self.pos.long(), self.cos, self.sin, kc, vc,
                        self.slots)
        scale = self.hd ** -0.5
        out = R.attn_decode(q, kc, vc, self.bt, self.lens, scale)
        # the newest key's weight, from the rotated q and the stored row
        blk = (self.slots // self.bs).long()
        off = (self.slots % self.bs).long()
        knew = R._kv_deq(kc[blk, :, off, :])             # [B, NKV, hd]
        s_new = torch.einsum("bngd,bnd->bng",
                             q.float().view(B, NKV, G, self.hd), knew) * scale
        ml = torch.zeros(B, NQ, 2)
        R.attn_decode(q, kc, vc, self.bt, self.lens, scale, out_ml=ml)
        w = torch.exp(s_new.reshape(B, NQ) - ml[..., 0]) / ml[..., 1]
        return out, float(w.min())


def _device_state(st):
    d = dict(kc=st.kc.to(DEV, copy=True), vc=st.vc.to(DEV, copy=True),
             bt=st.bt.to(DEV), pos=st.pos.to(DEV), lens=st.lens.to(DEV),
             slots=st.slots.to(DEV), cos=st.cos.to(DEV), sin=st.sin.to(DEV))
    return d


def _step(st, d, qkv, fused):
    q, k, v = st.views(qkv)
    if fused:
        ops.rope_kv_store(q, k, v, d["pos"], d["cos"], d["sin"], d["kc"],
                          d["vc"], d["slots"])
    else:
        ops.rope_inplace(q, k, d["pos"], d["cos"], d["sin"])
        ops.kv_cache_store(k, v, d["kc"], d["vc"], d["slots"])
    return ops.attn_decode(q, d["kc"], d["vc"], d["bt"], d["lens"],
                           st.hd ** -0.5)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-ops"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_decode_reads_the_key_just_stored(cfg, fused):
    st = Stream(**cfg)
    qkv = st.step(0)
    want, weight = st.reference(qkv)
    assert weight >= P.MIN_PROBE_WEIGHT, f"newest key weighs {weight:.3f}"
    # reading the stale row instead is far outside the tolerance
    stale, _ = Stream.reference(_without_the_store(st), qkv)
    assert float((stale - want).abs().max()) > 5 * st.tol * (
        1 + float(want.abs().max()))
    d = _device_state(st)
    out = _step(st, d, qkv.to(DEV, copy=True), fused)
    P.assert_close(out, want, atol=st.tol, rtol=st.tol,
                   msg=f"{IDS[CONFIGS.index(cfg)]} newest weight {weight:.2f}")


class _without_the_store:
    """A Stream whose reference write lands on a page no sequence reads."""

    def __init__(self, st):
        self.__dict__.update(st.__dict__)
        self.slots = torch.arange(B, dtype=torch.int32)   # page 0: unused
        assert B <= st.bs

    views = Stream.views


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_graph_replays_read_their_own_newest_key(cfg):
    st = Stream(**cfg)
    d = _device_state(st)
    static = st.step(0).to(DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):  # warm-up outside capture
        _step(st, d, static, True)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(st, d, static, True)
    for i in (1, 2, 3):
        qkv = st.step(i)
        want, weight = st.reference(qkv)
        assert weight >= P.MIN_PROBE_WEIGHT, f"newest key weighs {weight:.3f}"
        static.copy_(qkv)
        graph.replay()
        torch.cuda.synchronize()
        P.assert_close(out, want, atol=st.tol, rtol=st.tol,
                       msg=f"{IDS[CONFIGS.index(cfg)]} replay {i}")
