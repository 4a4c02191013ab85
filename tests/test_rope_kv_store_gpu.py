"""ops.rope_kv_store on the GPU: the one call against ops.rope_inplace +
ops.kv_cache_store on clones of the same inputs, bit for bit over the WHOLE
qkv buffer (the v slice and the padding included) and the WHOLE of both
sentinel-filled caches, so a stray write shows as well as a wrong one.

The fused kernel (rope_kv_store_kernel, ops/csrc/elementwise.hip) takes
head_dim % 16 == 0 with token strides that are multiples of 8 elements and
16-byte-aligned bases; the binding runs the two separate kernels for
anything else. Both are held to the same comparison here. head_dim 96
meets the fused kernel's conditions (6 lanes per head, the one head size
here that is no power of two); head_dim 24, a token stride of 4 mod 8 and a
base that is only 8-byte aligned take the two-kernel path.

The rotation itself is held to its derived bound by
tests/test_write_path_gpu.py::test_rope_probes (rope_kernel calls the same
rope_rotate), and the chain cases below run W.check_chain and the
write_path_model comparison of test_rope_then_store_as_the_runner_chains_them
on the fused call.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.engine.graphs import decode_slot_mapping
from bee2bee_amd.ops import reference as R
from tests import write_path_probes as W
from tests.test_write_path_gpu import ROPE_REFUSALS, STORE_REFUSALS

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load

TS = (1, 3, 6, 67)          # a partial wave, the chain case's, > one block
HEADS = ((1, 1), (4, 2), (28, 4), (32, 8))   # G = 7 among them
KINDS = ("bf16", "fp8", "fp8s")
LAYOUTS = ("fused", "separate")
PADS = {"fused": (8,), "separate": (8, 24, 40)}   # strides stay 0 mod 8


class Case:
    """Buffers, positions, slots and caches of one call, on the CPU."""

    def __init__(self, T, nq, nkv, hd, bs, layout, kind, pads=None,
                 lead=0, seed=0):
        g = torch.Generator().manual_seed(
            seed + 7 * T + 11 * nq + 13 * hd + bs + len(layout) + len(kind))
        self.T, self.nq, self.nkv, self.hd, self.bs = T, nq, nkv, hd, bs
        self.layout, self.kind, self.lead = layout, kind, lead
        self.name = f"T{T} q{nq} kv{nkv} hd{hd} bs{bs} {layout} {kind}"
        pads = PADS[layout] if pads is None else pads
        widths = ([(nq + 2 * nkv) * hd] if layout == "fused"
                  else [nq * hd, nkv * hd, nkv * hd])
        # v and the padding: random bit patterns (NaNs included); q, k finite
        self.bufs = tuple(W._random_bits((T, lead + w + p), g)
                          for w, p in zip(widths, pads))
        for x in self.views(self.bufs)[:2]:
            x.copy_((torch.randn(x.shape, generator=g) * 2).bfloat16())
        self.nb = max(2, -(-T // bs) + 1)
        self.slots = W.probe_slots(T, bs, self.nb, g)
        self.cos, self.sin = R.rope_tables(W.ROPE_MAX_LEN, hd, W.ROPE_THETA,
                                           "cpu")
        pos = torch.randint(0, W.ROPE_MAX_LEN, (T,), generator=g)
        pos[0] = W.ROPE_MAX_LEN - 1         # the last table row
        if T > 1:
            pos[1] = 0                      # the identity
        self.pos = pos.to(torch.int32)
        self.scales = {}
        if kind == "fp8s":   # per head, and K's differ from V's
            inv = torch.tensor([W.INV_SCALES[h % 4] for h in range(nkv)])
            self.scales = dict(
                k_inv_scale=inv,
                v_inv_scale=torch.tensor(
                    [W.INV_SCALES[(h + 1) % 4] for h in range(nkv)]))

    def views(self, bufs):
        T, nq, n, hd, o = self.T, self.nq, self.nkv, self.hd, self.lead
        if self.layout == "fused":
            (b,) = bufs
            cut = [o, o + nq * hd, o + (nq + n) * hd, o + (nq + 2 * n) * hd]
            return tuple(b[:, cut[i]:cut[i + 1]].view(T, h, hd)
                         for i, h in enumerate((nq, n, n)))
        return tuple(b[:, o:o + h * hd].view(T, h, hd)
                     for b, h in zip(bufs, (nq, n, n)))

    def caches(self):
        return tuple(W.sentinel_cache(self.nb, self.nkv, self.bs, self.hd,
                                      self.kind) for _ in range(2))

    def run(self, fused, T=None):
        """The call on device clones: (bufs, K cache, V cache) on the CPU."""
        bufs = tuple(b.to(DEV, copy=True) for b in self.bufs)
        q, k, v = (x[:T] for x in self.views(bufs))
        kc, vc = (c.to(DEV) for c in self.caches())
        pos, slots = self.pos[:T].to(DEV), self.slots[:T].to(DEV)
        cos, sin = self.cos.to(DEV), self.sin.to(DEV)
        kw = {n: s.to(DEV) for n, s in self.scales.items()}
        if fused:
            ops.rope_kv_store(q, k, v, pos, cos, sin, kc, vc, slots, **kw)
        else:
            ops.rope_inplace(q, k, pos, cos, sin)
            ops.kv_cache_store(k, v, kc, vc, slots, **kw)
        torch.cuda.synchronize()
        return tuple(b.cpu() for b in bufs), kc.cpu(), vc.cpu()


def assert_same_call(case, got, want):
    for i, (g, w) in enumerate(zip(got[0], want[0])):
        W.assert_same_bits(g, w, f"{case.name}: whole buffer {i}")
    W.assert_same_bits(got[1], want[1], f"{case.name}: whole K cache")
    W.assert_same_bits(got[2], want[2], f"{case.name}: whole V cache")


def check_against_the_two_ops(case):
    want = case.run(fused=False)
    got = case.run(fused=True)
    assert_same_call(case, got, want)
    # the two ops did something: the comparison is not sentinel to sentinel
    assert not torch.equal(W.bits(want[1]), W.bits(case.caches()[0]))


FAST = [dict(T=T, nq=nq, nkv=nkv, hd=hd, bs=bs, layout=layout, kind=kind)
        for T, (nq, nkv), hd, bs, layout, kind in itertools.product(
            TS, HEADS, (64, 128), (16, 256), LAYOUTS, KINDS)]


def _ids(configs):
    return ["-".join(f"{k}{v}" for k, v in c.items() if k != "pads")
            for c in configs]


@pytest.mark.parametrize("cfg", FAST, ids=_ids(FAST))
def test_fused_kernel_is_the_two_ops(cfg):
    check_against_the_two_ops(Case(**cfg))


OTHER = [dict(T=T, nq=nq, nkv=nkv, hd=hd, bs=16, layout=layout, kind=kind,
              **extra)
         for (hd, extra), T, (nq, nkv), layout, kind in itertools.product(
             ((96, {}),                       # 6 lanes per head
              (24, {}),                       # hd % 16 != 0: two kernels
              (128, {"pads": (4, 4, 12)}),    # stride 4 mod 8: two kernels
              # strides 0 mod 8, but a base that is only 8-byte aligned: two
              (64, {"lead": 4, "pads": (4, 12, 20)})),
             (3, 67), ((4, 2), (28, 4)), LAYOUTS, KINDS)]


@pytest.mark.parametrize("cfg", OTHER, ids=[
    f"{i}-" + s for i, s in enumerate(_ids(OTHER))])
def test_other_layouts_are_the_two_ops(cfg):
    case = Case(**cfg)
    q, k, v = case.views(case.bufs)
    if cfg["hd"] == 128:
        assert all(x.stride(0) % 8 == 4 for x in (q, k, v))
    if cfg["hd"] == 64:
        assert all(x.stride(0) % 8 == 0 and x.storage_offset() % 8 == 4
                   for x in (q, k, v))
    check_against_the_two_ops(case)


CHAIN = W.CHAIN_CONFIGS + [dict(hd=hd, kind="fp8") for hd in (128, 64)]


@pytest.mark.parametrize("cfg", CHAIN, ids=_ids(CHAIN))
def test_chain_case_through_the_fused_call(cfg):
    """Positions on both sides of two page edges, slots from the engine's
    decode_slot_mapping on a permuted block table."""
    case = W.chain_case(**cfg)
    pos = case.pos.to(DEV)
    slots = decode_slot_mapping(case.bt.to(DEV), pos, case.bs)
    cos, sin = case.cos.to(DEV), case.sin.to(DEV)
    kw = {n: s.to(DEV) for n, s in case.scale_kw().items()}

    def run(fused):
        qkv = case.qkv.to(DEV, copy=True)
        q, k, v = case.views(qkv)
        kc, vc = (c.to(DEV) for c in case.caches())
        if fused:
            ops.rope_kv_store(q, k, v, pos, cos, sin, kc, vc, slots, **kw)
        else:
            ops.rope_inplace(q, k, pos, cos, sin)
            ops.kv_cache_store(k, v, kc, vc, slots, **kw)
        return qkv.cpu(), kc.cpu(), vc.cpu()

    want, (qkv, kc, vc) = run(False), run(True)
    for name, g, w in zip(("qkv", "K cache", "V cache"), (qkv, kc, vc), want):
        W.assert_same_bits(g, w, f"{case.name}: whole {name}")
    W.check_chain(case, qkv, kc, vc, msg="fused")

    # the one-call model with the kernel's own rotation put in says the same
    def kernel_rope(mq, mk, *_):
        gq, gk, _gv = case.views(qkv)
        mq.copy_(gq)
        mk.copy_(gk)

    _mq, mkc, mvc = W.write_path_model(case, case.qkv, case.pos, slots,
                                       rope=kernel_rope)
    W.assert_same_bits(kc, mkc, f"{case.name}: model K cache")
    W.assert_same_bits(vc, mvc, f"{case.name}: model V cache")
    rq, _kc, _vc = W.write_path_model(case, case.qkv, case.pos, slots)
    q = case.views(qkv)[0]
    assert torch.allclose(q.float(), rq.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hd", [128, 24])
def test_empty_call_leaves_everything_alone(kind, hd):
    case = Case(T=3, nq=4, nkv=2, hd=hd, bs=16, layout="fused", kind=kind)
    bufs, kc, vc = case.run(fused=True, T=0)
    assert_same_call(case, (bufs, kc, vc), (case.bufs, *case.caches()))


# ------------------------------------------ calls the binding refuses

def _args():
    """A valid tiny call, by name: the baselines of the two ops' refusal
    tables put together."""
    T, nq, n, hd, bs, nb = 3, 2, 2, 16, 4, 2
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.bfloat16)
    t = lambda: torch.zeros(8, hd // 2, device=DEV, dtype=torch.float32)
    return dict(q=z(T, nq, hd), k=z(T, n, hd), v=z(T, n, hd),
                pos=torch.arange(T, device=DEV, dtype=torch.int32),
                cos=t(), sin=t(), k_cache=z(nb, n, bs, hd),
                v_cache=z(nb, n, bs, hd),
                slots=torch.arange(T, device=DEV, dtype=torch.int32))


def _call(a, **kw):
    HIP.rope_kv_store(a["q"], a["k"], a["v"], a["pos"], a["cos"], a["sin"],
                      a["k_cache"], a["v_cache"], a["slots"],
                      kw.get("k_inv_scale"), kw.get("v_inv_scale"))


def _untouched(a, before):
    torch.cuda.synchronize()
    for name, was in before.items():
        if a[name].is_cuda and a[name].shape == was.shape \
                and a[name].dtype == was.dtype:
            assert torch.equal(a[name].cpu(), was), name


def test_accepts_the_baseline_of_the_refusals():
    _call(_args())
    torch.cuda.synchronize()


REFUSALS = {f"rope: {n}": f for n, f in ROPE_REFUSALS.items()}
REFUSALS.update({f"store: {n}": f for n, f in STORE_REFUSALS.items()})


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refuses_what_either_op_refuses(what):
    """Every condition rope_inplace or kv_cache_store refuses, refused here
    before any launch: q, k, v and the caches keep their contents."""
    a = _args()
    for name in ("q", "k", "v", "k_cache", "v_cache"):
        a[name].fill_(1.0)
    if what == "rope: odd head_dim":
        # the rope table's own baseline, at the store's shapes
        a.update(q=a["q"][..., :15], k=a["k"][..., :15], v=a["v"][..., :15],
                 cos=a["cos"][:, :7], sin=a["sin"][:, :7])
    else:
        REFUSALS[what](a)
    before = {n: a[n].cpu().clone()
              for n in ("q", "k", "v", "k_cache", "v_cache")}
    with pytest.raises(RuntimeError, match="rope|kv_cache_store|must be"):
        _call(a)
    _untouched(a, before)


SCALE_REFUSALS = {
    "one scale only": lambda s: s.update(v_inv_scale=None),
    "scales with a bf16 cache": lambda s: None,
    "scales fp64": lambda s: s.update(k_inv_scale=s["k_inv_scale"].double()),
    "scales on the CPU": lambda s: s.update(
        v_inv_scale=s["v_inv_scale"].cpu()),
    "scales of another length": lambda s: s.update(
        k_inv_scale=s["k_inv_scale"][:1]),
}


@pytest.mark.parametrize("what", list(SCALE_REFUSALS))
def test_refuses_bad_scales(what):
    a = _args()
    if what != "scales with a bf16 cache":
        a.update(k_cache=a["k_cache"].view(torch.uint8)[..., :16].contiguous(),
                 v_cache=a["v_cache"].view(torch.uint8)[..., :16].contiguous())
    s = dict(k_inv_scale=torch.ones(2, device=DEV),
             v_inv_scale=torch.ones(2, device=DEV))
    if what != "scales with a bf16 cache":
        _call(a, **s)   # the baseline of this table is accepted
    SCALE_REFUSALS[what](s)
    with pytest.raises(RuntimeError, match="kv_cache_store|scales"):
        _call(a, **s)


def test_refuses_tokens_for_an_empty_cache():
    a = _args()
    a.update(k_cache=a["k_cache"][:0], v_cache=a["v_cache"][:0])
    with pytest.raises(RuntimeError, match="empty cache"):
        _call(a)


# ------------------------------------------------------------ graph replay

@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_follows_new_inputs(kind):
    """Capture the call once; replay it twice with new contents in pos,
    slots and qkv. Each replay must leave what the eager call leaves."""
    cases = [Case(T=67, nq=32, nkv=8, hd=128, bs=16, layout="fused",
                  kind=kind, seed=s) for s in (0, 1, 2)]
    c0 = cases[0]
    assert not torch.equal(cases[1].pos, cases[2].pos)
    assert not torch.equal(cases[1].slots, cases[2].slots)
    (buf,) = (b.to(DEV) for b in c0.bufs)
    q, k, v = c0.views((buf,))
    kc, vc = (c.to(DEV) for c in c0.caches())
    pos, slots = c0.pos.to(DEV), c0.slots.to(DEV)
    cos, sin = c0.cos.to(DEV), c0.sin.to(DEV)
    kw = {n: s.to(DEV) for n, s in c0.scales.items()}

    def call():
        ops.rope_kv_store(q, k, v, pos, cos, sin, kc, vc, slots, **kw)

    def load(case):
        buf.copy_(case.bufs[0])
        pos.copy_(case.pos)
        slots.copy_(case.slots)
        for c, fresh in zip((kc, vc), case.caches()):
            c.copy_(fresh)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):  # warm-up outside capture
        call()
    torch.cuda.current_stream().wait_stream(stream)
    load(c0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for case in cases[1:]:
        load(case)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_call(case, ((buf.cpu(),), kc.cpu(), vc.cpu()),
                         case.run(fused=True))
        assert_same_call(case, ((buf.cpu(),), kc.cpu(), vc.cpu()),
                         case.run(fused=False))
