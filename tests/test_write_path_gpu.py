"""The write-path cases of tests/write_path_probes.py through the HIP
kernels: rope_kernel, kv_store_kernel and kv_store_fp8_kernel
(ops/csrc/elementwise.hip), bit for bit where the operation is exact and at
a derived bound where it rounds. tests/test_write_path.py proves on the CPU
that a write path which is one slot, head, stride or rounding step off fails
here.

Also: the calls the bindings of rope_inplace and kv_cache_store refuse
before any launch. Each of them would otherwise read or write out of bounds,
so every refusal below relies on a TORCH_CHECK that stands before the launch
in ops/csrc/ext.cpp.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.engine.graphs import decode_slot_mapping
from tests import write_path_probes as W

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load


def _ids(configs):
    return ["-".join(f"{k}{v}" for k, v in c.items()) for c in configs]


def _store(case):
    """The case's store on the GPU, into sentinel caches: (kc, vc) on the
    CPU. k and v are views of device copies of the case's buffers, so the
    strides are the case's."""
    k, v = case.views(tuple(b.to(DEV) for b in case.bufs))
    kc, vc = (c.to(DEV) for c in case.caches())
    kw = {n: s.to(DEV) for n, s in case.scale_kw().items()}
    ops.kv_cache_store(k, v, kc, vc, case.slots.to(DEV), **kw)
    return kc.cpu(), vc.cpu()


# --------------------------------------------------------------- quantizer

@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
def test_fp8_store_on_every_bf16_pattern(scaled):
    """One launch: every kv head converts all 65 536 bf16 patterns, and the
    whole cache must hold the plain-torch encoder's bytes (NaN bytes compared
    by NaN-ness). Unscaled: overflow above 464 is a NaN byte, as torch's
    cast has it. Scaled: clamped to +-448, inf included, and NaN stays NaN.
    The scales differ by head, and between K and V."""
    case = W.quant_case(scaled)
    kc, vc = _store(case)
    W.check_scatter(case, kc, vc)


# ----------------------------------------------------------------- scatter

@pytest.mark.parametrize("cfg", W.SCATTER_CONFIGS,
                         ids=_ids(W.SCATTER_CONFIGS))
def test_scatter_probes(cfg):
    case = W.scatter_case(**cfg)
    kc, vc = _store(case)
    W.check_scatter(case, kc, vc)


@pytest.mark.parametrize("kind", W.CACHE_KINDS)
def test_empty_store_leaves_the_cache_alone(kind):
    case = W.scatter_case(T=7, nkv=3, hd=96, bs=32, nb=3, layout="fused",
                          kind=kind)
    k, v = case.views(tuple(b.to(DEV) for b in case.bufs))
    kc, vc = (c.to(DEV) for c in case.caches())
    kw = {n: s.to(DEV) for n, s in case.scale_kw().items()}
    ops.kv_cache_store(k[:0], v[:0], kc, vc, case.slots[:0].to(DEV), **kw)
    for got, want in zip((kc, vc), case.caches()):
        W.assert_same_bits(got, want, f"{case.name}: T = 0")


# -------------------------------------------------------------------- RoPE

@pytest.mark.parametrize("cfg", W.ROPE_CONFIGS, ids=_ids(W.ROPE_CONFIGS))
def test_rope_probes(cfg):
    case = W.rope_case(**cfg)
    bufs = tuple(b.to(DEV) for b in case.bufs)
    q, k = case.views(bufs)
    ops.rope_inplace(q, k, case.pos.to(DEV), case.cos.to(DEV),
                     case.sin.to(DEV))
    ratio = W.check_rope(case, bufs)
    print(f"{case.name}: worst error / bound {ratio:.3f}")


# ------------------------------------------------------------------- chain

@pytest.mark.parametrize("cfg", W.CHAIN_CONFIGS, ids=_ids(W.CHAIN_CONFIGS))
def test_rope_then_store_as_the_runner_chains_them(cfg):
    """Slots from the engine's decode_slot_mapping on a permuted block
    table, positions on both sides of page edges: reading the cache through
    the table returns the ROTATED k the kernel left in the buffer, and v."""
    case = W.chain_case(**cfg)
    qkv = case.qkv.to(DEV)
    q, k, v = case.views(qkv)
    kc, vc = (c.to(DEV) for c in case.caches())
    pos = case.pos.to(DEV)
    slots = decode_slot_mapping(case.bt.to(DEV), pos, case.bs)
    kw = {n: s.to(DEV) for n, s in case.scale_kw().items()}
    ops.rope_inplace(q, k, pos, case.cos.to(DEV), case.sin.to(DEV))
    ops.kv_cache_store(k, v, kc, vc, slots, **kw)
    W.check_chain(case, qkv, kc, vc)
    # the one-call model with the kernel's own rotation put in says the same
    after = qkv.cpu()

    def kernel_rope(mq, mk, *_):
        gq, gk, _gv = case.views(after)
        mq.copy_(gq)
        mk.copy_(gk)

    mq, mkc, mvc = W.write_path_model(case, case.qkv, case.pos, slots,
                                      rope=kernel_rope)
    W.assert_same_bits(kc, mkc, f"{case.name}: model K cache")
    W.assert_same_bits(vc, mvc, f"{case.name}: model V cache")
    # and with the reference's rotation, q agrees to 2e-2 (a sanity check:
    # test_rope_probes holds the kernel to the derived bound)
    rq, _kc, _vc = W.write_path_model(case, case.qkv, case.pos, slots)
    assert torch.allclose(q.cpu().float(), rq.float(), atol=2e-2, rtol=2e-2)


# ------------------------------------ calls the bindings refuse, unlaunched

def _store_args():
    """A valid tiny kv_cache_store call, by name."""
    T, n, hd, bs, nb = 3, 2, 16, 4, 2
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.bfloat16)
    return dict(k=z(T, n, hd), v=z(T, n, hd), k_cache=z(nb, n, bs, hd),
                v_cache=z(nb, n, bs, hd),
                slots=torch.arange(T, device=DEV, dtype=torch.int32))


def _call_store(a):
    HIP.kv_cache_store(a["k"], a["v"], a["k_cache"], a["v_cache"],
                       a["slots"], None, None)


STORE_REFUSALS = {
    "k not bf16": lambda a: a.update(k=a["k"].half()),
    "k on the CPU": lambda a: a.update(k=a["k"].cpu()),
    "k 2-D": lambda a: a.update(k=a["k"].flatten(1), v=a["v"].flatten(1)),
    "v not bf16": lambda a: a.update(v=a["v"].float()),
    "v on the CPU": lambda a: a.update(v=a["v"].cpu()),
    "v with fewer tokens": lambda a: a.update(v=a["v"][:2]),
    "v with fewer heads": lambda a: a.update(v=a["v"][:, :1]),
    "v with a smaller head_dim": lambda a: a.update(v=a["v"][..., :8]),
    "v 2-D": lambda a: a.update(v=a["v"].flatten(1)),
    "caches 3-D": lambda a: a.update(k_cache=a["k_cache"].flatten(0, 1),
                                     v_cache=a["v_cache"].flatten(0, 1)),
    "caches 5-D": lambda a: a.update(k_cache=a["k_cache"][None],
                                     v_cache=a["v_cache"][None]),
    "v_cache with fewer blocks": lambda a: a.update(
        v_cache=a["v_cache"][:1]),
    "v_cache with a smaller block size": lambda a: a.update(
        v_cache=a["v_cache"][:, :, :2].contiguous()),
    "v_cache of another dtype": lambda a: a.update(
        v_cache=a["v_cache"].view(torch.uint8)[..., :16].contiguous()),
    "v_cache on the CPU": lambda a: a.update(v_cache=a["v_cache"].cpu()),
    "k_cache on the CPU": lambda a: a.update(k_cache=a["k_cache"].cpu()),
    "cache heads differ from k's": lambda a: a.update(
        k_cache=a["k_cache"][:, :1].contiguous(),
        v_cache=a["v_cache"][:, :1].contiguous()),
    "slots int64": lambda a: a.update(slots=a["slots"].long()),
    "slots 2-D": lambda a: a.update(slots=a["slots"].view(3, 1)),
    "slots not contiguous": lambda a: a.update(
        slots=torch.arange(6, device=DEV, dtype=torch.int32)[::2]),
    "slots on the CPU": lambda a: a.update(slots=a["slots"].cpu()),
    "slots shorter than T": lambda a: a.update(slots=a["slots"][:2]),
    "slots longer than T": lambda a: a.update(
        slots=torch.arange(4, device=DEV, dtype=torch.int32)),
}


def test_kv_cache_store_accepts_the_baseline_of_the_refusals():
    a = _store_args()
    _call_store(a)
    torch.cuda.synchronize()


@pytest.mark.parametrize("what", list(STORE_REFUSALS))
def test_kv_cache_store_refuses(what):
    a = _store_args()
    STORE_REFUSALS[what](a)
    with pytest.raises(RuntimeError, match="kv_cache_store|must be"):
        _call_store(a)


def _rope_args(hd=16):
    T, nq, n = 3, 2, 1
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.bfloat16)
    t = lambda: torch.zeros(8, hd // 2, device=DEV, dtype=torch.float32)
    return dict(q=z(T, nq, hd), k=z(T, n, hd),
                pos=torch.arange(T, device=DEV, dtype=torch.int32),
                cos=t(), sin=t())


def _call_rope(a):
    HIP.rope_inplace(a["q"], a["k"], a["pos"], a["cos"], a["sin"])


ROPE_REFUSALS = {
    "q 2-D": lambda a: a.update(q=a["q"].flatten(1)),
    "q 4-D": lambda a: a.update(q=a["q"][None]),
    "k 2-D": lambda a: a.update(k=a["k"].flatten(1)),
    "odd head_dim": lambda a: a.update(_rope_args(hd=15)),
    "head_dim 0": lambda a: a.update(q=a["q"][..., :0], k=a["k"][..., :0],
                                     cos=a["cos"][:, :0], sin=a["sin"][:, :0]),
    "pos int64": lambda a: a.update(pos=a["pos"].long()),
    "pos 2-D": lambda a: a.update(pos=a["pos"].view(3, 1)),
    "pos not contiguous": lambda a: a.update(
        pos=torch.arange(6, device=DEV, dtype=torch.int32)[::2]),
    "pos on the CPU": lambda a: a.update(pos=a["pos"].cpu()),
    "pos shorter than T": lambda a: a.update(pos=a["pos"][:2]),
    "pos longer than T": lambda a: a.update(
        pos=torch.arange(4, device=DEV, dtype=torch.int32)),
    "cos fp64": lambda a: a.update(cos=a["cos"].double()),
    "sin bf16": lambda a: a.update(sin=a["sin"].bfloat16()),
    "cos on the CPU": lambda a: a.update(cos=a["cos"].cpu()),
    "sin on the CPU": lambda a: a.update(sin=a["sin"].cpu()),
    "sin with fewer rows": lambda a: a.update(sin=a["sin"][:4]),
    "sin 1-D": lambda a: a.update(sin=a["sin"].flatten()),
    "tables of another head_dim": lambda a: a.update(
        cos=a["cos"][:, :4].contiguous(), sin=a["sin"][:, :4].contiguous()),
}


def test_rope_accepts_the_baseline_of_the_refusals():
    _call_rope(_rope_args())
    torch.cuda.synchronize()


@pytest.mark.parametrize("what", list(ROPE_REFUSALS))
def test_rope_refuses(what):
    a = _rope_args()
    ROPE_REFUSALS[what](a)
    with pytest.raises(RuntimeError, match="rope|must be"):
        _call_rope(a)
