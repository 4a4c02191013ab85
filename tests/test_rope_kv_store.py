"""ops.rope_kv_store on the CPU: the reference version is the composition of
reference.rope_inplace and reference.kv_cache_store, so the one call leaves
the qkv buffer and both caches bit for bit as the two calls do, and the
comparison that says so rejects a store of the unrotated k.

tests/test_rope_kv_store_gpu.py holds the fused HIP kernel to the same
comparison against the two HIP kernels.
"""
import pytest
import torch

from bee2bee_amd import ops
from bee2bee_amd.engine.graphs import decode_slot_mapping
from bee2bee_amd.ops import reference as R
from tests import write_path_probes as W

CONFIGS = W.CHAIN_CONFIGS + [dict(hd=hd, kind="fp8") for hd in (128, 64)]


def _ids(configs):
    return ["-".join(f"{k}{v}" for k, v in c.items()) for c in configs]


def _run(case, fn):
    """fn(q, k, v, pos, kc, vc, slots, **scales) on fresh copies of the
    case: (qkv, K cache, V cache) afterwards, and the slots."""
    qkv = case.qkv.clone()
    q, k, v = case.views(qkv)
    kc, vc = case.caches()
    slots = decode_slot_mapping(case.bt, case.pos, case.bs)
    fn(q, k, v, case.pos, kc, vc, slots, **case.scale_kw())
    return qkv, kc, vc, slots


def _two_ops(case):
    def fn(q, k, v, pos, kc, vc, slots, **kw):
        R.rope_inplace(q, k, pos, case.cos, case.sin)
        R.kv_cache_store(k, v, kc, vc, slots, **kw)
    return fn


def _one_call(case, op):
    def fn(q, k, v, pos, kc, vc, slots, **kw):
        op(q, k, v, pos, case.cos, case.sin, kc, vc, slots, **kw)
    return fn


def _same(case, got, want):
    for name, g, w in zip(("qkv", "K cache", "V cache"), got, want):
        W.assert_same_bits(g, w, f"{case.name}: whole {name}")


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids(CONFIGS))
@pytest.mark.parametrize("entry", ["reference", "ops"])
def test_one_call_is_the_two_op_chain(cfg, entry):
    case = W.chain_case(**cfg)
    op = R.rope_kv_store if entry == "reference" else ops.rope_kv_store
    *want, slots = _run(case, _two_ops(case))
    *got, _ = _run(case, _one_call(case, op))
    _same(case, got, want)
    W.check_chain(case, got[0], got[1], got[2], msg="rope_kv_store")
    # the one-call model says the same
    mq, mkc, mvc = W.write_path_model(case, case.qkv, case.pos, slots)
    assert torch.equal(W.bits(mq), W.bits(case.views(got[0])[0]))
    W.assert_same_bits(got[1], mkc, f"{case.name}: model K cache")
    W.assert_same_bits(got[2], mvc, f"{case.name}: model V cache")


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids(CONFIGS))
def test_the_comparison_rejects_a_store_before_rope(cfg):
    case = W.chain_case(**cfg)
    qkv, _kc, _vc, slots = _run(case, _one_call(case, R.rope_kv_store))
    _q, bkc, bvc = W.write_path_model(case, case.qkv, case.pos, slots,
                                      mutant="store before rope")
    with pytest.raises(AssertionError, match="K cache"):
        _same(case, (qkv, bkc, bvc), _run(case, _two_ops(case))[:3])


def test_empty_call_touches_nothing():
    case = W.chain_case(hd=64, kind="bf16")
    qkv = case.qkv.clone()
    q, k, v = case.views(qkv)
    kc, vc = case.caches()
    none = torch.zeros(0, dtype=torch.int32)
    R.rope_kv_store(q[:0], k[:0], v[:0], none, case.cos, case.sin, kc, vc,
                    none)
    _same(case, (qkv, kc, vc), (case.qkv, *case.caches()))
