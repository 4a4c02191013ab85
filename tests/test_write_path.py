"""Standing proof that the write-path probes of tests/write_path_probes.py
have power (CPU only):

  * the plain-torch e4m3 encoder and ops/reference.py's two quantizers are
    two independent definitions, and agree on all 65 536 bf16 patterns;
  * ops/reference.py's store and rope pass the checkers that the HIP kernels
    meet in tests/test_write_path_gpu.py;
  * every mutant (a wrong model in plain torch) fails them. No mutant may
    survive and there is no waiver list;
  * the two checks this replaces would have let a mutant through: a
    zero-prefilled cache does not see a stray write of zeros, and the
    2e-2 tolerance does not see a truncating bf16 store.

`pytest -s` prints one line per mutant with the case that kills it.
"""
import pytest
import torch

from bee2bee_amd.engine.graphs import decode_slot_mapping
from bee2bee_amd.ops import reference as R
from tests import write_path_probes as W


def _ids(configs):
    return ["-".join(f"{k}{v}" for k, v in c.items()) for c in configs]


def _killed(case_name, mutant, fn):
    """The checker must raise on the mutant's output."""
    try:
        fn()
    except AssertionError as e:
        print(f"KILLED  {case_name:44s} {mutant:40s} "
              f"{str(e).split(': ', 1)[-1][:60]}")
        return
    pytest.fail(f"mutant survived: {case_name}: {mutant}")


# --------------------------------------------------------------- quantizer

def test_e4m3_values_are_the_formats():
    vals = W.e4m3_values()
    assert vals.numel() == 127 and bool((vals[1:] > vals[:-1]).all())
    assert float(vals[0]) == 0.0 and float(vals[1]) == 2.0 ** -9
    assert float(vals[8]) == 2.0 ** -6 and float(vals[126]) == W.E4M3_MAX
    # decoding is the inverse on the codes themselves
    enc = W.e4m3_encode(torch.cat([vals, -vals]).float())
    assert enc.tolist() == list(range(127)) + [128 + c for c in range(127)]


def test_encoder_agrees_with_the_reference_on_every_bf16_pattern():
    """Unscaled: torch's cast (overflow above 464 -> NaN byte). Scaled:
    clamp to +-448, then the cast; every head of the exhaustive case sees
    all 65 536 patterns under its own reciprocal scale."""
    x = W.all_bf16()
    kc = torch.empty(0, dtype=torch.uint8)
    W.assert_same_bits(W.quant_unscaled(x), R._kv_quant_like(x, kc),
                       "unscaled")
    case = W.quant_case(True)
    assert case.k_inv.tolist() == torch.tensor(W.INV_SCALES).tolist()
    for rows, inv in zip(case.views(case.bufs), (case.k_inv, case.v_inv)):
        W.assert_same_bits(W.quant_scaled(rows, inv),
                           R._kv_quant_scaled(rows, inv), "scaled")


def test_encoder_edges():
    """The edges the random tests used to meet by luck, spelled out."""
    def enc(*vals):
        return W.e4m3_encode(torch.tensor(vals, dtype=torch.float32)).tolist()
    inf, nan = float("inf"), float("nan")
    assert enc(0.0, -0.0) == [0x00, 0x80]
    assert enc(448.0, 449.0, 464.0, -464.0) == [0x7E, 0x7E, 0x7E, 0xFE]
    assert enc(464.00003, 480.0, inf) == [0x7F] * 3
    assert [b & 0x7F for b in enc(nan, -inf, -1e30)] == [0x7F] * 3
    # subnormals: 2^-9 apart; halfway cases go to the even code
    assert enc(2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 7 * 2.0 ** -9) == \
        [0x01, 0x00, 0x02, 0x07]
    assert enc(2.0 ** -10 * 1.0001, 15 * 2.0 ** -10) == [0x01, 0x08]
    # normals: 1.0 = 0x38, spacing 1/8; ties to even
    assert enc(1.0, 1.0625, 1.1875, 1.0626) == [0x38, 0x38, 0x3A, 0x39]
    # scaled path: +-inf saturate, NaN stays NaN
    one = torch.ones(1)
    x = torch.tensor([inf, -inf, nan, 1000.0]).view(4, 1, 1).bfloat16()
    got = W.quant_scaled(x, one).flatten().tolist()
    assert got[:2] == [0x7E, 0xFE] and got[2] & 0x7F == 0x7F
    assert got[3] == 0x7E


QUANT_MUTANTS = [
    ("truncate instead of round to nearest even", False,
     dict(ties="truncate")),
    ("round half away from zero", False, dict(ties="away")),
    ("flush e4m3 subnormals to zero", False, dict(flush_subnormals=True)),
    ("no clamp in the scaled path", True, dict(clamp="none")),
    ("NaN -> 0xfe (fminf / fmaxf clamp)", True, dict(clamp="minmax")),
]


@pytest.mark.parametrize("name,scaled,kw", QUANT_MUTANTS,
                         ids=[m[0] for m in QUANT_MUTANTS])
def test_quantizer_mutants_disagree_with_the_encoder(name, scaled, kw):
    case = W.quant_case(scaled)
    k, _v = case.views(case.bufs)
    if scaled:
        want = W.quant_scaled(k, case.k_inv)
        got = W.quant_scaled(k, case.k_inv, **kw)
    else:
        want, got = W.quant_unscaled(k), W.quant_unscaled(k, **kw)
    _killed(case.name, name, lambda: W.assert_same_bits(got, want, name))


def test_quant_case_layout():
    for scaled in (False, True):
        case = W.quant_case(scaled)
        k, v = case.views(case.bufs)
        assert k.shape == (512, 4, 128) and k.numel() == 262144
        assert torch.equal(W.bits(v), W.bits(k).roll(1, dims=0))
        assert sorted(case.slots.tolist()) == list(range(512))
        assert case.slots.tolist() != list(range(512))


# ----------------------------------------------------------------- scatter

@pytest.mark.parametrize("cfg", W.SCATTER_CONFIGS,
                         ids=_ids(W.SCATTER_CONFIGS))
def test_scatter_probes(cfg):
    case = W.scatter_case(**cfg)
    k, v = case.views(case.bufs)
    # the slot list the issue of each edge asks for
    slots = case.slots.tolist()
    assert len(set(slots)) == case.T == len(slots)
    assert case.nb * case.bs - 1 in slots
    if case.T >= 4:
        assert {0, case.bs - 1, case.bs} <= set(slots)
    assert slots != sorted(slots) or case.T == 1
    # ops/reference.py's store meets the whole-cache check
    kc, vc = case.caches()
    R.kv_cache_store(k, v, kc, vc, case.slots, **case.scale_kw())
    W.check_scatter(case, kc, vc, msg="reference")
    # T = 0 leaves the sentinel alone
    kc, vc = case.caches()
    R.kv_cache_store(k[:0], v[:0], kc, vc, case.slots[:0], **case.scale_kw())
    for c, s in zip((kc, vc), case.caches()):
        W.assert_same_bits(c, s, "empty store")
    # every mutant dies
    mutants = W.scatter_mutants(case)
    assert len(mutants) >= 5
    for name in mutants:
        mk, mv = case.expected(mutant=name)
        _killed(case.name, name, lambda: W.check_scatter(case, mk, mv))
    # ... and the stray write of zeros dies only because of the sentinel
    name = "zeros written to an untouched slot"
    for a, b in zip(case.expected(mutant=name, fill=0),
                    case.expected(fill=0)):
        W.assert_same_bits(a, b, "a zero-prefilled cache cannot see it")


def test_scatter_mutants_all_apply_somewhere():
    seen = set()
    for cfg in W.SCATTER_CONFIGS:
        seen.update(W.scatter_mutants(W.scatter_case(**cfg)))
    assert len(seen) == 8, sorted(seen)


# -------------------------------------------------------------------- RoPE

@pytest.mark.parametrize("cfg", W.ROPE_CONFIGS, ids=_ids(W.ROPE_CONFIGS))
def test_rope_probes(cfg):
    case = W.rope_case(**cfg)
    pos = case.pos.tolist()
    assert 299 in pos and max(pos) < W.ROPE_MAX_LEN
    if case.T > 1:
        assert 0 in pos and len(set(pos)) < len(pos)
    # cos = 1 and sin = 0 exactly at position 0
    assert bool((case.cos[0] == 1).all()) and bool((case.sin[0] == 0).all())
    # the reference, the model of the kernel and its fma-contracted variant
    # all stay inside the derived bound
    for name, bufs in (("reference", W.rope_reference(case)),
                       ("model", W.rope_model(case)),
                       ("fma model", W.rope_model(case, fma=True))):
        ratio = W.check_rope(case, bufs, msg=name)
        print(f"PASSED  {case.name:44s} {name:12s} worst error / bound "
              f"{ratio:.3f}")
        assert ratio <= 1.0
    for a, b in zip(W.rope_reference(case), W.rope_model(case)):
        assert torch.equal(W.bits(a), W.bits(b))
    mutants = W.rope_mutants(case)
    for name in mutants:
        bufs = W.rope_model(case, mutant=name)
        _killed(case.name, name, lambda: W.check_rope(case, bufs))
    # the case for the tighter bound: the old check lets truncation through
    W.old_rope_check(
        case, W.rope_model(case, mutant="bf16 store by truncation"))


def test_rope_checker_sees_a_write_outside_the_views():
    """One flipped bit in V, and one in the padding."""
    case = W.rope_case(**W.ROPE_CONFIGS[1])
    width = (case.nq + case.nkv) * case.hd
    for col in (width, case.bufs[0].shape[1] - 1):
        bufs = W.rope_reference(case)
        raw = bufs[0].view(torch.int16)  # a fresh copy, by its bits
        raw[case.T - 1, col] ^= 1
        _killed(case.name, f"bit flipped in column {col}",
                lambda: W.check_rope(case, bufs))


def test_rope_mutants_all_apply_somewhere():
    seen = set()
    for cfg in W.ROPE_CONFIGS:
        seen.update(W.rope_mutants(W.rope_case(**cfg)))
    assert len(seen) == 6, sorted(seen)


# ------------------------------------------------------------------- chain

@pytest.mark.parametrize("cfg", W.CHAIN_CONFIGS, ids=_ids(W.CHAIN_CONFIGS))
def test_chain_probes(cfg):
    case = W.chain_case(**cfg)
    bs = case.bs
    assert {bs - 1, bs, 2 * bs - 1, 2 * bs} <= set(case.pos.tolist())
    assert int(case.bt.min()) == 1
    assert case.bt.flatten().unique().numel() == case.bt.numel()
    slots = decode_slot_mapping(case.bt, case.pos, bs)
    assert slots.dtype == torch.int32 and slots.is_contiguous()
    # the ops chained as Runner._layer chains them (CPU: the reference)
    qkv = case.qkv.clone()
    q, k, v = case.views(qkv)
    kc, vc = case.caches()
    R.rope_inplace(q, k, case.pos.long(), case.cos, case.sin)
    R.kv_cache_store(k, v, kc, vc, slots, **case.scale_kw())
    W.check_chain(case, qkv, kc, vc, msg="reference")
    # and the one-call model says the same
    mq, mkc, mvc = W.write_path_model(case, case.qkv, case.pos, slots)
    assert torch.equal(W.bits(mq), W.bits(q))
    W.assert_same_bits(kc, mkc, "model K cache")
    W.assert_same_bits(vc, mvc, "model V cache")
    # a store that sees the unrotated K, and slots that ignore the table
    _q, bkc, bvc = W.write_path_model(case, case.qkv, case.pos, slots,
                                      mutant="store before rope")
    _killed(case.name, "store before rope",
            lambda: W.check_chain(case, qkv, bkc, bvc))
    ident = torch.arange(1, case.bt.numel() + 1, dtype=torch.int32).view_as(
        case.bt)
    _q, bkc, bvc = W.write_path_model(
        case, case.qkv, case.pos, decode_slot_mapping(ident, case.pos, bs))
    _killed(case.name, "slots from an unpermuted block table",
            lambda: W.check_chain(case, qkv, bkc, bvc))
