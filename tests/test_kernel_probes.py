"""Standing proof that the probe cases of tests/kernel_probes.py have power
(CPU only). For every case the builders produce:

  * a reference that emulates the kernels' rounding (q * scale in the MFMA
    input type, p stored as bf16 before PV, outputs stored as bf16) passes
    the checker against the exact reference: the inputs leave the kernels
    room at the existing tolerances;
  * every applicable mutant (a wrong reference in plain torch) makes the
    checker raise. No mutant may survive and there is no waiver list: a
    survivor means the inputs are wrong.

`pytest -s` prints one line per mutant with the case that kills it.
"""
import pytest
import torch

from bee2bee_amd.ops import reference as R
from tests import kernel_probes as P


def _ids(configs):
    return ["-".join(f"{k}{v}" for k, v in c.items()) for c in configs]


def _killed(case_name, mutant, fn):
    """The checker must raise on the mutant's output."""
    try:
        fn()
    except AssertionError as e:
        print(f"KILLED  {case_name:44s} {mutant:32s} "
              f"{str(e).split(': ', 1)[-1][:60]}")
        return
    pytest.fail(f"mutant survived: {case_name}: {mutant}")


def _attn(case):
    # the model the mutants are cut from is the reference's operation
    out, ml = P.attn_model(case)
    r_out, r_ml = P.attn_exact(case)
    assert torch.allclose(out, r_out, atol=1e-4, rtol=1e-4), case.name
    if r_ml is not None:
        assert torch.allclose(ml, r_ml, atol=1e-4, rtol=1e-4), case.name
    # every must-see probe carries the weight the builder promised
    assert case.weights or not any(s.see for s in case.seqs)
    assert all(w >= P.MIN_PROBE_WEIGHT for _i, _p, w in case.weights)
    # room for the kernels' rounding
    out, ml = P.attn_model(case, emulate=True)
    P.check_attn(case, out, ml, msg="rounding-emulating reference")
    # every mutant dies; a probe's mutant on the one sequence it changes
    mutants = P.attn_mutants(case)
    assert mutants
    for name, i, kw in mutants:
        seqs = None if i is None else [i]
        out, ml = P.attn_model(case, seqs=seqs, emulate=True, **kw)
        _killed(case.name, name if i is None else f"seq {i}: {name}",
                lambda: P.check_attn(case, out, ml, seqs=seqs))


@pytest.mark.parametrize("cfg", P.DECODE_CONFIGS + P.DECODE_GENERIC_CONFIGS,
                         ids=_ids(P.DECODE_CONFIGS + P.DECODE_GENERIC_CONFIGS))
def test_decode_probes(cfg):
    _attn(P.decode_case(**cfg))


@pytest.mark.parametrize("cfg", P.PREFILL_CONFIGS, ids=_ids(P.PREFILL_CONFIGS))
def test_prefill_probes(cfg):
    _attn(P.prefill_case(**cfg))


@pytest.mark.parametrize("cfg", P.PAGED_CONFIGS, ids=_ids(P.PAGED_CONFIGS))
def test_paged_prefill_probes(cfg):
    _attn(P.paged_case(**cfg))


def test_decode_positions_are_the_listed_ones():
    """Page 0 unused, a permuted table, one sequence per position."""
    case = P.decode_case()
    assert [s.see[0] for s in case.seqs[:10]] == \
        [0, 31, 32, 63, 64, 255, 256, 511, 512, 599]
    assert [s.L for s in case.seqs] == [600] * 10 + [1, 256, 257]
    assert all(s.hide == (s.L,) for s in case.seqs)
    assert int(case.bt.min()) == 1
    assert case.bt.flatten().unique().numel() == case.bt.numel()
    assert not torch.equal(case.bt.flatten().sort().values, case.bt.flatten())
    big = P.decode_case(bs=256)
    assert {s.L for s in big.seqs} == {1025} and big.bs == 256
    for w in (256, 300):
        los = [s.L - w for s in P.decode_case(window=w).seqs[:3]]
        assert los[0] % 32 and los[1] % 256 == 0
        assert los[2] % 32 == 0 and los[2] % 256


@pytest.mark.parametrize("op,H,spike_in", P.norm_configs())
def test_norm_spikes(op, H, spike_in):
    case = P.norm_case(op, H, spike_in)
    exact, model = P.norm_exact(case), P.norm_model(case)
    for a, b in zip(*((exact, model) if case.resid is not None
                      else ((exact,), (model,)))):
        assert torch.allclose(a, b, atol=1e-4, rtol=1e-4), case.name
    P.check_norm(case, P.norm_model(case, emulate=True),
                 msg="rounding-emulating reference")
    for mutant in P.norm_mutants(case):
        got = P.norm_model(case, mutant, emulate=True)
        _killed(case.name, mutant, lambda: P.check_norm(case, got))


@pytest.mark.parametrize("hd", P.QKN_HD)
def test_qk_norm_spikes(hd):
    case = P.qk_norm_case(hd)
    for a, b in zip(P.qk_norm_exact(case), P.qk_norm_model(case)):
        assert torch.allclose(a, b, atol=1e-4, rtol=1e-4), case.name
    P.check_qk_norm(case, P.qk_norm_model(case, emulate=True),
                    msg="rounding-emulating reference")
    for mutant in P.qk_norm_mutants(case):
        got = P.qk_norm_model(case, mutant, emulate=True)
        _killed(case.name, mutant, lambda: P.check_qk_norm(case, got))


def test_divide_mutant_applicability():
    """Dividing by H - 8 is a uniform relative error of sqrt(H / (H - 8)) - 1;
    it is a mutant only where that exceeds the relative tolerance."""
    assert [H for H in P.NORM_H if P.divide_mutant_applies(H)] == [8, 64]
    assert [h for h in P.QKN_HD if P.divide_mutant_applies(h)] == [64, 128]


@pytest.mark.parametrize("K", P.GEMM_ONEHOT_K)
def test_grouped_gemm_onehot(K):
    case = P.gemm_onehot_case(K)
    assert {k // P.GEMM_KG for k in case.hot} == set(range(K // P.GEMM_KG))
    P.check_gemm(case, P.gemm_model(case, emulate=True))
    for mutant, g in P.gemm_mutants(case):
        got = P.gemm_model(case, mutant, g, emulate=True)
        _killed(case.name, f"{mutant} (group {g})",
                lambda: P.check_gemm(case, got))


def test_grouped_gemm_segments():
    case = P.gemm_segment_case()
    sizes = (case.offs[1:] - case.offs[:-1]).tolist()
    assert [n for n in sizes if n] == list(P.GEMM_SEGMENTS)
    assert sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1]
    ref = R.grouped_gemm(case.x.float(), case.w.float(), case.offs)
    assert torch.allclose(P.gemm_model(case), ref, atol=1e-4, rtol=1e-4)
    P.check_gemm(case, P.gemm_model(case, emulate=True))
    for mutant, g in P.gemm_mutants(case):
        got = P.gemm_model(case, mutant, g, emulate=True)
        _killed(case.name, f"{mutant} (group {g})",
                lambda: P.check_gemm(case, got))


# ----------------------------------------- what the randn inputs cannot see

def _old_assert_close(a, b, atol=2e-2, rtol=2e-2):
    """tests/test_ops_gpu.py's assert_close."""
    diff = (a.float() - b.float()).abs()
    assert not bool((diff > atol + rtol * b.float().abs()).any()), \
        f"max diff {float(diff.max()):.4f}"


def test_randn_inputs_pass_a_dropped_newest_key():
    """test_attn_decode_long_context's inputs (L = 2048) accept a decode
    that drops the newest key; the probe case does not."""
    torch.manual_seed(8)
    B, nkv, G, hd, bs, L = 2, 4, 4, 128, 32, 2048
    W = L // bs
    bt = torch.arange(1, B * W + 1).reshape(B, W).to(torch.int32)
    kc = torch.randn(B * W + 1, nkv, bs, hd).bfloat16()
    vc = torch.randn(B * W + 1, nkv, bs, hd).bfloat16()
    q = torch.randn(B, nkv * G, hd).bfloat16()
    lens = torch.tensor([L, L - 17], dtype=torch.int32)
    ref = R.attn_decode(q, kc, vc, bt, lens, hd ** -0.5)
    mutant = R.attn_decode(q, kc, vc, bt, lens - 1, hd ** -0.5)
    _old_assert_close(mutant, ref)  # passes: the old inputs are blind
    err = float((mutant.float() - ref.float()).abs().max())
    print(f"dropped newest key, randn L=2048: max error {err:.4f} < 0.02")
    case = P.decode_case()
    i = [s.see[0] for s in case.seqs].index(599)
    name, _i, kw = [m for m in P.attn_mutants(case)
                    if m[1] == i and m[0] == "drop key 599"][0]
    out, ml = P.attn_model(case, seqs=[i], emulate=True, **kw)
    with pytest.raises(AssertionError):
        P.check_attn(case, out, ml, seqs=[i])


@pytest.mark.parametrize("tail", [8, 64])
def test_randn_inputs_pass_an_rmsnorm_that_omits_the_tail(tail):
    """test_rmsnorm's 7 x 4096 inputs accept a sum of squares without the
    row's last 8 or 64 elements; the spike at H - 1 does not."""
    torch.manual_seed(1)
    x = torch.randn(7, 4096).bfloat16()
    w = torch.randn(4096).bfloat16()
    ref = R.rmsnorm(x, w, 1e-5)
    xf = x.float()
    ms = xf[:, :-tail].pow(2).sum(-1, keepdim=True) / 4096
    mutant = (xf * torch.rsqrt(ms + 1e-5) * w.float()).bfloat16()
    _old_assert_close(mutant, ref)  # passes: the old inputs are blind
    case = P.norm_case("rmsnorm", 4096)
    t = case.spikes.index(4095)
    v = case.x.float()
    ms = v[:, :-tail].pow(2).sum(-1, keepdim=True) / 4096
    got = (v * torch.rsqrt(ms + P.EPS) * case.w.float()).bfloat16()
    with pytest.raises(AssertionError):
        P.assert_close(got[t], P.norm_exact(case)[t],
                       atol=P.TOL_ELEMENTWISE, rtol=P.TOL_ELEMENTWISE)
