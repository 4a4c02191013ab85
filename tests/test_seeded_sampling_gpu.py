"""Seeded sampling on the GPU engine: with fused_sampler every request of a
mixed batch samples through one ops.sample_rows launch per step and equals
its solo run; with the option off and no seed the old path runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.engine.engine import GenerationRequest, InferenceEngine
from bee2bee_amd.engine.sampler import SamplingParams

# eight requests of mixed parameters: greedy, penalties, top_k 1..1024
_MIX = [
    dict(temperature=0.8, seed=11),
    dict(temperature=0.0, repetition_penalty=1.0, seed=12),
    dict(temperature=1.2, top_k=8, seed=13),
    dict(temperature=0.7, top_p=0.5, repetition_penalty=1.3, seed=14),
    dict(temperature=1.0, top_k=1024, repetition_penalty=1.0, seed=15),
    dict(temperature=0.0, seed=16),
    dict(temperature=0.9, top_k=200, seed=17),
    dict(temperature=0.6, top_k=3, repetition_penalty=1.0, seed=18),
]


def _engine(**kw):
    return InferenceEngine("tiny", device="cuda:0", max_batch=8,
                           max_seq_len=128, seed=7, **kw)


def _req(i, knobs, n=16):
    k = dict(knobs)
    return GenerationRequest(
        prompt_ids=[9 + i, 4, 6, 20 + 3 * i] * (1 + i % 3), max_new_tokens=n,
        sampling=SamplingParams.from_request(
            k.pop("temperature"), k.pop("top_p", None), k.pop("top_k", None),
            k.pop("repetition_penalty", None), k.pop("seed", None)))


def _drain(req):
    while isinstance(req.out_queue.get(timeout=120), int):
        pass
    assert req.error is None, req.error
    return list(req.output_ids)


def test_fused_mixed_batch_equals_solo_runs(monkeypatch):
    calls = []
    real = ops.sample_rows

    def counting(logits, *a, **k):
        calls.append(logits.shape[0])
        return real(logits, *a, **k)

    monkeypatch.setattr(ops, "sample_rows", counting)
    eng = _engine(fused_sampler=True)
    try:
        solo = [_drain(eng.submit(_req(i, k))) for i, k in enumerate(_MIX)]
        assert all(len(s) == 16 for s in solo)
        calls.clear()
        reqs = [eng.submit(_req(i, k)) for i, k in enumerate(_MIX)]
        mixed = [_drain(r) for r in reqs]
        assert mixed == solo
        # the mix shared launches: some call sampled several rows at once
        assert max(calls) > 1, calls
        # the sampled rows are not all greedy
        assert solo[0] != solo[5] or solo[2] != solo[5]
    finally:
        eng.shutdown()


def test_default_path_never_calls_sample_rows(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("ops.sample_rows called on the default path")

    monkeypatch.setattr(ops, "sample_rows", boom)
    monkeypatch.delenv("BEE2BEE_FUSED_SAMPLER", raising=False)
    eng = _engine()
    try:
        assert not eng.fused_sampler
        reqs = [eng.submit(_req(i, {k: v for k, v in knobs.items()
                                    if k != "seed"}, n=6))
                for i, knobs in enumerate(_MIX)]
        assert all(len(_drain(r)) == 6 for r in reqs)
    finally:
        eng.shutdown()


def test_engine_rows_match_the_reference_sampler():
    """One fused step's tokens, recomputed on the CPU from the same logits:
    greedy rows exactly, sampled rows within the float64 acceptance."""
    from tests import sampler_probes as P

    g = torch.Generator().manual_seed(5)
    x = (torch.randn(8, 512, generator=g) * 3).bfloat16()
    kw = dict(T=[1.0, 0.8, 1.2, 0.7, 1.0, 1.0, 0.9, 0.6],
              k=[1, 64, 8, 64, 512, 1, 200, 3],
              p=[1.0, 0.95, 0.95, 0.5, 0.95, 1.0, 0.95, 0.95],
              seed=list(range(8)), pos=4)
    got = P.run(ops.sample_rows, x.to("cuda:0"), **kw)
    P.check_accepted(got, P.accept_sets(x, **kw), "engine-shaped batch")
