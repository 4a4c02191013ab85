"""The sampler's probe cases on the CPU: ops.reference.sample_rows passes
every case of tests/sampler_probes.py, and every mutant fails one."""
import pytest
import torch

from bee2bee_amd import ops
from bee2bee_amd.ops import reference as R
from tests import sampler_probes as P


def test_philox_known_answers():
    P.case_philox(None, "cpu", None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", [n for n in P.CASES if n != "philox"])
def test_reference_passes(name, dtype):
    P.CASES[name](R.sample_rows, "cpu", dtype)


def test_dispatch_takes_the_reference_on_cpu():
    P.CASES["penalty"](ops.sample_rows, "cpu", torch.float32)


@pytest.mark.parametrize("name", list(P.MUTANTS))
def test_mutant_fails(name):
    fn, cases = P.MUTANTS[name]
    caught = []
    for c in cases:
        try:
            P.CASES[c](fn, "cpu", torch.bfloat16)
        except AssertionError:
            caught.append(c)
    assert caught, f"mutant {name} passed {cases}"


@pytest.mark.parametrize("name", list(P.RANDOM_SHAPES))
def test_random_rows_are_rarely_ambiguous(name):
    """At most 5 % of a case's rows may accept more than one token, from
    the reference alone (random_inputs asserts it); no row is skipped."""
    x, kw, acc = P.random_inputs(*P.RANDOM_SHAPES[name])
    assert len(acc) == P.RANDOM_ROWS == x.shape[0]
    assert all(len(a) >= 1 for a in acc)
    many = sum(len(a) > 1 for a in acc)
    print(f"{name}: {many} of {len(acc)} rows accept more than one token")
    assert many <= P.MAX_AMBIGUOUS * len(acc)


def test_greedy_is_argmax_lowest_index():
    x = torch.tensor([[1.0, 3.0, 3.0, -2.0], [0.0, 0.0, 0.0, 0.0]])
    assert P.run(R.sample_rows, x, T=1.0, k=1).tolist() == [1, 0]


def test_top_k_is_clamped():
    x = torch.randn(4, 2000, generator=torch.Generator().manual_seed(0))
    kw = dict(T=1.0, p=1.0, seed=[1, 2, 3, 4], pos=9)
    assert P.run(R.sample_rows, x, k=0, **kw).tolist() == \
        P.run(R.sample_rows, x, k=1, **kw).tolist()
    assert P.run(R.sample_rows, x, k=5000, **kw).tolist() == \
        P.run(R.sample_rows, x, k=1024, **kw).tolist()
