"""The sampler's probe cases through the HIP kernel (ops.sample_rows on
the GPU): the cases of tests/sampler_probes.py on bf16 and fp32 logits, one
full-vocabulary random case, the calls the binding refuses, and run-to-run
determinism."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.ops import reference as R
from tests import sampler_probes as P

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", [n for n in P.CASES if n != "philox"])
def test_kernel_passes(name, dtype):
    P.CASES[name](ops.sample_rows, DEV, dtype)


def test_full_vocabulary_random_rows():
    """[64, 152064] bf16 under the random rows' acceptance rule."""
    x, kw, acc = P.random_inputs(152064, 64, 3.0, 0.7, 0.95, rows=64)
    got = P.run(ops.sample_rows, x.to(DEV), **kw)
    P.check_accepted(got, acc, "random_152064_k64")


def test_kernel_agrees_with_reference_on_mixed_batch():
    """The 16-row, 6-parameter-set batch: every row the kernel samples is
    one the float64 evaluation accepts, and greedy rows are exact."""
    x, pool, kw = P._mixed_inputs()
    acc = P.accept_sets(x, pool=pool, **kw)
    got = P.run(ops.sample_rows, x.to(DEV).bfloat16(), pool=pool.to(DEV),
                **kw)
    P.check_accepted(got, acc, "mixed batch")
    ref = P.run(R.sample_rows, x, pool=pool, **kw)
    greedy = [r for r, k in enumerate(kw["k"]) if k == 1]
    assert got[greedy].tolist() == ref[greedy].tolist()


def test_two_launches_are_identical():
    x, kw, _ = P.random_inputs(*P.RANDOM_SHAPES["random_8192_k1024"])
    xd = x.to(DEV)
    a = P.run(ops.sample_rows, xd, **kw)
    b = P.run(ops.sample_rows, xd, **kw)
    assert torch.equal(a, b)


def _args(B=4, V=512, dtype=torch.bfloat16, device=DEV):
    x = torch.zeros(B, V, dtype=dtype, device=device)
    q = P.params(B, device)
    return [x, q["temperature"], q["top_k"], q["top_p"], q["penalty"], None,
            q["seen_slot"], q["seed"], q["pos"]]


def test_refused_calls():
    hip = ops.require_hip()
    hip.sample_rows(*_args())                       # the good call
    # wrong dtype: logits, then each parameter
    a = _args()
    a[0] = a[0].half()
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        hip.sample_rows(*a)
    for i, bad in ((1, torch.float64), (2, torch.int64), (3, torch.bfloat16),
                   (4, torch.float64), (6, torch.int64), (7, torch.int32),
                   (8, torch.int64)):
        a = _args()
        a[i] = a[i].to(bad)
        with pytest.raises(RuntimeError, match="sample_rows"):
            hip.sample_rows(*a)
    # wrong device: CPU logits, then a CPU parameter
    a = _args()
    a[0] = a[0].cpu()
    with pytest.raises(RuntimeError, match="GPU"):
        hip.sample_rows(*a)
    a = _args()
    a[7] = a[7].cpu()
    with pytest.raises(RuntimeError, match="sample_rows"):
        hip.sample_rows(*a)
    # wrong shape: 3-d logits, a parameter of another length, a pool of
    # another width, a 2-d parameter
    a = _args()
    a[0] = a[0][None]
    with pytest.raises(RuntimeError, match=r"\[B, V\]"):
        hip.sample_rows(*a)
    a = _args()
    a[2] = a[2][:3]
    with pytest.raises(RuntimeError, match="sample_rows"):
        hip.sample_rows(*a)
    a = _args()
    a[5] = torch.zeros(2, 511, dtype=torch.bool, device=DEV)
    with pytest.raises(RuntimeError, match="seen_pool"):
        hip.sample_rows(*a)
    a = _args()
    a[5] = torch.zeros(2, 512, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="seen_pool"):
        hip.sample_rows(*a)
    a = _args()
    a[1] = a[1][:, None]
    with pytest.raises(RuntimeError, match="sample_rows"):
        hip.sample_rows(*a)
    # a non-contiguous last dimension
    a = _args()
    a[0] = torch.zeros(4, 1024, dtype=torch.bfloat16, device=DEV)[:, ::2]
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.sample_rows(*a)
    # a strided parameter
    a = _args()
    a[1] = torch.ones(8, dtype=torch.float32, device=DEV)[::2]
    with pytest.raises(RuntimeError, match="sample_rows"):
        hip.sample_rows(*a)


def test_out_of_range_values_are_clamped():
    """top_k and seen_slot cannot be checked without a sync: the kernel
    clamps them (a slot past the pool reads as none)."""
    x, kw, _ = P.random_inputs(*P.RANDOM_SHAPES["random_4096_k64"])
    xd = x[:8].to(DEV)
    kw = {k: (v[:8] if isinstance(v, list) else v) for k, v in kw.items()}
    pool = torch.ones(2, xd.shape[1], dtype=torch.bool, device=DEV)
    base = P.run(ops.sample_rows, xd, **dict(kw, k=1024))
    assert torch.equal(P.run(ops.sample_rows, xd, **dict(kw, k=10 ** 6)),
                       base)
    assert torch.equal(
        P.run(ops.sample_rows, xd, pool=pool, pen=1.5, slot=2,
              **dict(kw, k=1024)), base)
    assert torch.equal(P.run(ops.sample_rows, xd, **dict(kw, k=-3)),
                       P.run(ops.sample_rows, xd, **dict(kw, k=1)))


def test_graph_capture():
    """No sync and no allocation beyond the output: the launch captures
    into a graph, and a replay follows pos on the device."""
    x, kw, _ = P.random_inputs(*P.RANDOM_SHAPES["random_4096_k64"])
    xd = x.to(DEV)
    q = P.params(xd.shape[0], DEV, **kw)
    args = (xd, q["temperature"], q["top_k"], q["top_p"], q["penalty"], None,
            q["seen_slot"], q["seed"], q["pos"])
    eager0 = ops.sample_rows(*args).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sample_rows(*args)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.sample_rows(*args)
    g.replay()
    assert torch.equal(out, eager0)
    q["pos"].add_(1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.sample_rows(*args))
    assert not torch.equal(out, eager0)
