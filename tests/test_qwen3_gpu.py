"""Qwen3 on the MI355X: the fused per-head QK-norm + RoPE HIP kernel vs
reference.qk_norm_rope_inplace on identical bf16 inputs, and tiny-qwen3 /
tiny-qwen3-moe through the engine's HIP path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.engine.engine import InferenceEngine
from bee2bee_amd.ops import reference as R

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load
MAX_LEN = 256
EPS = 1e-6
GUARD = 3  # sentinel rows on each side of the live rows


def assert_close(a, b, atol=2e-2, rtol=2e-2, msg=""):
    """tests/test_ops_gpu.py's assert_close, same defaults."""
    a = a.float().cpu()
    b = b.float().cpu()
    diff = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = diff > tol
    assert not bool(bad.any()), (
        f"{msg}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; "
        f"max diff {float(diff.max()):.4f}"
    )


def _case(T, nq, nkv, hd):
    """One fused [GUARD + T + GUARD, q + 2kv] allocation: sentinel rows
    around the T live rows, per-head magnitudes spread ~100x, distinct
    random q/k weights, non-monotonic positions hitting 0 and MAX_LEN-1."""
    g = torch.Generator().manual_seed(1000 * hd + 10 * nq + T)
    heads = nq + 2 * nkv
    buf = torch.randn(T + 2 * GUARD, heads, hd, generator=g)
    buf *= torch.logspace(-1, 1, heads)[torch.randperm(heads, generator=g)][
        None, :, None]
    buf = buf.reshape(T + 2 * GUARD, heads * hd).bfloat16()
    qw = (1 + 0.3 * torch.randn(hd, generator=g)).bfloat16()
    kw = (1 + 0.3 * torch.randn(hd, generator=g)).bfloat16()
    pos = torch.tensor([MAX_LEN - 1, 0, 200, 3, 3, 77, 1, 255, 128][:T],
                       dtype=torch.int32)
    if T == 1:
        pos = torch.tensor([MAX_LEN - 1], dtype=torch.int32)
    return buf, qw, kw, pos


def _views(buf, T, nq, nkv, hd):
    live = buf[GUARD:GUARD + T]
    q, k, v = live.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
    return q.view(T, nq, hd), k.view(T, nkv, hd), v


SHAPES = [(4, 2, 16), (3, 1, 64), (5, 1, 128), (32, 8, 128), (2, 1, 256)]


@pytest.mark.parametrize("T", [1, 9])
@pytest.mark.parametrize("nq,nkv,hd", SHAPES)
def test_qk_norm_rope_kernel(nq, nkv, hd, T):
    buf_cpu, qw, kw, pos = _case(T, nq, nkv, hd)
    cos, sin = R.rope_tables(MAX_LEN, hd, 1000000.0, "cpu")

    # fp32-throughout reference on the identical bf16 values
    ref = buf_cpu.clone()
    rq, rk, _ = _views(ref, T, nq, nkv, hd)
    R.qk_norm_rope_inplace(rq, rk, pos, cos, sin, qw, kw, EPS)

    buf = buf_cpu.to(DEV)
    q, k, v = _views(buf, T, nq, nkv, hd)
    assert not q.is_contiguous() or T == 1
    dcos, dsin, dpos = cos.to(DEV), sin.to(DEV), pos.to(DEV)
    dqw, dkw = qw.to(DEV), kw.to(DEV)
    ops.qk_norm_rope_inplace(q, k, dpos, dcos, dsin, dqw, dkw, EPS)
    torch.cuda.synchronize()
    got = buf.cpu()

    msg = f"nq{nq} nkv{nkv} hd{hd} T{T}"
    gq, gk, gv = _views(got, T, nq, nkv, hd)
    assert_close(gq, rq, msg=msg + " q")
    assert_close(gk, rk, msg=msg + " k")
    # v slice and the guard rows: bit-identical
    assert torch.equal(gv, _views(buf_cpu, T, nq, nkv, hd)[2]), msg + " v"
    assert torch.equal(got[:GUARD], buf_cpu[:GUARD]), msg + " guard before"
    assert torch.equal(got[GUARD + T:], buf_cpu[GUARD + T:]), msg + " guard after"
    # the comparison tells the wrong variants apart: swapped q/k weights,
    # and a norm taken across the heads of a row, land outside it
    bad = buf_cpu.clone()
    bq, bk, _ = _views(bad, T, nq, nkv, hd)
    R.qk_norm_rope_inplace(bq, bk, pos, cos, sin, kw, qw, EPS)
    for got_t, bad_t in ((gq, bq), (gk, bk)):
        with pytest.raises(AssertionError):
            assert_close(got_t, bad_t)
    if nq > 1:
        x = _views(buf_cpu, T, nq, nkv, hd)[0].float()
        x = x * torch.rsqrt(x.pow(2).mean(dim=(-1, -2), keepdim=True) + EPS)
        x = x * qw.float()
        c = cos[pos.long()].unsqueeze(1)
        s = sin[pos.long()].unsqueeze(1)
        x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
        across = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
        with pytest.raises(AssertionError):
            assert_close(gq, across)


@pytest.mark.parametrize("nq,nkv,hd", [(5, 1, 128), (2, 1, 256)])
def test_qk_norm_rope_graph_capture_bit_identical(nq, nkv, hd):
    T = 9
    buf_cpu, qw, kw, pos = _case(T, nq, nkv, hd)
    cos, sin = R.rope_tables(MAX_LEN, hd, 1000000.0, DEV)
    dpos, dqw, dkw = pos.to(DEV), qw.to(DEV), kw.to(DEV)

    eager = buf_cpu.to(DEV)
    q, k, _ = _views(eager, T, nq, nkv, hd)
    ops.qk_norm_rope_inplace(q, k, dpos, cos, sin, dqw, dkw, EPS)

    static = buf_cpu.to(DEV)
    sq, sk, _ = _views(static, T, nq, nkv, hd)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):  # warm-up outside capture
        ops.qk_norm_rope_inplace(sq, sk, dpos, cos, sin, dqw, dkw, EPS)
    torch.cuda.current_stream().wait_stream(stream)
    static.copy_(buf_cpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.qk_norm_rope_inplace(sq, sk, dpos, cos, sin, dqw, dkw, EPS)
    for _ in range(2):  # in place: reset the input before every replay
        static.copy_(buf_cpu)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)


def test_qk_norm_rope_rejects_bad_arguments():
    T, nq, nkv = 2, 2, 1
    cos, sin = R.rope_tables(MAX_LEN, 16, 1e6, DEV)
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)

    def call(hd=16, wdtype=torch.bfloat16, wlen=None, cs=None, p=pos):
        q = torch.zeros(T, nq, hd, device=DEV, dtype=torch.bfloat16)
        k = torch.zeros(T, nkv, hd, device=DEV, dtype=torch.bfloat16)
        w = torch.ones(wlen or hd, device=DEV, dtype=wdtype)
        c, s = cs or R.rope_tables(MAX_LEN, hd, 1e6, DEV)
        ops.qk_norm_rope_inplace(q, k, p, c, s, w, w.clone(), EPS)

    call()  # the baseline is accepted
    with pytest.raises(RuntimeError):
        call(hd=512)  # head_dim > 256
    with pytest.raises(RuntimeError):
        call(wdtype=torch.float32)
    with pytest.raises(RuntimeError):
        call(wlen=32)
    with pytest.raises(RuntimeError):
        call(hd=64, cs=(cos, sin))  # tables built for another head_dim
    with pytest.raises(RuntimeError):
        call(p=pos.long())
    with pytest.raises(RuntimeError):
        q = torch.zeros(T, nq, 16, device=DEV, dtype=torch.bfloat16)
        k = torch.zeros(T, nkv, 16, device=DEV, dtype=torch.bfloat16)
        w = torch.ones(32, device=DEV, dtype=torch.bfloat16)[::2]
        ops.qk_norm_rope_inplace(q, k, pos, cos, sin, w, w, EPS)


# ---------------------------------------------------------------- engine

PROMPT = [(i * 7 + 3) % 500 + 4 for i in range(40)]


def _engine(model, **kw):
    return InferenceEngine(model, device=DEV, max_batch=2, max_seq_len=128,
                           seed=7, **kw)


def _graph_vs_eager(model, **kw):
    outs = {}
    for graphs in (True, False):
        eng = _engine(model, use_graphs=graphs, **kw)
        try:
            assert (eng.graphs is not None) == graphs
            assert eng.weights.layers[0].q_norm is not None
            if kw.get("kv_dtype") == "fp8":
                eng.calibrate_kv_scales([PROMPT, PROMPT[::-1]])
                assert eng.stats()["kv_scales"] == "calibrated"
                assert bool((eng.kv.k_scale != 1.0).all())
            req = eng.generate(PROMPT, max_new_tokens=12, temperature=0.0,
                               repetition_penalty=1.0)
            assert req.error is None, req.error
            assert len(req.output_ids) == 12
            outs[graphs] = req.output_ids
        finally:
            eng.shutdown()
    assert outs[True] == outs[False], outs
    return outs[True]


def test_tiny_qwen3_graph_matches_eager():
    _graph_vs_eager("tiny-qwen3")


def test_tiny_qwen3_fp8_kv_calibrated_graph_matches_eager():
    """fp8 KV: calibration observes post-norm, post-RoPE K through the new
    call site, then chunked prefill + decode with graphs on and off."""
    _graph_vs_eager("tiny-qwen3", kv_dtype="fp8", max_prefill_tokens=16)


def test_tiny_qwen3_moe_graph_matches_eager():
    _graph_vs_eager("tiny-qwen3-moe")


def _prefill_logits(runner, kv, ids, seq_id):
    dev = runner.device
    T = len(ids)
    kv.new_seq(seq_id)
    kv.extend_seq(seq_id, T)
    slots = torch.tensor(kv.slot_mapping(seq_id, range(T)),
                         dtype=torch.int32, device=dev)
    hidden = runner.forward_prefill(
        torch.tensor(ids, dtype=torch.int64, device=dev),
        torch.arange(T, dtype=torch.int32, device=dev), slots,
        torch.tensor([0, T], dtype=torch.int32, device=dev), T,
    )
    kv.free_seq(seq_id)
    return runner.lm_head(hidden).float().cpu()


def _cpu_fp32_copy(weights):
    """The same (bf16-valued) weights as fp32 tensors on the CPU."""
    from bee2bee_amd.models.weights import ModelWeights

    cpu = ModelWeights(weights.spec, torch.device("cpu"), torch.float32)
    for name in ("embed", "final_norm", "lm_head"):
        setattr(cpu, name, getattr(weights, name).float().cpu())
    for a, b in zip(weights.layers, cpu.layers):
        for slot in type(a).__slots__:
            t = getattr(a, slot)
            setattr(b, slot, None if t is None else t.float().cpu())
    return cpu


@pytest.mark.parametrize("kv_dtype", ["native", "fp8"])
def test_tiny_qwen3_prefill_logits_vs_cpu_fp32_reference(kv_dtype):
    """HIP bf16 stack vs the CPU fp32 reference runner on the same weights,
    held to tests/test_engine_gpu.py::test_hip_vs_reference_logits' bound
    (argmax agreement >= 0.99, max drift < 8% of the logit scale). With fp8
    KV the engine is calibrated first (through the new call site); the
    whole-prompt prefill attends the fresh bf16 K/V, so the bound is the
    same."""
    from bee2bee_amd.engine.kv import PagedKV
    from bee2bee_amd.engine.runner import Runner

    ids = [5, 17, 99, 345, 6, 88, 250, 44]
    eng = _engine("tiny-qwen3", kv_dtype=kv_dtype)
    try:
        if kv_dtype == "fp8":
            eng.calibrate_kv_scales([PROMPT])
            assert eng.stats()["kv_scales"] == "calibrated"
        hip = _prefill_logits(eng.runner, eng.kv, ids, seq_id=10_000)
        cpu_w = _cpu_fp32_copy(eng.weights)
    finally:
        eng.shutdown()
    cpu = torch.device("cpu")
    kv = PagedKV(cpu_w.spec, cpu, torch.float32, n_blocks=8)
    ref = _prefill_logits(Runner(cpu_w.spec, cpu_w, kv, cpu, torch.float32),
                          kv, ids, seq_id=0)
    agree = (hip.argmax(-1) == ref.argmax(-1)).float().mean()
    diff = (hip - ref).abs().max()
    scale = ref.abs().max()
    print(f"kv={kv_dtype} argmax agreement {agree} drift {diff / scale}")
    assert agree >= 0.99, f"argmax agreement {agree}"
    assert diff / scale < 0.08, f"relative logit drift {diff / scale}"
