"""The probe cases of tests/kernel_probes.py through the HIP kernels, against
ops/reference.py at the suite's existing tolerances. Each case is one batch
with one sequence (row, token) per probed position, so one launch covers
every edge of a configuration; tests/test_kernel_probes.py proves on the CPU
that a kernel which drops or leaks one key, row or element fails here.

Also: the grid-stride second trip of swiglu / gelu, and the calls the
bindings reject before any launch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.ops import reference as R
from tests import kernel_probes as P

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load


def _ids(configs):
    return ["-".join(f"{k}{v}" for k, v in c.items()) for c in configs]


def _dev(case):
    """The case's tensors on the GPU, uploaded once."""
    if not hasattr(case, "_dev"):
        d = {n: getattr(case, n).to(DEV)
             for n in ("q", "k", "v", "kc", "vc", "bt")
             if getattr(case, n) is not None}
        d["lens"] = torch.tensor(case.lens, dtype=torch.int32, device=DEV)
        d["cu"] = torch.tensor(case.cu, dtype=torch.int32, device=DEV)
        d["kw"] = {k: (v.to(DEV) if torch.is_tensor(v) else v)
                   for k, v in case.kw().items()}
        case._dev = d
    return case._dev


# ------------------------------------------------------------------- decode

def _decode(case, path, max_z):
    d = _dev(case)
    out, ml = ops.attn_decode_select(d["q"], d["kc"], d["vc"], d["bt"],
                                     d["lens"], case.scale, path=path,
                                     max_z=max_z, **d["kw"])
    return out, ml


@pytest.mark.parametrize("max_z", [1, 0])
@pytest.mark.parametrize("cfg", P.DECODE_CONFIGS, ids=_ids(P.DECODE_CONFIGS))
def test_decode_probes(cfg, max_z):
    """Fused and split (head_dim 64 / 128): bit-identical to each other, and
    every probe position right. max_z=1 forces the FOLD kernels, max_z=0
    leaves partials + combine."""
    case = P.decode_case(**cfg)
    f_out, f_ml = _decode(case, "fused", max_z)
    s_out, s_ml = _decode(case, "split", max_z)
    msg = f"max_z={max_z}"
    P.check_attn(case, f_out.cpu(), f_ml.cpu(), msg=f"fused {msg}")
    P.check_attn(case, s_out.cpu(), s_ml.cpu(), msg=f"split {msg}")
    assert torch.equal(f_out, s_out), (
        f"{case.name} {msg}: fused out != split out, "
        f"{int((f_out != s_out).sum())}/{f_out.numel()} differ")
    assert torch.equal(f_ml, s_ml), \
        f"{case.name} {msg}: fused (m, l) != split (m, l)"


@pytest.mark.parametrize("max_z", [1, 0])
@pytest.mark.parametrize("cfg", P.DECODE_GENERIC_CONFIGS,
                         ids=_ids(P.DECODE_GENERIC_CONFIGS))
def test_decode_probes_generic_head_dims(cfg, max_z):
    case = P.decode_case(**cfg)
    out, ml = _decode(case, "auto", max_z)
    P.check_attn(case, out.cpu(), ml.cpu(), msg=f"auto max_z={max_z}")


def test_decode_probes_serving_entry_point():
    """ops.attn_decode (what the engine calls) on the base case."""
    case = P.decode_case()
    d = _dev(case)
    out, ml = ops.attn_decode_lse(d["q"], d["kc"], d["vc"], d["bt"],
                                  d["lens"], case.scale)
    P.check_attn(case, out.cpu(), ml.cpu(), msg="attn_decode_lse")
    plain = ops.attn_decode(d["q"], d["kc"], d["vc"], d["bt"], d["lens"],
                            case.scale)
    assert torch.equal(plain, out)


# ------------------------------------------------------------------ prefill

@pytest.mark.parametrize("cfg", P.PREFILL_CONFIGS, ids=_ids(P.PREFILL_CONFIGS))
def test_prefill_probes(cfg):
    """The causal edge at row p, inside and across 64-row tiles; with a
    window also the band's lower edge; one non-causal case (basic kernel at
    head_dim 128)."""
    case = P.prefill_case(**cfg)
    d = _dev(case)
    out = ops.attn_prefill(d["q"], d["k"], d["v"], d["cu"], max(case.lens),
                           case.scale, case.causal, window=case.window)
    P.check_attn(case, out.cpu())


@pytest.mark.parametrize("cfg", P.PAGED_CONFIGS, ids=_ids(P.PAGED_CONFIGS))
def test_paged_prefill_probes(cfg):
    case = P.paged_case(**cfg)
    d = _dev(case)
    out = ops.attn_prefill_paged(d["q"], d["kc"], d["vc"], d["bt"],
                                 d["lens"], d["cu"],
                                 max(s.QL for s in case.seqs), case.scale,
                                 **d["kw"])
    P.check_attn(case, out.cpu())


# ----------------------------------------------------------- row reductions

@pytest.mark.parametrize("op,H,spike_in", P.norm_configs())
def test_norm_spikes(op, H, spike_in):
    case = P.norm_case(op, H, spike_in)
    x, w = case.x.to(DEV), case.w.to(DEV)
    if op == "rmsnorm":
        got = ops.rmsnorm(x, w, P.EPS)
    elif op == "fused_add_rmsnorm":
        got = ops.fused_add_rmsnorm(x, case.resid.to(DEV), w, P.EPS)
    elif op == "layernorm":
        got = ops.layernorm(x, w, case.b.to(DEV), P.EPS)
    else:
        got = ops.fused_add_layernorm(x, case.resid.to(DEV), w,
                                      case.b.to(DEV), P.EPS)
    P.check_norm(case, got)


@pytest.mark.parametrize("hd", P.QKN_HD)
def test_qk_norm_spikes(hd):
    case = P.qk_norm_case(hd)
    q, k = case.q.to(DEV), case.k.to(DEV)
    ops.qk_norm_rope_inplace(q, k, case.pos.to(DEV), case.cos.to(DEV),
                             case.sin.to(DEV), case.qw.to(DEV),
                             case.kw.to(DEV), P.EPS)
    P.check_qk_norm(case, (q, k))


# ------------------------------------------------------------- grouped GEMM

@pytest.mark.parametrize("K", P.GEMM_ONEHOT_K)
def test_grouped_gemm_onehot(K):
    """Each K position consumed exactly once: a one-hot row gives its column
    of w bit for bit. K=384 is the main loop followed by the 2-group tail."""
    case = P.gemm_onehot_case(K)
    got = ops.grouped_gemm(case.x.to(DEV), case.w.to(DEV), case.offs.to(DEV))
    P.check_gemm(case, got)


def test_grouped_gemm_segments():
    case = P.gemm_segment_case()
    got = ops.grouped_gemm(case.x.to(DEV), case.w.to(DEV), case.offs.to(DEV))
    P.check_gemm(case, got)


# -------------------------------------------------- grid-stride second trip

GRID_TRIP = 2048 * 256 * 8  # elements one trip of the capped grid covers


def test_swiglu_second_grid_stride_trip():
    T, I = 300, 14336
    assert GRID_TRIP < T * I < 2 * GRID_TRIP
    g = torch.Generator().manual_seed(5)
    gu = torch.randn(T, 2 * I, generator=g).bfloat16().to(DEV)
    got = ops.swiglu(gu)
    assert got.shape == (T, I)
    P.assert_close(got, R.swiglu(gu), atol=P.TOL_ELEMENTWISE,
                   rtol=P.TOL_ELEMENTWISE, msg="swiglu past one trip")


def test_gelu_second_grid_stride_trip():
    n = GRID_TRIP + 8
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, generator=g) * 3).bfloat16().to(DEV)
    P.assert_close(ops.gelu(x), R.gelu(x), atol=P.TOL_ELEMENTWISE,
                   rtol=P.TOL_ELEMENTWISE, msg="gelu past one trip")


# ------------------------------------- calls the bindings reject, unlaunched

def _bf16(*shape):
    return torch.zeros(*shape, device=DEV, dtype=torch.bfloat16)


@pytest.mark.parametrize("op", P.NORM_OPS)
def test_norms_reject_a_row_larger_than_lds(op):
    """H * 4 bytes of dynamic LDS per row: past the device's limit the call
    is refused with the limit in the message."""
    H = 65536
    args = [_bf16(1, H)] + ([_bf16(1, H)] if op.startswith("fused") else [])
    args += [_bf16(H)] + ([_bf16(H)] if "layernorm" in op else [])
    with pytest.raises(RuntimeError, match="LDS.*limit"):
        getattr(HIP, op)(*args, P.EPS)


@pytest.mark.parametrize("op", P.NORM_OPS)
def test_norms_reject_wrong_weight_length_and_dtype(op):
    H = 64
    lead = [_bf16(2, H)] + ([_bf16(2, H)] if op.startswith("fused") else [])
    n_par = 2 if "layernorm" in op else 1
    for bad in (_bf16(H - 8), _bf16(H + 8), _bf16(H).float()):
        for slot in range(n_par):
            par = [_bf16(H)] * n_par
            par[slot] = bad
            with pytest.raises(RuntimeError):
                getattr(HIP, op)(*lead, *par, P.EPS)


@pytest.mark.parametrize("hd", [256, 160, 15])
def test_attn_prefill_rejects_head_dims_the_basic_kernel_cannot_cover(hd):
    q, k = _bf16(4, 2, hd), _bf16(4, 2, hd)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.attn_prefill(q, k, k.clone(), cu, 4, 1.0, True)


def test_attn_prefill_paged_rejects_head_dim_above_128():
    hd = 256
    q = _bf16(4, 2, hd)
    kc = _bf16(2, 2, 32, hd)
    bt = torch.ones(1, 1, dtype=torch.int32, device=DEV)
    lens = torch.tensor([4], dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.attn_prefill_paged(q, kc, kc.clone(), bt, lens, cu, 4, 1.0)


def test_swiglu_output_is_shaped_like_its_input():
    """[..., 2I] -> [..., I] for any number of leading dimensions."""
    g = torch.Generator().manual_seed(6)
    gu = torch.randn(2, 3, 5, 256, generator=g).bfloat16().to(DEV)
    got = ops.swiglu(gu)
    assert got.shape == (2, 3, 5, 128)
    P.assert_close(got, R.swiglu(gu), atol=P.TOL_ELEMENTWISE,
                   rtol=P.TOL_ELEMENTWISE, msg="swiglu 4-D")
    flat = ops.swiglu(gu.view(30, 256))
    assert torch.equal(got.view(30, 128), flat)
    with pytest.raises(RuntimeError, match="swiglu"):
        ops.swiglu(_bf16(4, 24))  # I = 12 is no multiple of 8
