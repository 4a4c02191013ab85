"""Per-head fp8 KV scales on the GPU: each scaled HIP path vs the torch
reference (ops/reference.py) on the SAME quantized cache, on the shared
outlier input (tests/kv_scales_common.py). Run on an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.ops import reference as R

from tests import kv_scales_common as C

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load
NKV, BS = C.NKV, C.BS


def assert_close(a: torch.Tensor, b: torch.Tensor, atol=3e-2, rtol=3e-2,
                 msg=""):
    a = a.float().cpu()
    b = b.float().cpu()
    assert bool(torch.isfinite(a).all()), f"{msg}: non-finite output"
    diff = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = diff > tol
    assert not bool(bad.any()), (
        f"{msg}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; "
        f"max diff {float(diff.max()):.4f}"
    )


def _scaled_cache(n_blocks, hd, seed):
    """Outlier K/V for every slot of an [n_blocks, NKV, BS, hd] pool, stored
    through the HIP scaled store. Returns (kc, vc, k_scale, v_scale)."""
    g = torch.Generator().manual_seed(seed)
    k, v = C.outlier_kv(n_blocks * BS, hd, g, dtype=torch.bfloat16)
    ks, vs, kis, vis = (t.to(DEV) for t in C.amax_scales(k, v))
    kc = torch.zeros(n_blocks, NKV, BS, hd, dtype=torch.uint8, device=DEV)
    vc = torch.zeros_like(kc)
    slots = torch.arange(n_blocks * BS, dtype=torch.int32, device=DEV)
    ops.kv_cache_store(k.to(DEV), v.to(DEV), kc, vc, slots,
                       k_inv_scale=kis, v_inv_scale=vis)
    return kc, vc, ks, vs


@pytest.mark.parametrize("hd", [128, 64])
def test_scaled_store_bytes(hd):
    """HIP scaled quantize-at-store == reference bytes: outlier input plus
    values beyond 448*scale on both signs, K/V as strided views of a fused
    qkv buffer (as Runner passes them), random slots."""
    g = torch.Generator().manual_seed(31)
    T, nb, nq = 45, 4, 8
    k, v = C.outlier_kv(T, hd, g, dtype=torch.bfloat16)
    ks, vs, kis, vis = C.amax_scales(k, v)  # amax BEFORE the overflow rows
    for t, f in ((3, 3.0), (7, -1.5), (11, 1000.0), (12, -1.02)):
        k[t] = (448.0 * ks * f).view(NKV, 1).to(torch.bfloat16)
        v[t + 20] = (448.0 * vs * f).view(NKV, 1).to(torch.bfloat16)
    qkv = torch.zeros(T, (nq + 2 * NKV) * hd, dtype=torch.bfloat16)
    qkv[:, nq * hd: (nq + NKV) * hd] = k.reshape(T, -1)
    qkv[:, (nq + NKV) * hd:] = v.reshape(T, -1)
    qkv = qkv.to(DEV)
    _q, kk, vv = qkv.split([nq * hd, NKV * hd, NKV * hd], dim=-1)
    kk, vv = kk.view(T, NKV, hd), vv.view(T, NKV, hd)
    assert not kk.is_contiguous()
    slots = torch.randperm(nb * BS, generator=g)[:T].to(torch.int32).to(DEV)
    kis, vis = kis.to(DEV), vis.to(DEV)
    kc = torch.zeros(nb, NKV, BS, hd, dtype=torch.uint8, device=DEV)
    vc = torch.zeros_like(kc)
    kc_ref, vc_ref = kc.clone(), vc.clone()
    ops.kv_cache_store(kk, vv, kc, vc, slots, k_inv_scale=kis,
                       v_inv_scale=vis)
    R.kv_cache_store(kk, vv, kc_ref, vc_ref, slots, k_inv_scale=kis,
                     v_inv_scale=vis)
    assert torch.equal(kc, kc_ref)
    assert torch.equal(vc, vc_ref)
    # the overflow rows saturated to +-448 (0x7e / 0xfe), never NaN (0x7f)
    assert int((kc & 0x7F).max()) == 0x7E and int((vc & 0x7F).max()) == 0x7E
    # unit reciprocal scales on in-range input: today's bytes
    ones = torch.ones(NKV, device=DEV)
    small = (torch.randn(T, NKV, hd, generator=g) * 2).bfloat16().to(DEV)
    a, b = torch.zeros_like(kc), torch.zeros_like(kc)
    a1, b1 = torch.zeros_like(kc), torch.zeros_like(kc)
    ops.kv_cache_store(small, small, a, b, slots)
    ops.kv_cache_store(small, small, a1, b1, slots, k_inv_scale=ones,
                       v_inv_scale=ones)
    assert torch.equal(a, a1) and torch.equal(b, b1)


def _decode_case(B, G, hd, maxlen, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(2, maxlen + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = maxlen
    lens[-1] = 1  # one sequence of length 1
    W = (maxlen + BS - 1) // BS
    bt, nb = C.permuted_block_table(B, W, g)
    kc, vc, ks, vs = _scaled_cache(nb, hd, seed + 100)
    q = C.outlier_q(B, G, hd, g, dtype=torch.bfloat16).to(DEV)
    return q, kc, vc, bt.to(DEV), lens.to(DEV), ks, vs


@pytest.mark.parametrize(
    "B,G,hd,maxlen",
    [
        (3, 4, 128, 500),  # two chunks: PV + combine
        (2, 4, 128, 200),  # W*bs <= 256: one chunk, Z == 1 FOLD path
        (2, 7, 128, 300),  # Qwen group size
        (2, 1, 64, 129),   # hd 64
        (2, 4, 96, 300),   # generic (non-MFMA) scores kernel
    ],
)
def test_scaled_attn_decode(B, G, hd, maxlen):
    q, kc, vc, bt, lens, ks, vs = _decode_case(B, G, hd, maxlen, seed=41)
    if maxlen == 200:
        assert bt.shape[1] * BS <= 256
    scale = hd**-0.5
    got = ops.attn_decode(q, kc, vc, bt, lens, scale, k_scale=ks, v_scale=vs)
    ref = R.attn_decode(q, kc, vc, bt, lens, scale, k_scale=ks, v_scale=vs)
    assert_close(C.div_by_v_std(got, G), C.div_by_v_std(ref, G),
                 msg=f"scaled fp8 decode G{G} hd{hd} L{maxlen}")
    # all-ones scales take the scaled kernels and must change nothing. The
    # scaled MFMA scores kernel lifts a q whose amax (after the softmax
    # scale) is below 2^-5 out of e4m3's subnormals, which the unscaled
    # path does not do, so the identity is checked with a q of unit
    # magnitude in every head (0.3 * randn, not divided by the K std).
    ones = torch.ones(NKV, device=DEV)
    g = torch.Generator().manual_seed(43)
    q1 = (0.3 * torch.randn(q.shape, generator=g)).bfloat16().to(DEV)
    amax = (q1.float() * scale).reshape(B, NKV, -1).abs().amax(-1)
    assert float(amax.min()) >= 2.0**-5
    plain = ops.attn_decode(q1, kc, vc, bt, lens, scale)
    unit = ops.attn_decode(q1, kc, vc, bt, lens, scale, k_scale=ones,
                           v_scale=ones)
    assert torch.equal(plain, unit)


def test_scales_rejected_for_bf16_cache():
    hd = 64
    kc = torch.zeros(2, NKV, BS, hd, dtype=torch.bfloat16, device=DEV)
    q = torch.zeros(1, NKV, hd, dtype=torch.bfloat16, device=DEV)
    bt = torch.ones(1, 1, dtype=torch.int32, device=DEV)
    lens = torch.ones(1, dtype=torch.int32, device=DEV)
    ones = torch.ones(NKV, device=DEV)
    with pytest.raises(RuntimeError, match="fp8"):
        ops.attn_decode(q, kc, kc, bt, lens, 1.0, k_scale=ones, v_scale=ones)
    k = torch.zeros(1, NKV, hd, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="fp8"):
        ops.kv_cache_store(k, k, kc, kc.clone(), lens, k_inv_scale=ones,
                           v_inv_scale=ones)


@pytest.mark.parametrize(
    "B,G,hd,maxlen",
    [
        (8, 4, 128, 256),   # W*bs <= 256: Z == 1 FOLD path writes out_ml
        (2, 4, 128, 2048),  # Z > 1: PV + combine
    ],
)
def test_scaled_attn_decode_lse(B, G, hd, maxlen):
    """(m, l) of the scaled cache match the reference, shard + merge equals
    the unsharded scaled result, and an L == 0 row still yields zeros and
    (-1e30, 0)."""
    from bee2bee_amd.parallel.cp import merge_partials

    g = torch.Generator().manual_seed(51)
    lens = torch.randint(64, maxlen + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = maxlen
    W = (maxlen + BS - 1) // BS
    # the pool is smaller than B * W: sequences share pages (reads only)
    nb = 2 * W + 1
    bt = (torch.randint(1, nb, (B, W), generator=g)).to(torch.int32)
    kc, vc, ks, vs = _scaled_cache(nb, hd, 151)
    q = C.outlier_q(B, G, hd, g, dtype=torch.bfloat16).to(DEV)
    scale = hd**-0.5
    bt_d, lens_d = bt.to(DEV), lens.to(DEV)
    kw = dict(k_scale=ks, v_scale=vs)

    full = ops.attn_decode(q, kc, vc, bt_d, lens_d, scale, **kw)
    out1, ml1 = ops.attn_decode_lse(q, kc, vc, bt_d, lens_d, scale, **kw)
    assert torch.equal(out1, full)
    _r_out, r_ml = R.attn_decode_lse(q, kc, vc, bt_d, lens_d, scale, **kw)
    assert_close(ml1[..., 0], r_ml[..., 0], msg="m")
    assert_close(torch.log(ml1[..., 1]), torch.log(r_ml[..., 1]),
                 msg="log l")

    # two-way page shard + merge == full context (construction of
    # test_ops_gpu.py::test_attn_decode_lse_merge); the last sequence is
    # short enough that the second shard owns nothing of it (L == 0)
    lens2 = lens.clone()
    lens2[-1] = BS - 3
    lens2_d = lens2.to(DEV)
    full2 = ops.attn_decode(q, kc, vc, bt_d, lens2_d, scale, **kw)
    outs, mls = [], []
    for r in range(2):
        llens = torch.zeros_like(lens2)
        lbt = torch.zeros_like(bt)
        for i, L in enumerate(lens2.tolist()):
            n_pages = -(-L // BS)
            lo = (n_pages // 2 + n_pages % 2) * r
            hi = n_pages // 2 + n_pages % 2 if r == 0 else n_pages
            tok_lo, tok_hi = lo * BS, min(hi * BS, L)
            llens[i] = max(0, tok_hi - tok_lo)
            lbt[i, : hi - lo] = bt[i, lo:hi]
        o, ml = ops.attn_decode_lse(q, kc, vc, lbt.to(DEV), llens.to(DEV),
                                    scale, **kw)
        if r == 1:
            assert int(llens[-1]) == 0
            _ro, rml = R.attn_decode_lse(q, kc, vc, lbt.to(DEV),
                                         llens.to(DEV), scale, **kw)
            assert bool((_ro[-1] == 0).all())
            assert bool((rml[-1, :, 0] == -1e30).all())
            assert bool((rml[-1, :, 1] == 0).all())
        ml = ml.clone()
        ml[llens.to(DEV) == 0, :, 0] = -1e30
        ml[llens.to(DEV) == 0, :, 1] = 0.0
        outs.append(o)
        mls.append(ml)
    merged = merge_partials(outs, mls)
    assert_close(C.div_by_v_std(merged, G), C.div_by_v_std(full2, G),
                 msg=f"scaled cp merge B{B} G{G} hd{hd}")


@pytest.mark.parametrize("hd", [128, 64])
def test_scaled_attn_prefill_paged(hd):
    g = torch.Generator().manual_seed(61)
    nq, G = 16, 4
    hist_q = [(200, 70), (0, 64)]
    B = len(hist_q)
    seq_lens = [h + ql for h, ql in hist_q]
    W = (max(seq_lens) + BS - 1) // BS
    bt, nb = C.permuted_block_table(B, W, g)
    kc, vc, ks, vs = _scaled_cache(nb, hd, 161)
    T = sum(ql for _, ql in hist_q)
    q = C.outlier_q(T, G, hd, g, dtype=torch.bfloat16).to(DEV)
    assert q.shape[1] == nq
    cu_list = [0]
    for _, ql in hist_q:
        cu_list.append(cu_list[-1] + ql)
    cu = torch.tensor(cu_list, dtype=torch.int32, device=DEV)
    lens_dev = torch.tensor(seq_lens, dtype=torch.int32, device=DEV)
    qlens = torch.tensor([ql for _, ql in hist_q], dtype=torch.int32,
                         device=DEV)
    scale = hd**-0.5
    bt = bt.to(DEV)
    got = ops.attn_prefill_paged(q, kc, vc, bt, lens_dev, cu,
                                 max(ql for _, ql in hist_q), scale,
                                 k_scale=ks, v_scale=vs)
    ref = R.attn_decode_with_history(q, kc, vc, bt, lens_dev, qlens, scale,
                                     k_scale=ks, v_scale=vs)
    assert_close(C.div_by_v_std(got, G), C.div_by_v_std(ref, G),
                 msg=f"scaled fp8 prefill_paged hd{hd}")


def test_engine_calibrated_graph_matches_eager():
    """"tiny" with fp8 KV: calibrate, then greedy-generate through chunked
    prefill + decode. Captured-graph and eager decode must emit the same
    tokens — the graph reads the scale tensors the calibration filled."""
    from bee2bee_amd.engine.engine import InferenceEngine

    prompt = [(i * 7 + 3) % 500 + 4 for i in range(40)]
    outs = {}
    for graphs in (True, False):
        eng = InferenceEngine("tiny", device=DEV, max_batch=2,
                              max_seq_len=128, seed=7, kv_dtype="fp8",
                              max_prefill_tokens=16, use_graphs=graphs)
        try:
            assert (eng.graphs is not None) == graphs
            eng.calibrate_kv_scales([prompt, prompt[::-1]])
            assert eng.stats()["kv_scales"] == "calibrated"
            assert bool((eng.kv.k_scale != 1.0).all())
            req = eng.generate(prompt, max_new_tokens=12, temperature=0.0,
                               repetition_penalty=1.0)
            assert len(req.output_ids) == 12
            outs[graphs] = (req.output_ids, eng.kv.k_scale.clone(),
                            eng.kv.v_scale.clone())
            for cache in eng.kv.k_cache + eng.kv.v_cache:
                # no e4m3 NaN byte (0x7f / 0xff) was ever stored
                assert int(((cache & 0x7F) == 0x7F).sum()) == 0
        finally:
            eng.shutdown()
    assert torch.equal(outs[True][1], outs[False][1])
    assert torch.equal(outs[True][2], outs[False][2])
    assert outs[True][0] == outs[False][0], (outs[True][0], outs[False][0])
