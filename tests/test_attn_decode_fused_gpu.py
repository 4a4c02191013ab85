"""Fused scores + PV decode kernel (attn_decode_fused_kernel) on the GPU.

Every case checks three things:
  * fused == split, bit for bit, on `out` and on `(m, l)` (torch.equal);
  * fused against ops/reference.py at test_ops_gpu.py's assert_close
    defaults (2e-2 / 2e-2);
  * `(m, l)` against the reference at test_attn_decode_lse_merge's bounds.
`max_z=1` forces one block per (seq, kv head), i.e. the multi-chunk FOLD
kernels that no small shape reaches on its own; `max_z=0` leaves the
launcher's rule (Z = C at these batch sizes: part_o / part_ml + combine).

Caches: permuted block table, page 0 unused (finite, never mapped). The
window cases use the layout of tests/test_sliding_window_gpu.py: table
entries wholly below the band or past L point at an all-NaN page, and in the
page that straddles the band's lower edge the rows below it carry K * 50.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # allow collection on CPU boxes
    pytest.skip("requires MI355X", allow_module_level=True)

from bee2bee_amd import ops
from bee2bee_amd.ops import reference as R

DEV = "cuda:0"
HIP = ops.require_hip()  # loud failure if the extension didn't load
NKV = 2
E4M3_NAN = 0x7F


def assert_close(a, b, atol=2e-2, rtol=2e-2, msg=""):
    a = a.float().cpu()
    b = b.float().cpu()
    assert bool(torch.isfinite(b).all()), f"{msg}: reference is not finite"
    assert bool(torch.isfinite(a).all()), f"{msg}: non-finite output"
    diff = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = diff > tol
    assert not bool(bad.any()), (
        f"{msg}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; "
        f"max diff {float(diff.max()):.4f}"
    )


def assert_ml_close(ml, r_ml, msg=""):
    """The (m, l) bounds of test_ops_gpu.py::test_attn_decode_lse_merge."""
    assert bool(torch.isfinite(ml).all()), msg
    assert torch.allclose(ml[..., 0], r_ml[..., 0], atol=0.25, rtol=0.02), \
        (msg, (ml[..., 0] - r_ml[..., 0]).abs().max())
    assert torch.allclose(ml[..., 1] / r_ml[..., 1].clamp_min(1e-6),
                          torch.ones_like(r_ml[..., 1]), atol=0.1), \
        f"{msg}: sum-exp mismatch"


def make_case(lens, G, hd, bs, fp8=False, scaled=False, window=0, seed=0):
    """(q, kc, vc, bt, lens, kwargs) for sequences of lengths `lens`."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    W = (max(max(lens), 1) + bs - 1) // bs + 1  # one spare column past L
    poison = 1 if window else None
    first_live = 2 + (bs if window else 0)
    nb = first_live + B * W
    ksrc = torch.randn(nb, NKV, bs, hd, generator=g)
    vsrc = torch.randn(nb, NKV, bs, hd, generator=g)
    qsrc = torch.randn(B, NKV * G, hd, generator=g)
    if fp8:
        ksrc *= 0.7
        vsrc *= 0.7
        qsrc *= 0.2
    if scaled:
        # kv head 0: K runs large and its q correspondingly small, so the
        # staged q has amax < 2^-5 and takes the power-of-two lift
        ksrc[:, 0] *= 40.0 / 0.7
        qsrc[:, :G] /= 40.0
    if window:
        for r in range(1, bs):  # straddling page for lo % bs == r
            ksrc[2 + r, :, :r] *= 50.0
    live = torch.randperm(B * W, generator=g) + first_live
    bt = torch.zeros(B, W, dtype=torch.int32)
    for b, L in enumerate(lens):
        lo = max(0, L - window) if window else 0
        for p in range(W):
            if window and ((p + 1) * bs <= lo or p * bs >= L):
                bt[b, p] = poison
            elif window and p * bs < lo:
                bt[b, p] = 2 + lo % bs
            else:
                bt[b, p] = int(live[b * W + p])
    kw = {}
    if not fp8:
        kc = ksrc.to(DEV).bfloat16()
        vc = vsrc.to(DEV).bfloat16()
        if window:
            kc[poison] = float("nan")
            vc[poison] = float("nan")
    else:
        kc = torch.zeros(nb, NKV, bs, hd, dtype=torch.uint8, device=DEV)
        vc = torch.zeros_like(kc)
        kf = ksrc.permute(0, 2, 1, 3).reshape(nb * bs, NKV, hd)
        vf = vsrc.permute(0, 2, 1, 3).reshape(nb * bs, NKV, hd)
        slots = torch.arange(nb * bs, dtype=torch.int32, device=DEV)
        skw = {}
        if scaled:
            ks = (kf.abs().amax(dim=(0, 2)) / 448.0).to(DEV)
            vs = (vf.abs().amax(dim=(0, 2)) / 448.0).to(DEV)
            assert float(ks.min()) < 0.02  # the small k_scale
            kw = {"k_scale": ks, "v_scale": vs}
            skw = {"k_inv_scale": 1.0 / ks, "v_inv_scale": 1.0 / vs}
        ops.kv_cache_store(kf.to(DEV).bfloat16(), vf.to(DEV).bfloat16(),
                           kc, vc, slots, **skw)
        if window:
            kc[poison] = E4M3_NAN
            vc[poison] = E4M3_NAN
    if window:
        kw["window"] = window
    q = qsrc.to(DEV).bfloat16()
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    return q, kc, vc, bt.to(DEV), lens_t, kw


def check(lens, G=4, hd=128, bs=32, max_z=1, **case_kw):
    q, kc, vc, bt, lens_t, kw = make_case(lens, G, hd, bs, **case_kw)
    scale = hd ** -0.5
    msg = f"lens={lens} G{G} hd{hd} bs{bs} max_z={max_z} {case_kw}"
    f_out, f_ml = ops.attn_decode_select(q, kc, vc, bt, lens_t, scale,
                                         path="fused", max_z=max_z, **kw)
    s_out, s_ml = ops.attn_decode_select(q, kc, vc, bt, lens_t, scale,
                                         path="split", max_z=max_z, **kw)
    r_out, r_ml = R.attn_decode_lse(q, kc, vc, bt, lens_t, scale, **kw)
    assert torch.equal(f_out, s_out), (
        f"{msg}: fused out != split out, "
        f"{int((f_out != s_out).sum())}/{f_out.numel()} differ")
    assert torch.equal(f_ml, s_ml), f"{msg}: fused (m, l) != split (m, l)"
    assert_close(f_out, r_out, msg=msg)
    assert_ml_close(f_ml, r_ml, msg=msg)
    return q, f_out, f_ml


def test_scaled_case_takes_the_q_lift():
    """The input the scaled case relies on: kv head 0's staged q is below
    2^-5 (lifted), kv head 1's is not."""
    q, *_ = make_case([600, 257], 4, 128, 32, fp8=True, scaled=True)
    amax = (q.float() * 128 ** -0.5).reshape(2, NKV, -1).abs().amax(-1)
    assert float(amax[:, 0].max()) < 2.0 ** -5 <= float(amax[:, 1].min())


@pytest.mark.parametrize("lens", [
    [600, 257],  # FOLD over 3 chunks, partial last chunk, 1-key chunk
    [256, 1],    # exactly one full chunk; L = 1
])
def test_fold_multi_chunk(lens):
    check(lens)


@pytest.mark.parametrize("G,hd", [(1, 128), (2, 128), (7, 128), (8, 128),
                                  (16, 128), (4, 64)])
def test_fold_group_sizes(G, hd):
    check([600, 257], G=G, hd=hd)


def test_fold_flagship_page_layout():
    check([1025, 256], bs=256)  # one key in the fifth chunk


def test_partials_and_combine():
    check([900, 300], max_z=0)  # Z = C: fused + combine vs split + combine


@pytest.mark.parametrize("max_z", [1, 0])
def test_fp8_unscaled(max_z):
    check([600, 257], fp8=True, max_z=max_z)


@pytest.mark.parametrize("max_z", [1, 0])
def test_fp8_scaled_q_lift(max_z):
    check([600, 257], fp8=True, scaled=True, max_z=max_z)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("max_z", [1, 0])
@pytest.mark.parametrize("window", [256, 300])
def test_window(window, max_z, fp8):
    # lens 700 / w256: lo = 444 inside a chunk; lens 300 / w300: lo = 0;
    # lens 700 / w300: lo = 400; lens 300 / w256: lo = 44. The chunk-edge
    # lo is lens 512 + w256 below.
    check([700, 300], window=window, max_z=max_z, fp8=fp8)


@pytest.mark.parametrize("fp8", [False, True])
def test_window_lo_on_chunk_edge(fp8):
    check([768, 512], window=256, fp8=fp8)  # lo = 512 and 256


def test_empty_row():
    """L == 0 (an empty context-parallel shard): zeros and (-1e30, 0), and
    the other row is what a run without the empty row gives."""
    lens, G, hd, bs = [0, 300], 4, 128, 32
    q, kc, vc, bt, lens_t, kw = make_case(lens, G, hd, bs)
    scale = hd ** -0.5
    out, ml = ops.attn_decode_select(q, kc, vc, bt, lens_t, scale,
                                     path="fused", max_z=1)
    r_out, r_ml = R.attn_decode_lse(q, kc, vc, bt, lens_t, scale)
    assert torch.equal(out[0], torch.zeros_like(out[0]))
    assert torch.equal(ml[0, :, 0], torch.full_like(ml[0, :, 0], -1e30))
    assert torch.equal(ml[0, :, 1], torch.zeros_like(ml[0, :, 1]))
    assert torch.equal(out[0], r_out[0].to(out.dtype))
    assert torch.equal(ml[0], r_ml[0].to(ml.dtype))
    for path in ("fused", "split"):
        o1, ml1 = ops.attn_decode_select(q[1:], kc, vc, bt[1:], lens_t[1:],
                                         scale, path=path, max_z=1)
        assert torch.equal(out[1:], o1), path
        assert torch.equal(ml[1:], ml1), path
    assert_close(out, r_out, msg="empty row")
    assert_ml_close(ml[1:], r_ml[1:], msg="empty row")


def test_fused_rejects_unsupported_head_dim():
    q, kc, vc, bt, lens_t, _ = make_case([70, 33], 2, 16, 32)
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.attn_decode_select(q, kc, vc, bt, lens_t, 0.25, path="fused")
    # the other paths serve it
    out, _ml = ops.attn_decode_select(q, kc, vc, bt, lens_t, 0.25,
                                      path="auto")
    assert_close(out, R.attn_decode(q, kc, vc, bt, lens_t, 0.25))
